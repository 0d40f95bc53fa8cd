"""k_preintegrate and the whitened factor on the device at 1 .. 150 samples per factor — the points of tests/imu_lengths_util.py (one factor per count;
the counts shuffled over the waves, with a partly dead last workgroup), whose conditions tests/test_imu_lengths_host.py asserts on the oracle. Every
wave of k_preintegrate runs its own sample count without a workgroup barrier, keeps the next sample in flight while it works on this one, and closes
with a factorisation spread over its lanes: a count under, at and over every power of two up to 128 stands beside very short and very long factors.

The device is held by the rule of tests/test_gpu_imu.py (_hold): device - restatement <= 10 x max(oracle's distance, floor) per factor and quantity,
and by the per-factor parity bounds of that module. The one-sample factor is weightless: exact zeros, counted once in covgpu_result::reserved.
"""
import time

import numpy as np
import pytest

from covins_amd import backend
from tests import imu_lengths_util as lu
from tests import imu_util as iu
from tests.test_gpu_imu import PARITY_FACTOR, PARITY_PRE, _hold, _opts

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    t0 = time.perf_counter()
    c = backend.Context(0)
    yield c
    c.close()
    print(f"\ntests/test_gpu_imu_lengths.py: {time.perf_counter() - t0:.1f} s")


@pytest.mark.parametrize("pid", lu.IDS)
def test_preintegration(ctx, pid):
    p, h = lu.build(pid), iu.host_reference(pid)
    g, _ = _opts()
    d, J, P = ctx.preintegrate(p, g)
    dist = iu.distances(h["ref"], pre=(d, J, P))
    for k, bound in PARITY_PRE.items():
        assert dist[k].max() < bound, (k, dist[k].max())
    _hold(pid, dist, iu.PRE_QUANTITIES)


@pytest.mark.parametrize("pid", lu.IDS)
def test_factor(ctx, pid):
    p, h = lu.build(pid), iu.host_reference(pid)
    ref = h["ref"]
    g, _ = _opts()
    r, J = ctx.linearize_imu(p, g)
    dist = iu.distances(ref, lin=(r, J))
    assert dist["r"].max() < PARITY_FACTOR and dist["Jw"].max() < PARITY_FACTOR
    _hold(pid, dist, iu.WHITE_QUANTITIES)
    w = ref["n"] < 2
    assert w.sum() == 1
    assert not r[w].any() and not J[w].any()                             # the one-sample factor: exact zeros
    assert np.all(np.abs(J[~w]).max(axis=1) > 0)                          # every other factor carries weight


@pytest.mark.parametrize("pid", lu.IDS)
def test_one_sample_factor_is_counted_once(ctx, pid):
    g, _ = _opts(max_iterations=1)
    _, res = ctx.gba_solve(lu.build(pid), g)
    assert res.reserved == 1
