"""covgpu_relpose_batch (covins_amd/csrc/k_relpose.hip) against the CPU oracle (oracle/covo_relpose.cpp) off the Gauss-Newton path and at the
edges of its sizes: the regimes of tests/relpose_util.py, which tests/test_relpose_host.py proves to reach rejected steps, the reuse of the
linearisation, both radius halvings, radius-limited steps, the empty-system exit and the min_inliers gate from both sides. A stale alpha,
gh or gn after a rejection, or a radius updated on the wrong branch, changes T_AB of `mid`, `far` and `wide` far beyond their tolerances.

Per regime one launch, and the oracle pair by pair (computed once per session, relpose_util.reference). Compared on the pairs that
relpose_util.selected keeps: inlier counts and outlier flags exactly, T_AB within relpose_util.TOL (measured on the oracle, see there)."""
import numpy as np
import pytest

from covins_amd import backend
from oracle import covo
from tests import relpose_util as ru

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = backend.Context(0)
    yield c
    c.close()


def _compare(name, bt, ref, sel, T, out, inl):
    """Pairs of `sel`: counts and flags as the oracle's, T within the regime's tolerance; a pair that returns 0 keeps its input bytes."""
    worst = 0.0
    for b in np.flatnonzero(sel):
        r, s = ref[b], slice(bt["ptr"][b], bt["ptr"][b + 1])
        assert inl[b] == r["n"] and np.array_equal(out[s], r["out"]), (b, inl[b], r["n"])
        if r["n"] == 0 and ru.min_inliers_of(name) > 0:
            assert T[b].tobytes() == bt["T0"][b].tobytes(), b
        d = np.abs(T[b] - r["T"]).max()
        assert d <= ru.TOL[name], (b, d)
        worst = max(worst, d)
    print(f"{name}: {int(sel.sum())} pairs, max |dT| {worst:.2e} (tolerance {ru.TOL[name]:.1e})")


@pytest.mark.parametrize("th", ru.TH)
@pytest.mark.parametrize("dist_type", [0, 1])
@pytest.mark.parametrize("name", ["near", "mid", "far", "wide", "stride", "unnormalised"])
def test_regime_follows_the_oracle(ctx, name, dist_type, th):
    bt = ru.regime(name, dist_type)
    T, out, inl = ctx.relpose_batch(bt, th_outlier=th, min_inliers=ru.MIN_INLIERS)
    _compare(name, bt, ru.reference(name, dist_type, th), ru.selected(name, dist_type, th), T, out, inl)


@pytest.mark.parametrize("th", ru.TH)
@pytest.mark.parametrize("dist_type", [0, 1])
def test_few_correspondences_follow_the_oracle(ctx, dist_type, th):
    """0 to 4 correspondences, empty pairs between the others, min_inliers = 0. One or two correspondences leave the pose rank-deficient up
    to the 1e-8 damping: there the objective at the two returned poses is compared, not the poses."""
    bt = ru.regime("few", dist_type)
    ref, sel = ru.reference("few", dist_type, th), ru.selected("few", dist_type, th)
    T, out, inl = ctx.relpose_batch(bt, th_outlier=th, min_inliers=0)
    assert np.isfinite(T).all()
    n = np.diff(bt["ptr"])
    _compare("few", bt, ref, sel & ((n == 0) | (n >= 3)), T, out, inl)
    for b in np.flatnonzero(sel & (n > 0) & (n < 3)):
        r, s = ref[b], slice(bt["ptr"][b], bt["ptr"][b + 1])
        assert inl[b] == r["n"] and np.array_equal(out[s], r["out"]), b
        c_dev, c_ref = (covo.relpose_cost(X, *ru.pair_args(bt, b), outlier=r["out"]) for X in (T[b], r["T"]))
        assert abs(c_dev - c_ref) <= ru.FEW_COST_TOL, (b, c_dev, c_ref)
    assert (inl[n == 0] == 0).all()
    # a batch of empty pairs only: no correspondence array holds anything
    e = ru.subbatch(bt, list(np.flatnonzero(n == 0)[:2]))
    Te, oute, inle = ctx.relpose_batch(e, th_outlier=th, min_inliers=0)
    assert len(oute) == 0 and (inle == 0).all() and np.abs(Te - e["T0"]).max() <= 4.5e-16


@pytest.mark.parametrize("dist_type", [0, 1])
def test_gate_on_both_sides_of_min_inliers(ctx, dist_type):
    """Exactly min_inliers survivors: the second solve runs and the count is returned. One fewer: 0, T_AB's bytes untouched, the flags of
    the outlier pass written all the same."""
    bt, cases = ru.gate_cases(dist_type)
    for b, th_in, th_out in cases:
        s = slice(bt["ptr"][b], bt["ptr"][b + 1])
        for th, survivors in ((th_in, ru.MIN_INLIERS), (th_out, ru.MIN_INLIERS - 1)):
            n0, T0, o0 = covo.relpose(*ru.pair_args(bt, b), bt["T0"][b], th_outlier=th, min_inliers=ru.MIN_INLIERS)
            T, out, inl = ctx.relpose_batch(bt, th_outlier=th, min_inliers=ru.MIN_INLIERS)
            assert (~out[s]).sum() == survivors and np.array_equal(out[s], o0), (b, th)
            assert inl[b] == n0 == (survivors if survivors == ru.MIN_INLIERS else 0)
            if survivors == ru.MIN_INLIERS:
                assert np.abs(T[b] - T0).max() <= ru.TOL["gate"], (b, np.abs(T[b] - T0).max())
            else:
                assert T[b].tobytes() == bt["T0"][b].tobytes() and out[s].any()


@pytest.mark.parametrize("dist_type", [0, 1])
def test_unnormalised_input_bytes_survive_a_refused_pair(ctx, dist_type):
    bt = ru.regime("unnormalised", dist_type)
    T, out, inl = ctx.relpose_batch(bt, th_outlier=0.9, min_inliers=ru.MIN_INLIERS)
    zero = np.flatnonzero(inl == 0)
    assert {ru.UNNORMALISED_SCALE[b % 4] for b in zero} == set(ru.UNNORMALISED_SCALE)
    assert T[zero].tobytes() == bt["T0"][zero].tobytes()
    done = np.flatnonzero(inl > 0)
    assert np.abs(np.linalg.norm(T[done, :4], axis=1) - 1).max() <= 1e-15


@pytest.mark.parametrize("name", ["mid", "stride"])
def test_a_pair_alone_equals_the_pair_inside_its_batch(ctx, name):
    """Bit for bit: a wavefront's sums do not depend on where its pair lies in the batch."""
    bt = ru.regime(name, 0)
    num = len(bt["ptr"]) - 1
    T, out, inl = ctx.relpose_batch(bt, th_outlier=0.9, min_inliers=ru.MIN_INLIERS)
    for b in (0, num // 2, num - 1):
        T1, out1, inl1 = ctx.relpose_batch(ru.subbatch(bt, [b]), th_outlier=0.9, min_inliers=ru.MIN_INLIERS)
        assert inl1[0] == inl[b] and np.array_equal(out1, out[bt["ptr"][b]:bt["ptr"][b + 1]]) and T1[0].tobytes() == T[b].tobytes(), b


@pytest.mark.parametrize("dist_type", [0, 1])
def test_unified_instantiation_off_the_gauss_newton_path(ctx, dist_type):
    """k_relpose<true> (both sides COVGPU_CAM_UNIFIED, xi = 0: the pinhole projection through the unified code) on `mid`."""
    bt = ru.regime("mid", dist_type)
    num = len(bt["ptr"]) - 1
    bu = dict(bt, modelA=np.ones(num, np.int32), modelB=np.ones(num, np.int32), xiA=np.zeros(num), xiB=np.zeros(num))
    for th in ru.TH:
        T0, o0, n0 = ctx.relpose_batch(bt, th_outlier=th, min_inliers=ru.MIN_INLIERS)
        T1, o1, n1 = ctx.relpose_batch(bu, th_outlier=th, min_inliers=ru.MIN_INLIERS)
        _compare("mid", bt, ru.reference("mid", dist_type, th), ru.selected("mid", dist_type, th), T1, o1, n1)
        for b in np.flatnonzero(ru.selected("mid", dist_type, th)):
            s = slice(bt["ptr"][b], bt["ptr"][b + 1])
            assert n0[b] == n1[b] and np.array_equal(o0[s], o1[s]) and np.abs(T0[b] - T1[b]).max() <= ru.TOL["mid"], b
