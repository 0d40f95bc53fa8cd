"""The whole-record transport of the landmark Schur pass (k_visual.hip: the cooperative gathers of k_pair_blocks, the tile stores of k_lm_lin) on the
points of tests/record_lines_util.py (their properties are asserted on the CPU by tests/test_record_lines_host.py): pairs of 1 .. 72 common
landmarks, a pair that owns the first and the last record of the array, the same pairs renumbered at random, and track-length cycles for the three
widths of k_lm_lin with a last workgroup of one landmark. Per point:
  - S, b and the cost of Context.schur at mu = 1e-8 and 1e-2 against the oracle, normalised and bounded as tests/test_gpu_structure.py does
    (_check_schur: 1e-9, 1e-9, 1e-12), and the step of Context.gn_step at mu = 1e-4 within C_BOUND x max(spread of the oracle's two solvers, H_FLOOR)
  - common-scattered additionally against the device's own result on the original numbering
  - the BYTES of S, b, the cost and the step against tests/golden/record_lines_parent.npz: what the commit before the transport changed computed
    on an MI355X (tools/make_record_lines_golden.py; the file names that commit). The transport changes how a record travels, not which terms a lane
    adds in which order: every bit is the parent's.
"""
import os

import numpy as np
import pytest

from covins_amd import backend
from tests import record_lines_util as ru
from tests import structure_util as su
from tests.test_gpu_forms import C_BOUND, H_FLOOR
from tests.test_gpu_lm_forms import _check_schur

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = backend.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", ru.GOLDEN)) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("pt", ru.POINTS, ids=ru.IDS)
def test_schur_complement(ctx, pt):
    p = ru.build(pt).p
    ref = ru.host_reference(pt)
    g = backend.default_options(visual_only=1)
    for mu in ru.MUS_SCHUR:
        S, b, c = ctx.schur(p, g, mu)
        S0, b0, c0 = ref["schur"][mu]
        scale = np.sqrt(np.abs(np.diag(S0)))
        print(f"{pt.id} mu={mu:g}: K={p.K} L={p.L} O={p.O}  S {np.abs((S - S0) / scale[:, None] / scale[None, :]).max():.2e}  "
              f"b {np.abs((b - b0) / scale).max() / np.abs(b0 / scale).max():.2e}  cost {abs(c - c0) / c0:.2e}  (bounds 1e-9, 1e-9, 1e-12)")
        _check_schur(S, b, c, S0, b0, c0)


@pytest.mark.parametrize("pt", ru.POINTS, ids=ru.IDS)
def test_gauss_newton_step(ctx, pt):
    p = ru.build(pt).p
    ref = ru.host_reference(pt)
    dx, dl, cost = ctx.gn_step(p, backend.default_options(visual_only=1), ru.MU_STEP)
    e_pose, e_lm = ru.scaled_err(dx, ref["x0"], ref["d"]), ru.rel(dl, ref["l0"])
    hp, hl = max(ref["h_pose"], H_FLOOR), max(ref["h_lm"], H_FLOOR)
    print(f"{pt.id}: spread h_pose={ref['h_pose']:.2e} h_lm={ref['h_lm']:.2e} ({ref['whole']}) | device pose {e_pose:.2e} (bound {C_BOUND * hp:.1e}, {e_pose / hp:.2f} h)  "
          f"landmarks {e_lm:.2e} (bound {C_BOUND * hl:.1e}, {e_lm / hl:.2f} h)")
    c0 = ref["schur"][ru.MU_STEP][2]
    assert abs(cost - c0) <= 1e-12 * c0
    assert e_pose <= C_BOUND * hp, (e_pose, ref["h_pose"])
    assert e_lm <= C_BOUND * hl, (e_lm, ref["h_lm"])


def test_scattered_problem_gives_the_device_the_same_answer(ctx):
    """As tests/test_gpu_structure.py::test_relabelled_problem_gives_the_device_the_same_answer: the device on common-scattered, mapped back, against the
    device on common-1..72 (summation order of S, b; elimination order of the step)."""
    pt = ru.BY_ID["common-scattered"]
    b = ru.build(pt)
    ref = ru.host_reference(pt)
    g = backend.default_options(visual_only=1)
    r = su.rows_of(b.maps.kf, 6)
    for mu in ru.MUS_SCHUR:
        S0, b0, c0 = ctx.schur(b.orig, g, mu)
        S1, b1, c1 = ctx.schur(b.p, g, mu)
        eS, eb = _check_schur(S1[np.ix_(r, r)], b1[r], c1, S0, b0, c0)
        print(f"{pt.id} mu={mu:g}: device relabelled against device original: S {eS:.2e}  b {eb:.2e}")
    dx0, dl0, _ = ctx.gn_step(b.orig, g, ru.MU_STEP)
    dx1, dl1, _ = ctx.gn_step(b.p, g, ru.MU_STEP)
    d = ref["d"][r]
    e_pose, e_lm = ru.scaled_err(dx1[r], dx0, d), ru.rel(dl1[b.maps.lm], dl0)
    hp, hl = max(ref["h_pose"], H_FLOOR), max(ref["h_lm"], H_FLOOR)
    print(f"{pt.id}: step relabelled against original: pose {e_pose:.2e} ({e_pose / hp:.2f} h)  landmarks {e_lm:.2e} ({e_lm / hl:.2f} h)")
    assert e_pose <= C_BOUND * hp and e_lm <= C_BOUND * hl


@pytest.mark.parametrize("pt", ru.POINTS, ids=ru.IDS)
def test_bytes_are_the_parent_commits(ctx, golden, pt):
    got = ru.device_record(ctx, pt)
    want = {k: v for k, v in golden.items() if k.startswith(pt.id + "/")}
    assert set(got) == set(want)
    diff = []
    for k in sorted(got):
        same = got[k].shape == want[k].shape and got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes()
        if not same:
            n = int((got[k] != want[k]).sum()) if got[k].shape == want[k].shape else -1
            diff.append((k, n))
    print(f"{pt.id}: {len(got)} arrays against the parent commit {golden['parent_commit']}: {'all bytes equal' if not diff else diff}")
    assert not diff, diff
