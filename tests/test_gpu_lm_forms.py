"""The 4-, 8- and 16-lane forms of the landmark-major kernels (k_visual.hip: k_lm_lin, k_lm_backsub, k_lm_outliers as G lanes per landmark, each as a
pinhole and a unified instantiation) against host references, at the edges of every width.

Which width runs is decided by the data alone (covgpu_lm_group: mean track length O/L <= 5 -> 4 lanes, <= 8 -> 8, else 16), and every small map of
the suite lands on 16. The points of tests/lm_forms_util.py are problems cut to prescribed track lengths: per width, tracks of 2, G - 1, G, G + 1, 2 G,
2 G + 1 and of 4 or 5 chunks (the second loop of k_lm_lin re-evaluates a multi-chunk landmark's Jacobians), landmark counts of one workgroup
(256 / G groups) and one more and one less, one point of several workgroups with three degenerate landmarks, and a single landmark at G = 4.
tests/test_lm_forms_host.py asserts on the CPU that every point selects the width it is meant for and holds those tracks.

Per point and camera base (26 in all):
  - S, b and the cost of covgpu_schur (k_lm_lin, k_kf_reduce, k_pair_blocks) at mu = 1e-8 and 1e-2 against the oracle (pinhole) or the numpy Schur
    complement of the restated linearisation (unified), in the normalisation and to the bounds of test_schur_complement;
  - the step of covgpu_gn_step (k_lm_backsub for its landmark part) at mu = 1e-4 against the DENSE host step, within C_BOUND times the spread h of the
    two host solvers of that point (dense against Schur-then-back-substitute), pose part in the metric of the system, landmark part max-relative;
    C_BOUND and H_FLOOR are those of tests/test_gpu_forms.py;
  - erase flags, per-landmark remaining counts and totals of covgpu_outlier_pass (k_lm_outliers) at the estimate one iteration leaves on the device,
    with keypoints displaced in the last lane of a full chunk, in the first lane of the second chunk, on all and on all but one observation of a
    landmark, against the thresholded host residual norms at the downloaded estimate.
One point per width also runs visual-inertial (pinhole), its largest point is fetched from a fresh second context bit for bit, and the second round of
a GlobalBundleAdjustment derived on the device is held to the literal two-flatten sequence on a map whose tracks flatten to the 4-lane form.

Observed on one MI355X. Step: error / max(h, 1e-13) per point in the order of the form's point list, pose part | landmark part (C_BOUND = 100):

  G = 4   pinhole   L 1, 63, 64, 65, 449   h 1.4e-13 .. 2.8e-12   0, 0.20, 0.73, 0.73, 0.42 | 5.88, 1.14, 1.14, 1.15, 0.95
  G = 4   unified   L 1, 63, 64, 65, 449   h 0 .. 8.1e-12         0, 0.73, 1.28, 1.15, 0.26 | 8.19, 0.85, 0.96, 0.92, 1.00
  G = 8   pinhole   L 31, 32, 33, 450      h 7.7e-13 .. 9.7e-12   0.06, 0.07, 0.06, 0.67 | 1.09, 0.85, 0.97, 1.04
  G = 8   unified   L 31, 32, 33, 450      h 8.5e-13 .. 1.3e-11   0.03, 0.21, 0.39, 0.39 | 1.05, 0.88, 1.11, 1.01
  G = 16  pinhole   L 15, 16, 17, 451      h 8.2e-13 .. 6.1e-12   0.30, 0.18, 0.37, 1.12 | 1.50, 1.27, 1.49, 1.08
  G = 16  unified   L 15, 16, 17, 451      h 1.7e-13 .. 4.6e-12   0.68, 0.50, 0.99, 0.54 | 3.74, 0.95, 3.79, 1.46

(L = 1: both observers of the single landmark are constant keyframes; the pose step is exactly zero on both sides, the landmark step differs by 8e-13
where the two host solvers differ by 1.4e-13 and 0: the floor of 1e-13 is what the ratio is taken against.)
Schur complement, normalised as in test_schur_complement (bounds 1e-9, cost 1e-12): mu = 1e-2: S <= 5e-14, b <= 2.8e-13 everywhere; mu = 1e-8: S <= 1.1e-10, b <= 4e-12
except at g8-L450 (b 6.7e-10 pinhole, 8.1e-10 unified) and g16-L451 (1.6e-10) — there the two host references, the oracle and the numpy Schur complement of the same
pinhole problem, differ by 6.2e-10 and 2.8e-10 themselves: the damped H_ll of a two-observation landmark with little parallax has a condition of 2e9
at mu = 1e-8. Cost <= 3.4e-14. Visual-inertial: S, b 1.1e-14, 1.4e-14. Outlier pass: no observation inside the 1e-9 margin at any point; 2 .. 22 erased,
1 .. 6 landmarks left short.
With k_lm_lin's re-evaluation skipped for two-chunk landmarks and k_lm_outliers reading the first chunk's keypoint in the second, 75 of the 88 tests fail;
with k_lm_backsub's butterfly one step short, the 24 step tests with more than one landmark do.
"""
import numpy as np
import pytest

from covins_amd import backend
from oracle import covo
from tests import lm_forms_util as lu
from tests.test_gpu_forms import C_BOUND, H_FLOOR

pytestmark = pytest.mark.gpu

VI_POINT = {G: lu.POINTS[G][-2] for G in (4, 8, 16)}        # one workgroup and one landmark: L = 65, 33, 17


@pytest.fixture(scope="module")
def ctx():
    c = backend.Context(0)
    yield c
    c.close()


def _problem(pt, cam):
    p = lu.build(pt, cam).p
    assert backend.lm_group(p.O, p.L) == pt.G and (p.cam_model is not None) == (cam == "unified")
    return p


def _check_schur(S, b, c, S0, b0, c0):
    """The normalisation and bounds of tests/test_gpu_parity.py::test_schur_complement."""
    assert abs(c - c0) <= 1e-12 * abs(c0), (c, c0)
    scale = np.sqrt(np.abs(np.diag(S0)))
    eS = np.abs(S / scale[:, None] / scale[None, :] - S0 / scale[:, None] / scale[None, :]).max()
    if b0.any():
        eb = np.abs(b / scale - b0 / scale).max() / np.abs(b0 / scale).max()
    else:       # (the single landmark of g4-L1 is seen by constant keyframes only: no right-hand side, on either side)
        eb = 0.0 if not b.any() else np.inf
    assert eS < 1e-9 and eb < 1e-9, (eS, eb)
    assert np.allclose(S, S.T)
    return eS, eb


@pytest.mark.parametrize("pt,cam", lu.ALL, ids=lu.IDS)
def test_schur_complement(ctx, pt, cam):
    p = _problem(pt, cam)
    ref = lu.host_reference(pt, cam)
    g = backend.default_options(visual_only=1)
    for mu in lu.MUS_SCHUR:
        S, b, c = ctx.schur(p, g, mu)
        S0, b0, c0 = ref["schur"][mu]
        eS, eb = _check_schur(S, b, c, S0, b0, c0)
        print(f"{pt.id}-{cam} mu={mu:g}: L={p.L} O={p.O} G={pt.G}  S {eS:.2e}  b {eb:.2e}  cost {abs(c - c0) / c0:.2e}")


@pytest.mark.parametrize("G", [4, 8, 16])
def test_schur_complement_visual_inertial(ctx, G):
    pt = VI_POINT[G]
    p = _problem(pt, "pinhole")
    assert p.I > 0
    g, o = backend.default_options(visual_only=0), covo.default_options(visual_only=0)
    for mu in lu.MUS_SCHUR:
        S, b, c = ctx.schur(p, g, mu)
        assert S.shape == (15 * p.K, 15 * p.K)
        eS, eb = _check_schur(S, b, c, *covo.schur(p, o, mu))
        print(f"{pt.id} visual-inertial mu={mu:g}: S {eS:.2e}  b {eb:.2e}")


@pytest.mark.parametrize("pt,cam", lu.ALL, ids=lu.IDS)
def test_gauss_newton_step(ctx, pt, cam):
    p = _problem(pt, cam)
    ref = lu.host_reference(pt, cam)
    dx, dl, cost = ctx.gn_step(p, backend.default_options(visual_only=1), lu.MU_STEP)
    e_pose = lu.scaled_err(dx, ref["x0"], ref["d"])
    e_lm = lu.rel(dl, ref["l0"])
    hp, hl = max(ref["h_pose"], H_FLOOR), max(ref["h_lm"], H_FLOOR)
    print(f"{pt.id}-{cam}: L={p.L} O={p.O} G={pt.G}  h_pose={ref['h_pose']:.2e} h_lm={ref['h_lm']:.2e} | device pose {e_pose:.2e} ({e_pose / hp:.2f} h)  "
          f"landmarks {e_lm:.2e} ({e_lm / hl:.2f} h)")
    c0 = ref["schur"][lu.MU_STEP][2]
    assert abs(cost - c0) <= 1e-12 * c0
    assert e_pose <= C_BOUND * hp, (e_pose, ref["h_pose"])
    assert e_lm <= C_BOUND * hl, (e_lm, ref["h_lm"])


def _host_norms(sol, cam):
    if cam == "pinhole":
        return covo.residual_norms(sol, covo.default_options(visual_only=1))
    from tests.test_omni_host import linearize_ref
    return np.linalg.norm(linearize_ref(sol, loss_a=1.0)[0], axis=1)


@pytest.mark.parametrize("pt,cam", lu.ALL, ids=lu.IDS)
def test_outlier_pass(ctx, pt, cam):
    p, rows = lu.outlier_problem(pt, cam)
    assert backend.lm_group(p.O, p.L) == pt.G
    th = lu.OUTLIER_THRESHOLD
    g = backend.default_options(visual_only=1, max_iterations=1)
    ctx.upload(p, g)
    res = ctx.solve_resident(g)
    sol = ctx.download()
    erase, left, (n_bad, n_short) = ctx.outlier_pass(p.O, p.L, th)
    n0 = _host_norms(sol, cam)
    outside = np.abs(n0 - th) > 1e-9              # (an observation exactly on the threshold may fall either way)
    print(f"{pt.id}-{cam}: iterations {res.iterations}, erased {n_bad} of {p.O}, landmarks left with < 2: {n_short}, inside the margin {(~outside).sum()}; "
          + ", ".join(f"{k} {int(erase[r].sum())}/{len(r)}" for k, r in rows.items()))
    assert res.iterations == 1
    assert (~outside).sum() <= 1
    assert np.array_equal(erase[outside], (n0 > th)[outside])
    obs_lm = np.repeat(np.arange(p.L), np.diff(p.lm_obs_ptr))
    assert np.array_equal(left, np.bincount(obs_lm, weights=~erase, minlength=p.L).astype(np.int32))
    assert (n_bad, n_short) == (int(erase.sum()), int((left < 2).sum()))
    assert n_bad > 0 and n_short > 0
    for k in ("last_lane", "chunk_2"):            # the displaced keypoint at the chunk boundary is what the rule removes
        if k in rows:
            assert erase[rows[k]].all() and (n0[rows[k]] > th).all(), k


@pytest.mark.parametrize("cam", lu.CAMERAS)
@pytest.mark.parametrize("G", [4, 8, 16])
def test_fresh_context_is_bit_identical(ctx, G, cam):
    """The kernels claim a fixed summation order: S, b and the cost of the form's largest point from a second, fresh context."""
    p = _problem(lu.LARGE[G], cam)
    g = backend.default_options(visual_only=1)
    S, b, c = ctx.schur(p, g, 1e-8)
    c2 = backend.Context(0)
    try:
        S2, b2, cc = c2.schur(p, g, 1e-8)
    finally:
        c2.close()
    assert cc == c and np.array_equal(S, S2) and np.array_equal(b, b2)


def test_device_second_round_at_four_lanes():
    """tests/test_gpu_omni.py::test_two_round_call_equals_the_literal_two_flatten_sequence on a map whose tracks are cut (Map.erase_observations) to
    the 4-lane pattern: the second round derived on the device against the literal second flattening."""
    from covins_amd import mapdata
    from covins_amd.optimization import Optimization
    pt = lu.LARGE[4]
    m, keep_n = lu.map_with_cut_tracks(pt, outlier_frac=0.03)
    p = mapdata.flatten_gba(m, False, False)[0]
    assert p.L == pt.L and sorted(np.diff(p.lm_obs_ptr).tolist()) == sorted(lu.point_lengths(pt).tolist())
    assert p.O / p.L <= 5 and backend.lm_group(p.O, p.L) == 4
    a, b = m.copy(), m.copy()
    ia = Optimization.GlobalBundleAdjustment(a, 10, -1.0, False, True, False, device_second_round=True)
    ib = Optimization.GlobalBundleAdjustment(b, 10, -1.0, False, True, False, device_second_round=False)
    print(f"K={p.K} L={p.L} O={p.O}: outliers removed {ia['outliers_removed']} | {ib['outliers_removed']}")
    assert ia["outliers_removed"] == ib["outliers_removed"] > 0
    assert ia["problem"] == ib["problem"]
    assert list(ia["round2"].accepted_trace[:10]) == list(ib["round2"].accepted_trace[:10])
    assert np.array_equal(a.lm_invalid, b.lm_invalid)
    assert np.abs(a.kf_pose - b.kf_pose).max() < 1e-10 and np.abs(a.lm_pos - b.lm_pos).max() < 1e-9
