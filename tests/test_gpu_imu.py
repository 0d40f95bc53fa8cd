"""The inertial path on the device — k_preintegrate, imu_unwhitened / imu_stage (inertial_dev.hpp), k_imu_build, k_imu_gather, the inertial half of
k_pose_finish and the three-launch finish beside it (enqueue_build), the IMU segments of k_tail_jvp / k_tail_cost — on the points of tests/imu_util.py
(its docstring is the table; tests/test_imu_host.py asserts each point's property on the CPU), against the long double restatement of tests/imu_ref.py.

  1 preintegration   covgpu_preintegrate: delta, J, P per factor, relative to that factor's largest reference entry
  2 factor           covgpu_linearize_imu: whitened r, J per factor, and J^T J, J^T r (formed in long double from the returned r, J). fixed-inside: the
                     columns of constant poses are exactly zero. bias-shift: the block (3..5, 12..14) of the un-whitened Jacobian, recovered as W_ref^-1 J,
                     is held to the restatement's on its own scale and differs from its value at zero shift by far more than that bound
  3 reduced system   covgpu_schur at mu = 1e-8 and 1e-2 against covo.schur, normalised and bounded as tests/test_gpu_lm_forms._check_schur, on every point;
                     the cross blocks of the added edges alone on edge-beside / edge-far; identity speed-bias rows on count-I; the one-sample rule
  4 step             covgpu_gn_step at mu = 1e-4 against the oracle's whole-system step within C_BOUND x max(spread of its two solvers, H_FLOOR)
  5 solve            tests.test_gpu_edge_cases.check with max_iterations = 5: iterations, termination, accepted trace, final cost, poses
  6 twice            edge-beside from a fresh second context: S, b and the step bit for bit

Bounds. Wherever the calibration is the map's (every point but mixed-calib) those of tests/test_gpu_parity.py, per factor: delta 1e-12, J 1e-11, P 1e-11;
whitened r, J 1e-8 overall and 1e-7 per factor. On top, for every point and quantity, per factor:
    device - restatement  <=  MARGIN x max(e_orc, floor)
e_orc: the ORACLE's largest per-factor distance from the restatement at that point (imu_util.host_reference; the figures are in test_imu_host.py's
docstring); floor: 2^-52 x samples of the factor for the preintegration, 2^-52 x cond(chol P_ref) for the whitened quantities (cond = 1.46e4 .. 1.65e4 at
every point, mixed-calib's agent B included: 1.47e4). Both sides evaluate the same recurrences in FP64 and differ in summation order and contraction
only; MARGIN covers that and nothing else. MARGIN = 10 unless the worst ratio seen leaves less than a factor 3 under it (then 30, then 100: the
rule of tests/test_gpu_forms.py for C_BOUND).

Seen on the MI355X (e_dev | e_orc | worst per-factor e_dev / max(e_orc, floor); largest per-factor distances):
  point            delta                       J (preintegration)          P                           whitened r                  whitened J                J^T J                     J^T r
  bias-shift       4.48e-16 4.48e-16 0.04    6.91e-16 6.91e-16 0.06    2.67e-15 2.22e-15 0.24    7.87e-16 7.87e-16 0.00    6.84e-16 6.84e-16 0.00    1.37e-15 1.37e-15 0.00    1.47e-15 1.47e-15 0.00
  bias-shift-one   4.43e-16 4.22e-16 0.04    7.12e-16 7.12e-16 0.06    3.10e-15 2.29e-15 0.28    5.43e-14 5.07e-14 0.02    6.44e-16 6.44e-16 0.00    1.29e-15 1.29e-15 0.00    1.05e-13 1.72e-13 0.03
  ragged-cut       3.08e-16 3.08e-16 0.36    7.12e-16 7.12e-16 0.17    2.46e-15 1.34e-15 0.46    3.45e-14 1.18e-13 0.01    6.44e-16 6.44e-16 0.00    1.29e-15 1.29e-15 0.00    2.67e-14 1.43e-13 0.01
  count-1          8.35e-17 2.75e-17 0.19    3.02e-17 3.02e-17 0.07    4.17e-16 1.23e-16 0.94    4.35e-16 2.44e-16 0.00    9.12e-17 9.12e-17 0.00    1.82e-16 1.82e-16 0.00    6.36e-16 1.43e-16 0.00
  count-3, -4      1.12e-16 1.12e-16 0.19    7.12e-16 7.12e-16 0.06    1.86e-15 1.12e-15 0.44    1.75e-14 2.19e-14 0.01    5.01e-16 5.01e-16 0.00    1.00e-15 1.00e-15 0.00    2.00e-14 2.34e-14 0.01
  count-5          3.08e-16 3.08e-16 0.19    7.12e-16 7.12e-16 0.06    1.86e-15 1.31e-15 0.44    3.45e-14 5.07e-14 0.01    6.44e-16 6.44e-16 0.00    1.29e-15 1.29e-15 0.00    2.00e-14 2.34e-14 0.01
  ragged-fused     6.84e-16 5.59e-16 0.03    7.57e-16 7.57e-16 0.06    3.37e-15 2.57e-15 0.28    2.91e-13 2.58e-13 0.08    1.42e-15 1.42e-15 0.00    2.85e-15 2.85e-15 0.00    3.25e-13 2.99e-13 0.09
  mixed-calib      4.43e-16 4.22e-16 0.04    7.12e-16 7.12e-16 0.06    3.78e-15 3.02e-15 0.34    1.07e-13 1.61e-13 0.03    6.44e-16 6.44e-16 0.00    1.29e-15 1.29e-15 0.00    2.51e-13 3.47e-13 0.08
  fixed-inside, edge-beside, edge-far, edge-none (the inertial data of bias-shift-one without the shift)
                   4.43e-16 4.22e-16 0.04    7.12e-16 7.12e-16 0.06    3.10e-15 2.29e-15 0.28    5.43e-14 5.07e-14 0.02    6.44e-16 6.44e-16 0.00    1.29e-15 1.29e-15 0.00    1.05e-13 1.72e-13 0.03
  one-sample       3.08e-16 3.08e-16 0.36    7.12e-16 7.12e-16 0.17    2.46e-15 1.34e-15 0.46    3.45e-14 1.18e-13 0.01    6.44e-16 6.44e-16 0.00    1.29e-15 1.29e-15 0.00    2.67e-14 1.43e-13 0.01
The worst ratio is 0.94 (P of count-1, a factor of two samples: e_dev 4.2e-16 against a floor of 4.4e-16): more than a factor 3 under 10, so MARGIN = 10. The whitened
quantities stay two orders under their floor on both sides (the floor is the worst case of the triangular inverse; J and J^T J of the device equal the oracle's distance
digit for digit). bias-shift: the block (3..5, 12..14) recovered from the device is 1.6e-15 of its largest entry from the restatement's; the shift moves it by at least
2.9e-4. Reduced systems: S <= 3.9e-14, b <= 2.1e-14, cost <= 3.1e-15 (bounds 1e-9, 1e-9, 1e-12); the pose block (7, 5) of edge-beside 4.0e-15 of its largest entry
3.8e8, the edge blocks of edge-far <= 3.2e-13. Step: 0.16 .. 0.69 (poses) and 0.86 .. 1.04 (landmarks) spreads of the oracle's two solvers (1.1e-12 .. 7.3e-12), bound
100 spreads. Solve: equal traces, speed-bias blocks within 2.7e-10 after the biases moved by 0.03 .. 0.07. The module takes 2.6 s.

Without the one-sample rule (k_preintegrate deciding by its pivots alone) one of the three one-sample factors passed the pivot test on the MI355X: reserved was 2, the
whitened J of the point was 1.6e6 of its largest reference entry away (bound 1e-8) and the cost of the point 1.2e23 instead of 8.9e10. Mutations of the library, tried once by hand: Jq_bg transposed
in imu_unwhitened: 39 of the 55 tests fail; mul(Jv_bg, dbg) dropped: 33; the calibration of factor 0 for every factor: the 4 of mixed-calib; `on` replaced by `true` in the
J <- F J step of k_preintegrate: 20 (every point with ragged lengths); the cross-block addition of k_imu_gather skipped: the 4 of edge-beside.
tests/test_gpu_parity.py::test_preintegration and ::test_imu_factor pass on the last three. They fail test_imu_factor on the first two: agent A of the synthetic maps
carries a bias random walk of 2e-5 m/s^2 and 1e-7 rad/s from keyframe to keyframe, and the block -L(e^-1) J[R,BG] does not depend on dbg at all.
"""
import time

import numpy as np
import pytest

from covins_amd import backend
from oracle import covo
from tests import imu_ref
from tests import imu_util as iu
from tests.test_gpu_edge_cases import check
from tests.test_gpu_forms import C_BOUND, H_FLOOR
from tests.test_gpu_lm_forms import _check_schur
from tests.util import rel_err

pytestmark = pytest.mark.gpu

MARGIN = 10
PARITY_PRE = dict(delta=1e-12, J=1e-11, P=1e-11)        # tests/test_gpu_parity.py::test_preintegration, per factor
PARITY_OVERALL, PARITY_FACTOR = 1e-8, 1e-7              # tests/test_gpu_parity.py::test_imu_factor


@pytest.fixture(scope="module")
def ctx():
    t0 = time.perf_counter()
    c = backend.Context(0)
    yield c
    c.close()
    print(f"\ntests/test_gpu_imu.py: {time.perf_counter() - t0:.1f} s")


def _opts(**kw):
    return backend.default_options(**kw), covo.default_options(**kw)


def _hold(pid, dist, quantities):
    """device - restatement <= MARGIN x max(e_orc, floor), per factor; prints e_dev, e_orc and the worst ratio per quantity."""
    h = iu.host_reference(pid)
    bad = []
    line = []
    for k in quantities:
        bound = np.maximum(h["e_orc"][k], h["floor"][k])
        ratio = np.where(bound > 0, dist[k] / np.where(bound > 0, bound, 1.0), np.where(dist[k] > 0, np.inf, 0.0))
        line.append(f"{k} {dist[k].max():.2e} | {h['e_orc'][k]:.2e} | {ratio.max():.2f}")
        if not np.all(ratio <= MARGIN):
            bad.append((k, float(ratio.max())))
    print(f"{pid}: device | oracle | worst device / max(e_orc, floor):  " + "   ".join(line))
    assert not bad, bad


@pytest.mark.parametrize("pid", iu.IDS)
def test_preintegration(ctx, pid):
    p, h = iu.build(pid), iu.host_reference(pid)
    g, _ = _opts()
    d, J, P = ctx.preintegrate(p, g)
    dist = iu.distances(h["ref"], pre=(d, J, P))
    if pid in iu.DEFAULT_CALIB_IDS:
        for k, bound in PARITY_PRE.items():
            assert dist[k].max() < bound, (k, dist[k].max())
    _hold(pid, dist, iu.PRE_QUANTITIES)


@pytest.mark.parametrize("pid", iu.IDS)
def test_factor(ctx, pid):
    p, h = iu.build(pid), iu.host_reference(pid)
    ref = h["ref"]
    g, _ = _opts()
    r, J = ctx.linearize_imu(p, g)
    dist = iu.distances(ref, lin=(r, J))
    if pid == "mixed-calib":
        odd = np.arange(p.I) % 2 == 1
        print(f"mixed-calib: cond(chol P_ref) agent A {ref['cond'][~odd].max():.3e}, agent B {ref['cond'][odd].max():.3e}")
    else:
        r0, J0 = ref["r"].astype(np.float64), ref["Jw"].astype(np.float64).reshape(p.I, 450)
        assert rel_err(r, r0) < PARITY_OVERALL and rel_err(J, J0) < PARITY_OVERALL
        assert dist["r"].max() < PARITY_FACTOR and dist["Jw"].max() < PARITY_FACTOR
    _hold(pid, dist, iu.WHITE_QUANTITIES)
    w = ref["n"] < 2
    assert not r[w].any() and not J[w].any()                             # a factor without weight: exact zeros
    assert np.all(np.abs(J[~w]).max(axis=1) > 0)
    J3 = J.reshape(p.I, 15, 30)
    fi, fj = p.kf_fixed[p.imu_kf_i] == 1, p.kf_fixed[p.imu_kf_j] == 1
    assert not J3[fi][:, :, 0:6].any() and not J3[fj][:, :, 15:21].any()  # the columns of constant poses
    assert np.all(np.abs(J3[~fi & ~w][:, :, 0:6]).max(axis=(1, 2)) > 0) and np.all(np.abs(J3[~fj & ~w][:, :, 15:21]).max(axis=(1, 2)) > 0)
    if pid == "fixed-inside":
        assert (fi & fj).sum() == 1 and (fi & ~fj).sum() >= 2 and (~fi & fj).sum() >= 2


def test_bias_correction_block_is_not_compared_on_zeros(ctx):
    """bias-shift: the block d r_theta / d bg_i = -L(e^-1) J[R,BG] of the un-whitened Jacobian, recovered from the device's whitened J as W_ref^-1 J = chol(P_ref) J,
    against the restatement's, on the block's own scale; and the restatement's block at zero shift (the same poses and velocities) is far further away
    than that bound: dq_c, and with it e, moved."""
    p, ref = iu.build("bias-shift"), iu.host_reference("bias-shift")["ref"]
    zero = imu_ref.problem(iu.zero_shift("bias-shift"))
    g, _ = _opts()
    _, J = ctx.linearize_imu(p, g)
    J = J.reshape(p.I, 15, 30)
    worst, least = 0.0, np.inf
    for f in range(p.I):
        C = imu_ref.chol_lower(ref["P"][f])
        blk = (C @ J[f].astype(imu_ref.LD))[3:6, 12:15]
        want, at_zero = ref["A"][f][3:6, 12:15], zero["A"][f][3:6, 12:15]
        scale = np.abs(want).max()
        worst = max(worst, float(np.abs(blk - want).max() / scale))
        least = min(least, float(np.abs(want - at_zero).max() / scale))
    print(f"bias-shift: block (3..5, 12..14): device against restatement {worst:.2e} of the block's largest entry (bound 1e-9); the shift moves it by at least {least:.2e}")
    assert worst < 1e-9 and least > 1e4 * 1e-9


def _edge_blocks(p):
    return sorted({(int(max(i, j)), int(min(i, j))) for i, j in zip(p.edge_i[iu.base().E:], p.edge_j[iu.base().E:])})


@pytest.mark.parametrize("pid", iu.IDS)
def test_reduced_system(ctx, pid):
    p = iu.build(pid)
    sysref = iu.system_reference(pid)
    g, _ = _opts()
    for mu in iu.MUS_SCHUR:
        S, b, c = ctx.schur(p, g, mu)
        S0, b0, c0 = sysref["schur"][mu]
        scale = np.sqrt(np.abs(np.diag(S0)))
        print(f"{pid} mu={mu:g}: S {np.abs((S - S0) / scale[:, None] / scale[None, :]).max():.2e}  b {np.abs((b - b0) / scale).max() / np.abs(b0 / scale).max():.2e}"
              f"  cost {abs(c - c0) / c0:.2e}  (bounds 1e-9, 1e-9, 1e-12)")
        _check_schur(S, b, c, S0, b0, c0)
        if pid in iu.EDGE_IDS:
            for hi, lo in _edge_blocks(p):                               # the pair block of every added edge alone, on its own scale: all 15 x 15 and its pose part
                for n in (15, 6):
                    B, B0 = S[15 * hi:15 * hi + n, 15 * lo:15 * lo + n], S0[15 * hi:15 * hi + n, 15 * lo:15 * lo + n]
                    e = np.abs(B - B0).max() / np.abs(B0).max()
                    print(f"{pid} mu={mu:g}: block ({hi}, {lo}) {n} x {n}: {e:.2e} of its largest entry {np.abs(B0).max():.2e}")
                    assert e < 1e-9
        if pid.startswith("count-"):
            lone = np.setdiff1d(np.arange(p.K), np.concatenate([p.imu_kf_i, p.imu_kf_j]))
            rows = (15 * lone[:, None] + np.arange(6, 15)[None, :]).reshape(-1)
            assert len(lone) == p.K - len(set(p.imu_kf_i) | set(p.imu_kf_j)) >= p.K - 2 * p.I
            for M, v in ((S, b), (S0, b0)):                              # speed-bias rows of keyframes without a factor: identity rows, no right-hand side
                assert np.array_equal(M[rows], np.eye(15 * p.K)[rows]) and np.array_equal(M[:, rows], np.eye(15 * p.K)[:, rows]) and not v[rows].any()


def test_one_sample_factors_are_counted(ctx):
    """The rule of covgpu_result::reserved: the three one-sample factors are reported, carry no weight (test_factor holds their r and J to exact zeros, test_reduced_system
    S, b and the cost to the oracle's, which leaves them out by the same rule), and the ragged point without them reports none."""
    g, _ = _opts(max_iterations=1)
    _, res = ctx.gba_solve(iu.build("one-sample"), g)
    assert res.reserved == len(iu.ONE_SAMPLE) == 3
    _, res = ctx.gba_solve(iu.build("ragged-cut"), g)
    assert res.reserved == 0


@pytest.mark.parametrize("pid", iu.STEP_IDS)
def test_gauss_newton_step(ctx, pid):
    p, ref = iu.build(pid), iu.system_reference(pid)
    g, _ = _opts()
    dx, dl, cost = ctx.gn_step(p, g, iu.MU_STEP)
    e_pose, e_lm = iu.scaled_err(dx, ref["x0"], ref["d"]), iu.rel(dl, ref["l0"])
    hp, hl = max(ref["h_pose"], H_FLOOR), max(ref["h_lm"], H_FLOOR)
    print(f"{pid}: spread h_pose={ref['h_pose']:.2e} h_lm={ref['h_lm']:.2e} | device pose {e_pose:.2e} (bound {C_BOUND * hp:.1e}, {e_pose / hp:.2f} h)  "
          f"landmarks {e_lm:.2e} (bound {C_BOUND * hl:.1e}, {e_lm / hl:.2f} h)")
    c0 = ref["schur"][iu.MU_STEP][2]
    assert abs(cost - c0) <= 1e-12 * c0
    assert e_pose <= C_BOUND * hp, (e_pose, ref["h_pose"])
    assert e_lm <= C_BOUND * hl, (e_lm, ref["h_lm"])


@pytest.mark.parametrize("pid", iu.SOLVE_IDS)
def test_solve(ctx, pid):
    """Five iterations: the IMU segments of k_tail_jvp / k_tail_cost after the biases have moved away from the linearisation point."""
    p = iu.build(pid)
    g, o = _opts(max_iterations=5)
    sol, ref = check(ctx, p, g, o)
    moved = np.abs(sol.kf_speed_bias[:, 3:] - p.kf_speed_bias[:, 3:]).max()
    print(f"{pid}: biases moved by up to {moved:.2e}; speed-bias device against oracle {np.abs(sol.kf_speed_bias - ref.kf_speed_bias).max():.2e}")
    assert moved > 0
    assert np.abs(sol.kf_speed_bias - ref.kf_speed_bias).max() < 1e-6


def test_edge_beside_imu_twice_bit_for_bit(ctx):
    """The three launches that finish the pose dimensions where a loop edge lies on an IMU cross block are ordered by launch order only: the same S, b
    and cost, to the last bit, from the module's context and from a fresh one, and the same step from two fresh ones. (The step of the module's context is
    no party to that: a context keeps the elimination tree of its previous upload while the new problem's couplings are a subset of that one's —
    up_choose_plan's plan cache; edge-far's tree serves edge-beside — and another valid elimination order rounds differently.)"""
    p = iu.build("edge-beside")
    g, _ = _opts()
    S, b, c = ctx.schur(p, g, 1e-8)
    fresh = []
    for _ in range(2):
        c2 = backend.Context(0)
        try:
            fresh.append(c2.schur(p, g, 1e-8) + c2.gn_step(p, g, iu.MU_STEP))
        finally:
            c2.close()
    for S2, b2, cc, _, _, _ in fresh:
        assert cc == c and np.array_equal(S, S2) and np.array_equal(b, b2)
    (_, _, _, dx, dl, cost), (_, _, _, dx2, dl2, cost2) = fresh
    assert dx.any() and cost2 == cost and np.array_equal(dx, dx2) and np.array_equal(dl, dl2)
