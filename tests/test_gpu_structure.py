"""The reduced-system assembly on PRESCRIBED covisibility structures: the pair lists of k_pairs.hip (build_pairs_device, build_kf_lists_device,
round2_compact_device, k_obs_unpack), the reductions k_kf_reduce and k_pair_blocks of k_visual.hip, the edge gathers of k_between.hip and the host code
that feeds them (build_chains of plan_api.hip; key_of_kf and the edge-pair lists of upload.hip), against the oracle and numpy — never against the code under test.

The points are those of tests/structure_util.py (their structure is asserted on the CPU by tests/test_structure_host.py): exactly N covisible pairs of
one common landmark each on both sides of the group, chunk and round boundaries of k_pair_blocks; pairs of 1 .. 100 common landmarks and keyframes of
0 .. 129 observations around the lane and trip counts; keyframe counts around the powers of two of the radix key width; landmark and observation counts
around the 256-thread grids with empty and single-observation landmarks at the seams; two problems renumbered at random, so that tracks, IMU chains and
pair orientation run against the index order. Per point:
  - covgpu_covisibility at thresholds 1, 2 and the largest weight == the triples of the incidence matrix, exactly; the number of pair blocks of the
    reduced system (Context.layout()['covisible_pairs']) == the covisible pairs of FREE keyframes
  - S, b and the cost of covgpu_schur at mu = 1e-8 and 1e-2 against the oracle, normalised and bounded as test_schur_complement
  - the step of covgpu_gn_step at mu = 1e-4 against the oracle's whole-system step, within C_BOUND times the spread of the oracle's two solvers (floors
    and constant of tests/test_gpu_forms.py)
  - relabelled points: additionally the device against itself on the original numbering, and a full solve of the relabelled `tiny` map.
  (lone-free, whose single-observation landmarks are seen by free keyframes, is compared at mu = 1e-2 and by its step: structure_util._lone_tracks.)
Then the second round of covgpu_gba_two_round on planted erasures (first and last landmark, landmarks left with one and with two observations, a keyframe
left with none, all landmarks but one) against the literal sequence compact-in-numpy + solve; a pose graph with a hub of more than 256 edges, a triple
edge given in both orientations, an edge between constant keyframes and mixed losses; and the library's refusal of a landmark observed twice by one
keyframe.

Seen on the MI355X (every Schur figure against its bound of 1e-9; the step against C_BOUND x max(spread of the oracle's two solvers, H_FLOOR); cost <= 3.7e-15
against 1e-12 everywhere):
  point                S mu=1e-8  b         S mu=1e-2  b          pose: spread  error   bound   landmarks: spread  error   bound
  pairs-1              3.17e-14 7.43e-14   2.81e-14 7.56e-14   9.96e-14 2.01e-13 1.0e-11   3.07e-15 1.33e-14 1.0e-11
  pairs-8              2.17e-14 1.48e-14   2.07e-14 1.47e-14   1.16e-13 1.17e-13 1.2e-11   2.02e-14 3.02e-14 1.0e-11
  pairs-9              1.29e-14 1.98e-14   1.23e-14 2.02e-14   8.95e-14 1.73e-13 1.0e-11   3.34e-14 5.30e-14 1.0e-11
  pairs-512            4.34e-14 1.84e-14   3.19e-14 1.71e-14   3.80e-13 2.15e-13 3.8e-11   2.06e-13 2.03e-13 2.1e-11
  pairs-513            1.72e-13 2.30e-14   1.02e-13 2.33e-14   4.45e-13 3.73e-13 4.4e-11   3.71e-13 3.42e-13 3.7e-11
  pairs-4096           1.20e-12 1.86e-13   4.71e-14 3.29e-14   1.06e-12 7.24e-13 1.1e-10   1.30e-12 7.39e-13 1.3e-10
  pairs-4097           4.15e-13 3.16e-14   3.86e-14 3.11e-14   1.04e-12 7.01e-13 1.0e-10   2.03e-12 1.68e-12 2.0e-10
  lanes                2.44e-14 7.06e-15   2.43e-14 7.00e-15   5.87e-13 2.95e-13 5.9e-11   3.45e-12 2.27e-12 3.4e-10
  bits-2               7.25e-14 2.23e-14   7.52e-15 2.17e-14   2.98e-14 1.58e-13 1.0e-11   1.06e-13 3.15e-13 1.1e-11
  bits-3               3.60e-15 5.38e-15   3.93e-15 4.86e-15   7.61e-14 1.88e-14 1.0e-11   2.07e-15 1.56e-14 1.0e-11
  bits-4               2.66e-15 3.20e-15   2.71e-15 3.23e-15   6.94e-14 3.90e-14 1.0e-11   1.34e-14 4.06e-14 1.0e-11
  bits-5               3.26e-15 4.32e-15   3.89e-15 4.37e-15   7.12e-14 4.40e-14 1.0e-11   5.88e-15 1.19e-14 1.0e-11
  bits-64              2.67e-14 2.67e-14   1.85e-14 2.68e-14   2.21e-13 2.91e-13 2.2e-11   1.28e-14 4.65e-14 1.0e-11
  bits-65              1.50e-14 2.27e-14   1.51e-14 2.27e-14   1.87e-13 1.87e-13 1.9e-11   7.33e-14 1.25e-13 1.0e-11
  bits-128             2.02e-14 4.47e-14   2.04e-14 4.49e-14   5.44e-13 3.23e-13 5.4e-11   1.26e-13 9.31e-14 1.3e-11
  bits-129             2.00e-14 2.43e-14   1.99e-14 2.47e-14   3.86e-13 2.48e-13 3.9e-11   1.12e-13 1.99e-13 1.1e-11
  blocks-L255-O1023    1.37e-14 8.75e-15   1.39e-14 8.61e-15   1.37e-13 2.69e-13 1.4e-11   4.02e-13 7.51e-13 4.0e-11
  blocks-L255-O1024    9.21e-15 1.63e-14   9.18e-15 1.63e-14   1.05e-13 1.06e-13 1.1e-11   8.24e-13 4.62e-13 8.2e-11
  blocks-L255-O1025    1.71e-14 2.85e-14   1.82e-14 2.86e-14   1.70e-13 9.88e-14 1.7e-11   7.35e-13 1.01e-12 7.3e-11
  blocks-L256-O1023    8.28e-15 3.34e-14   7.90e-15 3.33e-14   1.02e-13 1.18e-13 1.0e-11   4.29e-13 1.09e-12 4.3e-11
  blocks-L256-O1024    2.37e-14 2.45e-14   1.96e-14 2.48e-14   1.56e-13 1.55e-13 1.6e-11   1.62e-13 5.53e-13 1.6e-11
  blocks-L256-O1025    1.70e-14 3.79e-14   1.67e-14 3.76e-14   2.20e-13 1.33e-13 2.2e-11   4.14e-13 1.72e-12 4.1e-11
  blocks-L257-O1023    1.65e-14 1.01e-14   1.75e-14 1.04e-14   1.46e-13 1.09e-13 1.5e-11   1.46e-12 6.61e-13 1.5e-10
  blocks-L257-O1024    1.14e-14 1.26e-14   1.13e-14 1.25e-14   2.36e-13 1.55e-13 2.4e-11   1.32e-13 9.36e-13 1.3e-11
  blocks-L257-O1025    1.04e-14 1.88e-14   1.05e-14 1.87e-14   2.36e-13 7.99e-14 2.4e-11   3.62e-13 7.51e-13 3.6e-11
  relabel-ring         1.51e-14 2.45e-14   1.46e-14 2.46e-14   1.04e-13 9.51e-14 1.0e-11   2.95e-12 2.83e-12 3.0e-10
  relabel-vi           7.76e-15 1.22e-14   7.37e-15 1.19e-14   3.72e-12 1.21e-12 3.7e-10   8.13e-12 7.13e-12 8.1e-10
  relabel-vi-reversed  7.76e-15 1.22e-14   7.37e-15 1.19e-14   3.67e-12 1.11e-12 3.7e-10   7.40e-12 7.52e-12 7.4e-10
  lone-free                   -        -   2.17e-14 1.12e-14   1.56e-11 1.92e-12 1.6e-09   3.62e-12 2.72e-12 3.6e-10
Relabelled against original on the device: S <= 5.6e-16, b <= 2.5e-16; the six erasure patterns: flags equal to the planted set, poses and landmarks equal to the
literal sequence to the last bit; pose graphs: r 5.1e-15, J 1.7e-15 (bound 1e-12), S 1.4e-17, b 2.1e-16 (bound 1e-10). The module takes 4.3 s.
"""
import numpy as np
import pytest

from covins_amd import backend
from oracle import covo
from tests import structure_util as su
from tests.test_gpu_edge_cases import check
from tests.test_gpu_forms import C_BOUND, H_FLOOR
from tests.test_gpu_lm_forms import _check_schur
from tests.test_gpu_parity import _NoValidate
from tests.util import rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = backend.Context(0)
    yield c
    c.close()


def _opts(pt, **kw):
    return backend.default_options(**su.options_kw(pt), **kw), covo.default_options(**su.options_kw(pt), **kw)


@pytest.mark.parametrize("pt", su.POINTS, ids=su.IDS)
def test_covisibility_and_pair_count(ctx, pt):
    p = su.build(pt).p
    g, _ = _opts(pt)
    ctx.upload(p, g)
    W, _ = su.incidence(p)
    top = int(np.tril(W, -1).max())
    for th in (1, 2, top):
        ki, kj, w = ctx.covisibility(th)
        ref = su.covisible_triples(W, th)
        assert len(ref) > 0 or th == 2
        assert list(zip(ki.tolist(), kj.tolist(), w.tolist())) == ref, th
    n_free = su.free_pairs(p, W)
    print(f"{pt.id}: K={p.K} L={p.L} O={p.O}  covisible pairs {len(su.covisible_triples(W, 1))}, of free keyframes {n_free}, largest weight {top}")
    assert ctx.layout()["covisible_pairs"] == n_free


@pytest.mark.parametrize("pt", su.POINTS, ids=su.IDS)
def test_schur_complement(ctx, pt):
    p = su.build(pt).p
    ref = su.host_reference(pt)
    g, _ = _opts(pt)
    for mu in su.schur_mus(pt):
        S, b, c = ctx.schur(p, g, mu)
        S0, b0, c0 = ref["schur"][mu]
        scale = np.sqrt(np.abs(np.diag(S0)))
        print(f"{pt.id} mu={mu:g}: S {np.abs((S - S0) / scale[:, None] / scale[None, :]).max():.2e}  b {np.abs((b - b0) / scale).max() / np.abs(b0 / scale).max():.2e}"
              f"  cost {abs(c - c0) / c0:.2e}  (bounds 1e-9, 1e-9, 1e-12)")
        _check_schur(S, b, c, S0, b0, c0)


@pytest.mark.parametrize("pt", su.POINTS, ids=su.IDS)
def test_gauss_newton_step(ctx, pt):
    p = su.build(pt).p
    ref = su.host_reference(pt)
    g, _ = _opts(pt)
    dx, dl, cost = ctx.gn_step(p, g, su.MU_STEP)
    e_pose, e_lm = su.scaled_err(dx, ref["x0"], ref["d"]), su.rel(dl, ref["l0"])
    hp, hl = max(ref["h_pose"], H_FLOOR), max(ref["h_lm"], H_FLOOR)
    print(f"{pt.id}: spread h_pose={ref['h_pose']:.2e} h_lm={ref['h_lm']:.2e} ({ref['whole']}) | device pose {e_pose:.2e} (bound {C_BOUND * hp:.1e}, {e_pose / hp:.2f} h)  "
          f"landmarks {e_lm:.2e} (bound {C_BOUND * hl:.1e}, {e_lm / hl:.2f} h)")
    c0 = ref["schur"][su.MU_STEP][2]
    assert abs(cost - c0) <= 1e-12 * c0
    assert e_pose <= C_BOUND * hp, (e_pose, ref["h_pose"])
    assert e_lm <= C_BOUND * hl, (e_lm, ref["h_lm"])


@pytest.mark.parametrize("pt", su.RELABELLED, ids=[pt.id for pt in su.RELABELLED])
def test_relabelled_problem_gives_the_device_the_same_answer(ctx, pt):
    """Additional to the oracle comparisons above: the device on the relabelled problem, mapped back, against the device on the original. The two differ
    in summation order only (S, b: the bound of the Schur comparison) and in the elimination order of the solve (step: the spread bound of this point)."""
    b = su.build(pt)
    ref = su.host_reference(pt)
    g, _ = _opts(pt)
    D = 6 if g.visual_only else 15
    r = su.rows_of(b.maps.kf, D)
    for mu in su.MUS_SCHUR:
        S0, b0, c0 = ctx.schur(b.orig, g, mu)
        S1, b1, c1 = ctx.schur(b.p, g, mu)
        eS, eb = _check_schur(S1[np.ix_(r, r)], b1[r], c1, S0, b0, c0)
        print(f"{pt.id} mu={mu:g}: device relabelled against device original: S {eS:.2e}  b {eb:.2e}")
    dx0, dl0, _ = ctx.gn_step(b.orig, g, su.MU_STEP)
    dx1, dl1, _ = ctx.gn_step(b.p, g, su.MU_STEP)
    d = ref["d"][r]                                                                        # sqrt(diag S) of the oracle, in the original keyframe order
    e_pose, e_lm = su.scaled_err(dx1[r], dx0, d), su.rel(dl1[b.maps.lm], dl0)
    hp, hl = max(ref["h_pose"], H_FLOOR), max(ref["h_lm"], H_FLOOR)
    print(f"{pt.id}: step relabelled against original: pose {e_pose:.2e} ({e_pose / hp:.2f} h)  landmarks {e_lm:.2e} ({e_lm / hl:.2f} h)")
    assert e_pose <= C_BOUND * hp and e_lm <= C_BOUND * hl


def test_full_solve_of_the_relabelled_visual_inertial_map(ctx):
    pt = su.BY_ID["relabel-vi"]
    g, o = _opts(pt)
    check(ctx, su.build(pt).p, g, o)
    assert ctx.layout()["chains"] == len(np.setdiff1d(np.arange(su.build(pt).p.K), su.build(pt).p.imu_kf_j))


# ------------------------------------------------------------------------------------------------ the second round on planted erasures
@pytest.mark.parametrize("name", su.ERASE_PATTERNS)
def test_second_round_on_planted_erasures(ctx, name):
    """covgpu_gba_two_round (round2_compact_device, the pair lists rebuilt on the device) against the literal sequence: compact the problem in numpy, solve
    that problem from the same initial estimate. Bounds of case (i) of test_two_round_call_degenerate_cases."""
    p, rows, want_left = su.erase_problem(name)
    planted = np.zeros(p.O, bool); planted[rows] = True
    o = backend.default_options(max_iterations=6, visual_only=1)
    sol, r1, r2, bad, left, (nb, ns) = ctx.gba_two_round(p, o, su.ERASE_THRESHOLD)
    print(f"{name}: erased {nb} (planted {len(rows)}), landmarks left short {ns} (expected {(want_left < 2).sum()})")
    assert np.array_equal(bad, planted)
    assert np.array_equal(left, want_left) and (nb, ns) == (len(rows), int((want_left < 2).sum()))
    q, keep = su.compact(p, planted)
    ref, rr = ctx.gba_solve(q, o)
    n = rr.iterations
    print(f"{name}: second round L={q.L} O={q.O}, iterations {r2.iterations} | {n}, final cost {r2.final_cost:.6e} | {rr.final_cost:.6e}, "
          f"poses {np.abs(sol.kf_pose - ref.kf_pose).max():.2e}, landmarks {np.abs(sol.lm_pos[keep] - ref.lm_pos).max():.2e}")
    n1 = covo.gba_solve(p, covo.default_options(max_iterations=5, visual_only=1))[1].iterations     # (the clean problem converges in four)
    assert r1.iterations == n1 <= 5 and r2.iterations == n and list(r2.accepted_trace[:6]) == list(rr.accepted_trace[:6])
    assert np.allclose(np.array(r2.cost_trace[:n]), np.array(rr.cost_trace[:n]), rtol=1e-12)
    assert np.abs(sol.kf_pose - ref.kf_pose).max() < 1e-10 and np.abs(sol.lm_pos[keep] - ref.lm_pos).max() < 1e-9
    assert np.array_equal(sol.lm_pos[~keep], p.lm_pos[~keep])                              # dropped landmarks come back untouched
    assert np.array_equal(sol.kf_pose[p.kf_fixed == 1], p.kf_pose[p.kf_fixed == 1])


# ------------------------------------------------------------------------------------------------ a pose graph with awkward incidence
@pytest.mark.parametrize("name", su.PG_NAMES)
def test_pose_graph_edge_gathers(ctx, name):
    p = su.pose_graph(name)
    g, o = backend.default_options(), covo.default_options()
    r, J, c = ctx.linearize_between(p, g)
    r0, J0, c0 = covo.linearize_between(p, o)
    print(f"{name}: E={p.E}  r {rel_err(r, r0):.2e}  J {rel_err(J, J0):.2e}  cost {rel_err(c, c0):.2e}  (bound 1e-12)")
    assert rel_err(r, r0) < 1e-12 and rel_err(J, J0) < 1e-12 and rel_err(c, c0) < 1e-12
    S, b, cc = ctx.schur(p, g, 1e-8, pgo=True)
    S0, b0, cc0 = covo.schur(p, o, 1e-8, pgo=True)
    print(f"{name}: S {rel_err(S, S0):.2e}  b {rel_err(b, b0):.2e}  cost {abs(cc - cc0) / cc0:.2e}  (bound 1e-10, 1e-10, 1e-12)")
    assert rel_err(S, S0) < 1e-10 and rel_err(b, b0) < 1e-10 and abs(cc - cc0) < 1e-12 * cc0
    assert np.allclose(S, S.T)


@pytest.mark.parametrize("name", su.PG_NAMES)
def test_pose_graph_solve(ctx, name):
    p = su.pose_graph(name)
    sol, ref = check(ctx, p, backend.default_options(), covo.default_options(), pgo=True)
    fx = np.nonzero(p.kf_fixed)[0]
    assert np.array_equal(sol.kf_pose[fx], p.kf_pose[fx])


# ------------------------------------------------------------------------------------------------ one observation per landmark and keyframe
def test_library_refuses_a_landmark_observed_twice_by_one_keyframe(ctx):
    p = su.build(su.BY_ID["bits-5"]).p.copy()
    g = backend.default_options(visual_only=1)
    ctx.gba_solve.__func__(ctx, _NoValidate(p), g)                                         # (valid as built)
    o0 = p.lm_obs_ptr[3]
    p.obs_kf[o0 + 1] = p.obs_kf[o0]
    with pytest.raises(backend.CovGpuError, match="landmark observed twice by one keyframe"):
        ctx.gba_solve.__func__(ctx, _NoValidate(p), g)
    with pytest.raises(backend.CovGpuError, match="landmark observed twice by one keyframe"):
        ctx.schur(p, g, 1e-4)
    with pytest.raises(backend.CovGpuError, match="landmark observed twice by one keyframe"):
        ctx.upload(p, g)
