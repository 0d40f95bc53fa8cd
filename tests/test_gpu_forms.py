"""Every kernel form of the multifrontal solve, at small sizes, against host solvers.

Which kernel a launch of the multifrontal FP64 Cholesky takes (k_chol.hip, k_panel.hip, k_bwd.hip, k_front.hip) is decided by the shape of the fronts: the
four-wave panel factorisation by the number of small fronts in a level, the width of k_trsm_sub4 by the real columns of a panel, full tiles or
quadrants by the length of a tile list, the backward substitution by the interior tiles of a level, ... The default plans of the small maps reach
few of them. Here ONE context runs a sweep of plan shapes (tests/forms_util.SWEEP: maps x leaf sizes x the two cuts of three agents; the host half
of it is tests/test_nd_plan.py::test_sweep_of_plan_shapes_reaches_what_the_device_test_relies_on), one damped Gauss-Newton step per point, and

  - every step is held to the spread of the HOST solvers of the same system: the oracle's S, b (covo.schur_sparse) solved by SuperLU (x_lu), by
    dense LAPACK (n <= 9 000) and by the numpy replay of the same plan (tests/test_nd_plan._replay_sparse); h = their largest pairwise difference in
    the metric max |(x - y) d| / max |x_lu d|, d = sqrt(diag S), r_h = their largest relative residual. The device step must satisfy
    err(dx, x_lu) <= C max(h, 1e-13) and |S dx - b| / |b| <= C max(r_h, 1e-16), and its cost the oracle's to 1e-10. Never compared with
    another run of the device code;
  - after every step the census of kernel forms is read (Context.kernel_forms()): over the sweep EVERY form named in include/covgpu.h must have run,
    except the ones listed below with their reasons;
  - three points are repeated on a fresh context each: dx, dl and the cost must be bit-identical to what the context with history returned
    (cached plan, cached live-tile lists, border tiles stored by the extend-add instead of cleared).

References above 9 000 unknowns: the replay runs once, at the four-wave point, and serves the map's other point; at 36 000 unknowns (the 12-agent point)
SuperLU gives up ("not enough memory"), the reference there is the LAPACK multifrontal port oracle/covo_mf.py and the second host solver the replay.

C = 100: the smallest of 10, 30, 100 that leaves a factor 3 over the worst observed ratio err / h (17.8). Observed on one MI355X (err / h | residual / r_h):

  mh123-leaf15        mu 1e-4  n 22 125  1 509 fronts / 13 levels  h 5.4e-13   5.5 | 1.0    k_potrf_panel4: 1 launch, 494 fronts
  mh123-leafdefault   mu 1e-4  n 22 125    200 / 7                 h 5.4e-13   7.4 | 1.0    no k_potrf_panel4
  small               leaf 128, 15, 60, default   mu 1e-4  n 2 700   h 2.6e-12 .. 3.8e-12   0.83, 0.81, 0.55, 0.42 | 0.96 .. 1.01;  leaf 15 mu 1e-8: h 4.2e-9  0.37 | 0.80
  mh123@200           leaf 1920, top 0, top 1, 15, 128, 256   mu 1e-4  n 9 000   h 5.3e-12   0.35, 0.31, 0.38, 0.23, 0.27, 0.28 | 0.97 .. 1.03;  leaf 15 mu 1e-8: h 6.2e-8  0.03 | 0.80
  mh01-vo             leaf 1920, 15, 128, 384   mu 1e-4  n 3 288   h 3.0e-13 .. 3.4e-13   14.5, 13.8, 15.3, 15.2 | 9.6, 9.6, 9.5, 9.9;  leaf 128 mu 1e-8: h 5.2e-10  7.8 | 7.4
  a12x1000@200        default  mu 1e-4  n 36 000  271 / 8   h 1.8e-12 (LAPACK multifrontal against the replay: both in the device's elimination order)   17.8 | 3.0
  pose graph          mh123@200 / mh12345, leaf 6, 60, 384, default: oracle's own spread (dense Cholesky against SuperLU) 2.0e-14 / 1.1e-12 m on poses; device 0.04 .. 0.06 of it

The visual-only ratios do not move between 3 fronts and 65: they are the system's, not a kernel form's — the device assembles S in another summation
order than the oracle (whose S all host solvers share); its cost differs from the oracle's by 1.3e-14 there against 1e-16 on the visual-inertial maps.
Cost: <= 2.3e-15 relative on the visual-inertial maps.
"""
import numpy as np
import pytest

from covins_amd import backend, capi, mapdata, synth
from oracle import covo
from tests import forms_util as fu

pytestmark = pytest.mark.gpu

C_BOUND = 100         # factor over the host solvers' spread: the smallest of 10, 30, 100 that leaves a factor 3 over the worst observed ratio (15.1)
H_FLOOR, R_FLOOR = 1e-13, 1e-16

# Forms the sweep is NOT required to reach, each with its reason. Everything else named in include/covgpu.h must run at some sweep point.
EXCEPTIONS = {
    # only a non-default environment switch selects them (tests/test_gpu_schedule.py runs those switches)
    "k_nd_extend": "COVGPU_EXT_RECORDS=0",
    "last_update_whole": "COVGPU_ND_LOOKAHEAD=0 (and the arrow blocks of the block-arrow pose graph)",
    "k_bwd_given": "launch-per-tile substitution of a front with a border: COVGPU_BWD_PIPE=0 / COVGPU_ND_BWD_FUSED=0, and the block-arrow pose graph",
    # forms of the sharded solve (tests/test_gpu_shard*.py)
    "k_nd_top_pack": "sharded solve", "k_nd_gh": "sharded solve", "k_nd_top_damp": "sharded solve", "k_nd_panel_xfer": "sharded solve, distributed top",
    "dist_panel": "sharded solve, distributed top",
    # the pose graph without its elimination tree (COVGPU_PGO_ND=0 / COVGPU_PGO_DENSE=1: test_pgo_block_arrow_solve_equals_dense_solve)
    "pgo_arrow": "block-arrow pose-graph solve", "pgo_dense": "dense pose-graph solve",
    # forms of the one-matrix dense solve, which no front of a tree takes: tests/test_gpu_parity.py::test_mfma_cholesky_solve_forms asserts them
    "panel_one_tile": "a front's interior is padded to whole 256-column panels; only the dense solve has an odd tile count to factor",
    "k_bwd_step_sub": "launch-per-tile substitution: the dense solve, COVGPU_BWD_PIPE=0",
}
# Named in the header, reachable by no plan: a level's padded interior order is the round-up of its largest REAL interior order (front_layout,
# nd_tables.hip), so no panel of a level is all padding. Asserted to stay at zero: if one comes alive, the sweep has to reach it.
DEAD = {"potrf_skipped": "no all-padding panel exists in a level", "kd_zero": "no all-padding panel exists in a level"}


@pytest.fixture(scope="module")
def shared():
    c = backend.Context(0)
    state = dict(ctx=c, runs={})
    yield state
    c.close()


def _step(ctx, pt, mu):
    with fu.forced_env(pt, leaf_too=True):     # COVGPU_ND_LEAF / COVGPU_ND_TOP are read on every upload
        dx, dl, cost = ctx.gn_step(fu.point_problem(pt), fu.point_options(pt), mu)
        return dict(dx=dx, dl=dl, cost=cost, forms=ctx.kernel_forms(), layout=ctx.layout())


def _run_through(shared, pt):
    """The shared context's history is always SWEEP's order: every point up to `pt` that has not run yet runs first."""
    for q in fu.SWEEP:
        if q.id not in shared["runs"]:
            shared["runs"][q.id] = {mu: _step(shared["ctx"], q, mu) for mu in q.mus}
        if q is pt:
            break
    return shared["runs"][pt.id]


def _fmt(forms):
    return ", ".join(f"{k}={v}" for k, v in forms.items() if v)


@pytest.mark.parametrize("pt", fu.SWEEP, ids=[p.id for p in fu.SWEEP])
def test_sweep_point(shared, pt):
    runs = _run_through(shared, pt)
    info = fu.host_plan(pt)[0]
    shape = fu.plan_shape(pt)
    for mu in pt.mus:
        r = runs[mu]
        sysm = fu.host_system(pt, mu)
        h, r_h, xs = fu.host_spread(pt, mu)
        err = fu.scaled_err(r["dx"], sysm["x_ref"], sysm["d"])
        res = float(np.linalg.norm(sysm["S"] @ r["dx"] - sysm["b"]) / np.linalg.norm(sysm["b"]))
        print(f"{pt.id} mu={mu:g}: n={sysm['n']} fronts={r['layout']['nd_fronts']} levels={r['layout']['nd_levels']} host {'/'.join(sorted(xs))} h={h:.2e} r_h={r_h:.2e} | "
              f"device err={err:.2e} ({err / max(h, H_FLOOR):.2f} h) residual={res:.2e} ({res / max(r_h, R_FLOOR):.2f} r_h) | {_fmt(r['forms'])}")
        msg = f"{pt.id} mu={mu:g}: forms that ran: {_fmt(r['forms'])}"
        assert abs(r["cost"] - sysm["cost"]) <= 1e-10 * sysm["cost"], msg
        assert err <= C_BOUND * max(h, H_FLOOR), (err, h, msg)
        assert res <= C_BOUND * max(r_h, R_FLOOR), (res, r_h, msg)
        # the device ran THIS point's plan (the plan cache keys on the leaf size and on the cut of three agents): fronts, levels, root order
        lay = r["layout"]
        assert (lay["nd_fronts"], lay["nd_levels"]) == (info[0], info[1]) == (shape["fronts"], shape["levels"]), (lay, msg)
        assert lay["nd_root_order"] == max(256, -(-shape["root_order"] // 256) * 256), (lay, shape["root_order"])


def test_every_kernel_form_ran(shared):
    _run_through(shared, fu.SWEEP[-1])
    names = backend.kernel_form_names()
    assert set(EXCEPTIONS) | set(DEAD) <= set(names)
    ran = {k: {} for k in names}     # form -> {point: count}
    for pt in fu.SWEEP:
        for mu, r in shared["runs"][pt.id].items():
            for k, v in r["forms"].items():
                if v:
                    ran[k][pt.id] = v
    for k in names:
        print(f"{k:24s} {len(ran[k]):2d} points: " + ", ".join(f"{p}={v}" for p, v in list(ran[k].items())[:4]))
    missing = [k for k in names if not ran[k] and k not in EXCEPTIONS and k not in DEAD]
    assert not missing, f"forms no sweep point launched: {missing}"
    for k in DEAD:
        assert not ran[k], f"{k} was believed unreachable ({DEAD[k]}) and ran at {ran[k]}: take it off the list"
    # by name
    four = fu.FOUR_WAVE.id
    dflt = [p.id for p in fu.SWEEP if (p.map, p.kf, p.leaf) == (fu.FOUR_WAVE.map, fu.FOUR_WAVE.kf, 0) and not p.env][0]
    assert four in ran["k_potrf_panel4"] and ran["k_potrf_panel4.fronts"][four] > fu.K_SMALL_MIN, "the four-wave panel form ran at its point"
    assert dflt not in ran["k_potrf_panel4"] and dflt in ran["k_potrf_panel"], "and NOT at the default plan of the same map"
    assert [p for p in ran["k_potrf_panel4"] if p != four] == [], ran["k_potrf_panel4"]
    for w in (4, 8, 12, 16):
        assert ran[f"k_trsm_sub4<{w}>"], w
    assert ran["k_gemm_abt.tri"] and ran["k_gemm_abt_q.tri"] and ran["k_gemm_abt.tri_grid"] and ran["k_gemm_abt.rect"] and ran["k_gemm_abt_q.rect"]
    assert ran["k_bwd_front"] and ran["k_bwd_pipe"] and ran["k_bwd_pipe64"] and ran["k_bwd_tree"] and ran["k_bwd_tree64"]
    # every solve of a tree factors every front exactly once per panel it has columns in
    for pt in fu.SWEEP:
        s = fu.plan_shape(pt)
        panels = int(((s["own"] + 255) // 256).sum())
        for mu, r in shared["runs"][pt.id].items():
            assert r["forms"]["k_potrf_panel.fronts"] + r["forms"]["k_potrf_panel4.fronts"] == panels, (pt.id, panels, _fmt(r["forms"]))


@pytest.mark.parametrize("pt", fu.REPEAT, ids=[p.id for p in fu.REPEAT])
def test_context_with_history_equals_fresh_context(shared, pt):
    """test_solves_are_bit_reproducible_across_contexts states the property for two fresh contexts; here one of them has solved other plans before
    (and after: the whole sweep runs first): the plan cached per context, the live-tile lists cached per level and the border tiles that are stored
    rather than cleared must leave no trace."""
    old = _run_through(shared, fu.SWEEP[-1]) and shared["runs"][pt.id]
    c = backend.Context(0)
    try:
        for mu in pt.mus:
            new = _step(c, pt, mu)
            assert new["cost"] == old[mu]["cost"]
            assert np.array_equal(new["dx"], old[mu]["dx"]) and np.array_equal(new["dl"], old[mu]["dl"]), (pt.id, mu, np.abs(new["dx"] - old[mu]["dx"]).max())
            assert new["forms"] == old[mu]["forms"]
    finally:
        c.close()


# ---- pose graph: covgpu_gn_step has no pose-graph form; one Levenberg-Marquardt iteration of the whole solve instead
PGO_MAPS = [("mh123", 200), ("mh12345", None)]
PGO_LEAVES = [6, 60, 384, 0]
PGO_POSE_CEILING = 1e-9     # the bound of test_pgo_block_arrow_solve_equals_dense_solve (there against the device's own dense solve)
_pgo = {}


def _pgo_problem(name, kf):
    if (name, kf) not in _pgo:
        cfg = synth.config_named(name)
        if kf:
            cfg.max_kf_per_agent = kf
        cfg.drift_trans = 0.05; cfg.drift_yaw_deg = 0.5
        p = mapdata.flatten_pgo(synth.make_map(cfg), {}, mapdata.PgoParams())[0]
        # the oracle against itself: the same iteration with its own dense Cholesky and with SuperLU (the LAPACK multifrontal port oracle/covo_mf.py
        # plans visual-inertial bundle adjustments only: it has no pose-graph form)
        o = covo.default_options(strategy=capi.COVGPU_LM, max_iterations=1)
        try:
            covo.use_sparse_solver(enable=False)
            qd, rd = covo.gba_solve(p, o, pgo=True)
            covo.use_sparse_solver(min_n=0)
            qs, rs = covo.gba_solve(p, o, pgo=True)
        finally:
            covo.use_sparse_solver(enable=False)
        assert rd.iterations == rs.iterations == 1 and rd.accepted_trace[0] == rs.accepted_trace[0]
        h_pose = float(np.abs(qd.kf_pose - qs.kf_pose).max())
        h_cost = abs(rd.cost_trace[0] - rs.cost_trace[0]) / abs(rs.cost_trace[0])
        _pgo[(name, kf)] = (p, qs, rs, h_pose, h_cost)
    return _pgo[(name, kf)]


@pytest.mark.parametrize("name,kf", PGO_MAPS, ids=[f"{n}{'@%d' % k if k else ''}" for n, k in PGO_MAPS])
def test_pose_graph_iteration_at_every_leaf_size(shared, name, kf, monkeypatch):
    """One Levenberg-Marquardt iteration of the pose-graph solve on its elimination tree at leaf sizes 6, 60, 384 and the default against the oracle
    (SuperLU): the same accept decision, the candidate cost and the poses within C times the oracle's own spread between its dense Cholesky and SuperLU
    (floors: 1e-13 m on poses — unit-scale positions carry 1e-16 — and 1e-14 relative on the cost), and never above the 1e-9 of the default-leaf test."""
    p, ref, rres, h_pose, h_cost = _pgo_problem(name, kf)
    g = backend.default_options(strategy=capi.COVGPU_LM, max_iterations=1)
    ctx = shared["ctx"]
    seen = set()
    for leaf in PGO_LEAVES:
        if leaf:
            monkeypatch.setenv("COVGPU_ND_LEAF", str(leaf))
        else:
            monkeypatch.delenv("COVGPU_ND_LEAF", raising=False)
        sol, res = ctx.pgo_solve(p, g)
        forms, lay = ctx.kernel_forms(), ctx.layout()
        dpose = float(np.abs(sol.kf_pose - ref.kf_pose).max())
        dcost = abs(res.cost_trace[0] - rres.cost_trace[0]) / abs(rres.cost_trace[0])
        print(f"pgo {name}{'@%d' % kf if kf else ''} leaf {leaf or 'default'}: K={p.K} E={p.E} fronts={lay['nd_fronts']} levels={lay['nd_levels']} oracle spread poses {h_pose:.2e} cost {h_cost:.2e} | "
              f"device poses {dpose:.2e} ({dpose / max(h_pose, 1e-13):.2f} h) cost {dcost:.2e} | {_fmt(forms)}")
        msg = f"leaf {leaf}: {_fmt(forms)}"
        assert res.iterations == rres.iterations == 1 and res.accepted_trace[0] == rres.accepted_trace[0], msg
        assert abs(res.initial_cost - rres.initial_cost) <= 1e-10 * rres.initial_cost, msg
        assert dcost <= C_BOUND * max(h_cost, 1e-14), (dcost, h_cost, msg)
        assert dpose <= min(C_BOUND * max(h_pose, 1e-13), PGO_POSE_CEILING), (dpose, h_pose, msg)
        assert lay["nd_fronts"] >= 1 and forms["pgo_arrow"] == forms["pgo_dense"] == 0 and forms["k_potrf_panel"] > 0, msg
        seen.add((lay["nd_fronts"], lay["nd_levels"]))
    assert len(seen) >= 3, f"the leaf sizes gave the same tree: {seen}"
