"""The host half of the trust-region tail's tests (tests/tail_util.py): the Python restatement of the step logic reproduces the oracle's own
solve, every point of the table has the property it is named for, every row of the logic table takes the branch it names. No GPU.
tests/test_gpu_tail.py holds the device to the same restatement and references."""
import math

import numpy as np
import pytest

from covins_amd import backend, capi
from oracle import covo
from tests import tail_util as tu

T, S = capi.TR, capi.SC


def _opts(**kw):
    return covo.default_options(**kw)


def _rejected_lm_input():
    """The input of tests/test_gpu_parity.py::test_rejected_lm_steps_follow_the_oracle."""
    from scipy.spatial.transform import Rotation as R
    rng = np.random.default_rng(5)
    q = tu.tiny_problem().copy()
    for k in range(q.K):
        if q.kf_fixed[k]:
            continue
        q.kf_pose[k, :4] = (R.from_quat(q.kf_pose[k, :4]) * R.from_rotvec(rng.normal(0, 0.6, 3))).as_quat()
        q.kf_pose[k, 4:] += rng.normal(0, 1.2, 3)
    return q


def _same_solve(p, o):
    ref, rres = covo.gba_solve(p, o)
    mine = tu.oracle_loop(p, o)
    n = rres.iterations
    assert mine["iterations"] == n and mine["termination"] == rres.termination
    assert mine["accepted"] == list(rres.accepted_trace[:n]) and sum(mine["accepted"]) == rres.accepted
    assert np.allclose(mine["cost"], np.array(rres.cost_trace[:n]), rtol=1e-9, atol=0.0)
    assert np.allclose(mine["radius"], np.array(rres.radius_trace[:n]), rtol=1e-9, atol=0.0)
    assert abs(mine["rows"][0][T["INITCOST"]] - rres.initial_cost) <= 1e-9 * rres.initial_cost
    return mine


@pytest.mark.parametrize("strategy", [capi.COVGPU_DOGLEG, capi.COVGPU_LM], ids=["dogleg", "lm"])
@pytest.mark.parametrize("r0", [0.1, 10.0, 1e4])
def test_restated_step_reproduces_the_oracles_solve(strategy, r0):
    """step() looped over covo.step, covo.tail_ref and covo.cost == covo.gba_solve: iterations, termination, accepted / cost / radius traces to 1e-9.
    The oracle evaluates g.step, step^T H step and |step| on the step it takes; the restatement forms them from the six products of (c, n)."""
    mine = _same_solve(tu.tiny_problem(), _opts(strategy=strategy, initial_radius=r0, max_iterations=8))
    if strategy == capi.COVGPU_DOGLEG and r0 == 0.1:
        assert mine["regimes"][0] != "gn" and mine["radius"][0] == 3.0 * r0   # (radius-limited and good: tripled)


def test_restated_step_reproduces_the_rejected_lm_steps():
    mine = _same_solve(_rejected_lm_input(), _opts(strategy=capi.COVGPU_LM, max_iterations=6))
    assert mine["accepted"][:3] == [0, 0, 1]
    assert any("lm_reject" in h for h in mine["hits"]) and any("lm_accept" in h for h in mine["hits"])


# ------------------------------------------------------------------------------------------------ the points
def _point_opts(pt, **kw):
    return _opts(**dict(pt.opt, **kw))


def test_dogleg_ladder_reaches_all_three_regimes_on_the_oracle():
    pt = tu.POINT["tiny-dogleg-ladder"]
    seen, rhos = {}, []
    for run in pt.runs:
        out = tu.oracle_loop(pt.build(), _point_opts(pt, **run.kw))
        assert out["iterations"] == 1 and out["termination"] == 0
        seen.setdefault(out["regimes"][0], []).append(run.kw["initial_radius"])
        rhos.append(out["rho"][0])
        # both beta branches are the restatement's; the oracle's inputs take the one with c > 0 (Cauchy-Schwarz: (c^T H n)^2 <= (c^T H c)(n^T H n))
        if out["regimes"][0] == "interp":
            assert "beta_c_positive" in out["hits"][0]
    assert set(seen) == {"gn", "cauchy", "interp"}, seen
    assert len(seen["interp"]) >= 2 and len(seen["cauchy"]) >= 2
    # no rho of the ladder within 1e-6 of a threshold it is compared with
    for rho in rhos:
        assert all(abs(rho - th) > 1e-6 for th in (1e-3, 0.25, 0.75)), rho


def test_reuse_ladder_halves_the_radius_at_a_fixed_state():
    pt = tu.POINT["tiny-dogleg-reuse"]
    out = tu.oracle_loop(pt.build(), _point_opts(pt, **pt.runs[-1].kw))
    n = tu.REUSE_ITERATIONS[-1]
    assert out["iterations"] == n and out["termination"] == 0 and out["accepted"] == [0] * n
    assert out["radius"] == [64.0 * 0.5 ** (i + 1) for i in range(n)]
    assert all("rederived" in h for h in out["hits"][1:]) and "rederived" not in out["hits"][0]
    assert set(out["regimes"]) == {"cauchy"}
    ref, rres = covo.gba_solve(pt.build(), _point_opts(pt, **pt.runs[-1].kw))
    assert list(rres.radius_trace[:n]) == out["radius"] and rres.termination == 0
    assert np.array_equal(ref.kf_pose, pt.build().kf_pose)


def test_lm_chain_moves_the_radius_and_no_rho_sits_on_a_threshold():
    pt = tu.POINT["tiny-lm"]
    out = tu.oracle_loop(pt.build(), _point_opts(pt, max_iterations=tu.LM_ITERATIONS[-1]))
    assert out["iterations"] == tu.LM_ITERATIONS[-1] and out["termination"] == 0
    assert len(set(out["radius"])) == len(out["radius"])
    for rho in out["rho"]:
        assert abs(rho - 1e-3) > 1e-6


def test_edge_points_have_the_edge_counts_and_segments_they_are_named_for():
    tiny = tu.tiny_problem()
    assert (tiny.I, tiny.E) == (26, 1) and tiny.I % 4 != 0          # dead IMU waves in the last workgroup of the segment
    for E in (0, 64, 65, 257):
        p = tu.POINT[f"tiny-E{E}"].build()
        assert p.E == E and p.I == 26 and p.O == tiny.O
        pairs = {(min(a, b), max(a, b)) for a, b in zip(p.edge_i.tolist(), p.edge_j.tolist())}
        assert len(pairs) == E
        if E:
            assert np.array_equal(p.edge_meas[0], tiny.edge_meas[0])
            # the added measurements disagree with the current poses: a non-zero residual
            r, _, c = covo.linearize_between(p, _opts())
            assert (np.abs(r).max(axis=1) > 1e-4).all() and (c > 0).all()
    vo = tu.POINT["tiny-vo-E65"]
    assert vo.build().E == 65 and vo.opt["visual_only"] == 1
    pg = tu.POINT["small-pose-graph"].build()
    assert pg.K == 180 and pg.E > 256 and tu.POINT["small-pose-graph"].pgo
    om = tu.POINT["omni"].build()
    assert tu.is_omni(om) and om.E == 0 and om.kf_fixed.sum() == 2 * om.A


def test_restated_reference_equals_the_oracles_on_a_pinhole_problem():
    """tu.reference's per-observation restatement (the omni point's reference) against covo.tail_ref where both apply."""
    p = tu.omni_problem().copy()
    d = dict(p.__dict__); d.pop("cam_model", None); d.pop("cam_xi", None)
    p = capi.FlatProblem(**d)
    o = _opts(visual_only=1)
    D, n, N = tu.dims(p, o)
    rng = np.random.default_rng(3)
    va, vb = rng.normal(size=N), rng.normal(size=N)
    g0, d0, dbl0, ldbl0 = covo.tail_ref(p, o, va, vb)
    g1, d1, dbl1 = tu._restated_sums(p, o, va, vb, np.longdouble)
    assert np.abs(g1 - g0).max() <= 1e-11 * np.abs(g0).max() and np.abs(d1 - d0).max() <= 1e-11 * np.abs(d0).max()
    for k_ in covo.TAIL_REF_KEYS:
        scale = {"aHb": math.sqrt(ldbl0["aHa"] * ldbl0["bHb"]), "a_b": math.sqrt(ldbl0["a_a"] * ldbl0["b_b"])}.get(k_, abs(ldbl0[k_]))
        assert abs(dbl1[k_] - ldbl0[k_]) <= 1e-11 * scale, (k_, dbl1[k_], ldbl0[k_])


def test_tail_ref_is_the_solvers_own_arithmetic():
    """covo.tail_ref's double row is what the solve loop computes: the quadratic form of quad_form, x_norm, the cost; its long double row differs by
    rounding only; the bilinear form is symmetric and consistent with the quadratic one."""
    p, o = tu.tiny_problem(), _opts()
    D, n, N = tu.dims(p, o)
    rng = np.random.default_rng(1)
    va, vb = rng.normal(size=N), rng.normal(size=N)
    ref = tu.reference(p, o, va, vb)
    assert ref["dbl"]["cost"] == covo.cost(p, o)
    for k_, h in ref["h"].items():
        scale = {"aHb": math.sqrt(ref["ldbl"]["aHa"] * ref["ldbl"]["bHb"]), "a_b": math.sqrt(ref["ldbl"]["a_a"] * ref["ldbl"]["b_b"])}.get(k_, abs(ref["ldbl"][k_]))
        assert h <= 1e-13 * scale, (k_, h, scale)
    swapped = tu.reference(p, o, vb, va)
    assert abs(swapped["ldbl"]["aHb"] - ref["ldbl"]["aHb"]) <= 1e-13 * math.sqrt(ref["ldbl"]["aHa"] * ref["ldbl"]["bHb"])
    assert swapped["ldbl"]["aHa"] == ref["ldbl"]["bHb"]
    both = tu.reference(p, o, va + vb, va)
    assert abs(both["ldbl"]["aHa"] - (ref["ldbl"]["aHa"] + 2 * ref["ldbl"]["aHb"] + ref["ldbl"]["bHb"])) <= 1e-12 * (ref["ldbl"]["aHa"] + ref["ldbl"]["bHb"])
    # g and d are the solver's: the Gauss-Newton step solves (H + mu D^2) n = -g, so g.n = -n^T (H + mu D^2) n
    mu = 1e-4
    dp, dl = covo.step(p, o, mu, dense=True)
    nvec = np.concatenate([dp, dl.reshape(-1)])
    r2 = tu.reference(p, o, nvec, nvec)
    damp = mu * math.fsum(((r2["d"] * nvec) ** 2).tolist())
    assert abs(r2["ldbl"]["g_a"] + r2["ldbl"]["aHa"] + damp) <= 1e-9 * r2["ldbl"]["aHa"]
    fixed = np.nonzero(p.kf_fixed)[0]
    assert len(fixed) and all(not r2["g"][15 * i:15 * i + 6].any() and (r2["d"][15 * i:15 * i + 6] == 1e-6).all() for i in fixed)


# ------------------------------------------------------------------------------------------------ the logic table
@pytest.mark.parametrize("row", tu.LOGIC_ROWS, ids=[r.id for r in tu.LOGIC_ROWS])
def test_every_logic_row_takes_the_branch_it_names(row):
    t, hits = tu.row_expected(row)
    for b in row.branches:
        assert b in hits, (row.id, b, hits)
    assert np.isfinite(t[[T[f] for f in tu.LOGIC_FIELDS + tu.FLAG_FIELDS]]).all()


def test_logic_table_covers_every_branch_of_the_restatement():
    named = {b for row in tu.LOGIC_ROWS for b in row.branches}
    want = {"first", "retry", "not_ok_no_retry", "term3", "rederived", "dogleg_gn", "dogleg_cauchy", "dogleg_interp", "beta_c_nonpositive",
            "beta_c_positive", "a_returns_on_term", "model_not_positive", "term2", "b_returns_on_retry", "b_returns_on_term", "invalid_lm",
            "invalid_dogleg", "term4", "lm_accept", "lm_accept_clamped", "rho_below_quarter", "rho_above_three_quarters", "rho_between", "lm_reject",
            "dogleg_reject", "term1"}
    assert named == want, (named ^ want)
    ids = [r.id for r in tu.LOGIC_ROWS]
    assert len(set(ids)) == len(ids)
    # the values the rows are built around
    t, _ = tu.row_expected(tu.LOGIC_ROWS[0])
    assert (t[T["CG"]], t[T["CN"]], t[T["MODEL"]], t[T["RHO"]]) == (0.0, 1.0, 3.0, 0.5)
    t, _ = tu.row_expected(next(r for r in tu.LOGIC_ROWS if r.id == "dogleg-interp-c-positive"))
    assert (t[T["CG"]], t[T["CN"]], t[T["MODEL"]]) == (-0.25, 0.5, 2.5)
    t, _ = tu.row_expected(next(r for r in tu.LOGIC_ROWS if r.id == "lm-accept-max-radius"))
    assert t[T["RADIUS"]] == 12.0
    t, _ = tu.row_expected(next(r for r in tu.LOGIC_ROWS if r.id == "solve-failed-mu-tenth"))
    assert (t[T["MU"]], t[T["TERM"]], t[T["OK"]]) == (10.0, 4.0, 0.0)


def test_finish_sizes_straddle_every_loop_bound_of_the_finisher():
    """k_tail_finish: one pass of 4096 (four loads per thread), a remainder loop of 1024, a tree over 1024 threads."""
    s = tu.FINISH_SIZES
    assert 1 in s and {1023, 1024, 1025} <= set(s) and {4096, 4097} <= set(s) and 3073 in s and max(s) == 8192 + 7 + 5 + 8192
    for n in s:
        part = tu.finish_partials(n)
        assert part.shape == (capi.SC_COUNT, n) and (part > 0).any() and (part < 0).any() if n > 1 else True


def test_the_test_entry_points_reject_a_null_context():
    import ctypes as C
    lib = backend.lib()
    assert (capi.TR_COUNT, capi.SC_COUNT) == (32, 16) and len(capi.TR_NAMES) == 31 and len(capi.SC_NAMES) == 15
    calls = {"covgpu_solve_resident_traced": (None, None, None, 0, None), "covgpu_fetch_tail_state": (None,) * 7,
             "covgpu_tail_logic_probe": (None, 0, 1, 0, 0, 0, None, None, None, 0)}
    for name, args in calls.items():
        assert getattr(lib, name)(None, *args) == 1, name
        msg = lib.covgpu_last_error()
        assert b"NULL context" in msg and name.encode() in msg, (name, msg)


def test_wide_reuse_ladder_rederives_all_three_regimes():
    pt = tu.POINT["tiny-dogleg-reuse-wide"]
    n = tu.REUSE_WIDE_ITERATIONS[-1]
    out = tu.oracle_loop(pt.build(), _point_opts(pt, **pt.runs[-1].kw))
    assert out["iterations"] == n and out["termination"] == 0 and out["accepted"] == [0] * n
    assert out["radius"] == [2.0 ** (19 - i) for i in range(n)]
    assert set(out["regimes"][1:]) == {"gn", "interp", "cauchy"}, out["regimes"]
    # the last iteration of every run of the point (the one whose candidate the device test reads back): all three regimes
    assert {out["regimes"][m - 1] for m in tu.REUSE_WIDE_ITERATIONS} == {"gn", "interp", "cauchy"}, out["regimes"]
