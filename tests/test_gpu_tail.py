"""The trust-region tail on the device (csrc/k_tail.hip; its COVGPU_TAIL=0 predecessor in csrc/k_dense.hip) against the references and the restated
step logic of tests/tail_util.py, point by point and logged iteration by logged iteration.

What is compared (the field of k_tail.hip every assertion pins is listed in DESIGN.md 4.7):
  inputs      grad / hdiag (landmark part included) against the oracle's g and clamped d; vtmp == grad / clamp(hdiag)^2
  reductions  TR_GG .. TR_JC, TR_COST, TR_INITCOST against the reference evaluated on the DEVICE'S OWN vtmp and gn (the solve's conditioning does not
              enter); signed sums on their Cauchy-Schwarz scale
  logic       every logged round against tail_util.step() fed the device's own reduced scalars; flags exactly
  candidate   pose_c / sb_c / lm_c against covo_pose_plus / plain addition of cg c + cn n; TR_COSTNEW against covo.cost at that candidate
  exits       termination 3 / 2 / 1 placed just either side of the reference thresholds
  probe       the logic table and the finisher's sizes through covgpu_tail_logic_probe: k_tail_logic, the ticketed k_tail_finish, the legacy trio
  legacy      the tiny ladders under COVGPU_TAIL=0 in a child process, the fields that form fills

Bounds (_MEASURED below holds every figure). For every compared quantity r = |device - reference(long double)| / scale was measured on one MI355X
beside the oracle's own h / scale (its double against its long double evaluation of the same sum); the bound is the smallest power of ten that leaves
a factor 3 over the worst r, not below 1e-15 (4.5 ulp: what a double sum can be asked for) and never above 1e-9. scale = |reference|, for the signed
sums GDOT, VG, JC the Cauchy-Schwarz product sqrt(GG GN2), sqrt(VV NN), sqrt(JA JB), for grad max|g|, for MODEL |g.step| + |J step|^2 / 2.
Most reductions sit at 1e-15 .. 1e-14. Three stand out, all on tiny-lm at its fifth and sixth iteration, none of them the tail's doing:
  JB     5.2e-11 against n^T H n — whose double evaluation is itself 2.8e-11 off its long double one: the oracle forms it through the ASSEMBLED H,
         where the whitened IMU blocks (entries 1e4 times the sum) cancel; the device sums |J n|^2 per residual and cancels nothing. MODEL (8.3e-12)
         is the same number seen through -(g.n + JB / 2).
  grad   2.1e-10 of max|g|: J^T r of the whitened IMU factors (chol(P)^-1 amplifies rounding by 1e4: tests/test_gpu_parity.py holds those blocks
         to 1e-8). GG (3.4e-13) is |g / d|^2 of that gradient against the oracle's.
A logic field against step() on the device's own scalars: LOGIC_TOL = 1e-12 (FMA contraction only; sqrt and division are correctly rounded).
"""
import math
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from covins_amd import backend, capi
from oracle import covo
from tests import tail_util as tu
from tests.helpers.tail_legacy import run_point

pytestmark = pytest.mark.gpu

T, S = capi.TR, capi.SC
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "tail_legacy.py")

# quantity: (bound, worst ratio observed on one MI355X, the oracle's own worst h / scale there; 0: the reference is an exactly rounded sum)
_MEASURED = {
    "GG": (1e-11, 3.4e-13, 0.0), "GN2": (1e-14, 1.7e-15, 0.0), "GDOT": (1e-14, 4.6e-16, 3.1e-15), "VV": (1e-15, 2.5e-16, 6.7e-15),
    "VG": (1e-15, 1.6e-17, 2.3e-14), "NN": (1e-15, 2.0e-16, 2.4e-14), "XN2": (1e-14, 3.5e-16, 4.8e-16), "JA": (1e-14, 1.2e-15, 4.0e-15),
    "JB": (1e-9, 5.2e-11, 2.8e-11), "JC": (1e-14, 5.5e-16, 9.3e-16), "COST": (1e-11, 9.6e-13, 2.4e-13), "INITCOST": (1e-13, 1.3e-14, 0.0),
    "COSTNEW": (1e-13, 3.2e-14, 0.0), "MODEL": (1e-10, 8.3e-12, 0.0), "SN": (1e-15, 3.0e-16, 0.0), "grad": (1e-9, 2.1e-10, 0.0),
    "hdiag": (1e-12, 5.4e-14, 0.0), "candidate": (1e-15, 2.2e-16, 0.0),
    "legacy GG": (1e-11, 3.4e-13, 0.0), "legacy GN2": (1e-14, 1.7e-15, 0.0), "legacy GDOT": (1e-14, 4.6e-16, 1.4e-15),
    "legacy ALPHA": (1e-14, 8.4e-16, 0.0), "legacy COST": (1e-11, 9.6e-13, 1.7e-15), "legacy INITCOST": (1e-14, 1.8e-15, 0.0),
    "legacy COSTNEW": (1e-13, 7.2e-15, 0.0), "legacy MODEL": (1e-10, 8.3e-12, 0.0), "legacy SN": (1e-15, 3.0e-16, 0.0),
    "legacy grad": (1e-9, 2.1e-10, 0.0), "legacy hdiag": (1e-13, 1.3e-14, 0.0), "legacy candidate": (1e-15, 9.9e-17, 0.0),
}
BOUNDS = {name: v[0] for name, v in _MEASURED.items()}
assert all(3.0 * v[1] <= v[0] <= 1e-9 for v in _MEASURED.values())
LOGIC_TOL = 1e-12      # a logic field against step() on the device's own scalars: FMA contraction only (sqrt and division are correctly rounded)
CS_SCALE = {"GDOT": ("GG", "GN2"), "VG": ("VV", "NN"), "JC": ("JA", "JB")}
_worst = {}


def _held(name, ratio, where, h=0.0, fused=True):
    """Record the ratio and hold it to the bound of its quantity (the legacy form has bounds of its own)."""
    name = name if fused else "legacy " + name
    w = _worst.setdefault(name, [0.0, 0.0, ""])
    if ratio > w[0]:
        w[0], w[2] = ratio, where
    w[1] = max(w[1], h)
    assert ratio <= BOUNDS[name], (where, name, ratio, BOUNDS[name])


@pytest.fixture(scope="module")
def ctx():
    c = backend.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module", autouse=True)
def report():
    """The figures behind BOUNDS (pytest -s shows them): the worst ratio of every compared quantity and the oracle's own h / scale beside it."""
    yield
    for name in sorted(_worst):
        print(f"tail worst {name:16s} ratio {_worst[name][0]:.3e}  oracle h/scale {_worst[name][1]:.3e}  at {_worst[name][2]}")


def _close(a, b, tol, scale=None):
    scale = max(abs(b), 1e-300) if scale is None else scale
    return abs(a - b) <= tol * scale


def _check_logic(pt, rec, gmax, fused=True):
    """Every logged round against the restatement on the device's own scalars."""
    o = covo.default_options(**rec["kw"]); k = tu.consts(o)
    prev = tu.initial_tr(o)
    for i, row in enumerate(rec["trace"]):
        where = f"{pt.id} {rec['kw']} round {i}"
        fresh = prev[T["REUSE"]] == 0.0
        assert row[T["OK"]] == 1.0, where                       # (no named point has an indefinite system)
        if fused:
            sc = np.zeros(capi.SC_COUNT)
            for f in tu.SUM_FIELDS:
                sc[S[f]] = row[T[f]]
            sc[S["COST"]] = row[T["INITCOST"]]; sc[S["GMAX"]] = gmax
            exp = tu.step(prev, sc, k, 0, fresh, cost_new=row[T["COSTNEW"]])
            if not fresh:
                for f in tu.SUM_FIELDS + ("ALPHA",):                # a re-derived step reads the STORED dot products
                    assert row[T[f]] == prev[T[f]], (where, f)
            fields = tu.LOGIC_FIELDS
        else:
            # legacy form: MODEL and SN come from kernels that reduce the combined step; stage A's coefficients from its own GG, GN2, GDOT, ALPHA
            a = np.array(prev)
            for f in ("GG", "GN2", "GDOT", "ALPHA"):
                a[T[f]] = row[T[f]]
            sc = np.zeros(capi.SC_COUNT); sc[S["GMAX"]] = gmax; sc[S["COST"]] = row[T["INITCOST"]]
            a = tu.step_a(a, sc, k, 0, False)
            if fresh and prev[T["FIRST"]] != 0.0:
                a[T["COST"]] = a[T["INITCOST"]] = row[T["INITCOST"]]; a[T["FIRST"]] = 0.0
            for f in ("CG", "CN", "DNORM"):
                assert _close(row[T[f]], a[T[f]], LOGIC_TOL), (where, f, row[T[f]], a[T[f]])
            for f in ("MODEL", "SN"):
                a[T[f]] = row[T[f]]
            a[T["VALID"]] = 1.0 if row[T["MODEL"]] > 0.0 else 0.0
            a[T["OK"]] = 1.0; a[T["TERM"]] = 0.0               # (stage A above saw no step norm: its parameter-tolerance exit is not the device's)
            sc[S["COST"]] = row[T["COSTNEW"]]
            exp = tu.step_b(a, sc, k)
            fields = ("RHO", "RADIUS", "MU", "LMDF")
        for f in fields:
            assert _close(row[T[f]], exp[T[f]], LOGIC_TOL), (where, f, row[T[f]], exp[T[f]])
        for f in tu.FLAG_FIELDS + ("FIRST",):
            assert row[T[f]] == exp[T[f]], (where, f, row[T[f]], exp[T[f]])
        for f in ("COST", "INITCOST"):
            assert row[T[f]] == exp[T[f]], (where, f)
        prev = row


def _check_record(pt, p0, rec, before, fused=True):
    """The last logged iteration of a run, whose vectors and candidate the device still holds, at the state `before` it was computed at."""
    o = covo.default_options(**rec["kw"]); k = tu.consts(o)
    D, n, N = tu.dims(p0, o, pt.pgo)
    ts, row = rec["ts"], rec["trace"][-1]
    dog = k["strategy"] == tu.DOGLEG
    where = f"{pt.id} {rec['kw']}"
    assert row[T["RETRY"]] == 0.0 and row[T["TERM"]] == 0.0, where
    have_c = fused or dog                                          # (the legacy form forms c = g / d^2 for the dogleg only)
    va = ts["vtmp"] if have_c else np.zeros(N)
    with covo.preintegrated_at(p0):
        ref = tu.reference(before, o, va, ts["gn"], pgo=pt.pgo)
        cost0 = tu.cost_at(p0, o, pgo=pt.pgo)
    g, d = ref["g"], ref["d"]
    # ---- inputs
    r = float(np.abs(ts["grad"] - g).max() / np.abs(g).max())
    _held("grad", r, where, fused=fused)
    dd = tu.clamp(ts["hdiag"])
    r = float((np.abs(dd - d) / d).max())
    _held("hdiag", r, where, fused=fused)
    if have_c:
        assert np.array_equal(ts["vtmp"], ts["grad"] / (dd * dd)), where
    lm_part = slice(n, N)
    if N > n:
        assert np.abs(ts["grad"][lm_part]).max() > 0 and np.abs(ts["hdiag"][lm_part]).min() > 0
    # ---- reductions, on the device's own vtmp and gn
    scr = tu.reference_scalars(ref, ts["gn"], "ldbl")
    hkey = dict(GDOT="g_b", VV="a_a", VG="a_b", NN="b_b", JA="aHa", JB="bHb", JC="aHb", XN2="xnorm")
    fields = tu.SUM_FIELDS if fused else ("GG", "GN2", "GDOT")
    for f in fields:
        if f in ("JA", "JC") and not dog:
            continue                                               # (Levenberg-Marquardt: one direction, k_tail_jvp<TWO = false>)
        want = scr[S[f]]
        scale = math.sqrt(scr[S[CS_SCALE[f][0]]] * scr[S[CS_SCALE[f][1]]]) if f in CS_SCALE else abs(want)
        r = abs(row[T[f]] - want) / scale
        h = ref["h"][hkey[f]] / (scale if f != "XN2" else math.sqrt(scale)) if f in hkey else 0.0
        _held(f, r, where, h, fused)
    r = abs(row[T["INITCOST"]] - cost0) / cost0
    _held("INITCOST", r, where, fused=fused)
    if not fused and dog:
        r = abs(row[T["ALPHA"]] - scr[S["GG"]] / scr[S["JA"]]) / (scr[S["GG"]] / scr[S["JA"]])
        _held("ALPHA", r, where, fused=fused)
    # ---- model and step norm of the step the device took, from the reference's products (the identity |J step|^2 = cg^2 JA + 2 cg cn JC + cn^2 JB)
    cg, cn = row[T["CG"]], row[T["CN"]]
    gs = cg * scr[S["GG"]] + cn * scr[S["GDOT"]]
    jv2 = cg * cg * scr[S["JA"]] + 2 * cg * cn * scr[S["JC"]] + cn * cn * scr[S["JB"]]
    sn2 = cg * cg * scr[S["VV"]] + 2 * cg * cn * scr[S["VG"]] + cn * cn * scr[S["NN"]]
    r = abs(row[T["MODEL"]] + (gs + 0.5 * jv2)) / (abs(gs) + 0.5 * jv2)
    _held("MODEL", r, where, fused=fused)
    r = abs(row[T["SN"]] - math.sqrt(sn2)) / math.sqrt(sn2)
    _held("SN", r, where, fused=fused)
    # ---- candidate
    assert row[T["VALID"]] == 1.0, where
    stepv = cn * ts["gn"] + (cg * va if cg != 0.0 else 0.0)
    cand = tu.apply_step(before, o, stepv, pgo=pt.pgo)
    fixed = before.kf_fixed != 0
    assert np.array_equal(ts["pose_c"][fixed], before.kf_pose[fixed]), where
    err = [np.abs(ts["pose_c"] - cand.kf_pose).max() / max(1.0, np.abs(cand.kf_pose).max())]
    if D == 15:
        err.append(np.abs(ts["sb_c"] - cand.kf_speed_bias).max() / max(1.0, np.abs(cand.kf_speed_bias).max()))
    if N > n:
        err.append(np.abs(ts["lm_c"] - cand.lm_pos).max() / max(1.0, np.abs(cand.lm_pos).max()))
    r = float(max(err))
    _held("candidate", r, where, fused=fused)
    dev_cand = tu.with_state(before, ts["pose_c"], ts["sb_c"] if D == 15 else None, ts["lm_c"] if N > n else None)
    with covo.preintegrated_at(p0):
        cnew = tu.cost_at(dev_cand, o, pgo=pt.pgo)
    r = abs(row[T["COSTNEW"]] - cnew) / cnew
    _held("COSTNEW", r, where, fused=fused)
    r = abs(row[T["COST"]] - (cnew if row[T["ACC"]] else ref["ldbl"]["cost"])) / cnew
    _held("COST", r, where, ref["h"]["cost"] / cnew, fused)
    # ---- accept: the estimate the solve left is the candidate, bit for bit, or the state before
    want = dev_cand if row[T["ACC"]] else before
    assert np.array_equal(rec["after"]["pose"], want.kf_pose), where
    if D == 15:
        assert np.array_equal(rec["after"]["sb"], want.kf_speed_bias), where
    if N > n:
        assert np.array_equal(rec["after"]["lm"], want.lm_pos), where
    # ---- the result the caller sees is the trace's
    res = rec["res"]
    rows = [t for t in rec["trace"] if t[T["RETRY"]] == 0.0]
    assert res["iterations"] == len(rows) and res["termination"] == int(row[T["TERM"]])
    assert res["cost_trace"] == [t[T["COST"]] for t in rows] and res["radius_trace"] == [t[T["RADIUS"]] for t in rows]
    assert res["accepted_trace"] == [int(t[T["ACC"]]) for t in rows] and res["initial_cost"] == row[T["INITCOST"]]
    return ref


def _check_point(pt, recs, fused=True):
    p0 = pt.build()
    before = p0
    regimes = []
    for run, rec in zip(pt.runs, recs):
        if not run.chain:
            before = p0
            assert all(t[T["ACC"]] == 0.0 for t in rec["trace"][:-1]), pt.id   # (the state before the last iteration is the uploaded one)
        ref = _check_record(pt, p0, rec, before, fused)
        _check_logic(pt, rec, ref["ldbl"]["gmax"], fused)
        regimes.append(tu.dogleg_regime(rec["trace"][-1]))
        if run.chain:
            before = tu.with_state(p0, rec["after"]["pose"], rec["after"]["sb"], rec["after"]["lm"] if p0.L and not pt.pgo else None)
    return regimes


@pytest.mark.parametrize("pt", tu.POINTS, ids=[p.id for p in tu.POINTS])
def test_point(ctx, pt):
    recs = run_point(ctx, pt)
    regimes = _check_point(pt, recs)
    if pt.runs is tu.TWO_RADII:
        assert regimes == ["gn", "interp"], regimes
    if pt.id == "tiny-dogleg-ladder":
        assert set(regimes) == {"gn", "interp", "cauchy"}
    if pt.id == "tiny-dogleg-reuse":
        n = tu.REUSE_ITERATIONS[-1]
        assert recs[-1]["res"]["radius_trace"] == [64.0 * 0.5 ** (i + 1) for i in range(n)] and recs[-1]["res"]["termination"] == 0
    if pt.id == "tiny-dogleg-reuse-wide":
        assert set(regimes) == {"gn", "interp", "cauchy"}, regimes
    if pt.id == "tiny-lm":
        assert len({rec["trace"][-1][T["RADIUS"]] for rec in recs}) == len(recs)


# ------------------------------------------------------------------------------------------------ exits
def test_exits_sit_where_the_reference_puts_them(ctx):
    p = tu.tiny_problem()
    base = dict(strategy=tu.DOGLEG, initial_radius=tu.GN_INSIDE_RADIUS, max_iterations=1)
    o = backend.default_options(**base)
    ctx.upload(p, o)
    res, trace = ctx.solve_resident_traced(o)
    ts = ctx.fetch_tail_state(o)
    ref = tu.reference(p, covo.default_options(**base), ts["vtmp"], ts["gn"])
    assert res.termination == 0 and res.iterations == 1 and tu.dogleg_regime(trace[-1]) == "gn"
    # gradient tolerance: the atomic max over the bit patterns of |g|
    gmax = ref["ldbl"]["gmax"]
    res, trace = ctx.solve_resident_traced(backend.default_options(**dict(base, gradient_tolerance=gmax * (1 + 1e-9))))
    assert (res.termination, res.iterations, len(trace)) == (3, 0, 1) and trace[0][T["TERM"]] == 3.0
    res, trace = ctx.solve_resident_traced(backend.default_options(**dict(base, gradient_tolerance=gmax * (1 - 1e-9))))
    assert res.termination == 0 and res.iterations == 1 and trace[0][T["TERM"]] == 0.0 and trace[0][T["ACC"]] == 1.0
    # ... cleared with every linearisation: the second iteration exits on the max of ITS state, which is below the first's
    p1 = ctx.download()
    with covo.preintegrated_at(p):
        gmax1 = tu.reference(p1, covo.default_options(**base), np.zeros_like(ts["gn"]), np.zeros_like(ts["gn"]))["ldbl"]["gmax"]
    assert gmax1 < 0.5 * gmax
    res, trace = ctx.solve_resident_traced(backend.default_options(**dict(base, gradient_tolerance=gmax1 * (1 + 1e-9), max_iterations=2)))
    assert (res.termination, res.iterations, len(trace)) == (3, 1, 2) and trace[1][T["TERM"]] == 3.0
    res, trace = ctx.solve_resident_traced(backend.default_options(**dict(base, gradient_tolerance=gmax1 * (1 - 1e-9), max_iterations=2)))
    assert res.iterations == 2 and all(t[T["TERM"]] != 3.0 for t in trace)
    # parameter tolerance: sn <= tol (|x| + tol) at the reference |n| (the Gauss-Newton step is the step) and |x|
    sn, xn = math.sqrt(ref["ldbl"]["b_b"]), ref["ldbl"]["xnorm"]
    tol = sn / xn
    for _ in range(50):
        tol = sn / (xn + tol)
    res, trace = ctx.solve_resident_traced(backend.default_options(**dict(base, parameter_tolerance=tol * (1 + 1e-9))))
    assert (res.termination, res.iterations) == (2, 0) and trace[0][T["TERM"]] == 2.0 and trace[0][T["VALID"]] == 1.0
    res, trace = ctx.solve_resident_traced(backend.default_options(**dict(base, parameter_tolerance=tol * (1 - 1e-9))))
    assert (res.termination, res.iterations) == (0, 1) and trace[0][T["TERM"]] == 0.0
    # function tolerance 1: any accepted step converges
    res, trace = ctx.solve_resident_traced(backend.default_options(**dict(base, function_tolerance=1.0, max_iterations=5)))
    assert (res.termination, res.iterations, res.accepted) == (1, 1, 1) and trace[0][T["FNCONV"]] == 1.0 and trace[0][T["ACC"]] == 1.0


# ------------------------------------------------------------------------------------------------ the probe
def _row_options(row):
    return backend.default_options(**{k_: v for k_, v in row.k.items()})


def _same_state(got, exp, where, tol=LOGIC_TOL):
    for f in capi.TR_NAMES:
        a, b = got[T[f]], exp[T[f]]
        if f in tu.FLAG_FIELDS + ("FIRST",):
            assert a == b, (where, f, a, b)
        else:
            assert (np.isnan(a) and np.isnan(b)) or _close(a, b, tol), (where, f, a, b)


def _partials_summing_to(sc, part_n, seed):
    """part[SC_COUNT][part_n] whose rows sum to about sc: the value itself and cancelling pairs of mixed sign."""
    rng = np.random.default_rng(seed)
    part = np.zeros((capi.SC_COUNT, part_n))
    x = rng.integers(-50, 51, size=(capi.SC_COUNT, (part_n - 1) // 2)).astype(np.float64)   # (dyadic row values sum exactly in any order)
    part[:, 1:1 + x.shape[1]] = x; part[:, 1 + x.shape[1]:1 + 2 * x.shape[1]] = -x
    part[:, 0] = sc
    return part


@pytest.mark.parametrize("row", tu.LOGIC_ROWS, ids=[r.id for r in tu.LOGIC_ROWS])
def test_logic_row_through_every_form(ctx, row):
    o = _row_options(row)
    exp, _ = tu.row_expected(row)
    cost_sc = np.array(row.sc); cost_sc[S["COST"]] = row.cost_new
    # ---- k_tail_logic: stage A, stage B
    t = row.tr
    if "A" in row.stages:
        t, _ = ctx.tail_logic_probe(o, capi.TAIL_LOGIC, t, row.sc, flag0=row.flag0, stage=1, fresh=row.fresh)
    if "B" in row.stages:
        t, _ = ctx.tail_logic_probe(o, capi.TAIL_LOGIC, t, cost_sc, flag0=row.flag0, stage=2)
    _same_state(t, exp, (row.id, "k_tail_logic"))
    # ---- k_tail_finish: the sums of the partials, then the logic in the workgroup that draws the last ticket (a re-derived step has no stage-1
    #      finisher in the product: its stage A stays k_tail_logic's)
    t, sc_dev = row.tr, np.array(row.sc)
    if "A" in row.stages:
        if row.fresh:
            part = _partials_summing_to(np.nan_to_num(row.sc), 37, seed=1)
            t, sc_dev = ctx.tail_logic_probe(o, capi.TAIL_FINISH, t, row.sc, flag0=row.flag0, stage=1, with_logic=True, fresh=True, part=part)
            two = row.k["strategy"] == tu.DOGLEG
            for f in tu.SUM_FIELDS:
                if f in ("JA", "JC") and not two:
                    assert sc_dev[S[f]] == row.sc[S[f]]                # (not this strategy's slots: untouched)
                else:
                    assert abs(sc_dev[S[f]] - math.fsum(part[S[f]].tolist())) <= tu.finish_bound(37, np.abs(part[S[f]]).sum()), (row.id, f)
            assert sc_dev[S["COST"]] == row.sc[S["COST"]] and sc_dev[S["GMAX"]] == row.sc[S["GMAX"]]
        else:
            t, _ = ctx.tail_logic_probe(o, capi.TAIL_LOGIC, t, row.sc, flag0=row.flag0, stage=1, fresh=False)
    if "B" in row.stages:
        part = _partials_summing_to(cost_sc, 37, seed=2)
        t, sc2 = ctx.tail_logic_probe(o, capi.TAIL_FINISH, t, np.nan_to_num(sc_dev), flag0=row.flag0, stage=2, with_logic=True, part=part)
        assert abs(sc2[S["COST"]] - row.cost_new) <= tu.finish_bound(37, np.abs(part[S["COST"]]).sum())
    hits = []
    e2 = row.tr
    if "A" in row.stages:
        e2 = tu.step_a(e2, sc_dev if row.fresh else row.sc, row.k, row.flag0, row.fresh, hits)
    if "B" in row.stages:
        e2 = tu.step_b(e2, sc2, row.k, hits)
    _same_state(t, e2, (row.id, "k_tail_finish"))
    assert all(b in hits for b in row.branches), (row.id, hits)      # (the rounding of the sums moved no row off its branch)
    # ---- logic = 0: the sums alone, the state untouched
    t0, _ = ctx.tail_logic_probe(o, capi.TAIL_FINISH, row.tr, row.sc, flag0=row.flag0, stage=1, with_logic=False,
                                 part=_partials_summing_to(np.nan_to_num(row.sc), 37, seed=3))
    assert np.array_equal(t0, row.tr, equal_nan=True)
    # ---- the legacy trio: k_tr_after_solve, (the kernels between reduce the combined step: their sums from the row's products), k_tr_after_model,
    #      k_tr_decide
    t = row.tr
    if "A" in row.stages:
        sc = np.array(row.sc); sc[S["JV2"]] = row.sc[S["JA"]]
        src = row.sc if row.fresh else np.array([row.tr[T[f]] if f in T else 0.0 for f in capi.SC_NAMES] + [0.0])
        t, _ = ctx.tail_logic_probe(o, capi.TR_AFTER_SOLVE, t, sc, flag0=row.flag0, fresh=row.fresh)
        cg, cn = t[T["CG"]], t[T["CN"]]
        sc = np.array(sc)
        sc[S["GS"]] = cg * src[S["GG"]] + cn * src[S["GDOT"]]
        sc[S["JV2"]] = cg * cg * src[S["JA"]] + 2.0 * cg * cn * src[S["JC"]] + cn * cn * src[S["JB"]]
        sc[S["SN2"]] = max(cg * cg * src[S["VV"]] + 2.0 * cg * cn * src[S["VG"]] + cn * cn * src[S["NN"]], 0.0)
        sc[S["XN2"]] = src[S["XN2"]]
        t, _ = ctx.tail_logic_probe(o, capi.TR_AFTER_MODEL, t, sc, flag0=row.flag0)
    if "B" in row.stages:
        t, _ = ctx.tail_logic_probe(o, capi.TR_DECIDE, t, cost_sc, flag0=row.flag0)
    for f in tu.LOGIC_FIELDS + ("COST", "INITCOST", "COSTNEW", "GG", "GN2", "GDOT"):
        assert (np.isnan(t[T[f]]) and np.isnan(exp[T[f]])) or _close(t[T[f]], exp[T[f]], LOGIC_TOL), (row.id, "legacy", f, t[T[f]], exp[T[f]])
    for f in tu.FLAG_FIELDS + ("FIRST",):
        assert t[T[f]] == exp[T[f]], (row.id, "legacy", f, t[T[f]], exp[T[f]])


@pytest.mark.parametrize("part_n", tu.FINISH_SIZES)
def test_finish_sums_at_every_loop_bound(ctx, part_n):
    """k_tail_finish against math.fsum, both stages' slot lists, with and without the logic riding along."""
    part = tu.finish_partials(part_n)
    row = tu.LOGIC_ROWS[0]
    o = _row_options(row)
    stage1 = [S[f] for f in tu.SUM_FIELDS]
    for stage, with_logic, slots in ((1, False, stage1), (1, True, stage1), (2, False, [S["COST"]]), (2, True, [S["COST"]])):
        sc_in = np.full(capi.SC_COUNT, -7.0)
        _, sc = ctx.tail_logic_probe(o, capi.TAIL_FINISH, row.tr, sc_in, stage=stage, with_logic=with_logic, part=part)
        for s in range(capi.SC_COUNT):
            if s in slots:
                want = math.fsum(part[s].tolist())
                assert abs(sc[s] - want) <= tu.finish_bound(part_n, np.abs(part[s]).sum()), (part_n, stage, s, sc[s], want)
            else:
                assert sc[s] == -7.0, (part_n, stage, s)
    # the ticket counter is back at zero: a second launch on the same flags runs the logic again (the probe uploads fresh flags; here the state shows it)
    sc0 = np.array(row.sc)
    t, sc = ctx.tail_logic_probe(o, capi.TAIL_FINISH, row.tr, sc0, stage=1, with_logic=True, part=_partials_summing_to(row.sc, part_n, seed=4))
    exp = tu.step_a(row.tr, sc, row.k, 0, True)
    _same_state(t, exp, ("finish", part_n))


# ------------------------------------------------------------------------------------------------ the legacy form
def test_legacy_tail_fills_its_fields_to_the_same_references(tmp_path):
    out = str(tmp_path / "legacy.pkl")
    r = subprocess.run([sys.executable, WORKER, out], env=dict(os.environ, COVGPU_TAIL="0"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with open(out, "rb") as f:
        got = pickle.load(f)
    assert got["tail"] == "0"
    for name in tu.LEGACY_POINTS:
        regimes = _check_point(tu.POINT[name], got["records"][name], fused=False)
        if name == "tiny-dogleg-ladder":
            assert set(regimes) == {"gn", "interp", "cauchy"}
        # the form did run: the fused tail's stored products stay zero
        assert all(not rec["trace"][-1][[T[f] for f in ("JA", "JB", "JC", "VV", "VG", "NN")]].any() for rec in got["records"][name])
