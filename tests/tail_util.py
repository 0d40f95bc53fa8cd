"""The trust-region tail (csrc/k_tail.hip, and its COVGPU_TAIL=0 predecessor in csrc/k_dense.hip) without any GPU code: the reference numbers,
a Python restatement of one pass of the oracle's loop as the two stages the device runs it in, the table of points (problem + radius schedule)
and the table of prescribed logic rows. tests/test_tail_host.py checks these against the oracle's own solve; tests/test_gpu_tail.py holds the
device to them.

The trust-region state travels as the array the device keeps (capi.TR_NAMES, csrc/common.hpp TR_*), the reduced scalars as capi.SC_NAMES."""
import math
from collections import namedtuple

import numpy as np

from covins_amd import capi, mapdata, synth
from oracle import covo

T, S = capi.TR, capi.SC
DOGLEG, LM = capi.COVGPU_DOGLEG, capi.COVGPU_LM
EPS = 2.0 ** -52


# ------------------------------------------------------------------------------------------------ a) the restated step
def consts(o):
    """What the step logic reads of the options (TrConsts)."""
    return dict(strategy=int(o.strategy), max_radius=o.max_radius, min_relative_decrease=o.min_relative_decrease,
                function_tolerance=o.function_tolerance, parameter_tolerance=o.parameter_tolerance, gradient_tolerance=o.gradient_tolerance)


def initial_tr(o):
    """The state a solve starts from (solve_impl_dev)."""
    t = np.zeros(capi.TR_COUNT)
    t[T["RADIUS"]] = o.initial_radius; t[T["MU"]] = 1e-8; t[T["LMDF"]] = 2.0; t[T["FIRST"]] = 1.0; t[T["OK"]] = 1.0
    return t


def clamp(h):
    """Ceres' Jacobi scaling of a diagonal entry of J^T J: clamp(sqrt(h), 1e-6, 1e32)."""
    return np.minimum(np.maximum(np.sqrt(np.maximum(h, 0.0)), 1e-6), 1e32)


def dogleg_regime(t):
    """'gn' | 'cauchy' | 'interp' of a state whose stage A has run."""
    if t[T["CG"]] == 0.0:
        return "gn"
    return "cauchy" if t[T["CN"]] == 0.0 else "interp"


def step_a(tr, sc, k, flag0=0, fresh=True, hits=None):
    """Stage A: everything between the linear solve and the candidate — the verdict on the factorisation, the gradient-tolerance exit, the dogleg
    coefficients (cg, cn) of step = cg c + cn n, the model decrease and step norm from the dot products, the parameter-tolerance exit
    (covo_solver.cpp: the head of the loop down to apply_step). `hits` collects the names of the branches taken."""
    t = np.array(tr, dtype=np.float64)
    hit = (lambda name: hits.append(name)) if hits is not None else (lambda name: None)
    dog = k["strategy"] == DOGLEG
    for f in ("RETRY", "VALID", "ACC", "FNCONV", "MODEL", "SN"):
        t[T[f]] = 0.0
    if fresh:
        if t[T["FIRST"]] != 0.0:
            t[T["COST"]] = t[T["INITCOST"]] = sc[S["COST"]]; t[T["FIRST"]] = 0.0
            hit("first")
        ok = flag0 == 0
        t[T["OK"]] = 1.0 if ok else 0.0
        if not ok and dog and t[T["MU"]] * 10.0 < 1.0:
            t[T["MU"]] *= 10.0; t[T["RETRY"]] = 1.0
            hit("retry")
            return t
        if not ok and dog:
            t[T["MU"]] *= 10.0
            hit("not_ok_no_retry")
        if sc[S["GMAX"]] <= k["gradient_tolerance"]:
            t[T["TERM"]] = 3.0
            hit("term3")
            return t
        for f in ("GG", "GN2", "GDOT", "JA", "JB", "JC", "VV", "VG", "NN", "XN2"):
            t[T[f]] = sc[S[f]]
        if dog:
            t[T["ALPHA"]] = t[T["GG"]] / t[T["JA"]]
    else:
        hit("rederived")
    cg, cn = 0.0, 1.0
    if dog:
        radius, alpha, GG, GN2, GDOT = (t[T[f]] for f in ("RADIUS", "ALPHA", "GG", "GN2", "GDOT"))
        gn_norm, g_norm = math.sqrt(GN2), math.sqrt(GG)
        if gn_norm <= radius:
            cg, cn = 0.0, 1.0; t[T["DNORM"]] = gn_norm
            hit("dogleg_gn")
        elif g_norm * alpha >= radius:
            cg, cn = -radius / g_norm, 0.0; t[T["DNORM"]] = radius
            hit("dogleg_cauchy")
        else:
            b_dot_a, a_sq = -alpha * GDOT, alpha * alpha * GG
            bma, cc = GN2 - 2.0 * b_dot_a + a_sq, b_dot_a - a_sq
            dd = math.sqrt(cc * cc + bma * (radius * radius - a_sq))
            if cc <= 0.0:
                beta = (dd - cc) / bma
                hit("beta_c_nonpositive")
            else:
                beta = (radius * radius - a_sq) / (dd + cc)
                hit("beta_c_positive")
            cg, cn = -alpha * (1.0 - beta), beta; t[T["DNORM"]] = radius
            hit("dogleg_interp")
    t[T["CG"]] = cg; t[T["CN"]] = cn
    if t[T["TERM"]] != 0.0:
        hit("a_returns_on_term")
        return t
    ok = t[T["OK"]] != 0.0
    gs = cg * t[T["GG"]] + cn * t[T["GDOT"]]
    jv2 = cg * cg * t[T["JA"]] + 2.0 * cg * cn * t[T["JC"]] + cn * cn * t[T["JB"]]
    sn2 = cg * cg * t[T["VV"]] + 2.0 * cg * cn * t[T["VG"]] + cn * cn * t[T["NN"]]
    model = -(gs + 0.5 * jv2) if ok else 0.0
    sn = math.sqrt(max(sn2, 0.0)) if ok else 0.0
    t[T["MODEL"]] = model; t[T["SN"]] = sn
    valid = ok and model > 0.0
    t[T["VALID"]] = 1.0 if valid else 0.0
    if ok and not model > 0.0:
        hit("model_not_positive")
    if valid and sn <= k["parameter_tolerance"] * (math.sqrt(t[T["XN2"]]) + k["parameter_tolerance"]):
        t[T["TERM"]] = 2.0
        hit("term2")
    return t


def step_b(tr, sc, k, hits=None):
    """Stage B: the verdict on the candidate, whose cost is sc[COST] (covo_solver.cpp: from evaluate_cost(xn) to the end of the loop body)."""
    t = np.array(tr, dtype=np.float64)
    hit = (lambda name: hits.append(name)) if hits is not None else (lambda name: None)
    if t[T["RETRY"]] != 0.0:
        hit("b_returns_on_retry")
        return t
    if t[T["TERM"]] != 0.0:
        hit("b_returns_on_term")
        return t
    lm = k["strategy"] == LM
    acc = False
    if t[T["VALID"]] == 0.0:
        if lm:
            t[T["RADIUS"]] /= t[T["LMDF"]]; t[T["LMDF"]] *= 2.0
            hit("invalid_lm")
        else:
            t[T["MU"]] *= 10.0
            hit("invalid_dogleg")
        t[T["REUSE"]] = 0.0
        if t[T["MU"]] >= 1.0 and t[T["OK"]] == 0.0:
            t[T["TERM"]] = 4.0
            hit("term4")
    else:
        cost, cost_new = t[T["COST"]], sc[S["COST"]]
        rho = (cost - cost_new) / t[T["MODEL"]]
        t[T["RHO"]] = rho; t[T["COSTNEW"]] = cost_new
        acc = rho > k["min_relative_decrease"]
        if acc:
            t[T["FNCONV"]] = 1.0 if abs(cost - cost_new) <= k["function_tolerance"] * cost else 0.0
            t[T["COST"]] = cost_new
            if lm:
                u = 2.0 * rho - 1.0
                grown = t[T["RADIUS"]] / max(1.0 / 3.0, 1.0 - u * u * u)
                hit("lm_accept_clamped" if grown > k["max_radius"] else "lm_accept")
                t[T["RADIUS"]] = min(k["max_radius"], grown)
                t[T["LMDF"]] = 2.0
            else:
                if rho < 0.25:
                    t[T["RADIUS"]] *= 0.5
                    hit("rho_below_quarter")
                if rho > 0.75:
                    t[T["RADIUS"]] = max(t[T["RADIUS"]], 3.0 * t[T["DNORM"]])
                    hit("rho_above_three_quarters")
                if 0.25 <= rho <= 0.75:
                    hit("rho_between")
                t[T["MU"]] = max(1e-8, 2.0 * t[T["MU"]] / 10.0)
            t[T["REUSE"]] = 0.0
        elif lm:
            t[T["RADIUS"]] /= t[T["LMDF"]]; t[T["LMDF"]] *= 2.0; t[T["REUSE"]] = 0.0
            hit("lm_reject")
        else:
            t[T["RADIUS"]] *= 0.5; t[T["REUSE"]] = 1.0
            hit("dogleg_reject")
        if t[T["FNCONV"]] != 0.0:
            t[T["TERM"]] = 1.0
            hit("term1")
    t[T["ACC"]] = 1.0 if acc else 0.0
    return t


def step(tr, sc, k, flag0=0, fresh=True, cost_new=None, hits=None):
    """One pass of the loop: stage A on the scalars `sc`, stage B on the candidate's cost `cost_new` (the two stages share the COST slot on the
    device as well: the linearisation writes the cost of the state there, the tail the cost of the candidate)."""
    t = step_a(tr, sc, k, flag0, fresh, hits)
    s2 = np.array(sc, dtype=np.float64)
    if cost_new is not None:
        s2[S["COST"]] = cost_new
    return step_b(t, s2, k, hits)


LOGIC_FIELDS = ("ALPHA", "CG", "CN", "DNORM", "MODEL", "SN", "RHO", "RADIUS", "MU", "LMDF")
FLAG_FIELDS = ("OK", "VALID", "ACC", "REUSE", "RETRY", "FNCONV", "TERM")
SUM_FIELDS = ("GG", "GN2", "GDOT", "VV", "VG", "NN", "XN2", "JA", "JB", "JC")


# ------------------------------------------------------------------------------------------------ the reference
def is_omni(p):
    return p.cam_model is not None and bool(np.any(np.asarray(p.cam_model) != capi.COVGPU_CAM_PINHOLE))


def _restated_sums(p, o, va, vb, acc):
    """covo_tail_ref for a reprojection-only problem from the per-observation restatement of tests/test_omni_host.py (the oracle has no
    unified-camera model): sums accumulated in dtype `acc`."""
    from tests.test_omni_host import linearize_ref
    assert p.E == 0 and o.visual_only, "the restatement holds reprojection blocks only"
    r, Jp, Jl, c = linearize_ref(p, loss_a=o.reproj_loss_a)
    K, L = p.K, p.L
    n = 6 * K
    lm_of = np.repeat(np.arange(L), np.diff(p.lm_obs_ptr))
    kf = p.obs_kf
    Jp = Jp.reshape(-1, 2, 6).astype(acc); Jl = Jl.reshape(-1, 2, 3).astype(acc); r = r.astype(acc)
    g = np.zeros((K, 6), acc); gl = np.zeros((L, 3), acc); hp = np.zeros((K, 6), acc); hl = np.zeros((L, 3), acc)
    np.add.at(g, kf, np.einsum("oki,ok->oi", Jp, r)); np.add.at(gl, lm_of, np.einsum("oki,ok->oi", Jl, r))
    np.add.at(hp, kf, (Jp * Jp).sum(1)); np.add.at(hl, lm_of, (Jl * Jl).sum(1))
    gv = np.concatenate([g.reshape(-1), gl.reshape(-1)]); hv = np.concatenate([hp.reshape(-1), hl.reshape(-1)])

    def jv(v):
        v = np.asarray(v).astype(acc)
        return np.einsum("oki,oi->ok", Jp, v[:n].reshape(K, 6)[kf]) + np.einsum("oki,oi->ok", Jl, v[n:].reshape(L, 3)[lm_of])
    ja, jb = jv(va), jv(vb)
    a, b = np.asarray(va).astype(acc), np.asarray(vb).astype(acc)
    free = p.kf_fixed == 0
    xn = (p.kf_pose[free].astype(acc) ** 2).sum() + (p.lm_pos.astype(acc) ** 2).sum()
    sums = dict(cost=c.astype(acc).sum(), xnorm=np.sqrt(xn), gmax=np.abs(gv).max(), aHa=(ja * ja).sum(), bHb=(jb * jb).sum(), aHb=(ja * jb).sum(),
                g_a=(gv * a).sum(), g_b=(gv * b).sum(), a_a=(a * a).sum(), a_b=(a * b).sum(), b_b=(b * b).sum())
    return gv.astype(np.float64), clamp(hv.astype(np.float64)), {k_: float(v) for k_, v in sums.items()}


def reference(p, o, va, vb, pgo=False):
    """What the step logic reads at the state held in `p` for the two vectors va, vb [N]: dict(g, d (clamped), dbl = the sums in double,
    ldbl = the same sums accumulated in long double, h = |dbl - ldbl| per sum: the rounding scale of a double evaluation). Keys of the sums:
    covo.TAIL_REF_KEYS."""
    if is_omni(p):
        g, d, dbl = _restated_sums(p, o, va, vb, np.float64)
        _, _, ldbl = _restated_sums(p, o, va, vb, np.longdouble)
    else:
        g, d, dbl, ldbl = covo.tail_ref(p, o, va, vb, pgo=pgo)
    return dict(g=g, d=d, dbl=dbl, ldbl=ldbl, h={k_: abs(dbl[k_] - ldbl[k_]) for k_ in dbl})


def cost_at(p, o, pgo=False):
    """The objective at the state held in `p` (covo.cost; the per-observation restatement for a unified-camera problem)."""
    if is_omni(p):
        return _restated_sums(p, o, np.zeros(6 * p.K + 3 * p.L), np.zeros(6 * p.K + 3 * p.L), np.longdouble)[2]["cost"]
    return covo.cost(p, o, pgo=pgo)


def reference_scalars(ref, vb, which="ldbl"):
    """The scalars stage A reads (capi.SC_NAMES) from a reference evaluated with va = c = g / d^2 and vb = n."""
    s, g, d = ref[which], ref["g"], ref["d"]
    sc = np.zeros(capi.SC_COUNT)
    sc[S["COST"]] = s["cost"]; sc[S["GMAX"]] = s["gmax"]; sc[S["XN2"]] = s["xnorm"] ** 2
    sc[S["GG"]] = math.fsum(((g / d) ** 2).tolist()); sc[S["GN2"]] = math.fsum(((d * vb) ** 2).tolist()); sc[S["GDOT"]] = s["g_b"]
    sc[S["VV"]] = s["a_a"]; sc[S["VG"]] = s["a_b"]; sc[S["NN"]] = s["b_b"]
    sc[S["JA"]] = s["aHa"]; sc[S["JB"]] = s["bHb"]; sc[S["JC"]] = s["aHb"]
    return sc


def dims(p, o, pgo=False):
    D = 6 if (pgo or o.visual_only) else 15
    return D, D * p.K, D * p.K + (0 if pgo else 3 * p.L)


def with_state(p, pose, sb=None, lm=None):
    """`p` at another estimate."""
    q = p.copy()
    q.kf_pose[:] = np.asarray(pose).reshape(-1, 7)
    if sb is not None:
        q.kf_speed_bias[:] = np.asarray(sb).reshape(-1, 9)
    if lm is not None and q.L:
        q.lm_pos[:] = np.asarray(lm).reshape(-1, 3)
    return q


def apply_step(p, o, stepv, pgo=False):
    """x (+) step as the oracle applies it: covo_pose_plus on every free pose (fixed ones keep their bits), plain addition elsewhere."""
    D, n, N = dims(p, o, pgo)
    stepv = np.asarray(stepv, dtype=np.float64)
    assert stepv.shape == (N,)
    q = p.copy()
    out = np.zeros(7)
    for i in range(p.K):
        if p.kf_fixed[i]:
            continue
        covo.lib().covo_pose_plus(capi.dptr(np.ascontiguousarray(p.kf_pose[i])), capi.dptr(np.ascontiguousarray(stepv[D * i:D * i + 6])), capi.dptr(out))
        q.kf_pose[i] = out
    if D == 15:
        q.kf_speed_bias[:] = p.kf_speed_bias + stepv[:n].reshape(-1, 15)[:, 6:]
    if not pgo and p.L:
        q.lm_pos[:] = p.lm_pos + stepv[n:].reshape(-1, 3)
    return q


def oracle_loop(p, o):
    """covo.gba_solve's loop (visual-inertial or visual-only bundle adjustment) as step() over the oracle's exports: the damped step from
    covo.step, the scalars from covo.tail_ref at c = g / d^2 and that step, the candidate's cost from covo.cost. Returns dict(iterations,
    termination, accepted, cost, radius, rows = the state after every round, regimes = the dogleg regime of every iteration)."""
    k = consts(o)
    D, n, N = dims(p, o)
    tr, x = initial_tr(o), p.copy()
    out = dict(accepted=[], cost=[], radius=[], rows=[], regimes=[], rho=[], hits=[])
    with covo.preintegrated_at(p):   # (as the solve: preintegrated once, at the biases it starts from)
        _oracle_iterations(p, o, k, N, tr, x, out)
    return out


def _oracle_iterations(p, o, k, N, tr, x, out):
    sc = c = gn = None
    reuse, it = False, 0
    while it < o.max_iterations:
        fresh = not reuse
        if fresh:
            mu = 1.0 / tr[T["RADIUS"]] if k["strategy"] == LM else tr[T["MU"]]
            dp, dl = covo.step(x, o, mu, dense=False)
            gn = np.concatenate([dp, dl.reshape(-1)])
            pre = covo.tail_ref(x, o, np.zeros(N), gn)
            c = pre[0] / (pre[1] * pre[1])
            sc = reference_scalars(reference(x, o, c, gn), gn, "dbl")
        hits = []
        tr = step_a(tr, sc, k, 0, fresh, hits)
        if tr[T["RETRY"]] == 0.0 and tr[T["TERM"]] == 0.0:
            cand = apply_step(x, o, tr[T["CG"]] * c + tr[T["CN"]] * gn)
            s2 = sc.copy(); s2[S["COST"]] = covo.cost(cand, o)
            tr = step_b(tr, s2, k, hits)
        out["rows"].append(tr.copy()); out["hits"].append(hits)
        if tr[T["RETRY"]] != 0.0:
            reuse = False
            continue
        term = int(tr[T["TERM"]])
        if term in (2, 3):
            break
        acc = tr[T["ACC"]] != 0.0
        out["accepted"].append(int(acc)); out["cost"].append(tr[T["COST"]]); out["radius"].append(tr[T["RADIUS"]]); out["rho"].append(tr[T["RHO"]])
        out["regimes"].append(dogleg_regime(tr) if k["strategy"] == DOGLEG else "lm")
        if acc:
            x = cand
        reuse = tr[T["REUSE"]] != 0.0
        it += 1
        if term in (1, 4):
            break
    out.update(iterations=it, termination=int(tr[T["TERM"]]), state=x)


# ------------------------------------------------------------------------------------------------ b) the points
# A run = one resident solve of the point's problem with these option overrides. chain: the state before the run's LAST iteration is the estimate the
# previous run of the list left (the runs of a chain differ in max_iterations only, and a solve is bit-reproducible); otherwise the uploaded one
# (every earlier iteration of the run was rejected, or there is none). radius "interp": the geometric mean of the Gauss-Newton and the Cauchy step's
# scaled norms, read from the point's first run — a radius at which the dogleg interpolates.
Run = namedtuple("Run", "kw chain")
Point = namedtuple("Point", "id build opt pgo runs")
_cache = {}

LADDER = tuple(1e7 * 4.0 ** -i for i in range(16))          # fresh dogleg iterations at these initial radii: 1e7 down to 9.3e-3
REUSE_KW = dict(initial_radius=64.0, min_relative_decrease=1e9, parameter_tolerance=0.0)   # every step rejected: the radius halves at a fixed state
REUSE_ITERATIONS = (1, 2, 5, 12)
REUSE_WIDE_ITERATIONS = (3, 8, 11, 16)
LM_ITERATIONS = (1, 2, 3, 4, 5, 6)
GN_INSIDE_RADIUS = 1e12
TWO_RADII = (Run(dict(initial_radius=GN_INSIDE_RADIUS, max_iterations=1), False), Run(dict(initial_radius="interp", max_iterations=1), False))


def tiny_problem(visual_only=False):
    key = ("tiny", visual_only)
    if key not in _cache:
        _cache[key] = mapdata.flatten_gba(synth.make_map(synth.config_named("tiny")), visual_only, True)[0]
    return _cache[key]


def with_edges(p, E, seed=11):
    """`p` with E between factors: its own first, then edges over distinct random keyframe pairs whose measurement is the relative pose of the two
    current poses after a perturbation of 0.01 rad / 2 cm each — a non-zero residual at the current estimate. E = 0 drops the map's own."""
    from scipy.spatial.transform import Rotation as R
    key = ("edges", id(p), E, seed)
    if key in _cache:
        return _cache[key][1]
    rng = np.random.default_rng(seed)
    have = {(min(a, b), max(a, b)) for a, b in zip(p.edge_i.tolist(), p.edge_j.tolist())}
    pairs = [(i, j) for i in range(p.K) for j in range(i + 1, p.K) if (i, j) not in have]
    order = rng.permutation(len(pairs))
    ei, ej, meas = p.edge_i.tolist(), p.edge_j.tolist(), [m for m in p.edge_meas]
    for q in order[:max(E - p.E, 0)]:
        i, j = pairs[q]
        if rng.random() < 0.5:
            i, j = j, i
        Ts = []
        for t in (i, j):
            rot = (R.from_quat(p.kf_pose[t, :4]) * R.from_rotvec(rng.normal(0, 0.01, 3))).as_quat()
            Ts.append(np.concatenate([rot, p.kf_pose[t, 4:] + rng.normal(0, 0.02, 3)]))
        ei.append(i); ej.append(j); meas.append(mapdata._pose_inv_mul(Ts[0], Ts[1]))
    ei, ej, meas = ei[:E], ej[:E], meas[:E]
    d = dict(p.__dict__)
    d.update(edge_i=np.array(ei, np.int32), edge_j=np.array(ej, np.int32), edge_meas=np.array(meas).reshape(-1, 7),
             edge_sqrt_info=np.tile(mapdata.GBA_LOOP_SQRT_INFO.reshape(1, 36), (E, 1)), edge_loss_a=np.full(E, 1.0))
    q = capi.FlatProblem(**d)
    assert q.E == E
    _cache[key] = (p, q)   # (keeps `p` alive: the key holds its id)
    return q


def small_pose_graph():
    if "small-pgo" not in _cache:
        cfg = synth.config_named("small")
        cfg.drift_trans = 0.05; cfg.drift_yaw_deg = 0.5
        _cache["small-pgo"] = mapdata.flatten_pgo(synth.make_map(cfg), {}, mapdata.PgoParams())[0]
    return _cache["small-pgo"]


def omni_problem():
    """The unified-camera problem of tests/test_gpu_omni.py::test_gn_step_equals_a_dense_numpy_gauss_newton_step: three agents, one pinhole and two
    unified cameras, reprojection blocks only, two constant keyframes per camera."""
    if "omni" not in _cache:
        cams = (synth.SynthCamera(0, 0), synth.SynthCamera(1, 0, 0.9), synth.SynthCamera(1, 1, 1.3))
        m = synth.make_map(synth.SynthConfig(agents=(1, 2, 3), max_kf_per_agent=10, new_lm_per_kf=15, track_window=4, seed=2, cameras=cams))
        p = mapdata.flatten_gba(m, True, True)[0]
        d = dict(p.__dict__)
        d.update(edge_i=np.zeros(0, np.int32), edge_j=np.zeros(0, np.int32), edge_meas=np.zeros((0, 7)), edge_sqrt_info=np.zeros((0, 36)),
                 edge_loss_a=np.zeros(0))
        p = capi.FlatProblem(**d)
        for a in range(p.A):
            p.kf_fixed[np.nonzero(p.kf_cam == a)[0][:2]] = 1
        assert is_omni(p)
        _cache["omni"] = p
    return _cache["omni"]


CAPS_K, CAPS_L = 24, 176_000


def caps_problem():
    """A ring problem (tests/structure_util.ring_problem) past every grid cap of the tail: L = 176 000 landmarks with 3 observers each, so
    O = 528 000 > 2048 * 256 (k_tail_jvp, k_tail_cost: grid-stride over the observations), 3 L > 2048 * 256 (k_tail_apply) and
    N > 256 * 256 (k_tail_stats)."""
    if "caps" not in _cache:
        from tests import structure_util as su
        rng = np.random.default_rng(176)
        first = rng.integers(0, CAPS_K, CAPS_L)
        gaps = rng.integers(1, 8, (CAPS_L, 2))
        tracks = np.stack([first, (first + gaps[:, 0]) % CAPS_K, (first + gaps[:, 0] + gaps[:, 1]) % CAPS_K], 1)
        p = su.ring_problem(CAPS_K, list(tracks), (0, CAPS_K // 2), seed=177)
        assert p.O == 3 * CAPS_L > 2048 * 256 and 6 * p.K + 3 * p.L > 256 * 256
        _cache["caps"] = p
    return _cache["caps"]


def _ladder_runs():
    return tuple(Run(dict(initial_radius=r, max_iterations=1), False) for r in LADDER)


POINTS = [
    Point("tiny-dogleg-ladder", tiny_problem, dict(strategy=DOGLEG), False, _ladder_runs()),
    Point("tiny-dogleg-reuse", tiny_problem, dict(strategy=DOGLEG), False, tuple(Run(dict(REUSE_KW, max_iterations=m), False) for m in REUSE_ITERATIONS)),
    # the same from 2^20: the halved radii cross from the Gauss-Newton step through the interpolation to the Cauchy step, all re-derived (fresh = 0)
    Point("tiny-dogleg-reuse-wide", tiny_problem, dict(strategy=DOGLEG), False,
          tuple(Run(dict(REUSE_KW, initial_radius=2.0 ** 20, max_iterations=m), False) for m in REUSE_WIDE_ITERATIONS)),
    Point("tiny-lm", tiny_problem, dict(strategy=LM), False, tuple(Run(dict(max_iterations=m), True) for m in LM_ITERATIONS)),
] + [
    Point(f"tiny-E{E}", (lambda E=E: with_edges(tiny_problem(), E)), dict(strategy=DOGLEG), False, TWO_RADII) for E in (0, 64, 65, 257)
] + [
    Point("tiny-vo-E65", lambda: with_edges(tiny_problem(True), 65), dict(strategy=DOGLEG, visual_only=1), False, TWO_RADII),
    Point("small-pose-graph", small_pose_graph, dict(strategy=DOGLEG), True, TWO_RADII),
    Point("omni", omni_problem, dict(strategy=DOGLEG, visual_only=1), False, TWO_RADII),
    Point("caps", caps_problem, dict(strategy=DOGLEG, visual_only=1), False, TWO_RADII),
]
POINT = {pt.id: pt for pt in POINTS}
# the ladders the COVGPU_TAIL=0 form is held to (tests/helpers/tail_legacy.py runs them in a process of its own)
LEGACY_POINTS = ("tiny-dogleg-ladder", "tiny-dogleg-reuse", "tiny-dogleg-reuse-wide", "tiny-lm")

FINISH_SIZES = (1, 1023, 1024, 1025, 3073, 4096, 4097, 8192 + 7 + 5 + 8192)


def finish_partials(part_n, seed=0):
    """part[SC_COUNT][part_n] of mixed sign and six decades of magnitude."""
    rng = np.random.default_rng(1000 + part_n + seed)
    return rng.normal(size=(capi.SC_COUNT, part_n)) * 10.0 ** rng.uniform(-3, 3, (capi.SC_COUNT, part_n))


def finish_bound(part_n, absum):
    """Bound on |sum - fsum| of k_tail_finish: every partial passes through at most ceil(part_n / 4096) + 2 additions of a thread's serial sums and
    the 10 levels of the workgroup's tree, each with a relative error of at most 2^-53 on a partial sum bounded by sum |x|."""
    return (math.ceil(part_n / 4096) + 12) * 0.5 * EPS * absum


# ------------------------------------------------------------------------------------------------ c) the logic table
# A consistent small model: |g/d| = 2, |d n| = 3, alpha = GG / JA = 0.5 (Cauchy point at scaled norm 1), g.n = -n^T H n = -6, (J c).(J n) = -GG.
BASE_TR = dict(RADIUS=10.0, MU=1e-8, LMDF=2.0, COST=100.0, OK=1.0)
BASE_SC = dict(COST=100.0, GG=4.0, GN2=9.0, GDOT=-6.0, GMAX=3.0, XN2=400.0, VV=2.0, VG=-1.5, NN=5.0, JA=8.0, JB=6.0, JC=-4.0)
BASE_K = dict(strategy=DOGLEG, max_radius=1e16, min_relative_decrease=1e-3, function_tolerance=1e-6, parameter_tolerance=1e-8, gradient_tolerance=1e-10)
Row = namedtuple("Row", "id branches k tr sc flag0 fresh stages cost_new")


def _row(id_, branches, k=None, tr=None, sc=None, flag0=0, fresh=True, stages="AB", cost_new=99.0):
    t = np.zeros(capi.TR_COUNT); s = np.zeros(capi.SC_COUNT)
    for name, v in dict(BASE_TR, **(tr or {})).items():
        t[T[name]] = v
    for name, v in dict(BASE_SC, **(sc or {})).items():
        s[S[name]] = v
    return Row(id_, tuple(branches), dict(BASE_K, **(k or {})), t, s, flag0, fresh, stages, cost_new)


# the state a rejected dogleg step leaves: the dot products stored, the radius halved (stage A, fresh = 0, reads NO scalar: they are NaN here)
_STORED = dict(BASE_TR, RADIUS=1.5, ALPHA=0.5, REUSE=1.0, **{f: BASE_SC[f] for f in SUM_FIELDS})
_NAN_SC = {f: float("nan") for f in capi.SC_NAMES if f != "COST"}
# the Gauss-Newton step of the base model decreases the model by 3: cost_new = 100 - 3 rho
LOGIC_ROWS = [
    _row("dogleg-gn", ["dogleg_gn", "rho_between"], cost_new=98.5),
    _row("dogleg-cauchy", ["dogleg_cauchy"], tr=dict(RADIUS=0.5), cost_new=99.9),
    _row("dogleg-interp-c-positive", ["dogleg_interp", "beta_c_positive"], tr=dict(RADIUS=2.0), cost_new=99.0),
    _row("dogleg-interp-c-nonpositive", ["dogleg_interp", "beta_c_nonpositive"], tr=dict(RADIUS=2.0), sc=dict(GDOT=-1.0), cost_new=99.9),
    _row("solve-failed-retry", ["retry", "b_returns_on_retry"], flag0=1),
    _row("solve-failed-mu-tenth", ["not_ok_no_retry", "invalid_dogleg", "term4"], tr=dict(MU=0.1), flag0=1),
    _row("solve-failed-mu-above-one", ["not_ok_no_retry", "term4"], tr=dict(MU=2.0), flag0=1),
    _row("solve-failed-lm", ["invalid_lm"], k=dict(strategy=LM), flag0=1),
    _row("model-not-positive-dogleg", ["model_not_positive", "invalid_dogleg"], sc=dict(JB=100.0)),
    _row("model-not-positive-lm", ["model_not_positive", "invalid_lm"], k=dict(strategy=LM), sc=dict(JB=100.0)),
    _row("model-zero", ["model_not_positive", "invalid_dogleg"], sc=dict(JB=12.0)),
    _row("rho-below-quarter", ["dogleg_gn", "rho_below_quarter"], cost_new=99.7),
    _row("rho-between", ["dogleg_gn", "rho_between"], cost_new=98.5),
    _row("rho-above-three-quarters", ["dogleg_gn", "rho_above_three_quarters"], tr=dict(RADIUS=3.5), cost_new=97.3),
    _row("dogleg-reject", ["dogleg_reject"], cost_new=101.0),
    _row("dogleg-rederived", ["rederived", "dogleg_interp", "rho_between"], tr=_STORED, sc=_NAN_SC, fresh=False, cost_new=99.0),
    _row("dogleg-rederived-cauchy", ["rederived", "dogleg_cauchy"], tr=dict(_STORED, RADIUS=0.75), sc=_NAN_SC, fresh=False, cost_new=99.9),
    _row("lm-accept-grows", ["lm_accept"], k=dict(strategy=LM), cost_new=97.3),
    _row("lm-accept-shrinks", ["lm_accept"], k=dict(strategy=LM), cost_new=99.7),
    _row("lm-accept-max-radius", ["lm_accept_clamped"], k=dict(strategy=LM, max_radius=12.0), cost_new=97.3),
    _row("lm-reject", ["lm_reject"], k=dict(strategy=LM), tr=dict(LMDF=4.0), cost_new=101.0),
    _row("first", ["first"], tr=dict(FIRST=1.0, COST=-1.0), sc=dict(COST=250.0), cost_new=249.0),
    _row("term1", ["term1"], k=dict(function_tolerance=1.0), cost_new=98.5),
    _row("term2", ["term2", "b_returns_on_term"], k=dict(parameter_tolerance=1.0)),
    _row("term3", ["term3", "b_returns_on_term"], k=dict(gradient_tolerance=5.0)),
    _row("a-returns-on-term", ["a_returns_on_term", "b_returns_on_term"], tr=dict(TERM=1.0)),
    _row("b-returns-on-term", ["b_returns_on_term"], tr=dict(TERM=2.0, VALID=1.0, MODEL=3.0), stages="B"),
    _row("b-returns-on-retry", ["b_returns_on_retry"], tr=dict(RETRY=1.0, VALID=1.0, MODEL=3.0), stages="B"),
]


def row_expected(row, sc=None):
    """(state after the row's stages, branches taken) by the restatement; sc: the scalars to read instead of the row's (the device's own sums)."""
    hits = []
    sc = row.sc if sc is None else sc
    t = row.tr
    if "A" in row.stages:
        t = step_a(t, sc, row.k, row.flag0, row.fresh, hits)
    if "B" in row.stages:
        s2 = np.array(sc); s2[S["COST"]] = row.cost_new
        t = step_b(t, s2, row.k, hits)
    return t, hits
