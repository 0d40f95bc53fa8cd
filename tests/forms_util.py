"""The sweep of plan shapes that tests/test_gpu_forms.py runs on the device and tests/test_nd_plan.py checks on the host: ONE table, so that the
shape conditions the GPU test relies on (which kernel form a point is meant to reach) fail on the CPU first when the plan heuristics change.

A point is a synthetic map (optionally cut to `kf` keyframes per agent), visual-inertial (15 unknowns per keyframe) or visual-only (6), a leaf
size for COVGPU_ND_LEAF (0: the default candidates of nd_plan_build) and optional further plan switches. `mus`: the dampings the device test runs
at this point (1e-4 = the first iteration of every real solve, everywhere; 1e-8 at one point per map, comparable with
test_single_linearisation_at_full_size)."""
import os
from collections import namedtuple

import numpy as np

from covins_amd import backend, mapdata, synth

Point = namedtuple("Point", "id map kf visual_only leaf env mus")


def _pt(map_, kf, vo, leaf, env=None, mus=(1e-4,)):
    name = f"{map_}{'@%d' % kf if kf else ''}{'-vo' if vo else ''}-leaf{leaf if leaf else 'default'}" + "".join(f"-{k[7:].lower()}{v}" for k, v in (env or {}).items())
    return Point(name, map_, kf, vo, leaf, dict(env or {}), tuple(mus))


# Order = the order the device test runs them in on its ONE shared context: large and small plans alternate, so that everything a context
# caches per problem (live-tile lists per level, the plan, border tiles stored by the extend-add) meets a problem it was not made for.
FOUR_WAVE = _pt("mh123", None, False, 15)                        # > 384 small fronts in one level: k_potrf_panel4
SWEEP = [
    FOUR_WAVE,
    _pt("small", None, False, 128),
    _pt("mh01", None, True, 1920),                               # fronts of 1 290 / 1 422 own columns (six panels) under a 576 root
    _pt("small", None, False, 15, mus=(1e-4, 1e-8)),
    _pt("mh123", None, False, 0),                                # the default plan at full size: NO four-wave launch
    _pt("mh01", None, True, 15),
    _pt("mh123", 200, False, 1920),
    _pt("small", None, False, 60),
    _pt("mh123", 200, False, 0, env={"COVGPU_ND_TOP": "0"}),     # both ways of cutting three agents, one after the other on one context
    _pt("mh123", 200, False, 0, env={"COVGPU_ND_TOP": "1"}),
    _pt("mh01", None, True, 128, mus=(1e-4, 1e-8)),
    _pt("mh123", 200, False, 15, mus=(1e-4, 1e-8)),
    _pt("small", None, False, 0),
    _pt("mh01", None, True, 384),
    _pt("mh123", 200, False, 128),
    _pt("mh123", 200, False, 256),
    # 12 agents x 200 keyframes, 36 000 unknowns: what only size selects. 186 two-tile fronts in one level (k_bwd_pipe: more than 128 tile
    # workgroups) and a look-ahead update of more than 512 tiles (k_gemm_abt.rect as full tiles)
    _pt("a12x1000", 200, False, 0),
]
# repeated on a fresh context each, bit for bit: the first | the one that followed the largest plan | one visual-only
REPEAT = [SWEEP[0], SWEEP[1], SWEEP[2]]
# default-plan points below the 12-agent size: at most kSmallMin = 384 small fronts in any level and panel (launch_potrf_panel, k_panel.hip)
K_SMALL_MIN = 384

_maps, _probs = {}, {}


def point_map(pt):
    key = (pt.map, pt.kf)
    if key not in _maps:
        cfg = synth.config_named(pt.map)
        if pt.kf:
            cfg.max_kf_per_agent = pt.kf
        _maps[key] = synth.make_map(cfg)
    return _maps[key]


def point_problem(pt):
    key = (pt.map, pt.kf, pt.visual_only)
    if key not in _probs:
        _probs[key] = mapdata.flatten_gba(point_map(pt), visual_only=pt.visual_only, loop_loss=True)[0]
    return _probs[key]


def point_options(pt, **kw):
    return backend.default_options(visual_only=1 if pt.visual_only else 0, **kw)


class forced_env:
    """The point's plan switches in os.environ for the length of a `with` (the host plan reads them as the upload does)."""

    def __init__(self, pt, leaf_too=False):
        self.env = dict(pt.env)
        if leaf_too and pt.leaf:
            self.env["COVGPU_ND_LEAF"] = str(pt.leaf)
        self.names = set(self.env) | {"COVGPU_ND_TOP", "COVGPU_ND_GROUP_FRAC"} | ({"COVGPU_ND_LEAF"} if leaf_too else set())

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.names}
        for k in self.names:
            os.environ.pop(k, None)
        os.environ.update(self.env)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def host_plan(pt):
    """(info, parent, level, own, st) of the point's plan from covgpu_nd_plan_create: the tree the device builds at upload under the same switches."""
    from tests.test_nd_plan import _plan
    with forced_env(pt):
        return _plan(point_problem(pt), point_options(pt), pt.leaf)


def plan_shape(pt, plan=None):
    """Shape figures of a point's host plan, from the plan arrays alone (nd_tables.hip front_layout / k_chol.hip read the same quantities):
    own / border order per front, per level the padded interior order (multiple of 256 = two tiles) and, per 256-column panel, the number of
    fronts with 1 .. 128 real columns in it (NdLevel::psmall: what selects k_potrf_panel4)."""
    info, parent, level, own, st = plan if plan is not None else host_plan(pt)
    dim = (lambda v: 6) if pt.visual_only else (lambda v: 9 if v & 1 else 6)
    od = np.array([sum(dim(int(v)) for v in o) for o in own])
    bd = np.array([sum(dim(int(v)) for v in s) for s in st])
    level = np.asarray(level); parent = np.asarray(parent)
    nlev = int(level.max()) + 1
    small = []
    for l in range(nlev):
        o = od[level == l]
        npan = (int(o.max()) + 255) // 256
        small.append([int(((o - 256 * P >= 1) & (o - 256 * P <= 128)).sum()) for P in range(npan)])
    tiles = (od + 127) // 128
    lev_tiles = [2 * ((int(od[level == l].max()) + 255) // 256) + (int(bd[level == l].max()) + 127) // 128 for l in range(nlev)]
    nfr = [int((level == l).sum()) for l in range(nlev)]
    # tiles of the largest look-ahead update of the rows below the next panel (k_chol.hip: (T - h1) * w * fronts; full tiles above kRectQuarterMax = 512)
    rect = [(lev_tiles[l] - min(2 * P + 4, lev_tiles[l])) * 2 * nfr[l] for l in range(nlev) for P in range(1, (int(od[level == l].max()) + 255) // 256)]
    # tile workgroups of a level's pipelined backward substitution (fronts x interior tiles, levels of two tiles and more; k_bwd_pipe above 128)
    pipe = [nfr[l] * int(tiles[level == l].max()) for l in range(nlev) if int(tiles[level == l].max()) >= 2]
    return dict(rect_max=max(rect, default=0), pipe_max=max(pipe, default=0), fronts=len(od), levels=nlev, own=od, border=bd, parent=parent, level=level, root_order=int(od[level == nlev - 1].max()),
                small=small, max_small=max(max(s) for s in small), tiles=tiles,
                lev_own_max=[int(od[level == l].max()) for l in range(nlev)],
                # tiles of a level's padded order: interior rounded up to the 256-column panel + the widest border rounded up to the tile
                lev_tiles=lev_tiles)


# ---- host references of a point's linear system (the oracle's S, b alone; nothing of the device code)
_sys, _mf = {}, {}


def scaled_err(x, x0, d):   # (x0: the reference, host_system(..)["x_ref"])
    """Difference of two steps in the metric of the system, d = sqrt(diag S) (test_single_linearisation_at_full_size)."""
    return float(np.abs((x - x0) * d).max() / np.abs(x0 * d).max())


SUPERLU_MAX_N = 33000


def _lapack_multifrontal(p, ptr, col, blocks, b):
    """oracle/covo_mf.py on the block-CSR system: LAPACK potrf / trsm / syrk per front of the DEFAULT plan, on the host."""
    import ctypes as C
    from oracle import covo, covo_mf
    n, K = len(b), len(ptr) - 1
    covo_mf.set_problem(p, backend.default_options(), int(covo.lib().covo_num_threads()))
    ptr = np.ascontiguousarray(ptr, np.int32); col = np.ascontiguousarray(col, np.int32)
    vals = np.ascontiguousarray(blocks, np.float64).reshape(-1); rhs = np.ascontiguousarray(b, np.float64); x = np.zeros(n)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)); dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    rc = covo_mf.solve(n, 15, K, ip(ptr), ip(col), dp(vals), dp(rhs), dp(x))
    assert rc == 0, rc
    return x


def host_system(pt, mu):
    """The oracle's reduced camera system of the point's problem at damping mu and its host solutions, built once per (map, mu): S (CSR), b, cost,
    d = sqrt(diag S), x_lu (SuperLU, as test_single_linearisation_at_full_size) and, for n <= 9 000, x_d (dense LAPACK). Above SUPERLU_MAX_N
    unknowns SuperLU gives up (it reports "not enough memory" at 36 000, with tens of gigabytes free): there x_ref is the LAPACK multifrontal port oracle/covo_mf.py, the
    reference test_single_linearisation_at_full_size uses at the 12-agent sizes; x_ref = x_lu everywhere else."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    from oracle import covo
    key = (pt.map, pt.kf, pt.visual_only, mu)
    if key not in _sys:
        p = point_problem(pt)
        D = 6 if pt.visual_only else 15
        ptr, col, blocks, b, cost = covo.schur_sparse(p, covo.default_options(visual_only=1 if pt.visual_only else 0), mu)
        n = D * p.K
        S = sp.bsr_matrix((blocks, col, ptr), shape=(n, n)).tocsr()
        x_lu = x_mfl = None
        if n <= SUPERLU_MAX_N:
            x_lu = spla.splu(S.tocsc(), permc_spec="MMD_AT_PLUS_A", diag_pivot_thresh=0.0, options=dict(SymmetricMode=True)).solve(b)
        else:
            x_mfl = _lapack_multifrontal(p, ptr, col, blocks, b)
        x_d = np.linalg.solve(S.toarray(), b) if n <= 9000 else None
        _sys[key] = dict(S=S, b=np.asarray(b), cost=cost, d=np.sqrt(np.abs(S.diagonal())), x_lu=x_lu, x_mfl=x_mfl, x_ref=x_lu if x_lu is not None else x_mfl,
                         x_d=x_d, n=n, D=D)
    return _sys[key]


def host_replay(pt, mu):
    """x_mf: the numpy replay (tests/test_nd_plan._replay_sparse) of the SAME plan as the device uses at this point, on the oracle's system. Run per
    point where n <= 9 000 and, above, at the four-wave point only (None elsewhere) — and where SuperLU is out of reach: a second host solver."""
    from tests.test_nd_plan import _replay_sparse
    sysm = host_system(pt, mu)
    if 9000 < sysm["n"] <= SUPERLU_MAX_N and pt is not FOUR_WAVE:
        return None
    key = (pt.id, mu)
    if key not in _mf:
        info, parent, level, own, st = host_plan(pt)
        _mf[key] = _replay_sparse(sysm["S"], sysm["b"], parent, level, own, st, sysm["D"])
    return _mf[key]


def host_spread(pt, mu):
    """(h, r_h, solutions): the largest pairwise scaled difference among the host solutions of this point's system and their largest relative
    residual. Above n = 9 000 the replay exists at the four-wave point only; the map's other points take it from there (another elimination order
    of the same system: all the spread measures)."""
    sysm = host_system(pt, mu)
    xs = {"lu": sysm["x_lu"]} if sysm["x_lu"] is not None else {"lapack_mf": sysm["x_mfl"]}
    if sysm["x_d"] is not None:
        xs["dense"] = sysm["x_d"]
    x_mf = host_replay(pt, mu)
    if x_mf is None and (FOUR_WAVE.map, FOUR_WAVE.kf, FOUR_WAVE.visual_only) == (pt.map, pt.kf, pt.visual_only):
        x_mf = host_replay(FOUR_WAVE, mu)
    if x_mf is not None:
        xs["replay"] = x_mf
    names = sorted(xs)
    h = max(scaled_err(xs[a], xs[b], sysm["d"]) for a in names for b in names if a != b)
    nb = np.linalg.norm(sysm["b"])
    r_h = max(float(np.linalg.norm(sysm["S"] @ x - sysm["b"]) / nb) for x in xs.values())
    return h, r_h, xs
