"""Marginal covariances of selected keyframes from the multifrontal factor (Context.marginal_covariance) against host references.

Every covariance is held to the spread of three HOST routes to the same block of S^-1 on the oracle's system (tests/marginal_util.py: SuperLU
solves of the unit columns, dense LU, dense Cholesky + forward solves + Gram): err(device, lu) <= C max(h, 1e-13) in the metric
max |(A - B) o d d^T| / max |A_lu o d d^T|, d = sqrt(diag S). Never compared with another run of the device code, except where the assertion IS
that two runs return the same bits.

Points: the smallest shapes at which the sweep can go wrong — many levels of tiny fronts (small, leaf 15), the default plan and leaf 128,
fronts of 1 290 / 1 422 own columns under a 576 root (mh01 visual-only, leaf 1920: substitution through several panels of one front), three
agents under both cuts of the top (paths that meet only at the root), and the pose graphs of two maps. Selections come from the host plan: one
keyframe, two whose poses one front owns, two in different subtrees, one owned by a root, one whose pose and speed-bias blocks have different
owners, a shuffled list, 1 / 2 / 3 / the limit's number of keyframes, pose rows and all rows — column ranges below 16, at 16 and far above.

C = 30: the smallest of 10, 30, 100 that leaves a factor 3 over the worst observed ratio err / max(h, 1e-13). Observed on one MI355X:

  small-leaf15        mu 0     n 2 700   h 2.2e-8    10 selections, up to 69 fronts   worst err / h 0.60 (one keyframe, all rows)
  small-leaf128       mu 0     n 2 700   h 2.2e-8    up to 25 fronts   0.26;   small default: up to 16 fronts   0.15
  mh01-vo-leaf1920    mu 0     n 3 288   h 2.9e-9    up to 3 fronts    7.58 (one keyframe);   mu 1e-8: h 9.4e-10   4.58 (root-owned)
  mh123@200 default   COVGPU_ND_TOP=0 / 1   mu 0   n 9 000   h 2.3e-8   up to 48 fronts   0.36 / 0.29 (two poses of one front)
  pose graph          small: h 4.2e-14 (below the floor)  0.85;   mh123@200: h 3.1e-13   up to 22 fronts   2.22 (the limit's 32 keyframes)

The visual-only ratios are the system's, as in tests/test_gpu_forms.py: the device assembles S in another summation order than the oracle, whose S
all three host routes share. Both forms ran at every point (a one-keyframe pose selection is 6 columns wide, the limit's 480).
"""
import os
from collections import defaultdict

import numpy as np
import pytest

from covins_amd import backend, capi
from tests import forms_util as fu
from tests import marginal_util as mu_

pytestmark = pytest.mark.gpu

C_BOUND = 30          # the smallest of 10, 30, 100 that leaves a factor 3 over the worst observed ratio (7.58)
H_FLOOR = mu_.H_FLOOR

GBA_POINTS = [
    (fu._pt("small", None, False, 15), (0.0,)),
    (fu._pt("small", None, False, 128), (0.0,)),
    (fu._pt("small", None, False, 0), (0.0,)),
    (fu._pt("mh01", None, True, 1920), (0.0, 1e-8)),
    (fu._pt("mh123", 200, False, 0, env={"COVGPU_ND_TOP": "0"}), (0.0,)),
    (fu._pt("mh123", 200, False, 0, env={"COVGPU_ND_TOP": "1"}), (0.0,)),
]
PGO_POINTS = [("small", None), ("mh123", 200)]


@pytest.fixture(scope="module")
def shared():
    c = backend.Context(0)
    state = dict(ctx=c, stats=[], first={})
    yield state
    c.close()


def selections(pt, prob):
    """name -> (keyframes, block) from the point's host plan."""
    info, parent, level, own, st = fu.host_plan(pt)
    lim = backend.marginal_limits()
    owner = {int(v): n for n, o in enumerate(own) for v in o}
    free = [int(k) for k in np.flatnonzero(prob.kf_fixed == 0)]
    vi = not pt.visual_only

    def path(n):
        s = set()
        while n >= 0:
            s.add(int(n)); n = parent[n]
        return s

    by_node = defaultdict(list)
    for k in free:
        by_node[owner[2 * k]].append(k)
    n0 = min((int(level[n]), n) for n, l in by_node.items() if len(l) >= 2)[1]
    a = by_node[n0][0]
    pa = path(owner[2 * a])
    b = next(k for k in reversed(free) if owner[2 * k] not in pa and owner[2 * a] not in path(owner[2 * k]))
    sel = {"one": ([free[len(free) // 3]], "pose"), "one_full": ([free[len(free) // 3]], "full"),
           "same_front": (by_node[n0][:2], "pose"), "two_subtrees": ([a, b], "pose"), "two_subtrees_full": ([a, b], "full")}
    root_kf = [k for k in free if parent[owner[2 * k]] < 0]
    if root_kf:
        sel["root_owned"] = ([root_kf[0], a], "full")
    if vi:
        split = [k for k in free if owner[2 * k] != owner[2 * k + 1]]
        if split:
            sel["split_owners"] = ([split[len(split) // 2]], "full")
    rng = np.random.default_rng(11)
    spread = [free[i] for i in np.linspace(0, len(free) - 1, lim["max_kf"]).astype(int)]
    assert len(set(spread)) == lim["max_kf"]
    sel["shuffled"] = ([int(k) for k in rng.permutation(spread[:7])], "pose")
    sel["three"] = (spread[:3], "pose")
    sel["limit"] = ([int(k) for k in rng.permutation(spread)], "full")
    return sel


def _union(sel):
    seen = []
    for kfs, _ in sel.values():
        for k in kfs:
            if k not in seen:
                seen.append(int(k))
    return seen


def _check_cov(tag, cov, stats, ref, ref_kfs, kfs, block, shared):
    full = block == "full"
    want = {k: mu_.take(ref[k], ref_kfs, ref["D"], kfs, full) for k in ("lu", "dense", "chol") if k in ref}
    pos = {int(k): i for i, k in enumerate(ref_kfs)}
    d = np.concatenate([ref["d"][ref["D"] * pos[int(k)]: ref["D"] * pos[int(k)] + (ref["D"] if full else 6)] for k in kfs])
    e = mu_.err(cov, want["lu"], want["lu"], d)
    ratio = e / max(ref["h"], H_FLOOR)
    print(f"{tag}: m={cov.shape[0]} fronts={stats['fronts']} launches={stats['launches']} (mfma {stats['mfma_launches']}, vector {stats['vector_launches']}) "
          f"scratch={stats['scratch_bytes']} h={ref['h']:.2e} err={e:.2e} ({ratio:.2f} h)")
    shared["stats"].append(stats)
    assert stats["columns"] == cov.shape[0] and stats["launches"] == stats["mfma_launches"] + stats["vector_launches"] + 2
    assert np.array_equal(cov, cov.T), tag
    assert (np.diag(cov) > 0).all(), tag
    assert e <= C_BOUND * max(ref["h"], H_FLOOR), (tag, e, ref["h"])
    return ratio, d


@pytest.mark.parametrize("pt,mus", GBA_POINTS, ids=[p.id for p, _ in GBA_POINTS])
def test_point(shared, pt, mus):
    ctx = shared["ctx"]
    prob, opt = fu.point_problem(pt), fu.point_options(pt)
    sel = selections(pt, prob)
    ref_kfs = _union(sel)
    with fu.forced_env(pt, leaf_too=True):
        ctx.upload(prob, opt)
        for mu in mus:
            ref = mu_.point_reference(pt, mu, ref_kfs)
            got = {}
            for name, (kfs, block) in sel.items():
                cov, st = ctx.marginal_covariance_resident(opt, kfs, block=block, mu=mu)
                _, d = _check_cov(f"{pt.id} mu={mu:g} {name}", cov, st, ref, ref_kfs, kfs, block, shared)
                got[name] = (cov, d)
            # the pose rows of the full block against the pose block, to the same bound
            for p_name, f_name in (("one", "one_full"), ("two_subtrees", "two_subtrees_full")):
                kfs = sel[p_name][0]
                idx = np.array([15 * i + r for i in range(len(kfs)) for r in range(6)]) if not pt.visual_only else np.arange(6 * len(kfs))
                sub = got[f_name][0][np.ix_(idx, idx)]
                want = mu_.take(ref["lu"], ref_kfs, ref["D"], kfs, False)
                assert mu_.err(got[p_name][0], sub, want, got[p_name][1]) <= C_BOUND * max(ref["h"], H_FLOOR), (pt.id, p_name)
            # the one-call form (upload + factor + sweep) returns the resident call's bits, in the request's order
            kfs, block = sel["shuffled"]
            cov2, _ = ctx.marginal_covariance(prob, opt, kfs, block=block, mu=mu)
            assert np.array_equal(cov2, got["shuffled"][0])
    shared["first"].setdefault(pt.id, (sel, got))


@pytest.mark.parametrize("name,kf", PGO_POINTS, ids=[f"pgo-{n}{'@%d' % k if k else ''}" for n, k in PGO_POINTS])
def test_pose_graph(shared, name, kf):
    ctx = shared["ctx"]
    prob = mu_.pgo_problem(name, kf)
    opt = backend.default_options()
    free = [int(k) for k in np.flatnonzero(prob.kf_fixed == 0)]
    lim = backend.marginal_limits()
    spread = [free[i] for i in np.linspace(0, len(free) - 1, lim["max_kf"]).astype(int)]
    sel = {"one": [spread[5]], "two": [spread[-1], spread[0]], "three": spread[10:13], "limit": spread[::-1]}
    ref = mu_.reference(prob, False, 0.0, spread, pgo=True, key=("pgo", name, kf))
    for tag, kfs in sel.items():
        for block in ("pose", "full"):   # (the same six rows on a pose graph)
            cov, st = ctx.marginal_covariance(prob, opt, kfs, block=block, mu=0.0, pgo=True)
            _check_cov(f"pgo {name} {tag} {block}", cov, st, ref, spread, kfs, block, shared)


def test_both_forms_ran_over_the_file(shared):
    if not shared["stats"]:
        pt = GBA_POINTS[0][0]
        test_point(shared, pt, GBA_POINTS[0][1])
    assert sum(s["mfma_launches"] for s in shared["stats"]) > 0 and sum(s["vector_launches"] for s in shared["stats"]) > 0


def test_repeat_on_a_fresh_context_is_bit_identical(shared):
    pt, mus = GBA_POINTS[0]
    if pt.id not in shared["first"]:
        test_point(shared, pt, mus)
    sel, got = shared["first"][pt.id]
    prob, opt = fu.point_problem(pt), fu.point_options(pt)
    c = backend.Context(0)
    try:
        with fu.forced_env(pt, leaf_too=True):
            for name in ("limit", "two_subtrees", "split_owners"):
                if name not in sel:
                    continue
                kfs, block = sel[name]
                cov, _ = c.marginal_covariance(prob, opt, kfs, block=block, mu=mus[-1])
                assert np.array_equal(cov, got[name][0]), name
                cov, _ = c.marginal_covariance(prob, opt, kfs, block=block, mu=mus[-1])   # and with history
                assert np.array_equal(cov, got[name][0]), name
    finally:
        c.close()


def test_resident_call_behind_a_solve_leaves_the_next_solve_its_bits():
    pt = fu._pt("small", None, False, 0)
    prob = fu.point_problem(pt)
    opt = fu.point_options(pt, max_iterations=3)
    free = [int(k) for k in np.flatnonzero(prob.kf_fixed == 0)]
    kfs = [free[-2], free[3], free[len(free) // 2]]
    a, b, c = backend.Context(0), backend.Context(0), backend.Context(0)
    try:
        a.upload(prob, opt); ra1 = a.solve_resident(opt); qa1 = a.download()
        cov_r, st = a.marginal_covariance_resident(opt, kfs, block="full", mu=0.0)
        ra2 = a.solve_resident(opt); qa2 = a.download()
        b.upload(prob, opt); b.solve_resident(opt); rb2 = b.solve_resident(opt); qb2 = b.download()
        for f in ("kf_pose", "kf_speed_bias", "lm_pos"):
            assert np.array_equal(getattr(qa2, f), getattr(qb2, f)), f
            assert np.array_equal(getattr(qa2, f), getattr(qa1, f)), f
        assert ra2.final_cost == rb2.final_cost == ra1.final_cost and ra2.iterations == rb2.iterations
        # the resident call at the solve's estimate == the one-call form at the downloaded estimate, bit for bit
        cov_d, _ = c.marginal_covariance(qa1, opt, kfs, block="full", mu=0.0)
        assert np.array_equal(cov_r, cov_d)
        assert np.array_equal(cov_r, cov_r.T) and (np.diag(cov_r) > 0).all()
    finally:
        a.close(); b.close(); c.close()


def test_facade_shim_returns_the_python_calls_bits(shared):
    import ctypes as C
    from covins_amd import mapdata, synth
    from tests.facade_util import StandinMap
    m = synth.make_map(synth.config_named("tiny"))
    lib = mu_.shim()
    sm = StandinMap(m)
    try:
        # (tiny visual-only is not positive definite without damping: that case runs at the damping of a solve's first iteration)
        for visual_only, full, mu in ((False, True, 0.0), (False, False, 0.0), (True, False, 1e-4)):
            prob, idx = mapdata.flatten_gba(m, visual_only, loop_loss=True)
            # the facade reads poses and extrinsics through 4x4 transforms (quaternion -> matrix -> quaternion moves last bits) and lists a
            # landmark's observations in its container's order: the Python call gets the facade's own arrays — the same problem in its bits
            prob, moved = mu_.facade_problem(sm, prob, visual_only)
            print(f"facade visual_only={visual_only}: arrays whose bits differ from Python's flattening: {moved}")
            free = [int(k) for k in np.flatnonzero(prob.kf_fixed == 0)]
            kfs = [free[-1], free[0], free[len(free) // 2]]
            opt = backend.default_options(visual_only=1 if visual_only else 0)
            cov, st = shared["ctx"].marginal_covariance(prob, opt, kfs, block="full" if full else "pose", mu=mu)
            rows = np.ascontiguousarray(np.asarray(idx.kf_rows)[kfs], np.int32)
            out = np.zeros_like(cov); stats = (C.c_longlong * 8)(); msg = C.create_string_buffer(256)
            rc = lib.shim_marginal(sm.h, len(rows), rows.ctypes.data_as(C.POINTER(C.c_int)), int(visual_only), int(full), mu,
                                   out.ctypes.data_as(C.POINTER(C.c_double)), stats, msg)
            assert rc == 0, msg.value
            assert np.array_equal(out, cov) and [int(v) for v in stats] == [st[k] for k in capi.MARGINAL_STATS]
            if not full:   # the covariance of the relative pose of the first two: the facade's product against the Python helper
                c12 = np.ascontiguousarray(cov[:12, :12]); r = np.zeros((6, 6))
                lib.shim_relative_pose_covariance(sm.h, int(rows[0]), int(rows[1]), c12.ctypes.data_as(C.POINTER(C.c_double)),
                                                  r.ctypes.data_as(C.POINTER(C.c_double)))
                want = backend.relative_pose_covariance(c12, prob.kf_pose[kfs[0]], prob.kf_pose[kfs[1]])
                assert np.array_equal(r, r.T) and np.abs(r - want).max() <= 1e-12 * np.abs(want).max()
        bad = np.ascontiguousarray(np.asarray(idx.kf_rows)[[free[0], free[0]]], np.int32)
        rc = lib.shim_marginal(sm.h, 2, bad.ctypes.data_as(C.POINTER(C.c_int)), 1, 0, 0.0, out.ctypes.data_as(C.POINTER(C.c_double)), None, msg)
        assert rc == 1 and b"duplicate keyframe" in msg.value, msg.value
    finally:
        sm.close()


def test_refusals_that_depend_on_the_context(shared):
    ctx = shared["ctx"]
    prob = mu_.pgo_problem("small")
    opt = backend.default_options()
    free = [int(k) for k in np.flatnonzero(prob.kf_fixed == 0)]
    old = os.environ.get("COVGPU_PGO_ND")
    os.environ["COVGPU_PGO_ND"] = "0"
    try:
        with pytest.raises(backend.CovGpuError, match="off the elimination tree"):
            ctx.marginal_covariance(prob, opt, free[:2], pgo=True)
    finally:
        if old is None:
            os.environ.pop("COVGPU_PGO_ND", None)
        else:
            os.environ["COVGPU_PGO_ND"] = old
    fixed = [int(k) for k in np.flatnonzero(prob.kf_fixed != 0)]
    ctx.upload(prob, opt, pgo=True)
    with pytest.raises(backend.CovGpuError, match="constant pose"):
        ctx.marginal_covariance_resident(opt, [free[0], fixed[0]])
    fresh = backend.Context(0)
    try:
        with pytest.raises(backend.CovGpuError, match="no problem uploaded"):
            fresh.marginal_covariance_resident(opt, free[:1])
    finally:
        fresh.close()
    # a sharded context holds one rank's share of the factor: refused before anything is uploaded or exchanged
    from covins_amd import distrib
    pt = GBA_POINTS[2][0]
    gprob, gopt = fu.point_problem(pt), fu.point_options(pt)
    gfree = [int(k) for k in np.flatnonzero(gprob.kf_fixed == 0)]
    plan = distrib.shard_plan(gprob, gopt, 2)
    assert plan is not None
    grp = distrib.Group(2)
    sc = backend.Context(0)
    try:
        sc.set_shard_group(plan, 0, grp)
        with pytest.raises(backend.CovGpuError, match="sharded context"):
            sc.marginal_covariance(gprob, gopt, gfree[:2])
        with pytest.raises(backend.CovGpuError, match="sharded context"):
            sc.marginal_covariance_resident(gopt, gfree[:2])
        sc.set_shard_none()
    finally:
        sc.close(); grp.close()
