"""Covariance of every keyframe by selected inversion of the multifrontal factor (Context.keyframe_covariances) against host
references.

Every block is held to the spread of three HOST routes to the same block of S^-1 on the oracle's system (tests/selinv_util.py over
tests/marginal_util.py: SuperLU, dense LU, dense Cholesky + Gram): err(device, lu) <= C max(h, 1e-13) per block, in the metric
max |(A - B) o di dj^T| / max |A_lu o di dj^T|, d = sqrt(diag S), h the worst pairwise err of the host routes over the blocks checked. Never
compared with another run of the device code, except where the assertion IS that two runs return the same bits, and in the consistency check
against the marginal sweep (another device route: held to the same bound, not to bits).

Points: the smallest shapes at which the sweep can go wrong — many levels of tiny fronts (small, leaf 15), leaf 128 and the default plan,
fronts of 1 290 / 1 422 own columns under a 576 root (mh01 visual-only, leaf 1920: several panels of 128 columns per front), three agents
under both cuts of the top (the device computes all keyframes, the reference covers 32 spread neighbouring pairs = 64 keyframes), and the
pose graphs of two maps. At every point: every diagonal block for "pose" and "full"; pair_ok == 1 on the whole off-diagonal pattern of the
oracle's S ("pose") and on every IMU factor ("full"), those blocks against the reference; a pair from two subtrees is refused with a zero
block; constant poses give zero blocks; bit symmetry and a positive diagonal; the diagonal blocks of 32 spread keyframes against
marginal_covariance_resident; the launch counts.

C = 30: the smallest of 10, 30, 100 that leaves a factor 3 over the worst observed ratio err / max(h, 1e-13). Observed on one MI355X, worst
ratio over diagonal and pair blocks, "pose" / "full":

  small-leaf15        mu 0     h 2.3e-8 / 2.5e-8   179 diagonal + 14 276 / 352 pair blocks   0.16 / 0.55
  small-leaf128       mu 0     0.09 / 0.23;   small default: 0.04 / 0.14
  mh01-vo-leaf1920    mu 0     h 3.3e-9   547 + 29 140 blocks   7.57 (a pair block; diagonal 6.55);   mu 1e-8: h 1.6e-9   4.56 (diagonal 2.75)
  mh123@200 default   COVGPU_ND_TOP=0 / 1   mu 0   h 4.5e-8 / 6.3e-8   64 + 482 / 64 blocks   0.23 / 0.05 and 0.18 / 0.05
  pose graph          small: h 6.2e-14 (below the floor) 179 + 1 698 blocks   2.04;   mh123@200: h 4.1e-13   64 + 64 blocks   1.99
  against the marginal sweep, 32 keyframes: at most 0.01 h at every point

The visual-only ratios are the system's, as in tests/test_gpu_marginal.py (7.58 there): the device assembles S in another summation order than
the oracle, whose S all three host routes share. Both forms ran over the file (asserted below).
"""
import os

import numpy as np
import pytest

from covins_amd import backend
from tests import forms_util as fu
from tests import marginal_util as mu_
from tests import selinv_util as su

pytestmark = pytest.mark.gpu

C_BOUND = 30
H_FLOOR = su.H_FLOOR

GBA_POINTS = [
    (fu._pt("small", None, False, 15), (0.0,), None),
    (fu._pt("small", None, False, 128), (0.0,), None),
    (fu._pt("small", None, False, 0), (0.0,), None),
    (fu._pt("mh01", None, True, 1920), (0.0, 1e-8), None),
    (fu._pt("mh123", 200, False, 0, env={"COVGPU_ND_TOP": "0"}), (0.0,), 32),
    (fu._pt("mh123", 200, False, 0, env={"COVGPU_ND_TOP": "1"}), (0.0,), 32),
]
PGO_POINTS = [("small", None, None), ("mh123", 200, 32)]


@pytest.fixture(scope="module")
def shared():
    c = backend.Context(0)
    state = dict(ctx=c, stats=[], first={}, ratios={})
    yield state
    c.close()


def _ref_keyframes(free, npairs, pairs):
    """All free keyframes, or the keyframes of `npairs` pairs spread over the sorted list `pairs` (so the reference covers pair blocks too)."""
    if npairs is None:
        return list(free)
    out = []
    for q in np.linspace(0, len(pairs) - 1, npairs).astype(int):
        for k in pairs[q]:
            if k not in out:
                out.append(int(k))
    assert len(out) >= npairs
    return out


def two_subtrees(parent, own, free):
    """Two free keyframes whose pose owners lie in different subtrees: neither front is on the other's path to the root."""
    owner = {int(v): n for n, o in enumerate(own) for v in o}

    def path(n):
        s = set()
        while n >= 0:
            s.add(int(n)); n = parent[n]
        return s

    for a in free:
        pa = path(owner[2 * a])
        for b in reversed(free):
            if owner[2 * b] not in pa and owner[2 * a] not in path(owner[2 * b]):
                return a, b
    return None


def _check_stats(tag, st, shared):
    shared["stats"].append(st)
    gathers = st["launches"] - st["mfma_launches"] - st["vector_launches"] - 1
    assert st["launches"] == st["mfma_launches"] + st["vector_launches"] + gathers + 1
    assert (0 if st["levels"] == 1 else 1) <= gathers <= st["levels"] - 1, (tag, st)
    assert st["mfma_launches"] + st["vector_launches"] >= 1 and st["mfma_launches"] <= 4 * st["levels"] and st["vector_launches"] <= st["levels"], (tag, st)
    assert st["fronts"] >= st["levels"] >= 1 and st["scratch_bytes"] > 0 and st["reserved7"] == 0


def _check_all(tag, ctx, opt, prob, ref, d_full, pose_pairs, full_pairs, far, mu, shared):
    """The two resident calls of a point and every check on them. Returns the outputs."""
    K = prob.K
    free = su.free_keyframes(prob)
    fixed = [k for k in range(K) if k not in set(free)]
    req_p = list(pose_pairs) + ([far, far[::-1]] if far else [])
    kp, pcp, okp, stp = ctx.keyframe_covariances_resident(opt, block="pose", mu=mu, pairs=req_p)
    kf_, pcf, okf, stf = ctx.keyframe_covariances_resident(opt, block="full", mu=mu, pairs=full_pairs)
    _check_stats(tag + " pose", stp, shared); _check_stats(tag + " full", stf, shared)
    assert kp.shape == (K, 6, 6) and kf_.shape == (K, d_full, d_full)
    # constant poses: zeros; free keyframes: symmetric bit for bit, positive diagonal
    for k in fixed:
        assert not kp[k].any() and not kf_[k].any(), (tag, k)
    for out in (kp, kf_):
        assert np.array_equal(out, out.transpose(0, 2, 1)), tag
        assert (np.diagonal(out[free], axis1=1, axis2=2) > 0).all(), tag
    # the guaranteed pairs are served; the pair from two subtrees is not
    npp = len(pose_pairs)
    assert okp[:npp].all(), (tag, "pose", [req_p[i] for i in np.flatnonzero(okp[:npp] == 0)[:5]])
    assert okf.all(), (tag, "full", [full_pairs[i] for i in np.flatnonzero(okf == 0)[:5]])
    if far:
        assert not okp[npp:].any() and not pcp[npp:].any(), (tag, far)
    assert stp["pairs_served"] == int(okp.sum()) and stf["pairs_served"] == int(okf.sum())
    # against the reference: the blocks whose keyframes it covers
    have = set(ref.kfs)
    dblocks = [(k, k) for k in ref.kfs]
    pblocks = [(q, i, j) for q, (i, j) in enumerate(pose_pairs) if i in have and j in have]
    fblocks = [(q, i, j) for q, (i, j) in enumerate(full_pairs) if i in have and j in have]
    worst = {}
    for name, d, kc, pc, blocks in (("pose", 6, kp, pcp, pblocks), ("full", d_full, kf_, pcf, fblocks)):
        h = ref.spread(dblocks + [(i, j) for _, i, j in blocks], d)
        bound = C_BOUND * max(h, H_FLOOR)
        e_d = max(ref.err(kc[k], k, k, d) for k in ref.kfs)
        e_p = max((ref.err(pc[q], i, j, d) for q, i, j in blocks), default=0.0)
        worst[name] = max(e_d, e_p) / max(h, H_FLOOR)
        print(f"{tag} mu={mu:g} {name}: {len(dblocks)} diagonal + {len(blocks)} pair blocks  h={h:.2e}  diagonal {e_d / max(h, H_FLOOR):.2f} h  "
              f"pairs {e_p / max(h, H_FLOOR):.2f} h")
        assert e_d <= bound and e_p <= bound, (tag, name, e_d, e_p, h)
        # a pair block and its transposed request are the same numbers
        pos = {p: q for q, p in enumerate(pose_pairs if name == "pose" else full_pairs)}
        for q, i, j in blocks[:50]:
            if (j, i) in pos:
                assert np.array_equal(pc[q], pc[pos[(j, i)]].T), (tag, i, j)
    # the pose rows of "full" against "pose", to the same bound
    h6 = ref.spread(dblocks, 6)
    e = max(su.block_err(kf_[k][:6, :6], kp[k], ref.block("lu", k, k, 6), ref.scale(k, 6), ref.scale(k, 6)) for k in ref.kfs)
    assert e <= C_BOUND * max(h6, H_FLOOR), (tag, e, h6)
    # the other device route: the marginal sweep on 32 spread keyframes
    lim = backend.marginal_limits()
    sp = [ref.kfs[i] for i in np.linspace(0, len(ref.kfs) - 1, lim["max_kf"]).astype(int)]
    assert len(set(sp)) == lim["max_kf"]
    cov, _ = ctx.marginal_covariance_resident(opt, sp, block="full", mu=mu)
    hf = ref.spread([(k, k) for k in sp], d_full)
    e = max(su.block_err(kf_[k], cov[d_full * t:d_full * t + d_full, d_full * t:d_full * t + d_full], ref.block("lu", k, k, d_full),
                         ref.scale(k, d_full), ref.scale(k, d_full)) for t, k in enumerate(sp))
    print(f"{tag} mu={mu:g}: against the marginal sweep {e / max(hf, H_FLOOR):.2f} h")
    assert e <= C_BOUND * max(hf, H_FLOOR), (tag, e, hf)
    shared["ratios"][f"{tag} mu={mu:g}"] = worst
    return dict(kp=kp, pcp=pcp, okp=okp, kf=kf_, pcf=pcf, okf=okf, req_p=req_p)


@pytest.mark.parametrize("pt,mus,npairs", GBA_POINTS, ids=[p.id for p, _, _ in GBA_POINTS])
def test_point(shared, pt, mus, npairs):
    ctx = shared["ctx"]
    prob, opt = fu.point_problem(pt), fu.point_options(pt)
    info, parent, level, own, st = fu.host_plan(pt)
    free = su.free_keyframes(prob)
    far = two_subtrees(parent, own, free)
    assert far is not None
    d_full = 6 if pt.visual_only else 15
    ref_kfs = _ref_keyframes(free, npairs, su.system_pairs(prob, pt.visual_only, 0.0) if pt.visual_only else su.imu_pairs(prob))
    with fu.forced_env(pt, leaf_too=True):
        ctx.upload(prob, opt)
        for mu in mus:
            ref = su.reference(prob, pt.visual_only, mu, ref_kfs, key=("selinv", pt.map, pt.kf))
            pose_pairs = su.system_pairs(prob, pt.visual_only, mu)
            full_pairs = pose_pairs if pt.visual_only else su.imu_pairs(prob)
            assert pose_pairs and full_pairs
            got = _check_all(pt.id, ctx, opt, prob, ref, d_full, pose_pairs, full_pairs, far, mu, shared)
            # a second call returns the same bits; the one-call form (upload + factor + sweep) returns the resident call's bits
            again = ctx.keyframe_covariances_resident(opt, block="pose", mu=mu, pairs=got["req_p"])
            assert np.array_equal(again[0], got["kp"]) and np.array_equal(again[1], got["pcp"]) and np.array_equal(again[2], got["okp"])
            one = ctx.keyframe_covariances(prob, opt, block="full", mu=mu, pairs=full_pairs)
            assert np.array_equal(one[0], got["kf"]) and np.array_equal(one[1], got["pcf"]) and np.array_equal(one[2], got["okf"])
    shared["first"].setdefault(pt.id, (mus[-1], full_pairs, got))


@pytest.mark.parametrize("name,kf,npairs", PGO_POINTS, ids=[f"pgo-{n}{'@%d' % k if k else ''}" for n, k, _ in PGO_POINTS])
def test_pose_graph(shared, name, kf, npairs):
    from tests.test_nd_plan import _plan
    ctx = shared["ctx"]
    prob = mu_.pgo_problem(name, kf)
    opt = backend.default_options()
    free = su.free_keyframes(prob)
    info, parent, level, own, st = _plan(prob, opt, 0, pgo=True)
    far = two_subtrees(parent, own, free)
    pairs = su.system_pairs(prob, False, 0.0, pgo=True)
    assert pairs
    ref = su.reference(prob, False, 0.0, _ref_keyframes(free, npairs, pairs), pgo=True, key=("selinv-pgo", name, kf))
    ctx.upload(prob, opt, pgo=True)
    _check_all(f"pgo {name}", ctx, opt, prob, ref, 6, pairs, pairs, far, 0.0, shared)


def test_both_forms_ran_over_the_file(shared):
    if not shared["stats"]:
        test_point(shared, *GBA_POINTS[0])
    assert sum(s["mfma_launches"] for s in shared["stats"]) > 0 and sum(s["vector_launches"] for s in shared["stats"]) > 0
    for tag, w in shared["ratios"].items():
        print(f"worst ratio {tag}: " + "  ".join(f"{k} {v:.2f}" for k, v in w.items()))


def test_repeat_on_a_fresh_context_is_bit_identical(shared):
    pt, mus, npairs = GBA_POINTS[0]
    if pt.id not in shared["first"]:
        test_point(shared, pt, mus, npairs)
    mu, full_pairs, got = shared["first"][pt.id]
    prob, opt = fu.point_problem(pt), fu.point_options(pt)
    c = backend.Context(0)
    try:
        with fu.forced_env(pt, leaf_too=True):
            for _ in range(2):   # (the second with history)
                one = c.keyframe_covariances(prob, opt, block="full", mu=mu, pairs=full_pairs)
                assert np.array_equal(one[0], got["kf"]) and np.array_equal(one[1], got["pcf"]) and np.array_equal(one[2], got["okf"])
            one = c.keyframe_covariances(prob, opt, block="pose", mu=mu, pairs=got["req_p"])
            assert np.array_equal(one[0], got["kp"]) and np.array_equal(one[1], got["pcp"]) and np.array_equal(one[2], got["okp"])
    finally:
        c.close()


def test_resident_call_between_two_solves_leaves_the_second_its_bits():
    pt = fu._pt("small", None, False, 0)
    prob = fu.point_problem(pt)
    opt = fu.point_options(pt, max_iterations=3)
    pairs = su.imu_pairs(prob)[:40]
    a, b, c = backend.Context(0), backend.Context(0), backend.Context(0)
    try:
        a.upload(prob, opt); ra1 = a.solve_resident(opt); qa1 = a.download()
        got = a.keyframe_covariances_resident(opt, block="full", mu=0.0, pairs=pairs)
        ra2 = a.solve_resident(opt); qa2 = a.download()
        b.upload(prob, opt); b.solve_resident(opt); rb2 = b.solve_resident(opt); qb2 = b.download()
        for f in ("kf_pose", "kf_speed_bias", "lm_pos"):
            assert np.array_equal(getattr(qa2, f), getattr(qb2, f)), f
            assert np.array_equal(getattr(qa2, f), getattr(qa1, f)), f
        assert ra2.final_cost == rb2.final_cost == ra1.final_cost and ra2.iterations == rb2.iterations
        # the resident call at the solve's estimate == the one-call form at the downloaded estimate, bit for bit
        one = c.keyframe_covariances(qa1, opt, block="full", mu=0.0, pairs=pairs)
        for x, y in zip(got[:3], one[:3]):
            assert np.array_equal(x, y)
        assert got[2].all() and got[3] == one[3]
    finally:
        a.close(); b.close(); c.close()


def test_facade_shim_returns_the_python_calls_bits(shared):
    import ctypes as C
    from covins_amd import capi, mapdata, synth
    from tests.facade_util import StandinMap
    m = synth.make_map(synth.config_named("tiny"))
    lib = su.shim()
    sm = StandinMap(m)
    try:
        # (tiny visual-only is not positive definite without damping: that case runs at the damping of a solve's first iteration)
        for visual_only, full, mu in ((False, True, 0.0), (False, False, 0.0), (True, False, 1e-4)):
            prob, idx = mapdata.flatten_gba(m, visual_only, loop_loss=True)
            prob, moved = mu_.facade_problem(sm, prob, visual_only)   # the same problem in the facade's bits (tests/marginal_util.py)
            free = su.free_keyframes(prob)
            pairs = [(free[0], free[1]), (free[1], free[0]), (free[-1], free[0]), (free[len(free) // 2], free[len(free) // 2 + 1])]
            opt = backend.default_options(visual_only=1 if visual_only else 0)
            kc, pc, ok, st = shared["ctx"].keyframe_covariances(prob, opt, block="full" if full else "pose", mu=mu, pairs=pairs)
            rows = np.asarray(idx.kf_rows)
            ri = np.ascontiguousarray(rows[[p[0] for p in pairs]], np.int32); rj = np.ascontiguousarray(rows[[p[1] for p in pairs]], np.int32)
            kc2 = np.zeros_like(kc); pc2 = np.zeros_like(pc); ok2 = np.zeros(len(pairs), np.uint8)
            stats = (C.c_longlong * 8)(); msg = C.create_string_buffer(256)
            ip = C.POINTER(C.c_int)
            rc = lib.shim_keyframe_covariances(sm.h, int(visual_only), int(full), mu, len(pairs), ri.ctypes.data_as(ip), rj.ctypes.data_as(ip),
                                               kc2.ctypes.data_as(C.POINTER(C.c_double)), pc2.ctypes.data_as(C.POINTER(C.c_double)),
                                               ok2.ctypes.data_as(C.POINTER(C.c_ubyte)), stats, msg)
            assert rc == 0, msg.value
            assert np.array_equal(kc2[rows], kc) and np.array_equal(pc2, pc) and np.array_equal(ok2, ok)
            assert [int(v) for v in stats] == [st[k] for k in capi.SELINV_STATS]
            assert ok[0] == ok[1] and np.array_equal(pc[0], pc[1].T) and ok.any()
        rc = lib.shim_keyframe_covariances(sm.h, 1, 0, -1.0, 0, None, None, kc2.ctypes.data_as(C.POINTER(C.c_double)), None, None, None, msg)
        assert rc == 1 and b"mu negative or not finite" in msg.value, msg.value
    finally:
        sm.close()


def test_refusals_that_depend_on_the_context(shared):
    ctx = shared["ctx"]
    prob = mu_.pgo_problem("small")
    opt = backend.default_options()
    free = su.free_keyframes(prob)
    old = os.environ.get("COVGPU_PGO_ND")
    os.environ["COVGPU_PGO_ND"] = "0"
    try:
        with pytest.raises(backend.CovGpuError, match="off the elimination tree"):
            ctx.keyframe_covariances(prob, opt, pgo=True)
    finally:
        if old is None:
            os.environ.pop("COVGPU_PGO_ND", None)
        else:
            os.environ["COVGPU_PGO_ND"] = old
    fixed = [int(k) for k in np.flatnonzero(prob.kf_fixed != 0)]
    ctx.upload(prob, opt, pgo=True)
    with pytest.raises(backend.CovGpuError, match="constant pose in a pair"):
        ctx.keyframe_covariances_resident(opt, pairs=[(free[0], fixed[0])])
    with pytest.raises(backend.CovGpuError, match="pair index out of range"):
        ctx.keyframe_covariances_resident(opt, pairs=[(free[0], prob.K)])
    fresh = backend.Context(0)
    try:
        with pytest.raises(backend.CovGpuError, match="no problem uploaded"):
            fresh.keyframe_covariances_resident(opt)
    finally:
        fresh.close()
    # a sharded context holds one rank's share of the factor: refused before anything is uploaded or exchanged
    from covins_amd import distrib
    pt = GBA_POINTS[2][0]
    gprob, gopt = fu.point_problem(pt), fu.point_options(pt)
    plan = distrib.shard_plan(gprob, gopt, 2)
    assert plan is not None
    grp = distrib.Group(2)
    sc = backend.Context(0)
    try:
        sc.set_shard_group(plan, 0, grp)
        with pytest.raises(backend.CovGpuError, match="sharded context"):
            sc.keyframe_covariances(gprob, gopt)
        with pytest.raises(backend.CovGpuError, match="sharded context"):
            sc.keyframe_covariances_resident(gopt)
        sc.set_shard_none()
    finally:
        sc.close(); grp.close()
