"""covgpu_match_batch (k_match.hip) on the GPU: DENSE against the reference DenseMatcher's own match lists
(tests/golden/densematcher_ref.npz), both modes against the numpy restatement (tests/match_ref.py) on map-derived and adversarial jobs,
batch independence, edge cases, argument validation, the chain DENSE -> covgpu_abspose_ransac_batch -> covgpu_relpose_batch, and
the C++ facade."""
import ctypes as C

import numpy as np
import pytest
from scipy.spatial.transform import Rotation as Rot

from covins_amd import backend, capi, synth
from tests import match_ref as mr
from tests import match_util as mu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = backend.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def small():
    return synth.make_map(synth.config_named("small"))


def _lists(res, bt, mode):
    off = res["offset"]
    return [mr.from_rows(res["match"][off[j]:off[j + 1]], res["dist"][off[j]:off[j + 1]], mode) for j in range(len(bt["set_a"]))]


def _run(ctx, bt, mode, **opts):
    sets = dict(row_ptr=bt["row_ptr"], desc=bt["desc"], skip=bt["skip"] if mode == "dense" else None)
    return ctx.match_batch(sets, bt["set_a"], bt["set_b"], mode, **opts)


def _check(ctx, bt, mode, **opts):
    res = _run(ctx, bt, mode, **opts)
    ref = mu.reference(bt, mode, **opts)
    got = _lists(res, bt, mode)
    for j, (g, r) in enumerate(zip(got, ref)):
        assert g == r, (mode, j, len(g), len(r))
        assert res["nmatches"][j] == len(r), j
    return res, ref


def test_dense_equals_the_reference_densematcher(ctx):
    from tests.test_match_host import fixture_cases
    cs, thr = fixture_cases()
    sb = mu.SetBuilder()
    for A, B, sA, sB, dg, dref, _ in cs:
        assert dg == dref
        sb.job(sb.add(A, sA), sb.add(B, sB))
    bt = sb.batch()
    res = _run(ctx, bt, "dense", dist_threshold=thr)
    got = _lists(res, bt, "dense")
    for j, c in enumerate(cs):
        assert got[j] == c[6], j
        assert res["nmatches"][j] == len(c[6])


@pytest.mark.parametrize("mode", ["dense", "knn2"])
def test_map_jobs_equal_the_restatement(ctx, small, mode):
    bt = mu.map_batch(small, 300, seed=21)
    res, ref = _check(ctx, bt, mode)
    n = np.array([len(r) for r in ref])
    print(f"{mode}: 300 map jobs, matches per job median {np.median(n):.0f}, min {n.min()}, max {n.max()}")
    assert n.mean() > 20


@pytest.mark.parametrize("mode", ["dense", "knn2"])
def test_adversarial_jobs_equal_the_restatement(ctx, mode):
    for seed in (0, 1, 2):
        _check(ctx, mu.adversarial_batch(seed), mode)


@pytest.mark.parametrize("mode,opts", [("dense", dict(dist_threshold=30.5)), ("dense", dict(dist_threshold=200.0)),
                                       ("knn2", dict(dist_threshold=50.0, ratio=0.9)), ("knn2", dict(dist_threshold=25.0, ratio=0.6))])
def test_other_thresholds_equal_the_restatement(ctx, small, mode, opts):
    bt = mu.map_batch(small, 40, seed=23)
    _check(ctx, bt, mode, **opts)
    _check(ctx, mu.adversarial_batch(3), mode, **opts)


@pytest.mark.parametrize("mode", ["dense", "knn2"])
def test_a_job_alone_equals_the_same_job_in_a_batch(ctx, small, mode):
    bt = mu.map_batch(small, 64, seed=25)
    full = _lists(_run(ctx, bt, mode), bt, mode)
    rng = np.random.default_rng(26)
    for j in (0, 17, 63):
        alone = dict(bt, set_a=bt["set_a"][j:j + 1], set_b=bt["set_b"][j:j + 1])
        assert _lists(_run(ctx, alone, mode), alone, mode)[0] == full[j]
    perm = rng.permutation(64)
    shuf = dict(bt, set_a=bt["set_a"][perm], set_b=bt["set_b"][perm])
    got = _lists(_run(ctx, shuf, mode), shuf, mode)
    for i, j in enumerate(perm):
        assert got[i] == full[j]


def test_edge_cases(ctx):
    rng = np.random.default_rng(27)
    rnd = lambda n: rng.integers(0, 256, (n, 32), dtype=np.uint8)
    # zero jobs, zero sets
    r = ctx.match_batch(dict(row_ptr=np.zeros(1, np.int32), desc=np.zeros((0, 32), np.uint8)), [], [], "dense")
    assert len(r["nmatches"]) == 0 and len(r["match"]) == 0
    sb = mu.SetBuilder()
    e = sb.add(np.zeros((0, 32), np.uint8))
    x = rnd(1)
    one = sb.add(x)
    X = np.concatenate([x, mu.at_dist(x[0], 5, rng)[0][None], rnd(30)])
    s30 = sb.add(X)
    allskip = sb.add(X, np.ones(len(X), np.uint8))
    for a, b in ((e, s30), (s30, e), (e, e), (allskip, s30), (s30, allskip), (s30, one), (one, s30), (allskip, allskip)):
        sb.job(a, b)
    bt = sb.batch()
    for mode in ("dense", "knn2"):
        res, ref = _check(ctx, bt, mode)
        if mode == "dense":
            assert list(res["nmatches"][:5]) == [0, 0, 0, 0, 0] and res["nmatches"][7] == 0
        else:
            assert list(res["nmatches"][:3]) == [0, 0, 0] and res["nmatches"][5] == 0     # one-row train set: no match
            assert res["nmatches"][3] > 0                                               # KNN2 reads no skip flags
    # a set at the row limit, matched against itself and against a small set
    L = capi.MATCH_MAX_ROWS
    sb = mu.SetBuilder()
    big = sb.add(np.concatenate([rnd(L - 100), mu.flip(np.repeat(x, 100, 0), 0.04, rng)]), rng.random(L) < 0.2)
    sm = sb.add(np.concatenate([x, mu.flip(np.repeat(x, 10, 0), 0.04, rng), rnd(40)]))
    sb.job(big, big); sb.job(big, sm); sb.job(sm, big)
    bt = sb.batch()
    for mode in ("dense", "knn2"):
        _check(ctx, bt, mode)


def test_dense_job_with_an_empty_query_set_and_no_skip_flags(ctx):
    """No output row at all: the list, match and distance buffers of the call are the zero-sized ones."""
    desc = np.random.default_rng(28).integers(0, 256, (3, 32), dtype=np.uint8)
    r = ctx.match_batch(dict(row_ptr=np.array([0, 0, 3], np.int32), desc=desc), [0], [1], "dense")
    assert list(r["nmatches"]) == [0] and len(r["match"]) == 0 and list(r["offset"]) == [0, 0]


def test_invalid_arguments_are_rejected(ctx):
    rng = np.random.default_rng(29)
    sets = dict(row_ptr=np.array([0, 20, 35], np.int32), desc=rng.integers(0, 256, (35, 32), dtype=np.uint8))
    for mode, kw in (("dense", dict(dist_threshold=0.0)), ("dense", dict(dist_threshold=float("nan"))), ("knn2", dict(ratio=0.0)),
                     ("knn2", dict(ratio=float("inf"))), ("knn2", dict(dist_threshold=-1.0)), (7, {})):
        with pytest.raises(backend.CovGpuError, match="covgpu_match_batch"):
            ctx.match_batch(sets, [0], [1], mode, **kw)
    with pytest.raises(backend.CovGpuError, match="monotone"):
        ctx.match_batch(dict(sets, row_ptr=np.array([0, 30, 20], np.int32)), [0], [1], "dense")
    with pytest.raises(backend.CovGpuError, match="out of range"):
        ctx.match_batch(sets, [0], [2], "dense")
    with pytest.raises(backend.CovGpuError, match="skip"):
        ctx.match_batch(dict(sets, skip=np.zeros(35, np.uint8)), [0], [1], "knn2")
    L = capi.MATCH_MAX_ROWS
    big = dict(row_ptr=np.array([0, L + 1, L + 11], np.int32), desc=rng.integers(0, 256, (L + 11, 32), dtype=np.uint8))
    with pytest.raises(backend.CovGpuError, match="MAX_ROWS"):
        ctx.match_batch(big, [1], [1], "knn2")
    o = capi.MatchOpts(); backend.lib().covgpu_default_match_opts(C.byref(o), capi.MATCH_DENSE)
    s = capi.MatchBatch(); s.num_sets = 2; s.num_jobs = 1
    assert backend.lib().covgpu_match_batch(ctx._h, C.byref(s), C.byref(o)) != 0      # NULL arrays
    assert b"NULL" in backend.lib().covgpu_last_error()
    s.num_jobs = -1; s.num_sets = 0
    assert backend.lib().covgpu_match_batch(ctx._h, C.byref(s), C.byref(o)) != 0
    assert backend.lib().covgpu_match_batch(None, C.byref(s), C.byref(o)) != 0                 # NULL context: checked, not dereferenced
    assert b"NULL context" in backend.lib().covgpu_last_error()


def _pose(p7):
    T = np.eye(4); T[:3, :3] = Rot.from_quat(p7[:4]).as_matrix(); T[:3, 3] = p7[4:]
    return T


def test_chain_dense_abspose_relpose_recovers_the_relative_pose(ctx, small):
    """ComputeSE3 on the GPU: DENSE matches of a query keyframe against map candidates (with distractor rows) -> the P3P RANSAC on
    (query bearing, candidate landmark) -> OptimizeRelativePose from the RANSAC's T12 = Twc1^-1 Twc2 (placerec_be.cpp:142)."""
    from tests import abspose_ref as ar
    from tests import abspose_util as au
    m = small
    bt = mu.map_batch(m, 12, seed=31)
    res = _run(ctx, bt, "dense")
    obs_of = {}
    for l in range(m.L):
        for o in range(m.lm_obs_ptr[l], m.lm_obs_ptr[l + 1]):
            obs_of[(int(m.obs_kf[o]), l)] = o
    Twc = lambda k: _pose(m.kf_pose[k]) @ _pose(m.cam_extr[int(m.kf_cam[k])])
    cands, jobs = [], []
    for j, (q, c) in enumerate(zip(bt["set_a"], bt["set_b"])):
        q, c = int(q), int(c)
        lists = mr.from_rows(res["match"][res["offset"][j]:res["offset"][j + 1]], res["dist"][res["offset"][j]:res["offset"][j + 1]], "dense")
        if len(lists) < 25:                                               # matches_thres
            continue
        a_idx = np.array([a for a, _, _ in lists]); b_idx = np.array([b for _, b, _ in lists])
        lA, lB = bt["lm_of_row"][q][a_idx], bt["lm_of_row"][c][b_idx]
        assert np.all(lA >= 0) and np.all(lB >= 0)
        assert np.mean(lA == lB) > 0.95
        cam = int(m.kf_cam[q]); intr, dist = m.cam_intr[cam], m.cam_dist[cam]
        uvA = np.array([m.obs_uv[obs_of[(q, int(l))]] for l in lA], np.float64)
        cands.append(dict(q=q, c=c, lA=lA, lB=lB, uvA=uvA, b_idx=b_idx,
                          bearing=au.bearings(au.undistort_radtan(uvA, intr, dist), intr), point_w=m.lm_pos[lB]))
        jobs.append(j)
    assert len(cands) >= 6
    ptr = np.zeros(len(cands) + 1, np.int32); ptr[1:] = np.cumsum([len(x["lA"]) for x in cands])
    cam0 = m.cam_intr[0]
    ab = dict(ptr=ptr, bearing=np.concatenate([x["bearing"] for x in cands]), point_w=np.concatenate([x["point_w"] for x in cands]),
              sigma_angle=np.concatenate([ar.sigma_angle(np.zeros(len(x["lA"])), cam0[0], cam0[1]) for x in cands]),
              seed=np.arange(len(cands), dtype=np.uint64) * 977 + 5)
    ra = ctx.abspose_ransac_batch(ab)
    assert np.all(ra["inliers"] > 0)
    rel = dict(ptr=[0], pA=[], pB=[], kpA=[], kpB=[], sigA=[], sigB=[], T0=[], Ttrue=[])
    for i, x in enumerate(cands):
        T1 = _pose(ra["T_wc"][i])
        assert np.linalg.norm(T1[:3, 3] - Twc(x["q"])[:3, 3]) < 0.3
        T12 = np.linalg.inv(T1) @ Twc(x["c"])
        Tt = np.linalg.inv(Twc(x["q"])) @ Twc(x["c"])
        keep = np.flatnonzero(ra["inlier"][ptr[i]:ptr[i + 1]])
        lA, lB = x["lA"][keep], x["lB"][keep]
        inv = lambda T: np.linalg.inv(T)
        rel["pA"].append((inv(Twc(x["q"])) @ np.c_[m.lm_pos[lA], np.ones(len(lA))].T).T[:, :3])
        rel["pB"].append((inv(Twc(x["c"])) @ np.c_[m.lm_pos[lB], np.ones(len(lB))].T).T[:, :3])
        rel["kpA"].append(x["uvA"][keep]); rel["kpB"].append(np.array([m.obs_uv[obs_of[(x["c"], int(l))]] for l in lB], np.float64))
        rel["sigA"].append(np.full(len(keep), 1.0)); rel["sigB"].append(np.full(len(keep), 1.0))
        q = Rot.from_matrix(T12[:3, :3]).as_quat(); rel["T0"].append(np.concatenate([q if q[3] >= 0 else -q, T12[:3, 3]]))
        rel["Ttrue"].append(Tt)
        rel["ptr"].append(rel["ptr"][-1] + len(keep))
    n = len(cands)
    camv = np.concatenate([m.cam_intr[0], m.cam_dist[0]])
    rb = dict(ptr=np.array(rel["ptr"], np.int32), pA=np.concatenate(rel["pA"]), pB=np.concatenate(rel["pB"]), kpA=np.concatenate(rel["kpA"]),
              kpB=np.concatenate(rel["kpB"]), sigA=np.concatenate(rel["sigA"]), sigB=np.concatenate(rel["sigB"]), camA=np.tile(camv, (n, 1)),
              camB=np.tile(camv, (n, 1)), distA=np.full(n, int(m.cam_dist_type[0]), np.int32), distB=np.full(n, int(m.cam_dist_type[0]), np.int32), T0=np.array(rel["T0"]))
    T, _, inl = ctx.relpose_batch(rb, th_outlier=1.3, min_inliers=12)
    for i in range(n):
        assert inl[i] > 0
        Tt = rel["Ttrue"][i]
        assert np.linalg.norm(T[i, 4:] - Tt[:3, 3]) < 0.1
        assert np.rad2deg(Rot.from_matrix(Rot.from_quat(T[i, :4]).as_matrix().T @ Tt[:3, :3]).magnitude()) < 1.0


# ------------------------------------------------------------------------------------------------ C++ facade
@pytest.mark.parametrize("mode", [0, 1])
def test_facade_matcher_equals_the_python_route(ctx, small, mode):
    """LoopMatcherT (tests/cpp/facade_match_shim.cpp): one query keyframe against five candidates, descriptors and row landmarks
    through the optional traits; mode 0 = MatchLandmarksBatch (DENSE over descriptors_), 1 = MatchImagesBatch (KNN2 over
    descriptors_add_, the same rows here)."""
    from tests import facade_util
    from tests.test_match_host import match_shim
    lib = match_shim()
    saved = facade_util._LIB
    facade_util._LIB = lib
    try:
        sm = facade_util.StandinMap(small)
    finally:
        facade_util._LIB = saved
    try:
        bt = mu.map_batch(small, 1, seed=33)
        q = int(bt["set_a"][0])
        cands = [c for c in range(max(0, q - 3), min(small.K, q + 4)) if c != q][:5]
        for k in [q] + cands:
            d, _ = mu.rows(bt, k)
            lm = bt["lm_of_row"][k].astype(np.int32).copy()
            lm[(lm >= 0) & bt["skip"][bt["row_ptr"][k]:bt["row_ptr"][k + 1]].astype(bool)] = -2    # invalid landmarks
            d = np.ascontiguousarray(d)
            lib.match_set_descriptors(sm.h, k, mode, len(d), d.ctypes.data_as(C.POINTER(C.c_uint8)), 1 if mode == 0 else 0,
                                      lm.ctypes.data_as(C.POINTER(C.c_int)))
        cand = np.array(cands, np.int32)
        counts = np.zeros(len(cands), np.int32)
        cap = C.c_int(200000)
        tri = np.zeros(3 * cap.value, np.int32)
        total = lib.match_candidates(sm.h, q, len(cands), cand.ctypes.data_as(C.POINTER(C.c_int)), mode,
                                     counts.ctypes.data_as(C.POINTER(C.c_int)), tri.ctypes.data_as(C.POINTER(C.c_int)), C.byref(cap))
        assert total == cap.value == counts.sum() and total > 0
        name = "dense" if mode == 0 else "knn2"
        sets = dict(row_ptr=bt["row_ptr"], desc=bt["desc"], skip=bt["skip"] if mode == 0 else None)
        res = ctx.match_batch(sets, np.full(len(cands), q, np.int32), cand, name)
        got = tri[:3 * total].reshape(-1, 3)
        pos = 0
        for j in range(len(cands)):
            want = mr.from_rows(res["match"][res["offset"][j]:res["offset"][j + 1]], res["dist"][res["offset"][j]:res["offset"][j + 1]], name)
            assert [tuple(int(v) for v in t) for t in got[pos:pos + counts[j]]] == want, j
            assert counts[j] == res["nmatches"][j]
            pos += counts[j]
    finally:
        sm.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_facade_default_path_equals_the_python_route(ctx, small, mode):
    """LoopMatcherT on COVINS-shaped classes without traits (tests/cpp/facade_match_covins_like.cpp): descriptors from the
    descriptors_ / descriptors_add_ members, skip flags from the non-const GetLandmark(k) / IsInvalid()."""
    from tests.test_match_host import covins_like_lib
    lib = covins_like_lib()
    bt = mu.map_batch(small, 1, seed=35)
    q = int(bt["set_a"][0])
    ks = [q] + [c for c in range(max(0, q - 3), min(small.K, q + 4)) if c != q][:4]
    desc = np.ascontiguousarray(np.concatenate([mu.rows(bt, k)[0] for k in ks]))
    lm = np.concatenate([np.where(bt["lm_of_row"][k] < 0, 0, np.where(mu.rows(bt, k)[1], 2, 1)) for k in ks]).astype(np.uint8)
    ptr = np.zeros(len(ks) + 1, np.int32); ptr[1:] = np.cumsum([int(bt["row_ptr"][k + 1] - bt["row_ptr"][k]) for k in ks])
    counts = np.zeros(len(ks) - 1, np.int32)
    cap = C.c_int(200000)
    tri = np.zeros(3 * cap.value, np.int32)
    total = lib.match_covins_like(len(ks), ptr.ctypes.data_as(C.POINTER(C.c_int)), desc.ctypes.data_as(C.POINTER(C.c_uint8)),
                                  lm.ctypes.data_as(C.POINTER(C.c_uint8)), mode, counts.ctypes.data_as(C.POINTER(C.c_int)),
                                  tri.ctypes.data_as(C.POINTER(C.c_int)), C.byref(cap))
    assert total == cap.value == counts.sum() and total > 0
    name = "dense" if mode == 0 else "knn2"
    got = tri[:3 * total].reshape(-1, 3)
    pos = 0
    for j, c in enumerate(ks[1:]):
        A, sA = mu.rows(bt, q); B, sB = mu.rows(bt, c)
        want = mr.dense(A, B, sA, sB) if mode == 0 else mr.knn2(A, B)
        assert [tuple(int(v) for v in t) for t in got[pos:pos + counts[j]]] == want, j
        pos += counts[j]
