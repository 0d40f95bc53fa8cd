"""covgpu_search_se3_batch / covgpu_search_projection_batch (k_guided.hip) on the GPU against the numpy restatement
(tests/guided_ref.py): map-derived jobs in both configurations, the hand-built cases in both visiting orders, batch independence, edge
cases and argument validation, the chain DENSE -> P3P RANSAC -> SearchBySE3 -> OptimizeRelativePose on device outputs, and the C++
facade. Fragile points (guided_ref's module doc) are left out of the comparisons; tests/test_guided_host.py caps their share."""
import ctypes as C

import numpy as np
import pytest
from scipy.spatial.transform import Rotation as Rot

from covins_amd import backend, capi
from tests import guided_ref as gr
from tests import guided_util as gu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = backend.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("agreement", [0, 1])
@pytest.mark.parametrize("config", ["ref", "pyr"])
def test_map_se3_jobs_equal_the_restatement(ctx, config, agreement):
    case = gu.map_se3_case(config)
    out = gu.run_se3(ctx, case, agreement=agreement)
    nf, frag, ev = gu.check_se3(out, gu.ref_se3(case), agreement)
    m1 = int((out["match1"] >= 0).sum()); m2 = int((out["match2"] >= 0).sum())
    print(f"{config} agreement {agreement}: 64 jobs, nfound per job median {np.median(nf):.0f} max {max(nf)} sum {sum(nf)}; "
          f"one-direction matches {m1} + {m2}; fragile {frag} of {ev} evaluated points")
    assert sum(nf) > 0 and m1 > 0 and m2 > 0


@pytest.mark.parametrize("config", ["ref", "pyr"])
def test_map_projection_jobs_equal_the_restatement(ctx, config):
    case = gu.map_projection_case(config)
    out, ptr = gu.run_projection(ctx, case)
    nm, frag, ev = gu.check_projection(out, ptr, gu.ref_projection(case))
    print(f"{config}: 16 jobs, {int(ptr[-1])} points, nmatches per job median {np.median(nm):.0f}, remap proposals "
          f"{int((out['remap_to'] >= 0).sum())}; fragile {frag} of {ev} evaluated points")
    assert sum(nm) > 0 and (out["remap_to"] >= 0).any()


@pytest.mark.parametrize("agreement", [0, 1])
@pytest.mark.parametrize("grid", [False, True])
def test_adversarial_se3_cases(ctx, grid, agreement):
    for case in gu.adversarial_se3(grid):
        out = gu.run_se3(ctx, case, agreement=agreement)
        gu.check_se3(out, gu.ref_se3(case), agreement, exact=True)


@pytest.mark.parametrize("grid", [False, True])
def test_adversarial_projection_cases(ctx, grid):
    for case in gu.adversarial_projection(grid):
        out, ptr = gu.run_projection(ctx, case)
        gu.check_projection(out, ptr, gu.ref_projection(case), exact=True)
        if case["name"] == "cluster":                                   # the truncated-list rescan ran and found the last four keypoints
            assert sorted(out["claimed"][:12].tolist()) == list(range(12)) and np.all(out["claimed"][12:] == -1)


def test_se3_job_alone_in_a_batch_and_permuted(ctx):
    case = gu.map_se3_case("pyr")
    jobs = case["jobs"][:12]
    whole = gu.run_se3(ctx, case, jobs)
    rows = lambda o, j, k="match", off="offset": o[k][o[off][j]:o[off][j + 1]]
    for j in (0, 5, 11):
        one = gu.run_se3(ctx, case, [jobs[j]])
        np.testing.assert_array_equal(one["match"], rows(whole, j))
        np.testing.assert_array_equal(one["match2"], rows(whole, j, "match2", "offset2"))
        assert one["nfound"][0] == whole["nfound"][j]
    perm = np.random.default_rng(3).permutation(len(jobs))
    shuf = gu.run_se3(ctx, case, [jobs[i] for i in perm])
    for k, i in enumerate(perm):
        np.testing.assert_array_equal(rows(shuf, k), rows(whole, i))
        np.testing.assert_array_equal(rows(shuf, k, "match1"), rows(whole, i, "match1"))
        assert shuf["nfound"][k] == whole["nfound"][i]


def test_projection_job_alone_in_a_batch_and_permuted(ctx):
    case = gu.map_projection_case("pyr")
    jobs = case["jobs"][:6]
    whole, ptr = gu.run_projection(ctx, case, jobs)
    keys = ("claimed", "remap_to", "best_dist")
    for j in (0, 3, 5):
        one, _ = gu.run_projection(ctx, case, [jobs[j]])
        for k in keys:
            np.testing.assert_array_equal(one[k], whole[k][ptr[j]:ptr[j + 1]])
        assert one["nmatches"][0] == whole["nmatches"][j]
    perm = [4, 0, 5, 2, 1, 3]
    shuf, sptr = gu.run_projection(ctx, case, [jobs[i] for i in perm])
    for k, i in enumerate(perm):
        for key in keys:
            np.testing.assert_array_equal(shuf[key][sptr[k]:sptr[k + 1]], whole[key][ptr[i]:ptr[i + 1]])
        assert shuf["nmatches"][k] == whole["nmatches"][i]


def _big_kf(n, rng):
    """n keypoints on integer pixels, every row a free landmark on its own keypoint with the keypoint's descriptor."""
    kp = np.stack([np.arange(n) % 640, (np.arange(n) // 640) * 7 + 5], 1).astype(np.float64)
    d = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    return gu._kf(kp, desc=d, lm_pos=gu._at(kp), lm_desc=d, lm_free=np.ones(n))


def test_edge_cases_and_validation(ctx):
    rng = np.random.default_rng(5)
    case = gu.adversarial_se3(False)[1]
    empty = gu._kf(np.zeros((0, 2)), desc=np.zeros((0, 32)))
    # zero jobs; an empty keypoint set on either side; all rows non-free
    out = gu.run_se3(ctx, case, [])
    assert len(out["match"]) == 0 and len(out["nfound"]) == 0
    c2 = dict(kfs=case["kfs"] + [empty], jobs=[(0, 2, gu.IDENT), (2, 0, gu.IDENT), (2, 2, gu.IDENT)], opts={})
    out = gu.run_se3(ctx, c2)
    gu.check_se3(out, gu.ref_se3(c2), 0, exact=True)
    assert np.all(out["match"] == -1) and np.all(out["nfound"] == 0) and len(out["match"]) == 3
    locked = [dict(k, lm_free=np.zeros(len(k["kp"]), np.uint8)) for k in case["kfs"]]
    out = gu.run_se3(ctx, dict(kfs=locked, jobs=case["jobs"], opts={}))
    assert np.all(out["match"] == -1) and np.all(out["match1"] == -1) and np.all(out["match2"] == -1) and out["nfound"][0] == 0
    # 4096 rows accepted (every landmark finds its own keypoint: two tiles per direction and more), 4097 refused
    L = capi.MATCH_MAX_ROWS
    big = _big_kf(L, rng)
    out = gu.run_se3(ctx, dict(kfs=[big], jobs=[(0, 0, gu.IDENT)], opts={}))
    np.testing.assert_array_equal(out["match"], np.arange(L))
    assert out["nfound"][0] == L
    with pytest.raises(backend.CovGpuError, match="MAX_ROWS"):
        gu.run_se3(ctx, dict(kfs=[_big_kf(L + 1, rng)], jobs=[(0, 0, gu.IDENT)], opts={}))
    for bad in (dict(radius=0.0), dict(radius=-1.0), dict(radius=float("nan")), dict(num_octaves=0), dict(th_low=-1), dict(agreement=2)):
        with pytest.raises(backend.CovGpuError):
            gu.run_se3(ctx, case, **bad)
    with pytest.raises(backend.CovGpuError, match="set index"):
        gu.run_se3(ctx, case, [(0, 5, gu.IDENT)])
    # PROJECTION: zero jobs, an empty point list, an empty keypoint set, the row limit, radius <= 0, existing_idx out of range
    pc = gu.adversarial_projection(False)[0]
    out, _ = gu.run_projection(ctx, pc, [])
    assert len(out["claimed"]) == 0 and len(out["nmatches"]) == 0
    none = gu._pts(np.zeros((0, 2)), np.zeros((0, 32)))
    c3 = dict(kfs=pc["kfs"] + [empty], jobs=[(0, gu.IDENT, none), (1, gu.IDENT, pc["jobs"][0][2]), pc["jobs"][0]], opts={})
    out, ptr = gu.run_projection(ctx, c3)
    gu.check_projection(out, ptr, gu.ref_projection(c3), exact=True)
    assert out["nmatches"].tolist() == [0, 0, 12]
    pts = gu._pts(big["kp"][:600], big["desc"][:600])
    out, ptr = gu.run_projection(ctx, dict(kfs=[big], jobs=[(0, gu.IDENT, pts)], opts={}))
    np.testing.assert_array_equal(out["claimed"], np.arange(600))
    with pytest.raises(backend.CovGpuError, match="MAX_ROWS"):
        gu.run_projection(ctx, dict(kfs=[_big_kf(L + 1, rng)], jobs=[(0, gu.IDENT, pts)], opts={}))
    for bad in (dict(radius=0.0), dict(radius=-3.0), dict(num_octaves=0)):
        with pytest.raises(backend.CovGpuError):
            gu.run_projection(ctx, pc, **bad)
    wrong = dict(pc["jobs"][0][2]); wrong["existing_idx"] = np.full(40, 12, np.int32)
    with pytest.raises(backend.CovGpuError, match="existing_idx"):
        gu.run_projection(ctx, pc, [(0, gu.IDENT, wrong)])
    # NULL arrays and a NULL context are refused before any device work
    o = capi.GuidedOpts(); backend.lib().covgpu_default_guided_opts(C.byref(o), capi.GUIDED_SE3)
    s = capi.SearchSe3Batch(); s.sets.num_sets = 2; s.num_jobs = 1
    assert backend.lib().covgpu_search_se3_batch(ctx._h, C.byref(s), C.byref(o)) == 1
    assert b"NULL" in backend.lib().covgpu_last_error()
    assert backend.lib().covgpu_search_se3_batch(None, C.byref(s), C.byref(o)) == 1
    p = capi.SearchProjectionBatch(); p.sets.num_sets = 1; p.num_jobs = 1
    assert backend.lib().covgpu_search_projection_batch(ctx._h, C.byref(p), C.byref(o)) == 1
    assert backend.lib().covgpu_search_projection_batch(None, C.byref(p), C.byref(o)) == 1
    assert b"NULL context" in backend.lib().covgpu_last_error()


def _pose(p7):
    T = np.eye(4); T[:3, :3] = Rot.from_quat(p7[:4]).as_matrix(); T[:3, 3] = p7[4:]
    return T


def _pose7(T):
    q = Rot.from_matrix(T[:3, :3]).as_quat()
    return np.concatenate([q if q[3] >= 0 else -q, T[:3, 3]])


def test_chain_on_device_outputs(ctx):
    """ComputeSE3's stages 1-4 on device outputs, 32 small-map jobs: DENSE matches -> P3P RANSAC -> SearchBySE3 with T12 from the RANSAC
    pose (placerec_be.cpp:142) and the RANSAC inliers as matches12 -> OptimizeRelativePose over inliers + added pairs. The new stage runs
    with agreement = 1: the literal test of the reference compares rows of two unrelated keypoint orders and adds next to nothing."""
    from tests import abspose_ref as ar
    from tests import abspose_util as au
    m = gu.small_map()
    kfs, ex = gu.map_keyframes("ref")
    case0 = gu.map_se3_case("ref")
    pairs = [(q, c) for q, c, _ in case0["jobs"][:32]]
    used = sorted({k for p in pairs for k in p})
    idx = {k: i for i, k in enumerate(used)}
    ptr = np.zeros(len(used) + 1, np.int32); ptr[1:] = np.cumsum([len(kfs[k]["kp"]) for k in used])
    invalid = m.lm_invalid.astype(bool)
    skip = np.concatenate([(kfs[k]["lm"] < 0) | invalid[np.maximum(kfs[k]["lm"], 0)] for k in used])
    res = ctx.match_batch(dict(row_ptr=ptr, desc=np.concatenate([kfs[k]["desc"] for k in used]), skip=skip.astype(np.uint8)),
                          [idx[q] for q, _ in pairs], [idx[c] for _, c in pairs], "dense")
    Twc = lambda k: np.linalg.inv(kfs[k]["T_cw"])
    cands = []
    for j, (q, c) in enumerate(pairs):
        mt = res["match"][res["offset"][j]:res["offset"][j + 1]]
        a = np.flatnonzero(mt >= 0); b = mt[a]
        if len(a) < 25:                                                  # matches_thres
            continue
        cam = int(m.kf_cam[q]); intr, dist = m.cam_intr[cam], m.cam_dist[cam]
        uvA = kfs[q]["kp"][a].astype(np.float64)
        cands.append(dict(q=q, c=c, a=a, b=b, bearing=au.bearings(au.undistort_radtan(uvA, intr, dist), intr),
                          point_w=m.lm_pos[kfs[c]["lm"][b]]))
    assert len(cands) >= 8
    cptr = np.zeros(len(cands) + 1, np.int32); cptr[1:] = np.cumsum([len(x["a"]) for x in cands])
    cam0 = m.cam_intr[0]
    ra = ctx.abspose_ransac_batch(dict(ptr=cptr, bearing=np.concatenate([x["bearing"] for x in cands]),
                                       point_w=np.concatenate([x["point_w"] for x in cands]),
                                       sigma_angle=np.concatenate([ar.sigma_angle(np.zeros(len(x["a"])), cam0[0], cam0[1]) for x in cands]),
                                       seed=np.arange(len(cands), dtype=np.uint64) * 977 + 5))
    # the new stage: one keyframe pair per job with the job's own free flags (alreadyMatched1 / 2 from the RANSAC inliers, :313-324)
    s_kfs, jobs = [], []
    for i, x in enumerate(cands):
        assert ra["inliers"][i] > 0
        keep = np.flatnonzero(ra["inlier"][cptr[i]:cptr[i + 1]])
        x["ia"], x["ib"] = x["a"][keep], x["b"][keep]
        k1, k2 = dict(kfs[x["q"]]), dict(kfs[x["c"]])
        valid = lambda k: ((k["lm"] >= 0) & ~invalid[np.maximum(k["lm"], 0)])
        f1 = valid(k1); f1[x["ia"]] = False
        f2 = valid(k2); f2[x["ib"]] = False
        k1["lm_free"], k2["lm_free"] = f1.astype(np.uint8), f2.astype(np.uint8)
        s_kfs += [k1, k2]
        x["T12"] = _pose7(np.linalg.inv(_pose(ra["T_wc"][i])) @ Twc(x["c"]))
        jobs.append((2 * i, 2 * i + 1, x["T12"]))
    case = dict(kfs=s_kfs, jobs=jobs, opts=dict(gu.CONFIGS["ref"]))
    out = gu.run_se3(ctx, case, agreement=1)
    refs = gu.ref_se3(case)
    gu.check_se3(out, refs, 1)
    added = same = 0
    rel = dict(ptr=[0], pA=[], pB=[], kpA=[], kpB=[], T0=[])
    rel_ref = dict(ptr=[0], pA=[], pB=[], kpA=[], kpB=[], T0=[])
    identical = []
    for i, x in enumerate(cands):
        k1, k2 = s_kfs[2 * i], s_kfs[2 * i + 1]
        for o, dst in ((out["match"][out["offset"][i]:out["offset"][i + 1]], rel), (gr.agree(refs[i]["match1"], refs[i]["match2"], 1), rel_ref)):
            na = np.flatnonzero(o >= 0)
            a = np.concatenate([x["ia"], na]); b = np.concatenate([x["ib"], o[na]]).astype(np.int64)
            dst["pA"].append(k1["lm_pos"][a]); dst["pB"].append(k2["lm_pos"][b])
            dst["kpA"].append(k1["kp"][a].astype(np.float64)); dst["kpB"].append(k2["kp"][b].astype(np.float64))
            dst["T0"].append(x["T12"]); dst["ptr"].append(dst["ptr"][-1] + len(a))
            if dst is rel:
                added += len(na); same += int((k1["lm"][na] == k2["lm"][o[na]]).sum())
                x["na"] = na
        identical.append(np.array_equal(out["match"][out["offset"][i]:out["offset"][i + 1]], gr.agree(refs[i]["match1"], refs[i]["match2"], 1)))
    print(f"chain: {len(cands)} jobs, {added} added pairs, {added - same} ({(added - same) / max(added, 1):.2%}) join different landmarks; "
          f"{sum(identical)} jobs identical to the restatement's")
    assert added > 0 and added - same <= 0.05 * added
    n = len(cands)
    camv = np.concatenate([m.cam_intr[0], m.cam_dist[0]])

    def refine(r):
        C_ = r["ptr"][-1]
        rb = dict(ptr=np.array(r["ptr"], np.int32), pA=np.concatenate(r["pA"]), pB=np.concatenate(r["pB"]), kpA=np.concatenate(r["kpA"]),
                  kpB=np.concatenate(r["kpB"]), sigA=np.full(C_, 2.0), sigB=np.full(C_, 2.0), camA=np.tile(camv, (n, 1)), camB=np.tile(camv, (n, 1)),
                  distA=np.full(n, int(m.cam_dist_type[0]), np.int32), distB=np.full(n, int(m.cam_dist_type[0]), np.int32), T0=np.array(r["T0"]))
        return ctx.relpose_batch(rb, th_outlier=1.3, min_inliers=12)
    T, _, inl = refine(rel)
    Tr, _, inlr = refine(rel_ref)
    for i, x in enumerate(cands):
        assert inl[i] > 0
        if identical[i]:                                                 # the same correspondences: the same refinement
            np.testing.assert_allclose(T[i], Tr[i], rtol=0, atol=1e-9)
            assert inl[i] == inlr[i]
        Tt = kfs[x["q"]]["T_cw"] @ Twc(x["c"])
        assert np.linalg.norm(T[i, 4:] - Tt[:3, 3]) < 0.1
        assert np.rad2deg(Rot.from_matrix(Rot.from_quat(T[i, :4]).as_matrix().T @ Tt[:3, :3]).magnitude()) < 1.0


# ------------------------------------------------------------------------------------------------ C++ facade
@pytest.fixture(scope="module")
def standin():
    """The stand-in map of the small synthetic map behind tests/cpp/facade_guided_shim.cpp, with the "pyr" landmark extras."""
    from tests import facade_util
    lib = gu.guided_shim()
    saved = facade_util._LIB
    facade_util._LIB = lib
    try:
        sm = facade_util.StandinMap(gu.small_map())
    finally:
        facade_util._LIB = saved
    _, ex = gu.map_keyframes("pyr")
    keep = [np.ascontiguousarray(ex["lm_desc"]), np.ascontiguousarray(ex["lm_normal"]), np.ascontiguousarray(ex["lm_mind"]),
            np.ascontiguousarray(ex["lm_maxd"])]
    dp = C.POINTER(C.c_double)
    lib.guided_set_landmarks(sm.h, keep[0].ctypes.data_as(C.POINTER(C.c_uint8)), keep[1].ctypes.data_as(dp), keep[2].ctypes.data_as(dp),
                             keep[3].ctypes.data_as(dp))
    yield sm, lib
    sm.close()


def _set_keyframe(lib, sm, k, kf, row_lm):
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    kp = np.ascontiguousarray(kf["kp"], np.float32); lv = np.ascontiguousarray(kf["level"], np.int32)
    d = np.ascontiguousarray(kf["desc"], np.uint8); rl = np.ascontiguousarray(row_lm, np.int32)
    b = np.array(kf["bounds"], np.float64); g = np.array(kf["grid_inv"] if kf.get("grid_inv") else (0.0, 0.0), np.float64)
    lib.guided_set_keyframe(sm.h, k, len(kp), kp.ctypes.data_as(C.POINTER(C.c_float)), lv.ctypes.data_as(ip),
                            d.ctypes.data_as(C.POINTER(C.c_uint8)), rl.ctypes.data_as(ip), b.ctypes.data_as(dp), g.ctypes.data_as(dp))


@pytest.mark.parametrize("agreement", [0, 1])
def test_facade_search_by_se3_batch(standin, agreement):
    """LoopMatcherT::SearchBySE3Batch: matches12 on entry marks shared landmarks as already matched (both sides, :313-324); on return
    it holds kf2's landmark of every agreed row, as the restatement predicts."""
    sm, lib = standin
    m = gu.small_map()
    invalid = m.lm_invalid.astype(bool)
    case0 = gu.map_se3_case("pyr")
    kfs = case0["kfs"]
    jobs = case0["jobs"][:6]
    for k in sorted({k for j in jobs for k in j[:2]}):
        _set_keyframe(lib, sm, k, kfs[k], kfs[k]["lm"])
    rng = np.random.default_rng(9)
    s_kfs, s_jobs, m12 = [], [], []
    for q, c, T in jobs:
        k1, k2 = dict(kfs[q]), dict(kfs[c])
        row2 = {int(l): r for r, l in enumerate(k2["lm"]) if l >= 0}
        already = np.array([l >= 0 and int(l) in row2 and rng.random() < 0.5 for l in k1["lm"]])
        mm = np.where(already, k1["lm"], -1).astype(np.int32)              # matches12[i] = the shared landmark
        valid = lambda k: (k["lm"] >= 0) & ~invalid[np.maximum(k["lm"], 0)]
        f1 = valid(k1) & ~already
        f2 = valid(k2); f2[[row2[int(l)] for l in k1["lm"][already]]] = False
        k1["lm_free"], k2["lm_free"] = f1.astype(np.uint8), f2.astype(np.uint8)
        s_jobs.append((len(s_kfs), len(s_kfs) + 1, T)); s_kfs += [k1, k2]; m12.append(mm)
    case = dict(kfs=s_kfs, jobs=s_jobs, opts=dict(gu.CONFIGS["pyr"]))
    refs = gu.ref_se3(case)
    ptr = np.zeros(len(jobs) + 1, np.int32); ptr[1:] = np.cumsum([len(x) for x in m12])
    io = np.ascontiguousarray(np.concatenate(m12)); found = np.zeros(len(jobs), np.int32)
    ip = C.POINTER(C.c_int)
    k1s = np.array([j[0] for j in jobs], np.int32); k2s = np.array([j[1] for j in jobs], np.int32)
    T = np.ascontiguousarray(np.array([j[2] for j in jobs]))
    lib.guided_set_params(50, 1.2, 8, agreement)
    lib.guided_se3(sm.h, len(jobs), k1s.ctypes.data_as(ip), k2s.ctypes.data_as(ip), T.ctypes.data_as(C.POINTER(C.c_double)),
                   ptr.ctypes.data_as(ip), io.ctypes.data_as(ip), found.ctypes.data_as(ip), 9.5)
    total = 0
    for j, r in enumerate(refs):
        want_rows = gr.agree(r["match1"], r["match2"], agreement)
        want = np.where(want_rows >= 0, s_kfs[2 * j + 1]["lm"][np.maximum(want_rows, 0)], m12[j])
        ok = gr.se3_comparable(r, agreement)
        np.testing.assert_array_equal(io[ptr[j]:ptr[j + 1]][ok], want[ok], err_msg=f"job {j}")
        if not (r["fragile1"].any() or r["fragile2"].any()):
            assert found[j] == (want_rows >= 0).sum()
        total += int(found[j])
    assert total > 0 or agreement == 0


def test_facade_search_by_projection(standin):
    """LoopMatcherT::SearchByProjection: vpMatched gets the claims, the remap proposals go through RemapLandmark in point order; the
    stand-in keyframe's landmark rows and every landmark's feature index end as the restatement predicts."""
    sm, lib = standin
    m = gu.small_map()
    case0 = gu.map_projection_case("pyr")
    lib.guided_set_params(50, 1.2, 8, 0)
    done = 0
    for kf_i, T, pts0 in case0["jobs"]:
        kf = case0["kfs"][kf_i]
        k = kf["index"]                                                  # the map keyframe behind the job's copy
        rows = kf["lm_assoc"].astype(np.int32)
        taken = kf["taken"].astype(bool)
        ids = pts0["lm"]
        pts = dict(pts0)
        pts["skip"] = (m.lm_invalid[ids].astype(bool) | np.isin(ids, rows[taken])).astype(np.uint8)   # IsInvalid() or in spAlreadyFound
        r = gr.search_projection(kf, T, pts, **case0["opts"])
        if r["fragile"].any():
            continue
        _set_keyframe(lib, sm, k, kf, rows)
        matched = np.where(taken, rows, -1).astype(np.int32)
        want = matched.copy()
        want[r["claimed"][r["claimed"] >= 0]] = ids[r["claimed"] >= 0]
        fi = np.full(m.L, -1, np.int64); fi[rows[rows >= 0]] = np.flatnonzero(rows >= 0)
        wrows = rows.astype(np.int64).copy()
        for p in np.flatnonzero(r["remap_to"] >= 0):                       # Keyframe::RemapLandmark, keyframe_be.cpp:484-495
            now, to, l = int(pts["existing_idx"][p]), int(r["remap_to"][p]), int(ids[p])
            lm_new = wrows[to]
            wrows[now] = -1; wrows[to] = l
            fi[l] = to
            if lm_new >= 0:
                fi[lm_new] = -1
        ip = C.POINTER(C.c_int)
        pi = np.ascontiguousarray(ids, np.int32); Tc = np.ascontiguousarray(T, np.float64)
        nm = lib.guided_projection(sm.h, k, Tc.ctypes.data_as(C.POINTER(C.c_double)), len(pi), pi.ctypes.data_as(ip), len(matched),
                                   matched.ctypes.data_as(ip), 10.0)
        got_rows = np.zeros(len(rows), np.int32); got_fi = np.zeros(m.L, np.int32)
        lib.guided_get_keyframe(sm.h, k, len(rows), got_rows.ctypes.data_as(ip), got_fi.ctypes.data_as(ip))
        assert nm == r["nmatches"] and nm > 0 and (r["remap_to"] >= 0).any()
        np.testing.assert_array_equal(matched, want)
        np.testing.assert_array_equal(got_rows, wrows)
        np.testing.assert_array_equal(got_fi, fi)
        done += 1
        if done == 2:
            break
    assert done >= 1
