"""covgpu_fivept_ransac_batch / covgpu_fivept_solve_batch (k_fivept.hip) against the numpy restatement
tests/fivept_ref.py: the minimal solver's solution sets and chosen poses on noise-free and degenerate tuples, the RANSAC loop draw
for draw at every size where the kernel takes another path, each status, batch invariance, the chain from match_batch on a synthetic
map, and the C++ facade (RelPoseSolverT) against the flat calls bit for bit.

Tolerances: 10 s_E and 10 s_T, the measured spread of two host formulations (tests/fivept_util.py, tests/test_fivept_host.py); they
are computed again here, once per session. Measured on an MI355X: solutions of the 1992 separated tuples within 1.1e-5 of route
A's (s_E 1.1e-5: the spread is route A's own error, which the device shares with route B), chosen poses within 2.1e-7 rad."""
import math

import numpy as np
import pytest

from covins_amd import backend
from tests import fivept_ref as fr
from tests import fivept_util as fu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = backend.Context(0)
    yield c
    c.close()


def _pose_err(T, R, t):
    return max(fr.pose_error(fr.quat_to_rot(T[:4]), T[4:], R, t))


def test_solver_matches_route_a_on_separated_tuples(ctx):
    tp, y = fu.standard()
    out = ctx.fivept_solve_batch(tp["f1"], tp["f2"])
    assert np.all(np.isfinite(out["E"])) and np.all(np.isfinite(out["T"])) and out["nsol"].max() <= 10 and out["nsol"].min() >= 0
    worst_E = worst_T = worst_res = 0.0
    for i in range(len(tp["f1"])):
        Ed = [out["E"][i, k] for k in range(out["nsol"][i])]
        assert not np.any(out["E"][i, out["nsol"][i]:])
        for E in Ed:
            assert abs(np.linalg.norm(E) - math.sqrt(2.0)) < 1e-12 and E.ravel()[np.argmax(np.abs(E))] > 0
            worst_res = max(worst_res, fr.cubic_residual(E), fr.epipolar_residual(E, tp["f1"][i], tp["f2"][i]))
        if not y["sep"][i]:
            continue
        assert len(Ed) == len(y["A"][i]), (i, len(Ed), len(y["A"][i]))
        worst_E = max(worst_E, fr.match_sets(y["A"][i], Ed))
        k, R, t = y["chosen_A"][i]
        assert out["chosen"][i] >= 0
        worst_T = max(worst_T, _pose_err(out["T"][i], R, t))
        assert float(np.max(np.abs(Ed[out["chosen"][i]] - y["A"][i][k]))) <= 10 * y["s_E"]
    print(f"device against route A: E {worst_E:.3e} (s_E {y['s_E']:.3e})  pose {worst_T:.3e} (s_T {y['s_T']:.3e})  residual {worst_res:.3e} (route A {y['res_A']:.3e})")
    assert worst_E <= 10 * y["s_E"] and worst_T <= 10 * y["s_T"] and worst_res <= 10 * y["res_A"]


def test_solver_on_degenerate_tuples(ctx):
    """All bearings equal, pure rotation, planar scene, two repeated correspondences: the call returns, at most 10 solutions, nothing
    non-finite, and whatever is returned satisfies its epipolar equations and the ten cubics to 10x route A's largest residual."""
    _, y = fu.standard()
    f1, f2 = fu.degenerate(500)
    out = ctx.fivept_solve_batch(f1, f2)
    assert np.all(np.isfinite(out["E"])) and np.all(np.isfinite(out["T"])) and out["nsol"].max() <= 10 and out["nsol"].min() >= 0
    assert not out["nsol"][0::4].any() and not out["nsol"][3::4].any()      # rank-deficient samples have no solution
    assert np.all(out["chosen"][0::4] == -1) and not out["T"][0::4].any()
    assert out["nsol"][2::4].min() >= 1                                       # a planar scene is no degeneracy of five points
    worst = 0.0
    for i in range(500):
        assert -1 <= out["chosen"][i] < max(out["nsol"][i], 1) and (out["chosen"][i] >= 0 or out["nsol"][i] == 0 or not out["T"][i].any())
        for k in range(out["nsol"][i]):
            worst = max(worst, fr.cubic_residual(out["E"][i, k]), fr.epipolar_residual(out["E"][i, k], f1[i], f2[i]))
    print(f"degenerate tuples: largest residual {worst:.3e} (bound {10 * y['res_A']:.3e})")
    assert worst <= 10 * y["res_A"]


@pytest.fixture(scope="module")
def sized_jobs():
    """64 jobs over the sizes at which the kernel takes another path: below, at and above the sample size, the wave, the workgroup
    and the LDS staging cap; 10-60 % wrong matches; 50 iterations at most above 257."""
    cap = backend.fivept_limits()["stage_cap"]
    sizes = [0, 7, 8, 9, 63, 64, 65, 255, 256, 257, cap - 1, cap, cap + 1]
    rng = np.random.default_rng(64)
    small, large = [], []
    for k in range(64):
        n = sizes[k % len(sizes)]
        frac = float(rng.uniform(0.1, 0.6))
        if n > 257:
            large.append(fu.job(n, frac, 9000 + k, max_iterations=50))
        else:
            small.append(fu.job(n, frac, 9000 + k))
    return small, large


def _compare(ctx, jobs, y, **opts):
    bt = fu.batch(jobs)
    bt["T0"] = np.full((len(jobs), 7), 7.0)
    r = ctx.fivept_ransac_batch(bt, **opts)
    for b, j in enumerate(jobs):
        ref = j["ref"]
        s = slice(bt["ptr"][b], bt["ptr"][b + 1])
        got = (r["status"][b], r["inliers"][b], r["iterations"][b], r["best_draw"][b])
        assert got == (ref["status"], ref["inliers"], ref["iterations"], ref["best_draw"]), (b, len(j["f1"]), got)
        assert np.array_equal(r["inlier"][s], ref["mask"]), (b, len(j["f1"]))
        if ref["status"] == 0:
            assert _pose_err(r["T_12"][b], ref["R"], ref["t"]) <= 10 * y["s_T"]
            assert abs(np.linalg.norm(r["T_12"][b, :4]) - 1.0) < 1e-12 and abs(np.linalg.norm(r["T_12"][b, 4:]) - 1.0) < 1e-12
        else:
            assert np.all(r["T_12"][b] == 7.0)
    return r


def test_ransac_matches_the_replay_at_every_size(ctx, sized_jobs):
    _, y = fu.standard()
    small, large = sized_jobs
    _compare(ctx, small, y)
    _compare(ctx, large, y, max_iterations=50)
    assert {0, 1} <= {j["ref"]["status"] for j in small + large}


def test_every_status_is_reached(ctx):
    _, y = fu.standard()
    rng = np.random.default_rng(3)
    # 4: all wrong matches, 20 iterations (min_inliers 0: with the default 20 the few chance inliers would make it status 3, which
    # the reference tests first)
    j4 = fu.job(60, 1.0, 41, max_iterations=20, min_inliers=0)
    r = _compare(ctx, [j4], y, max_iterations=20, min_inliers=0)
    assert r["status"][0] == 4 and r["iterations"][0] >= 20
    r = _compare(ctx, [fu.job(60, 1.0, 41, max_iterations=20)], y, max_iterations=20)
    assert r["status"][0] == 3
    # 3: 15 true matches of 40
    j3 = fu.job(40, 25 / 40, 42)
    r = _compare(ctx, [j3], y)
    assert r["status"][0] == 3 and 0 < r["inliers"][0] < 20 and not r["inlier"].any()
    # 1: n = 7
    r = _compare(ctx, [fu.job(7, 0.0, 43)], y)
    assert r["status"][0] == 1 and r["inliers"][0] == 0 and r["best_draw"][0] == -1
    # 2: identical bearings: every draw fails, the loop stops after 10 max_iterations skipped draws
    a, b, _, _ = fu.scene(rng, 1)
    f1, f2 = np.repeat(a, 30, 0), np.repeat(b, 30, 0)
    ref = fr.ransac(f1, f2, 44, max_iterations=20)
    assert (ref["status"], ref["draws"], ref["iterations"]) == (2, 200, 0)
    r = _compare(ctx, [dict(f1=f1, f2=f2, seed=44, ref=ref)], y, max_iterations=20)
    assert r["status"][0] == 2 and r["iterations"][0] == 0 and r["best_draw"][0] == -1 and r["inliers"][0] == 0
    # 0
    r = _compare(ctx, [fu.job(120, 0.2, 45)], y)
    assert r["status"][0] == 0 and r["inliers"][0] >= 20


def test_a_job_does_not_depend_on_its_batch(ctx):
    jobs = [fu.job(n, o, 700 + k) for k, (n, o) in enumerate(((90, 0.2), (0, 0.0), (300, 0.35), (0, 0.0), (64, 0.3), (7, 0.0)))]
    keys = ("T_12", "inlier", "inliers", "status", "iterations", "best_draw")
    whole = ctx.fivept_ransac_batch(fu.batch(jobs))
    ptr = fu.batch(jobs)["ptr"]
    for b, j in enumerate(jobs):
        alone = ctx.fivept_ransac_batch(fu.batch([j]))
        s = slice(ptr[b], ptr[b + 1])
        assert alone["T_12"][0].tobytes() == whole["T_12"][b].tobytes()
        assert np.array_equal(alone["inlier"], whole["inlier"][s])
        assert all(alone[k][0] == whole[k][b] for k in keys[2:])
    # seed = NULL: job b runs with opts seed + b
    bt = fu.batch(jobs)
    del bt["seed"]
    base = ctx.fivept_ransac_batch(bt, seed=1000)
    for b, j in enumerate(jobs):
        one = fu.batch([j])
        del one["seed"]
        alone = ctx.fivept_ransac_batch(one, seed=1000 + b)
        explicit = ctx.fivept_ransac_batch(dict(fu.batch([j]), seed=np.array([1000 + b], np.uint64)))
        for got in (alone, explicit):
            assert got["T_12"][0].tobytes() == base["T_12"][b].tobytes() and np.array_equal(got["inlier"], base["inlier"][ptr[b]:ptr[b + 1]])
            assert all(got[k][0] == base[k][b] for k in keys[2:])
    # two empty jobs
    e = ctx.fivept_ransac_batch(dict(ptr=[0, 0, 0], bearing1=np.zeros((0, 3)), bearing2=np.zeros((0, 3))))
    assert list(e["status"]) == [1, 1] and not e["inliers"].any() and len(e["inlier"]) == 0
    assert len(ctx.fivept_ransac_batch(dict(ptr=[0], bearing1=np.zeros((0, 3)), bearing2=np.zeros((0, 3))))["status"]) == 0


def test_arguments_are_refused_before_any_device_work(ctx):
    with pytest.raises(backend.CovGpuError, match="covgpu_fivept_ransac_batch: corr_ptr not monotone"):
        ctx.fivept_ransac_batch(dict(ptr=[0, 9, 8], bearing1=np.ones((9, 3)), bearing2=np.ones((9, 3))))
    with pytest.raises(backend.CovGpuError, match="covgpu_fivept_ransac_batch: sigma not finite or not positive"):
        ctx.fivept_ransac_batch(dict(ptr=[0, 9], bearing1=np.ones((9, 3)), bearing2=np.ones((9, 3))), sigma=0.0)
    with pytest.raises(backend.CovGpuError, match="covgpu_fivept_solve_batch: non-finite bearing"):
        ctx.fivept_solve_batch(np.full((1, 8, 3), np.nan), np.ones((1, 8, 3)))
    assert len(ctx.fivept_solve_batch(np.zeros((0, 8, 3)), np.zeros((0, 8, 3)))["nsol"]) == 0


def test_every_entry_point_refuses_a_null_context():
    """(tests/test_gpu_batch_errors.py lists the entry points of batch.hip; these live in fivept.hip.)"""
    import ctypes as C
    from covins_amd import capi
    lib = backend.lib()
    o = capi.FiveptOpts()
    lib.covgpu_default_fivept_opts(C.byref(o))
    assert lib.covgpu_fivept_ransac_batch(None, C.byref(capi.FiveptBatch()), C.byref(o)) != 0
    assert lib.covgpu_last_error() == b"covgpu_fivept_ransac_batch: NULL context"
    assert lib.covgpu_fivept_solve_batch(None, 0, None, None, None, None, None, None) != 0
    assert lib.covgpu_last_error() == b"covgpu_fivept_solve_batch: NULL context"


# ---------------------------------------------------------------------------------------------- the chain and the facade
GRID_OPTS = dict(min_inliers=20, max_iterations=200, threshold=16.0)


@pytest.fixture(scope="module")
def grid(ctx):
    """The scene of fivept_util.grid_scene through match_batch in image mode (KNN2) on the 2 x 3 grids of its three candidates and
    through the flat five-point call with the facade's seeds: per candidate the cells' match lists, bearings and results."""
    import ctypes as C
    sc = fu.grid_scene()
    lib = fu.facade_shim()
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    h = lib.f5_build(11, sc["row_ptr"].ctypes.data_as(ip), sc["desc"].ctypes.data_as(C.POINTER(C.c_ubyte)), sc["bearing"].ctypes.data_as(dp),
                     sc["client"].ctypes.data_as(ip), sc["pred"].ctypes.data_as(ip), np.ascontiguousarray(sc["T_wc"]).ctypes.data_as(dp),
                     np.ascontiguousarray(sc["T_cw"]).ctypes.data_as(dp))
    b = sc["bearing"]
    unit = b / np.sqrt(b[:, 0] * b[:, 0] + b[:, 1] * b[:, 1] + b[:, 2] * b[:, 2])[:, None]     # the facade's order of operations
    cands = {2: (2, 3, 4), 5: (5, 6, 7), 8: (8, 9, 10)}
    out = {}
    for c, chain in cands.items():
        pairs = [(a, k) for a in (0, 1) for k in chain]
        m = ctx.match_batch(dict(row_ptr=sc["row_ptr"], desc=sc["desc"]), [p[0] for p in pairs], [p[1] for p in pairs], mode="knn2",
                            dist_threshold=40.0, ratio=0.8)
        cells = []
        for q, (a, k) in enumerate(pairs):
            mm = m["match"][m["offset"][q]:m["offset"][q + 1]]
            ia = np.flatnonzero(mm >= 0)
            assert len(ia) == m["nmatches"][q]
            idx = np.stack([ia, mm[ia]], 1).astype(np.int32)
            cells.append(dict(a=a, b=k, idx=idx, f1=unit[sc["row_ptr"][a] + idx[:, 0]], f2=unit[sc["row_ptr"][k] + idx[:, 1]],
                              seed=int(lib.f5_seed(h, a, k, q))))
        r = ctx.fivept_ransac_batch(fu.batch(cells), **GRID_OPTS)
        out[c] = dict(cells=cells, res=r, ptr=fu.batch(cells)["ptr"])
    yield dict(scene=sc, lib=lib, h=h, cands=out)
    lib.f5_free(h)


def test_chain_from_match_batch_recovers_the_relative_poses(grid):
    """Synthetic map -> match_batch (image mode) on the 2 x 3 grid -> five-point: every cell's T_12 within 10 e_truth of the map's true
    relative camera pose, e_truth being route A's own error against the truth on the same cells with the same seeds (keypoint noise)."""
    sc, g = grid["scene"], grid["cands"][2]
    errs_A, errs_D = [], []
    for q, cell in enumerate(g["cells"]):
        assert len(cell["idx"]) >= 100                                     # the matcher found the shared points
        T = sc["T_cw"][cell["a"]] @ sc["T_wc"][cell["b"]]                    # frame 2 in frame 1
        R, t = T[:3, :3], T[:3, 3] / np.linalg.norm(T[:3, 3])
        ref = fr.ransac(cell["f1"], cell["f2"], cell["seed"], **GRID_OPTS)
        assert ref["status"] == 0 and g["res"]["status"][q] == 0
        assert (g["res"]["iterations"][q], g["res"]["best_draw"][q], g["res"]["inliers"][q]) == (ref["iterations"], ref["best_draw"], ref["inliers"])
        errs_A.append(max(fr.pose_error(ref["R"], ref["t"], R, t)))
        errs_D.append(_pose_err(g["res"]["T_12"][q], R, t))
    e_truth = max(errs_A)
    print(f"chain: e_truth {e_truth:.3e} rad, device against the truth {max(errs_D):.3e} rad")
    assert e_truth < 0.2 and max(errs_D) <= 10 * e_truth


def test_facade_equals_the_flat_calls_bit_for_bit(grid):
    import ctypes as C
    lib, h, sc = grid["lib"], grid["h"], grid["scene"]
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    # computePose on the matches of cell (0, 0) of the good candidate (seed of cell 0), and on too few of them (not found, T untouched)
    g = grid["cands"][2]
    cell, res = g["cells"][0], g["res"]
    idx = np.ascontiguousarray(cell["idx"])
    T = np.full(16, -1.0); inl = np.zeros(len(idx), np.int32); n = C.c_int()
    assert lib.f5_compute_pose(h, cell["a"], cell["b"], len(idx), idx.ctypes.data_as(ip), 16.0, 20, 200, T.ctypes.data_as(dp), inl.ctypes.data_as(ip), C.byref(n)) == 1
    assert T.tobytes() == fu.pose_to_transform(res["T_12"][0]).ravel().tobytes()
    assert list(inl[:n.value]) == list(np.flatnonzero(res["inlier"][g["ptr"][0]:g["ptr"][1]])) and n.value == res["inliers"][0]
    T = np.full(16, -1.0)
    assert lib.f5_compute_pose(h, cell["a"], cell["b"], 7, idx.ctypes.data_as(ip), 16.0, 20, 200, T.ctypes.data_as(dp), inl.ctypes.data_as(ip), C.byref(n)) == 0
    assert np.all(T == -1.0) and n.value == 0
    # ComputePoseGrid: all three candidates in one call; 5 and 8 are the reference's early false
    cand = np.array([2, 5, 8], np.int32)
    cap = 20000
    ok = np.zeros(3, np.uint8); nm = np.zeros(18, np.int32); ni = np.zeros(18, np.int32); Ti = np.zeros((3, 16)); TF = np.zeros((3, 5, 4, 4))
    midx = np.zeros((cap, 2), np.int32); iidx = np.zeros(cap, np.int32)
    tot = lib.f5_grid(h, 0, 3, cand.ctypes.data_as(ip), 16.0, 20, 200, 20, 40.0, 0.8, ok.ctypes.data_as(C.POINTER(C.c_ubyte)), nm.ctypes.data_as(ip),
                      ni.ctypes.data_as(ip), Ti.ctypes.data_as(dp), TF.ctypes.data_as(dp), midx.ctypes.data_as(ip), iidx.ctypes.data_as(ip), cap)
    assert tot >= 0 and list(ok) == [1, 0, 0]
    few = [len(c["idx"]) for c in grid["cands"][5]["cells"]]
    assert min(few) < 20 and few.index(min(few)) in (2, 5)                       # too few matches against keyframe 7
    bad = grid["cands"][8]
    assert min(len(c["idx"]) for c in bad["cells"]) >= 20 and set(np.flatnonzero(bad["res"]["status"] != 0)) == {1, 4}   # the cells of keyframe 9 fail
    assert list(nm[:6]) == [len(c["idx"]) for c in g["cells"]] and list(ni[:6]) == list(res["inliers"])
    assert np.array_equal(midx[:tot], np.concatenate([c["idx"] for c in g["cells"]]))
    assert np.array_equal(iidx[:ni[:6].sum()], np.concatenate([np.flatnonzero(res["inlier"][g["ptr"][q]:g["ptr"][q + 1]]) for q in range(6)]))
    assert Ti[0].tobytes() == fu.pose_to_transform(res["T_12"][0]).ravel().tobytes()
    for k, kf in enumerate((0, 1)):
        assert np.allclose(TF[0, k], sc["T_cw"][0] @ sc["T_wc"][kf], rtol=0, atol=1e-14)
    for k, kf in enumerate((2, 3, 4)):
        assert np.allclose(TF[0, 2 + k], sc["T_cw"][2] @ sc["T_wc"][kf], rtol=0, atol=1e-14)
