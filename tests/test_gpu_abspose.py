"""covgpu_abspose_ransac_batch / covgpu_p3p_batch (k_abspose.hip) against the numpy restatement tests/abspose_ref.py:
P3P solution sets, the RANSAC loop draw for draw (iterations, the model's draw, inlier mask, T_wc), edge cases, argument validation, the
chain into covgpu_relpose_batch and the C++ facade's Se3Solver."""
import ctypes as C

import numpy as np
import pytest
from scipy.spatial.transform import Rotation as Rot

from covins_amd import backend, synth
from tests import abspose_ref as ar
from tests import abspose_util as au

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = backend.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def small():
    return synth.make_map(synth.config_named("small"))


def _R(q):
    return Rot.from_quat(q).as_matrix()


def _quads(rng, n):
    """n quadruples: 2/3 generic, 1/6 nearly collinear triples, 1/6 tiny triangles far away (near-degenerate)."""
    F = np.zeros((n, 4, 3)); P = np.zeros((n, 4, 3)); kind = np.zeros(n, int)
    for e in range(n):
        R = Rot.random(random_state=int(rng.integers(1 << 31))).as_matrix(); t = rng.normal(0, 2, 3)
        X = np.stack([rng.uniform(-2, 2, 4), rng.uniform(-2, 2, 4), rng.uniform(2, 8, 4)], 1)
        kind[e] = 0 if e % 6 < 4 else (1 if e % 6 == 4 else 2)
        if kind[e] == 1:
            X[2] = X[0] + (X[1] - X[0]) * rng.uniform(0.2, 0.8) + rng.normal(0, 1e-3, 3)
        elif kind[e] == 2:
            X = X[0] + rng.normal(0, 0.05, (4, 3))
        F[e] = X / np.linalg.norm(X, axis=1, keepdims=True); P[e] = X @ R.T + t
    return F, P, kind


def _sane(f, P):
    """Conditioning of a quadruple's quartic: every root at least 1e-2 (relative) from every other root."""
    A, _ = ar.grunert_coeffs(f, P)
    if not np.all(np.isfinite(A)) or A[0] == 0:
        return False
    r = np.roots(A)
    sc = max(1.0, np.abs(r).max())
    return all(abs(r[i] - r[j]) > 1e-2 * sc for i in range(len(r)) for j in range(i))


def test_p3p_batch_matches_the_numpy_restatement(ctx):
    rng = np.random.default_rng(0)
    F, P, kind = _quads(rng, 10000)
    T, ns, ch = ctx.p3p_batch(F, P)
    nmis, checked = 0, 0
    for e in range(len(F)):
        sols = ar.p3p(F[e], P[e])
        sane = _sane(F[e], P[e])
        if ns[e] != len(sols):
            nmis += 1
            assert kind[e] != 0 and not sane, (e, kind[e], ns[e], len(sols))
            continue
        c = ar.pick(sols, F[e, 3], P[e, 3])
        if not sane:
            continue
        assert ch[e] == c, e
        checked += 1
        if kind[e] != 0:    # a nearly collinear or tiny triangle fixes the pose to far less than 1e-9: counts and choice only
            continue
        for i, (Rr, tr) in enumerate(sols):
            assert np.abs(_R(T[e, i, :4]) - Rr).max() < 1e-9 and np.abs(T[e, i, 4:] - tr).max() < 1e-9, (e, i)
    print(f"p3p: {checked} quadruples compared, {nmis} near-degenerate ones with different solution counts")
    assert checked > 6500 and nmis <= 50, (checked, nmis)


def _check_parity(res, bt, opts=None):
    ptr = bt["ptr"]
    for b, r in enumerate(bt["ref"]):
        s = slice(int(ptr[b]), int(ptr[b + 1]))
        assert res["iterations"][b] == r["iterations"], (b, res["iterations"][b], r["iterations"])
        assert res["best_draw"][b] == r["best_draw"], b
        assert res["inliers"][b] == r["inliers"], b
        assert np.array_equal(res["inlier"][s], r["mask"]), b
        if r["inliers"] > 0:
            assert np.abs(_R(res["T_wc"][b, :4]) - r["R"]).max() < 1e-9 and np.abs(res["T_wc"][b, 4:] - r["t"]).max() < 1e-9, b


def test_ransac_batch_matches_the_numpy_restatement_on_map_candidates(ctx, small):
    bt = au.map_batch(small, 500, seed=3, outlier_range=(0.1, 0.6))
    res = ctx.abspose_ransac_batch(bt)
    _check_parity(res, bt)
    ok = res["inliers"] > 0
    assert ok.mean() > 0.95
    et = [np.linalg.norm(res["T_wc"][b, 4:] - bt["truth"][b][:3, 3]) for b in np.flatnonzero(ok)]
    er = [np.rad2deg(Rot.from_matrix(_R(res["T_wc"][b, :4]).T @ bt["truth"][b][:3, :3]).magnitude()) for b in np.flatnonzero(ok)]
    print(f"map candidates: pose vs the query's estimate: median {np.median(et):.3f} m {np.median(er):.2f} deg, max {max(et):.3f} m {max(er):.2f} deg")
    assert np.median(et) < 0.15 and np.median(er) < 1.5


def test_ransac_batch_recovers_the_true_pose(ctx):
    rng = np.random.default_rng(5)
    bt = au.random_batch(list(rng.integers(60, 600, 100)), seed=6, outlier_frac=0.4, px=0.5)
    res = ctx.abspose_ransac_batch(bt)
    _check_parity(res, bt)
    for b in range(100):
        assert res["inliers"][b] > 0
        assert np.linalg.norm(res["T_wc"][b, 4:] - bt["truth"][b][:3, 3]) < 0.1
        assert np.rad2deg(Rot.from_matrix(_R(res["T_wc"][b, :4]).T @ bt["truth"][b][:3, :3]).magnitude()) < 1.0


def test_edge_cases(ctx):
    empty = dict(ptr=np.zeros(1, np.int32), bearing=np.zeros((0, 3)), point_w=np.zeros((0, 3)), sigma_angle=np.zeros(0))
    r = ctx.abspose_ransac_batch(empty)
    assert len(r["inliers"]) == 0
    # n < 4, all outliers, a candidate above the LDS stage (5 000), max_iterations = 1
    bt = au.random_batch([0, 3, 50, 5000, 200], seed=7, outlier_frac=0.2)
    bt["point_w"][int(bt["ptr"][2]):int(bt["ptr"][3])] = np.random.default_rng(8).normal(0, 50, (50, 3))
    bt["ref"][2] = ar.ransac(bt["bearing"][3:53], bt["point_w"][3:53], bt["sigma_angle"][3:53], int(bt["seed"][2]))
    T0 = np.full((5, 7), 7.0)
    res = ctx.abspose_ransac_batch(dict(bt, T0=T0))
    _check_parity(res, bt)
    assert list(res["inliers"][:3]) == [0, 0, 0] and np.all(res["T_wc"][:3] == 7.0)
    assert res["inliers"][3] > 3000
    one = ctx.abspose_ransac_batch(bt, max_iterations=1)
    for b in range(2, 5):
        s = slice(int(bt["ptr"][b]), int(bt["ptr"][b + 1]))
        r = ar.ransac(bt["bearing"][s], bt["point_w"][s], bt["sigma_angle"][s], int(bt["seed"][b]), max_iterations=1)
        assert one["iterations"][b] == r["iterations"] <= 2 and one["best_draw"][b] == r["best_draw"] and one["inliers"][b] == r["inliers"]


def test_a_candidate_alone_equals_the_same_inside_a_batch(ctx, small):
    bt = au.map_batch(small, 300, seed=9, with_ref=False)
    full = ctx.abspose_ransac_batch(bt)
    for b in (0, 17, 299):
        s = slice(int(bt["ptr"][b]), int(bt["ptr"][b + 1]))
        alone = dict(ptr=np.array([0, s.stop - s.start], np.int32), bearing=bt["bearing"][s], point_w=bt["point_w"][s],
                     sigma_angle=bt["sigma_angle"][s], seed=bt["seed"][b:b + 1])
        r = ctx.abspose_ransac_batch(alone)
        assert r["iterations"][0] == full["iterations"][b] and r["best_draw"][0] == full["best_draw"][b]
        assert np.array_equal(r["inlier"], full["inlier"][s]) and np.array_equal(r["T_wc"][0], full["T_wc"][b])


def test_invalid_arguments_are_rejected(ctx):
    bt = au.random_batch([20, 20], seed=10, with_ref=False)
    for kw in (dict(max_iterations=0), dict(probability=1.0), dict(probability=0.0), dict(threshold=0.0), dict(threshold=float("inf"))):
        with pytest.raises(backend.CovGpuError, match="covgpu_abspose_ransac_batch"):
            ctx.abspose_ransac_batch(bt, **kw)
    with pytest.raises(backend.CovGpuError, match="monotone"):
        ctx.abspose_ransac_batch(dict(bt, ptr=np.array([0, 30, 20], np.int32)))
    bad = bt["bearing"].copy(); bad[3, 1] = np.nan
    with pytest.raises(backend.CovGpuError, match="non-finite"):
        ctx.abspose_ransac_batch(dict(bt, bearing=bad))
    from covins_amd import capi
    o = capi.RansacOpts(); backend.lib().covgpu_default_ransac_opts(C.byref(o))
    s = capi.AbsposeBatch(); s.num = -1
    assert backend.lib().covgpu_abspose_ransac_batch(ctx._h, C.byref(s), C.byref(o)) != 0
    s.num = 2
    assert backend.lib().covgpu_abspose_ransac_batch(ctx._h, C.byref(s), C.byref(o)) != 0   # NULL arrays
    assert b"NULL" in backend.lib().covgpu_last_error()


def test_chain_into_relpose_batch_converges_to_the_true_T12(ctx):
    """RANSAC's T_wc of the query (camera 1) against a candidate camera 2 with a known pose gives the T12 guess that covgpu_relpose_batch
    refines: T12 = Twc1^-1 Twc2 (placerec_be.cpp:142)."""
    from tests.util import make_relpose_batch
    rng = np.random.default_rng(11)
    rel = make_relpose_batch(40, seed=12, outlier_frac=0.1)
    Tt = rel["Ttrue"]
    cam = rel["camA"][0, :4]
    ptr = rel["ptr"]
    bts, T0 = [], []
    Twc2 = []
    for b in range(40):
        s = slice(int(ptr[b]), int(ptr[b + 1]))
        # camera 2 = B at a random world pose; world points = the B-frame landmarks moved into the world; bearings of A's keypoints
        Rw = Rot.random(random_state=int(rng.integers(1 << 31))).as_matrix(); tw = rng.normal(0, 3, 3)
        Tw2 = np.eye(4); Tw2[:3, :3] = Rw; Tw2[:3, 3] = tw
        Twc2.append(Tw2)
        uv = rel["kpA"][s]
        bts.append(dict(bearing=au.bearings(au.undistort_radtan(uv, rel["camA"][b, :4], rel["camA"][b, 4:]), rel["camA"][b, :4]),
                        point_w=rel["pB"][s] @ Rw.T + tw, sigma_angle=ar.sigma_angle(np.zeros(s.stop - s.start), cam[0], cam[1])))
    batch = dict(ptr=ptr, bearing=np.concatenate([x["bearing"] for x in bts]), point_w=np.concatenate([x["point_w"] for x in bts]),
                 sigma_angle=np.concatenate([x["sigma_angle"] for x in bts]), seed=np.arange(40, dtype=np.uint64) * 977)
    res = ctx.abspose_ransac_batch(batch)
    assert np.all(res["inliers"] > 0)
    for b in range(40):
        Twc1 = np.eye(4); Twc1[:3, :3] = _R(res["T_wc"][b, :4]); Twc1[:3, 3] = res["T_wc"][b, 4:]
        T12 = np.linalg.inv(Twc1) @ Twc2[b]                       # T_AB: camera B in camera A
        q = Rot.from_matrix(T12[:3, :3]).as_quat()
        T0.append(np.concatenate([q if q[3] >= 0 else -q, T12[:3, 3]]))
    T, out, inl = ctx.relpose_batch(dict(rel, T0=np.array(T0)), th_outlier=1.3, min_inliers=12)
    Tg, _, inlg = ctx.relpose_batch(rel, th_outlier=1.3, min_inliers=12)    # from the generator's own perturbed guess
    for b in range(40):
        assert inl[b] > 0
        assert np.linalg.norm(T[b, 4:] - Tt[b, 4:]) < 0.1
        assert np.rad2deg(Rot.from_matrix(_R(T[b, :4]).T @ _R(Tt[b, :4])).magnitude()) < 1.0
        if inlg[b] > 0:    # 5 + 5 dogleg iterations from two different starts end within millimetres of each other
            assert np.linalg.norm(T[b, 4:] - Tg[b, 4:]) < 1e-2


# ------------------------------------------------------------------------------------------------ C++ facade
def abspose_shim():
    """tests/cpp/facade_abspose_shim.cpp: the facade's Se3Solver on the stand-in map with the optional bearing trait (compiled here)."""
    from tests.test_abspose_host import abspose_shim as build
    return build()


def _facade_seed(m, q, c):
    M = (1 << 64) - 1
    ident = lambda k: 0 if k < 0 else ((int(m.kf_id[k]) << 20) ^ int(m.kf_client[k])) & M
    return (ident(q) * 0x9E3779B97F4A7C15 + ident(c)) & M


@pytest.mark.parametrize("cand", [-1, 5])
def test_facade_se3solver_equals_the_python_route(ctx, small, cand):
    from tests import facade_util
    lib = abspose_shim()
    saved = facade_util._LIB
    facade_util._LIB = lib
    try:
        sm = facade_util.StandinMap(small)
    finally:
        facade_util._LIB = saved
    try:
        rng = np.random.default_rng(13)
        q = 40
        obs = np.flatnonzero(small.obs_kf == q)
        lm_of_obs = np.searchsorted(small.lm_obs_ptr, obs, side="right") - 1
        a = int(small.kf_cam[q]); intr, dist = small.cam_intr[a], small.cam_dist[a]
        n = len(obs) + 30
        f = np.zeros((n, 3)); f[:, 2] = 1.0
        f[:len(obs)] = au.bearings(au.undistort_radtan(small.obs_uv[obs].astype(np.float64), intr, dist), intr)
        match = np.full(n, -1, np.int32)
        match[:len(obs)] = lm_of_obs
        wrong = rng.random(len(obs)) < 0.3
        match[:len(obs)][wrong] = rng.integers(small.L, size=int(wrong.sum()))
        match[rng.random(n) < 0.1] = -1                                # NULL matches
        octave = rng.integers(0, 4, n).astype(np.int32)
        nb = n - 5                                                    # bearings_ shorter than the match vector
        lib.abspose_set_features(sm.h, q, nb, f.ctypes.data_as(C.POINTER(C.c_double)), octave.ctypes.data_as(C.POINTER(C.c_int)))
        T = np.zeros(16); kept = np.zeros(n, np.uint8); seed = C.c_uint64(0)
        found = lib.abspose_align(sm.h, q, cand, n, match.ctypes.data_as(C.POINTER(C.c_int)), 25.0, 6, 300, T.ctypes.data_as(C.POINTER(C.c_double)),
                                  kept.ctypes.data_as(C.POINTER(C.c_ubyte)), C.byref(seed))
        assert seed.value == _facade_seed(small, q, cand)
        valid = (match >= 0) & ~small.lm_invalid[np.maximum(match, 0)]
        ind = np.flatnonzero(valid)                                   # Se3Solver's indMap
        use = ind[ind < nb]                                           # the adapter: i < min(bearings_.size(), matches.size())
        bt = dict(ptr=np.array([0, len(use)], np.int32), bearing=f[use], point_w=small.lm_pos[match[use]],
                  sigma_angle=ar.sigma_angle(octave[use], intr[0], intr[1]), seed=np.array([seed.value], np.uint64))
        res = ctx.abspose_ransac_batch(bt)
        assert found == 1 and res["inliers"][0] > 0
        want = np.zeros(n, np.uint8)
        want[ind[:len(use)][res["inlier"]]] = 1
        assert np.array_equal(kept, want)
        Tws = T.reshape(4, 4)
        assert np.abs(Tws[:3, :3] - _R(res["T_wc"][0, :4])).max() < 1e-12 and np.abs(Tws[:3, 3] - res["T_wc"][0, 4:]).max() == 0.0
        assert np.array_equal(Tws[3], [0, 0, 0, 1])
        # a failing candidate (min_inliers above the match count) leaves matches and Tws untouched
        T2 = np.zeros(16); kept2 = np.zeros(n, np.uint8)
        assert lib.abspose_align(sm.h, q, cand, n, match.ctypes.data_as(C.POINTER(C.c_int)), 25.0, n + 1, 300, T2.ctypes.data_as(C.POINTER(C.c_double)),
                                 kept2.ctypes.data_as(C.POINTER(C.c_ubyte)), C.byref(seed)) == 0
        assert np.all(T2 == -1.0) and np.array_equal(kept2.astype(bool), match >= 0)
    finally:
        sm.close()
