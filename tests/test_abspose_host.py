"""The numpy restatement of the loop-candidate geometric verification (tests/abspose_ref.py) on the CPU: its P3P, its
score against a line-by-line transcription of FrameAbsolutePoseSacProblem::getSelectedDistancesToModel, the RANSAC loop's semantics on
hand-built cases, and the sampler; plus the C ABI declarations."""
import ctypes as C
import math

import numpy as np
import pytest
from scipy.spatial.transform import Rotation as Rot

from covins_amd import capi
from tests import abspose_ref as ar


def _triple(rng, n=4):
    R = Rot.random(random_state=int(rng.integers(1 << 31))).as_matrix(); t = rng.normal(0, 2, 3)
    Xc = np.stack([rng.uniform(-2, 2, n), rng.uniform(-2, 2, n), rng.uniform(2, 8, n)], 1)
    return R, t, Xc / np.linalg.norm(Xc, axis=1, keepdims=True), Xc @ R.T + t


def test_p3p_contains_the_true_pose_and_reproduces_its_bearings():
    rng = np.random.default_rng(0)
    for _ in range(500):
        R, t, f, P = _triple(rng)
        sols = ar.p3p(f, P)
        assert min(np.abs(Rs - R).max() + np.abs(ts - t).max() for Rs, ts in sols) < 1e-9
        for Rs, ts in sols:
            b = (P[:3] - ts) @ Rs
            assert np.abs(b / np.linalg.norm(b, axis=1, keepdims=True) - f[:3]).max() < 1e-12
            assert np.all(np.sum(b * f[:3], axis=1) > 0)                   # positive depths
        assert sols[ar.pick(sols, f[3], P[3])][0] == pytest.approx(R, abs=1e-9)


def _triad(X, P):
    """The kernel's alignment (two orthonormal triads), restated: R, t with P = R X + t."""
    def frame(A):
        e1 = A[1] - A[0]; e1 /= np.linalg.norm(e1)
        w = A[2] - A[0]; e2 = w - e1 * (w @ e1); e2 /= np.linalg.norm(e2)
        return np.stack([e1, e2, np.cross(e1, e2)], 1)
    R = frame(P) @ frame(X).T
    return R, P.mean(0) - R @ X.mean(0)


def _ferrari_roots(A):
    """Real roots of the quartic the kernel's way (closed form, no numpy.roots), for the cross-check of the two formulations."""
    a, b, c, d = A[1] / A[0], A[2] / A[0], A[3] / A[0], A[4] / A[0]
    p = b - 3 * a * a / 8; q = c - a * b / 2 + a ** 3 / 8; r = d - a * c / 4 + a * a * b / 16 - 3 * a ** 4 / 256
    m = max(z.real for z in np.roots([1, p, p * p / 4 - r, -q * q / 8]) if abs(z.imag) < 1e-9)
    s = math.sqrt(2 * m); h = q / (2 * s)
    out = []
    for sg, hh in ((1, h), (-1, -h)):
        D = s * s - 4 * (m + p / 2 + hh)
        if D >= 0:
            out += [(sg * s + math.sqrt(D)) / 2 - a / 4, (sg * s - math.sqrt(D)) / 2 - a / 4]
    return sorted(out)


def test_two_p3p_formulations_give_the_same_solution_sets():
    rng = np.random.default_rng(1)
    for _ in range(300):
        R, t, f, P = _triple(rng)
        A, (ca, cb, cg, amc, a2, b2, c2) = ar.grunert_coeffs(f, P)
        sols = ar.p3p(f, P)
        other = []
        for v in _ferrari_roots(A):
            u = ((-1 + amc) * v * v - 2 * amc * cb * v + 1 + amc) / (2 * (cg - v * ca))
            qq = 1 + v * v - 2 * v * cb
            if v > 0 and u > 0 and qq > 0:
                s1 = math.sqrt(b2 / qq)
                s = ar.refine_depths(np.array([s1, u * s1, v * s1]), ca, cb, cg, a2, b2, c2)
                other.append(_triad(s[:, None] * f[:3], P[:3]))
        assert len(other) == len(sols)
        for (R1, t1), (R2, t2) in zip(sols, other):
            assert np.abs(R1 - R2).max() < 1e-9 and np.abs(t1 - t2).max() < 1e-9


def test_score_is_the_transcription_of_getSelectedDistancesToModel():
    rng = np.random.default_rng(2)
    R, t, f, P = _triple(rng, 50)
    R = Rot.from_matrix(R) * Rot.from_rotvec(rng.normal(0, 0.01, 3)); R = R.as_matrix(); t = t + rng.normal(0, 0.05, 3)
    sig = ar.sigma_angle(rng.integers(0, 4, 50), 458.654, 457.296)
    got = ar.score(R, t, f, P, sig)
    model = np.concatenate([R, t[:, None]], 1)                      # opengv transformation_t, 3x4
    inv = np.zeros((3, 4)); inv[:, :3] = model[:, :3].T; inv[:, 3] = -inv[:, :3] @ model[:, 3]
    for i in range(50):
        p_hom = np.append(P[i], 1.0)
        body = inv @ p_hom
        rep = np.eye(3).T @ (body - np.zeros(3))                     # getCamRotation = I, getCamOffset = 0
        rep = rep / np.linalg.norm(rep)
        err = rep - f[i]
        assert got[i] == pytest.approx((err @ err) / sig[i], rel=1e-14)
    s = 0.8 * (np.arange(4) + 1); fu = (458.654 + 457.296) / 2
    assert np.allclose(ar.sigma_angle(np.arange(4), 458.654, 457.296), math.sqrt(2) * s * s / (fu * fu), rtol=0, atol=0)


# ------------------------------------------------------------------------------------------------ loop semantics
def _loop(n, counts, **kw):
    """ransac() with a scripted hypothesis per draw: counts[d] = None (failed draw) or the number c of correspondences the model of
    draw d keeps (a stand-in score: 0 for the first c correspondences, 1e9 for the rest). Returns (result, draws made)."""
    f = np.tile([0.0, 0.0, 1.0], (n, 1)); P = np.tile([0.0, 0.0, 1.0], (n, 1)); sig = np.ones(n)
    seen = []

    def hyp(d, idx):
        seen.append(d)
        c = counts[d] if d < len(counts) else counts[-1]
        if c is None:
            return None
        return ("model", c)
    orig = ar.score
    ar.score = lambda R, t, f_, P_, s_: np.where(np.arange(len(f_)) < t, 0.0, 1e9) if isinstance(R, str) else orig(R, t, f_, P_, s_)
    try:
        r = ar.ransac(f, P, sig, 0, hypothesis=hyp, **kw)
    finally:
        ar.score = orig
    return r, seen


def test_loop_k_update_and_stop():
    n = 100
    r, seen = _loop(n, [50, 90], probability=0.99, max_iterations=300)
    k = math.log(0.01) / math.log(1 - 0.9 ** 4)                    # after draw 1
    assert r["best_draw"] == 1 and r["inliers"] == 90
    assert r["iterations"] == math.ceil(k) and len(seen) == math.ceil(k)


def test_failed_draws_do_not_count():
    r, seen = _loop(100, [None, None, 100], max_iterations=300)
    assert r["iterations"] == 1 and len(seen) == 3 and r["best_draw"] == 2


def test_stop_after_max_iterations_plus_one():
    r, seen = _loop(100, [5], max_iterations=7)                     # w = 0.05: k is huge
    assert r["iterations"] == 8 and len(seen) == 8 and r["best_draw"] == 0


def test_skip_limit_ends_the_loop_without_a_model():
    r, seen = _loop(100, [None], max_iterations=3)
    assert len(seen) == 30 and r["iterations"] == 0 and r["best_draw"] == -1 and r["inliers"] == 0


def test_fewer_than_four_correspondences_have_no_model():
    for n in range(4):
        r = ar.ransac(np.zeros((n, 3)), np.zeros((n, 3)), np.ones(n), 0)
        assert r["inliers"] == 0 and r["iterations"] == 0 and r["best_draw"] == -1 and r["R"] is None


def test_min_inliers_boundary():
    assert _loop(100, [6], max_iterations=2, min_inliers=6)[0]["inliers"] == 6
    r = _loop(100, [5], max_iterations=2, min_inliers=6)[0]
    assert r["inliers"] == 0 and not r["mask"].any()


def test_threshold_is_strict():
    rng = np.random.default_rng(3)
    R, t, f, P = _triple(rng, 20)
    sig = np.ones(20)
    sc = ar.score(R, t, f, P, sig)
    th = float(np.sort(sc)[10])
    assert int(np.sum(ar.score(R, t, f, P, sig) < th)) == 10      # the correspondence AT the threshold is out


# ------------------------------------------------------------------------------------------------ sampler
def test_sampler_draws_are_distinct_in_range_and_reproducible():
    rng = np.random.default_rng(4)
    for _ in range(2000):
        n = int(rng.integers(4, 5000)); s = int(rng.integers(1 << 64, dtype=np.uint64)); d = int(rng.integers(0, 3300))
        idx = ar.draw(s, d, n)
        assert len(set(idx)) == 4 and all(0 <= i < n for i in idx)
        assert ar.draw(s, d, n) == idx
    assert ar.draw(0, 0, 4) != ar.draw(1, 0, 4) or ar.draw(0, 1, 4) != ar.draw(1, 1, 4)
    assert sorted(ar.draw(7, 3, 4)) == [0, 1, 2, 3]
    assert ar.splitmix64(0) == 0xE220A8397B1DCDAF                 # the published first output of splitmix64 seeded with 0


def test_c_abi_structs_and_defaults_are_declared():
    assert C.sizeof(capi.AbsposeBatch) == 8 + 10 * 8                 # int32 num (padded), ten pointers
    assert C.sizeof(capi.RansacOpts) == 32
    from covins_amd import backend
    o = capi.RansacOpts()
    backend.lib().covgpu_default_ransac_opts(C.byref(o))
    assert (o.min_inliers, o.max_iterations, o.probability, o.threshold, o.seed) == (6, 300, 0.99, 25.0, 0)


_SHIM = None


def abspose_shim():
    """tests/cpp/facade_abspose_shim.cpp: the facade's Se3Solver instantiated on the stand-in map with the optional bearing trait."""
    global _SHIM
    if _SHIM is None:
        import os
        import subprocess
        here = os.path.dirname(os.path.abspath(__file__)); root = os.path.dirname(here)
        so = os.path.join(here, "cpp", "libfacade_abspose_shim.so")
        srcs = [os.path.join(here, "cpp", f) for f in ("facade_abspose_shim.cpp", "facade_shim.cpp", "standin_map.hpp")] + \
               [os.path.join(root, "include", "covins_gpu", "optimization_gpu.hpp"), os.path.join(root, "include", "covgpu.h")]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", srcs[0], "-o", so, "-L" + os.path.join(root, "covins_amd"),
                                   "-lcovgpu", "-Wl,-rpath," + os.path.join(root, "covins_amd")])
        lib = C.CDLL(so)
        lib.shim_build.restype = C.c_void_p
        lib.shim_free.argtypes = [C.c_void_p]
        lib.abspose_set_features.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int)]
        lib.abspose_align.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_double, C.c_int, C.c_int,
                                      C.POINTER(C.c_double), C.POINTER(C.c_ubyte), C.POINTER(C.c_uint64)]
        lib.abspose_align.restype = C.c_int
        _SHIM = lib
    return _SHIM


def test_facade_se3solver_compiles():
    """The facade's Se3Solver instantiates on the stand-in map (the GPU test drives it: tests/test_gpu_abspose.py)."""
    assert abspose_shim().abspose_align is not None
