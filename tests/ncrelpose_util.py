"""Builders for the tests of the 17-point batch: synthetic two-rig scenes, tuples for the solve entry point, jobs for
the whole call, and the yardsticks the device tests apply.

The scene: two rigs, 2 cameras on the query side and 3 on the candidate side (6 cells, query-major); per-axis camera offsets N(0, 0.3),
camera rotations of 0.1 rad, the first camera of each rig at the identity; relative rotation of up to 40 degrees, t ~ N(0, 0.5); depths
4-12 along bearings within 0.5 rad of the first camera's axis. A tuple is "separated" when sigma_17 / sigma_1 >= 1e-5.

Points of the device tests (tests/test_gpu_ncrelpose.py), and why:
  solve      N = 17 (the zero row), 18 (square), 24 (the covariance solve of 6 cells), 32 (a full lane pass of rows); 2000 tuples each,
             a count that is no multiple of the 8 tuples of a workgroup is covered by the degenerate batch of 4
  ransac     n = 0, 16 (status 1), 17 (one possible sample), 18, 63-65 and 255-257 (the 64-lane scoring loop's edges), cap-1, cap,
             cap+1 (the staged and the global-memory path), the rest 120-200; 10-25 % wrong matches, noise 1e-4..3e-4 rad
  statuses   a cell of 7 correspondences (4), cov_max_iters = cov_iters - 2 (5), cov_thres 1e-12 (6), 40 % wrong with min_inliers (3)
  batch      one job alone and inside 65; one job longer than the cap staged (stage_cap 0) and forced through global memory"""
import functools
import math

import numpy as np

from tests import ncrelpose_ref as nr

NQ, NC = 2, 3
SEP = 1e-5


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _rand_rot(rng, angle):
    return nr.exp_so3(_unit(rng.normal(size=3)) * angle)


def rig(rng):
    """cam [5,12] (R_c row-major | o_c; cameras 0, 1 on side 1, 2..4 on side 2), the true R, t, and the two extrinsics [7]"""
    cam = np.zeros((NQ + NC, 12))
    for i in range(NQ + NC):
        first = i in (0, NQ)
        cam[i, :9] = (np.eye(3) if first else _rand_rot(rng, 0.1)).ravel()
        cam[i, 9:] = 0.0 if first else rng.normal(0.0, 0.3, 3)
    R = _rand_rot(rng, rng.uniform(0.0, math.radians(40.0)))
    t = rng.normal(0.0, 0.5, 3)
    Tq = nr.pose7(_rand_rot(rng, 0.3), rng.normal(0.0, 0.1, 3))
    Tc = nr.pose7(_rand_rot(rng, 0.3), rng.normal(0.0, 0.1, 3))
    return cam, R, t, Tq, Tc


def _observe(rng, cam, R, t, a, b, n):
    """n points seen by camera a of side 1 and camera b of side 2: unit bearings f1, f2 [n,3]"""
    Ra, oa, Rb, ob = cam[a, :9].reshape(3, 3), cam[a, 9:], cam[b, :9].reshape(3, 3), cam[b, 9:]
    d = _unit(np.array([0.0, 0.0, 1.0]) + rng.uniform(-0.5, 0.5, (n, 3)) * np.array([1.0, 1.0, 0.0]))
    X1 = oa + (d @ Ra.T) * rng.uniform(4.0, 12.0, (n, 1))
    X2 = (X1 - t) @ R
    return _unit((X1 - oa) @ Ra), _unit((X2 - ob) @ Rb)


def _perturb(rng, f, noise):
    if noise <= 0.0:
        return f
    return _unit(f + np.cross(rng.normal(size=f.shape), f) * noise / math.sqrt(2.0))


def tuples(count, N, seed=0):
    """Noise-free N-tuples, one scene each: dict(ray1, ray2 [count,N,6] (g | o), R [count,3,3], t [count,3])"""
    rng = np.random.default_rng(seed)
    r1, r2 = np.zeros((count, N, 6)), np.zeros((count, N, 6))
    Rs, ts = np.zeros((count, 3, 3)), np.zeros((count, 3))
    for i in range(count):
        cam, R, t, _, _ = rig(rng)
        c1, c2 = rng.integers(0, NQ, N), NQ + rng.integers(0, NC, N)
        f1, f2 = np.zeros((N, 3)), np.zeros((N, 3))
        for a in range(NQ):
            for b in range(NQ, NQ + NC):
                k = np.flatnonzero((c1 == a) & (c2 == b))
                if len(k):
                    f1[k], f2[k] = _observe(rng, cam, R, t, a, b, len(k))
        g1, o1, g2, o2 = nr.rays(f1, f2, c1, c2, cam)
        r1[i], r2[i], Rs[i], ts[i] = np.hstack([g1, o1]), np.hstack([g2, o2]), R, t
    return dict(ray1=r1, ray2=r2, R=Rs, t=ts)


def tuple_rows(tp):
    return nr.rows(tp["ray1"][..., :3], tp["ray1"][..., 3:], tp["ray2"][..., :3], tp["ray2"][..., 3:])


@functools.lru_cache(maxsize=None)
def standard(N, count=2000):
    """The tuples of tuples(count, N, seed=N), route A and route B on them, and the yardsticks: sep [count] (separated), s_R [rad] and
    s_t, the largest differences between the routes on the separated tuples, truth_R / truth_t: route A against the truth there."""
    tp = tuples(count, N, seed=N)
    A = tuple_rows(tp)
    sv = np.array([nr.singular_values(a) for a in A])
    sep = sv[:, 1] >= SEP * sv[:, 0]
    okb, Rb, tb, svb = nr.solve_b(A)
    a = [nr.solve_a(x) for x in A]
    s_R = s_t = truth_R = truth_t = 0.0
    for i in np.flatnonzero(sep):
        assert a[i] is not None and okb[i]
        dr, dt = nr.pose_error(a[i][0], a[i][1], Rb[i], tb[i])
        s_R, s_t = max(s_R, dr), max(s_t, dt)
        dr, dt = nr.pose_error(a[i][0], a[i][1], tp["R"][i], tp["t"][i])
        truth_R, truth_t = max(truth_R, dr), max(truth_t, dt)
    return tp, dict(sep=sep, sv=sv, A=a, okb=okb, Rb=Rb, tb=tb, svb=svb, s_R=s_R, s_t=s_t, truth_R=truth_R, truth_t=truth_t)


def job(sizes, wrong, noise, seed):
    """One job of len(sizes) = 6 cells (query-major) with sizes[j] correspondences in cell j, a share `wrong` of them wrong matches (a random
    bearing on side 2), bearings perturbed by `noise` rad."""
    rng = np.random.default_rng(seed)
    cam, R, t, Tq, Tc = rig(rng)
    f1, f2, c1, c2, good = [], [], [], [], []
    for j, m in enumerate(sizes):
        a, b = j // NC, NQ + j % NC
        x1, x2 = _observe(rng, cam, R, t, a, b, m)
        bad = rng.random(m) < wrong
        x2 = np.where(bad[:, None], _unit(np.array([0.0, 0.0, 1.0]) + rng.uniform(-0.5, 0.5, (m, 3))), x2)
        f1.append(_perturb(rng, x1, noise)); f2.append(_perturb(rng, x2, noise))
        c1.append(np.full(m, a, np.int32)); c2.append(np.full(m, b, np.int32)); good.append(~bad)
    cat = lambda v, w: np.concatenate(v) if len(v) else np.zeros((0,) + w)
    return dict(f1=cat(f1, (3,)).reshape(-1, 3), f2=cat(f2, (3,)).reshape(-1, 3), cam1=cat(c1, ()).astype(np.int32), cam2=cat(c2, ()).astype(np.int32),
                cam=cam, cell_ptr=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32), T_sc_q=Tq, T_sc_c=Tc, R=R, t=t, good=cat(good, ()).astype(bool))


def split(n, cells=6):
    """n correspondences over the cells, as evenly as they go"""
    return [n // cells + (1 if j < n % cells else 0) for j in range(cells)]


def margin_job(sizes, wrong, noise, seed, job_seed, **opts):
    """A job whose replay (route A) keeps every score at least 1e-7 (relative) away from both thresholds: the job is rebuilt with another
    noise seed until it does; after 20 rounds it raises. Returns (job, replay)."""
    for k in range(20):
        j = job(sizes, wrong, noise, seed + 1000003 * k)
        r = nr.run(j, job_seed, "a", **opts)
        if r["margin"] > 1e-7:
            return j, r
    raise RuntimeError("no job with every score 1e-7 away from the thresholds in 20 rounds")


def batch(jobs, seeds=None):
    """The dict Context.ncrelpose_batch takes"""
    ptr = np.concatenate([[0], np.cumsum([len(j["f1"]) for j in jobs])]).astype(np.int32)
    cp = np.concatenate([[0], np.cumsum([len(j["cam"]) for j in jobs])]).astype(np.int32)
    bt = dict(ptr=ptr, cell_ptr=np.stack([j["cell_ptr"] for j in jobs]).astype(np.int32), bearing1=np.concatenate([j["f1"] for j in jobs]),
              bearing2=np.concatenate([j["f2"] for j in jobs]), cam1=np.concatenate([j["cam1"] for j in jobs]), cam2=np.concatenate([j["cam2"] for j in jobs]),
              cam_ptr=cp, cam=np.concatenate([j["cam"] for j in jobs]), T_sc_q=np.stack([j["T_sc_q"] for j in jobs]), T_sc_c=np.stack([j["T_sc_c"] for j in jobs]))
    if seeds is not None:
        bt["seed"] = np.asarray(seeds, np.uint64)
    return bt


# ------------------------------------------------------------------------------------------------ the facade shim
def facade_shim():
    """tests/cpp/facade_ncrelpose_shim.cpp: RelPoseSolverT's 17-point stage on a COVINS-G-shaped stand-in, no traits."""
    import ctypes as C
    import os
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    so = os.path.join(here, "cpp", "libfacade_ncrelpose_shim.so")
    srcs = [os.path.join(here, "cpp", f) for f in ("facade_ncrelpose_shim.cpp", "standin_fivept.hpp")] + \
           [os.path.join(root, "include", "covins_gpu", "optimization_gpu.hpp"), os.path.join(root, "include", "covgpu.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", srcs[0], "-o", so, "-L" + os.path.join(root, "covins_amd"),
                               "-lcovgpu", "-Wl,-rpath," + os.path.join(root, "covins_amd")])
    lib = C.CDLL(so)
    ip, dp, bp = C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_ubyte)
    lib.n17_build.restype = C.c_void_p
    lib.n17_build.argtypes = [C.c_int, ip, bp, dp, ip, ip, dp, dp, dp]
    lib.n17_free.argtypes = [C.c_void_p]
    lib.n17_seed.restype = C.c_ulonglong
    lib.n17_seed.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.n17_batch.argtypes = [C.c_void_p, C.c_int, C.c_int, ip, C.c_double, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, dp, bp, ip, ip, dp, dp, dp]
    lib.n17_single.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, dp, dp, dp]
    return lib


def shim_scene(lib, sc, T_sc):
    """The keyframes of a fivept_util.grid_scene() in the shim, with the extrinsics T_sc [nk,4,4]; returns the handle"""
    import ctypes as C
    ip, dp, bp = C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_ubyte)
    keep = [np.ascontiguousarray(sc["row_ptr"], np.int32), np.ascontiguousarray(sc["desc"], np.uint8), np.ascontiguousarray(sc["bearing"], np.float64),
            np.ascontiguousarray(sc["client"], np.int32), np.ascontiguousarray(sc["pred"], np.int32), np.ascontiguousarray(sc["T_wc"], np.float64),
            np.ascontiguousarray(sc["T_cw"], np.float64), np.ascontiguousarray(T_sc, np.float64)]
    return lib.n17_build(len(sc["pred"]), keep[0].ctypes.data_as(ip), keep[1].ctypes.data_as(bp), keep[2].ctypes.data_as(dp), keep[3].ctypes.data_as(ip),
                         keep[4].ctypes.data_as(ip), keep[5].ctypes.data_as(dp), keep[6].ctypes.data_as(dp), keep[7].ctypes.data_as(dp))
