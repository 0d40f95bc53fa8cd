"""Builders of the five-point tests (tests/test_fivept_host.py, tests/test_gpu_fivept.py).

Scenes: frame 1 at the origin, frame 2 at T_12 = [R | t] with ||t|| = 1 (one baseline) and a rotation of up to 60 degrees about a
random axis; points along bearings within ~35 degrees of frame 1's optical axis at a depth of 2 to 20 baselines.

    builder              what                                                       noise            wrong matches
    tuples(n)            8 correspondences each, with the true R, t                 none             none
    degenerate(n)        8-tuples in four kinds, n/4 each: all bearings equal,      none             -
                         pure rotation (t = 0), planar scene, two repeated
                         correspondences (slots 1 = 0 and 3 = 2)
    job(n, outliers)     n correspondences, the true R, t and route A's replay      1e-3 rad/axis    10-60 %: f2 replaced by a
                                                                                    (~half a pixel)  random bearing
    grid_scene()         11 keyframes over one point cloud for the 2 x 3 grid, with   1e-3 rad/axis    15 % wrong geometry; one chain
                         ORB-like descriptors and unnormalised bearings (chain                         without shared descriptors,
                         and facade tests; see its docstring)                                          one with random bearings

A job is re-perturbed (a new noise draw) until route A's replay with the job's seed has no correspondence whose score lies within
1e-7 relative of the threshold under the final model, and no draw whose two smallest selection sums lie within 1e-9 relative: the
device may then differ from route A in the last digits without flipping an inlier or a choice. After 20 rounds the builder raises.

Yardsticks, measured by tests/test_fivept_host.py on tuples(2000) (the tests compute them again, they do not read them here):
    separated tuples   1992 of 2000
    s_E = 1.1e-05      largest entry-wise difference between routes A and B over all solutions of the separated tuples
    s_T = 2.1e-07 rad  largest rotation / translation-direction angle between the poses routes A and B choose
    (both are route A's unpolished eigenvectors on the few tuples whose elimination has a condition number of 1e9 and more; route B
    and the device polish on the cubics at E itself and keep them below 1e-11 there)
The device is held to 10 s_E and 10 s_T: the margin is for a different pivot order and FMA contraction."""
from __future__ import annotations

import functools
import math

import numpy as np

from tests import fivept_ref as fr

NOISE = 1e-3


def _rotation(rng, max_deg=60.0):
    from scipy.spatial.transform import Rotation
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    return Rotation.from_rotvec(ax * math.radians(rng.uniform(0.0, max_deg))).as_matrix()


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def scene(rng, n, planar=False, rotation_only=False):
    """n noise-free correspondences of a random scene: (f1 [n,3], f2 [n,3], R, t)."""
    R = _rotation(rng)
    t = _unit(rng.normal(size=3))
    f1 = _unit(rng.normal(size=(n, 3)) * [0.4, 0.4, 0.0] + [0.0, 0.0, 1.0])
    if planar:                                             # points on a plane 6 baselines in front, tilted
        nrm = _unit(np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), 1.0]))
        depth = 6.0 / (f1 @ nrm)
    else:
        depth = rng.uniform(2.0, 20.0, n)
    X1 = f1 * depth[:, None]
    X2 = (X1 - (0.0 if rotation_only else 1.0) * t) @ R    # x1 = R x2 + t
    return f1, _unit(X2), R, t


def tuples(n, seed=20240611):
    """n noise-free 8-tuples: dict(f1 [n,8,3], f2 [n,8,3], R [n,3,3], t [n,3])."""
    rng = np.random.default_rng(seed)
    out = dict(f1=np.zeros((n, 8, 3)), f2=np.zeros((n, 8, 3)), R=np.zeros((n, 3, 3)), t=np.zeros((n, 3)))
    for i in range(n):
        out["f1"][i], out["f2"][i], out["R"][i], out["t"][i] = scene(rng, 8)
    return out


def degenerate(n, seed=77):
    """n degenerate 8-tuples (f1, f2 [n,8,3]), kind i % 4: 0 all bearings equal, 1 pure rotation, 2 planar scene, 3 two repeated
    correspondences among the five of the solver."""
    rng = np.random.default_rng(seed)
    f1 = np.zeros((n, 8, 3))
    f2 = np.zeros((n, 8, 3))
    for i in range(n):
        kind = i % 4
        if kind == 0:
            a, b, _, _ = scene(rng, 1)
            f1[i], f2[i] = a[0], b[0]
        elif kind == 1:
            f1[i], f2[i], _, _ = scene(rng, 8, rotation_only=True)
        elif kind == 2:
            f1[i], f2[i], _, _ = scene(rng, 8, planar=True)
        else:
            f1[i], f2[i], _, _ = scene(rng, 8)
            f1[i, 1], f2[i, 1] = f1[i, 0], f2[i, 0]
            f1[i, 3], f2[i, 3] = f1[i, 2], f2[i, 2]
    return f1, f2


def _perturbed(rng, n, n_out):
    f1, f2, R, t = scene(rng, n)
    f1 = _unit(f1 + rng.normal(size=f1.shape) * NOISE)
    f2 = _unit(f2 + rng.normal(size=f2.shape) * NOISE)
    bad = rng.permutation(n)[:n_out]
    f2[bad] = _unit(rng.normal(size=(len(bad), 3)) * [0.5, 0.5, 0.0] + [0.0, 0.0, 1.0])
    return f1, f2, R, t


def _clean(f1, f2, ref, trace, threshold, sigma):
    if ref["R"] is not None:
        with np.errstate(all="ignore"):
            s = fr.score(ref["R"], ref["t"], f1, f2, sigma)
        s = s[np.isfinite(s)]
        if np.any(np.abs(s - threshold) <= 1e-7 * threshold):
            return False
    for sums in trace:
        if len(sums) >= 2:
            a, b = np.sort(sums)[:2]
            if b - a <= 1e-9 * max(abs(a), abs(b)):
                return False
    return True


def job(n, outliers, seed, **opts):
    """One RANSAC job: dict(f1 [n,3], f2 [n,3], R, t (truth), seed, ref (route A's replay with `opts`)). outliers: fraction."""
    o = dict(fr.DEFAULTS)
    o.update(opts)
    n_out = int(round(outliers * n))
    for rnd in range(20):
        rng = np.random.default_rng([seed, rnd])
        f1, f2, R, t = _perturbed(rng, n, n_out) if n > 0 else (np.zeros((0, 3)), np.zeros((0, 3)), np.eye(3), np.array([1.0, 0, 0]))
        trace = []
        ref = fr.ransac(f1, f2, seed, trace=trace, **o)
        if _clean(f1, f2, ref, trace, o["threshold"], o["sigma"]):
            return dict(f1=f1, f2=f2, R=R, t=t, seed=seed, ref=ref, n_out=n_out)
    raise RuntimeError(f"job n={n} outliers={outliers} seed={seed}: still near a threshold or a tie after 20 rounds")


def batch(jobs):
    """The batch dict of Context.fivept_ransac_batch for a list of jobs, with their seeds."""
    ptr = np.zeros(len(jobs) + 1, np.int32)
    ptr[1:] = np.cumsum([len(j["f1"]) for j in jobs])
    cat = lambda k: np.concatenate([j[k] for j in jobs]).reshape(-1, 3) if jobs else np.zeros((0, 3))
    return dict(ptr=ptr, bearing1=cat("f1"), bearing2=cat("f2"), seed=np.array([j["seed"] for j in jobs], np.uint64))


@functools.lru_cache(maxsize=None)
def standard():
    """tuples(2000) and their yardsticks, computed once per session (about a minute: route B bisects in numpy) and shared by
    every test that needs them: (tuples, yardsticks)."""
    tp = tuples(2000)
    return tp, yardsticks(tp)


def yardsticks(tp):
    """Routes A and B on the tuples `tp`: dict(sep [n] bool, A (list of solution lists), chosen_A (list of (i, R, t)), s_E, s_T,
    res_A (largest cubic / epipolar residual of route A on the separated set))."""
    n = len(tp["f1"])
    sep = np.zeros(n, bool)
    A, chosen = [], []
    s_E = s_T = res = 0.0
    for i in range(n):
        f1, f2 = tp["f1"][i], tp["f2"][i]
        Ea, real, xyz = fr.solve_A(f1, f2, detail=True)
        ca = fr.choose(Ea, f1, f2)
        A.append(Ea)
        chosen.append(ca)
        sep[i] = fr.separated(real, xyz)
        if not sep[i]:
            continue
        Eb = fr.solve_B(f1, f2)
        cb = fr.choose(Eb, f1, f2, decompose=fr.decompose_closed)
        s_E = max(s_E, fr.match_sets(Ea, Eb))
        s_T = max(s_T, *(fr.pose_error(ca[1], ca[2], cb[1], cb[2]) if ca[0] >= 0 and cb[0] >= 0 else (math.inf,)))
        res = max(res, max(max(fr.cubic_residual(E), fr.epipolar_residual(E, f1, f2)) for E in Ea))
    return dict(sep=sep, A=A, chosen_A=chosen, s_E=s_E, s_T=s_T, res_A=res)


# ------------------------------------------------------------------------------------------------ the facade shim and its scene
def facade_shim():
    """tests/cpp/facade_fivept_shim.cpp: RelPoseSolverT on the COVINS-G-shaped classes of tests/cpp/standin_fivept.hpp, no traits."""
    import ctypes as C
    import os
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    so = os.path.join(here, "cpp", "libfacade_fivept_shim.so")
    srcs = [os.path.join(here, "cpp", f) for f in ("facade_fivept_shim.cpp", "standin_fivept.hpp")] + \
           [os.path.join(root, "include", "covins_gpu", "optimization_gpu.hpp"), os.path.join(root, "include", "covgpu.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", srcs[0], "-o", so, "-L" + os.path.join(root, "covins_amd"),
                               "-lcovgpu", "-Wl,-rpath," + os.path.join(root, "covins_amd")])
    lib = C.CDLL(so)
    ip, dp, bp = C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_ubyte)
    lib.f5_build.restype = C.c_void_p
    lib.f5_build.argtypes = [C.c_int, ip, bp, dp, ip, ip, dp, dp]
    lib.f5_free.argtypes = [C.c_void_p]
    lib.f5_seed.restype = C.c_ulonglong
    lib.f5_seed.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    lib.f5_compute_pose.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, ip, C.c_double, C.c_int, C.c_int, dp, ip, ip]
    lib.f5_grid.argtypes = [C.c_void_p, C.c_int, C.c_int, ip, C.c_double, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, bp, ip, ip, dp, dp, ip, ip,
                            C.c_int]
    return lib


def grid_scene(seed=11, n_points=260):
    """A synthetic map for the 2 x 3 grid: 11 keyframes observing one cloud of points, each feature with an ORB-like descriptor (the
    point's 256 random bits with 6 flipped), a bearing of arbitrary length with 1e-3 rad of noise, and 40 features of its own.
        0, 1        the query keyframe and its predecessor
        2, 3, 4     a good candidate and its two predecessors; 15 % of every keyframe's bearings point elsewhere (wrong geometry)
        5, 6, 7     a candidate whose last predecessor shares no descriptor with anyone: a cell with too few matches
        8, 9, 10    a candidate whose first predecessor has random bearings: a cell whose RANSAC fails
    Returns dict(row_ptr, desc [rows,32], bearing [rows,3], pred, client, T_wc [11,4,4], T_cw)."""
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(-4, 4, n_points), rng.uniform(-3, 3, n_points), rng.uniform(5, 14, n_points)], 1)
    base = rng.integers(0, 256, (n_points, 32), dtype=np.uint8)
    from scipy.spatial.transform import Rotation
    centres = [(0, 0, 0), (-0.4, 0.05, 0.1), (1.0, 0.2, -0.3), (1.3, 0.1, -0.1), (1.6, 0.3, 0.1), (-1.0, 0.3, 0.2), (-1.3, 0.2, 0.0),
               (-1.6, 0.1, 0.3), (0.3, 0.9, 0.2), (0.5, 1.2, 0.1), (0.7, 1.4, -0.2)]
    pred = [1, -1, 3, 4, -1, 6, 7, -1, 9, 10, -1]
    ptr, desc, bear, Twc, Tcw = [0], [], [], [], []
    for k, c in enumerate(centres):
        R = Rotation.from_rotvec(rng.normal(size=3) * 0.08).as_matrix()          # camera in the world
        T = np.eye(4); T[:3, :3] = R; T[:3, 3] = c
        Twc.append(T); Tcw.append(np.linalg.inv(T))
        seen = rng.permutation(n_points)[:int(0.85 * n_points)]
        d = base[seen].copy()
        for row in d:
            for bit in rng.integers(0, 256, 6):
                row[bit >> 3] ^= np.uint8(1 << (bit & 7))
        b = _unit((X[seen] - np.array(c)) @ R + rng.normal(size=(len(seen), 3)) * NOISE)
        wrong = rng.permutation(len(seen))[:int(0.15 * len(seen))] if k >= 2 else []
        b[wrong] = _unit(rng.normal(size=(len(wrong), 3)) * [0.5, 0.5, 0.0] + [0.0, 0.0, 1.0])
        if k == 7:
            d = rng.integers(0, 256, d.shape, dtype=np.uint8)
        if k == 9:
            b = _unit(rng.normal(size=b.shape) * [0.5, 0.5, 0.0] + [0.0, 0.0, 1.0])
        d = np.concatenate([d, rng.integers(0, 256, (40, 32), dtype=np.uint8)])
        b = np.concatenate([b, _unit(rng.normal(size=(40, 3)) * [0.5, 0.5, 0.0] + [0.0, 0.0, 1.0])])
        b = b * rng.uniform(0.5, 2.0, (len(b), 1))                                  # bearings_add_ is not normalised
        desc.append(d); bear.append(b); ptr.append(ptr[-1] + len(d))
    return dict(row_ptr=np.array(ptr, np.int32), desc=np.ascontiguousarray(np.concatenate(desc)), bearing=np.ascontiguousarray(np.concatenate(bear)),
                pred=np.array(pred, np.int32), client=np.arange(11, dtype=np.int32) % 3, T_wc=np.array(Twc), T_cw=np.array(Tcw))


def pose_to_transform(p):
    """The facade's detail::pose_to_transform in the same order of operations: [qx qy qz qw x y z] -> 4x4."""
    x, y, z, w = (float(v) for v in p[:4])
    n = math.sqrt(x * x + y * y + z * z + w * w)
    x /= n; y /= n; z /= n; w /= n
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), p[4]],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x), p[5]],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y), p[6]],
                     [0.0, 0.0, 0.0, 1.0]])
