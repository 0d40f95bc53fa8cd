"""Host references for the covariance of every keyframe (Context.keyframe_covariances): marginal_util.reference over ALL free
keyframes of a problem — the full inverse on their rows by three host routes (SuperLU, dense LU, dense Cholesky + Gram) on the oracle's
reduced camera system, never from device code — and the block metric.

Metric per block: err = max |(A - B) o di dj^T| / max |A_lu o di dj^T| with d = sqrt(diag S) on the block's rows (di) and columns (dj); a
diagonal block has di = dj. h = the worst pairwise err of the host routes over all blocks checked.
Measured on the CPU for all free keyframes: small default plan mu 0: 179 keyframes, h 1.6e-8; mh01 visual-only mu 0: 547, h 2.9e-9;
mu 1e-8: 1.2e-9. Each of these references takes 6 - 11 s to build, so they are built once and shared.
"""
import numpy as np

from oracle import covo
from tests import marginal_util as mu_

H_FLOOR = mu_.H_FLOOR
ROUTES = ("lu", "dense", "chol")


_shim = None


def shim():
    """tests/cpp/libfacade_selinv_shim.so: KeyframeCovariances of the C++ facade on the stand-in map (built as marginal_util.shim builds its)."""
    global _shim
    if _shim is None:
        import ctypes as C
        import os
        import subprocess
        from tests import facade_util
        here = os.path.dirname(os.path.abspath(__file__)); root = os.path.dirname(here)
        so = os.path.join(here, "cpp", "libfacade_selinv_shim.so")
        srcs = [os.path.join(here, "cpp", f) for f in ("facade_selinv_shim.cpp", "facade_shim.cpp", "standin_map.hpp")] + \
               [os.path.join(root, "include", "covins_gpu", "optimization_gpu.hpp"), os.path.join(root, "include", "covgpu.h")]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", srcs[0], "-o", so, "-L" + os.path.join(root, "covins_amd"),
                                   "-lcovgpu", "-Wl,-rpath," + os.path.join(root, "covins_amd")])
        facade_util.lib()
        lib = C.CDLL(so)
        ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
        lib.shim_keyframe_covariances.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int, ip, ip, dp, dp, C.POINTER(C.c_ubyte),
                                                  C.POINTER(C.c_longlong), C.c_char_p]
        _shim = lib
    return _shim


def free_keyframes(prob):
    return [int(k) for k in np.flatnonzero(prob.kf_fixed == 0)]


def block_err(A, B, A_lu, di, dj):
    w = np.outer(di, dj)
    return float(np.abs((A - B) * w).max() / np.abs(A_lu * w).max())


class Reference:
    """The blocks of a marginal_util.reference over the keyframes `kfs` (D rows each)."""

    def __init__(self, ref, kfs):
        self.ref, self.D, self.kfs = ref, ref["D"], [int(k) for k in kfs]
        self.pos = {k: i for i, k in enumerate(self.kfs)}
        self.routes = [r for r in ROUTES if r in ref]

    def rows(self, k, d):
        return slice(self.D * self.pos[int(k)], self.D * self.pos[int(k)] + d)

    def block(self, route, i, j, d):
        return self.ref[route][self.rows(i, d), self.rows(j, d)]

    def scale(self, k, d):
        return self.ref["d"][self.rows(k, d)]

    def spread(self, blocks, d):
        """h over the blocks [(i, j)] at d rows per keyframe."""
        h = 0.0
        for i, j in blocks:
            lu = self.block("lu", i, j, d)
            for a in self.routes:
                for b in self.routes:
                    if a < b:
                        h = max(h, block_err(self.block(a, i, j, d), self.block(b, i, j, d), lu, self.scale(i, d), self.scale(j, d)))
        return h

    def err(self, got, i, j, d):
        """err of the device's block (i, j) against the SuperLU route."""
        lu = self.block("lu", i, j, d)
        return block_err(got, lu, lu, self.scale(i, d), self.scale(j, d))


def reference(prob, visual_only, mu, kfs=None, pgo=False, key=None):
    kfs = free_keyframes(prob) if kfs is None else [int(k) for k in kfs]
    return Reference(mu_.reference(prob, visual_only, mu, kfs, pgo=pgo, key=key), kfs)


def system_pairs(prob, visual_only, mu, pgo=False):
    """Every ordered pair (i, j), i != j, of free keyframes whose block of the oracle's S holds a non-zero: the whole off-diagonal pattern."""
    ptr, col, blocks, b, cost = covo.schur_sparse(prob, covo.default_options(visual_only=1 if visual_only else 0), mu, pgo=pgo)
    blocks = np.asarray(blocks)
    out = set()
    for i in range(len(ptr) - 1):
        for e in range(ptr[i], ptr[i + 1]):
            j = int(col[e])
            if j != i and np.any(blocks[e] != 0) and not prob.kf_fixed[i] and not prob.kf_fixed[j]:
                out.add((i, j)); out.add((j, i))
    return sorted(out)


def imu_pairs(prob):
    """Both orders of every IMU factor between two free keyframes."""
    out = set()
    for i, j in zip(prob.imu_kf_i, prob.imu_kf_j):
        if not prob.kf_fixed[i] and not prob.kf_fixed[j]:
            out.add((int(i), int(j))); out.add((int(j), int(i)))
    return sorted(out)
