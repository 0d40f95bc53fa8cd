"""Helpers of the float (SIFT) descriptor matching tests: the facade shim (tests/cpp/facade_matchf_shim.cpp) and its calls."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CV_8U, CV_32F = 0, 5
_SHIM = None
_ip, _dp, _fp = C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_float


def shim_path():
    return os.path.join(HERE, "cpp", "libfacade_matchf_shim.so")


def matchf_shim():
    """tests/cpp/facade_matchf_shim.cpp: LoopMatcherT's float and pair-list entry points on the COVINS-shaped classes of
    tests/cpp/standin_matchf.hpp, no traits."""
    global _SHIM
    if _SHIM is None:
        so = shim_path()
        srcs = [os.path.join(HERE, "cpp", f) for f in ("facade_matchf_shim.cpp", "standin_matchf.hpp")] + \
               [os.path.join(ROOT, "include", "covins_gpu", "optimization_gpu.hpp"), os.path.join(ROOT, "include", "covgpu.h")]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", srcs[0], "-o", so, "-L" + os.path.join(ROOT, "covins_amd"),
                                   "-lcovgpu", "-Wl,-rpath," + os.path.join(ROOT, "covins_amd")])
        lib = C.CDLL(so)
        lib.mf_build.restype = C.c_void_p
        lib.mf_build.argtypes = [C.c_int, _ip, C.c_int, C.c_int, C.c_void_p, _ip]
        lib.mf_free.argtypes = [C.c_void_p]
        lib.mf_shutdown.argtypes = []
        for f in (lib.mf_match_float, lib.mf_match_orb):
            f.argtypes = [C.c_void_p, C.c_int, C.c_int, _ip, _fp, _fp, _ip, _ip, _dp, _ip]
            f.restype = C.c_int
        lib.mf_match_grid.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, _fp, _fp, _ip, _ip, _ip, _dp, _ip]
        lib.mf_match_grid.restype = C.c_int
        _SHIM = lib
    return _SHIM


def build(lib, parts, cv_type, pred):
    """A handle on keyframes with the given descriptors_add_ matrices ([rows, cols] each) and predecessor indices."""
    ptr = np.zeros(len(parts) + 1, np.int32); ptr[1:] = np.cumsum([len(p) for p in parts])
    data = np.ascontiguousarray(np.concatenate(parts), np.float32 if cv_type == CV_32F else np.uint8)
    pred = np.ascontiguousarray(pred, np.int32)
    return lib.mf_build(len(parts), ptr.ctypes.data_as(_ip), int(parts[0].shape[1]), cv_type, data.ctypes.data_as(C.c_void_p), pred.ctypes.data_as(_ip))


def _lists(counts, idx, dist, total):
    out, pos = [], 0
    for n in counts:
        out.append([(int(idx[2 * i]), int(idx[2 * i + 1]), float(dist[i])) for i in range(pos, pos + n)])
        pos += n
    assert pos == total
    return out


def match(lib, h, q, cands, thr, ratio, orb=False, cap=200000):
    """MatchImagesFloatBatch (or MatchImagesBatch for orb) of keyframe q against cands: per candidate [(idxA, idxB, distance)]."""
    cand = np.ascontiguousarray(cands, np.int32)
    counts = np.zeros(max(len(cand), 1), np.int32); idx = np.zeros(2 * cap, np.int32); dist = np.zeros(cap); c = C.c_int(cap)
    f = lib.mf_match_orb if orb else lib.mf_match_float
    total = f(h, q, len(cand), cand.ctypes.data_as(_ip), thr, ratio, counts.ctypes.data_as(_ip), idx.ctypes.data_as(_ip), dist.ctypes.data_as(_dp),
              C.byref(c))
    assert total == c.value <= cap
    return _lists(counts[:len(cand)], idx, dist, total)


def match_grid(lib, h, q, c, nq, nc, feature_type, thr, ratio, cap=200000):
    """MatchImagePairsBatch on the nq x nc predecessor grid of (q, c): ([(kfA, kfB)], per pair [(idxA, idxB, distance)])."""
    pairs = np.zeros(2 * nq * nc, np.int32); counts = np.zeros(nq * nc, np.int32)
    idx = np.zeros(2 * cap, np.int32); dist = np.zeros(cap); cc = C.c_int(cap)
    n = lib.mf_match_grid(h, q, c, nq, nc, feature_type.encode(), thr, ratio, pairs.ctypes.data_as(_ip), counts.ctypes.data_as(_ip),
                          idx.ctypes.data_as(_ip), dist.ctypes.data_as(_dp), C.byref(cc))
    assert cc.value <= cap
    return [(int(pairs[2 * i]), int(pairs[2 * i + 1])) for i in range(n)], _lists(counts[:n], idx, dist, cc.value)
