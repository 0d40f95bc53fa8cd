"""Shared inputs of the vocabulary-training tests: the named cases (hand-built ones, the seeded ones whose seeds a
search on the CPU found, the size sweep), their restatement computed once per process, and the serial C++ restatement
(tests/cpp/voctrain_serial.cpp). References must be left unchanged by the tests."""
from __future__ import annotations

import ctypes as C
import functools
import os
import subprocess

import numpy as np

from covins_amd import vocio
from tests import voctrain_ref as vr

HERE = os.path.dirname(os.path.abspath(__file__))
WAVE_MAX, TILE, MAX_K, THREADS = 256, 2048, 32, 256               # covgpu_voc_train_limits (checked against the library by both test files)


def clustered(n, seed, protos=12, flip=0.08):
    """n descriptors around `protos` random prototypes, each bit flipped with probability `flip`."""
    rng = np.random.default_rng(seed)
    p = rng.integers(0, 256, (protos, 32), dtype=np.uint8)
    rows = p[rng.integers(0, protos, n)]
    noise = np.packbits(rng.random((n, 256)) < flip, axis=1)
    return rows ^ noise


def low_entropy(n, seed, bits=6):
    """n descriptors whose only free bits are the lowest `bits` (<= 16) of bytes 0 and 1: many equal rows, tied distances and exact-half
    counts."""
    rng = np.random.default_rng(seed)
    rows = np.zeros((n, 32), np.uint8)
    v = rng.integers(0, 1 << bits, n)
    rows[:, 0] = v & 255; rows[:, 1] = v >> 8
    return rows


def even_sets(n, sets):
    return np.linspace(0, n, sets + 1).astype(np.int32)


def _case(desc, k, L, row_ptr=None, **kw):
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    ptr = even_sets(len(desc), min(4, max(1, len(desc)))) if row_ptr is None else np.asarray(row_ptr, np.int32)
    return dict(row_ptr=ptr, desc=desc, k=k, L=L, weighting=kw.pop("weighting", vocio.TF_IDF), seed=kw.pop("seed", 0), opts=kw)


def _hand():
    rng = np.random.default_rng(7)
    a, b, c = (rng.integers(0, 256, 32, dtype=np.uint8) for _ in range(3))
    six = rng.integers(0, 256, (6, 32), dtype=np.uint8)
    return {
        "root_n_below_k": _case(six[:3], 5, 2),
        "root_n_equals_k": _case(six[:5], 5, 2),
        "root_n_above_k": _case(six, 5, 2),
        "one_row": _case(six[:1], 3, 2),
        "all_identical": _case(np.tile(a, (40, 1)), 4, 4),
        "two_values": _case(np.stack([a, b] * 30), 4, 3),
        "complementary": _case(np.stack([c, ~c] * 6), 3, 2),
        "duplicates": _case(np.stack([a, a, b, a, b]), 8, 2, row_ptr=[0, 2, 5]),
    }


# seeds found by a search on the CPU over the restatements (tests/test_voctrain_host.py asserts what each is for)
TIE_SEED, EMPTIED_SEED, CAPPED_SEED = 0, 43, 6


def _seeded():
    return {
        "ties": _case(low_entropy(90, TIE_SEED, bits=7), 4, 3, seed=TIE_SEED),
        "emptied": _case(low_entropy(24, EMPTIED_SEED, bits=10), 8, 2, seed=EMPTIED_SEED),
        "capped_1": _case(clustered(700, CAPPED_SEED, protos=9, flip=0.2), 4, 3, seed=CAPPED_SEED, max_iterations=1),
        "capped_2": _case(clustered(700, CAPPED_SEED, protos=9, flip=0.2), 4, 3, seed=CAPPED_SEED, max_iterations=2),
    }


def _sweep():
    out = {}
    for n in (WAVE_MAX - 1, WAVE_MAX, WAVE_MAX + 1, TILE - 1, TILE, TILE + 1):
        out[f"rows_{n}"] = _case(clustered(n, n), 10, 2, seed=n)
    out["three_tiles"] = _case(clustered(2 * TILE + 77, 5, protos=5), 3, 3, seed=5)
    for k in (2, 3, 10, MAX_K):
        out[f"k_{k}"] = _case(clustered(900, 100 + k, protos=2 * k), k, 2, seed=k)
    for L, k, n in ((1, 6, 500), (2, 5, 700), (3, 4, 800), (6, 2, 300)):
        out[f"L_{L}"] = _case(clustered(n, 200 + L, protos=7, flip=0.15), k, L, seed=L)
    d = clustered(600, 31)
    out["one_set"] = _case(d, 5, 2, row_ptr=[0, 600])
    out["empty_sets"] = _case(d, 5, 2, row_ptr=[0, 0, 0, 150, 150, 400, 400, 400, 600, 600])
    out["many_sets"] = _case(clustered(900, 41), 5, 2, row_ptr=even_sets(900, 300))       # more sets than one 1 KiB pass of word bitmaps holds
    for w, name in ((vocio.TF_IDF, "tf_idf"), (vocio.TF, "tf"), (vocio.IDF, "idf"), (vocio.BINARY, "binary")):
        out[f"weighting_{name}"] = _case(d, 5, 2, row_ptr=even_sets(600, 9), weighting=w)
    return out


@functools.lru_cache(maxsize=None)
def cases():
    out = {}
    out.update(_hand()); out.update(_seeded()); out.update(_sweep())
    return out


HAND = ("root_n_below_k", "root_n_equals_k", "root_n_above_k", "one_row", "all_identical", "two_values", "complementary", "duplicates",
        "ties", "emptied")
CAPPED = ("capped_1", "capped_2")
SWEEP = tuple(f"rows_{n}" for n in (WAVE_MAX - 1, WAVE_MAX, WAVE_MAX + 1, TILE - 1, TILE, TILE + 1)) + ("three_tiles",) + \
    tuple(f"k_{k}" for k in (2, 3, 10, MAX_K)) + tuple(f"L_{L}" for L in (1, 2, 3, 6))
DOCS = ("one_set", "empty_sets", "many_sets", "weighting_tf_idf", "weighting_tf", "weighting_idf", "weighting_binary")
ALL = HAND + CAPPED + SWEEP + DOCS


def run_ref(c):
    return vr.train(c["row_ptr"], c["desc"], c["k"], c["L"], weighting=c["weighting"], seed=c["seed"],
                    max_iterations=c["opts"].get("max_iterations", 100))


@functools.lru_cache(maxsize=None)
def ref(name):
    """(voc, info) of the restatement for a named case."""
    return run_ref(cases()[name])


_SERIAL = None


def serial_lib():
    global _SERIAL
    if _SERIAL is None:
        so = os.path.join(HERE, "cpp", "libvoctrain_serial.so")
        src = os.path.join(HERE, "cpp", "voctrain_serial.cpp")
        if not os.path.exists(so) or os.path.getmtime(src) > os.path.getmtime(so):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", src, "-o", so])
        lib = C.CDLL(so)
        ip, bp, dp, lp = C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_double), C.POINTER(C.c_int64)
        lib.voctrain_serial.argtypes = [C.c_int, ip, bp, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_int, C.c_int, ip, ip, bp, ip, dp, ip, lp]
        lib.voctrain_serial.restype = C.c_int
        _SERIAL = lib
    return _SERIAL


def serial(row_ptr, desc, k, L, weighting=vocio.TF_IDF, seed=0, max_iterations=100):
    """The serial C++ restatement: (voc, stats [6], row_word)."""
    ptr = np.ascontiguousarray(row_ptr, np.int32)
    d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    ip, bp = C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    cap = 1024
    while True:
        parent, cdesc, wid, weight = np.zeros(cap, np.int32), np.zeros((cap, 32), np.uint8), np.zeros(cap, np.int32), np.zeros(cap)
        rw, stats, nw = np.zeros(len(d), np.int32), np.zeros(6, np.int64), C.c_int32(0)
        N = serial_lib().voctrain_serial(len(ptr) - 1, ptr.ctypes.data_as(ip), d.ctypes.data_as(bp), k, L, weighting, seed, max_iterations, cap,
                                         C.byref(nw), parent.ctypes.data_as(ip), cdesc.ctypes.data_as(bp), wid.ctypes.data_as(ip),
                                         weight.ctypes.data_as(C.POINTER(C.c_double)), rw.ctypes.data_as(ip),
                                         stats.ctypes.data_as(C.POINTER(C.c_int64)))
        if N < 0:
            raise ValueError("refused (D4)")
        if N <= cap:
            break
        cap = N
    voc = vocio.from_nodes(k, L, vocio.L1_NORM, weighting, parent[1:N], wid[1:N] >= 0, cdesc[1:N], weight[1:N])
    assert voc["num_words"] == nw.value and np.array_equal(voc["word_id"], wid[:N])
    return voc, stats, rw


def run_gpu(ctx, c, **more):
    """Context.train_vocabulary of a case (row_word asked for)."""
    return ctx.train_vocabulary(c["row_ptr"], c["desc"], c["k"], c["L"], weighting=c["weighting"], seed=c["seed"], row_word=True,
                                **dict(c["opts"], **more))


_SHIM = None


def shim():
    """tests/cpp/facade_voctrain_shim.cpp: the C++ facade's CreateVocabulary on the stand-in types."""
    global _SHIM
    if _SHIM is None:
        root = os.path.dirname(HERE)
        so = os.path.join(HERE, "cpp", "libfacade_voctrain_shim.so")
        srcs = [os.path.join(HERE, "cpp", f) for f in ("facade_voctrain_shim.cpp", "facade_shim.cpp", "standin_map.hpp")] + \
               [os.path.join(root, "include", "covins_gpu", "optimization_gpu.hpp"), os.path.join(root, "include", "covgpu.h")]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", srcs[0], "-o", so, "-L" + os.path.join(root, "covins_amd"),
                                   "-lcovgpu", "-Wl,-rpath," + os.path.join(root, "covins_amd")])
        lib = C.CDLL(so)
        ip, bp, dp = C.POINTER(C.c_int), C.POINTER(C.c_uint8), C.POINTER(C.c_double)
        lib.voctrain_create.argtypes = [C.c_int, ip, bp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_ulonglong, C.c_int, C.c_int, ip, ip, ip, ip, bp,
                                        ip, dp, C.POINTER(C.c_longlong)]
        lib.voctrain_create.restype = C.c_int
        _SHIM = lib
    return _SHIM


def run_shim(c, capacity=4096):
    """CreateVocabulary of a case through the facade: (voc in flat form with the facade's own child lists, stats [8])."""
    ptr = np.ascontiguousarray(c["row_ptr"], np.int32)
    d = np.ascontiguousarray(c["desc"], np.uint8)
    ip, bp = C.POINTER(C.c_int), C.POINTER(C.c_uint8)
    parent, cptr, child = np.zeros(capacity, np.int32), np.zeros(capacity + 1, np.int32), np.zeros(capacity, np.int32)
    cdesc, wid, weight = np.zeros((capacity, 32), np.uint8), np.zeros(capacity, np.int32), np.zeros(capacity)
    stats, nw = np.zeros(8, np.int64), C.c_int(0)
    N = shim().voctrain_create(len(ptr) - 1, ptr.ctypes.data_as(ip), d.ctypes.data_as(bp), c["k"], c["L"], c["weighting"], vocio.L1_NORM,
                               c["seed"], c["opts"].get("max_iterations", 0), capacity, C.byref(nw), parent.ctypes.data_as(ip),
                               cptr.ctypes.data_as(ip), child.ctypes.data_as(ip), cdesc.ctypes.data_as(bp), wid.ctypes.data_as(ip),
                               weight.ctypes.data_as(C.POINTER(C.c_double)), stats.ctypes.data_as(C.POINTER(C.c_longlong)))
    assert 0 < N <= capacity, N
    voc = dict(k=c["k"], L=c["L"], scoring=vocio.L1_NORM, weighting=c["weighting"], parent=parent[:N], child_ptr=cptr[:N + 1],
               child=child[:N - 1], desc=cdesc[:N], word_id=wid[:N], weight=weight[:N], num_words=nw.value)
    return voc, stats
