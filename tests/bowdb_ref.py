"""Restatement of the resident keyframe database (covgpu_bowdb): the yardstick of tests/test_gpu_bowdb.py.

  Database              put / set_neighbours / set_invalid / add / erase / query on slots; a query is bow_ref.detect_candidates over the
                        live slots in insertion order: the contract of covgpu_bowdb_query
  StatefulWithErase     bow_ref.StatefulDatabase, the reference's KeyframeDatabase with its scratch fields on the keyframes, plus
                        EraseKeyframe as kf_database.cpp:189-202
  replay(), replay_stateful()
                        the arrival of the small map's keyframes (tests/bow_util.py) in both forms: query, add, then the erasures of
                        erase_after(); tests/test_bowdb_host.py holds the two equal

References are computed once per process and must be left unchanged by the tests."""
from __future__ import annotations

import functools

import numpy as np

from tests import bow_ref
from tests import bow_util as bu

EMPTY = (np.zeros(0, np.int32), np.zeros(0))


class Database:
    def __init__(self, opts):
        self.opts = dict(opts)
        self.bow, self.id, self.client, self.nb, self.invalid = {}, {}, {}, {}, {}
        self.order = []                           # the live slots in insertion order

    def put(self, slot, id, client, bow):
        assert slot not in self.order, "put on a live slot"
        self.bow[slot] = (np.asarray(bow[0], np.int32), np.asarray(bow[1], np.float64))
        self.id[slot], self.client[slot] = int(id), int(client)

    def set_neighbours(self, slot, nb):
        self.nb[slot] = [int(k) for k in nb][:10]  # kf_database.cpp:141-142: the first ten

    def set_invalid(self, slot, flag):
        self.invalid[slot] = bool(flag)

    def add(self, slot):
        assert slot in self.bow and slot not in self.order
        self.order.append(slot)

    def erase(self, slot):
        if slot in self.order:
            self.order.remove(slot)

    def table(self, query=None, con=()):
        """The table of covgpu_detect_candidates_batch this state stands for: index = slot; the query's row holds its whole connected
        list, every other row the stored first ten."""
        n = 1 + max([-1] + list(self.bow) + list(self.nb) + list(self.invalid) + [int(k) for k in con])
        nbs = [self.nb.get(k, []) for k in range(n)]
        if query is not None:
            nbs[query] = [int(k) for k in con]
        return bow_ref.Table([self.id.get(k, 0) for k in range(n)], [self.client.get(k, 0) for k in range(n)],
                             [self.bow.get(k, EMPTY) for k in range(n)], nbs, [self.invalid.get(k, False) for k in range(n)])

    def query(self, slot, con, minsc=None):
        tab = self.table(slot, con)
        order = np.asarray(self.order, np.int32)
        return bow_ref.detect_candidates(tab, order, len(order), slot, self.opts, minsc)


class StatefulWithErase(bow_ref.StatefulDatabase):
    def EraseKeyframe(self, k):
        for w in self.tab.bow(k)[0]:
            lst = self.inverted.get(int(w), [])   # operator[] of the reference makes an empty list
            if k in lst:
                lst.remove(k)                     # the first occurrence, then break


def erase_after(q, live):
    """The erasures that follow the add of keyframe q."""
    if q >= 45 and q % 3 == 0 and (q - 45 + q % 7) in live:
        return [q - 45 + q % 7]
    return []


@functools.lru_cache(maxsize=None)
def replay():
    """Every keyframe of the small map in turn: query against the database, add, erase_after(). Neighbour lists and invalid flags are
    those of bu.map_table(), set at arrival. Returns (results per keyframe, the live slots at the end, the number of erasures)."""
    tab, nbs = bu.map_table(), bu.map_neighbours()
    db = Database(bu.MAP_OPTS)
    out, erased = [], 0
    for q in range(len(tab)):
        db.put(q, tab.id[q], tab.client[q], tab.bow(q)); db.set_neighbours(q, nbs[q]); db.set_invalid(q, tab.invalid[q])
        # the minimum score reads neighbours that arrive later: it is taken from the whole table, as bu.map_queries() does
        out.append(db.query(q, nbs[q], bow_ref.min_score(tab, q, bu.MAP_OPTS["min_score_factor"])))
        db.add(q)
        for e in erase_after(q, db.order):
            db.erase(e); erased += 1
    return out, list(db.order), erased


@functools.lru_cache(maxsize=None)
def replay_stateful():
    tab = bu.map_table()
    db = StatefulWithErase(tab)
    live, out = [], []
    for q in range(len(tab)):
        out.append(db.DetectCandidates(q, bu.MAP_OPTS))
        db.AddKeyframe(q); live.append(q)
        for e in erase_after(q, live):
            db.EraseKeyframe(e); live.remove(e)
    return out, live


def same(a, b):
    """Two results of the restatement agree in everything a query returns."""
    return (list(a["candidates"]) == list(b["candidates"]) and
            np.array_equal(np.array(a["acc_score"], np.float32).view(np.uint32), np.array(b["acc_score"], np.float32).view(np.uint32)) and
            all(a[k] == b[k] for k in ("num_sharing", "max_common_words", "num_scored")) and
            np.float64(a["min_score"]).view(np.uint64) == np.float64(b["min_score"]).view(np.uint64))


_SHIM = None


def bowdb_shim():
    """tests/cpp/facade_bowdb_shim.cpp: ResidentKeyframeDatabaseT beside KeyframeDatabaseT on the stand-in map (the traits, tables and
    entry points of tests/cpp/facade_bow_shim.cpp are compiled in)."""
    global _SHIM
    if _SHIM is None:
        import ctypes as C
        import os
        import subprocess
        here = os.path.dirname(os.path.abspath(__file__)); root = os.path.dirname(here)
        so = os.path.join(here, "cpp", "libfacade_bowdb_shim.so")
        srcs = [os.path.join(here, "cpp", f) for f in ("facade_bowdb_shim.cpp", "facade_bow_shim.cpp", "facade_shim.cpp", "standin_map.hpp")] + \
               [os.path.join(root, "include", "covins_gpu", "optimization_gpu.hpp"), os.path.join(root, "include", "covgpu.h")]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", srcs[0], "-o", so, "-L" + os.path.join(root, "covins_amd"),
                                   "-lcovgpu", "-Wl,-rpath," + os.path.join(root, "covins_amd")])
        lib = C.CDLL(so)
        ip, dp, bp, fp, lp, vp = (C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_float), C.POINTER(C.c_int64),
                                  C.c_void_p)
        lib.shim_build.restype = vp
        lib.shim_free.argtypes = [vp]
        lib.bow_shutdown.argtypes = []
        lib.bow_set_keyframe.argtypes = [vp, C.c_int, C.c_int, bp, C.c_int, ip]
        lib.bow_set_vocab.argtypes = [C.c_int] * 6 + [ip, ip, ip, bp, ip, dp]
        lib.bow_get.argtypes = [vp, C.c_int, C.c_int, ip, dp]
        lib.bow_get_features.argtypes = [vp, C.c_int, C.c_int, ip]
        lib.bowdb_replay.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, dp, ip, ip, C.c_int, ip, ip, fp, ip, ip, ip, lp]
        lib.bowdb_detect.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, ip, C.c_int, ip, dp, C.c_int, ip, ip, fp, dp]
        _SHIM = lib
    return _SHIM
