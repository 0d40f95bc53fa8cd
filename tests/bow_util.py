"""Shared inputs of the bag-of-words tests: seeded vocabularies built here, the keyframe descriptor sets of the small
synthetic map (tests/match_util.keyframe_sets) with their restated bow vectors, and neighbour lists from shared-landmark counts.
References are computed once per process and must be left unchanged by the tests."""
from __future__ import annotations

import functools

import numpy as np

from covins_amd import synth, vocio
from tests import bow_ref, match_util


def random_vocab(k=8, L=4, seed=0, stop_frac=0.03, weighting=vocio.TF_IDF, scoring=vocio.L1_NORM):
    """A complete k-ary tree of depth L in the file's line order (breadth first). A child's descriptor is its parent's with a share of
    the bits flipped that halves per level, so close descriptors share a path; leaf weights are idf-like, ~stop_frac of them 0."""
    rng = np.random.default_rng(seed)
    parent, leaf, desc, level = [], [], [], [(0, rng.integers(0, 256, 32, dtype=np.uint8))]
    nid = 0
    for depth in range(1, L + 1):
        nxt = []
        for pid, pdesc in level:
            for _ in range(k):
                nid += 1
                d = match_util.flip(pdesc, 0.5 if depth == 1 else 0.25 / 2 ** (depth - 2), rng)[0]
                parent.append(pid); leaf.append(depth == L); desc.append(d)
                nxt.append((nid, d))
        level = nxt
    weight = np.where(np.array(leaf), rng.uniform(0.5, 9.0, len(leaf)), 0.0)
    weight[np.array(leaf) & (rng.random(len(leaf)) < stop_frac)] = 0.0
    return vocio.from_nodes(k, L, scoring, weighting, parent, leaf, np.array(desc), weight)


def irregular_vocab(seed=1, weighting=vocio.TF_IDF):
    """A leaf directly under the root, a one-child node, a node with 20 children, two sibling inner nodes with identical descriptors
    (the first wins every tie), leaves at depths 1 to 4, one stopped word."""
    rng = np.random.default_rng(seed)
    rnd = lambda: rng.integers(0, 256, 32, dtype=np.uint8)
    parent, leaf, desc = [], [], []

    def add(p, is_leaf, d):
        parent.append(p); leaf.append(is_leaf); desc.append(d)
        return len(parent)                                       # node id (the root is 0)
    twin = rnd()
    a = add(0, False, twin)                                      # 1: inner
    add(0, True, rnd())                                          # 2: a leaf under the root
    b = add(0, False, twin.copy())                               # 3: the twin of node 1 — never chosen
    c = add(0, False, rnd())                                     # 4: one child
    wide = add(0, False, rnd())                                  # 5: 20 children
    for _ in range(3):
        add(a, True, rnd())
    add(b, True, rnd())
    c1 = add(c, False, rnd())                                    # the only child of node 4
    for _ in range(20):
        add(wide, True, match_util.flip(desc[wide - 1], 0.1, rng)[0])
    c2 = add(c1, False, rnd())
    add(c1, True, rnd())
    for _ in range(2):
        add(c2, True, rnd())                                     # depth 4
    weight = np.where(np.array(leaf), rng.uniform(0.5, 9.0, len(leaf)), 0.0)
    weight[np.flatnonzero(leaf)[5]] = 0.0
    return vocio.from_nodes(20, 3, vocio.L1_NORM, weighting, parent, leaf, np.array(desc), weight)


@functools.lru_cache(maxsize=None)
def vocab(weighting=vocio.TF_IDF):
    return random_vocab(weighting=weighting)


def features_near(voc, n, seed, p=0.04):
    """n descriptors near random nodes of the vocabulary (so that the descent meets close and tied distances)."""
    rng = np.random.default_rng(seed)
    nodes = rng.integers(1, len(voc["parent"]), n)
    return match_util.flip(voc["desc"][nodes], p, rng) if n else np.zeros((0, 32), np.uint8)


@functools.lru_cache(maxsize=None)
def small_map():
    return synth.make_map(synth.config_named("small"))


@functools.lru_cache(maxsize=None)
def map_sets():
    """The keyframe descriptor sets of the small map (K = 180): dict(row_ptr, desc) and per keyframe its landmark list."""
    m = small_map()
    sb, _, kf_lms = match_util.keyframe_sets(m, seed=3, distractors=(20, 120))
    bt = sb.batch()
    return dict(row_ptr=bt["row_ptr"], desc=bt["desc"]), kf_lms


@functools.lru_cache(maxsize=None)
def map_bows():
    """The restatement's transform of map_sets() under vocab() (levelsup 4)."""
    sets, _ = map_sets()
    return bow_ref.transform_sets(vocab(), sets["row_ptr"], sets["desc"], 4)


def neighbour_lists(kf_lms, min_shared=15):
    """Per keyframe the keyframes that share at least min_shared landmarks, by descending count (ties: lower index first): the shape
    of GetConnectedKeyframesByWeight(0)."""
    K = len(kf_lms)
    sets = [set(s) for s in kf_lms]
    out = []
    for a in range(K):
        cnt = [(len(sets[a] & sets[b]), b) for b in range(K) if b != a]
        out.append([b for c, b in sorted(cnt, key=lambda t: (-t[0], t[1])) if c >= min_shared])
    return out


@functools.lru_cache(maxsize=None)
def map_neighbours():
    return neighbour_lists(map_sets()[1])


@functools.lru_cache(maxsize=None)
def map_table():
    """bow_ref.Table over the small map: ids and clients of the map, the restated bow vectors, neighbour_lists()."""
    m = small_map()
    _, kf_lms = map_sets()
    b = map_bows()
    bows = [(b["word"][b["bow_ptr"][k]:b["bow_ptr"][k + 1]], b["value"][b["bow_ptr"][k]:b["bow_ptr"][k + 1]]) for k in range(m.K)]
    inv = np.zeros(m.K, np.uint8); inv[::17] = 1
    return bow_ref.Table(m.kf_id, m.kf_client, bows, map_neighbours(), inv)


MAP_OPTS = dict(bow_ref.default_opts(), min_loop_dist=30)


@functools.lru_cache(maxsize=None)
def map_queries():
    """One query per keyframe against the keyframes before it (db_order = table order), min_loop_dist 30: the restatement's results."""
    tab = map_table()
    order = np.arange(len(tab), dtype=np.int32)
    inv = bow_ref.inverted_index(tab, order)
    return order, [bow_ref.detect_candidates(tab, order, q, q, MAP_OPTS, inv=inv) for q in range(len(tab))]


def table_dict(tab):
    return dict(id=tab.id, client=tab.client, bow_ptr=tab.bow_ptr, word=tab.word, value=tab.value, nb_ptr=tab.nb_ptr, nb=tab.nb,
                invalid=tab.invalid)


def hand_table(bows, neighbours=None, ids=None, clients=None, invalid=None):
    """A table from hand-written bow vectors [(words, values)]; ids default to 1000 + 200 * index (every pair past min_loop_dist and
    the id cut), clients to 0, neighbours to none."""
    n = len(bows)
    ids = [1000 + 200 * i for i in range(n)] if ids is None else ids
    return bow_ref.Table(ids, [0] * n if clients is None else clients, bows, [[] for _ in range(n)] if neighbours is None else neighbours,
                         invalid)


def unit(words, values=None):
    """An L1-normalised bow vector over the given ascending words."""
    w = np.asarray(words, np.int32)
    v = np.ones(len(w)) if values is None else np.asarray(values, np.float64)
    return w, v / v.sum() if len(w) else v


_SHIM = None


def bow_shim():
    """tests/cpp/facade_bow_shim.cpp: KeyframeDatabaseT on the stand-in map, descriptors, bow vectors and neighbours through the
    optional traits."""
    global _SHIM
    if _SHIM is None:
        import ctypes as C
        import os
        import subprocess
        here = os.path.dirname(os.path.abspath(__file__)); root = os.path.dirname(here)
        so = os.path.join(here, "cpp", "libfacade_bow_shim.so")
        srcs = [os.path.join(here, "cpp", f) for f in ("facade_bow_shim.cpp", "facade_shim.cpp", "standin_map.hpp")] + \
               [os.path.join(root, "include", "covins_gpu", "optimization_gpu.hpp"), os.path.join(root, "include", "covgpu.h")]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", srcs[0], "-o", so, "-L" + os.path.join(root, "covins_amd"),
                                   "-lcovgpu", "-Wl,-rpath," + os.path.join(root, "covins_amd")])
        lib = C.CDLL(so)
        ip, dp, bp, fp, vp = C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_float), C.c_void_p
        lib.shim_build.restype = vp
        lib.shim_free.argtypes = [vp]
        lib.bow_shutdown.argtypes = []
        lib.bow_set_keyframe.argtypes = [vp, C.c_int, C.c_int, bp, C.c_int, ip]
        lib.bow_set_vocab.argtypes = [C.c_int] * 6 + [ip, ip, ip, bp, ip, dp]
        lib.bow_compute.argtypes = [vp, C.c_int, ip, C.c_int]
        lib.bow_get.argtypes = [vp, C.c_int, C.c_int, ip, dp]
        lib.bow_get_features.argtypes = [vp, C.c_int, C.c_int, ip]
        lib.bow_detect.argtypes = [vp, C.c_int, C.c_int, C.c_int, ip, C.c_int, ip, ip, dp, C.c_int, ip, ip, fp, dp]
        lib.bow_detect_one.argtypes = [vp, C.c_int, ip, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, ip]
        lib.bow_consistency.argtypes = [vp, C.c_int, C.c_int, ip, ip, ip, ip]
        _SHIM = lib
    return _SHIM
