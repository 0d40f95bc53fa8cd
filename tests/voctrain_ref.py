"""Restatement of DBoW2's TemplatedVocabulary::create for ORB descriptors under L1 scoring (TemplatedVocabulary.h:557-996,
FORB.cpp:28-101), with the departures D1-D4 of DESIGN.md §4.18: counter-based random numbers, an emptied cluster keeps its centre, the
k-means loop of a node is capped, degenerate inputs are refused. The recursion is the reference's, depth first; everything is integer
work except cut_d = u * dist_sum and the weights log(NDocs / Ni), which are single double operations.

train(row_ptr, desc, k, L, ...) -> (voc, info): voc is the flat form of covins_amd/vocio.py; info holds stats [6] (associations
summed, most of one node, nodes cut short by the cap, centre updates that met an empty group, nodes seeded with fewer than k centres,
levels worked), row_word (the transform leaf of every training row), train_leaf (the word each row was grouped into while training, -1
for a row that was never split off on its own), and what the host tests ask about the run (ties, exact-half bits, per-node records)."""
from __future__ import annotations

import math

import numpy as np

from covins_amd import vocio

M64 = (1 << 64) - 1
MAX_WORDS = (1 << 20) - 1
MAX_REDRAWS = 64
_POP = np.array([bin(i).count("1") for i in range(256)], np.int64)


def splitmix64(x: int) -> int:
    z = (x + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def child_key(key: int, c: int) -> int:
    return splitmix64((key + 1 + c) & M64)


def unit(key: int, j: int) -> float:
    """Draw j of the node with this key, in [0, 1)."""
    r = splitmix64((splitmix64(key) + j) & M64)
    return float(r >> 11) * 2.0 ** -53


def distance(rows, centre):
    """FORB::distance of every row to one centre."""
    return _POP[np.bitwise_xor(rows, centre[None, :])].sum(axis=1)


def mean_value(rows):
    """FORB::meanValue of a non-empty group: a bit is set iff its count >= n / 2 + n % 2. Returns (centre, exact-half bits)."""
    n = len(rows)
    if n == 1:
        return rows[0].copy(), 0
    cnt = np.unpackbits(rows, axis=1, bitorder="little").sum(axis=0, dtype=np.int64)
    half = int((2 * cnt == n).sum())
    return np.packbits(cnt >= n // 2 + n % 2, bitorder="little"), half


def seed_centres(rows, k, key, rec):
    """initiateClustersKMpp with the draws of D1. Returns the centres; rec['draws'] counts the draws."""
    n = len(rows)
    j = 0
    idx = min(int(unit(key, j) * n), n - 1); j += 1
    centres = [rows[idx].copy()]
    mind = distance(rows, centres[0])
    while len(centres) < k:
        mind = np.minimum(mind, distance(rows, centres[-1]))
        total = int(mind.sum())
        if total == 0:
            break
        for _ in range(MAX_REDRAWS):
            cut = unit(key, j) * float(total); j += 1
            if cut != 0.0:
                break
        at = np.flatnonzero(np.cumsum(mind).astype(np.float64) >= cut)
        centres.append(rows[int(at[0]) if len(at) else n - 1].copy())
    rec["draws"] = j
    return centres


def associate(rows, centres):
    """Per row the centre of least distance, the lowest index winning a tie. Returns (association, rows with a tied minimum)."""
    d = np.stack([distance(rows, c) for c in centres], axis=1)
    a = d.argmin(axis=1)                                           # the first minimum
    ties = int(((d == d.min(axis=1, keepdims=True)).sum(axis=1) > 1).sum())
    return a, ties


def train(row_ptr, desc, k, L, weighting=vocio.TF_IDF, scoring=vocio.L1_NORM, seed=0, max_iterations=100):
    row_ptr = np.asarray(row_ptr, np.int64)
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    R = len(desc)
    if R == 0 or k < 2 or L < 1 or k ** L > MAX_WORDS or scoring != vocio.L1_NORM or weighting not in (0, 1, 2, 3):
        raise ValueError("refused (D4)")
    parent, cdesc, nchild = [-1], [np.zeros(32, np.uint8)], [0]
    train_rows = {}                                                # node id -> row indices of its group
    stats = [0, 0, 0, 0, 0, 0]
    info = dict(ties=0, half_bits=0, nodes=[])

    def step(node, idx, level, key):
        rows = desc[idx]
        n = len(idx)
        rec = dict(node=node, level=level, n=n, iters=0, capped=False, centres=n, draws=0, converged=True, kmeans=n > k)
        stats[5] = max(stats[5], level)
        if n <= k:
            centres = [r.copy() for r in rows]
            assoc = np.arange(n)
        else:
            centres = seed_centres(rows, k, key, rec)
            if len(centres) < k:
                stats[4] += 1
            prev, it, conv = None, 0, False
            while it < max_iterations:
                if it > 0:
                    for c in range(len(centres)):
                        g = rows[prev == c]
                        if len(g) == 0:
                            stats[3] += 1                          # D2
                        else:
                            centres[c], half = mean_value(g)
                            info["half_bits"] += half
                assoc, ties = associate(rows, centres)
                info["ties"] += ties
                it += 1
                if prev is not None and np.array_equal(assoc, prev):
                    conv = True
                    break
                prev = assoc
            stats[0] += it; stats[1] = max(stats[1], it)
            if not conv:
                stats[2] += 1
            rec.update(iters=it, capped=not conv, centres=len(centres), converged=conv)
        info["nodes"].append(rec)
        first = len(parent)
        for c in centres:
            parent.append(node); cdesc.append(c); nchild.append(0)
        nchild[node] = len(centres)
        groups = [idx[assoc == c] for c in range(len(centres))]
        for c, g in enumerate(groups):
            train_rows[first + c] = g
        if level < L:
            for c, g in enumerate(groups):
                if len(g) > 1:
                    step(first + c, g, level + 1, child_key(key, c))

    step(0, np.arange(R), 1, seed & M64)
    N = len(parent)
    is_leaf = np.array(nchild[1:]) == 0
    voc = vocio.from_nodes(k, L, scoring, weighting, parent[1:], is_leaf, np.array(cdesc[1:]), np.zeros(N - 1))
    row_word = transform_leaves(voc, desc)
    weight = np.zeros(N)
    leaves = np.flatnonzero(voc["word_id"] >= 0)
    if weighting in (vocio.TF, vocio.BINARY):
        weight[leaves] = 1.0
    else:
        ndocs = len(row_ptr) - 1
        ni = np.zeros(voc["num_words"], np.int64)
        for s in range(ndocs):
            ni[np.unique(row_word[row_ptr[s]:row_ptr[s + 1]])] += 1
        for n in leaves:
            c = int(ni[voc["word_id"][n]])
            if c > 0:
                weight[n] = math.log(ndocs / c)
    voc["weight"] = weight
    train_leaf = np.full(R, -1, np.int64)
    for n in leaves:
        train_leaf[train_rows[int(n)]] = voc["word_id"][n]
    info.update(stats=np.array(stats, np.int64), row_word=row_word.astype(np.int32), train_leaf=train_leaf, train_rows=train_rows)
    return voc, info


def transform_leaves(voc, desc):
    """The word of every row by TemplatedVocabulary::transform's greedy descent (the first minimum wins), whatever its weight.
    Equal rows descend alike, so each distinct row is walked once."""
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    uniq, inv = np.unique(desc, axis=0, return_inverse=True)
    inv = np.asarray(inv).ravel()
    cp, ch, nd, wid = voc["child_ptr"], voc["child"], voc["desc"], voc["word_id"]
    node = np.zeros(len(uniq), np.int64)
    active = np.arange(len(uniq))
    while len(active):
        groups = {}
        for n in np.unique(node[active]):
            groups[int(n)] = active[node[active] == n]
        nxt = []
        for n, rows in groups.items():
            kids = ch[cp[n]:cp[n + 1]]
            d = np.stack([distance(uniq[rows], nd[c]) for c in kids], axis=1)
            node[rows] = kids[d.argmin(axis=1)]
            nxt.append(rows[wid[node[rows]] < 0])
        active = np.concatenate(nxt) if nxt else np.zeros(0, np.int64)
    return wid[node][inv]


def assert_same(got, ref, what=""):
    """Two vocabularies in flat form, every integer, byte and double equal."""
    for key in ("k", "L", "scoring", "weighting", "num_words"):
        assert int(got[key]) == int(ref[key]), (what, key, got[key], ref[key])
    for key in ("parent", "child_ptr", "child", "desc", "word_id"):
        assert np.array_equal(np.asarray(got[key]), np.asarray(ref[key])), (what, key)
    assert np.asarray(got["weight"]).dtype == np.float64 and \
        np.array_equal(np.asarray(got["weight"]).view(np.uint64), np.asarray(ref["weight"], np.float64).view(np.uint64)), (what, "weight")
