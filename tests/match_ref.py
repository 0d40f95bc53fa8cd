"""numpy restatement of the loop candidates' descriptor matching (covgpu_match_batch).

dense(): COVINS, placerec_be.cpp:84-90 — LandmarkMatchingAlgorithm(thr) driven by estd2::DenseMatcher(numBest = 4, no ratio test):
    LandmarkMatchingAlgorithm::doSetup (skip flags), ::distance (d if d < thr, else FLT_MAX), DenseMatcher.hpp doWorkLinearMatching
    (180-224) and listBIteration (152-178), DenseMatcher.cpp assignbest (62-104) in the single-thread order, matchBody's emission (98).
knn2(): COVINS-G, placerec_gen_be.cpp:82-114 — cv::BFMatcher(NORM_HAMMING).knnMatch(k = 2) (OpenCV batchDistance's K-best insertion),
    then d1 <= img_match_thres and d1 < ratio_thres * d2, in float32 (config_backend.hpp:119-120 declares both thresholds float).
Both return the reference's match list [(idxA, idxB, distance)] in its order."""
from __future__ import annotations

import numpy as np

NUM_BEST = 4


def hamming(A, B):
    """[nA, nB] Hamming distances of 32-byte rows: popcount of the eight 32-bit XORs (feature_matcher_be.cpp:49-64)."""
    A = np.ascontiguousarray(A, np.uint8).reshape(-1, 32).view(np.uint64)
    B = np.ascontiguousarray(B, np.uint8).reshape(-1, 32).view(np.uint64)
    if len(A) == 0 or len(B) == 0:
        return np.zeros((len(A), len(B)), np.int64)
    return np.bitwise_count(A[:, None, :] ^ B[None, :, :]).sum(-1).astype(np.int64)


def dense_lists(D, skipA, skipB, thr=50.0):
    """Per A row the 4-entry list [(b, dist)] after the ascending scan over B (None for a skipped row). distance() is FLT_MAX unless
    d < thr, and FLT_MAX never beats an entry (init (-1, thr)): only the B rows with d < thr are visited, in ascending order."""
    thr = np.float32(thr)
    lists = []
    for a in range(D.shape[0]):
        if skipA[a]:
            lists.append(None)
            continue
        best = [(-1, thr)] * NUM_BEST                               # aiBest.resize(numBest_, pairing_t(-1, const_distthres))
        for b in np.flatnonzero(D[a] < thr):                        # D[a] < thr in float: exact for integers up to 256
            if skipB[b]:
                continue
            d = np.float32(D[a, b])
            if d < best[-1][1]:                                     # tmpdist < aiBest[numBest_ - 1].distance
                lb = next(i for i, e in enumerate(best) if not e[1] < d)   # std::lower_bound with Pairing::operator< (distance only)
                best = best[:lb] + [(int(b), d)] + best[lb:-1]      # shift back, the last entry drops out
        lists.append(best)
    return lists


def dense_assign(lists, nB):
    """assignbest(a, 0) for every listed A row in ascending order; a steal re-assigns the loser with assignbest(loser, 1)."""
    vpairs = [(-1, np.float32(np.finfo(np.float32).max))] * nB     # pairing_t(-1, numeric_limits<distance_t>::max())

    def assignbest(a, start):
        while True:
            best = lists[a]
            for index in range(start, NUM_BEST):
                b, d = best[index]
                if b == -1:
                    return
                if vpairs[b][0] == -1:
                    vpairs[b] = (a, d)
                    return
                if d < vpairs[b][1]:
                    old = vpairs[b][0]
                    vpairs[b] = (a, d)
                    a, start = old, 1                               # assignbest(oldPairIndexFromListA, ..., 1)
                    break
            else:
                return

    for a in range(len(lists)):
        if lists[a] is not None:
            assignbest(a, 0)
    return vpairs


def dense(A, B, skipA=None, skipB=None, thr=50.0):
    """The reference's Matches of one (query A, candidate B) pair: [(a, b, dist)] in ascending b."""
    D = hamming(A, B)
    nA, nB = D.shape
    skipA = np.zeros(nA, bool) if skipA is None else np.asarray(skipA, bool)
    skipB = np.zeros(nB, bool) if skipB is None else np.asarray(skipB, bool)
    vpairs = dense_assign(dense_lists(D, skipA, skipB, thr), nB)
    return [(int(a), b, int(d)) for b, (a, d) in enumerate(vpairs) if d < np.float32(thr)]   # matchBody:98, no ratio test


def knn2(A, B, thr=40.0, ratio=0.8):
    """The COVINS-G matches of one pair: [(a, b, dist)] in ascending a. A train set with fewer than two rows gives none (the reference
    reads matches_vect[i][1] unguarded there)."""
    D = hamming(A, B)
    nA, nB = D.shape
    if nB < 2:
        return []
    order = np.argsort(D, axis=1, kind="stable")[:, :2]             # top-2 by (d, index): equal distances keep the lower index first
    d1 = D[np.arange(nA), order[:, 0]].astype(np.float32)
    d2 = D[np.arange(nA), order[:, 1]].astype(np.float32)
    ok = (d1 <= np.float32(thr)) & (d1 < np.float32(ratio) * d2)
    return [(int(a), int(order[a, 0]), int(d1[a])) for a in np.flatnonzero(ok)]


def to_rows(matches, nA):
    """[(a, b, d)] -> per A row match (b or -1) and dist (d or -1), the layout of covgpu_match_batch's outputs."""
    m = np.full(nA, -1, np.int32); d = np.full(nA, -1, np.int32)
    for a, b, dd in matches:
        m[a] = b; d[a] = dd
    return m, d


def from_rows(match, dist, mode):
    """covgpu_match_batch's per-row outputs of one job -> the reference's match list and order (DENSE: ascending b; KNN2: ascending a)."""
    a = np.flatnonzero(match >= 0)
    out = [(int(i), int(match[i]), int(dist[i])) for i in a]
    return sorted(out, key=lambda t: t[1]) if mode == "dense" else out
