"""Descriptor sets and matching jobs for covgpu_match_batch. Kept apart from covins_amd/synth.py so the golden input
digests of the synthetic maps do not move.

map_batch(): one descriptor set per keyframe of a synthetic map. Every landmark gets a random 256-bit descriptor; each observation of
it is that descriptor with every bit flipped with probability p (drawn per keyframe), and the keyframe gets a number of distractor rows
(random descriptors, keypoints without a landmark). The rows are shuffled. A row is skipped (DENSE) when it has no landmark or its
landmark is invalid; a fraction of the landmarks is marked invalid. Jobs pair a query keyframe with a candidate that shares landmarks,
as tests/abspose_util.map_batch picks them.
adversarial_batch(): hand-built sets at exact distances — equal distances, duplicated rows, every pair under the threshold (long
steal chains), the scan-order eviction of DESIGN §4.11 step 3, and distances on each side of 40, 50 and the ratio boundary."""
from __future__ import annotations

import hashlib

import numpy as np


class SetBuilder:
    """Accumulates descriptor sets ([n, 32] uint8, skip [n]) and jobs (query set, candidate set)."""

    def __init__(self):
        self.desc, self.skip, self.ptr, self.set_a, self.set_b, self.info = [], [], [0], [], [], {}

    def add(self, desc, skip=None):
        desc = np.asarray(desc, np.uint8).reshape(-1, 32)
        self.desc.append(desc)
        self.skip.append(np.zeros(len(desc), np.uint8) if skip is None else np.asarray(skip, np.uint8))
        self.ptr.append(self.ptr[-1] + len(desc))
        return len(self.ptr) - 2

    def job(self, a, b):
        self.set_a.append(a); self.set_b.append(b)

    def batch(self):
        cat = lambda v, w: np.ascontiguousarray(np.concatenate(v)) if v else np.zeros((0,) + w, np.uint8)
        bt = dict(row_ptr=np.array(self.ptr, np.int32), desc=cat(self.desc, (32,)), skip=cat(self.skip, ()),
                  set_a=np.array(self.set_a, np.int32), set_b=np.array(self.set_b, np.int32))
        bt.update(self.info)
        return bt


def rows(bt, s):
    """Descriptors and skip flags of set s."""
    r = slice(int(bt["row_ptr"][s]), int(bt["row_ptr"][s + 1]))
    return bt["desc"][r], bt["skip"][r].astype(bool)


def digest(bt):
    """sha256 over what the matcher reads: row_ptr, desc, skip, set_a, set_b."""
    h = hashlib.sha256()
    for k in ("row_ptr", "desc", "skip", "set_a", "set_b"):
        h.update(np.ascontiguousarray(bt[k]).tobytes())
    return h.hexdigest()


def flip(desc, p, rng):
    """Every bit of every row flipped with probability p."""
    desc = np.asarray(desc, np.uint8).reshape(-1, 32)
    mask = np.packbits(rng.random((len(desc), 256)) < p, axis=1)
    return desc ^ mask


def at_dist(x, d, rng, avoid=None):
    """A row at Hamming distance exactly d from x (bits chosen outside `avoid`, a set of bit indices, when given)."""
    pool = np.setdiff1d(np.arange(256), np.fromiter(avoid, int) if avoid else np.zeros(0, int))
    bits = rng.choice(pool, d, replace=False)
    m = np.zeros(256, bool); m[bits] = True
    return np.asarray(x, np.uint8) ^ np.packbits(m), set(bits.tolist())


def keyframe_sets(m, seed=0, p_range=(0.02, 0.12), distractors=(50, 600), invalid_frac=0.05):
    """One set per keyframe of map m (see the module doc). Returns the SetBuilder (one set per keyframe, in keyframe order) and per set
    the landmark of every row (-1: distractor)."""
    rng = np.random.default_rng(seed)
    lm_desc = rng.integers(0, 256, (m.L, 32), dtype=np.uint8)
    invalid = rng.random(m.L) < invalid_frac
    kf_lms = [[] for _ in range(m.K)]
    for l in range(m.L):
        for o in range(m.lm_obs_ptr[l], m.lm_obs_ptr[l + 1]):
            kf_lms[m.obs_kf[o]].append(l)
    sb, lm_of_row = SetBuilder(), []
    for k in range(m.K):
        lms = np.array(kf_lms[k], np.int64)
        nd = int(rng.integers(*distractors))
        obs = flip(lm_desc[lms], rng.uniform(*p_range), rng) if len(lms) else np.zeros((0, 32), np.uint8)
        desc = np.concatenate([obs, rng.integers(0, 256, (nd, 32), dtype=np.uint8)])
        lm = np.concatenate([lms, np.full(nd, -1)])
        perm = rng.permutation(len(desc))
        desc, lm = desc[perm], lm[perm]
        skip = (lm < 0) | invalid[np.maximum(lm, 0)]
        sb.add(desc, skip)
        lm_of_row.append(lm)
    return sb, lm_of_row, kf_lms


def map_batch(m, num, seed=0, **kw):
    """`num` (query, candidate) jobs over the keyframe sets of map m: a query keyframe and a candidate that shares at least 20 of its
    landmarks (any other keyframe when none does). Batch dict plus lm_of_row (per set) and pairs."""
    sb, lm_of_row, kf_lms = keyframe_sets(m, seed, **kw)
    rng = np.random.default_rng(seed + 1)
    lm_sets = [set(s) for s in kf_lms]
    for _ in range(num):
        q = int(rng.integers(m.K))
        near = [c for c in range(max(0, q - 8), min(m.K, q + 9)) if c != q and len(lm_sets[q] & lm_sets[c]) >= 20]
        c = int(rng.choice(near)) if near else int((q + 1 + rng.integers(m.K - 1)) % m.K)
        sb.job(q, c)
    bt = sb.batch()
    bt["lm_of_row"] = lm_of_row
    return bt


def adversarial_batch(seed=0):
    """Hand-built sets at exact distances (module doc). Every set has at most 200 rows."""
    rng = np.random.default_rng(seed)
    sb = SetBuilder()
    rnd = lambda n: rng.integers(0, 256, (n, 32), dtype=np.uint8)
    x = rnd(1)[0]
    # (1) many equal distances: every B row at 10 from x, A = x repeated
    B = np.stack([at_dist(x, 10, rng)[0] for _ in range(40)])
    sb.job(sb.add(np.repeat(x[None], 12, 0)), sb.add(B))
    # (2) duplicated rows on both sides, with some distractors between them
    y = rnd(1)[0]
    A = np.concatenate([np.repeat(y[None], 6, 0), rnd(4), np.repeat(at_dist(y, 3, rng)[0][None], 5, 0)])
    B = np.concatenate([rnd(3), np.repeat(at_dist(y, 7, rng)[0][None], 4, 0), rnd(3), np.repeat(y[None], 3, 0)])
    sa, sbb = sb.add(A[rng.permutation(len(A))]), sb.add(B[rng.permutation(len(B))])
    sb.job(sa, sbb); sb.job(sbb, sa)
    # (3) every pair under the threshold: long steal chains
    z = rnd(1)[0]
    for n, p in ((200, 0.03), (150, 0.05), (64, 0.04)):
        A, B = flip(np.repeat(z[None], n, 0), p, rng), flip(np.repeat(z[None], n + 7, 0), p, rng)
        sb.job(sb.add(A), sb.add(B))
    # (4) the eviction of step 3: four B rows at 10 fill the list, a fifth at 10 is rejected, a later one at 5 evicts the lowest index
    B = [at_dist(x, 10, rng)[0] for _ in range(5)] + [at_dist(x, 5, rng)[0]]
    other = at_dist(x, 20, rng)[0]                                   # a second A row that also wants them
    sb.job(sb.add(np.stack([other, x])), sb.add(np.stack(B)))
    B2 = [at_dist(x, 10, rng)[0] for _ in range(4)] + [at_dist(x, 5, rng)[0], at_dist(x, 10, rng)[0], at_dist(x, 4, rng)[0]]
    sb.job(sb.add(np.stack([x, x, at_dist(x, 2, rng)[0]])), sb.add(np.stack(B2)))
    # (5) distances on each side of 40 and 50, one query row against one B row
    for d in (38, 39, 40, 41, 42, 48, 49, 50, 51, 52, 0, 256):
        sb.job(sb.add(x[None]), sb.add(at_dist(x, d, rng)[0][None]))
    #     and the ratio boundary: d1 against d2 (d1 < 0.8 d2 in float32; 32 vs 40 is not a match), both orders of the two rows
    for d1, d2 in ((32, 40), (31, 40), (32, 41), (24, 30), (23, 30), (36, 45), (35, 45), (40, 50), (39, 50), (40, 51), (16, 20), (0, 0),
                   (0, 1), (8, 10), (20, 20), (41, 60)):
        r1, used = at_dist(x, d1, rng)
        r2, _ = at_dist(x, d2, rng, avoid=used)
        far = rnd(2)
        sb.job(sb.add(x[None]), sb.add(np.stack([r1, r2, far[0]])))
        sb.job(sb.add(np.stack([rnd(1)[0], x])), sb.add(np.stack([far[1], r2, r1])))
    # (6) a set matched against itself, and skip flags on the adversarial rows
    A = flip(np.repeat(z[None], 120, 0), 0.05, rng)
    s = sb.add(A, rng.random(120) < 0.3)
    sb.job(s, s)
    return sb.batch()


def reference(bt, mode, **opts):
    """Per job the restatement's match list (tests/match_ref.py). DENSE reads the skip flags; KNN2 ignores them."""
    from tests import match_ref as mr
    out = []
    for a, b in zip(bt["set_a"], bt["set_b"]):
        A, sA = rows(bt, int(a)); B, sB = rows(bt, int(b))
        if mode == "dense":
            out.append(mr.dense(A, B, sA, sB, opts.get("dist_threshold", 50.0)))
        else:
            out.append(mr.knn2(A, B, opts.get("dist_threshold", 40.0), opts.get("ratio", 0.8)))
    return out
