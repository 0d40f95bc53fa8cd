#!/usr/bin/env python3
"""Times the arrival of a keyframe at a running place-recognition server in two forms, on the 5-agent synthetic map
(2 196 keyframes) with a seeded synthetic vocabulary:

  (a) resident    BowDb.put_descriptors + set_neighbours + query + add on one covgpu_bowdb handle
  (b) stateless   Context.bow_transform_batch of the one set + Context.detect_candidates_batch with one query over the table so far

Both forms see the same inputs (a keyframe's connected list holds the keyframes that arrived before it; the reference minimum score is
computed), run alternately keyframe by keyframe in the same process after a warm-up, and their candidates are compared. Times are host
clocks around calls that end in a stream synchronise. Writes one JSON file (default profiles/bowdb_bench.json). Needs an MI355X."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import scipy.sparse as sp  # noqa: E402

from covins_amd import backend, synth  # noqa: E402
from tests import bow_util as bu  # noqa: E402
from tests import match_util  # noqa: E402

SIZES = (100, 500, 1000, 2000)
WINDOW = 25                                        # steps on either side of a size that form its sample


def neighbours_before(kf_lms, num_lm, min_shared=15):
    """Per keyframe the earlier keyframes that share at least min_shared landmarks, by descending count (ties: lower index first)."""
    K = len(kf_lms)
    rows = np.concatenate([np.full(len(s), k) for k, s in enumerate(kf_lms)])
    A = sp.csr_matrix((np.ones(len(rows), np.int32), (rows, np.concatenate([np.asarray(s, np.int64) for s in kf_lms]))), shape=(K, num_lm))
    A.sum_duplicates()
    A.data[:] = 1
    C = (A @ A.T).tocsr()
    out = []
    for k in range(K):
        idx, cnt = C.indices[C.indptr[k]:C.indptr[k + 1]], C.data[C.indptr[k]:C.indptr[k + 1]]
        keep = (idx < k) & (cnt >= min_shared)
        out.append([int(i) for _, i in sorted(zip(-cnt[keep], idx[keep]))])
    return out


def pct(x, p):
    return float(np.percentile(np.asarray(x), p))


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--map", default="mh12345")
    ap.add_argument("--k", type=int, default=10, help="branching factor of the synthetic vocabulary")
    ap.add_argument("--L", type=int, default=5, help="its depth: k^L words")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=60, help="keyframes replayed in both forms before the timed replays")
    ap.add_argument("--limit", type=int, default=0, help="replay only the first LIMIT keyframes (0: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bowdb_bench.json"))
    a = ap.parse_args()
    m = synth.make_map(synth.config_named(a.map))
    sb, _, kf_lms = match_util.keyframe_sets(m, seed=3, distractors=(20, 120))
    sets = sb.batch()
    ptr, desc = np.ascontiguousarray(sets["row_ptr"], np.int32), np.ascontiguousarray(sets["desc"], np.uint8)
    K = m.K if a.limit <= 0 else min(m.K, a.limit)
    voc = bu.random_vocab(k=a.k, L=a.L, seed=0)
    nbs = neighbours_before(kf_lms, m.L)
    ctx = backend.Context(0)
    full = ctx.bow_transform_batch(voc, dict(row_ptr=ptr[:K + 1], desc=desc[:ptr[K]]))     # the table of form (b), sliced per step
    nptr = np.zeros(K + 1, np.int32); nptr[1:] = np.cumsum([len(nbs[k]) for k in range(K)])
    nb = np.ascontiguousarray(np.concatenate([np.asarray(nbs[k], np.int32) for k in range(K)] + [np.zeros(0, np.int32)]), np.int32)
    kid, client = np.ascontiguousarray(m.kf_id[:K], np.int32), np.ascontiguousarray(m.kf_client[:K], np.int32)
    order = np.arange(K, dtype=np.int32)
    one = lambda i: dict(row_ptr=ptr[i:i + 2] - ptr[i], desc=desc[ptr[i]:ptr[i + 1]])
    N, W = len(voc["parent"]), int(voc["num_words"])
    voc_bytes = 4 * (N + 1) + 4 * (N - 1) + 32 * N + 4 * N + 8 * W

    def step_a_bytes(db, i):
        """The four calls of a resident step with the handle's byte counters read after each."""
        moved = 0
        for call in (lambda: db.put_descriptors([i], kid[i:i + 1], client[i:i + 1], one(i)), lambda: db.set_neighbours([i], [nbs[i]]),
                     lambda: db.query([i], [nbs[i]], cap=i), lambda: db.add([i])):
            call()
            st = db.stats()
            moved += st["h2d_bytes"] + st["d2h_bytes"]
        return moved

    def step_a_timed(db, i):
        """The same four calls without the stats between them: the time of the step."""
        t0 = time.perf_counter()
        db.put_descriptors([i], kid[i:i + 1], client[i:i + 1], one(i))
        db.set_neighbours([i], [nbs[i]])
        got = db.query([i], [nbs[i]], cap=i)
        t1 = time.perf_counter()
        db.add([i])
        t2 = time.perf_counter()
        return 1e3 * (t2 - t0), 1e3 * (t2 - t1), got

    def step_b(i):
        t0 = time.perf_counter()
        ctx.bow_transform_batch(voc, one(i))
        e = int(full["bow_ptr"][i + 1])
        table = dict(id=kid[:i + 1], client=client[:i + 1], bow_ptr=full["bow_ptr"][:i + 2], word=full["word"][:e], value=full["value"][:e],
                     nb_ptr=nptr[:i + 2], nb=nb[:nptr[i + 1]])
        got = ctx.detect_candidates_batch(table, order[:i], [i], [i], cap=i)
        return 1e3 * (time.perf_counter() - t0), got

    def bytes_b(i):
        rows, e, nn = int(ptr[i + 1] - ptr[i]), int(full["bow_ptr"][i + 1]), int(nptr[i + 1])
        db_words = int(full["bow_ptr"][i])
        up = voc_bytes + 32 * rows + 8 + 8 * (i + 1) + 4 * (i + 2) + 12 * e + 4 * (i + 2) + 4 * nn + 4 * i + 4 * (i + 1) + 4 * (W + 1) + 4 * db_words + 8
        up += 8 * len(nbs[i]) + 8
        down = 12 * rows + 8 * rows + 4 + (4 * 4 + 8) + 8 * i
        return up + down

    for i in range(min(a.warmup, K)):                                     # warm-up: both forms, a handle of its own
        if i == 0:
            warm = ctx.bowdb(voc)
        step_a_timed(warm, i); step_b(i)
    warm.close()
    repeats, same = [], True
    for rep in range(a.repeats):
        db = ctx.bowdb(voc)
        ta, tb, tadd, rebuild_ms, rebuilds = [], [], [], 0.0, 0
        for i in range(K):
            if (i + rep) % 2 == 0:
                t, t_add, ga = step_a_timed(db, i); tb_i, gb = step_b(i)
            else:
                tb_i, gb = step_b(i); t, t_add, ga = step_a_timed(db, i)
            st = db.stats()
            if st["rebuilds"] != rebuilds:
                rebuilds = st["rebuilds"]; rebuild_ms += t_add           # the add that rebuilt, the add itself included
            ta.append(t); tb.append(tb_i); tadd.append(t_add)
            same = same and ga["candidates"][0].tolist() == gb["candidates"][0].tolist() and \
                ga["acc_score"][0].view(np.uint32).tolist() == gb["acc_score"][0].view(np.uint32).tolist()
        st = db.stats()
        db.close()
        at = {}
        for s in SIZES:
            if s + WINDOW > K:
                continue
            w = slice(s - WINDOW, s + WINDOW)
            at[str(s)] = dict(resident_ms_median=statistics.median(ta[w]), resident_ms_p90=pct(ta[w], 90), stateless_ms_median=statistics.median(tb[w]),
                              stateless_ms_p90=pct(tb[w], 90), ratio_stateless_over_resident=statistics.median(tb[w]) / statistics.median(ta[w]))
        row = dict(repeat=rep, at_database_size=at, resident_total_s=sum(ta) / 1e3, stateless_total_s=sum(tb) / 1e3, rebuilds=int(st["rebuilds"]),
                   rebuild_adds_ms_total=rebuild_ms, add_ms_median=statistics.median(tadd), device_bytes=int(st["device_bytes"]))
        repeats.append(row)
        print(json.dumps(row), flush=True)
    if not same:
        raise SystemExit("the two forms returned different candidates")
    # bytes moved per step: form (a) from the handle's counters in a pass of its own, form (b) from the shapes
    db = ctx.bowdb(voc)
    moved = {}
    for i in range(K):
        mv = step_a_bytes(db, i)
        if i in SIZES:
            moved[str(i)] = dict(resident_bytes=int(mv), stateless_bytes=int(bytes_b(i)))
    db.close()
    ctx.close()
    out = dict(tool="tools/bowdb_bench.py", map=a.map, keyframes=int(K), descriptor_rows=int(ptr[K]), vocabulary_words=W, vocabulary_nodes=N,
               vocabulary_bytes=int(voc_bytes), tail_limit=256, repeats=repeats, bytes_per_step=moved, same_candidates=bool(same),
               note="one run on one box. resident: put_descriptors + set_neighbours + query + add on a covgpu_bowdb handle; stateless: "
                    "bow_transform_batch of the one set + detect_candidates_batch with one query over the table so far (the parent "
                    "commit's entry points), alternating keyframe by keyframe in the same process. Per database size: median and 90th "
                    "percentile over the %d steps around it, host clock around calls that end in a stream synchronise, Python binding "
                    "included on both sides. The vocabulary is synthetic with %d words; ORBvoc has about 10^6, which makes the stateless "
                    "form's per-step vocabulary upload about ten times larger than measured here. stateless_bytes is computed from the "
                    "shapes of the call, resident_bytes is read from covgpu_bowdb_stats." % (2 * WINDOW, W))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
