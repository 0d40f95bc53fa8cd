#!/usr/bin/env python3
"""Times vocabulary training on the keyframe descriptor sets of the 5-agent synthetic map (the input of
tools/bowdb_bench.py: 2 196 sets, 1 018 089 rows), k = 10, L = 5:

  (a) device   Context.train_vocabulary, the whole call: upload, every level, weights, download. Median of --repeats after a warm-up.
  (b) serial   tests/cpp/voctrain_serial.cpp, the serial C++ restatement, on the same machine, run once.

The two vocabularies are compared bit for bit and the call's stats are recorded, among them the largest iteration count of one node:
how far the cap of D3 (max_iterations = 100) lies from these descriptors. Times are host clocks around calls that return after a stream
synchronise. Writes one JSON file (default profiles/voctrain_bench.json). Needs an MI355X."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from covins_amd import backend, capi, synth  # noqa: E402
from tests import match_util  # noqa: E402
from tests import voctrain_ref as vr  # noqa: E402
from tests import voctrain_util as vu  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--map", default="mh12345")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--L", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--limit", type=int, default=0, help="train on the first LIMIT sets only (0: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voctrain_bench.json"))
    a = ap.parse_args()
    m = synth.make_map(synth.config_named(a.map))
    sb, _, _ = match_util.keyframe_sets(m, seed=3, distractors=(20, 120))
    sets = sb.batch()
    S = len(sets["row_ptr"]) - 1 if a.limit <= 0 else min(a.limit, len(sets["row_ptr"]) - 1)
    ptr = np.ascontiguousarray(sets["row_ptr"][:S + 1], np.int32)
    desc = np.ascontiguousarray(sets["desc"][:ptr[S]], np.uint8)
    ctx = backend.Context(0)
    voc, stats = ctx.train_vocabulary(ptr, desc, a.k, a.L, seed=a.seed)            # warm-up
    times = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        voc_i, stats_i = ctx.train_vocabulary(ptr, desc, a.k, a.L, seed=a.seed)
        times.append(time.perf_counter() - t0)
        assert stats_i == stats and np.array_equal(voc_i["desc"], voc["desc"])
    ctx.close()
    print(json.dumps(dict(device_s=times, stats=stats)), flush=True)
    t0 = time.perf_counter()
    svoc, sstats, _ = vu.serial(ptr, desc, a.k, a.L, capi.BOW_TF_IDF, a.seed)
    serial_s = time.perf_counter() - t0
    try:
        vr.assert_same(voc, svoc, "bench")
        equal = bool([stats[k] for k in capi.VOCTRAIN_STATS[:6]] == sstats.tolist())
    except AssertionError:
        equal = False
    depth = np.zeros(len(voc["parent"]), np.int64)
    for n in range(1, len(depth)):
        depth[n] = depth[voc["parent"][n]] + 1
    out = dict(tool="tools/voctrain_bench.py", map=a.map, sets=int(S), descriptor_rows=int(ptr[S]), k=a.k, L=a.L, seed=a.seed,
               max_iterations=100, nodes=int(len(voc["parent"])), words=int(voc["num_words"]),
               words_by_depth=np.bincount(depth[voc["word_id"] >= 0], minlength=a.L + 1).tolist(),
               device_s=times, device_s_median=statistics.median(times), serial_s=serial_s,
               ratio_serial_over_device=serial_s / statistics.median(times),
               stats=stats, equal_to_serial=equal,
               note="one run on one box. device: the whole covgpu_voc_train call through the Python binding (upload of the rows, every "
                    "level with one host read per k-means iteration, the weights, download), median of %d after one warm-up call. "
                    "serial: tests/cpp/voctrain_serial.cpp compiled with g++ -O2, one thread, one run, on the same machine. No kernel "
                    "times were taken, and neither side was tuned against the other." % a.repeats)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: out[k] for k in ("device_s_median", "serial_s", "equal_to_serial", "nodes", "words")}))
    if not equal:
        raise SystemExit("the device and the serial restatement disagree")


if __name__ == "__main__":
    main()
