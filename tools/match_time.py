"""Host wall clock of covgpu_match_batch: 1, 5, 64 and 1 024 jobs of 1 000 x 1 000 rows in both modes, one query set
against as many candidate sets as jobs (the loop-candidate shape: one query keyframe, several candidates). Each candidate holds 300
noisy copies of query rows (bit-flip probability 0.06, shuffled) among random rows, and a fifth of its rows are skipped in DENSE.
The time is the whole call: upload, both launches, download, synchronise; median and spread after warm-up. Needs the GPU.
Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats` (--reps 5 keeps it short)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from covins_amd import backend  # noqa: E402
from tests import match_util as mu  # noqa: E402


def make_sets(J, n=1000, seed=0):
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    desc, skip = [q], [rng.random(n) < 0.2]
    for _ in range(J):
        c = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        pick = rng.choice(n, 300, replace=False)
        c[rng.choice(n, 300, replace=False)] = mu.flip(q[pick], 0.06, rng)
        desc.append(c); skip.append(rng.random(n) < 0.2)
    ptr = np.arange(J + 2, dtype=np.int32) * n
    return dict(row_ptr=ptr, desc=np.concatenate(desc), skip=np.concatenate(skip).astype(np.uint8)), np.zeros(J, np.int32), np.arange(1, J + 1, dtype=np.int32)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", default="1,5,64,1024")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    ctx = backend.Context(0)
    for J in [int(x) for x in a.jobs.split(",")]:
        sets, sa, sb = make_sets(J)
        for mode in ("dense", "knn2"):
            s = sets if mode == "dense" else dict(sets, skip=None)
            for _ in range(a.warmup):
                r = ctx.match_batch(s, sa, sb, mode)
            reps = a.reps if J < 1024 else max(3, a.reps // 3)
            t = []
            for _ in range(reps):
                t0 = time.perf_counter()
                r = ctx.match_batch(s, sa, sb, mode)
                t.append(time.perf_counter() - t0)
            t = np.array(t) * 1e3
            pairs = J * 1000 * 1000
            print(json.dumps(dict(mode=mode, jobs=J, rows=1000, reps=reps, ms_median=round(float(np.median(t)), 4),
                                  ms_min=round(float(t.min()), 4), ms_p90=round(float(np.percentile(t, 90)), 4),
                                  pairs_per_s_wall=float(pairs / (np.median(t) * 1e-3)), mean_matches=float(r["nmatches"].mean()))), flush=True)
    ctx.close()
