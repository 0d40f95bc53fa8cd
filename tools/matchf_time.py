#!/usr/bin/env python3
"""Times covgpu_match_float_batch: the whole call (upload, norms, scan, download, synchronise; median after warm-up)
for 1, 6, 64 and 1 024 jobs of 300 x 300 and 1 000 x 1 000 rows at dim 128, one query set against as many train sets as jobs (300 rows
is the front-end's nFeatures for SIFT). Rows are integer SIFT-like rows as the tests make them, a third of every train set noisy
copies of query rows. Two yardsticks are measured in the same run, as records and not as thresholds: (i) covgpu_match_batch mode KNN2
(32-byte ORB rows, Hamming) at the same row counts, and (ii) the numpy restatement of the contract on the host (float32 sgemm,
argpartition for the two nearest), on at most 32 jobs per point and scaled to the job count.

Kernel times come from a separate run under the profiler, which this tool then folds in:
    rocprofv3 --kernel-trace --stats -d DIR -o ks -- python tools/matchf_time.py --trace-run
    python tools/matchf_time.py --kernel-db DIR/<host>/ks_results.db          (the timing run; reads the scan kernel's dispatches)
The achieved fraction of the FP32 matrix peak is pairs * 2 * dim flop per kernel second against 157 TFLOP/s. Needs an MI355X."""
import argparse
import json
import os
import sqlite3
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from covins_amd import backend  # noqa: E402
from tests import matchf_ref as fr  # noqa: E402

DIM = 128
POINTS = [(rows, J) for rows in (300, 1000) for J in (1, 6, 64, 1024)]
TRACE_CALLS = 5                     # per point in the traced run; the first is dropped
PEAK_FP32_MATRIX = 157.0e12


def float_sets(rows, J, seed=0):
    rng = np.random.default_rng(seed)
    q = fr.sift_rows(rng, rows, DIM)
    base = [fr.train_rows(rng, q, rows) for _ in range(min(J, 64))]          # (beyond 64 train sets the rows repeat: the work is the same)
    return fr.make_sets([q] + [base[j % len(base)] for j in range(J)]), np.zeros(J, np.int32), np.arange(1, J + 1, dtype=np.int32)


def orb_sets(rows, J, seed=0):
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 256, (rows, 32), dtype=np.uint8)
    desc = [q]
    for _ in range(min(J, 64)):
        c = rng.integers(0, 256, (rows, 32), dtype=np.uint8)
        pick = rng.choice(rows, rows // 3, replace=False)
        flip = np.bitwise_and.reduce(rng.integers(0, 256, (4, rows // 3, 32), dtype=np.uint8), axis=0)   # about 16 of 256 bits
        c[rng.choice(rows, rows // 3, replace=False)] = q[pick] ^ flip
        desc.append(c)
    desc = [desc[0]] + [desc[1 + j % (len(desc) - 1)] for j in range(J)]
    return dict(row_ptr=np.arange(J + 2, dtype=np.int32) * rows, desc=np.concatenate(desc)), np.zeros(J, np.int32), np.arange(1, J + 1, dtype=np.int32)


def numpy_job(A, B, thr, ratio):
    """The contract in float32 on the host: sgemm, the two nearest by argpartition (ties by index), the two tests."""
    na = np.einsum("ij,ij->i", A, A); nb = np.einsum("ij,ij->i", B, B)
    D = np.maximum(np.float32(0), (na[:, None] + nb[None, :]) - np.float32(2) * (A @ B.T))
    two = np.argpartition(D, 1, axis=1)[:, :2]
    d = np.take_along_axis(D, two, 1)
    swap = (d[:, 1] < d[:, 0]) | ((d[:, 1] == d[:, 0]) & (two[:, 1] < two[:, 0]))
    i1 = np.where(swap, two[:, 1], two[:, 0])
    d1 = np.sqrt(np.where(swap, d[:, 1], d[:, 0])); d2 = np.sqrt(np.where(swap, d[:, 0], d[:, 1]))
    ok = (d1 <= np.float32(thr)) & (d1 < np.float32(ratio) * d2)
    return np.where(ok, i1, -1), int(ok.sum())


def timed(call, warmup, reps):
    for _ in range(warmup):
        r = call()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = call()
        t.append(1e3 * (time.perf_counter() - t0))
    return t, r


def kernel_times(db_path):
    """Per point the scan kernel's durations (ms) of the traced run: TRACE_CALLS dispatches per point in POINTS order, the first dropped."""
    db = sqlite3.connect(db_path)
    rows = db.execute("select name, start, end from kernels order by start").fetchall()
    scan = [(e - s) * 1e-6 for n, s, e in rows if "k_matchf_scan" in n]
    norms = [(e - s) * 1e-6 for n, s, e in rows if "k_matchf_norms" in n]
    if len(scan) != TRACE_CALLS * len(POINTS) or len(norms) != len(scan):
        raise SystemExit(f"{db_path}: {len(scan)} scan and {len(norms)} norm dispatches, expected {TRACE_CALLS * len(POINTS)} (was it a --trace-run?)")
    out = {}
    for i, p in enumerate(POINTS):
        out[p] = (scan[TRACE_CALLS * i + 1:TRACE_CALLS * (i + 1)], norms[TRACE_CALLS * i + 1:TRACE_CALLS * (i + 1)])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trace-run", action="store_true", help="only the float calls, TRACE_CALLS per point: the run to put under rocprofv3")
    ap.add_argument("--kernel-db", help="rocpd database of a traced --trace-run: its kernel times go into the output")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matchf_bench.json"))
    a = ap.parse_args()
    ctx = backend.Context(0)
    if a.trace_run:
        for rows, J in POINTS:
            sets, sa, sb = float_sets(rows, J)
            for _ in range(TRACE_CALLS):
                ctx.match_float_batch(sets, sa, sb)
        ctx.close()
        return
    kern = kernel_times(a.kernel_db) if a.kernel_db else None
    out_rows = []
    for rows, J in POINTS:
        reps = a.reps if J < 1024 else max(3, a.reps // 3)
        sets, sa, sb = float_sets(rows, J)
        t, r = timed(lambda: ctx.match_float_batch(sets, sa, sb), a.warmup, reps)
        osets, oa, ob = orb_sets(rows, J)
        to, ro = timed(lambda: ctx.match_batch(osets, oa, ob, "knn2"), a.warmup, reps)
        ptr, desc = sets["row_ptr"], sets["desc"]
        nj = min(J, 32)
        t0 = time.perf_counter()
        same = True
        for j in range(nj):
            m, n = numpy_job(desc[ptr[0]:ptr[1]], desc[ptr[j + 1]:ptr[j + 2]], 500.0, 0.8)
            same = same and n == int(r["nmatches"][j]) and np.array_equal(m, r["match"][r["offset"][j]:r["offset"][j + 1]])
        t_np = 1e3 * (time.perf_counter() - t0) / nj
        pairs = J * rows * rows
        row = dict(rows=rows, jobs=J, dim=DIM, reps=reps, call_ms=statistics.median(t), call_ms_min=min(t), call_ms_max=max(t),
                   pairs_per_s_call=pairs / (statistics.median(t) * 1e-3), mean_matches=float(r["nmatches"].mean()),
                   yardstick_orb_knn2_call_ms=statistics.median(to), yardstick_orb_knn2_call_ms_min=min(to),
                   yardstick_orb_mean_matches=float(ro["nmatches"].mean()),
                   yardstick_numpy_ms_per_job=t_np, yardstick_numpy_jobs_timed=nj, yardstick_numpy_ms_scaled=t_np * J,
                   numpy_same_matches=bool(same))
        if kern:
            ks, kn = kern[(rows, J)]
            k = statistics.median(ks)
            row.update(kernel_scan_ms=k, kernel_scan_ms_all=ks, kernel_norms_ms=statistics.median(kn),
                       tflops=pairs * 2.0 * DIM / (k * 1e-3) / 1e12, fraction_of_fp32_matrix_peak=pairs * 2.0 * DIM / (k * 1e-3) / PEAK_FP32_MATRIX)
        out_rows.append(row)
        print(json.dumps(row), flush=True)
    ctx.close()
    out = dict(tool="tools/matchf_time.py", note="One run on one machine. call_ms: the whole covgpu_match_float_batch call through the Python "
               "binding, median (min, max beside it). yardstick_orb_knn2_*: covgpu_match_batch mode KNN2 on 32-byte rows at the same row "
               "counts in the same run, a code path this kernel does not touch. yardstick_numpy_*: the contract in float32 numpy (sgemm, "
               "argpartition) on the same machine's host, timed on at most 32 jobs and scaled to the job count; numpy_same_matches: its "
               "matches equal the library's on those jobs (integer rows: every intermediate is exact). kernel_*: k_matchf_scan / "
               "k_matchf_norms durations from a separate run under rocprofv3 --kernel-trace --stats (5 calls per point, the first "
               "dropped), median; fraction_of_fp32_matrix_peak = pairs * 2 * dim flop / kernel_scan_ms against 157 TFLOP/s. Yardsticks "
               "are records, not thresholds.", peak_fp32_matrix_tflops=PEAK_FP32_MATRIX / 1e12, kernel_times_from_trace=bool(kern),
               rows=out_rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
