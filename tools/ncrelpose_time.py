"""Time of covgpu_ncrelpose_batch (COVINS-G's 17-point stage, polish and loop covariance) per batch: 1, 10 and 100
candidates of 6 x 100 correspondences with 20 % wrong matches, with the reference's defaults, beside the numpy checker per job
(tests/ncrelpose_ref.py, route A: a scale, not the reference's C++ opengv, which is not available to measure). Host wall clock around
the whole call (upload, one launch, download, synchronise), median and spread of `reps` calls after a warm-up. Writes
profiles/ncrelpose_bench.json, or the file named by the second argument. Usage: python tools/ncrelpose_time.py [reps] [out.json]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from covins_amd import backend  # noqa: E402
from tests import ncrelpose_ref as nr, ncrelpose_util as nu  # noqa: E402


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "ncrelpose_bench.json")
    ctx = backend.Context(0)
    rows = []
    print(f"{'jobs':>6} {'corr':>8} {'iters(mean)':>11} {'found':>6} {'ms median':>10} {'ms min':>8} {'ms max':>8} {'us/job':>8} {'numpy ms/job':>13}")
    for num in (1, 10, 100):
        jobs = [nu.job([100] * 6, 0.20, 2e-4, 100000 * num + k) for k in range(num)]
        seeds = [1000 * num + k for k in range(num)]
        bt = nu.batch(jobs, seeds)
        res = ctx.ncrelpose_batch(bt)       # warm-up (code object load, first allocations)
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            ctx.ncrelpose_batch(bt)
            ts.append((time.perf_counter() - t0) * 1e3)
        ts = np.array(ts)
        m = min(num, 3)                     # the checker on the first jobs only
        t0 = time.perf_counter()
        ref = [nr.run(j, s, "a") for j, s in zip(jobs[:m], seeds[:m])]
        ref_ms = (time.perf_counter() - t0) * 1e3 / m
        same = all(r["status"] == res["status"][b] and r["iterations"] == res["iterations"][b] and r["rows"] == res["cov_rows"][b] for b, r in enumerate(ref))
        rows.append(dict(jobs=num, correspondences=int(bt["ptr"][-1]), iterations_mean=float(res["iterations"].mean()),
                         cov_draws_mean=float(res["cov_draws"].mean()), found=int((res["status"] == 0).sum()), ms_median=float(np.median(ts)),
                         ms_min=float(ts.min()), ms_max=float(ts.max()), numpy_ms_per_job=ref_ms, numpy_jobs=m, numpy_agrees=bool(same)))
        print(f"{num:>6} {int(bt['ptr'][-1]):>8} {res['iterations'].mean():>11.1f} {int((res['status'] == 0).sum()):>6} {np.median(ts):>10.3f} "
              f"{ts.min():>8.3f} {ts.max():>8.3f} {np.median(ts) * 1e3 / num:>8.1f} {ref_ms:>13.1f}")
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    out = dict(what="covgpu_ncrelpose_batch, host wall clock per call; one run on one box", reps=reps, limits=backend.ncrelpose_limits(), rows=rows)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
