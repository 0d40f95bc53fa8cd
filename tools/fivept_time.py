"""Time of covgpu_fivept_ransac_batch (COVINS-G's five-point relative-pose RANSAC) per batch: 6, 60 and 600 jobs of
300 correspondences with 30 % wrong matches (6 = the 2 x 3 grid of one loop candidate), beside the numpy checker per job
(tests/fivept_ref.py, route A: a scale, not the reference's C++ opengv, which is not available to measure). Host wall clock around
the whole call (upload, one launch, download, synchronise), median and spread of `reps` calls after a warm-up. Writes
profiles/fivept_bench.json. Usage: python tools/fivept_time.py [reps]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from covins_amd import backend  # noqa: E402
from tests import fivept_ref as fr, fivept_util as fu  # noqa: E402


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    ctx = backend.Context(0)
    rows = []
    print(f"{'jobs':>6} {'corr':>8} {'iters(mean)':>11} {'found':>6} {'ms median':>10} {'ms min':>8} {'ms max':>8} {'us/job':>8} {'numpy ms/job':>13}")
    for num in (6, 60, 600):
        jobs = []
        for k in range(num):
            f1, f2, R, t = fu._perturbed(np.random.default_rng([num, k]), 300, 90)
            jobs.append(dict(f1=f1, f2=f2, seed=1000 * num + k))
        bt = fu.batch(jobs)
        res = ctx.fivept_ransac_batch(bt)   # warm-up (code object load, first allocations)
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            ctx.fivept_ransac_batch(bt)
            ts.append((time.perf_counter() - t0) * 1e3)
        ts = np.array(ts)
        m = min(num, 6)                     # the checker on the first jobs only: it takes ~0.1 s per job
        t0 = time.perf_counter()
        ref = [fr.ransac(j["f1"], j["f2"], j["seed"]) for j in jobs[:m]]
        ref_ms = (time.perf_counter() - t0) * 1e3 / m
        same = all(r["status"] == res["status"][b] and r["iterations"] == res["iterations"][b] for b, r in enumerate(ref))
        rows.append(dict(jobs=num, correspondences=int(bt["ptr"][-1]), iterations_mean=float(res["iterations"].mean()),
                         found=int((res["status"] == 0).sum()), ms_median=float(np.median(ts)), ms_min=float(ts.min()), ms_max=float(ts.max()),
                         numpy_ms_per_job=ref_ms, numpy_jobs=m, numpy_agrees=bool(same)))
        print(f"{num:>6} {int(bt['ptr'][-1]):>8} {res['iterations'].mean():>11.1f} {int((res['status'] == 0).sum()):>6} {np.median(ts):>10.3f} "
              f"{ts.min():>8.3f} {ts.max():>8.3f} {np.median(ts) * 1e3 / num:>8.1f} {ref_ms:>13.1f}")
    ctx.close()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    out = dict(what="covgpu_fivept_ransac_batch, host wall clock per call; one run on one box", reps=reps, limits=backend.fivept_limits(), rows=rows)
    with open(os.path.join(ROOT, "profiles", "fivept_bench.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
