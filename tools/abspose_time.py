"""Time of covgpu_abspose_ransac_batch (loop-candidate geometric verification) per batch, on synthetic candidates of
100-1 000 correspondences with 10-60 % outliers (tests/abspose_util.random_batch), against the numpy restatement per candidate
(tests/abspose_ref.py: a scale, not the reference's C++ opengv). Host wall clock around the whole call (upload, one launch, download,
synchronise), median and spread of `reps` calls after a warm-up. Usage: python tools/abspose_time.py [reps]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from covins_amd import backend  # noqa: E402
from tests import abspose_ref as ar, abspose_util as au  # noqa: E402


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    ctx = backend.Context(0)
    rng = np.random.default_rng(0)
    print(f"{'candidates':>10} {'corr':>8} {'iters(mean)':>11} {'ms median':>10} {'ms min':>8} {'ms max':>8} {'us/cand':>8}")
    for num in (1, 8, 256, 2000):
        sizes = list(rng.integers(100, 1001, num))
        bt = au.random_batch(sizes, seed=num, outlier_frac=float(rng.uniform(0.1, 0.6)), with_ref=False)
        res = ctx.abspose_ransac_batch(bt)   # warm-up (code object load, first allocations)
        ts = []
        for _ in range(reps):
            t = time.perf_counter()
            ctx.abspose_ransac_batch(bt)
            ts.append((time.perf_counter() - t) * 1e3)
        ts = np.array(ts)
        print(f"{num:>10} {int(bt['ptr'][-1]):>8} {res['iterations'].mean():>11.1f} {np.median(ts):>10.3f} {ts.min():>8.3f} {ts.max():>8.3f} "
              f"{np.median(ts) * 1e3 / num:>8.1f}")
    bt = au.random_batch(list(rng.integers(100, 1001, 8)), seed=99, outlier_frac=0.35, with_ref=False)
    t = time.perf_counter()
    ar.ransac_batch(bt, bt["seed"])
    print(f"numpy restatement: {(time.perf_counter() - t) * 1e3 / 8:.1f} ms per candidate (8 candidates, 35 % outliers)")
    ctx.close()


if __name__ == "__main__":
    main()
