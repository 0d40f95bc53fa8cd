#!/usr/bin/env python3
"""Times Context.marginal_covariance on the 5-agent synthetic map, visual-inertial, mu = 0: two keyframes of different
agents with the pose rows (12 columns) and 32 keyframes with all rows (480 columns). Per selection: the whole call (upload, linearisation,
factorisation, sweep; median after one warm-up), the resident call (no upload), and beside them one covgpu_gn_step of the same context and
problem from the same run — the same upload, linearisation and factorisation without the sweep. sweep_ms = the whole call minus the
Gauss-Newton step, both medians: the host plan of the sweep, its launches and the copy of the result. Nothing existed before this to
compare with, so the file states numbers and ratios, no threshold. Writes one JSON file (default profiles/marginal_bench.json). Needs an
MI355X."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from covins_amd import backend, mapdata, synth  # noqa: E402


def _median_ms(fn, repeats):
    fn()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(t), t, out


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--map", default="mh12345")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "marginal_bench.json"))
    a = ap.parse_args()
    m = synth.make_map(synth.config_named(a.map))
    prob, idx = mapdata.flatten_gba(m, visual_only=False, loop_loss=True)
    opt = backend.default_options()
    free = np.flatnonzero(prob.kf_fixed == 0)
    client = np.asarray(m.kf_client)[np.asarray(idx.kf_rows)]
    first, last = int(free[len(free) // 7]), int(next(k for k in free[::-1] if client[k] != client[free[len(free) // 7]]))
    lim = backend.marginal_limits()
    wide = [int(free[i]) for i in np.linspace(0, len(free) - 1, lim["max_kf"]).astype(int)]
    ctx = backend.Context(0)
    gn_ms, gn_all, _ = _median_ms(lambda: ctx.gn_step(prob, opt, 0.0), a.repeats)
    rows = []
    for name, kfs, block in (("two keyframes of different agents, pose rows", [first, last], "pose"), ("32 keyframes, all rows", wide, "full")):
        call_ms, call_all, (cov, st) = _median_ms(lambda: ctx.marginal_covariance(prob, opt, kfs, block=block, mu=0.0), a.repeats)
        res_ms, res_all, (cov_r, _) = _median_ms(lambda: ctx.marginal_covariance_resident(opt, kfs, block=block, mu=0.0), a.repeats)
        row = dict(selection=name, keyframes=len(kfs), block=block, stats=st, call_ms=call_ms, call_ms_all=call_all, resident_ms=res_ms,
                   resident_ms_all=res_all, gn_step_ms=gn_ms, sweep_ms=call_ms - gn_ms, call_over_gn_step=call_ms / gn_ms,
                   sweep_over_gn_step=(call_ms - gn_ms) / gn_ms, resident_equals_call=bool(np.array_equal(cov, cov_r)),
                   symmetric=bool(np.array_equal(cov, cov.T)), min_diag=float(np.diag(cov).min()))
        rows.append(row)
        print(json.dumps(row), flush=True)
    ctx.close()
    out = dict(tool="tools/marginal_bench.py", map=a.map, unknowns=int(15 * prob.K), keyframes=int(prob.K), repeats=a.repeats, gn_step_ms_all=gn_all,
               note="call_ms: Context.marginal_covariance through the Python binding (upload, linearisation, factorisation at mu = 0, sweep, "
               "download), median; resident_ms: the same without the upload; gn_step_ms: Context.gn_step of the same context and problem in "
               "the same run (upload, linearisation, factorisation, both substitutions, download); sweep_ms = call_ms - gn_step_ms. One run "
               "on one machine.", rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
