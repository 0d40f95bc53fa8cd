#!/usr/bin/env python3
"""Times Context.keyframe_covariances_resident on the 5-agent synthetic map, visual-inertial, mu = 0, through the Python
binding, against the only route there was before it: the loop of Context.marginal_covariance_resident over all free keyframes in groups of
32. All figures come from one run, medians after one warm-up: one covgpu_gn_step; the resident all-keyframe call at block "pose" and "full",
without pairs and with every off-diagonal block pair of the oracle's S ("pose") / every IMU factor ("full"); the loop of 32-keyframe calls at
both blocks. With them: scratch bytes, launches per form, the smallest diagonal entry, and the largest difference between the two routes'
diagonal blocks relative to the largest entry. Acceptance: the one call is faster than the loop in this run. Writes one JSON file (default
profiles/selinv_bench.json). Needs an MI355X."""
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


def _system_pairs(prob):
    from oracle import covo
    ptr, col, blocks, b, cost = covo.schur_sparse(prob, covo.default_options(visual_only=0), 0.0)
    blocks = np.asarray(blocks)
    out = []
    for i in range(len(ptr) - 1):
        for e in range(ptr[i], ptr[i + 1]):
            j = int(col[e])
            if j != i and not prob.kf_fixed[i] and not prob.kf_fixed[j] and np.any(blocks[e] != 0):
                out.append((i, j))
    return sorted(set(out) | {(j, i) for i, j in out})


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--map", default="mh12345")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "selinv_bench.json"))
    a = ap.parse_args()
    m = synth.make_map(synth.config_named(a.map))
    prob, idx = mapdata.flatten_gba(m, visual_only=False, loop_loss=True)
    opt = backend.default_options()
    free = [int(k) for k in np.flatnonzero(prob.kf_fixed == 0)]
    lim = backend.marginal_limits()
    groups = [free[i:i + lim["max_kf"]] for i in range(0, len(free), lim["max_kf"])]
    s_pairs = _system_pairs(prob)
    i_pairs = sorted({(int(i), int(j)) for i, j in zip(prob.imu_kf_i, prob.imu_kf_j) if not prob.kf_fixed[i] and not prob.kf_fixed[j]} |
                     {(int(j), int(i)) for i, j in zip(prob.imu_kf_i, prob.imu_kf_j) if not prob.kf_fixed[i] and not prob.kf_fixed[j]})
    ctx = backend.Context(0)
    gn_ms, gn_all, _ = _median_ms(lambda: ctx.gn_step(prob, opt, 0.0), a.repeats)
    ctx.upload(prob, opt)
    rows = []
    for block, pairs in (("pose", s_pairs), ("full", i_pairs)):
        d = 6 if block == "pose" else 15

        def loop():
            out = np.zeros((prob.K, d, d))
            for g in groups:
                cov, _ = ctx.marginal_covariance_resident(opt, g, block=block, mu=0.0)
                for t, k in enumerate(g):
                    out[k] = cov[d * t:d * t + d, d * t:d * t + d]
            return out

        one_ms, one_all, (kc, _, _, st) = _median_ms(lambda: ctx.keyframe_covariances_resident(opt, block=block, mu=0.0), a.repeats)
        pr_ms, pr_all, (kc2, pc, ok, st2) = _median_ms(lambda: ctx.keyframe_covariances_resident(opt, block=block, mu=0.0, pairs=pairs), a.repeats)
        loop_ms, loop_all, lc = _median_ms(loop, a.repeats)
        diag = np.diagonal(kc[free], axis1=1, axis2=2)
        row = dict(block=block, keyframes=len(free), stats=st, one_call_ms=one_ms, one_call_ms_all=one_all, pairs=len(pairs),
                   pairs_served=int(ok.sum()), with_pairs_ms=pr_ms, with_pairs_ms_all=pr_all, stats_with_pairs=st2,
                   loop_calls=len(groups), loop_ms=loop_ms, loop_ms_all=loop_all, loop_over_one_call=loop_ms / one_ms,
                   loop_over_with_pairs=loop_ms / pr_ms, gn_step_ms=gn_ms, one_call_over_gn_step=one_ms / gn_ms,
                   one_call_faster_than_loop=bool(one_ms < loop_ms), same_bits_with_pairs=bool(np.array_equal(kc, kc2)),
                   symmetric=bool(np.array_equal(kc, kc.transpose(0, 2, 1))), min_diag=float(diag.min()),
                   max_diff_to_loop_rel=float(np.abs(kc - lc).max() / np.abs(lc).max()))
        rows.append(row)
        print(json.dumps(row), flush=True)
    ctx.close()
    out = dict(tool="tools/selinv_bench.py", map=a.map, unknowns=int(15 * prob.K), keyframes=int(prob.K), repeats=a.repeats, gn_step_ms_all=gn_all,
               note="one_call_ms: Context.keyframe_covariances_resident through the Python binding (linearisation, factorisation at mu = 0, the "
               "top-down sweep, read-out, download) without pairs, with_pairs_ms: with every off-diagonal block pair of the oracle's S (pose) / "
               "every IMU factor (full), both orders; loop_ms: Context.marginal_covariance_resident over all free keyframes in groups of 32, "
               "diagonal blocks copied out; gn_step_ms: Context.gn_step of the same context and problem. Medians of `repeats` after one "
               "warm-up, all from one run on one machine.", rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    if not all(r["one_call_faster_than_loop"] for r in rows):
        sys.exit("the one call is not faster than the loop of 32-keyframe calls")


if __name__ == "__main__":
    main()
