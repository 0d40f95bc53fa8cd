#!/usr/bin/env python3
"""Times covgpu_prune_redundant on the single-agent and the 5-agent synthetic map, in threshold mode at 0.95 and in
count mode at K/2: the whole C call (median of five after one warm-up), the greedy-loop kernel alone (HIP events around it) and its time
per round, and the serial C++ restatement of the reference loop (tests/cpp/facade_prune_shim.cpp) on the same map in the same run.
Writes one JSON file (default profiles/prune_bench.json). Needs an MI355X."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from covins_amd import backend, synth  # noqa: E402
from tests import prune_ref as pr  # noqa: E402
from tests import prune_util as pu  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--maps", default="mh01,mh12345")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-serial", action="store_true", help="skip the serial restatement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prune_bench.json"))
    a = ap.parse_args()
    ctx = backend.Context(0)
    rows = []
    for name in a.maps.split(","):
        m = synth.make_map(synth.config_named(name))
        m.clean()
        inp = pr.inputs_of_map(m)
        for mode, opts in (("threshold 0.95", dict(th_red=0.95)), ("count K/2", dict(max_kfs=m.K // 2))):
            call = lambda: ctx.prune_redundant(inp["lm_obs_ptr"], inp["obs_kf"], inp["kf_pred"], inp["kf_succ"], inp["kf_time"],
                                               inp["lm_invalid"], inp["kf_invalid"], inp["kf_first"], inp["kf_loop"], loop_ms=True, **opts)
            call()
            wall, loop = [], []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                r = call()
                wall.append(1e3 * (time.perf_counter() - t0)); loop.append(r["loop_ms"])
            row = dict(map=name, mode=mode, keyframes=int(m.K), landmarks=int(m.L), observations=int(m.O), rounds=r["num_rounds"],
                       erased=int((r["round_action"] == 0).sum()), removed=r["removed"], stop_reason=r["stop_reason"],
                       call_ms=statistics.median(wall), call_ms_all=wall, loop_kernel_ms=statistics.median(loop),
                       loop_us_per_round=1e3 * statistics.median(loop) / max(r["num_rounds"], 1))
            if not a.no_serial:
                sm = pu.StandinPruneMap(m)
                s = sm.serial(th_red=opts.get("th_red", 0.95), max_kfs=opts.get("max_kfs"))
                sm.close()
                row.update(serial_ms=s["ms"], serial_rounds=s["num_rounds"], serial_removed=s["removed"],
                           serial_us_per_round=1e3 * s["ms"] / max(s["num_rounds"], 1), speedup_call=s["ms"] / row["call_ms"],
                           same_sequence=bool(np.array_equal(s["round_kf"], r["round_kf"]) and np.array_equal(s["round_action"], r["round_action"])))
            rows.append(row)
            print(json.dumps(row), flush=True)
    ctx.close()
    out = dict(tool="tools/prune_bench.py", repeats=a.repeats, note="call_ms: the whole covgpu_prune_redundant call through the Python binding, "
               "median; loop_kernel_ms: k_prune_loop alone between HIP events; serial_ms: the serial restatement of the reference loop "
               "on the host of the same machine, one run, reading each landmark's observation count in place (the reference copies the map)",
               rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
