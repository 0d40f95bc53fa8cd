#!/usr/bin/env python3
"""Times covgpu_landmark_refresh on the single-agent and the 5-agent synthetic map, descriptors made as the tests
make them (noisy copies of a per-landmark pattern): the whole C call (median of five after one warm-up), the kernels alone (HIP
events around them), and the serial C++ restatement of Landmark::ComputeDescriptor + Landmark::UpdateNormal
(tests/cpp/facade_refresh_shim.cpp) on the same map in the same run. The restatement copies no observation map and takes no mutex, so
it is favoured over the reference. Writes one JSON file (default profiles/lmrefresh_bench.json). Needs an MI355X."""
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
from tests import lmrefresh_ref as lr  # noqa: E402
from tests import lmrefresh_util as lu  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--maps", default="mh01,mh12345")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-serial", action="store_true", help="skip the serial restatement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lmrefresh_bench.json"))
    a = ap.parse_args()
    ctx = backend.Context(0)
    rows = []
    for name in a.maps.split(","):
        m = synth.make_map(synth.config_named(name))
        inp = lu.inputs_of_map(m, lu.map_descriptors(m))
        call = lambda: ctx.refresh_landmarks(inp["lm_obs_ptr"], inp["obs_kf"], inp["obs_desc"], inp["obs_octave"], inp["lm_ref_obs"],
                                             inp["lm_pos"], inp["kf_center"], inp["kf_invalid"], inp["lm_invalid"], kernel_ms=True)
        call()
        wall, kern = [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            r = call()
            wall.append(1e3 * (time.perf_counter() - t0)); kern.append(r["kernel_ms"])
        lens = np.diff(inp["lm_obs_ptr"])
        row = dict(map=name, keyframes=int(m.K), landmarks=int(m.L), observations=int(m.O), mean_track=float(lens.mean()),
                   max_track=int(lens.max()), form_count=r["form_count"].tolist(), call_ms=statistics.median(wall), call_ms_all=wall,
                   kernel_ms=statistics.median(kern), kernel_ms_all=kern)
        if not a.no_serial:
            sm = lu.StandinRefreshMap(inp)
            s = sm.serial()
            sm.close()
            same = all(np.array_equal(np.ascontiguousarray(s[k]).view(np.uint8), np.ascontiguousarray(r[k]).view(np.uint8)) for k in lr.OUTPUTS)
            row.update(serial_ms=s["ms"], speedup_call=s["ms"] / row["call_ms"], speedup_kernel=s["ms"] / row["kernel_ms"],
                       same_as_serial=bool(same))
        rows.append(row)
        print(json.dumps(row), flush=True)
    ctx.close()
    out = dict(tool="tools/lmrefresh_bench.py", repeats=a.repeats, note="call_ms: the whole covgpu_landmark_refresh call through the Python "
               "binding (uploads, kernels, downloads), median; kernel_ms: the kernels of all forms between HIP events; serial_ms: the serial "
               "restatement of Landmark::ComputeDescriptor + UpdateNormal on the host of the same machine, one run, one thread; it copies "
               "no observation map and takes no mutex, which favours it over the reference. One run on one machine.", rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
