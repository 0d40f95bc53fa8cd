#!/usr/bin/env python3
"""Writes tests/golden/record_lines_parent.npz: S, b, cost (Context.schur at mu = 1e-8 and 1e-2) and the step (Context.gn_step at mu = 1e-4) of the
points of tests/record_lines_util.py as THIS checkout's library computes them on the GPU. Run it at the commit BEFORE the whole-record transport
of k_pair_blocks / k_lm_lin (with tests/record_lines_util.py copied beside the tests of that checkout): tests/test_gpu_record_lines.py then holds
every later commit to those bytes. The file names the commit (--commit, default: git rev-parse HEAD).

  python tools/make_record_lines_golden.py [--commit SHA] [--out tests/golden/record_lines_parent.npz]
"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from covins_amd import backend
    from tests import record_lines_util as ru
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", ru.GOLDEN))
    a = ap.parse_args()
    commit = a.commit or subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True).strip()
    assert len(commit) == 40
    ctx = backend.Context(0)
    out = {"parent_commit": np.array(commit)}
    for pt in ru.POINTS:
        rec = ru.device_record(ctx, pt)
        again = ru.device_record(ctx, pt)       # (two solves of one problem are bit-identical: tests/test_gpu_schedule.py)
        assert all(rec[k].tobytes() == again[k].tobytes() for k in rec), pt.id
        out.update(rec)
        print(f"{pt.id}: {len(rec)} arrays, {sum(v.nbytes for v in rec.values())} bytes")
    ctx.close()
    np.savez(a.out, **out)
    print(f"wrote {a.out}: {os.path.getsize(a.out)} bytes, parent commit {commit}")
    assert os.path.getsize(a.out) < 1000000


if __name__ == "__main__":
    main()
