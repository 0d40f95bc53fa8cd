"""Makes tests/golden/refmap_omni.npz — a saved COVINS map with OMNI (unified-projection) keyframes, run through the REFERENCE'S OWN
cereal code.

Runs in the development container only (needs the reference tree): builds oracle/_ref/cereal_roundtrip (oracle/Makefile, target `ref`),
writes the `micro_omni` synthetic map (two agents, unified + RadTan xi 0.9 and unified + Equidistant xi 1.3) with
covins_amd.mapio.save_map, lets the reference load() -> save() it, and keeps in one archive
  * every file the reference wrote, one uint8 array per file (key: relative path with "/" -> ":")
  * `decoded`: the JSON of what the reference's load() decoded from our writer's bytes (uint8 array of its UTF-8 text)
tests/test_omni_host.py (runs anywhere) reads only that archive: mapio.save_map's bytes must equal the reference's, mapio.load_map must
read them back into the map they came from, and the reference must have decoded cam_model 1 with the 5 intrinsics xi fu fv cu cv."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from covins_amd import mapio, synth  # noqa: E402


def omni_map():
    return synth.make_map(synth.config_named("micro_omni"))


if __name__ == "__main__":
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "ref"])
    tmp = tempfile.mkdtemp()
    src, dst = os.path.join(tmp, "ours"), os.path.join(tmp, "ref")
    m = omni_map()
    mapio.save_map(src, m)
    js = subprocess.check_output([os.path.join(ROOT, "oracle", "_ref", "cereal_roundtrip"), src, dst])
    files = {os.path.relpath(os.path.join(r, f), dst).replace(os.sep, ":"): np.frombuffer(open(os.path.join(r, f), "rb").read(), np.uint8)
             for r, _, fs in os.walk(dst) for f in fs}
    same = all(open(os.path.join(src, k.replace(":", os.sep)), "rb").read() == v.tobytes() for k, v in files.items())
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "refmap_omni.npz"), decoded=np.frombuffer(js, np.uint8), **files)
    print(f"K={m.K} L={m.L}: {len(files)} files, {sum(v.size for v in files.values())} bytes; reference bytes == mapio.save_map bytes: {same}")
