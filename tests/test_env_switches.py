"""Every environment variable libcovgpu reads is documented in INTEGRATION.md §4, and the retired A/B switches stay gone."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RETIRED = {"COVGPU_" + n for n in (
    "RECORD_RIDE TRSM_MERGE BULK_CHUNK BULK_SPLIT EARLY_WAIT LATE_EH GATE_MERGE CU_MASK RECTR_QUARTER_MAX BWD_FRONT_TILES BWD_PIPE_MIN "
    "TRSM4 BWD_PIPE64 POTRF4_MIN STORE_BORDER BWD_TREE_TOP POTRF_LISTS PAIR_XCD SHARD_PACK MAILBOX HOST_TIMING LM_GROUP "
    "PFF PFQ PFR SIGNAL_RMW LMLIN_WAVES PAIR_WAVES").split()}


def test_env_switches_documented_and_retired_gone():
    srcs = glob.glob(os.path.join(ROOT, "covins_amd/csrc/*.hip")) + glob.glob(os.path.join(ROOT, "covins_amd/csrc/*.hpp"))
    srcs += [f for f in glob.glob(os.path.join(ROOT, "include/**"), recursive=True) if os.path.isfile(f)]
    text = "".join(open(f, encoding="utf-8").read() for f in srcs)
    read = set(re.findall(r'"(COVGPU_[A-Z0-9_]+)"', text))
    doc = open(os.path.join(ROOT, "INTEGRATION.md"), encoding="utf-8").read()
    sec = doc[doc.index("\n## 4."):doc.index("\n## 5.")]
    rows = "\n".join(line for line in sec.splitlines() if line.startswith("|"))
    documented = set(re.findall(r"`(COVGPU_[A-Z0-9_]+)", rows))
    assert read == documented, (sorted(read - documented), sorted(documented - read))
    assert not RETIRED & set(re.findall(r"COVGPU_[A-Z0-9_]+", text))
