"""Vocabulary training, host side: the numpy restatement tests/voctrain_ref.py against the serial C++ restatement
tests/cpp/voctrain_serial.cpp bit for bit on every case the GPU file runs, invariants of the trained tree, the conditions the GPU cases
rely on (so that none is vacuous), and what the library decides without a device: the argument checks of covgpu_voc_train_check, the
NULL-context refusal, option defaults, limits and struct sizes. No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from covins_amd import backend, capi, vocio
from tests import bow_ref
from tests import voctrain_ref as vr
from tests import voctrain_util as vu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", vu.ALL)
def test_restatement_equals_the_serial_form(name):
    c = vu.cases()[name]
    voc, info = vu.ref(name)
    svoc, sstats, srw = vu.serial(c["row_ptr"], c["desc"], c["k"], c["L"], c["weighting"], c["seed"], c["opts"].get("max_iterations", 100))
    vr.assert_same(voc, svoc, name)
    assert info["stats"].tolist() == sstats.tolist(), name
    assert np.array_equal(info["row_word"], srw), name


def _depth(voc):
    d = np.zeros(len(voc["parent"]), np.int64)
    for n in range(1, len(d)):
        d[n] = d[voc["parent"][n]] + 1
    return d


@pytest.mark.parametrize("name", vu.ALL)
def test_invariants_of_the_result(name, tmp_path):
    c = vu.cases()[name]
    voc, info = vu.ref(name)
    N = len(voc["parent"])
    assert (voc["parent"][1:] < np.arange(1, N)).all() and (voc["parent"][1:] >= 0).all()       # parent before child
    nchild = np.diff(voc["child_ptr"])
    assert nchild.max() <= c["k"]
    depth = _depth(voc)
    assert depth.max() <= c["L"] and (nchild[depth == c["L"]] == 0).all()                        # a node at depth L is a leaf
    assert info["stats"][5] == depth.max()
    # node ids: a node's children are consecutive, and child 0's subtree comes before child 1's
    for n in range(N):
        kids = voc["child"][voc["child_ptr"][n]:voc["child_ptr"][n + 1]]
        assert np.array_equal(kids, np.arange(kids[0], kids[0] + len(kids))) if len(kids) else True
    # every centre of a node that converged is the meanValue of its group
    for rec in info["nodes"]:
        if not (rec["kmeans"] and rec["converged"]):
            continue
        for ch in voc["child"][voc["child_ptr"][rec["node"]]:voc["child_ptr"][rec["node"] + 1]]:
            g = info["train_rows"][int(ch)]
            if len(g):
                assert np.array_equal(voc["desc"][ch], vr.mean_value(c["desc"][g])[0]), (name, ch)
    # the text format round trip
    path = str(tmp_path / "voc.txt")
    vocio.write_text(path, voc)
    vr.assert_same(vocio.read_text(path), voc, name)
    # bow_ref's transform of the training rows (weights of 1, so that no word is stopped)
    ones = dict(voc, weight=np.where(voc["word_id"] >= 0, 1.0, 0.0))
    t = bow_ref.transform_sets(ones, c["row_ptr"], c["desc"], 4)
    assert np.array_equal(t["row_word"], info["row_word"]), name
    # IDF weights: a word no set reaches keeps 0; NDocs counts the empty sets
    if c["weighting"] in (vocio.TF_IDF, vocio.IDF):
        S = len(c["row_ptr"]) - 1
        leaves = np.flatnonzero(voc["word_id"] >= 0)
        assert (voc["weight"][leaves] >= 0).all() and (voc["weight"][leaves] <= np.log(S) + 1e-12).all()
    else:
        assert set(voc["weight"][voc["word_id"] >= 0].tolist()) == {1.0}


def test_cases_do_what_they_are_for():
    st = lambda name: vu.ref(name)[1]["stats"]
    assert st("emptied")[3] >= 1
    for name, cap in (("capped_1", 1), ("capped_2", 2)):
        nodes = vu.ref(name)[1]["nodes"]
        assert st(name)[2] == sum(r["capped"] for r in nodes) >= 1 and st(name)[1] == cap
        assert sum(not r["capped"] for r in nodes) >= 1                                          # a node below the cap
    assert sum(r["kmeans"] and r["converged"] for r in vu.ref("capped_2")[1]["nodes"]) >= 1      # one that k-means itself finished in time
    assert st("two_values")[4] >= 1 and st("all_identical")[4] >= 1                              # fewer than k centres
    t = vu.ref("ties")[1]
    assert t["ties"] >= 1 and t["half_bits"] >= 1
    d = vu.ref("duplicates")[1]
    assert (d["row_word"] != d["train_leaf"]).sum() >= 1 and (d["train_leaf"] >= 0).all()
    # all rows identical: a chain of one-child nodes down to L
    v = vu.ref("all_identical")[0]
    assert len(v["parent"]) == 1 + vu.cases()["all_identical"]["L"] and v["num_words"] == 1
    assert vu.ref("complementary")[0]["num_words"] >= 2
    for name, n in (("root_n_below_k", 3), ("root_n_equals_k", 5)):
        assert len(vu.ref(name)[0]["parent"]) == 1 + n and st(name)[0] == 0
    assert st("root_n_above_k")[0] >= 2
    assert vu.ref("L_6")[0]["L"] == 6 and st("L_6")[5] >= 4 and len(set(_depth(vu.ref("L_6")[0])[vu.ref("L_6")[0]["word_id"] >= 0])) >= 2
    # the size sweep crosses the forms: a node of one wavefront, of one workgroup, of several
    assert vu.cases()["three_tiles"]["desc"].shape[0] > 2 * vu.TILE


def test_draws_are_counter_based():
    assert vr.splitmix64(0) == 0xE220A8397B1DCDAF
    assert vr.child_key(5, 2) == vr.splitmix64(8) and 0.0 <= vr.unit(9, 3) < 1.0
    a = vr.train([0, 50], vu.clustered(50, 1), 3, 2, seed=4)[0]
    b = vr.train([0, 50], vu.clustered(50, 1), 3, 2, seed=5)[0]
    assert not np.array_equal(a["desc"], b["desc"]) or len(a["desc"]) != len(b["desc"])


def test_struct_sizes_limits_and_defaults_match_the_header(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "covgpu.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %d %d %d %d\\n", '
                   "sizeof(covgpu_voc_train_t), sizeof(covgpu_voc_train_opts), offsetof(covgpu_voc_train_t, stats), "
                   "offsetof(covgpu_voc_train_opts, seed), offsetof(covgpu_voc_train_opts, scratch_kib), COVGPU_VOCTRAIN_WAVE_MAX, "
                   "COVGPU_VOCTRAIN_TILE, COVGPU_VOCTRAIN_MAX_K, COVGPU_VOCTRAIN_THREADS); return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[:5] == [C.sizeof(capi.VocTrain), C.sizeof(capi.VocTrainOpts), capi.VocTrain.stats.offset, capi.VocTrainOpts.seed.offset,
                       capi.VocTrainOpts.scratch_kib.offset]
    lim = (C.c_int32 * 4)()
    backend.lib().covgpu_voc_train_limits(lim)
    assert tuple(got[5:]) == tuple(lim) == (vu.WAVE_MAX, vu.TILE, vu.MAX_K, vu.THREADS)
    o = capi.VocTrainOpts()
    backend.lib().covgpu_default_voc_train_opts(C.byref(o))
    assert (o.k, o.L, o.weighting, o.scoring, o.seed, o.max_iterations, o.scratch_kib) == (10, 5, capi.BOW_TF_IDF, capi.BOW_L1_NORM, 0, 100, 65536)
    assert len(capi.VOCTRAIN_STATS) == 8


def test_null_context_is_refused():
    c = vu.cases()["root_n_above_k"]
    s, o, out, keep = backend.Context._voc_train_batch(c["row_ptr"], c["desc"], c["k"], c["L"], c["weighting"], c["seed"], {})
    assert backend.lib().covgpu_voc_train(None, C.byref(s), C.byref(o)) == 1
    assert backend.lib().covgpu_last_error() == b"covgpu_voc_train: NULL context"
    assert out["num_nodes"][0] == 0 and (out["parent"] == -2).all()


def _check(c, drop=(), k=None, L=None, weighting=None, node_capacity=None, row_ptr=None, desc=None, **opts):
    s, o, out, keep = backend.Context._voc_train_batch(c["row_ptr"] if row_ptr is None else row_ptr, c["desc"] if desc is None else desc,
                                                       c["k"] if k is None else k, c["L"] if L is None else L,
                                                       c["weighting"] if weighting is None else weighting, c["seed"], opts, node_capacity)
    for f in drop:
        setattr(s, f, None)
    rc = backend.lib().covgpu_voc_train_check(C.byref(s), C.byref(o))
    return rc, backend.lib().covgpu_last_error().decode()


def test_invalid_arguments_are_rejected_without_a_device():
    good = vu.cases()["rows_257"]
    assert _check(good)[0] == 0
    assert _check(good, drop=("row_word", "stats"))[0] == 0                                       # the optional outputs
    assert _check(good, node_capacity=0, drop=("parent", "desc_out", "word_id", "weight"))[0] == 0   # a call that only asks for the count

    def bad(msg, **kw):
        rc, err = _check(good, **kw)
        assert rc == 1 and err.startswith("covgpu_voc_train_check: ") and msg in err, (msg, rc, err)

    assert backend.lib().covgpu_voc_train_check(None, None) == 1
    for f in ("row_ptr", "desc", "num_nodes", "num_words", "parent", "desc_out", "word_id", "weight"):
        bad("NULL", drop=(f,))
    # D4
    bad("no descriptor rows", row_ptr=[0, 0, 0], desc=np.zeros((0, 32), np.uint8))
    bad("no descriptor rows", row_ptr=[0], desc=np.zeros((0, 32), np.uint8))
    for k in (1, 0, -3):
        bad("k < 2", k=k)
    bad("COVGPU_VOCTRAIN_MAX_K", k=vu.MAX_K + 1)
    for L in (0, -1):
        bad("L < 1", L=L)
    bad("k^L", k=10, L=7)
    bad("k^L", k=2, L=20)
    assert _check(good, k=2, L=19)[0] == 0 and _check(good, k=10, L=6)[0] == 0 and _check(good, k=vu.MAX_K, L=3)[0] == 0
    ptr = good["row_ptr"].copy(); ptr[1], ptr[2] = ptr[2], ptr[1]
    bad("not monotone", row_ptr=ptr)
    ptr = good["row_ptr"].copy(); ptr[0] = 1
    bad("row_ptr[0]", row_ptr=ptr)
    for w in (-1, 4):
        bad("unknown weighting", weighting=w)
    bad("L1_NORM", scoring=1)
    bad("max_iterations", max_iterations=0)
    bad("scratch_kib", scratch_kib=0)
    bad("scratch_kib", k=10, L=6, scratch_kib=122)                                               # 10^6 bits need 123 KiB
    assert _check(good, k=10, L=6, scratch_kib=123)[0] == 0
    bad("node_capacity", node_capacity=-1)
    # a row count at which a tile's position loop would step past 2^31 (the check reads row_ptr only)
    s, o, out, keep = backend.Context._voc_train_batch(good["row_ptr"], good["desc"], good["k"], good["L"], good["weighting"], 0, {})
    for rows, rc in ((2 ** 31 - 1 - vu.TILE, 0), (2 ** 31 - vu.TILE, 1)):
        ptr = np.array([0, rows], np.int32)
        s.num_sets, s.row_ptr = 1, capi.iptr(ptr)
        assert backend.lib().covgpu_voc_train_check(C.byref(s), C.byref(o)) == rc, rows


def test_the_facade_shim_compiles():
    """CreateVocabulary instantiates on the stand-in types (tests/cpp/facade_voctrain_shim.cpp)."""
    assert hasattr(vu.shim(), "voctrain_create")
