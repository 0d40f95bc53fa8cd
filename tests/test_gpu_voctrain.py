"""covgpu_voc_train on the GPU against tests/voctrain_ref.train: every node's parent, centre, word id and weight, the
transform leaf of every training row and the six counters, all with ==. Training is integer work; the weights are one host-side
log(NDocs / Ni) of integers, so there is no tolerance anywhere. tests/test_voctrain_host.py asserts on the CPU that each named case
meets the condition it is named for."""
import ctypes as C

import numpy as np
import pytest

from covins_amd import backend, capi, vocio
from tests import bow_ref
from tests import bow_util as bu
from tests import bowdb_ref as dr
from tests import voctrain_ref as vr
from tests import voctrain_util as vu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = backend.Context(0)
    yield c
    c.close()


def same(got, name, ref=None):
    """(voc, stats) of the device == the restatement of the named case."""
    voc, stats = got
    rvoc, info = vu.ref(name) if ref is None else ref
    vr.assert_same(voc, rvoc, name)
    assert [stats[k] for k in capi.VOCTRAIN_STATS[:6]] == info["stats"].tolist(), (name, stats, info["stats"])
    assert np.array_equal(stats["row_word"], info["row_word"]), name
    assert stats["h2d_bytes"] > 32 * len(info["row_word"]) and stats["d2h_bytes"] > 0


@pytest.mark.parametrize("name", vu.HAND)
def test_hand_built_inputs(ctx, name):
    """n < k, n = k, n = k + 1 and a single row at the root; all rows identical (a chain of one-child nodes down to L); two values
    repeated; a complementary pair; duplicates that become separate clusters; tied distances and exact-half bit counts; a cluster
    that loses all its members."""
    same(vu.run_gpu(ctx, vu.cases()[name]), name)


@pytest.mark.parametrize("name", vu.CAPPED)
def test_iteration_cap(ctx, name):
    got = vu.run_gpu(ctx, vu.cases()[name])
    same(got, name)
    assert got[1]["nodes_at_cap"] >= 1 and got[1]["max_node_iterations"] == vu.cases()[name]["opts"]["max_iterations"]


def test_limits_are_the_ones_the_sweep_was_built_for():
    lim = (C.c_int32 * 4)()
    backend.lib().covgpu_voc_train_limits(lim)
    assert tuple(lim) == (vu.WAVE_MAX, vu.TILE, vu.MAX_K, vu.THREADS)
    rows = {vu.cases()[n]["desc"].shape[0] for n in vu.SWEEP}
    assert {lim[0] - 1, lim[0], lim[0] + 1, lim[1] - 1, lim[1], lim[1] + 1} <= rows and max(rows) > 2 * lim[1]
    assert {vu.cases()[n]["k"] for n in vu.SWEEP} >= {2, 3, 10, lim[2]} and {vu.cases()[n]["L"] for n in vu.SWEEP} >= {1, 2, 3, 6}


@pytest.mark.parametrize("name", vu.SWEEP)
def test_size_sweep(ctx, name):
    """Root segments of one less, exactly and one more than each size at which the kernel form changes (one wavefront per node, one
    workgroup, several workgroups), a node over three tiles, k = 2, 3, 10 and the largest, L = 1, 2, 3 and 6 (irregular trees)."""
    same(vu.run_gpu(ctx, vu.cases()[name]), name)


@pytest.mark.parametrize("name", vu.DOCS)
def test_documents_and_weightings(ctx, name):
    same(vu.run_gpu(ctx, vu.cases()[name]), name)


def test_determinism_and_smallest_scratch(ctx):
    for name in ("many_sets", "three_tiles"):
        c = vu.cases()[name]
        a, b = vu.run_gpu(ctx, c), vu.run_gpu(ctx, c)
        small = -(-c["k"] ** c["L"] // 8192)
        s = vu.run_gpu(ctx, c, scratch_kib=small)
        for got in (a, b, s):
            same(got, name)
        assert a[1]["h2d_bytes"] == b[1]["h2d_bytes"] == s[1]["h2d_bytes"] and a[1]["d2h_bytes"] == b[1]["d2h_bytes"]
        with pytest.raises(backend.CovGpuError, match="scratch_kib"):
            vu.run_gpu(ctx, c, scratch_kib=small - 1)


def test_node_capacity_too_small_reports_the_count(ctx):
    c = vu.cases()["L_3"]
    N = len(vu.ref("L_3")[0]["parent"])
    s, o, out, keep = backend.Context._voc_train_batch(c["row_ptr"], c["desc"], c["k"], c["L"], c["weighting"], c["seed"], {}, N - 1, True)
    assert backend.lib().covgpu_voc_train(ctx._h, C.byref(s), C.byref(o)) == 1
    assert b"node_capacity too small" in backend.lib().covgpu_last_error()
    assert out["num_nodes"][0] == N and out["num_words"][0] == 0
    assert (out["parent"] == -2).all() and (out["word_id"] == -2).all() and (out["weight"] == -1.0).all() and not out["desc"].any()
    assert (out["row_word"] == -2).all() and not out["stats"].any()
    s, o, out, keep = backend.Context._voc_train_batch(c["row_ptr"], c["desc"], c["k"], c["L"], c["weighting"], c["seed"], {}, N, True)
    assert backend.lib().covgpu_voc_train(ctx._h, C.byref(s), C.byref(o)) == 0
    rvoc = vu.ref("L_3")[0]
    assert out["num_nodes"][0] == N and np.array_equal(out["parent"], rvoc["parent"]) and np.array_equal(out["desc"], rvoc["desc"])
    # the Python call finds the count by itself when its guess is too small
    same(ctx.train_vocabulary(c["row_ptr"], c["desc"], c["k"], c["L"], seed=c["seed"], row_word=True), "L_3")
    with pytest.raises(backend.CovGpuError, match="node_capacity too small"):
        ctx.train_vocabulary(c["row_ptr"], c["desc"], c["k"], c["L"], seed=c["seed"], node_capacity=5)


@pytest.mark.parametrize("name", ["L_3", "empty_sets", "capped_2", "duplicates"])
def test_facade(ctx, name):
    """CreateVocabulary of the C++ facade (tests/cpp/facade_voctrain_shim.cpp) == the Python call, child lists included."""
    voc, stats = vu.run_shim(vu.cases()[name])
    got = vu.run_gpu(ctx, vu.cases()[name])
    vr.assert_same(voc, got[0], name)
    vr.assert_same(voc, vu.ref(name)[0], name)
    assert stats[:6].tolist() == [got[1][k] for k in capi.VOCTRAIN_STATS[:6]]


def _equal_queries(got, refs):
    bits = lambda a: np.asarray(a, np.float64).view(np.uint64)
    for i, r in enumerate(refs):
        assert got["candidates"][i].tolist() == [int(k) for k in r["candidates"]], i
        assert got["acc_score"][i].view(np.uint32).tolist() == np.array(r["acc_score"], np.float32).view(np.uint32).tolist(), i
        assert bits(got["min_score"][i:i + 1])[0] == bits([r["min_score"]])[0], i
        for k in ("num_sharing", "max_common_words", "num_scored"):
            assert int(got[k][i]) == r[k], (i, k)


def test_chain_to_the_resident_database(ctx):
    """A vocabulary trained on the small map's descriptor sets (k = 8, L = 3) feeds Context.bowdb: put_descriptors and query over the
    map equal the restatements under that vocabulary; the text file written from it reads back equal."""
    sets, _ = bu.map_sets()
    ref = vr.train(sets["row_ptr"], sets["desc"], 8, 3, seed=11)
    voc, stats = ctx.train_vocabulary(sets["row_ptr"], sets["desc"], 8, 3, seed=11, row_word=True)
    same((voc, stats), "small map", ref)
    m, nbs = bu.small_map(), bu.map_neighbours()
    K = m.K
    bows = bow_ref.transform_sets(voc, sets["row_ptr"], sets["desc"], 4)
    assert (bows["row_word"] >= 0).sum() > 0.5 * len(bows["row_word"])
    inv = np.zeros(K, np.uint8); inv[::17] = 1
    db = ctx.bowdb(voc, **bu.MAP_OPTS)
    rdb = dr.Database(bu.MAP_OPTS)
    got = db.put_descriptors(np.arange(K), m.kf_id, m.kf_client, sets, want=True)
    for k in ("bow_ptr", "word", "row_word", "row_node"):
        assert np.array_equal(got[k], bows[k]), k
    assert np.array_equal(got["value"].view(np.uint64), bows["value"].view(np.uint64))
    for q in range(K):
        b0, b1 = bows["bow_ptr"][q], bows["bow_ptr"][q + 1]
        rdb.put(q, m.kf_id[q], m.kf_client[q], (bows["word"][b0:b1], bows["value"][b0:b1]))
        rdb.set_neighbours(q, nbs[q]); rdb.set_invalid(q, inv[q]); rdb.add(q)
    db.set_neighbours(np.arange(K), nbs); db.set_invalid(np.arange(K), inv); db.add(np.arange(K))
    qs = list(range(3, K, 8))
    refs = [rdb.query(q, nbs[q]) for q in qs]
    assert sum(len(r["candidates"]) > 0 for r in refs) >= 3
    _equal_queries(db.query(qs, [nbs[q] for q in qs]), refs)
    db.close()
