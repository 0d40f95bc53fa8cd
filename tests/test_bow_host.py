"""CPU checks of the bag-of-words restatement (tests/bow_ref.py), the vocabulary reader and the consistency filter."""
import numpy as np
import pytest

from covins_amd import backend, vocio
from tests import bow_ref as br
from tests import bow_util as bu


def _dict_transform(voc, feats, levelsup=4):
    """transform() recomputed with a std::map-like dict per step of the reference, independent of bow_ref's array form."""
    v = {}
    for f in feats:
        wid, w, _ = br.transform_one(voc, f, levelsup)
        if w > 0:
            if voc["weighting"] in (br.TF, br.TF_IDF):
                v[wid] = v.get(wid, 0.0) + w if wid in v else w
            else:
                v.setdefault(wid, w)
    norm = 0.0
    for k in sorted(v):
        norm += abs(v[k])
    return {k: (x / norm if norm > 0 else x) for k, x in v.items()}


def test_dict_recomputation_equals_array_form():
    voc = bu.vocab()
    sets, _ = bu.map_sets()
    b = bu.map_bows()
    for s in (0, 7, 91, 179):
        r = slice(int(sets["row_ptr"][s]), int(sets["row_ptr"][s + 1]))
        w, x, rw, rn = br.transform(voc, sets["desc"][r])
        d = _dict_transform(voc, sets["desc"][r])
        assert sorted(d) == w.tolist() and [d[k] for k in w.tolist()] == x.tolist()
        q = slice(int(b["bow_ptr"][s]), int(b["bow_ptr"][s + 1]))
        assert np.array_equal(b["word"][q], w) and np.array_equal(b["value"][q], x)
        assert np.array_equal(b["row_word"][r], rw) and np.array_equal(b["row_node"][r], rn)


def test_score_properties():
    tab = bu.map_table()
    rng = np.random.default_rng(0)
    for _ in range(50):
        a, b = (int(x) for x in rng.integers(len(tab), size=2))
        va, vb = tab.bow(a), tab.bow(b)
        assert br.score(va, vb) == br.score(vb, va) == br.score_dict(va, vb)
        assert abs(br.score(va, va) - 1.0) < 1e-12                   # a normalised non-empty vector
    x = bu.unit([1, 5, 9], [1.0, 2.0, 1.0])                          # dyadic values: the sums are exact
    assert br.score(x, x) == 1.0
    empty = (np.zeros(0, np.int32), np.zeros(0))
    assert br.score(empty, x) == 0.0 and br.score(x, empty) == 0.0 and br.score(empty, empty) == 0.0


@pytest.mark.parametrize("weighting", [vocio.TF_IDF, vocio.TF, vocio.IDF, vocio.BINARY])
def test_weightings(weighting):
    voc = dict(bu.vocab(), weighting=weighting)
    leaves = np.flatnonzero((voc["word_id"] >= 0) & (voc["weight"] > 0))[:3]
    a, b, c = voc["desc"][leaves]                                     # exactly a leaf's descriptor: distance 0 on its whole path
    stopped = voc["desc"][np.flatnonzero((voc["word_id"] >= 0) & (voc["weight"] == 0))[0]]
    w, x, rw, _ = br.transform(voc, np.stack([a, b, a, stopped, a, c]))
    wa, wb, wc = voc["weight"][leaves]
    ids = voc["word_id"][leaves]
    assert rw.tolist() == [ids[0], ids[1], ids[0], -1, ids[0], ids[2]]
    raw = {ids[0]: (wa + wa) + wa, ids[1]: wb, ids[2]: wc} if weighting in (vocio.TF_IDF, vocio.TF) else {ids[0]: wa, ids[1]: wb, ids[2]: wc}
    norm = 0.0
    for k in sorted(raw):
        norm += raw[k]
    assert w.tolist() == sorted(raw) and x.tolist() == [raw[k] / norm for k in sorted(raw)]


def test_levelsup_and_irregular_tree():
    voc = bu.irregular_vocab()
    assert np.diff(voc["child_ptr"]).max() == 20 and (np.diff(voc["child_ptr"]) == 1).any()
    feats = np.concatenate([voc["desc"][1:], bu.features_near(voc, 40, 2)])
    for levelsup in (0, 1, 2, 4, 9):
        for f in feats:
            wid, w, nid = br.transform_one(voc, f, levelsup)
            path, n = [], int(np.flatnonzero(voc["word_id"] == wid)[0])
            while n > 0:
                path.append(n); n = int(voc["parent"][n])
            path = path[::-1]                                         # nodes at depth 1, 2, ...
            level = voc["L"] - levelsup
            assert nid == (0 if level <= 0 else path[min(level, len(path)) - 1])
            assert 3 not in path                                      # the twin of node 1 never wins the tie


def test_stateful_database_equals_stateless():
    """Contract step 2: the reference's scratch fields on the keyframes (loop_query_, loop_words_, loop_score_) leave each query
    independent of the queries before it, as long as a keyframe is queried once."""
    tab = bu.map_table()
    order, ref = bu.map_queries()
    db = br.StatefulDatabase(tab)
    for q in range(len(tab)):
        got = db.DetectCandidates(q, bu.MAP_OPTS)
        assert got == ref[q], q
        db.AddKeyframe(q)
    # another insertion order, queries only now and then, and another option set
    rng = np.random.default_rng(5)
    perm = rng.permutation(len(tab)).astype(np.int32)
    opts = dict(br.default_opts("covins_g"), min_loop_dist=10, exclude_kfs_with_id_less_than=3)
    db = br.StatefulDatabase(tab)
    inv = br.inverted_index(tab, perm)
    for i, q in enumerate(perm.tolist()):
        if i % 3 == 0:
            assert db.DetectCandidates(q, opts) == br.detect_candidates(tab, perm, i, q, opts, inv=inv)
        db.AddKeyframe(q)


def test_map_queries_are_not_vacuous():
    _, ref = bu.map_queries()
    assert sum(len(r["candidates"]) > 0 for r in ref) * 3 >= len(ref)
    for k in ("moved", "dedup", "dropped"):
        assert sum(r["trace"][k] for r in ref) >= 1, k


def test_vocio_round_trip(tmp_path):
    for voc in (bu.random_vocab(k=3, L=3, seed=4), bu.irregular_vocab()):
        for blank in (False, True):
            path = tmp_path / f"voc_{blank}.txt"
            vocio.write_text(path, voc, trailing_blank_line=blank)
            if blank:
                assert path.read_text().endswith("\n\n")
            back = vocio.read_text(path)
            assert set(back) == set(voc)
            for k, v in voc.items():
                assert np.array_equal(back[k], v), k
            assert back["weight"].dtype == np.float64 and back["desc"].dtype == np.uint8
    with pytest.raises(ValueError):
        (tmp_path / "bad.txt").write_text("10 6\n")
        vocio.read_text(tmp_path / "bad.txt")


def test_consistency_filter_three_queries():
    """cov_consistency_thres 2 on a hand-written sequence: groups {10,11,12} -> {12,13} -> {13,14} chain through shared keyframes."""
    nbs = {10: [11, 12], 13: [12], 14: [13], 30: [31], 40: []}
    for F in (br.ConsistencyFilter, backend.ConsistencyFilter):
        f = F(threshold=2)
        assert f.feed([10, 30], nbs.__getitem__) == []                # first sight: two groups with counter 0
        assert [n for _, n in f.groups] == [0, 0]
        assert f.feed([13], nbs.__getitem__) == []                    # shares 12 with the first group: counter 1
        assert [n for _, n in f.groups] == [1]
        assert f.feed([14, 40], nbs.__getitem__) == [14]              # shares 13: counter 2 reaches the threshold; 40 starts anew
        assert [n for _, n in f.groups] == [2, 0]
        assert f.feed([], nbs.__getitem__) == [] and f.groups == []   # no candidates: the groups are cleared
    # both filters agree on the candidates retrieved from the map
    tab = bu.map_table()
    _, ref = bu.map_queries()
    a, b = br.ConsistencyFilter(3), backend.ConsistencyFilter(3)
    hits = 0
    for r in ref:
        ea, eb = a.feed(r["candidates"], tab.neighbours), b.feed(r["candidates"], tab.neighbours)
        assert ea == eb and [n for _, n in a.groups] == [n for _, n in b.groups]
        hits += len(ea)
    assert hits > 0


def test_library_defaults_and_argument_checks_need_no_device():
    """covgpu_default_detect_opts (config_backend.yaml:72-78); a NULL context is rejected before anything else."""
    import ctypes as C
    from covins_amd import capi
    for mode, factor in ((capi.DETECT_COVINS, 0.8), (capi.DETECT_COVINS_G, 0.7)):
        o = capi.DetectOpts()
        backend.lib().covgpu_default_detect_opts(C.byref(o), mode)
        assert (o.min_score_factor, o.min_loop_dist, o.exclude_kfs_with_id_less_than, o.inter_map_matches_only) == (factor, 100, 7, 0)
    assert br.default_opts("covins_g")["min_score_factor"] == 0.7 and br.default_opts()["min_loop_dist"] == 100
    assert backend.lib().covgpu_detect_candidates_batch(None, C.byref(capi.DetectBatch()), C.byref(capi.DetectOpts())) == 1
    assert b"NULL context" in backend.lib().covgpu_last_error()
    assert backend.lib().covgpu_bow_transform_batch(None, C.byref(capi.BowVocab()), C.byref(capi.BowTransformBatch())) == 1
    assert backend.lib().covgpu_bow_score_pairs(None, 0, None, None, None, 0, None, None, None) == 1


def test_every_batch_entry_point_rejects_a_null_context_by_name():
    """The shared prologue of batch.hip: INVALID_ARG and "<function>: NULL context", whatever the other arguments are."""
    import ctypes as C
    lib = backend.lib()
    calls = {
        "covgpu_relpose_batch": (None, C.c_double(1.3), 12),
        "covgpu_abspose_ransac_batch": (None, None),
        "covgpu_p3p_batch": (0, None, None, None, None, None),
        "covgpu_match_batch": (None, None),
        "covgpu_search_se3_batch": (None, None),
        "covgpu_search_projection_batch": (None, None),
        "covgpu_pgo_reanchor": (0, None, None, None, 0, None, None),
        "covgpu_bow_transform_batch": (None, None),
        "covgpu_bow_score_pairs": (0, None, None, None, 0, None, None, None),
        "covgpu_detect_candidates_batch": (None, None),
        # the test entry points of the trust-region tail (probe_api.hip) keep the same contract
        "covgpu_solve_resident_traced": (None, None, None, 0, None),
        "covgpu_fetch_tail_state": (None,) * 7,
        "covgpu_tail_logic_probe": (None, 0, 1, 0, 0, 0, None, None, None, 0),
    }
    for name, args in calls.items():
        assert getattr(lib, name)(None, *args) == 1, name               # COVGPU_ERR_INVALID_ARG
        msg = lib.covgpu_last_error()
        assert b"NULL context" in msg and name.encode() in msg, (name, msg)


def test_facade_bow_shim_compiles():
    """KeyframeDatabaseT instantiates on the stand-in map (tests/test_gpu_bow.py drives it)."""
    lib = bu.bow_shim()
    assert lib.bow_compute is not None and lib.bow_detect is not None and lib.bow_consistency is not None


def test_facade_database_compiles_on_covins_shaped_classes_without_traits(tmp_path):
    """The default path (bow_vec_ / feat_vec_ maps, cv::Mat-like descriptors_, non-const GetConnectedKeyframesByWeight /
    GetConnectedNeighborKeyframes / IsInvalid) instantiates: tests/cpp/facade_bow_covins_like.cpp."""
    import ctypes as C
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    so = str(tmp_path / "libfacade_bow_covins_like.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", os.path.join(root, "tests", "cpp", "facade_bow_covins_like.cpp"), "-o", so,
                           "-L" + os.path.join(root, "covins_amd"), "-lcovgpu", "-Wl,-rpath," + os.path.join(root, "covins_amd")])
    assert C.CDLL(so).bow_covins_like_instantiated() == 1
