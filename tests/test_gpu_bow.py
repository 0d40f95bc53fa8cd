"""GPU bag-of-words retrieval (k_bow.hip) against the restatement tests/bow_ref.py: every value with ==, floating
point bit for bit. Conditions that keep a comparison from being vacuous are asserted on the restatement's output, never on the GPU's."""
import numpy as np
import pytest

from covins_amd import backend, vocio
from tests import bow_ref as br
from tests import bow_util as bu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = backend.Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def check_transform(ctx, voc, row_ptr, desc, levelsup=4, ref=None):
    ref = br.transform_sets(voc, row_ptr, desc, levelsup) if ref is None else ref
    got = ctx.bow_transform_batch(voc, dict(row_ptr=row_ptr, desc=desc), levelsup=levelsup)
    assert np.array_equal(got["bow_ptr"], ref["bow_ptr"]) and got["total"] == len(ref["word"])
    assert np.array_equal(got["word"], ref["word"])
    assert np.array_equal(bits(got["value"]), bits(ref["value"]))
    assert np.array_equal(got["row_word"], ref["row_word"]) and np.array_equal(got["row_node"], ref["row_node"])
    return ref


# ---------------------------------------------------------------- transform

def test_transform_map_sets(ctx):
    sets, _ = bu.map_sets()
    ref = check_transform(ctx, bu.vocab(), sets["row_ptr"], sets["desc"], ref=bu.map_bows())
    assert (ref["row_word"] < 0).any() and len(ref["word"]) < len(ref["row_word"])     # stopped rows and repeated words occur


def test_transform_set_sizes(ctx):
    voc = bu.vocab()
    sizes = [0, 1, 63, 64, 65, 256, 257, 4096, 0]
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    desc = bu.features_near(voc, int(ptr[-1]), 11)
    ref = check_transform(ctx, voc, ptr, desc)
    assert np.diff(ref["bow_ptr"])[7] > 1500                          # the 4 096-row set fills most of its sort
    cut = ctx.bow_transform_batch(voc, dict(row_ptr=ptr, desc=desc), capacity=100)   # a capacity below the total
    assert cut["total"] == len(ref["word"]) and np.array_equal(cut["bow_ptr"], ref["bow_ptr"])
    assert np.array_equal(cut["word"], ref["word"][:100]) and np.array_equal(bits(cut["value"]), bits(ref["value"][:100]))
    none = ctx.bow_transform_batch(voc, dict(row_ptr=np.zeros(1, np.int32), desc=np.zeros((0, 32), np.uint8)))
    assert none["total"] == 0 and len(none["word"]) == 0


@pytest.mark.parametrize("levelsup", [0, 1, 2, 4, 9])
def test_transform_irregular_tree(ctx, levelsup):
    voc = bu.irregular_vocab()
    desc = np.concatenate([voc["desc"][1:], bu.features_near(voc, 300, 12, p=0.08), np.random.default_rng(3).integers(0, 256, (200, 32), dtype=np.uint8)])
    ptr = np.array([0, len(voc["desc"]) - 1, len(desc)], np.int32)
    ref = check_transform(ctx, voc, ptr, desc, levelsup)
    assert len(set(ref["row_node"].tolist())) > 1 or levelsup >= 3


@pytest.mark.parametrize("levelsup", [0, 4, 7])
def test_transform_levelsup(ctx, levelsup):
    voc = bu.vocab()
    desc = bu.features_near(voc, 500, 13)
    ref = check_transform(ctx, voc, np.array([0, 200, 500], np.int32), desc, levelsup)
    depth = {0: 4, 4: 0, 7: 0}[levelsup]                              # L = 4
    assert all(int(n) == 0 for n in ref["row_node"]) if depth == 0 else np.array_equal(voc["word_id"][ref["row_node"]] >= 0, np.ones(500, bool))


def test_transform_repeated_and_stopped_rows(ctx):
    voc = bu.vocab()
    leaf = np.flatnonzero((voc["word_id"] >= 0) & (voc["weight"] > 0))[7]
    stopped = np.flatnonzero((voc["word_id"] >= 0) & (voc["weight"] == 0))
    assert len(stopped) >= 2
    desc = np.concatenate([np.repeat(voc["desc"][leaf][None], 300, 0), voc["desc"][stopped], voc["desc"][stopped[:1]]])
    ptr = np.array([0, 300, len(desc)], np.int32)
    ref = check_transform(ctx, voc, ptr, desc)
    assert ref["bow_ptr"].tolist() == [0, 1, 1] and ref["value"][0] == 1.0 and (ref["row_word"][300:] == -1).all()
    # 300 sequential additions of one weight beside a second word: the sum is not 300 * w in general, and the norm sees both
    other = np.flatnonzero((voc["word_id"] >= 0) & (voc["weight"] > 0))[9]
    desc2 = np.concatenate([desc[:150], voc["desc"][other][None], desc[150:300]])
    ref2 = check_transform(ctx, voc, np.array([0, 301], np.int32), desc2)
    assert np.diff(ref2["bow_ptr"]).tolist() == [2]


@pytest.mark.parametrize("weighting", [vocio.TF_IDF, vocio.TF, vocio.IDF, vocio.BINARY])
def test_transform_weightings(ctx, weighting):
    voc = dict(bu.vocab(), weighting=weighting)
    rng = np.random.default_rng(14)
    desc = bu.features_near(voc, 400, 14)
    desc = desc[rng.integers(0, 120, 400)]                            # every row several times
    ref = check_transform(ctx, voc, np.array([0, 150, 400], np.int32), desc)
    assert len(ref["word"]) < 240


# ---------------------------------------------------------------- score

def test_score_pairs(ctx):
    tab = bu.map_table()
    rng = np.random.default_rng(20)
    n = len(tab)
    a, b = rng.integers(0, n, 2000), rng.integers(0, n, 2000)
    near = rng.random(2000) < 0.5                                     # half of the pairs close in time: many common words
    b[near] = np.clip(a[near] + rng.integers(-3, 4, int(near.sum())), 0, n - 1)
    # two more rows: an empty vector and nothing else
    ptr = np.concatenate([tab.bow_ptr, [tab.bow_ptr[-1]]]).astype(np.int32)
    a = np.concatenate([a, [n, 5, n, 5]]); b = np.concatenate([b, [5, n, n, 5]])
    ref = np.array([br.score((tab.word[ptr[i]:ptr[i + 1]], tab.value[ptr[i]:ptr[i + 1]]), (tab.word[ptr[j]:ptr[j + 1]], tab.value[ptr[j]:ptr[j + 1]]))
                    for i, j in zip(a, b)])
    got = ctx.bow_score_pairs(ptr, tab.word, tab.value, a, b)
    assert np.array_equal(bits(got), bits(ref))
    assert (ref[:2000] > 0.05).sum() > 200 and (ref[2000:2003] == 0).all() and abs(ref[2003] - 1) < 1e-12
    assert len(ctx.bow_score_pairs(ptr, tab.word, tab.value, [], [])) == 0


def test_score_of_two_empty_vectors_in_a_csr_without_entries(ctx):
    """The word and value arrays are empty: their device buffers are the zero-sized ones, which the kernel never reads."""
    got = ctx.bow_score_pairs(np.zeros(3, np.int32), np.zeros(0, np.int32), np.zeros(0), [0], [1])
    assert got.shape == (1,) and got[0] == 0.0


# ---------------------------------------------------------------- candidates

KEYS = ("num_candidates", "min_score", "num_sharing", "max_common_words", "num_scored")


def check_queries(ctx, tab, order, queries, opts, min_score=None, refs=None, cap=None, mode="covins"):
    """queries: [(keyframe, db_visible)]. GPU == restatement per query; returns the restatement's results."""
    order = np.asarray(order, np.int32)
    if refs is None:
        inv = br.inverted_index(tab, order)
        refs = [br.detect_candidates(tab, order, v, q, opts, None if min_score is None else float(min_score[i]), inv=inv)
                for i, (q, v) in enumerate(queries)]
    got = ctx.detect_candidates_batch(bu.table_dict(tab), order, [q for q, _ in queries], [v for _, v in queries], mode=mode,
                                      min_score=min_score, cap=cap, **opts)
    for i, r in enumerate(refs):
        n = len(r["candidates"]) if cap is None else min(cap, len(r["candidates"]))
        assert got["candidates"][i].tolist() == [int(k) for k in r["candidates"][:n]], i
        assert got["acc_score"][i].view(np.uint32).tolist() == np.array(r["acc_score"][:n], np.float32).view(np.uint32).tolist(), i
        assert int(got["num_candidates"][i]) == len(r["candidates"]), i
        assert bits(got["min_score"][i:i + 1])[0] == bits([r["min_score"]])[0], i
        for k in KEYS[2:]:
            assert int(got[k][i]) == r[k], (i, k)
    return refs


def test_candidates_on_map(ctx):
    tab = bu.map_table()
    order, refs = bu.map_queries()
    assert sum(len(r["candidates"]) > 0 for r in refs) * 3 >= len(refs)
    for k in ("moved", "dedup", "dropped"):
        assert sum(r["trace"][k] for r in refs) >= 1, k
    check_queries(ctx, tab, order, [(q, q) for q in range(len(tab))], bu.MAP_OPTS, refs=refs)


def test_candidates_on_map_covins_g_shuffled(ctx):
    """Another insertion order, the COVINS-G factor, and caller-supplied minimum scores."""
    tab = bu.map_table()
    rng = np.random.default_rng(31)
    perm = rng.permutation(len(tab)).astype(np.int32)
    opts = dict(br.default_opts("covins_g"), min_loop_dist=30)
    queries = [(int(perm[i]), i) for i in range(0, len(tab), 4)]
    refs = check_queries(ctx, tab, perm, queries, opts, mode="covins_g")
    assert sum(len(r["candidates"]) > 0 for r in refs) > 5
    check_queries(ctx, tab, perm, queries, opts, min_score=np.full(len(queries), 0.02))


def entry(i, shared, v=0.1):
    """Bow vector that shares `shared` words (value v each) with Q10 and keeps the rest of its mass on a word of its own."""
    rest = 1.0 - v * len(shared)
    if rest <= 1e-12:
        return np.asarray(shared, np.int32), np.full(len(shared), v)
    return np.asarray(list(shared) + [1000 + i], np.int32), np.asarray([v] * len(shared) + [rest])


Q10 = bu.unit(range(10))                                              # the query of the hand-built cases: words 0..9 at 0.1
OPTS = br.default_opts()


def hand(bows, queries=None, min_score=0.05, **kw):
    """Table whose keyframe 0 is the query Q10 and whose other keyframes are `bows`; database = keyframes 1.. in order."""
    tab = bu.hand_table([Q10] + list(bows), **kw)
    order = np.arange(1, len(tab), dtype=np.int32)
    queries = [(0, len(order))] if queries is None else queries
    return tab, order, queries, np.full(len(queries), min_score)


def test_filters_each_alone(ctx):
    e = entry(1, range(10))
    # the query itself is visible in the database, beside an identical keyframe
    tab = bu.hand_table([Q10, e])
    r = check_queries(ctx, tab, [0, 1], [(0, 2)], OPTS, min_score=np.array([0.05]))
    assert r[0]["candidates"] == [1] and r[0]["num_sharing"] == 1
    # inter_map_matches_only: the same-client keyframe goes, the other client's stays
    tab, order, q, ms = hand([e, e], clients=[0, 0, 1])
    r = check_queries(ctx, tab, order, q, dict(OPTS, inter_map_matches_only=1), min_score=ms)
    assert r[0]["candidates"] == [2]
    assert check_queries(ctx, tab, order, q, OPTS, min_score=ms)[0]["candidates"] == [1, 2]
    # |id difference| 99 and 100, same and other client
    tab, order, q, ms = hand([e, e, e, e], ids=[500, 401, 400, 599, 600], clients=[0, 0, 0, 1, 0])
    r = check_queries(ctx, tab, order, q, OPTS, min_score=ms)
    assert r[0]["candidates"] == [2, 3, 4]
    # ids 6 and 7 against exclude_kfs_with_id_less_than = 7
    tab, order, q, ms = hand([e, e], ids=[500, 6, 7])
    r = check_queries(ctx, tab, order, q, OPTS, min_score=ms)
    assert r[0]["candidates"] == [2]


def test_connected_keyframe_and_reference_min_score(ctx):
    """A connected keyframe that shares every word never joins the list; the minimum score comes from the valid neighbours."""
    tab = bu.hand_table([Q10, entry(1, range(10)), entry(2, range(6)), entry(3, range(3)), entry(4, range(2))],
                        neighbours=[[1, 3, 4], [], [], [], []], invalid=[0, 0, 0, 0, 1])
    r = check_queries(ctx, tab, [1, 2, 3, 4], [(0, 4)], OPTS)
    assert r[0]["min_score"] == float(np.float32(br.score(Q10, tab.bow(3)))) * 0.8     # keyframe 4 is invalid, keyframe 1 scores 1
    assert r[0]["candidates"] == [2] and r[0]["num_sharing"] == 1 and r[0]["max_common_words"] == 6
    r = check_queries(ctx, tab, [1, 2, 3, 4], [(0, 4)], br.default_opts("covins_g"), mode="covins_g")
    assert r[0]["min_score"] == float(np.float32(br.score(Q10, tab.bow(3)))) * 0.7


def test_common_word_cuts(ctx):
    """maxCommonWords 5 -> cut 4, 10 -> cut 8: only entries strictly above the cut are scored."""
    tab, order, q, ms = hand([entry(1, range(5)), entry(2, range(4)), entry(3, range(3, 8))], min_score=0.0)
    r = check_queries(ctx, tab, order, q, OPTS, min_score=ms)
    assert (r[0]["max_common_words"], r[0]["num_sharing"], r[0]["num_scored"]) == (5, 3, 2) and r[0]["candidates"] == [1, 3]
    tab, order, q, ms = hand([entry(1, range(8)), entry(2, range(10)), entry(3, range(1, 10)), entry(4, range(2, 10))], min_score=0.0)
    r = check_queries(ctx, tab, order, q, OPTS, min_score=ms)
    assert (r[0]["max_common_words"], r[0]["num_sharing"], r[0]["num_scored"]) == (10, 4, 2) and r[0]["candidates"] == [2, 3]


def test_score_equal_to_min_score_is_kept(ctx):
    bows = [entry(1, range(7), 0.07), entry(2, range(7), 0.05)]
    si = br.score(Q10, bows[0])
    assert br.score(Q10, bows[1]) < si
    tab, order, q, _ = hand(bows)
    r = check_queries(ctx, tab, order, q, OPTS, min_score=np.array([si]))
    assert r[0]["candidates"] == [1] and r[0]["num_scored"] == 2
    r = check_queries(ctx, tab, order, q, OPTS, min_score=np.array([np.nextafter(si, 1.0)]))
    assert r[0]["candidates"] == []


def test_encounter_order_beats_index_order(ctx):
    """The later-inserted keyframe shares the query's lowest word and therefore comes first."""
    tab, order, q, ms = hand([entry(1, range(2, 10)), entry(2, range(1, 9)), entry(3, range(0, 8)), entry(4, range(1, 9))])
    r = check_queries(ctx, tab, order, q, OPTS, min_score=ms)
    assert r[0]["candidates"] == [3, 2, 4, 1]
    r = check_queries(ctx, tab, [4, 3, 2, 1], q, OPTS, min_score=ms)
    assert r[0]["candidates"] == [3, 4, 2, 1]


def test_neighbour_accumulation_cases(ctx):
    # two entries whose best neighbour is the same keyframe: one candidate
    # (its own entry, unaccumulated, falls under the 0.75 threshold)
    bows = [entry(1, range(9)), entry(2, range(1, 10)), entry(3, range(10))]
    tab, order, q, ms = hand(bows, neighbours=[[], [3], [3], []])
    r = check_queries(ctx, tab, order, q, OPTS, min_score=ms)
    assert r[0]["candidates"] == [3] and r[0]["trace"] == dict(moved=2, dedup=1, dropped=1)
    # an eleventh neighbour is ignored: ten neighbours outside the database come first
    far = [entry(10 + i, [50 + i]) for i in range(10)]
    bows = [entry(1, range(9)), entry(2, range(10))] + far
    tab = bu.hand_table([Q10] + bows, neighbours=[[], list(range(3, 13)) + [2], []] + [[]] * 10)
    r = check_queries(ctx, tab, [1, 2], [(0, 2)], OPTS, min_score=np.array([0.05]))
    assert r[0]["candidates"] == [1, 2] and r[0]["trace"]["moved"] == 0
    tab = bu.hand_table([Q10] + bows, neighbours=[[], list(range(3, 12)) + [2], []] + [[]] * 10)      # as the tenth it counts
    r = check_queries(ctx, tab, [1, 2], [(0, 2)], OPTS, min_score=np.array([0.05]))
    assert r[0]["candidates"] == [2] and r[0]["trace"]["moved"] == 1
    # a neighbour beyond db_visible is ignored
    bows = [entry(1, range(9)), entry(2, range(10))]
    tab = bu.hand_table([Q10] + bows, neighbours=[[], [2], []])
    r = check_queries(ctx, tab, [1, 2], [(0, 1), (0, 2)], OPTS, min_score=np.array([0.05, 0.05]))
    assert r[0]["candidates"] == [1] and r[1]["candidates"] == [2]
    # a neighbour that fails min_score yet accumulates: many common words, small values
    bows = [entry(1, range(9)), entry(2, range(10), 0.01), entry(3, range(9))]
    tab, order, q, _ = hand(bows, neighbours=[[], [2], [], []])
    r = check_queries(ctx, tab, order, q, OPTS, min_score=np.array([0.5]))
    assert r[0]["num_scored"] == 3 and br.score(Q10, bows[1]) < 0.5
    assert r[0]["candidates"] == [1, 3] and r[0]["acc_score"][0] > r[0]["acc_score"][1] == np.float32(br.score(Q10, bows[2]))
    # the 0.75 threshold: a lone entry far below an accumulated one is dropped
    bows = [entry(1, range(10)), entry(2, range(10)), entry(3, range(9), 0.05)]
    tab, order, q, _ = hand(bows, neighbours=[[], [2], [1], []])
    r = check_queries(ctx, tab, order, q, OPTS, min_score=np.array([0.05]))
    assert r[0]["candidates"] == [1, 2] and r[0]["trace"]["dropped"] == 1


def test_many_passing_entries_and_cap(ctx):
    """1 500 identical database vectors all pass; a cap below the count reports the true count and writes the first `cap`."""
    e = entry(1, range(10))
    tab, order, q, ms = hand([e] * 1500, ids=[0] + list(range(1000, 2500)))
    r = check_queries(ctx, tab, order, q, OPTS, min_score=ms)
    assert r[0]["candidates"] == list(range(1, 1501)) and r[0]["num_scored"] == 1500
    check_queries(ctx, tab, order, q, OPTS, min_score=ms, refs=r, cap=7)
    check_queries(ctx, tab, order, q, OPTS, min_score=ms, refs=r, cap=0)
    # the same with first-encounter order against position: odd positions share word 0, even ones start at word 1
    bows = [entry(1, range(10)) if i % 2 else entry(2, range(1, 10)) for i in range(1500)]
    tab, order, q, ms = hand(bows, ids=[0] + list(range(1000, 2500)))
    r = check_queries(ctx, tab, order, q, OPTS, min_score=ms)
    assert r[0]["candidates"] == list(range(2, 1501, 2)) + list(range(1, 1501, 2))


def test_empty_cases_and_batching(ctx):
    tab = bu.map_table()
    order, refs = bu.map_queries()
    empty = bu.hand_table([(np.zeros(0, np.int32), np.zeros(0)), entry(1, range(10))])
    r = check_queries(ctx, empty, [1], [(0, 1)], OPTS, min_score=np.array([0.0]))          # a query with no words
    assert r[0]["candidates"] == [] and r[0]["num_sharing"] == 0
    r = check_queries(ctx, empty, [0, 1], [(1, 2)], OPTS, min_score=np.array([0.0]))       # an empty vector in the database
    assert r[0]["candidates"] == []
    busy = [q for q in range(len(tab)) if len(refs[q]["candidates"]) > 1][:6]
    assert len(busy) == 6
    # db_visible 0, and different db_visible within one batch
    queries = [(busy[0], 0)] + [(q, v) for q in busy for v in (q, q // 2, len(tab))]
    rr = check_queries(ctx, tab, order, queries, bu.MAP_OPTS)
    assert rr[0]["candidates"] == [] and rr[0]["num_sharing"] == 0
    assert any(rr[i]["candidates"] != rr[i + 1]["candidates"] for i in range(1, len(rr) - 1, 3))
    # a query alone equals the same query in a batch
    for q in busy[:2]:
        check_queries(ctx, tab, order, [(q, q)], bu.MAP_OPTS, refs=[refs[q]])
    got = ctx.detect_candidates_batch(bu.table_dict(tab), order, [], [])                   # zero queries
    assert len(got["num_candidates"]) == 0 and got["candidates"] == []


# ---------------------------------------------------------------- argument checks

def _bad(fn, *a, **k):
    with pytest.raises(backend.CovGpuError) as e:
        fn(*a, **k)
    msg = str(e.value)
    assert msg.startswith("covgpu error 1:") and len(msg.split(":", 2)[2].strip()) > 0, msg   # COVGPU_ERR_INVALID_ARG and a message
    return msg


def test_invalid_vocabularies(ctx):
    voc = bu.irregular_vocab()
    sets = dict(row_ptr=np.array([0, 2], np.int32), desc=np.zeros((2, 32), np.uint8))
    ctx.bow_transform_batch(voc, sets)

    def mut(**kw):
        v = {k: (np.array(x, copy=True) if isinstance(x, np.ndarray) else x) for k, x in voc.items()}
        for k, f in kw.items():
            v[k] = f(v[k]) if callable(f) else f
        return v

    def at(i, x):
        def f(a):
            a[i] = x
            return a
        return f
    leaf = int(np.flatnonzero(voc["word_id"] >= 0)[0]); inner = int(np.flatnonzero(voc["word_id"][1:] < 0)[0]) + 1
    N = len(voc["parent"])
    cases = dict(
        scoring=mut(scoring=1), weighting=mut(weighting=4), parent_after=mut(parent=at(5, 7)), parent_root=mut(parent=at(0, 0)),
        child_mismatch=mut(parent=at(N - 1, 1)), child_ptr_down=mut(child_ptr=at(3, 0)), child_range=mut(child=at(0, N)),
        leaf_without_word=mut(word_id=at(leaf, -1)), inner_with_word=mut(word_id=at(inner, 0)),
        word_twice=mut(word_id=at(leaf, int(voc["word_id"].max()))), word_range=mut(word_id=at(leaf, voc["num_words"])),
        weight_nan=mut(weight=at(leaf, np.nan)), weight_inf=mut(weight=at(leaf, np.inf)), too_many_words=mut(num_words=1 << 20),
        child_order=mut(child=lambda c: np.concatenate([c[1:2], c[0:1], c[2:]])))
    msgs = {k: _bad(ctx.bow_transform_batch, v, sets) for k, v in cases.items()}
    assert "L1_NORM" in msgs["scoring"]
    assert "rows" in _bad(ctx.bow_transform_batch, voc, dict(row_ptr=np.array([0, 4097], np.int32), desc=np.zeros((4097, 32), np.uint8)))
    _bad(ctx.bow_transform_batch, voc, dict(row_ptr=np.array([0, 2, 1], np.int32), desc=np.zeros((2, 32), np.uint8)))
    _bad(ctx.bow_transform_batch, voc, dict(row_ptr=np.array([1, 2], np.int32), desc=np.zeros((2, 32), np.uint8)))


def test_invalid_score_and_detect_arguments(ctx):
    ptr, word, val = np.array([0, 2, 4], np.int32), np.array([1, 3, 0, 3], np.int32), np.array([.5, .5, .5, .5])
    assert ctx.bow_score_pairs(ptr, word, val, [0], [1])[0] == 0.5
    _bad(ctx.bow_score_pairs, ptr, word, val, [0], [2])                                   # pair index out of range
    _bad(ctx.bow_score_pairs, ptr, word, val, [-1], [0])
    _bad(ctx.bow_score_pairs, ptr, np.array([3, 1, 0, 3], np.int32), val, [0], [1])        # unsorted words
    _bad(ctx.bow_score_pairs, ptr, np.array([1, 1, 0, 3], np.int32), val, [0], [1])        # duplicate words
    _bad(ctx.bow_score_pairs, ptr, np.array([-1, 1, 0, 3], np.int32), val, [0], [1])
    _bad(ctx.bow_score_pairs, np.array([0, 3, 2], np.int32), word, val, [0], [1])          # pointers not monotone
    _bad(ctx.bow_score_pairs, ptr, word, np.array([.5, np.nan, .5, .5]), [0], [1])

    tab = bu.hand_table([Q10, entry(1, range(10)), entry(2, range(5))], neighbours=[[1], [], []])
    t = bu.table_dict(tab)
    ok = ctx.detect_candidates_batch(t, [1, 2], [0], [2], min_score=[0.05])
    assert ok["candidates"][0].tolist() == [2]
    run = lambda tt=t, order=(1, 2), q=(0,), vis=(2,), **k: ctx.detect_candidates_batch(tt, list(order), list(q), list(vis), **k)
    assert "repeat" in _bad(run, order=(1, 1))
    _bad(run, order=(1, 3))                                                              # db_order out of range
    assert "db_visible" in _bad(run, vis=(3,))
    _bad(run, vis=(-1,))
    _bad(run, q=(3,))
    _bad(run, dict(t, nb=np.array([5], np.int32)))                                        # neighbour out of range
    _bad(run, dict(t, nb_ptr=np.array([0, 1, 0, 1], np.int32)))
    _bad(run, dict(t, bow_ptr=np.array([0, 10, 5, 17], np.int32)))
    w = t["word"].copy(); w[1] = w[0]
    _bad(run, dict(t, word=w))                                                            # duplicate word in a supplied bow row
    w = t["word"].copy(); w[[0, 1]] = w[[1, 0]]
    _bad(run, dict(t, word=w))
    v = t["value"].copy(); v[3] = np.inf
    _bad(run, dict(t, value=v))
    _bad(run, dict(t, id=np.array([-1, 5, 9], np.int32)))
    _bad(run, min_score=[np.nan])
    _bad(run, min_score_factor=float("inf"))


# ---------------------------------------------------------------- C++ facade

@pytest.fixture(scope="module")
def standin():
    """The stand-in map of the small synthetic map behind tests/cpp/facade_bow_shim.cpp."""
    from tests import facade_util
    lib = bu.bow_shim()
    saved = facade_util._LIB
    facade_util._LIB = lib
    try:
        sm = facade_util.StandinMap(bu.small_map())
    finally:
        facade_util._LIB = saved
    yield sm, lib
    lib.shim_free(sm.h)                                               # by the library that built it
    sm.h = None
    lib.bow_shutdown()


def test_facade_compute_bow_and_detect(ctx, standin):
    """KeyframeDatabaseT::ComputeBoWBatch + DetectCandidatesBatch (and the one-query form, EraseKeyframe, the consistency filter) over
    the stand-in map equal the Python route."""
    import ctypes as C
    sm, lib = standin
    m, voc = bu.small_map(), bu.vocab()
    sets, _ = bu.map_sets()
    nbs = bu.map_neighbours()
    K = m.K
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    i32 = lambda a: np.ascontiguousarray(a, np.int32)
    v = {k: (i32(x) if k != "desc" and k != "weight" else np.ascontiguousarray(x)) for k, x in voc.items() if isinstance(x, np.ndarray)}
    lib.bow_set_vocab(voc["k"], voc["L"], voc["scoring"], voc["weighting"], len(v["parent"]), voc["num_words"], ip(v["parent"]), ip(v["child_ptr"]),
                      ip(v["child"]), v["desc"].ctypes.data_as(C.POINTER(C.c_uint8)), ip(v["word_id"]), v["weight"].ctypes.data_as(C.POINTER(C.c_double)))
    for k in range(K):
        d = np.ascontiguousarray(sets["desc"][sets["row_ptr"][k]:sets["row_ptr"][k + 1]])
        nb = i32(nbs[k])
        lib.bow_set_keyframe(sm.h, k, len(d), d.ctypes.data_as(C.POINTER(C.c_uint8)), len(nb), ip(nb))
    allk = np.arange(K, dtype=np.int32)
    lib.bow_compute(sm.h, K, ip(allk), 4)
    py = ctx.bow_transform_batch(voc, sets, levelsup=4)
    for k in range(K):
        r0, r1 = int(sets["row_ptr"][k]), int(sets["row_ptr"][k + 1])
        b0, b1 = int(py["bow_ptr"][k]), int(py["bow_ptr"][k + 1])
        w = np.zeros(b1 - b0 + 1, np.int32); x = np.zeros(b1 - b0 + 1)
        assert lib.bow_get(sm.h, k, len(w), ip(w), x.ctypes.data_as(C.POINTER(C.c_double))) == b1 - b0
        assert np.array_equal(w[:-1], py["word"][b0:b1]) and np.array_equal(bits(x[:-1]), bits(py["value"][b0:b1]))
        rn = np.zeros(r1 - r0 + 1, np.int32)
        assert lib.bow_get_features(sm.h, k, r1 - r0, ip(rn)) == 1
        assert np.array_equal(rn[:-1], np.where(py["row_word"][r0:r1] >= 0, py["row_node"][r0:r1], -1))
    nptr = np.zeros(K + 1, np.int32); nptr[1:] = np.cumsum([len(x) for x in nbs])
    table = dict(id=m.kf_id, client=m.kf_client, bow_ptr=py["bow_ptr"], word=py["word"], value=py["value"], nb_ptr=nptr,
                 nb=np.concatenate([i32(x) for x in nbs]), invalid=m.kf_invalid)
    rng = np.random.default_rng(40)
    order = i32(rng.permutation(K))
    qs = i32(order[::3]); vis = i32(np.arange(K)[::3])
    for min_score in (None, np.full(len(qs), 0.03)):
        want = ctx.detect_candidates_batch(table, order, qs, vis, min_score=min_score, min_loop_dist=30)
        cnt = np.zeros(len(qs), np.int32); cand = np.full((len(qs), K), -1, np.int32); acc = np.zeros((len(qs), K), np.float32); mso = np.zeros(len(qs))
        lib.bow_detect(sm.h, 0, 30, K, ip(order), len(qs), ip(qs), ip(vis), None if min_score is None else min_score.ctypes.data_as(C.POINTER(C.c_double)),
                       K, ip(cnt), ip(cand), acc.ctypes.data_as(C.POINTER(C.c_float)), mso.ctypes.data_as(C.POINTER(C.c_double)))
        assert np.array_equal(cnt, want["num_candidates"]) and np.array_equal(bits(mso), bits(want["min_score"]))
        for i in range(len(qs)):
            assert cand[i, :cnt[i]].tolist() == want["candidates"][i].tolist()
            assert np.array_equal(acc[i, :cnt[i]].view(np.uint32), want["acc_score"][i].view(np.uint32))
    assert sum(len(c) > 0 for c in want["candidates"]) > 10
    # the one-query form after EraseKeyframe of the first candidate
    i = int(np.argmax(want["num_candidates"])); gone = int(want["candidates"][i][0])
    sub = i32(order[:vis[i]])
    one = np.zeros(K, np.int32)
    n = lib.bow_detect_one(sm.h, len(sub), ip(sub), gone, int(qs[i]), 0.03, 30, K, ip(one))
    ref = ctx.detect_candidates_batch(table, sub[sub != gone], [qs[i]], [len(sub) - 1], min_score=[0.03], min_loop_dist=30)
    assert one[:n].tolist() == ref["candidates"][0].tolist() and gone not in one[:n].tolist()
    # the consistency groups over the candidate sequence
    f = backend.ConsistencyFilter(2)
    exp = [f.feed(c, lambda k: nbs[k]) for c in want["candidates"]]
    flat = i32(np.concatenate(want["candidates"])); cnts = i32([len(c) for c in want["candidates"]])
    oc = np.zeros(len(qs), np.int32); out = np.zeros(len(flat) + 1, np.int32)
    lib.bow_consistency(sm.h, 2, len(qs), ip(cnts), ip(flat), ip(oc), ip(out))
    assert oc.tolist() == [len(e) for e in exp] and out[:oc.sum()].tolist() == [k for e in exp for k in e]
    assert oc.sum() > 0


# ---------------------------------------------------------------- chain

def _chain(ctx, pairs):
    """ComputeSE3's stages on device outputs for (query, candidate) pairs: DENSE matches -> P3P RANSAC -> SearchBySE3 -> relative pose.
    Returns per completed pair (query, candidate, pose [7], inliers)."""
    from scipy.spatial.transform import Rotation as Rot
    from tests import abspose_ref as ar
    from tests import abspose_util as au
    from tests import guided_util as gu
    m = gu.small_map()
    kfs, _ = gu.map_keyframes("ref")
    used = sorted({k for p in pairs for k in p})
    idx = {k: i for i, k in enumerate(used)}
    ptr = np.zeros(len(used) + 1, np.int32); ptr[1:] = np.cumsum([len(kfs[k]["kp"]) for k in used])
    invalid = m.lm_invalid.astype(bool)
    skip = np.concatenate([(kfs[k]["lm"] < 0) | invalid[np.maximum(kfs[k]["lm"], 0)] for k in used])
    res = ctx.match_batch(dict(row_ptr=ptr, desc=np.concatenate([kfs[k]["desc"] for k in used]), skip=skip.astype(np.uint8)),
                          [idx[q] for q, _ in pairs], [idx[c] for _, c in pairs], "dense")
    cands = []
    for j, (q, c) in enumerate(pairs):
        mt = res["match"][res["offset"][j]:res["offset"][j + 1]]
        a = np.flatnonzero(mt >= 0); b = mt[a]
        if len(a) < 25:                                                  # matches_thres
            continue
        cam = int(m.kf_cam[q]); intr, dist = m.cam_intr[cam], m.cam_dist[cam]
        cands.append(dict(q=q, c=c, a=a, b=b, bearing=au.bearings(au.undistort_radtan(kfs[q]["kp"][a].astype(np.float64), intr, dist), intr),
                          point_w=m.lm_pos[kfs[c]["lm"][b]]))
    if not cands:
        return []
    cptr = np.zeros(len(cands) + 1, np.int32); cptr[1:] = np.cumsum([len(x["a"]) for x in cands])
    cam0 = m.cam_intr[0]
    ra = ctx.abspose_ransac_batch(dict(ptr=cptr, bearing=np.concatenate([x["bearing"] for x in cands]),
                                       point_w=np.concatenate([x["point_w"] for x in cands]),
                                       sigma_angle=np.concatenate([ar.sigma_angle(np.zeros(len(x["a"])), cam0[0], cam0[1]) for x in cands]),
                                       seed=np.arange(len(cands), dtype=np.uint64) * 977 + 5))
    pose = lambda p7: np.block([[Rot.from_quat(p7[:4]).as_matrix(), p7[4:, None]], [np.zeros((1, 3)), np.ones((1, 1))]])

    def pose7(T):
        q = Rot.from_matrix(T[:3, :3]).as_quat()
        return np.concatenate([q if q[3] >= 0 else -q, T[:3, 3]])
    s_kfs, jobs, live = [], [], []
    for i, x in enumerate(cands):
        if ra["inliers"][i] <= 0:
            continue
        keep = np.flatnonzero(ra["inlier"][cptr[i]:cptr[i + 1]])
        x["ia"], x["ib"] = x["a"][keep], x["b"][keep]
        k1, k2 = dict(kfs[x["q"]]), dict(kfs[x["c"]])
        valid = lambda k: ((k["lm"] >= 0) & ~invalid[np.maximum(k["lm"], 0)])
        f1 = valid(k1); f1[x["ia"]] = False
        f2 = valid(k2); f2[x["ib"]] = False
        k1["lm_free"], k2["lm_free"] = f1.astype(np.uint8), f2.astype(np.uint8)
        x["T12"] = pose7(np.linalg.inv(pose(ra["T_wc"][i])) @ np.linalg.inv(kfs[x["c"]]["T_cw"]))
        jobs.append((len(s_kfs), len(s_kfs) + 1, x["T12"]))
        s_kfs += [k1, k2]
        live.append(x)
    if not live:
        return []
    out = gu.run_se3(ctx, dict(kfs=s_kfs, jobs=jobs, opts=dict(gu.CONFIGS["ref"])), agreement=1)
    rel = dict(ptr=[0], pA=[], pB=[], kpA=[], kpB=[], T0=[])
    for i, x in enumerate(live):
        k1, k2 = s_kfs[2 * i], s_kfs[2 * i + 1]
        o = out["match"][out["offset"][i]:out["offset"][i + 1]]
        na = np.flatnonzero(o >= 0)
        a = np.concatenate([x["ia"], na]); b = np.concatenate([x["ib"], o[na]]).astype(np.int64)
        rel["pA"].append(k1["lm_pos"][a]); rel["pB"].append(k2["lm_pos"][b])
        rel["kpA"].append(k1["kp"][a].astype(np.float64)); rel["kpB"].append(k2["kp"][b].astype(np.float64))
        rel["T0"].append(x["T12"]); rel["ptr"].append(rel["ptr"][-1] + len(a))
    n, C_ = len(live), rel["ptr"][-1]
    camv = np.concatenate([m.cam_intr[0], m.cam_dist[0]])
    rb = dict(ptr=np.array(rel["ptr"], np.int32), pA=np.concatenate(rel["pA"]), pB=np.concatenate(rel["pB"]), kpA=np.concatenate(rel["kpA"]),
              kpB=np.concatenate(rel["kpB"]), sigA=np.full(C_, 2.0), sigB=np.full(C_, 2.0), camA=np.tile(camv, (n, 1)), camB=np.tile(camv, (n, 1)),
              distA=np.full(n, int(m.cam_dist_type[0]), np.int32), distB=np.full(n, int(m.cam_dist_type[0]), np.int32), T0=np.array(rel["T0"]))
    T, _, inl = ctx.relpose_batch(rb, th_outlier=1.3, min_inliers=12)
    return [(x["q"], x["c"], T[i], int(inl[i])) for i, x in enumerate(live)]


def test_chain_from_retrieved_candidates(ctx):
    """Descriptors -> bow vectors -> loop candidates -> consistency groups -> ComputeSE3's stages, all on device outputs; the same
    chain fed by the restatement's candidates gives the same poses, and the verified candidates are true revisits. The covisibility
    graph is the one a detector sees before any loop is closed: same client, within 30 keyframes."""
    from scipy.spatial.transform import Rotation as Rot
    from tests import guided_util as gu
    m = gu.small_map()
    kfs, _ = gu.map_keyframes("ref")
    K = len(kfs)
    ptr = np.zeros(K + 1, np.int32); ptr[1:] = np.cumsum([len(k["desc"]) for k in kfs])
    tr = ctx.bow_transform_batch(bu.vocab(), dict(row_ptr=ptr, desc=np.concatenate([k["desc"] for k in kfs])))
    nbs = bu.neighbour_lists([k["lm"][k["lm"] >= 0].tolist() for k in kfs])
    nbs = [[n for n in l if m.kf_client[n] == m.kf_client[k] and abs(int(m.kf_id[n]) - int(m.kf_id[k])) < 30] for k, l in enumerate(nbs)]
    bows = [(tr["word"][tr["bow_ptr"][k]:tr["bow_ptr"][k + 1]], tr["value"][tr["bow_ptr"][k]:tr["bow_ptr"][k + 1]]) for k in range(K)]
    tab = br.Table(m.kf_id, m.kf_client, bows, nbs)
    order = np.arange(K, dtype=np.int32)
    queries = list(range(90, K))
    got = ctx.detect_candidates_batch(bu.table_dict(tab), order, queries, queries, **bu.MAP_OPTS)
    inv = br.inverted_index(tab, order)
    routes = []
    for lists in (got["candidates"], [br.detect_candidates(tab, order, q, q, bu.MAP_OPTS, inv=inv)["candidates"] for q in queries]):
        f = backend.ConsistencyFilter(3)
        routes.append([(q, int(c)) for q, cs in zip(queries, lists) for c in f.feed(cs, tab.neighbours)])
    assert routes[0] == routes[1] and len(routes[0]) >= 5
    a, b = _chain(ctx, routes[0]), _chain(ctx, routes[1])
    assert len(a) == len(b) >= 3
    for (q, c, T, inl), (q2, c2, T2, inl2) in zip(a, b):
        assert (q, c, inl) == (q2, c2, inl2) and np.array_equal(T, T2)
    ok = 0
    for q, c, T, inl in a:
        if inl <= 0:
            continue
        Tt = kfs[q]["T_cw"] @ np.linalg.inv(kfs[c]["T_cw"])
        assert np.linalg.norm(T[4:] - Tt[:3, 3]) < 0.1
        assert np.rad2deg(Rot.from_matrix(Rot.from_quat(T[:4]).as_matrix().T @ Tt[:3, :3]).magnitude()) < 1.0
        ok += 1
    assert ok >= 3


# ---------------------------------------------------------------- limits

def test_last_word_of_the_largest_vocabulary(ctx):
    """COVGPU_BOW_MAX_WORDS = 2^20 - 1 words: the last word id, 2^20 - 2, shares its high bits with no stopped-row key. A set of 301
    rows (padded to 512 in the sort) holds the last word several times among stopped rows and other words; TF_IDF sums per row."""
    W, inner = (1 << 20) - 1, 1024
    rng = np.random.default_rng(50)
    per = np.full(inner, 1024); per[0] = 1023                          # leaves per inner node: 2^20 - 1 in all
    leaf_parent = np.repeat(np.arange(1, inner + 1), per)
    desc = rng.integers(0, 256, (inner + W, 32), dtype=np.uint8)
    from tests import match_util
    desc[-1024:] = match_util.flip(np.repeat(desc[inner - 1][None], 1024, 0), 0.1, rng)   # the last node's leaves lie near it,
    desc[-1] = desc[inner - 1]                                        # and its last leaf equals it: that path has distance 0
    weight = np.concatenate([np.zeros(inner), rng.uniform(0.5, 9.0, W)])
    stopped = inner + W - 1 - rng.choice(1023, 40, replace=False) - 1  # siblings of the last leaf
    weight[stopped] = 0.0
    voc = vocio.from_nodes(1024, 2, vocio.L1_NORM, vocio.TF_IDF, np.concatenate([np.zeros(inner, np.int64), leaf_parent]),
                           np.arange(inner + W) >= inner, desc, weight)
    assert voc["num_words"] == W and voc["word_id"][-1] == W - 1 == 0xFFFFE and voc["weight"][-1] > 0
    last = desc[-1]
    rows = np.concatenate([np.repeat(last[None], 7, 0), desc[stopped[:25]], desc[rng.integers(inner, inner + W, 260)], np.repeat(last[None], 9, 0)])
    assert len(rows) == 301
    ptr = np.array([0, 301, 301 + 16], np.int32)
    rows = np.concatenate([rows, np.repeat(last[None], 16, 0)])       # and a set that is the last word alone
    ref = check_transform(ctx, voc, ptr, rows, levelsup=1)
    r0 = ref["row_word"][:301]
    assert (r0 == W - 1).sum() >= 16 and (r0 == -1).sum() >= 20 and ref["word"][ref["bow_ptr"][1] - 1] == W - 1
    assert ref["bow_ptr"][2] - ref["bow_ptr"][1] == 1 and ref["value"][-1] == 1.0
    _bad(ctx.bow_transform_batch, dict(voc, num_words=W + 1), dict(row_ptr=ptr, desc=rows))


def test_queries_in_a_later_chunk(ctx):
    """scratch_kib = 16 against 180 database entries leaves room for three queries per chunk: every query of the map, most of them in a
    later chunk, equals the restatement and the same query run alone under the default budget."""
    tab = bu.map_table()
    order, refs = bu.map_queries()
    assert (16 << 10) // (28 * len(tab)) == 3
    queries = [(q, q) for q in range(len(tab))]
    check_queries(ctx, tab, order, queries, dict(bu.MAP_OPTS, scratch_kib=16), refs=refs)
    check_queries(ctx, tab, order, queries, dict(bu.MAP_OPTS, scratch_kib=1), refs=refs)          # one query per chunk
    t = bu.table_dict(tab)
    many = ctx.detect_candidates_batch(t, order, [q for q, _ in queries], [v for _, v in queries], **dict(bu.MAP_OPTS, scratch_kib=16))
    busy = [q for q in range(len(tab)) if len(refs[q]["candidates"]) > 1][-3:]
    for q in busy:
        one = ctx.detect_candidates_batch(t, order, [q], [q], **bu.MAP_OPTS)
        assert one["candidates"][0].tolist() == many["candidates"][q].tolist() and len(one["candidates"][0]) > 1
        assert np.array_equal(one["acc_score"][0].view(np.uint32), many["acc_score"][q].view(np.uint32))
    # different db_visible and a chunk boundary inside a batch of 1 500-entry queries
    e = entry(1, range(10))
    tab2, order2, _, _ = hand([e] * 1500, ids=[0] + list(range(1000, 2500)))
    qs = [(0, v) for v in (1500, 0, 700, 1500, 3)]
    r = check_queries(ctx, tab2, order2, qs, dict(OPTS, scratch_kib=64), min_score=np.full(5, 0.05))  # 64 KiB / (28 * 1500): one per chunk
    assert [len(x["candidates"]) for x in r] == [1500, 0, 700, 1500, 3]
    _bad(ctx.detect_candidates_batch, t, order, [0], [0], scratch_kib=-1)
