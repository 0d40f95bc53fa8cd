"""The resident keyframe database on the GPU (covgpu_bowdb, k_bowdb.hip) against the restatement tests/bowdb_ref.py and
against the stateless call: every value with ==, floating point bit for bit. Conditions that keep a comparison from being vacuous are
asserted on the restatement's output, never on the GPU's."""
import numpy as np
import pytest

from covins_amd import backend, vocio
from tests import bow_ref as br
from tests import bow_util as bu
from tests import bowdb_ref as dr

pytestmark = pytest.mark.gpu

KEYS = ("num_sharing", "max_common_words", "num_scored")
OPTS = br.default_opts()


@pytest.fixture(scope="module")
def ctx():
    c = backend.Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def equal(got, refs, cap=None):
    """The result of BowDb.query / Context.detect_candidates_batch == the restatement's results, query by query."""
    assert len(got["num_candidates"]) == len(refs)
    for i, r in enumerate(refs):
        n = len(r["candidates"]) if cap is None else min(cap, len(r["candidates"]))
        assert got["candidates"][i].tolist() == [int(k) for k in r["candidates"][:n]], i
        assert got["acc_score"][i].view(np.uint32).tolist() == np.array(r["acc_score"][:n], np.float32).view(np.uint32).tolist(), i
        assert int(got["num_candidates"][i]) == len(r["candidates"]), i
        assert bits(got["min_score"][i:i + 1])[0] == bits([r["min_score"]])[0], i
        for k in KEYS:
            assert int(got[k][i]) == r[k], (i, k)


def same_output(a, b):
    """Two device results agree in every value."""
    assert [c.tolist() for c in a["candidates"]] == [c.tolist() for c in b["candidates"]]
    assert [c.view(np.uint32).tolist() for c in a["acc_score"]] == [c.view(np.uint32).tolist() for c in b["acc_score"]]
    assert np.array_equal(bits(a["min_score"]), bits(b["min_score"]))
    for k in KEYS + ("num_candidates",):
        assert np.array_equal(a[k], b[k]), k


class Both:
    """A handle and the restatement's database, driven together."""

    def __init__(self, ctx, opts=OPTS, voc=None, **kw):
        self.db = ctx.bowdb(voc, **opts, **kw)
        self.ref = dr.Database(opts)

    def put(self, slot, id, client, bow):
        self.db.put([slot], [id], [client], [0, len(bow[0])], bow[0], bow[1])
        self.ref.put(slot, id, client, bow)

    def put_all(self, bows, first=0, ids=None, clients=None):
        """bows go to the slots first, first + 1, ...; ids default to 1000 + 200 * slot, clients to 0."""
        for i, b in enumerate(bows):
            s = first + i
            self.put(s, 1000 + 200 * s if ids is None else ids[i], 0 if clients is None else clients[i], b)

    def neighbours(self, slot, nb):
        self.db.set_neighbours([slot], [nb]); self.ref.set_neighbours(slot, nb)

    def add(self, slots):
        self.db.add(slots)
        for s in slots:
            self.ref.add(s)

    def erase(self, slots):
        self.db.erase(slots)
        for s in slots:
            self.ref.erase(s)

    def query(self, slots, cons=None, min_score=0.05, cap=None):
        """Handle == restatement; returns (device result, restatement's results). min_score: one value for all, or None."""
        cons = [[] for _ in slots] if cons is None else cons
        refs = [self.ref.query(s, c, min_score) for s, c in zip(slots, cons)]
        got = self.db.query(slots, cons, min_score=None if min_score is None else np.full(len(slots), min_score), cap=cap)
        equal(got, refs, cap)
        return got, refs

    def close(self):
        self.db.close()


def entry(i, shared, v=0.1):
    """Bow vector that shares `shared` words (value v each) with Q10 and keeps the rest of its mass on a word of its own."""
    rest = 1.0 - v * len(shared)
    return np.asarray(list(shared) + [1000 + i], np.int32), np.asarray([v] * len(shared) + [rest])


Q10 = bu.unit(range(10))                                              # the query of the hand-built cases: words 0..9 at 0.1
QUERY = 5000                                                          # its slot; id 10 of client 1: no id filter touches an entry


def with_query(ctx, bows, **kw):
    b = Both(ctx, **kw)
    b.put(QUERY, 10, 1, Q10)
    b.put_all(bows)
    return b


# ---------------------------------------------------------------- the small-map replay

def _replay(ctx, prestore, **kw):
    """bowdb_ref.replay() through a handle. prestore: every vector is stored first and the reference minimum score is computed on the
    device; otherwise each keyframe's set is transformed at its arrival and the minimum score, which reads neighbours that arrive
    later, is given."""
    refs, live, erased = dr.replay()
    assert erased == 45 and sum(len(r["candidates"]) > 0 for r in refs) >= 100
    tab, nbs, (sets, _), bows = bu.map_table(), bu.map_neighbours(), bu.map_sets(), bu.map_bows()
    K = len(tab)
    db = ctx.bowdb(bu.vocab(), **bu.MAP_OPTS, **kw)
    one = lambda q: dict(row_ptr=sets["row_ptr"][q:q + 2] - sets["row_ptr"][q], desc=sets["desc"][sets["row_ptr"][q]:sets["row_ptr"][q + 1]])
    if prestore:
        got = db.put_descriptors(np.arange(K), tab.id, tab.client, sets, want=True)
        for k in ("bow_ptr", "word", "row_word", "row_node"):
            assert np.array_equal(got[k], bows[k]), k
        assert np.array_equal(bits(got["value"]), bits(bows["value"]))
        db.set_invalid(np.arange(K), tab.invalid)                        # the minimum score skips invalid neighbours, later ones too
    live_now = []
    for q in range(K):
        if not prestore:
            got = db.put_descriptors([q], [tab.id[q]], [tab.client[q]], one(q), want=True)
            b0, b1, r0, r1 = bows["bow_ptr"][q], bows["bow_ptr"][q + 1], sets["row_ptr"][q], sets["row_ptr"][q + 1]
            assert got["bow_ptr"].tolist() == [0, b1 - b0] and np.array_equal(got["word"], bows["word"][b0:b1])
            assert np.array_equal(bits(got["value"]), bits(bows["value"][b0:b1]))
            assert np.array_equal(got["row_word"], bows["row_word"][r0:r1]) and np.array_equal(got["row_node"], bows["row_node"][r0:r1])
        db.set_neighbours([q], [nbs[q]]); db.set_invalid([q], [tab.invalid[q]])
        equal(db.query([q], [nbs[q]], min_score=None if prestore else [refs[q]["min_score"]]), [refs[q]])
        db.add([q]); live_now.append(q)
        for e in dr.erase_after(q, live_now):
            db.erase([e]); live_now.remove(e)
    assert db.order().tolist() == live
    st = db.stats()
    db.close()
    return st


@pytest.mark.parametrize("tail_limit, rebuilds", [(0, 180), (7, 22), (1000, 0)])
def test_replay_with_erasures(ctx, tail_limit, rebuilds):
    st = _replay(ctx, False, tail_limit=tail_limit)
    assert (st["stored"], st["live"], st["rebuilds"]) == (180, 135, rebuilds)


def test_replay_from_the_smallest_buffers(ctx):
    """reserve_kf = reserve_words = 1: slots, positions, pool and index all grow by doubling many times, device to device."""
    st = _replay(ctx, False, tail_limit=7, reserve_kf=1, reserve_words=1)
    # the positions alone, added one at a time: 1 -> 256 is eight doublings of their two buffers
    assert st["slot_capacity"] >= 180 and st["position_capacity"] >= 135 and st["growths"] >= 16


def test_replay_with_the_minimum_score_computed(ctx):
    _replay(ctx, True, tail_limit=7)


# ---------------------------------------------------------------- tail and base together

def _mixed(i):
    """Entry i of the tail / base cases. Every sharing entry shares exactly one word of Q10, so maxCommonWords is 1 and each is scored."""
    kind = i % 5
    if kind == 1:
        return np.zeros(0, np.int32), np.zeros(0)                       # an empty vector
    if kind == 2:
        return bu.unit([2000 + i])                                      # one word, not the query's
    return bu.unit([{0: 9, 3: 0, 4: 5}[kind], 2000 + i])                # only the query's last word / first word / a middle one


@pytest.mark.parametrize("base", [0, 1, 100])
def test_tail_and_base_together(ctx, base):
    for tail in (0, 1, 63, 64, 65, 257):
        n = base + tail
        b = with_query(ctx, [_mixed(i) for i in range(n)], tail_limit=1000)
        b.put(QUERY + 1, 11, 1, (np.zeros(0, np.int32), np.zeros(0)))   # a query with an empty vector
        b.put(QUERY + 2, 12, 1, bu.unit([700, 701]))                    # a query none of whose words is in the database
        b.put(QUERY + 3, 13, 1, bu.unit(range(5, 15)))                  # shares 5 and 9: other first-word indices
        b.add(list(range(base)))
        b.db.compact()
        b.add(list(range(base, n)))
        st = b.db.stats()
        assert (st["positions"], st["tail"], st["live"]) == (n, tail, n)
        _, refs = b.query([QUERY, QUERY + 1, QUERY + 2, QUERY + 3], min_score=0.0)
        want = [i for k in (3, 4, 0) for i in range(n) if i % 5 == k]   # by first shared word (0, 5, 9), then by position
        assert refs[0]["candidates"] == want and refs[1]["candidates"] == [] and refs[2]["candidates"] == []
        assert refs[3]["candidates"] == [i for k in (4, 0) for i in range(n) if i % 5 == k]
        assert refs[0]["max_common_words"] == (1 if n > 0 else 0)
        b.close()


def test_the_same_entries_in_the_base_and_in_the_tail(ctx):
    bows = [entry(i, range(i % 3, 10 - i % 2)) for i in range(65)] + [_mixed(i) for i in range(20)]
    out = []
    for compact in (True, False):
        b = with_query(ctx, bows, tail_limit=1000)
        for i in range(65):                                             # 9-word entries whose neighbour shares all 10, and the reverse
            b.neighbours(i, [(i + 3) % 65, 70])
        b.add(list(range(len(bows))))
        if compact:
            b.db.compact()
        assert b.db.stats()["tail"] == (0 if compact else len(bows))
        got, refs = b.query([QUERY])
        assert len(refs[0]["candidates"]) >= 10 and refs[0]["num_scored"] > 20 and all(refs[0]["trace"][k] > 0 for k in ("moved", "dedup", "dropped"))
        out.append(got)
        b.close()
    same_output(out[0], out[1])


# ---------------------------------------------------------------- erase

def test_erase(ctx):
    # the best candidate goes; erased again and a slot that was never live: no-ops
    b = with_query(ctx, [entry(1, range(2, 10)), entry(2, range(1, 9)), entry(3, range(0, 8)), entry(4, range(1, 9))], tail_limit=2)
    b.add([0, 1, 2, 3])
    _, r = b.query([QUERY])
    assert r[0]["candidates"] == [2, 1, 3, 0]
    b.erase([2])
    _, r = b.query([QUERY])
    assert r[0]["candidates"] == [1, 3, 0]
    before = b.db.stats()
    b.erase([2]); b.erase([77]); b.erase([QUERY])
    after = b.db.stats()
    assert {k: after[k] for k in ("live", "positions", "tail", "pool_used", "pool_dead")} == {k: before[k] for k in ("live", "positions", "tail", "pool_used", "pool_dead")}
    b.query([QUERY])
    # a new vector on the erased slot, added again: it now sits at the end of the order, behind slot 3 with the same first word
    b.put(2, 1400, 0, entry(9, range(1, 9)))
    b.add([2])
    _, r = b.query([QUERY])
    assert r[0]["candidates"] == [1, 3, 2, 0] and b.db.order().tolist() == [0, 1, 3, 2]
    # compact: no dead position and no dead pool word is left, and the answers stay
    st = b.db.stats()
    assert st["positions"] == 5 and st["live"] == 4 and st["pool_dead"] == 9
    b.db.compact()
    st = b.db.stats()
    assert (st["positions"], st["live"], st["pool_dead"], st["tail"]) == (4, 4, 0, 0) and st["pool_used"] == 10 + 4 * 9
    _, r = b.query([QUERY])
    assert r[0]["candidates"] == [1, 3, 2, 0] and b.db.order().tolist() == [0, 1, 3, 2]
    # every entry erased: all outputs zero or empty, before and after a rebuild
    b.erase([0, 1, 2, 3])
    for _ in range(2):
        got, r = b.query([QUERY])
        assert r[0]["candidates"] == [] and r[0]["num_sharing"] == 0 and int(got["num_candidates"][0]) == 0 and b.db.order().tolist() == []
        b.db.compact()
    b.close()


def test_erase_the_best_neighbour_of_another_entry(ctx):
    b = with_query(ctx, [entry(1, range(9)), entry(2, range(1, 10)), entry(3, range(10))], tail_limit=1000)
    b.neighbours(0, [2]); b.neighbours(1, [2])
    b.add([0, 1, 2])
    _, r = b.query([QUERY])
    assert r[0]["candidates"] == [2] and r[0]["trace"]["moved"] == 2
    b.erase([2])
    _, r = b.query([QUERY])
    assert r[0]["candidates"] == [0, 1] and r[0]["trace"]["moved"] == 0
    b.db.compact()
    _, r = b.query([QUERY])
    assert r[0]["candidates"] == [0, 1]
    b.close()


# ---------------------------------------------------------------- rebuild widths

@pytest.mark.parametrize("W", [1, 255, 256, 257, 4096])
def test_rebuild_over_vocabularies_of_several_sizes(ctx, W):
    """The index is built over num_words + 1 counters: one scan block up to 1 024, several above."""
    rng = np.random.default_rng(W)
    b = Both(ctx, num_words=W, tail_limit=3)
    q = bu.unit(sorted(set([0, W - 1] + rng.integers(0, W, 8).tolist())))
    b.put(QUERY, 10, 1, q)
    bows = []
    for i in range(12):
        w = sorted(set(rng.integers(0, W, 6).tolist() + ([W - 1] if i % 2 else [0])))
        bows.append(bu.unit(w, rng.uniform(0.5, 2.0, len(w))))
    b.put_all(bows)
    for i in range(12):                                                 # rebuilds at the 4th, 8th and 12th add
        b.add([i])
        _, r = b.query([QUERY], min_score=0.0)
    assert b.db.stats()["rebuilds"] == 3 and len(r[0]["candidates"]) >= (1 if W > 1 else 12)
    assert r[0]["num_sharing"] == 12
    b.close()


def test_rebuild_at_the_largest_vocabulary(ctx):
    """COVGPU_BOW_MAX_WORDS = 2^20 - 1 words (the vocabulary of tests/test_gpu_bow.py's limit test): the scan runs at full width, and an
    entry holds the last word id."""
    from tests import match_util
    W, inner = (1 << 20) - 1, 1024
    rng = np.random.default_rng(50)
    per = np.full(inner, 1024); per[0] = 1023
    leaf_parent = np.repeat(np.arange(1, inner + 1), per)
    desc = rng.integers(0, 256, (inner + W, 32), dtype=np.uint8)
    desc[-1024:] = match_util.flip(np.repeat(desc[inner - 1][None], 1024, 0), 0.1, rng)
    desc[-1] = desc[inner - 1]
    weight = np.concatenate([np.zeros(inner), rng.uniform(0.5, 9.0, W)])
    voc = vocio.from_nodes(1024, 2, vocio.L1_NORM, vocio.TF_IDF, np.concatenate([np.zeros(inner, np.int64), leaf_parent]),
                           np.arange(inner + W) >= inner, desc, weight)
    assert voc["num_words"] == W
    last, d2, d3 = desc[-1], desc[-2], desc[-3]                          # the last three words: leaves of the last inner node
    other = desc[rng.integers(inner, inner + W, 12)]
    rows = np.concatenate([np.stack([last, d2]), other[:4], np.stack([last]), other[4:8], np.stack([d3]), other[8:], np.stack([last, d2, d3])])
    ptr = np.array([0, 6, 11, 16, 19], np.int32)                        # three entries and the query
    ref = br.transform_sets(voc, ptr, rows, 1)
    assert ref["word"][ref["bow_ptr"][1] - 1] == W - 1 and ref["word"][ref["bow_ptr"][2] - 1] == W - 1
    assert ref["word"][ref["bow_ptr"][3]:].tolist() == [W - 3, W - 2, W - 1]
    b = Both(ctx, voc=voc, levelsup=1, tail_limit=0)
    got = b.db.put_descriptors([0, 1, 2, QUERY], [1000, 1200, 1400, 10], [0, 0, 0, 1], dict(row_ptr=ptr, desc=rows), want=True)
    assert np.array_equal(got["word"], ref["word"]) and np.array_equal(bits(got["value"]), bits(ref["value"]))
    for i, s in enumerate([0, 1, 2, QUERY]):
        r = slice(ref["bow_ptr"][i], ref["bow_ptr"][i + 1])
        b.ref.put(s, [1000, 1200, 1400, 10][i], [0, 0, 0, 1][i], (ref["word"][r], ref["value"][r]))
    b.add([0]); b.add([1]); b.add([2])
    _, r = b.query([QUERY], min_score=0.0)
    assert r[0]["num_sharing"] == 3 and r[0]["max_common_words"] == 2 and r[0]["candidates"] == [0]
    assert b.db.stats()["rebuilds"] == 3
    b.close()


# ---------------------------------------------------------------- equivalence with the stateless call

def _map_handle(ctx, mode, opts, **kw):
    tab, nbs = bu.map_table(), bu.map_neighbours()
    K = len(tab)
    db = ctx.bowdb(None, mode=mode, num_words=bu.vocab()["num_words"], **opts, **kw)
    db.put(np.arange(K), tab.id, tab.client, tab.bow_ptr, tab.word, tab.value)
    db.set_neighbours(np.arange(K), nbs)
    db.set_invalid(np.arange(K), tab.invalid)
    return db


@pytest.mark.parametrize("mode", ["covins", "covins_g"])
def test_query_equals_the_stateless_call(ctx, mode):
    """30 seeded states of the small map, random live subsets in random insertion order, reached one from the other by erase and add."""
    tab, nbs = bu.map_table(), bu.map_neighbours()
    K, t = len(tab), bu.table_dict(bu.map_table())
    opts = dict(min_loop_dist=30)
    db = _map_handle(ctx, mode, opts, tail_limit=64)
    rng = np.random.default_rng(7 if mode == "covins" else 8)
    busy = 0
    for state in range(30):
        db.erase(db.order())
        order = rng.permutation(K)[:rng.integers(20, K + 1)].astype(np.int32)
        db.add(order)
        assert db.order().tolist() == order.tolist()
        qs = rng.integers(0, K, 20).astype(np.int32)
        cons = [nbs[q] for q in qs]
        for ms in (None, np.full(20, 0.02)):
            want = ctx.detect_candidates_batch(t, order, qs, np.full(20, len(order)), mode=mode, min_score=ms, **opts)
            same_output(db.query(qs, cons, min_score=ms, cap=len(order)), want)
            if state % 6 == 0:                                          # the same queries one at a time
                for i in range(20):
                    one = db.query(qs[i:i + 1], cons[i:i + 1], min_score=None if ms is None else ms[i:i + 1], cap=len(order))
                    assert one["candidates"][0].tolist() == want["candidates"][i].tolist()
                    assert one["acc_score"][0].view(np.uint32).tolist() == want["acc_score"][i].view(np.uint32).tolist()
                    assert bits(one["min_score"])[0] == bits(want["min_score"])[i] and int(one["num_scored"][0]) == int(want["num_scored"][i])
        # the vacuity condition on the restatement: this state's first query, restated
        r = br.detect_candidates(tab, order, len(order), int(qs[0]), dict(br.default_opts(mode), **opts))
        busy += len(r["candidates"]) > 0
    assert busy >= 5
    assert db.stats()["rebuilds"] >= 5
    db.close()


def test_queries_in_chunks_of_three(ctx):
    """scratch_kib = 16 against 180 positions leaves room for three queries per chunk."""
    tab, nbs = bu.map_table(), bu.map_neighbours()
    K, t = len(tab), bu.table_dict(bu.map_table())
    assert (16 << 10) // (28 * K) == 3
    db = _map_handle(ctx, "covins", dict(min_loop_dist=30, scratch_kib=16), tail_limit=50)
    order = np.random.default_rng(9).permutation(K).astype(np.int32)
    db.add(order)
    qs = np.arange(0, K, 9, dtype=np.int32)
    assert len(qs) == 20
    want = ctx.detect_candidates_batch(t, order, qs, np.full(20, K), min_loop_dist=30)
    same_output(db.query(qs, [nbs[q] for q in qs], cap=K), want)
    _, refs = bu.map_queries()
    assert sum(len(c) > 0 for c in want["candidates"]) >= 5 or len(refs) == 0
    db.close()


# ---------------------------------------------------------------- transfers

def test_transfers_do_not_grow_with_the_database(ctx):
    tab, nbs, (sets, _) = bu.map_table(), bu.map_neighbours(), bu.map_sets()
    voc = bu.vocab()
    K = len(tab)
    db = ctx.bowdb(voc, min_loop_dist=30, tail_limit=16)
    voc_bytes = db.stats()["h2d_bytes"]
    assert voc_bytes >= 32 * len(voc["parent"])
    db.put_descriptors(np.arange(K), tab.id, tab.client, sets)
    st = db.stats()
    rows = len(sets["desc"])
    assert st["h2d_bytes"] <= 32 * rows + 64 * K and st["d2h_bytes"] == 4 * K          # descriptors in, the vectors' lengths out
    one = dict(row_ptr=np.array([0, 300], np.int32), desc=sets["desc"][:300])
    db.put_descriptors([K], [5000], [0], one)
    assert db.stats()["h2d_bytes"] <= 32 * 300 + 64 < voc_bytes
    db.set_neighbours(np.arange(K), nbs)
    q, con, cap, seen = 175, nbs[175], 25, []
    for live in (40, 170):
        db.add(np.arange(db.stats()["live"], live))
        assert db.stats()["live"] == live
        for ms in (None, [0.02]):
            db.query([q], [con], min_score=ms, cap=cap)
            st = db.stats()
            seen.append((st["h2d_bytes"], st["d2h_bytes"]))
            assert st["d2h_bytes"] == 1 * (4 * 4 + 8) + 1 * cap * 8                      # Q and cap only
    assert seen[0] == seen[2] and seen[1] == seen[3]
    db.query([q, q, q], [con] * 3, cap=7)
    assert db.stats()["d2h_bytes"] == 3 * (4 * 4 + 8) + 3 * 7 * 8
    db.add([170])
    assert db.stats()["h2d_bytes"] <= 64
    db.erase([3])
    assert db.stats()["h2d_bytes"] <= 64
    db.close()


# ---------------------------------------------------------------- refusals

def _bad(fn, *a, **k):
    with pytest.raises(backend.CovGpuError) as e:
        fn(*a, **k)
    msg = str(e.value)
    assert msg.startswith("covgpu error 1:") and len(msg.split(":", 2)[2].strip()) > 0, msg   # COVGPU_ERR_INVALID_ARG and a message
    return msg


def test_refusals_leave_the_handle_usable(ctx):
    b = with_query(ctx, [entry(1, range(10)), entry(2, range(5)), entry(3, range(1, 10))], num_words=2000)
    b.add([0, 1])
    db = b.db
    vec = entry(7, range(3))
    ok = lambda: b.query([QUERY])[1][0]["candidates"]
    assert ok() == [0]
    before = db.stats()
    assert "index" in _bad(db.put, [0], [1000], [0], [0, len(vec[0])], vec[0], vec[1])     # put on a live slot
    assert "vector" in _bad(db.add, [9])                                                    # add without a vector
    assert "already" in _bad(db.add, [1])                                                   # add twice
    _bad(db.add, [2, 2])
    assert "vector" in _bad(db.query, [QUERY], [[0, 9]])                                    # connected slot 9 has no vector, minimum score wanted
    assert db.query([QUERY], [[9]], min_score=[0.05])["candidates"][0].tolist() == [0]      # given: slot 9 is not read
    db.set_invalid([9], [1])
    assert db.query([QUERY], [[9]])["candidates"][0].tolist() == [0]                        # invalid: skipped as in the reference
    assert "vocabulary" in _bad(db.put_descriptors, [4], [1], [0], dict(row_ptr=np.array([0, 1], np.int32), desc=np.zeros((1, 32), np.uint8)))
    w = np.array([5, 2000], np.int32)
    assert "num_words" in _bad(db.put, [4], [1], [0], [0, 2], w, np.array([0.5, 0.5]))      # a word id at num_words
    db.put([4], [1], [0], [0, 2], np.array([5, 1999], np.int32), np.array([0.5, 0.5]))      # the last word id is fine
    _bad(db.put, [5], [1], [0], [0, 2], np.array([5, 5], np.int32), np.array([0.5, 0.5]))   # the checks of a bow CSR
    _bad(db.put, [5], [1], [0], [0, 1], np.array([5], np.int32), np.array([np.nan]))
    _bad(db.put, [5], [-1], [0], [0, 1], np.array([5], np.int32), np.array([1.0]))
    _bad(db.put, [-1], [1], [0], [0, 1], np.array([5], np.int32), np.array([1.0]))
    _bad(db.put, [1 << 24], [1], [0], [0, 1], np.array([5], np.int32), np.array([1.0]))
    _bad(db.query, [3], [[]])                                                               # a query slot without a vector
    _bad(db.query, [QUERY], [[]], min_score=[np.nan])
    _bad(db.query, [QUERY], [[-2]])
    _bad(db.set_neighbours, [0], [[-1]])
    _bad(ctx.bowdb, None, tail_limit=-1)
    _bad(ctx.bowdb, None, num_words=1 << 20)
    _bad(ctx.bowdb, dict(bu.irregular_vocab(), scoring=1))
    after = db.stats()
    assert {k: after[k] for k in ("live", "positions", "tail")} == {k: before[k] for k in ("live", "positions", "tail")}
    assert after["stored"] == before["stored"] + 1
    assert ok() == [0]
    b.add([2])
    assert ok() == [0, 2]
    b.close()
    # a context closes the databases it still owns
    c2 = backend.Context(0)
    d2 = c2.bowdb(None)
    c2.close()
    d2.close()


# ---------------------------------------------------------------- C++ facade

@pytest.fixture(scope="module")
def standin():
    """The stand-in map of the small map behind tests/cpp/facade_bowdb_shim.cpp, descriptors, neighbours and the vocabulary set."""
    import ctypes as C
    from tests import facade_util
    lib = dr.bowdb_shim()
    saved = facade_util._LIB
    facade_util._LIB = lib
    try:
        sm = facade_util.StandinMap(bu.small_map())
    finally:
        facade_util._LIB = saved
    voc, (sets, _), nbs = bu.vocab(), bu.map_sets(), bu.map_neighbours()
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    i32 = lambda a: np.ascontiguousarray(a, np.int32)
    v = {k: (i32(x) if k != "desc" and k != "weight" else np.ascontiguousarray(x)) for k, x in voc.items() if isinstance(x, np.ndarray)}
    lib.bow_set_vocab(voc["k"], voc["L"], voc["scoring"], voc["weighting"], len(v["parent"]), voc["num_words"], ip(v["parent"]), ip(v["child_ptr"]),
                      ip(v["child"]), v["desc"].ctypes.data_as(C.POINTER(C.c_uint8)), ip(v["word_id"]), v["weight"].ctypes.data_as(C.POINTER(C.c_double)))
    for k in range(len(nbs)):
        d = np.ascontiguousarray(sets["desc"][sets["row_ptr"][k]:sets["row_ptr"][k + 1]])
        nb = i32(nbs[k])
        lib.bow_set_keyframe(sm.h, k, len(d), d.ctypes.data_as(C.POINTER(C.c_uint8)), len(nb), ip(nb))
    yield sm, lib
    lib.shim_free(sm.h)                                               # by the library that built it
    sm.h = None
    lib.bow_shutdown()


@pytest.mark.parametrize("track", [1, 0])
def test_facade_replay_with_erasures(standin, track):
    """ResidentKeyframeDatabaseT over the arrival of the small map's keyframes with erasures: equal to the restatement and to
    KeyframeDatabaseT on the same sequence, with the connections re-read before each query and with TouchConnections alone. The map's
    own invalid flags differ from bu.map_table()'s, which only the minimum score reads: it is given."""
    import ctypes as C
    sm, lib = standin
    refs, live, erased = dr.replay()
    assert erased == 45 and sum(len(r["candidates"]) > 0 for r in refs) >= 100
    K = len(refs)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    lists, now = [], []
    for q in range(K):
        now.append(q)
        lists.append(dr.erase_after(q, now))
        for e in lists[-1]:
            now.remove(e)
    eptr = np.zeros(K + 1, np.int32); eptr[1:] = np.cumsum([len(x) for x in lists])
    er = np.ascontiguousarray([e for x in lists for e in x], np.int32)
    ms = np.array([r["min_score"] for r in refs])
    cnt = np.zeros(K, np.int32); cand = np.full((K, K), -1, np.int32); acc = np.zeros((K, K), np.float32)
    cnt2 = np.zeros(K, np.int32); cand2 = np.full((K, K), -1, np.int32); order = np.full(K, -1, np.int32); st = np.zeros(16, np.int64)
    n = lib.bowdb_replay(sm.h, track, 7, 30, K, ms.ctypes.data_as(C.POINTER(C.c_double)), ip(eptr), ip(er), K, ip(cnt), ip(cand),
                         acc.ctypes.data_as(C.POINTER(C.c_float)), ip(cnt2), ip(cand2), ip(order), st.ctypes.data_as(C.POINTER(C.c_int64)))
    assert n == len(live) and order[:n].tolist() == live
    for q, r in enumerate(refs):
        assert cand[q, :cnt[q]].tolist() == [int(k) for k in r["candidates"]], q
        assert acc[q, :cnt[q]].view(np.uint32).tolist() == np.array(r["acc_score"], np.float32).view(np.uint32).tolist(), q
        assert cand2[q, :cnt2[q]].tolist() == cand[q, :cnt[q]].tolist(), q
    assert (int(st[0]), int(st[1]), int(st[5])) == (180, 135, 22)      # stored, live, rebuilds (tail_limit 7)
    # the vectors the facade wrote into bow_vec_ are the restatement's
    b = bu.map_bows()
    for k in (0, 57, K - 1):
        b0, b1 = int(b["bow_ptr"][k]), int(b["bow_ptr"][k + 1])
        w = np.zeros(b1 - b0 + 1, np.int32); x = np.zeros(b1 - b0 + 1)
        assert lib.bow_get(sm.h, k, len(w), ip(w), x.ctypes.data_as(C.POINTER(C.c_double))) == b1 - b0
        assert np.array_equal(w[:-1], b["word"][b0:b1]) and np.array_equal(bits(x[:-1]), bits(b["value"][b0:b1]))


def test_facade_batch_with_the_minimum_score_computed(ctx, standin):
    """DetectCandidatesBatch without minimum scores equals the stateless Python route on the map's own table, in both modes."""
    import ctypes as C
    sm, lib = standin
    m, nbs, bows = bu.small_map(), bu.map_neighbours(), bu.map_bows()
    K = m.K
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    i32 = lambda a: np.ascontiguousarray(a, np.int32)
    nptr = np.zeros(K + 1, np.int32); nptr[1:] = np.cumsum([len(x) for x in nbs])
    table = dict(id=m.kf_id, client=m.kf_client, bow_ptr=bows["bow_ptr"], word=bows["word"], value=bows["value"], nb_ptr=nptr,
                 nb=np.concatenate([i32(x) for x in nbs]), invalid=m.kf_invalid)
    order = i32(np.random.default_rng(41).permutation(K)[:150])
    qs = i32(np.arange(0, K, 6))
    for mode, name in ((0, "covins"), (1, "covins_g")):
        for min_score in (None, np.full(len(qs), 0.03)):
            want = ctx.detect_candidates_batch(table, order, qs, np.full(len(qs), len(order)), mode=name, min_score=min_score, min_loop_dist=30)
            cnt = np.zeros(len(qs), np.int32); cand = np.full((len(qs), K), -1, np.int32); acc = np.zeros((len(qs), K), np.float32); mso = np.zeros(len(qs))
            lib.bowdb_detect(sm.h, mode, 30, K, len(order), ip(order), len(qs), ip(qs),
                             None if min_score is None else min_score.ctypes.data_as(C.POINTER(C.c_double)), K, ip(cnt), ip(cand),
                             acc.ctypes.data_as(C.POINTER(C.c_float)), mso.ctypes.data_as(C.POINTER(C.c_double)))
            assert np.array_equal(cnt, want["num_candidates"]) and np.array_equal(bits(mso), bits(want["min_score"]))
            for i in range(len(qs)):
                assert cand[i, :cnt[i]].tolist() == want["candidates"][i].tolist()
                assert np.array_equal(acc[i, :cnt[i]].view(np.uint32), want["acc_score"][i].view(np.uint32))
    tab = br.Table(m.kf_id, m.kf_client, [bu.map_table().bow(k) for k in range(K)], nbs, m.kf_invalid)
    inv = br.inverted_index(tab, order)
    assert sum(len(br.detect_candidates(tab, order, len(order), int(q), bu.MAP_OPTS, inv=inv)["candidates"]) > 0 for q in qs) >= 5


# ---------------------------------------------------------------- chain

def test_chain_from_a_database_grown_by_adds(ctx):
    """Descriptors -> put_descriptors -> query -> consistency groups -> ComputeSE3's stages (tests/test_gpu_bow.py's chain), the database
    grown keyframe by keyframe; the candidates equal the restatement's and the verified ones are true revisits."""
    from scipy.spatial.transform import Rotation as Rot
    from tests import guided_util as gu
    from tests.test_gpu_bow import _chain
    m = gu.small_map()
    kfs, _ = gu.map_keyframes("ref")
    K = len(kfs)
    ptr = np.zeros(K + 1, np.int32); ptr[1:] = np.cumsum([len(k["desc"]) for k in kfs])
    db = ctx.bowdb(bu.vocab(), tail_limit=32, **bu.MAP_OPTS)
    tr = db.put_descriptors(np.arange(K), m.kf_id, m.kf_client, dict(row_ptr=ptr, desc=np.concatenate([k["desc"] for k in kfs])), want=True)
    nbs = bu.neighbour_lists([k["lm"][k["lm"] >= 0].tolist() for k in kfs])
    nbs = [[n for n in l if m.kf_client[n] == m.kf_client[k] and abs(int(m.kf_id[n]) - int(m.kf_id[k])) < 30] for k, l in enumerate(nbs)]
    db.set_neighbours(np.arange(K), nbs)
    bows = [(tr["word"][tr["bow_ptr"][k]:tr["bow_ptr"][k + 1]], tr["value"][tr["bow_ptr"][k]:tr["bow_ptr"][k + 1]]) for k in range(K)]
    tab = br.Table(m.kf_id, m.kf_client, bows, nbs)
    order = np.arange(K, dtype=np.int32)
    inv = br.inverted_index(tab, order)
    f_dev, f_ref, routes = backend.ConsistencyFilter(3), backend.ConsistencyFilter(3), ([], [])
    for q in range(K):
        if q >= 90:
            got = db.query([q], [nbs[q]])
            ref = br.detect_candidates(tab, order, q, q, bu.MAP_OPTS, inv=inv)
            equal(got, [ref])
            routes[0].extend((q, int(c)) for c in f_dev.feed(got["candidates"][0], tab.neighbours))
            routes[1].extend((q, int(c)) for c in f_ref.feed(ref["candidates"], tab.neighbours))
        db.add([q])
    db.close()
    assert routes[0] == routes[1] and len(routes[1]) >= 5
    a = _chain(ctx, routes[0])
    assert len(a) >= 3
    ok = 0
    for q, c, T, inl in a:
        if inl <= 0:
            continue
        Tt = kfs[q]["T_cw"] @ np.linalg.inv(kfs[c]["T_cw"])
        assert np.linalg.norm(T[4:] - Tt[:3, 3]) < 0.1
        assert np.rad2deg(Rot.from_matrix(Rot.from_quat(T[:4]).as_matrix().T @ Tt[:3, :3]).magnitude()) < 1.0
        ok += 1
    assert ok >= 3
