"""Line-by-line numpy restatement of the reference's bag-of-words retrieval: the yardstick of k_bow.hip, as
tests/guided_ref.py is for the guided matching. DBoW2 needs OpenCV and cannot be compiled for the tests, so parity is to this file.

  transform()          TemplatedVocabulary::transform (TemplatedVocabulary.h:1127-1194, 1218-1259), BowVector::addWeight /
                       addIfNotExist / normalize (BowVector.cpp:34-84), under L1 scoring
  score()              L1Scoring::score (ScoringObject.cpp:23-68)
  min_score()          the reference score of PlaceRecognition::DetectLoop (placerec_be.cpp:372-389)
  detect_candidates()  KeyframeDatabase::DetectCandidates (kf_database.cpp:47-187), stateless, on arrays
  StatefulDatabase     the same function literally, with the per-keyframe scratch fields loop_query_ / loop_words_ / loop_score_ and
                       AddKeyframe; tests/test_bow_host.py holds it equal to detect_candidates()
  ConsistencyFilter    the covisibility-consistency groups of DetectLoop (placerec_be.cpp:398-460)

Every float / double / int conversion sits where the reference has it: `float` is np.float32, `double` and precision_t are Python
floats (np.float64 arithmetic), `int` is a Python int. A vocabulary is the dict that covins_amd/vocio.py reads; a bow vector is a pair
(words int32 ascending, values float64)."""
from __future__ import annotations

import numpy as np

TF_IDF, TF, IDF, BINARY = 0, 1, 2, 3
L1_NORM = 0
f32 = np.float32

_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def transform_one(voc, feature, levelsup):
    """transform(feature, word_id, weight, nid, levelsup). Returns (word id, weight, nid). Where the leaf lies above nid_level (only in an
    irregular tree) the reference leaves *nid uninitialised; this project defines it as the leaf."""
    child_ptr, child, desc, word_id, weight = voc["child_ptr"], voc["child"], voc["desc"], voc["word_id"], voc["weight"]
    nid_level = int(voc["L"]) - levelsup
    nid = 0 if nid_level <= 0 else None
    final_id, current_level = 0, 0
    while True:
        current_level += 1
        nodes = child[child_ptr[final_id]:child_ptr[final_id + 1]]
        dist = _POP[np.bitwise_xor(desc[nodes], feature)].sum(axis=1).tolist()   # F::distance to every child, then the loop as written
        final_id = int(nodes[0])
        best_d = dist[0]
        for n, d in zip(nodes[1:].tolist(), dist[1:]):
            if d < best_d:
                best_d, final_id = d, n
        if current_level == nid_level:
            nid = final_id
        if word_id[final_id] >= 0:
            break
    if nid is None:
        nid = final_id
    return int(word_id[final_id]), float(weight[final_id]), nid


def transform(voc, features, levelsup=4):
    """transform(features, v, fv, levelsup) under L1. Returns (words, values, row_word, row_node): the BowVector in ascending word id,
    per feature the word id (-1 if stopped) and the FeatureVector key."""
    assert voc["scoring"] == L1_NORM
    features = np.asarray(features, np.uint8).reshape(-1, 32)
    v = {}                                        # std::map<WordId, WordValue>
    row_word = np.full(len(features), -1, np.int32)
    row_node = np.zeros(len(features), np.int32)
    add_weight = voc["weighting"] in (TF, TF_IDF)
    for i, f in enumerate(features):
        wid, w, nid = transform_one(voc, f, levelsup)
        row_node[i] = nid
        if w > 0:                                 # not stopped
            row_word[i] = wid
            if wid in v:
                if add_weight:
                    v[wid] = v[wid] + w           # addWeight: vit->second += v
            else:
                v[wid] = w                        # addWeight / addIfNotExist: insert
    words = np.array(sorted(v), np.int32)
    values = np.array([v[w] for w in words], np.float64)
    norm = 0.0                                    # BowVector::normalize(L1)
    for x in values:
        norm += abs(float(x))
    if norm > 0.0:
        values = np.array([float(x) / norm for x in values], np.float64)
    return words, values, row_word, row_node


def transform_sets(voc, row_ptr, desc, levelsup=4):
    """transform() of every set of a row_ptr / desc batch. Returns dict(bow_ptr, word, value, row_word, row_node). Equal descriptors
    descend alike, so each distinct row is walked once."""
    desc = np.asarray(desc, np.uint8).reshape(-1, 32)
    uniq, inv = np.unique(desc, axis=0, return_inverse=True) if len(desc) else (desc, np.zeros(0, np.int64))
    inv = np.asarray(inv).ravel()
    one = [transform_one(voc, u, levelsup) for u in uniq]
    add_weight = voc["weighting"] in (TF, TF_IDF)
    ptr, words, values = [0], [], []
    row_word = np.full(len(desc), -1, np.int32)
    row_node = np.zeros(len(desc), np.int32)
    for s in range(len(row_ptr) - 1):
        v = {}
        for r in range(int(row_ptr[s]), int(row_ptr[s + 1])):
            wid, w, nid = one[inv[r]]
            row_node[r] = nid
            if w > 0:
                row_word[r] = wid
                if wid in v:
                    if add_weight:
                        v[wid] = v[wid] + w
                else:
                    v[wid] = w
        ws = sorted(v)
        norm = 0.0
        for w in ws:
            norm += abs(v[w])
        words += ws
        values += [v[w] / norm if norm > 0.0 else v[w] for w in ws]
        ptr.append(len(words))
    return dict(bow_ptr=np.array(ptr, np.int32), word=np.array(words, np.int32), value=np.array(values, np.float64), row_word=row_word,
                row_node=row_node)


def score(v1, v2):
    """L1Scoring::score. lower_bound() on a map moves to the first id >= the other's; on sorted arrays that is a plain advance."""
    (w1, x1), (w2, x2) = v1, v2
    i, j, s = 0, 0, 0.0
    while i < len(w1) and j < len(w2):
        if w1[i] == w2[j]:
            vi, wi = float(x1[i]), float(x2[j])
            s += abs(vi - wi) - abs(vi) - abs(wi)
            i += 1; j += 1
        elif w1[i] < w2[j]:
            i += 1
        else:
            j += 1
    return -s / 2.0


def score_dict(v1, v2):
    """The same score on std::map-like dicts, the common words visited in ascending id (self-check of score())."""
    a, b = dict(zip(v1[0].tolist(), v1[1].tolist())), dict(zip(v2[0].tolist(), v2[1].tolist()))
    s = 0.0
    for w in sorted(set(a) & set(b)):
        s += abs(a[w] - b[w]) - abs(a[w]) - abs(b[w])
    return -s / 2.0


class Table:
    """The keyframe table of covgpu_detect_candidates_batch: id, client, bow CSR, neighbour CSR (table indices in the reference's
    order), invalid."""

    def __init__(self, id, client, bows, neighbours, invalid=None):
        self.id = np.asarray(id, np.int32); self.client = np.asarray(client, np.int32)
        n = len(self.id)
        self.bow_ptr = np.zeros(n + 1, np.int32); self.bow_ptr[1:] = np.cumsum([len(b[0]) for b in bows])
        self.word = np.concatenate([np.asarray(b[0], np.int32) for b in bows] + [np.zeros(0, np.int32)])
        self.value = np.concatenate([np.asarray(b[1], np.float64) for b in bows] + [np.zeros(0)])
        self.nb_ptr = np.zeros(n + 1, np.int32); self.nb_ptr[1:] = np.cumsum([len(x) for x in neighbours])
        self.nb = np.concatenate([np.asarray(x, np.int32) for x in neighbours] + [np.zeros(0, np.int32)])
        self.invalid = np.zeros(n, np.uint8) if invalid is None else np.asarray(invalid, np.uint8)

    def __len__(self):
        return len(self.id)

    def bow(self, k):
        r = slice(int(self.bow_ptr[k]), int(self.bow_ptr[k + 1]))
        return self.word[r], self.value[r]

    def neighbours(self, k):
        return self.nb[int(self.nb_ptr[k]):int(self.nb_ptr[k + 1])]


def default_opts(mode="covins"):
    """config_backend.yaml:72-78; the factor of placerec_be.cpp:389 (COVINS) and placerec_gen_be.cpp (COVINS-G)."""
    return dict(min_score_factor=0.7 if mode == "covins_g" else 0.8, min_loop_dist=100, exclude_kfs_with_id_less_than=7,
                inter_map_matches_only=0)


def min_score(tab, q, factor):
    minScore = f32(1)
    for n in tab.neighbours(q):
        if tab.invalid[n]:
            continue
        sc = f32(score(tab.bow(q), tab.bow(n)))   # float score = voc_->score(...)
        if sc < minScore:
            minScore = sc
    return float(minScore) * factor               # minScore * 0.8: float promoted to double


def _skipped(tab, q, i, opts):
    same = tab.client[i] == tab.client[q]
    if tab.id[i] == tab.id[q] and same:
        return True
    if opts["inter_map_matches_only"] and same:
        return True
    if same and abs(int(tab.id[q]) - int(tab.id[i])) < opts["min_loop_dist"]:
        return True
    return bool(tab.id[i] < opts["exclude_kfs_with_id_less_than"])


def _select(q_id, minsc, sharing, words_of, score_of, neighbours_of, in_list):
    """kf_database.cpp:88-186 from the sharing list on. words_of / score_of: loop_words_ / setter-getter of loop_score_; in_list(k):
    loop_query_ == kf->id_. Returns dict(candidates, acc_score, num_sharing, max_common_words, num_scored, trace)."""
    out = dict(candidates=[], acc_score=[], num_sharing=len(sharing), max_common_words=0, num_scored=0,
               trace=dict(moved=0, dedup=0, dropped=0))
    if not sharing:
        return out
    maxCommonWords = 0
    for k in sharing:
        if words_of(k) > maxCommonWords:
            maxCommonWords = words_of(k)
    out["max_common_words"] = maxCommonWords
    minCommonWords = int(f32(maxCommonWords) * f32(0.8))          # int = int * 0.8f
    lScoreAndMatch, loop_score = [], {}
    for k in sharing:
        if words_of(k) > minCommonWords:
            out["num_scored"] += 1
            si = score_of(k)
            loop_score[k] = si
            if si >= minsc:
                lScoreAndMatch.append((f32(si), k))               # listFloatKfPair
    if not lScoreAndMatch:
        return out
    lAcc = []
    bestAccScore = float(minsc)
    for first, k in lScoreAndMatch:
        bestScore, accScore, pBestKF = f32(first), f32(first), k
        for k2 in neighbours_of(k)[:10]:
            k2 = int(k2)
            if in_list(k2) and words_of(k2) > minCommonWords:
                accScore = f32(float(accScore) + loop_score[k2])  # float += double
                if loop_score[k2] > float(bestScore):
                    pBestKF, bestScore = k2, f32(loop_score[k2])
        out["trace"]["moved"] += pBestKF != k
        lAcc.append((accScore, pBestKF))
        if float(accScore) > bestAccScore:
            bestAccScore = float(accScore)
    minScoreToRetain = f32(float(f32(0.75)) * bestAccScore)      # float = 0.75f * double
    added = set()
    for a, k in lAcc:
        if a > minScoreToRetain:
            if k not in added:
                out["candidates"].append(k); out["acc_score"].append(a)
                added.add(k)
            else:
                out["trace"]["dedup"] += 1
        else:
            out["trace"]["dropped"] += 1
    return out


def inverted_index(tab, db_order):
    """inverted_file_index_ after AddKeyframe of db_order in turn: word -> [(position, keyframe)], posting lists in insertion order."""
    inv = {}
    for p, k in enumerate(db_order):
        for w in tab.bow(int(k))[0]:
            inv.setdefault(int(w), []).append((p, int(k)))
    return inv


def detect_candidates(tab, db_order, visible, q, opts, minsc=None, inv=None):
    """DetectCandidates of keyframe q against db_order[:visible], stateless. Candidates are table indices in the reference's order.
    `inv`: inverted_index(tab, db_order) when the caller keeps one for many queries."""
    if minsc is None:
        minsc = min_score(tab, q, opts["min_score_factor"])
    connected = set(int(n) for n in tab.neighbours(q))
    if inv is None:
        inv = inverted_index(tab, db_order)
    sharing, words = [], {}
    for w in tab.bow(q)[0]:
        for p, k in inv.get(int(w), ()):
            if p >= visible:
                break                             # not yet added
            if _skipped(tab, q, k, opts):
                continue
            if k in connected:
                continue                          # loop_query_ is never set: never joins, never counts
            if k not in words:
                words[k] = 0
                sharing.append(k)
            words[k] += 1
    qb = tab.bow(q)
    out = _select(None, minsc, sharing, lambda k: words[k], lambda k: score(qb, tab.bow(k)), tab.neighbours, lambda k: k in words)
    out["min_score"] = minsc
    return out


class StatefulDatabase:
    """KeyframeDatabase with the reference's scratch fields on the keyframes, literally (kf_database.cpp:41-187)."""
    DEFPAIR = (-1, -1)

    def __init__(self, tab):
        self.tab = tab
        self.inverted = {}
        n = len(tab)
        self.loop_words = [0] * n; self.loop_query = [self.DEFPAIR] * n; self.loop_score = [0.0] * n

    def AddKeyframe(self, k):
        for w in self.tab.bow(k)[0]:
            self.inverted.setdefault(int(w), []).append(k)

    def DetectCandidates(self, q, opts, minsc=None):
        tab = self.tab
        if minsc is None:
            minsc = min_score(tab, q, opts["min_score_factor"])
        qid = (int(tab.id[q]), int(tab.client[q]))
        connected = set(int(n) for n in tab.neighbours(q))
        sharing = []
        for w in tab.bow(q)[0]:
            for k in self.inverted.get(int(w), ()):
                if _skipped(tab, q, k, opts):
                    continue
                if not self.loop_query[k] == qid:
                    self.loop_words[k] = 0
                    if k not in connected:
                        self.loop_query[k] = qid
                        sharing.append(k)
                self.loop_words[k] += 1
        qb = tab.bow(q)

        def score_of(k):
            self.loop_score[k] = score(qb, tab.bow(k))
            return self.loop_score[k]
        out = _select(qid, minsc, sharing, lambda k: self.loop_words[k], score_of, tab.neighbours, lambda k: self.loop_query[k] == qid)
        out["min_score"] = minsc
        return out


class ConsistencyFilter:
    """mvConsistentGroups of PlaceRecognition::DetectLoop (placerec_be.cpp:391-460). feed(candidates, group_of) returns
    mvpEnoughConsistentCandidates; group_of(k) is the candidate's connected keyframes (the candidate itself is added here)."""

    def __init__(self, threshold=3):
        self.threshold = threshold                # mnCovisibilityConsistencyTh (cov_consistency_thres)
        self.groups = []                          # [(set, count)]

    def feed(self, candidates, group_of):
        if len(candidates) == 0:
            self.groups = []                      # mvConsistentGroups.clear()
            return []
        enough, current = [], []
        used = [False] * len(self.groups)
        for cand in candidates:
            group = set(int(k) for k in group_of(cand)) | {int(cand)}
            bEnough = bForSome = False
            for g, (prev, n) in enumerate(self.groups):
                if group & prev:
                    bForSome = True
                    if not used[g]:
                        current.append((group, n + 1))
                        used[g] = True
                    if n + 1 >= self.threshold and not bEnough:
                        enough.append(int(cand))
                        bEnough = True
            if not bForSome:
                current.append((group, 0))
        self.groups = current
        return enough
