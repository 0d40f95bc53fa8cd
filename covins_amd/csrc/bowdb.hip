// bowdb.hip — host side of the resident keyframe database (covgpu_bowdb; kernels in k_bowdb.hip and k_bow.hip).
// The handle owns its device buffers; each grows by doubling with a device-to-device copy, so the database never passes through the
// host. The host keeps what the argument checks need and no more: per slot whether it is stored, live and invalid and how long its
// vector is, and the counts. Every entry point checks all its arguments before it changes anything, makes every copy through
// BowDb::up / BowDb::down, which count the bytes covgpu_bowdb_stats reports, and synchronises the stream before it returns.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "host.hpp"

using namespace covgpu;

namespace {

struct DevBuf { char* p = nullptr; size_t cap = 0; };   // bytes

// One call's carve-up of the handle's scratch buffer: add() every piece, reserve, then at().
struct Carve {
  size_t total = 0;
  size_t add(size_t bytes) { const size_t off = total; total += (bytes + 255) & ~(size_t)255; return off; }
};

}  // namespace

struct covgpu_bowdb {
  covgpu_context* c = nullptr;
  covgpu_bowdb_opts o{};
  bool have_voc = false;
  BowVocabDev V{};
  int nid_level = 0, add_weight = 0, num_words = 0;
  DevBuf voc[5];
  // per slot
  DevBuf id, client, vec_beg, vec_end, pos_of, nb_beg, nb_end, nb;
  size_t slot_cap = 0;
  int num_slots = 0;                               // highest stored or named slot + 1
  // per position
  DevBuf order, dead;
  size_t pos_cap = 0;
  int P = 0, base = 0;                             // positions; those below `base` are in the index
  // vector pool and index
  DevBuf pword, pvalue, inv_ptr, inv_pos;
  size_t pool_cap = 0;
  int64_t pool_used = 0, pool_dead = 0, base_postings = 0;
  DevBuf tmp;                                      // scratch of one call, per-query scratch included
  // host mirror
  std::vector<uint8_t> stored, live, invalid;
  std::vector<int32_t> len;
  int stored_count = 0, live_count = 0;
  int64_t live_words = 0;
  int64_t rebuilds = 0, growths = 0, h2d = 0, d2h = 0, dev_bytes = 0;

  hipStream_t st() const { return c->st; }
  hipError_t up(void* d, const void* h, size_t bytes) {
    if (!bytes) return hipSuccess;
    h2d += (int64_t)bytes;
    return hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, st());
  }
  hipError_t down(void* h, const void* d, size_t bytes) {
    if (!bytes || !h) return hipSuccess;
    d2h += (int64_t)bytes;
    return hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, st());
  }
  // Grows b to at least `need` bytes (doubling). The first `keep` bytes survive through a device-to-device copy; the rest is set to `fill`.
  int grow(DevBuf& b, size_t need, size_t keep, int fill) {
    if (need <= b.cap && b.p) return COVGPU_OK;
    const size_t cap = std::max<size_t>(std::max(need, 2 * b.cap), 256);
    char* p = nullptr;
    HIPCHK(hipMalloc((void**)&p, cap));
    keep = std::min(keep, b.cap);
    if (keep) HIPCHK(hipMemcpyAsync(p, b.p, keep, hipMemcpyDeviceToDevice, st()));
    HIPCHK(hipMemsetAsync(p + keep, fill, cap - keep, st()));
    if (b.p) { HIPCHK(hipStreamSynchronize(st())); (void)hipFree(b.p); ++growths; }
    dev_bytes += (int64_t)cap - (int64_t)b.cap;
    b.p = p; b.cap = cap;
    return COVGPU_OK;
  }
  void release(DevBuf& b) { if (b.p) (void)hipFree(b.p); dev_bytes -= (int64_t)b.cap; b = DevBuf(); }
  int ensure_slots(size_t n) {
    if (n > stored.size()) { stored.resize(n, 0); live.resize(n, 0); invalid.resize(n, 0); len.resize(n, 0); }
    if (n <= slot_cap) return COVGPU_OK;
    const size_t cap = std::max(n, 2 * slot_cap), old = slot_cap;
    for (DevBuf* b : {&id, &client, &vec_beg, &vec_end, &nb_beg, &nb_end}) RC(grow(*b, 4 * cap, 4 * old, 0));
    RC(grow(pos_of, 4 * cap, 4 * old, 0xff));      // -1: not in the index
    RC(grow(nb, 4 * cap * kBowDbNeighbours, 4 * old * kBowDbNeighbours, 0));
    slot_cap = cap;
    return COVGPU_OK;
  }
  int ensure_positions(size_t n) {
    if (n <= pos_cap) return COVGPU_OK;
    const size_t cap = std::max(n, 2 * pos_cap);
    RC(grow(order, 4 * cap, 4 * pos_cap, 0)); RC(grow(dead, cap, pos_cap, 0));
    pos_cap = cap;
    return COVGPU_OK;
  }
  int ensure_pool(size_t n) {
    if (n <= pool_cap) return COVGPU_OK;
    const size_t cap = std::max(n, 2 * pool_cap);
    RC(grow(pword, 4 * cap, 4 * (size_t)pool_used, 0)); RC(grow(pvalue, 8 * cap, 8 * (size_t)pool_used, 0));
    pool_cap = cap;
    return COVGPU_OK;
  }
  BowDbDev dev() const {
    return BowDbDev{(int*)id.p, (int*)client.p, (int*)vec_beg.p, (int*)vec_end.p, (int*)pos_of.p, (int*)nb_beg.p, (int*)nb_end.p, (int*)nb.p,
                    (int*)order.p, (unsigned char*)dead.p, (int*)pword.p, (double*)pvalue.p};
  }
  int rebuild();
};

namespace {

// The prologue of every entry point that takes a handle: a NULL handle is an argument error, the byte counters start at zero, no C++
// exception leaves the call, and the stream has drained when the call returns (the host arrays of its copies are the caller's or the
// body's own).
template <typename F>
int db_entry(const char* fn, covgpu_bowdb* db, F&& body) {
  auto bad = [fn](const char* m) -> int { g_err = std::string(fn) + ": " + m; return COVGPU_ERR_INVALID_ARG; };
  if (!db) return bad("NULL handle");
  return guarded([&]() -> int {
    HIPCHK(hipSetDevice(db->c->device));
    db->h2d = db->d2h = 0;
    const int rc = body(bad);
    const hipError_t e = hipStreamSynchronize(db->st());
    if (rc == COVGPU_OK) HIPCHK(e);
    return rc;
  });
}

// The first violation of a list of n slots, or nullptr. `seen` (all zero, at least as long as the largest slot) catches a repeat.
const char* slots_check(int n, const int32_t* slot, std::vector<uint8_t>* seen) {
  if (n < 0) return "negative count";
  if (n > 0 && !slot) return "NULL slot array";
  for (int i = 0; i < n; ++i) if (slot[i] < 0 || slot[i] >= COVGPU_BOWDB_MAX_SLOTS) return "slot is not in 0..COVGPU_BOWDB_MAX_SLOTS-1";
  if (seen) {
    int hi = 0;
    for (int i = 0; i < n; ++i) hi = std::max(hi, slot[i] + 1);
    seen->assign((size_t)hi, 0);
    for (int i = 0; i < n; ++i) {
      if ((*seen)[slot[i]]) return "a slot twice in one call";
      (*seen)[slot[i]] = 1;
    }
  }
  return nullptr;
}

}  // namespace

// Renumbers the live positions (order kept), drops the dead words of the pool and builds the base index over every live position,
// all on the device: k_bowdb.hip.
int covgpu_bowdb::rebuild() {
  const int L = live_count, N = num_slots, W = num_words;
  if ((int64_t)live_words > (int64_t)INT32_MAX) { g_err = "covgpu_bowdb: more than 2^31 - 1 database words"; return COVGPU_ERR_INVALID_ARG; }
  Carve cv;
  const size_t scan_ints = bowdb_scan_tmp_ints(std::max(std::max(P, N), W) + 1);
  const size_t o_pos = cv.add(4 * ((size_t)P + 1)), o_ord = cv.add(4 * (size_t)std::max(L, 1)), o_beg = cv.add(4 * ((size_t)N + 1)),
               o_cur = cv.add(4 * (size_t)W), o_scan = cv.add(4 * scan_ints);
  RC(grow(tmp, cv.total, 0, 0));
  int *new_pos = (int*)(tmp.p + o_pos), *new_order = (int*)(tmp.p + o_ord), *new_beg = (int*)(tmp.p + o_beg), *cursor = (int*)(tmp.p + o_cur),
      *scan_tmp = (int*)(tmp.p + o_scan);
  if (P > L) {                                     // erased positions: the survivors move down
    launch_bowdb_renumber(dev(), P, new_pos, new_order, scan_tmp, st());
    if (L > 0) HIPCHK(hipMemcpyAsync(order.p, new_order, 4 * (size_t)L, hipMemcpyDeviceToDevice, st()));
    HIPCHK(hipMemsetAsync(dead.p, 0, (size_t)P, st()));
    P = L;
  }
  if (pool_dead > 0) {                             // replaced vectors: the pool is rewritten in slot order
    DevBuf nw, nv;
    RC(grow(nw, pword.cap, 0, 0));
    RC(grow(nv, pvalue.cap, 0, 0));
    launch_bowdb_compact_pool(dev(), N, new_beg, (int*)nw.p, (double*)nv.p, scan_tmp, st());
    HIPCHK(hipStreamSynchronize(st()));
    release(pword); release(pvalue);
    pword = nw; pvalue = nv;
    pool_used -= pool_dead; pool_dead = 0;
  }
  RC(grow(inv_pos, 4 * (size_t)std::max<int64_t>(live_words, 1), 0, 0));
  int* ip = (int*)inv_ptr.p;
  HIPCHK(hipMemsetAsync(ip, 0, 4 * ((size_t)W + 1), st()));
  launch_bowdb_histogram(dev(), L, ip, st());
  launch_bowdb_scan(ip, W, ip, W + 1, scan_tmp, st());
  HIPCHK(hipMemcpyAsync(cursor, ip, 4 * (size_t)W, hipMemcpyDeviceToDevice, st()));
  launch_bowdb_scatter(dev(), L, cursor, (int*)inv_pos.p, st());
  HIPCHK(hipGetLastError());
  base = P; base_postings = live_words; ++rebuilds;
  return COVGPU_OK;
}

extern "C" void covgpu_default_bowdb_opts(covgpu_bowdb_opts* o, int32_t mode) {
  if (!o) return;
  covgpu_default_detect_opts(&o->detect, mode);
  o->levelsup = 4; o->tail_limit = 256; o->reserve_kf = 1024; o->reserve_words = 1 << 18; o->num_words = 0;
}

extern "C" int covgpu_bowdb_create(covgpu_context* c, const covgpu_bow_vocab_t* v, const covgpu_bowdb_opts* opts, covgpu_bowdb** out) {
  auto bad = [](const char* m) -> int { g_err = std::string("covgpu_bowdb_create: ") + m; return COVGPU_ERR_INVALID_ARG; };
  if (!c) return bad("NULL context");
  if (!out) return bad("NULL out");
  *out = nullptr;
  covgpu_bowdb_opts o;
  if (opts) o = *opts; else covgpu_default_bowdb_opts(&o, COVGPU_DETECT_COVINS);
  if (!std::isfinite(o.detect.min_score_factor)) return bad("non-finite min_score_factor");
  if (o.detect.scratch_kib < 0) return bad("scratch_kib < 0");
  if (o.tail_limit < 0 || o.reserve_kf < 0 || o.reserve_words < 0) return bad("negative tail_limit, reserve_kf or reserve_words");
  if (o.reserve_kf > COVGPU_BOWDB_MAX_SLOTS) return bad("reserve_kf above COVGPU_BOWDB_MAX_SLOTS");
  if (o.num_words < 0 || o.num_words > COVGPU_BOW_MAX_WORDS) return bad("num_words is not in 0..COVGPU_BOW_MAX_WORDS");
  if (v) if (const char* m = bow_vocab_check(v)) return bad(m);
  return guarded([&]() -> int {
    HIPCHK(hipSetDevice(c->device));
    covgpu_bowdb* db = new covgpu_bowdb();
    db->c = c; db->o = o;
    c->bowdbs.push_back(db);
    auto fail = [&](int rc) { covgpu_bowdb_destroy(db); return rc; };
    db->num_words = v ? v->num_words : (o.num_words > 0 ? o.num_words : COVGPU_BOW_MAX_WORDS);
    if (v) {
      const size_t N = (size_t)v->num_nodes, W = (size_t)v->num_words;
      std::vector<double> ww(W);
      for (size_t n = 0; n < N; ++n) if (v->word_id[n] >= 0) ww[v->word_id[n]] = v->weight[n];
      const void* src[5] = {v->child_ptr, v->child, v->desc, v->word_id, ww.data()};
      const size_t bytes[5] = {4 * (N + 1), 4 * (N - 1), 32 * N, 4 * N, 8 * W};
      for (int i = 0; i < 5; ++i) {
        if (int rc = db->grow(db->voc[i], bytes[i], 0, 0)) return fail(rc);
        if (db->up(db->voc[i].p, src[i], bytes[i]) != hipSuccess) { g_err = "covgpu_bowdb_create: vocabulary upload failed"; return fail(COVGPU_ERR_NO_DEVICE); }
      }
      if (hipStreamSynchronize(c->st) != hipSuccess) { g_err = "covgpu_bowdb_create: vocabulary upload failed"; return fail(COVGPU_ERR_NO_DEVICE); }   // (ww leaves scope)
      db->V.num_nodes = (int)N;
      db->V.child_ptr = (const int*)db->voc[0].p; db->V.child = (const int*)db->voc[1].p; db->V.desc = (const uint4*)db->voc[2].p;
      db->V.word_id = (const int*)db->voc[3].p; db->V.word_weight = (const double*)db->voc[4].p;
      db->nid_level = v->L - o.levelsup;
      db->add_weight = v->weighting == COVGPU_BOW_TF_IDF || v->weighting == COVGPU_BOW_TF;
      db->have_voc = true;
    }
    if (int rc = db->grow(db->inv_ptr, 4 * ((size_t)db->num_words + 1), 0, 0)) return fail(rc);
    if (int rc = db->ensure_slots((size_t)std::max(o.reserve_kf, 1))) return fail(rc);
    db->stored.clear(); db->live.clear(); db->invalid.clear(); db->len.clear();     // (capacity is not content)
    if (int rc = db->ensure_positions((size_t)std::max(o.reserve_kf, 1))) return fail(rc);
    if (int rc = db->ensure_pool((size_t)std::max(o.reserve_words, 1))) return fail(rc);
    if (int rc = db->grow(db->inv_pos, 4 * (size_t)std::max(o.reserve_words, 1), 0, 0)) return fail(rc);
    if (hipStreamSynchronize(c->st) != hipSuccess) { g_err = "covgpu_bowdb_create: device initialisation failed"; return fail(COVGPU_ERR_NO_DEVICE); }
    db->growths = 0;
    *out = db;
    return COVGPU_OK;
  });
}

extern "C" void covgpu_bowdb_destroy(covgpu_bowdb* db) {
  if (!db) return;
  covgpu_context* c = db->c;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->st);
  for (DevBuf* b : {&db->voc[0], &db->voc[1], &db->voc[2], &db->voc[3], &db->voc[4], &db->id, &db->client, &db->vec_beg, &db->vec_end, &db->pos_of,
                    &db->nb_beg, &db->nb_end, &db->nb, &db->order, &db->dead, &db->pword, &db->pvalue, &db->inv_ptr, &db->inv_pos, &db->tmp})
    db->release(*b);
  c->bowdbs.erase(std::remove(c->bowdbs.begin(), c->bowdbs.end(), db), c->bowdbs.end());
  delete db;
}

extern "C" int covgpu_bowdb_put(covgpu_bowdb* db, int32_t n, const int32_t* slot, const int32_t* id, const int32_t* client,
                                const int32_t* bow_ptr, const int32_t* word, const double* value) {
  return db_entry("covgpu_bowdb_put", db, [&](auto bad) -> int {
    std::vector<uint8_t> seen;
    if (const char* m = slots_check(n, slot, &seen)) return bad(m);
    if (n == 0) return COVGPU_OK;
    if (!id || !client) return bad("NULL id or client");
    for (int i = 0; i < n; ++i) {
      if (id[i] < 0) return bad("negative keyframe id");
      if ((size_t)slot[i] < db->live.size() && db->live[slot[i]]) return bad("the slot is in the index: erase it before it gets another vector");
    }
    if (const char* m = bow_csr_check(n, bow_ptr, word, value)) return bad(m);
    for (int i = 0; i < n; ++i)
      if (bow_ptr[i + 1] > bow_ptr[i] && word[bow_ptr[i + 1] - 1] >= db->num_words) return bad("word id at or above num_words");
    const size_t tot = (size_t)bow_ptr[n], ns = (size_t)n;
    if (db->pool_used + (int64_t)tot > (int64_t)INT32_MAX) return bad("more than 2^31 - 1 words in the vector pool");
    int hi = 0;
    std::vector<int32_t> meta(2 * ns);                                  // begin, end in the pool
    for (int i = 0; i < n; ++i) {
      hi = std::max(hi, slot[i] + 1);
      meta[i] = (int32_t)db->pool_used + bow_ptr[i]; meta[ns + i] = (int32_t)db->pool_used + bow_ptr[i + 1];
    }
    RC(db->ensure_slots((size_t)hi));
    RC(db->ensure_pool((size_t)db->pool_used + tot));
    RC(db->grow(db->tmp, 5 * 4 * ns, 0, 0));
    int* d = (int*)db->tmp.p;
    HIPCHK(db->up(db->pword.p + 4 * (size_t)db->pool_used, word, 4 * tot));
    HIPCHK(db->up(db->pvalue.p + 8 * (size_t)db->pool_used, value, 8 * tot));
    HIPCHK(db->up(d, slot, 4 * ns)); HIPCHK(db->up(d + ns, id, 4 * ns)); HIPCHK(db->up(d + 2 * ns, client, 4 * ns));
    HIPCHK(db->up(d + 3 * ns, meta.data(), 8 * ns));
    launch_bowdb_store_meta(db->dev(), n, d, d + ns, d + 2 * ns, d + 3 * ns, d + 4 * ns, db->st());
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(db->st()));                             // (meta leaves scope)
    for (int i = 0; i < n; ++i) {
      const int s = slot[i];
      if (db->stored[s]) db->pool_dead += db->len[s]; else { db->stored[s] = 1; ++db->stored_count; }
      db->len[s] = bow_ptr[i + 1] - bow_ptr[i];
    }
    db->pool_used += (int64_t)tot;
    db->num_slots = std::max(db->num_slots, hi);
    return COVGPU_OK;
  });
}

extern "C" int covgpu_bowdb_put_descriptors(covgpu_bowdb* db, const int32_t* slot, const int32_t* id, const int32_t* client,
                                            const covgpu_bow_transform_batch_t* bt) {
  return db_entry("covgpu_bowdb_put_descriptors", db, [&](auto bad) -> int {
    if (!bt) return bad("NULL batch");
    if (!db->have_voc) return bad("the handle was created without a vocabulary");
    if (bt->levelsup != db->o.levelsup) return bad("levelsup differs from the handle's");
    const int S = bt->num_sets;
    std::vector<uint8_t> seen;
    if (const char* m = slots_check(S, slot, &seen)) return bad(m);
    if (bt->capacity < 0) return bad("capacity < 0");
    if (bt->total) *bt->total = 0;
    if (S == 0) return COVGPU_OK;
    if (!id || !client || !bt->row_ptr) return bad("NULL id, client or row_ptr");
    if (bt->row_ptr[0] != 0) return bad(kRowPtr.first);
    for (int s = 0; s < S; ++s) {
      if (id[s] < 0) return bad("negative keyframe id");
      if ((size_t)slot[s] < db->live.size() && db->live[slot[s]]) return bad("the slot is in the index: erase it before it gets another vector");
      if (const char* m = csr_row_check(bt->row_ptr, s, kRowPtr, COVGPU_MATCH_MAX_ROWS)) return bad(m);
    }
    const size_t R = (size_t)bt->row_ptr[S], Ss = (size_t)S;
    if (R > 0 && !bt->desc) return bad("NULL desc");
    if (bt->capacity > 0 && ((bt->word && !bt->value) || (!bt->word && bt->value))) return bad("word without value or value without word");
    if (db->pool_used + (int64_t)R > (int64_t)INT32_MAX) return bad("more than 2^31 - 1 words in the vector pool");
    int hi = 0;
    for (int s = 0; s < S; ++s) hi = std::max(hi, slot[s] + 1);
    RC(db->ensure_slots((size_t)hi));
    RC(db->ensure_pool((size_t)db->pool_used + R));                     // a set has at most as many words as rows
    Carve cv;
    const size_t o_desc = cv.add(32 * R), o_ptr = cv.add(4 * (Ss + 1)), o_rw = cv.add(4 * R), o_rn = cv.add(4 * R), o_ow = cv.add(4 * R),
                 o_ov = cv.add(8 * R), o_cnt = cv.add(4 * Ss), o_meta = cv.add(5 * 4 * Ss);
    RC(db->grow(db->tmp, cv.total, 0, 0));
    char* t = db->tmp.p;
    unsigned char* ddesc = (unsigned char*)(t + o_desc);
    int *dptr_ = (int*)(t + o_ptr), *drw = (int*)(t + o_rw), *drn = (int*)(t + o_rn), *dow = (int*)(t + o_ow), *dcnt = (int*)(t + o_cnt),
        *dmeta = (int*)(t + o_meta);
    double* dov = (double*)(t + o_ov);
    std::vector<int32_t> hc(Ss), meta(2 * Ss);
    HIPCHK(db->up(ddesc, bt->desc, 32 * R)); HIPCHK(db->up(dptr_, bt->row_ptr, 4 * (Ss + 1)));
    launch_bow_transform(db->V, ddesc, dptr_, S, (int)R, db->nid_level, db->add_weight, drw, drn, dow, dov, dcnt, db->st());
    HIPCHK(hipGetLastError());
    HIPCHK(db->down(hc.data(), dcnt, 4 * Ss));
    HIPCHK(hipStreamSynchronize(db->st()));                             // the counts place the vectors in the pool
    int64_t tot = 0;
    for (int s = 0; s < S; ++s) {
      meta[s] = (int32_t)(db->pool_used + tot); tot += hc[s]; meta[Ss + s] = (int32_t)(db->pool_used + tot);
    }
    HIPCHK(db->up(dmeta, slot, 4 * Ss)); HIPCHK(db->up(dmeta + Ss, id, 4 * Ss)); HIPCHK(db->up(dmeta + 2 * Ss, client, 4 * Ss));
    HIPCHK(db->up(dmeta + 3 * Ss, meta.data(), 8 * Ss));
    launch_bowdb_gather(S, dptr_, dcnt, dmeta + 3 * Ss, dow, dov, (int*)db->pword.p, (double*)db->pvalue.p, db->st());
    launch_bowdb_store_meta(db->dev(), S, dmeta, dmeta + Ss, dmeta + 2 * Ss, dmeta + 3 * Ss, dmeta + 4 * Ss, db->st());
    HIPCHK(hipGetLastError());
    if (bt->bow_ptr) {
      bt->bow_ptr[0] = 0;
      for (int s = 0; s < S; ++s) bt->bow_ptr[s + 1] = meta[Ss + s] - (int32_t)db->pool_used;
    }
    if (bt->total) *bt->total = tot;
    const size_t give = (size_t)std::min<int64_t>(tot, bt->capacity);
    HIPCHK(db->down(bt->word, db->pword.p + 4 * (size_t)db->pool_used, 4 * give));
    HIPCHK(db->down(bt->value, db->pvalue.p + 8 * (size_t)db->pool_used, 8 * give));
    HIPCHK(db->down(bt->row_word, drw, 4 * R)); HIPCHK(db->down(bt->row_node, drn, 4 * R));
    HIPCHK(hipStreamSynchronize(db->st()));                             // (meta leaves scope)
    for (int s = 0; s < S; ++s) {
      const int k = slot[s];
      if (db->stored[k]) db->pool_dead += db->len[k]; else { db->stored[k] = 1; ++db->stored_count; }
      db->len[k] = hc[s];
    }
    db->pool_used += tot;
    db->num_slots = std::max(db->num_slots, hi);
    return COVGPU_OK;
  });
}

extern "C" int covgpu_bowdb_set_neighbours(covgpu_bowdb* db, int32_t n, const int32_t* slot, const int32_t* nb_ptr, const int32_t* nb) {
  return db_entry("covgpu_bowdb_set_neighbours", db, [&](auto bad) -> int {
    std::vector<uint8_t> seen;
    if (const char* m = slots_check(n, slot, &seen)) return bad(m);
    if (n == 0) return COVGPU_OK;
    if (!nb_ptr) return bad("NULL nb_ptr");
    if (const char* m = csr_check(nb_ptr, n, kNbPtr)) return bad(m);
    if (nb_ptr[n] > 0 && !nb) return bad("NULL nb");
    const size_t ns = (size_t)n;
    std::vector<int32_t> rows(ns * kBowDbNeighbours, 0), cnt(ns);
    int hi = 0;
    for (int i = 0; i < n; ++i) {
      hi = std::max(hi, slot[i] + 1);
      cnt[i] = std::min(nb_ptr[i + 1] - nb_ptr[i], kBowDbNeighbours);
      for (int j = 0; j < cnt[i]; ++j) {
        const int k = nb[nb_ptr[i] + j];
        if (k < 0 || k >= COVGPU_BOWDB_MAX_SLOTS) return bad("neighbour slot is not in 0..COVGPU_BOWDB_MAX_SLOTS-1");
        rows[(size_t)i * kBowDbNeighbours + j] = k;
        hi = std::max(hi, k + 1);
      }
    }
    RC(db->ensure_slots((size_t)hi));
    Carve cv;
    const size_t o_slot = cv.add(4 * ns), o_rows = cv.add(4 * rows.size()), o_cnt = cv.add(4 * ns);
    RC(db->grow(db->tmp, cv.total, 0, 0));
    char* t = db->tmp.p;
    HIPCHK(db->up(t + o_slot, slot, 4 * ns)); HIPCHK(db->up(t + o_rows, rows.data(), 4 * rows.size())); HIPCHK(db->up(t + o_cnt, cnt.data(), 4 * ns));
    launch_bowdb_set_neighbours(db->dev(), n, (int*)(t + o_slot), (int*)(t + o_rows), (int*)(t + o_cnt), db->st());
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(db->st()));                             // (rows and cnt leave scope)
    db->num_slots = std::max(db->num_slots, hi);
    return COVGPU_OK;
  });
}

extern "C" int covgpu_bowdb_set_invalid(covgpu_bowdb* db, int32_t n, const int32_t* slot, const uint8_t* flag) {
  return db_entry("covgpu_bowdb_set_invalid", db, [&](auto bad) -> int {
    if (const char* m = slots_check(n, slot, nullptr)) return bad(m);
    if (n > 0 && !flag) return bad("NULL flag array");
    int hi = 0;
    for (int i = 0; i < n; ++i) hi = std::max(hi, slot[i] + 1);
    if ((size_t)hi > db->invalid.size()) RC(db->ensure_slots((size_t)hi));
    for (int i = 0; i < n; ++i) db->invalid[slot[i]] = flag[i] != 0;     // read on the host only: the minimum score's pair list
    db->num_slots = std::max(db->num_slots, hi);
    return COVGPU_OK;
  });
}

extern "C" int covgpu_bowdb_add(covgpu_bowdb* db, int32_t n, const int32_t* slot) {
  return db_entry("covgpu_bowdb_add", db, [&](auto bad) -> int {
    std::vector<uint8_t> seen;
    if (const char* m = slots_check(n, slot, &seen)) return bad(m);
    for (int i = 0; i < n; ++i) {
      if ((size_t)slot[i] >= db->stored.size() || !db->stored[slot[i]]) return bad("the slot has no stored vector");
      if (db->live[slot[i]]) return bad("the slot is already in the index");
    }
    if (n == 0) return COVGPU_OK;
    if ((int64_t)db->P + n > (int64_t)INT32_MAX / 64) return bad("too many positions");
    const size_t ns = (size_t)n;
    RC(db->ensure_positions((size_t)db->P + ns));
    RC(db->grow(db->tmp, 4 * ns, 0, 0));
    HIPCHK(db->up(db->tmp.p, slot, 4 * ns));
    launch_bowdb_add(db->dev(), n, (int*)db->tmp.p, db->P, db->st());
    HIPCHK(hipGetLastError());
    for (int i = 0; i < n; ++i) { db->live[slot[i]] = 1; db->live_words += db->len[slot[i]]; }
    db->P += n; db->live_count += n;
    if (db->P - db->base > db->o.tail_limit) {
      HIPCHK(hipStreamSynchronize(db->st()));                           // the rebuild may reallocate the scratch the add reads
      RC(db->rebuild());
    }
    return COVGPU_OK;
  });
}

extern "C" int covgpu_bowdb_erase(covgpu_bowdb* db, int32_t n, const int32_t* slot) {
  return db_entry("covgpu_bowdb_erase", db, [&](auto bad) -> int {
    if (const char* m = slots_check(n, slot, nullptr)) return bad(m);
    std::vector<int32_t> go;
    for (int i = 0; i < n; ++i) {
      const int s = slot[i];
      if ((size_t)s >= db->live.size() || !db->live[s]) continue;        // not in the index: nothing to do, as in the reference
      db->live[s] = 0; db->live_words -= db->len[s]; --db->live_count;
      go.push_back(s);
    }
    if (go.empty()) return COVGPU_OK;
    RC(db->grow(db->tmp, 4 * go.size(), 0, 0));
    HIPCHK(db->up(db->tmp.p, go.data(), 4 * go.size()));
    launch_bowdb_erase(db->dev(), (int)go.size(), (int*)db->tmp.p, db->st());
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(db->st()));                             // (go leaves scope)
    return COVGPU_OK;
  });
}

extern "C" int covgpu_bowdb_query(covgpu_bowdb* db, const covgpu_bowdb_query_t* q) {
  return db_entry("covgpu_bowdb_query", db, [&](auto bad) -> int {
    if (!q) return bad("NULL query");
    const int Q = q->num_queries, cap = q->cap, M = db->P;
    if (Q < 0 || cap < 0) return bad("negative count");
    if (Q == 0) return COVGPU_OK;
    if (!q->query_slot || !q->num_candidates) return bad("NULL query array");
    if (cap > 0 && !q->candidates) return bad("NULL candidates");
    if (q->con_ptr && q->con_ptr[0] != 0) return bad("con_ptr[0] != 0");
    int max_words = 0, hi = 0;
    for (int i = 0; i < Q; ++i) {
      const int s = q->query_slot[i];
      if (s < 0 || (size_t)s >= db->stored.size() || !db->stored[s]) return bad("a query slot has no stored vector");
      if (q->min_score_in && std::isnan(q->min_score_in[i])) return bad("min_score_in is NaN");
      if (q->con_ptr && q->con_ptr[i + 1] < q->con_ptr[i]) return bad("con_ptr not monotone");
      max_words = std::max(max_words, db->len[s]);
    }
    const size_t C = q->con_ptr ? (size_t)q->con_ptr[Q] : 0, Qs = (size_t)Q, caps = (size_t)cap;
    if (C > 0 && !q->con) return bad("NULL con");
    for (size_t i = 0; i < C; ++i) {
      if (q->con[i] < 0 || q->con[i] >= COVGPU_BOWDB_MAX_SLOTS) return bad("connected slot is not in 0..COVGPU_BOWDB_MAX_SLOTS-1");
      hi = std::max(hi, q->con[i] + 1);
    }
    // the reference minimum score: the pairs (query, connected keyframe that is not invalid), placerec_be.cpp:374-389
    std::vector<int32_t> pa, pb, poff(Qs + 1, 0), cptr, vis(Qs, M);
    if (!q->min_score_in) {
      pa.reserve(C); pb.reserve(C);
      for (int i = 0; i < Q; ++i) {
        for (int e = q->con_ptr ? q->con_ptr[i] : 0; e < (q->con_ptr ? q->con_ptr[i + 1] : 0); ++e) {
          const int k = q->con[e];
          if ((size_t)k < db->invalid.size() && db->invalid[k]) continue;
          if ((size_t)k >= db->stored.size() || !db->stored[k]) return bad("a connected slot has no stored vector and the minimum score needs it");
          pa.push_back(q->query_slot[i]); pb.push_back(k);
        }
        poff[i + 1] = (int32_t)pa.size();
      }
    }
    if (!q->con_ptr) cptr.assign(Qs + 1, 0);
    RC(db->ensure_slots((size_t)hi));                                    // (a connected slot the handle never saw has position -1)
    // per-query scratch is 28 B per position; queries run in chunks that keep it within the budget
    const size_t budget = (size_t)(db->o.detect.scratch_kib > 0 ? db->o.detect.scratch_kib : 65536) << 10;
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>(Qs, budget / (28 * std::max<size_t>(1, (size_t)M))));
    const size_t cm = (size_t)chunk * (size_t)M, NP = pa.size();
    const int hist_stride = max_words + 1;
    Carve cv;
    const size_t o_qs = cv.add(4 * Qs), o_vis = cv.add(4 * Qs), o_cp = cv.add(4 * (Qs + 1)), o_con = cv.add(4 * C), o_ms = cv.add(8 * Qs),
                 o_cnt = cv.add(16 * Qs), o_cand = cv.add(4 * Qs * caps), o_acc = cv.add(4 * Qs * caps), o_pa = cv.add(4 * NP), o_pb = cv.add(4 * NP),
                 o_po = cv.add(4 * (Qs + 1)), o_ps = cv.add(8 * NP), o_common = cv.add(4 * cm), o_first = cv.add(4 * cm), o_score = cv.add(8 * cm),
                 o_facc = cv.add(4 * cm), o_best = cv.add(4 * cm), o_order = cv.add(4 * cm), o_hist = cv.add(4 * (size_t)chunk * (size_t)hist_stride);
    RC(db->grow(db->tmp, cv.total, 0, 0));
    char* t = db->tmp.p;
    const BowDbDev B = db->dev();
    DetectDev D{};
    D.M = M; D.id = B.id; D.client = B.client; D.vec_beg = B.vec_beg; D.vec_end = B.vec_end; D.word = B.word; D.value = B.value;
    D.nb_beg = B.nb_beg; D.nb_end = B.nb_end; D.nb = B.nb;
    D.con_beg = (int*)(t + o_cp); D.con_end = D.con_beg + 1; D.con = (int*)(t + o_con); D.con_by_query = 1;
    D.db_order = B.db_order; D.pos_of = B.pos_of; D.dead = B.dead; D.tail = M - db->base;
    D.inv_words = db->num_words; D.inv_ptr = (int*)db->inv_ptr.p; D.inv_pos = (int*)db->inv_pos.p;
    D.query_kf = (int*)(t + o_qs); D.db_visible = (int*)(t + o_vis); D.min_score = (double*)(t + o_ms);
    int* counters = (int*)(t + o_cnt);
    D.max_common = counters; D.num_sharing = counters + Qs; D.num_scored = counters + 2 * Qs; D.num_candidates = counters + 3 * Qs;
    D.candidates = (int*)(t + o_cand); D.acc_score = (float*)(t + o_acc);
    HIPCHK(db->up(t + o_qs, q->query_slot, 4 * Qs)); HIPCHK(db->up(t + o_vis, vis.data(), 4 * Qs));
    HIPCHK(db->up(t + o_cp, q->con_ptr ? q->con_ptr : cptr.data(), 4 * (Qs + 1))); HIPCHK(db->up(t + o_con, q->con, 4 * C));
    HIPCHK(hipMemsetAsync(counters, 0, 16 * Qs, db->st()));
    if (cap > 0) { HIPCHK(hipMemsetAsync(D.candidates, 0xff, 4 * Qs * caps, db->st())); HIPCHK(hipMemsetAsync(D.acc_score, 0, 4 * Qs * caps, db->st())); }
    if (q->min_score_in) {
      HIPCHK(db->up(D.min_score, q->min_score_in, 8 * Qs));
    } else {
      HIPCHK(db->up(t + o_pa, pa.data(), 4 * NP)); HIPCHK(db->up(t + o_pb, pb.data(), 4 * NP)); HIPCHK(db->up(t + o_po, poff.data(), 4 * (Qs + 1)));
      launch_bow_score_pairs(D.vec_beg, D.vec_end, D.word, D.value, (int)NP, (int*)(t + o_pa), (int*)(t + o_pb), (double*)(t + o_ps), db->st());
      launch_bow_min_score(D, Q, (int*)(t + o_po), (double*)(t + o_ps), db->o.detect.min_score_factor, db->st());
    }
    const DetectOptsDev O{db->o.detect.min_loop_dist, db->o.detect.exclude_kfs_with_id_less_than, db->o.detect.inter_map_matches_only != 0};
    for (int q0 = 0; q0 < Q; q0 += chunk)
      launch_bow_detect_chunk(D, O, q0, std::min(chunk, Q - q0), cap, hist_stride, (int*)(t + o_common), (int*)(t + o_first), (double*)(t + o_score),
                              (float*)(t + o_facc), (int*)(t + o_best), (int*)(t + o_order), (int*)(t + o_hist), db->st());
    HIPCHK(hipGetLastError());
    HIPCHK(db->down(q->num_candidates, D.num_candidates, 4 * Qs)); HIPCHK(db->down(q->max_common_words, D.max_common, 4 * Qs));
    HIPCHK(db->down(q->num_sharing, D.num_sharing, 4 * Qs)); HIPCHK(db->down(q->num_scored, D.num_scored, 4 * Qs));
    HIPCHK(db->down(q->min_score, D.min_score, 8 * Qs));
    HIPCHK(db->down(q->candidates, D.candidates, 4 * Qs * caps)); HIPCHK(db->down(q->acc_score, D.acc_score, 4 * Qs * caps));
    HIPCHK(hipStreamSynchronize(db->st()));                             // (the pair lists leave scope)
    return COVGPU_OK;
  });
}

extern "C" int covgpu_bowdb_compact(covgpu_bowdb* db) {
  return db_entry("covgpu_bowdb_compact", db, [&](auto) -> int { return db->rebuild(); });
}

extern "C" int covgpu_bowdb_order(covgpu_bowdb* db, int32_t capacity, int32_t* slots, int32_t* count) {
  return db_entry("covgpu_bowdb_order", db, [&](auto bad) -> int {
    if (capacity < 0 || (capacity > 0 && !slots)) return bad("negative capacity or NULL slots");
    const size_t P = (size_t)db->P;
    std::vector<int32_t> ord(P);
    std::vector<uint8_t> dead(P);
    HIPCHK(db->down(ord.data(), db->order.p, 4 * P)); HIPCHK(db->down(dead.data(), db->dead.p, P));
    HIPCHK(hipStreamSynchronize(db->st()));
    int n = 0;
    for (size_t p = 0; p < P; ++p) {
      if (dead[p]) continue;
      if (n < capacity) slots[n] = ord[p];
      ++n;
    }
    if (count) *count = n;
    return COVGPU_OK;
  });
}

extern "C" int covgpu_bowdb_stats(covgpu_bowdb* db, int64_t out[16]) {
  if (!db || !out) { g_err = "covgpu_bowdb_stats: NULL handle or output"; return COVGPU_ERR_INVALID_ARG; }
  const int64_t v[16] = {db->stored_count, db->live_count, db->P, db->base_postings, db->P - db->base, db->rebuilds, db->h2d, db->d2h,
                         db->dev_bytes, db->pool_used, db->pool_dead, (int64_t)db->slot_cap, (int64_t)db->pos_cap, (int64_t)db->pool_cap,
                         db->growths, 0};
  std::memcpy(out, v, sizeof v);
  return COVGPU_OK;
}
