// facade_bow_shim.cpp — the C++ facade's bag-of-words retrieval (KeyframeDatabaseT, include/covins_gpu/optimization_gpu.hpp) on the
// stand-in map, which has neither descriptors, bow vectors nor a covisibility graph: the OPTIONAL traits supply them from tables the
// test fills. The stand-in map and its entry points (shim_build, ...) are facade_shim.cpp's, compiled into this library as they are.
#include <cstdint>
#include <map>
#include <unordered_map>
#include <vector>

#include "facade_shim.cpp"

namespace {
struct Extra {
  std::vector<uint8_t> desc;
  std::map<unsigned, double> bow_vec;                       // DBoW2::BowVector
  std::map<unsigned, std::vector<unsigned>> feat_vec;       // DBoW2::FeatureVector
  std::vector<KeyframePtr> connected;
};
std::unordered_map<const standin::Keyframe*, Extra> g_extra;
std::unordered_map<const standin::Keyframe*, int> g_index;
covins_gpu::BowVocabulary g_voc;

struct BowTypes : standin::Types {
  static bool descriptors(const standin::Keyframe& kf, int which, int* rows, const uint8_t** data) {
    if (which != 0) return false;
    Extra& e = g_extra[&kf];
    *rows = (int)(e.desc.size() / 32); *data = e.desc.data();
    return true;
  }
  template <class F> static void visit_bow(const standin::Keyframe& kf, F&& f) { for (const auto& e : g_extra[&kf].bow_vec) f((int32_t)e.first, e.second); }
  static void set_bow(const standin::Keyframe& kf, size_t n, const int32_t* word, const double* value) {
    auto& v = g_extra[&kf].bow_vec;
    v.clear();
    for (size_t i = 0; i < n; ++i) v[(unsigned)word[i]] = value[i];
  }
  static void set_features(const standin::Keyframe& kf, size_t rows, const int32_t* row_word, const int32_t* row_node) {
    auto& fv = g_extra[&kf].feat_vec;
    fv.clear();
    for (size_t i = 0; i < rows; ++i) if (row_word[i] >= 0) fv[(unsigned)row_node[i]].push_back((unsigned)i);
  }
  static std::vector<KeyframePtr> connected_keyframes(const standin::Keyframe& kf, bool) { return g_extra[&kf].connected; }
};
using Database = covins_gpu::KeyframeDatabaseT<BowTypes>;
}  // namespace

extern "C" {

void bow_set_keyframe(Handle* h, int kf, int n, const uint8_t* desc, int num_nb, const int* nb) {
  Extra& e = g_extra[h->kfs[kf].get()];
  g_index[h->kfs[kf].get()] = kf;
  e.desc.assign(desc, desc + 32 * (size_t)n);
  e.connected.clear();
  for (int i = 0; i < num_nb; ++i) e.connected.push_back(h->kfs[nb[i]]);
}

void bow_set_vocab(int k, int L, int scoring, int weighting, int num_nodes, int num_words, const int* parent, const int* child_ptr,
                   const int* child, const uint8_t* desc, const int* word_id, const double* weight) {
  g_voc.k = k; g_voc.L = L; g_voc.scoring = scoring; g_voc.weighting = weighting; g_voc.num_words = num_words;
  g_voc.parent.assign(parent, parent + num_nodes); g_voc.child_ptr.assign(child_ptr, child_ptr + num_nodes + 1);
  g_voc.child.assign(child, child + num_nodes - 1); g_voc.desc.assign(desc, desc + 32 * (size_t)num_nodes);
  g_voc.word_id.assign(word_id, word_id + num_nodes); g_voc.weight.assign(weight, weight + num_nodes);
}

void bow_compute(Handle* h, int n, const int* kfs, int levelsup) {
  std::vector<KeyframePtr> v;
  for (int i = 0; i < n; ++i) v.push_back(h->kfs[kfs[i]]);
  Database::ComputeBoWBatch(g_voc, v, levelsup);
}

// bow_vec_ of keyframe kf: returns its size; writes at most cap entries
int bow_get(Handle* h, int kf, int cap, int* word, double* value) {
  const auto& v = g_extra[h->kfs[kf].get()].bow_vec;
  int n = 0;
  for (const auto& e : v) { if (n < cap) { word[n] = (int)e.first; value[n] = e.second; } ++n; }
  return n;
}

// feat_vec_ of keyframe kf as the node of every row (-1: the row is in no entry); rows must be listed ascending within an entry
int bow_get_features(Handle* h, int kf, int rows, int* row_node) {
  for (int i = 0; i < rows; ++i) row_node[i] = -1;
  int ok = 1;
  for (const auto& e : g_extra[h->kfs[kf].get()].feat_vec)
    for (size_t i = 0; i < e.second.size(); ++i) {
      if ((int)e.second[i] >= rows || (i > 0 && e.second[i] <= e.second[i - 1])) { ok = 0; continue; }
      row_node[e.second[i]] = (int)e.first;
    }
  return ok;
}

// AddKeyframe(order[0..n)) then one DetectCandidatesBatch; min_score NULL = the reference score. Candidates come back as map indices.
void bow_detect(Handle* h, int mode, int min_loop_dist, int n, const int* order, int nq, const int* query, const int* visible,
                const double* min_score, int cap, int* counts, int* cands, float* acc, double* min_score_out) {
  Database db(mode);
  db.options().min_loop_dist = min_loop_dist;
  for (int i = 0; i < n; ++i) db.AddKeyframe(h->kfs[order[i]]);
  std::vector<Database::Query> qs(nq);
  for (int q = 0; q < nq; ++q) {
    qs[q].kf = h->kfs[query[q]]; qs[q].db_visible = (size_t)visible[q];
    qs[q].has_min_score = min_score != nullptr; qs[q].min_score = min_score ? min_score[q] : 0.0;
  }
  db.DetectCandidatesBatch(qs);
  for (int q = 0; q < nq; ++q) {
    counts[q] = (int)qs[q].candidates.size(); min_score_out[q] = qs[q].min_score;
    for (int i = 0; i < counts[q] && i < cap; ++i) { cands[q * cap + i] = g_index[qs[q].candidates[i].get()]; acc[q * cap + i] = qs[q].acc_score[i]; }
  }
}

// the reference's one-query form after AddKeyframe(order[0..n)) and EraseKeyframe(erase): returns the count
int bow_detect_one(Handle* h, int n, const int* order, int erase, int query, double min_score, int min_loop_dist, int cap, int* cands) {
  Database db;
  db.options().min_loop_dist = min_loop_dist;
  for (int i = 0; i < n; ++i) db.AddKeyframe(h->kfs[order[i]]);
  if (erase >= 0) db.EraseKeyframe(h->kfs[erase]);
  const auto c = db.DetectCandidates(h->kfs[query], min_score);
  for (size_t i = 0; i < c.size() && (int)i < cap; ++i) cands[i] = g_index[c[i].get()];
  return (int)c.size();
}

// ConsistencyFilter over a sequence of candidate lists: per query the enough-consistent candidates
void bow_consistency(Handle* h, int threshold, int nq, const int* counts, const int* cands, int* out_counts, int* out) {
  Database::ConsistencyFilter f(threshold);
  int at = 0, o = 0;
  for (int q = 0; q < nq; ++q) {
    std::vector<KeyframePtr> c;
    for (int i = 0; i < counts[q]; ++i) c.push_back(h->kfs[cands[at + i]]);
    at += counts[q];
    const auto e = f.Feed(c);
    out_counts[q] = (int)e.size();
    for (const auto& k : e) out[o++] = g_index[k.get()];
  }
}

// releases the calling thread's context of this binding (shim_shutdown releases the stand-in binding's)
void bow_shutdown() { covins_gpu::OptimizationT<BowTypes>::Shutdown(); }

}  // extern "C"
