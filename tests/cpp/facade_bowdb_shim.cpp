// facade_bowdb_shim.cpp — the C++ facade's resident keyframe database (ResidentKeyframeDatabaseT, include/covins_gpu/
// optimization_gpu.hpp) on the stand-in map. The optional traits, their tables and the entry points that fill them
// (bow_set_keyframe, bow_set_vocab, bow_get, ...) are facade_bow_shim.cpp's, compiled into this library as they are.
#include "facade_bow_shim.cpp"

namespace {
using Resident = covins_gpu::ResidentKeyframeDatabaseT<BowTypes>;
}  // namespace

extern "C" {

// The arrival of keyframes 0 .. n-1 in turn: ComputeBoW, one query with min_score[q] against the resident database and the same query
// against KeyframeDatabaseT, AddKeyframe on both, then EraseKeyframe of erase[erase_ptr[q] .. erase_ptr[q+1]) on both. Per query the
// candidates (map indices) and accScores of the resident database and the candidates of the stateless one; order_out receives the live
// keyframes at the end (read back from the device). Returns their number, or -1 if the two forms disagree on the database size.
int bowdb_replay(Handle* h, int track, int tail_limit, int min_loop_dist, int n, const double* min_score, const int* erase_ptr,
                 const int* erase, int cap, int* counts, int* cands, float* acc, int* counts_stateless, int* cands_stateless,
                 int* order_out, int64_t* stats) {
  Resident db(&g_voc);
  db.track_connections = track != 0;
  db.options().tail_limit = tail_limit;
  db.options().detect.min_loop_dist = min_loop_dist;
  Database plain;
  plain.options().min_loop_dist = min_loop_dist;
  for (int q = 0; q < n; ++q) {
    const KeyframePtr kf = h->kfs[q];
    db.ComputeBoW({kf});
    std::vector<Resident::Query> qs(1);
    qs[0].kf = kf; qs[0].has_min_score = true; qs[0].min_score = min_score[q];
    db.DetectCandidatesBatch(qs);
    counts[q] = (int)qs[0].candidates.size();
    for (int i = 0; i < counts[q] && i < cap; ++i) { cands[q * cap + i] = g_index[qs[0].candidates[i].get()]; acc[q * cap + i] = qs[0].acc_score[i]; }
    const auto c = plain.DetectCandidates(kf, min_score[q]);
    counts_stateless[q] = (int)c.size();
    for (size_t i = 0; i < c.size() && (int)i < cap; ++i) cands_stateless[q * cap + i] = g_index[c[i].get()];
    db.AddKeyframe(kf); plain.AddKeyframe(kf);
    for (int e = erase_ptr[q]; e < erase_ptr[q + 1]; ++e) { db.EraseKeyframe(h->kfs[erase[e]]); plain.EraseKeyframe(h->kfs[erase[e]]); }
  }
  const auto order = db.Order();
  for (size_t i = 0; i < order.size(); ++i) order_out[i] = g_index[order[i].get()];
  db.Stats(stats);
  return db.size() == plain.size() && order.size() == db.size() ? (int)order.size() : -1;
}

// ComputeBoW of every keyframe in one call, AddKeyframe(order[0..n)), then one DetectCandidatesBatch; min_score NULL = the reference
// score, whose neighbours' vectors are already resident.
void bowdb_detect(Handle* h, int mode, int min_loop_dist, int num_kf, int n, const int* order, int nq, const int* query,
                  const double* min_score, int cap, int* counts, int* cands, float* acc, double* min_score_out) {
  Resident db(&g_voc, mode);
  db.options().detect.min_loop_dist = min_loop_dist;
  std::vector<KeyframePtr> all(h->kfs.begin(), h->kfs.begin() + num_kf);
  db.ComputeBoW(all);
  for (int i = 0; i < n; ++i) db.AddKeyframe(h->kfs[order[i]]);
  std::vector<Resident::Query> qs(nq);
  for (int q = 0; q < nq; ++q) {
    qs[q].kf = h->kfs[query[q]];
    qs[q].has_min_score = min_score != nullptr; qs[q].min_score = min_score ? min_score[q] : 0.0;
  }
  db.DetectCandidatesBatch(qs);
  for (int q = 0; q < nq; ++q) {
    counts[q] = (int)qs[q].candidates.size(); min_score_out[q] = qs[q].min_score;
    for (int i = 0; i < counts[q] && i < cap; ++i) { cands[q * cap + i] = g_index[qs[q].candidates[i].get()]; acc[q * cap + i] = qs[q].acc_score[i]; }
  }
}

}  // extern "C"
