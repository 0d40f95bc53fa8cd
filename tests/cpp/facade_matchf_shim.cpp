// facade_matchf_shim.cpp — the C++ facade's float (SIFT) descriptor matching and its pair-list entry point (LoopMatcherT::
// MatchImagesFloatBatch / MatchImagePairsBatch, include/covins_gpu/optimization_gpu.hpp) on the COVINS-shaped classes of
// standin_matchf.hpp, without traits: the facade reads descriptors_add_ as a cv::Mat. tests/test_gpu_matchf.py drives it.
#include <cstdint>
#include <cstring>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../include/covins_gpu/optimization_gpu.hpp"
#include "standin_matchf.hpp"

namespace {
using standinf::KeyframePtr;
using Matcher = covins_gpu::LoopMatcherT<standinf::Types>;
struct Handle { std::vector<KeyframePtr> kfs; };

// the concatenated match lists as (idxA, idxB) and distances up to *cap, per list its length; returns the total
int emit(const std::vector<Matcher::Matches>& res, int* counts, int* idx, double* dist, int* cap) {
  int total = 0;
  for (size_t i = 0; i < res.size(); ++i) {
    counts[i] = (int)res[i].size();
    for (const auto& m : res[i]) {
      if (total < *cap) { idx[2 * total] = (int)m.idxA; idx[2 * total + 1] = (int)m.idxB; dist[total] = m.distance; }
      ++total;
    }
  }
  *cap = total;
  return total;
}
}  // namespace

template class covins_gpu::LoopMatcherT<standinf::Types>;   // the explicit instantiation compiles without the float path's members

extern "C" {

// nk keyframes; keyframe k owns rows [row_ptr[k], row_ptr[k+1]) of `data`, rows of `cols` elements of OpenCV type cv_type (5: float,
// 0: bytes), as its descriptors_add_; pred[k] = the index of its predecessor or -1.
void* mf_build(int nk, const int* row_ptr, int cols, int cv_type, const void* data, const int* pred) {
  auto* h = new Handle;
  const size_t row_bytes = (size_t)cols * (cv_type == standinf::kCv32F ? 4 : 1);
  for (int k = 0; k < nk; ++k) {
    auto kf = std::make_shared<standinf::Keyframe>();
    const int n = row_ptr[k + 1] - row_ptr[k];
    const unsigned char* src = static_cast<const unsigned char*>(data) + row_bytes * (size_t)row_ptr[k];
    kf->store_.assign(src, src + row_bytes * (size_t)n);
    kf->descriptors_add_.rows = n; kf->descriptors_add_.cols = cols; kf->descriptors_add_.type_ = cv_type;
    kf->descriptors_add_.data = kf->store_.data();
    h->kfs.push_back(kf);
  }
  for (int k = 0; k < nk; ++k) if (pred[k] >= 0) h->kfs[k]->pred_ = h->kfs[pred[k]];
  return h;
}
void mf_free(void* h) { delete static_cast<Handle*>(h); }
void mf_shutdown() { covins_gpu::OptimizationT<standinf::Types>::Shutdown(); }

// MatchImagesFloatBatch: query q against candidates cand[0..n)
int mf_match_float(void* hv, int q, int n, const int* cand, float thr, float ratio, int* counts, int* idx, double* dist, int* cap) {
  auto* h = static_cast<Handle*>(hv);
  std::vector<KeyframePtr> c;
  for (int i = 0; i < n; ++i) c.push_back(h->kfs[cand[i]]);
  return emit(Matcher::MatchImagesFloatBatch(h->kfs[q], c, thr, ratio), counts, idx, dist, cap);
}

// MatchImagesBatch (ORB): query q against candidates cand[0..n)
int mf_match_orb(void* hv, int q, int n, const int* cand, float thr, float ratio, int* counts, int* idx, double* dist, int* cap) {
  auto* h = static_cast<Handle*>(hv);
  std::vector<KeyframePtr> c;
  for (int i = 0; i < n; ++i) c.push_back(h->kfs[cand[i]]);
  return emit(Matcher::MatchImagesBatch(h->kfs[q], c, thr, ratio), counts, idx, dist, cap);
}

// MatchImagePairsBatch on findMatches' grid (RelNonCentralPosSolver.cpp:82-144): the query keyframe and its predecessors (nq keyframes
// in all) against the candidate and its predecessors (nc in all), query-major, in ONE call. pairs_out receives the keyframe indices.
int mf_match_grid(void* hv, int q, int c, int nq, int nc, const char* feature_type, float thr, float ratio, int* pairs_out, int* counts,
                  int* idx, double* dist, int* cap) {
  auto* h = static_cast<Handle*>(hv);
  auto index_of = [&](const KeyframePtr& kf) { for (size_t i = 0; i < h->kfs.size(); ++i) if (h->kfs[i] == kf) return (int)i; return -1; };
  std::vector<KeyframePtr> qs, cs;
  for (KeyframePtr k = h->kfs[q]; k && (int)qs.size() < nq; k = k->GetPredecessor()) qs.push_back(k);
  for (KeyframePtr k = h->kfs[c]; k && (int)cs.size() < nc; k = k->GetPredecessor()) cs.push_back(k);
  std::vector<std::pair<KeyframePtr, KeyframePtr>> pairs;
  for (const auto& a : qs) for (const auto& b : cs) {
    pairs_out[2 * pairs.size()] = index_of(a); pairs_out[2 * pairs.size() + 1] = index_of(b);
    pairs.emplace_back(a, b);
  }
  emit(Matcher::MatchImagePairsBatch(pairs, feature_type, thr, ratio), counts, idx, dist, cap);
  return (int)pairs.size();
}

}  // extern "C"
