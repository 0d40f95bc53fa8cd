// facade_match_shim.cpp — the C++ facade's batched descriptor matcher (LoopMatcherT, include/covins_gpu/optimization_gpu.hpp) on the
// stand-in map, which has no descriptors: the OPTIONAL traits supply them (descriptors_ / descriptors_add_ rows of 32 bytes per
// keyframe) and the landmark of every row (what KeyframeBase::GetLandmark returns in COVINS). The stand-in map and its entry points
// (shim_build, ...) are facade_shim.cpp's, compiled into this library as they are.
#include <array>
#include <cstdint>
#include <unordered_map>
#include <vector>

#include "facade_shim.cpp"

namespace {
struct Rows {
  std::vector<uint8_t> desc[2];
  std::vector<LandmarkPtr> lm;
};
std::unordered_map<const standin::Keyframe*, Rows> g_rows;

struct MatchTypes : standin::Types {
  static bool descriptors(const standin::Keyframe& kf, int which, int* rows, const uint8_t** data) {
    auto it = g_rows.find(&kf);
    if (it == g_rows.end()) return false;
    *rows = (int)(it->second.desc[which].size() / 32);
    *data = it->second.desc[which].data();
    return true;
  }
  static LandmarkPtr landmark(const standin::Keyframe& kf, size_t k) {
    auto it = g_rows.find(&kf);
    return it == g_rows.end() || k >= it->second.lm.size() ? LandmarkPtr() : it->second.lm[k];
  }
};
using Matcher = covins_gpu::LoopMatcherT<MatchTypes>;
}  // namespace

extern "C" {

// rows of keyframe kf: n descriptors of set `which` (0: descriptors_, 1: descriptors_add_); for which = 0 also the landmark of every
// row: row_lm[k] = map landmark index, -1 = none, -2 = an invalid landmark of its own
void match_set_descriptors(Handle* h, int kf, int which, int n, const uint8_t* desc, int with_lm, const int* row_lm) {
  Rows& r = g_rows[h->kfs[kf].get()];
  r.desc[which].assign(desc, desc + 32 * (size_t)n);
  if (!with_lm) return;
  r.lm.assign(n, LandmarkPtr());
  for (int k = 0; k < n; ++k) {
    if (row_lm[k] >= 0) {
      r.lm[k] = h->lms[row_lm[k]];
    } else if (row_lm[k] == -2) {
      r.lm[k] = std::make_shared<standin::Landmark>();
      r.lm[k]->SetInvalid();
    }
  }
}

// query kf against candidates cand[0..n): mode 0 = MatchLandmarksBatch (default threshold), 1 = MatchImagesBatch (defaults). Writes
// the concatenated match lists as (idxA, idxB, distance) triples and per candidate the list length; returns the total.
int match_candidates(Handle* h, int kf, int n, const int* cand, int mode, int* counts, int* triples, int* cap) {
  std::vector<KeyframePtr> c;
  for (int i = 0; i < n; ++i) c.push_back(h->kfs[cand[i]]);
  const auto res = mode == 0 ? Matcher::MatchLandmarksBatch(h->kfs[kf], c) : Matcher::MatchImagesBatch(h->kfs[kf], c);
  int total = 0;
  for (int i = 0; i < n; ++i) {
    counts[i] = (int)res[i].size();
    for (const auto& m : res[i]) {
      if (total < *cap) { triples[3 * total] = (int)m.idxA; triples[3 * total + 1] = (int)m.idxB; triples[3 * total + 2] = (int)m.distance; }
      ++total;
    }
  }
  *cap = total;
  return total;
}

}  // extern "C"
