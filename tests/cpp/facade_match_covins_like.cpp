// facade_match_covins_like.cpp — the facade's LoopMatcherT on keyframe and landmark classes shaped like COVINS's, with NO traits:
// KeyframeBase::GetLandmark(int) and LandmarkBase::IsInvalid() are non-const there (keyframe_base.hpp:124, landmark_base.hpp), and
// the descriptors are the cv::Mat members descriptors_ / descriptors_add_, of which the facade reads rows and data. The explicit
// instantiation below must compile; match_covins_like() runs it (tests/test_gpu_match.py).
#include <cstdint>
#include <memory>
#include <vector>

#include "../../include/covins_gpu/optimization_gpu.hpp"

namespace covlike {

struct Mat {  // the two fields of cv::Mat the facade reads
  int rows = 0;
  unsigned char* data = nullptr;
};
struct Mat4 { double m[16]; double& operator()(int r, int c) { return m[4 * r + c]; } };
struct Vec3 { double v[3]; double& operator[](int i) { return v[i]; } };

class Landmark {
 public:
  bool IsInvalid() { return invalid_; }      // non-const, as LandmarkBase's
  bool invalid_ = false;
};
using LandmarkPtr = std::shared_ptr<Landmark>;

class Keyframe {
 public:
  LandmarkPtr GetLandmark(int index) { return index < (int)landmarks_.size() ? landmarks_[index] : LandmarkPtr(); }   // non-const
  Mat descriptors_, descriptors_add_;
  std::vector<LandmarkPtr> landmarks_;
  std::vector<unsigned char> store_[2];
};
using KeyframePtr = std::shared_ptr<Keyframe>;
class Map;

struct Types {   // no descriptors / landmark traits
  using Map = covlike::Map;
  using Keyframe = covlike::Keyframe;
  using Landmark = covlike::Landmark;
  using TransformType = Mat4;
  using Vector3Type = Vec3;
};

}  // namespace covlike

template class covins_gpu::LoopMatcherT<covlike::Types>;

extern "C" {

// nk keyframes, keyframe k owning rows [row_ptr[k], row_ptr[k+1]) of desc (both descriptors_ and descriptors_add_) with landmark
// state lm[r] (0 = none, 1 = valid, 2 = invalid). Query 0 against keyframes 1..nk-1; mode 0 = MatchLandmarksBatch, 1 =
// MatchImagesBatch. Writes (idxA, idxB, distance) triples up to *cap and per candidate the list length; returns the total.
int match_covins_like(int nk, const int* row_ptr, const unsigned char* desc, const unsigned char* lm, int mode, int* counts, int* triples,
                      int* cap) {
  std::vector<covlike::KeyframePtr> kfs;
  for (int k = 0; k < nk; ++k) {
    auto kf = std::make_shared<covlike::Keyframe>();
    const int n = row_ptr[k + 1] - row_ptr[k];
    for (int w = 0; w < 2; ++w) {
      kf->store_[w].assign(desc + 32 * (size_t)row_ptr[k], desc + 32 * (size_t)row_ptr[k + 1]);
      covlike::Mat& M = w == 0 ? kf->descriptors_ : kf->descriptors_add_;
      M.rows = n; M.data = kf->store_[w].data();
    }
    for (int r = 0; r < n; ++r) {
      const unsigned char s = lm[row_ptr[k] + r];
      kf->landmarks_.push_back(s == 0 ? covlike::LandmarkPtr() : std::make_shared<covlike::Landmark>());
      if (s == 2) kf->landmarks_.back()->invalid_ = true;
    }
    kfs.push_back(kf);
  }
  using Matcher = covins_gpu::LoopMatcherT<covlike::Types>;
  const std::vector<covlike::KeyframePtr> cands(kfs.begin() + 1, kfs.end());
  const auto res = mode == 0 ? Matcher::MatchLandmarksBatch(kfs[0], cands) : Matcher::MatchImagesBatch(kfs[0], cands);
  int total = 0;
  for (size_t i = 0; i < res.size(); ++i) {
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
