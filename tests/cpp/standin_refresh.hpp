// standin_refresh.hpp — stand-ins for what Landmark::ComputeDescriptor (landmark_be.cpp:49-92) and Landmark::UpdateNormal (:185-220)
// touch: keyframes with descriptors_ (32-byte rows), keypoints_aors_ and GetPoseTwc(), landmarks with an observation list, a reference
// keyframe, a world position and the four derived members (descriptor_, normal_, min_distance_, max_distance_), protected as in
// LandmarkBase and written through the traits LandmarkRefreshT asks for. The observation list is a vector here so that a test fixes the
// order the reference leaves to the allocator (its std::map is keyed by shared_ptr address, typedefs_base.hpp:187).
// LandmarkRefreshT of include/covins_gpu/optimization_gpu.hpp is compiled on these by tests/cpp/facade_refresh_shim.cpp.
#pragma once
#include <array>
#include <cstdint>
#include <cstring>
#include <map>
#include <memory>
#include <utility>
#include <vector>

#include "standin_map.hpp"

namespace standin_refresh {

using standin::idpair;
using standin::Mat4;
using standin::Vec3;
class Keyframe;
class Landmark;
using KeyframePtr = std::shared_ptr<Keyframe>;
using LandmarkPtr = std::shared_ptr<Landmark>;

struct DescMat {   // the two fields of cv::Mat the facade reads
  int rows = 0;
  uint8_t* data = nullptr;
};

class Keyframe {
 public:
  idpair id_;
  DescMat descriptors_, descriptors_add_;
  std::vector<uint8_t> desc_store_;                    // what descriptors_.data points to
  std::vector<std::array<float, 4>> keypoints_aors_;   // angle, octave, response, size
  bool IsInvalid() const { return invalid_; }
  void MarkInvalid() { invalid_ = true; }
  Mat4 GetPoseTwc() const { return T_w_c_; }
  void SetCenter(const double* c) { for (int i = 0; i < 3; ++i) T_w_c_(i, 3) = c[i]; }

 private:
  bool invalid_ = false;
  Mat4 T_w_c_;
};

class Landmark {
 public:
  using KfObservations = std::vector<std::pair<KeyframePtr, size_t>>;
  idpair id_;
  bool IsInvalid() const { return invalid_; }
  void MarkInvalid() { invalid_ = true; }
  Vec3 GetWorldPos() const { return pos_w_; }
  void SetWorldPos(Vec3 p) { pos_w_ = p; }
  KfObservations GetObservations() const { return observations_; }
  void AddObservation(KeyframePtr kf, size_t idx) { observations_.emplace_back(kf, idx); }
  KeyframePtr GetReferenceKeyframe() const { return ref_.lock(); }
  void SetReferenceKeyframe(KeyframePtr kf) { ref_ = kf; }

 protected:
  friend struct Types;
  bool has_descriptor_ = false;
  uint8_t descriptor_[32] = {};
  Vec3 normal_;
  double min_distance_ = 0.0, max_distance_ = 0.0;

 private:
  bool invalid_ = false;
  Vec3 pos_w_;
  KfObservations observations_;
  std::weak_ptr<Keyframe> ref_;
};

class Map {
 public:
  std::map<idpair, KeyframePtr> keyframes_;
  std::map<idpair, LandmarkPtr> landmarks_;
  std::vector<KeyframePtr> GetKeyframesVec() const { std::vector<KeyframePtr> v; for (auto& p : keyframes_) v.push_back(p.second); return v; }
  std::vector<LandmarkPtr> GetLandmarksVec() const { std::vector<LandmarkPtr> v; for (auto& p : landmarks_) v.push_back(p.second); return v; }
};

struct Types {
  using Map = standin_refresh::Map;
  using Keyframe = standin_refresh::Keyframe;
  using Landmark = standin_refresh::Landmark;
  using TransformType = Mat4;
  using Vector3Type = Vec3;
  // what a binding supplies because LandmarkBase keeps the members protected
  static void set_landmark_descriptor(Landmark& lm, const uint8_t* d) { std::memcpy(lm.descriptor_, d, 32); lm.has_descriptor_ = true; }
  static void set_landmark_scale(Landmark& lm, const double* n, double mn, double mx) {
    for (int i = 0; i < 3; ++i) lm.normal_[i] = n[i];
    lm.min_distance_ = mn; lm.max_distance_ = mx;
  }
  static bool landmark_descriptor(const Landmark& lm, uint8_t* out) { if (lm.has_descriptor_) std::memcpy(out, lm.descriptor_, 32); return lm.has_descriptor_; }
  static void landmark_scale(const Landmark& lm, double* n, double* mn, double* mx) {
    for (int i = 0; i < 3; ++i) n[i] = lm.normal_[i];
    *mn = lm.min_distance_; *mx = lm.max_distance_;
  }
};

}  // namespace standin_refresh
