// facade_bow_covins_like.cpp — the facade's KeyframeDatabaseT on a keyframe class shaped like COVINS's, with NO traits: bow_vec_ is a
// DBoW2::BowVector (std::map<WordId, WordValue>), feat_vec_ a DBoW2::FeatureVector (std::map<NodeId, std::vector<unsigned>>),
// descriptors_ a cv::Mat of which the facade reads rows and data, and GetConnectedKeyframesByWeight / GetConnectedNeighborKeyframes /
// IsInvalid are non-const members (keyframe_be.hpp, keyframe_base.hpp). The explicit instantiation below must compile
// (tests/test_bow_host.py).
#include <cstdint>
#include <map>
#include <memory>
#include <utility>
#include <vector>

#include "../../include/covins_gpu/optimization_gpu.hpp"

namespace covlike {

struct Mat { int rows = 0; unsigned char* data = nullptr; };
struct Mat4 { double m[16]; double& operator()(int r, int c) { return m[4 * r + c]; } };
struct Vec3 { double v[3]; double& operator[](int i) { return v[i]; } };

class Keyframe;
using KeyframePtr = std::shared_ptr<Keyframe>;
class Keyframe {
 public:
  std::pair<size_t, size_t> id_;
  std::map<unsigned int, double> bow_vec_;
  std::map<unsigned int, std::vector<unsigned int>> feat_vec_;
  Mat descriptors_, descriptors_add_;
  bool IsInvalid() { return false; }
  std::vector<KeyframePtr> GetConnectedKeyframesByWeight(int) { return connected_; }
  std::vector<KeyframePtr> GetConnectedNeighborKeyframes() { return connected_; }
  std::vector<KeyframePtr> connected_;
};
class Landmark;
class Map;

struct Types {   // no traits
  using Map = covlike::Map;
  using Keyframe = covlike::Keyframe;
  using Landmark = covlike::Landmark;
  using TransformType = Mat4;
  using Vector3Type = Vec3;
};

}  // namespace covlike

template class covins_gpu::KeyframeDatabaseT<covlike::Types>;

extern "C" int bow_covins_like_instantiated() { return 1; }
