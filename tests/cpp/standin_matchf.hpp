// standin_matchf.hpp — keyframe and landmark classes shaped like COVINS's for the facade's float (SIFT) descriptor matching
// (LoopMatcherT::MatchImagesFloatBatch / MatchImagePairsBatch, include/covins_gpu/optimization_gpu.hpp), with NO traits: the
// descriptors are cv::Mat-shaped members, descriptors_add_ holding CV_32F rows of `cols` floats (feat.type SIFT) or CV_8U rows of 32
// bytes (feat.type ORB), and every keyframe knows its predecessor, which RelNonCentralPosSolver::findMatches walks.
#pragma once
#include <cstdint>
#include <memory>
#include <vector>

namespace standinf {

constexpr int kCv8U = 0, kCv32F = 5;   // CV_8UC1, CV_32FC1

struct Mat {   // the members of cv::Mat the facade reads
  int rows = 0, cols = 0;
  unsigned char* data = nullptr;
  int type_ = kCv8U;
  bool continuous_ = true;
  int type() const { return type_; }
  bool isContinuous() const { return continuous_; }
};
struct Mat4 { double m[16]; double& operator()(int r, int c) { return m[4 * r + c]; } };
struct Vec3 { double v[3]; double& operator[](int i) { return v[i]; } };

class Landmark {
 public:
  bool IsInvalid() { return false; }
};
using LandmarkPtr = std::shared_ptr<Landmark>;

class Keyframe {
 public:
  LandmarkPtr GetLandmark(int) { return LandmarkPtr(); }
  std::shared_ptr<Keyframe> GetPredecessor() { return pred_.lock(); }
  Mat descriptors_, descriptors_add_;
  std::weak_ptr<Keyframe> pred_;
  std::vector<unsigned char> store_;
};
using KeyframePtr = std::shared_ptr<Keyframe>;
class Map;

struct Types {   // no descriptors / descriptors_f32 / landmark traits
  using Map = standinf::Map;
  using Keyframe = standinf::Keyframe;
  using Landmark = standinf::Landmark;
  using TransformType = Mat4;
  using Vector3Type = Vec3;
};

}  // namespace standinf
