// standin_fivept.hpp — keyframe and landmark classes shaped like COVINS-G's for the facade's five-point stage (RelPoseSolverT,
// include/covins_gpu/optimization_gpu.hpp), with NO traits: bearings_add_ holds one 3-vector per additional feature (not normalised:
// the facade normalises, as frame-relative-adapter.cpp does), descriptors_add_ is a cv::Mat-shaped matrix of 32-byte ORB rows, a
// keyframe knows its id, its predecessor and its pose.
#pragma once
#include <cstdint>
#include <memory>
#include <utility>
#include <vector>

namespace standin5 {

struct Mat {   // the members of cv::Mat the facade reads
  int rows = 0, cols = 0;
  unsigned char* data = nullptr;
  int type_ = 0;   // CV_8UC1
  int type() const { return type_; }
  bool isContinuous() const { return true; }
};
struct Mat4 {
  double m[16];
  double& operator()(int r, int c) { return m[4 * r + c]; }
  double operator()(int r, int c) const { return m[4 * r + c]; }
};
struct Vec3 {
  double v[3];
  double& operator[](int i) { return v[i]; }
  double operator[](int i) const { return v[i]; }
};

class Landmark {
 public:
  bool IsInvalid() { return false; }
};
using LandmarkPtr = std::shared_ptr<Landmark>;

class Keyframe {
 public:
  LandmarkPtr GetLandmark(int) { return LandmarkPtr(); }
  std::shared_ptr<Keyframe> GetPredecessor() { return pred_.lock(); }
  Mat4 GetPoseTwc() { return T_wc_; }
  Mat4 GetPoseTcw() { return T_cw_; }
  std::pair<size_t, size_t> id_;
  Mat descriptors_, descriptors_add_;
  std::vector<Vec3> bearings_add_;
  std::weak_ptr<Keyframe> pred_;
  std::vector<unsigned char> store_;
  Mat4 T_wc_, T_cw_;
};
using KeyframePtr = std::shared_ptr<Keyframe>;
class Map;

struct Types {   // no traits
  using Map = standin5::Map;
  using Keyframe = standin5::Keyframe;
  using Landmark = standin5::Landmark;
  using TransformType = Mat4;
  using Vector3Type = Vec3;
};

}  // namespace standin5
