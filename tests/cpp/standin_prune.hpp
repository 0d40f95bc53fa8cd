// standin_prune.hpp — stand-ins for what Map::RemoveRedundantData (map_be.cpp:745-811) touches beyond tests/cpp/standin_map.hpp: keyframes
// with timestamp_, is_loop_kf_ and not_erase_, a SetInvalid that relinks the chain and fuses the IMU buffers (keyframe_be.cpp:500-540,
// :413-440), and a map with EraseKeyframeWithDatabase (map_be.cpp:456-483). MapPruneT of include/covins_gpu/optimization_gpu.hpp is
// compiled on these by tests/cpp/facade_prune_shim.cpp.
#pragma once
#include <algorithm>

#include "standin_map.hpp"

namespace standin_prune {

using standin::idpair;
using standin::Mat4;
using standin::Vec3;
class Keyframe;
class Landmark;
using KeyframePtr = std::shared_ptr<Keyframe>;
using LandmarkPtr = std::shared_ptr<Landmark>;

class Landmark {
 public:
  using KfObservations = std::map<KeyframePtr, size_t>;   // ordered by pointer here; the facade reads no order from it
  idpair id_;
  bool IsInvalid() const { return invalid_; }
  void SetInvalid() { invalid_ = true; observations_.clear(); }
  KfObservations GetObservations() const { return observations_; }
  size_t NumObservations() const { return observations_.size(); }   // what the serial restatement asks; the reference copies the map for it
  void AddObservation(KeyframePtr kf, size_t idx) { observations_[kf] = idx; }
  void EraseObservation(KeyframePtr kf) { observations_.erase(kf); }

 private:
  bool invalid_ = false;
  KfObservations observations_;
};

class Keyframe : public std::enable_shared_from_this<Keyframe> {
 public:
  idpair id_;
  double timestamp_ = 0.0;
  bool is_loop_kf_ = false, not_erase_ = false;
  std::vector<LandmarkPtr> landmarks_;
  std::vector<std::array<double, 7>> imu_;  // dt, acc, gyr between the predecessor and this keyframe
  double acc0_[3] = {0, 0, 0}, gyr0_[3] = {0, 0, 0};
  std::weak_ptr<Keyframe> pred_, succ_;

  bool IsInvalid() const { return invalid_; }
  void MarkInvalid() { invalid_ = true; }   // (a keyframe that arrives invalid)
  KeyframePtr GetPredecessor() const { return pred_.lock(); }
  KeyframePtr GetSuccessor() const { return succ_.lock(); }
  // Keyframe::SetInvalid (keyframe_be.cpp:500-540)
  bool SetInvalid() {
    if (invalid_) return false;
    KeyframePtr p = pred_.lock(), s = succ_.lock();
    if (id_.first == 0 || !p || !s || not_erase_) return false;
    for (auto& lm : landmarks_) if (lm) lm->EraseObservation(shared_from_this());
    p->succ_ = s; s->pred_ = p;
    s->imu_.insert(s->imu_.begin(), imu_.begin(), imu_.end());   // FusePreintegration (:413-440): ours, then the successor's own
    std::copy(acc0_, acc0_ + 3, s->acc0_); std::copy(gyr0_, gyr0_ + 3, s->gyr0_);
    imu_.clear();
    landmarks_.clear();
    invalid_ = true;
    return true;
  }

 private:
  bool invalid_ = false;
};

struct Database {
  std::vector<KeyframePtr> erased;
  void EraseKeyframe(KeyframePtr kf) { erased.push_back(kf); }
};
using DatabasePtr = std::shared_ptr<Database>;

class Map {
 public:
  size_t id_map_ = 0;
  std::map<idpair, KeyframePtr> keyframes_, keyframes_erased_;
  std::map<idpair, LandmarkPtr> landmarks_;
  std::vector<KeyframePtr> GetKeyframesVec() const { std::vector<KeyframePtr> v; for (auto& p : keyframes_) v.push_back(p.second); return v; }
  std::vector<LandmarkPtr> GetLandmarksVec() const { std::vector<LandmarkPtr> v; for (auto& p : landmarks_) v.push_back(p.second); return v; }
  void Clean() {
    for (auto& p : landmarks_) if (!p.second->IsInvalid() && p.second->GetObservations().size() < 2) p.second->SetInvalid();
  }
  // Map::EraseKeyframe (map_be.cpp:456-475) + the database
  bool EraseKeyframeWithDatabase(KeyframePtr kf, bool, DatabasePtr database) {
    bool success = false;
    auto it = keyframes_.find(kf->id_);
    if (it != keyframes_.end() && kf->SetInvalid()) { keyframes_erased_[kf->id_] = kf; keyframes_.erase(it); success = true; }
    if (database) database->EraseKeyframe(kf);
    return success;
  }
};

struct Types {
  using Map = standin_prune::Map;
  using Keyframe = standin_prune::Keyframe;
  using Landmark = standin_prune::Landmark;
  using TransformType = Mat4;
  using Vector3Type = Vec3;
  static double timestamp(const Keyframe& kf) { return kf.timestamp_; }
  static bool is_loop_kf(const Keyframe& kf) { return kf.is_loop_kf_; }
  static bool not_erase(const Keyframe& kf) { return kf.not_erase_; }
};

}  // namespace standin_prune
