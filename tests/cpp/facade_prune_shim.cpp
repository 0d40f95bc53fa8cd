// facade_prune_shim.cpp — C entry points for tests/test_gpu_prune.py and tools/prune_bench.py: MapPruneT of
// include/covins_gpu/optimization_gpu.hpp on the stand-in classes of standin_prune.hpp, and a plain serial restatement of the reference's
// loop (map_be.cpp:745-811) on the same classes: every round recomputes every remaining candidate's value as
// Keyframe::ComputeRedundancyValue does (keyframe_be.cpp:228-256: a double sum over the keyframe's landmarks, each asked for the size of
// its observation map), sorts all candidates and handles the first. It is the timing baseline and a second literal check. Two choices
// the reference leaves open are fixed here: std::stable_sort instead of std::sort, and a 0/0 value ranks last instead of being NaN.
// One thing favours the baseline: the reference copies every landmark's observation std::map under a mutex to take its size
// (GetObservations, landmark_base.cpp:84-87); the restatement reads the size in place, which is 40 times faster on the `small` map.
#include <chrono>

#include "../../include/covins_gpu/optimization_gpu.hpp"
#include "standin_prune.hpp"

using namespace standin_prune;
using Prune = covins_gpu::MapPruneT<Types>;

struct PruneHandle {
  std::shared_ptr<Map> map;
  DatabasePtr db;
  std::vector<KeyframePtr> kfs;   // table order of prune_build
  std::map<const Keyframe*, int> index;
};

namespace {

double redundancy_value(const Keyframe& kf) {
  double red_sum = 0, n_lms = 0;
  for (const auto& lm : kf.landmarks_) {
    if (!lm || lm->IsInvalid()) continue;
    const size_t n_obs = lm->NumObservations();
    if (n_obs < 2) continue;
    red_sum += n_obs == 2 ? 0.0 : n_obs == 3 ? 0.4 : n_obs == 4 ? 0.7 : n_obs == 5 ? 0.9 : 1.0;
    n_lms += 1.0;
  }
  return n_lms > 0 ? red_sum / n_lms : -1.0;
}

}  // namespace

extern "C" {

PruneHandle* prune_build(int K, const int* kf_id, const int* kf_client, const unsigned char* kf_invalid, const double* kf_time,
                         const unsigned char* kf_loop, const unsigned char* kf_not_erase, const int* pred, const int* succ,
                         const long* imu_ptr, const double* imu_samples, const double* imu_first, int L, const unsigned char* lm_invalid,
                         const int* lm_obs_ptr, const int* obs_kf) {
  PruneHandle* h = new PruneHandle();
  h->map = std::make_shared<Map>();
  h->db = std::make_shared<Database>();
  for (int k = 0; k < K; ++k) {
    auto kf = std::make_shared<Keyframe>();
    kf->id_ = {(size_t)kf_id[k], (size_t)kf_client[k]};
    kf->timestamp_ = kf_time[k]; kf->is_loop_kf_ = kf_loop[k]; kf->not_erase_ = kf_not_erase[k];
    if (kf_invalid[k]) kf->MarkInvalid();
    for (long s = imu_ptr[k]; s < imu_ptr[k + 1]; ++s) {
      std::array<double, 7> smp;
      for (int i = 0; i < 7; ++i) smp[i] = imu_samples[7 * s + i];
      kf->imu_.push_back(smp);
    }
    for (int i = 0; i < 3; ++i) { kf->acc0_[i] = imu_first[6 * k + i]; kf->gyr0_[i] = imu_first[6 * k + 3 + i]; }
    h->kfs.push_back(kf);
    h->index[kf.get()] = k;
    h->map->keyframes_[kf->id_] = kf;
  }
  for (int k = 0; k < K; ++k) {
    if (pred[k] >= 0) h->kfs[k]->pred_ = h->kfs[pred[k]];
    if (succ[k] >= 0) h->kfs[k]->succ_ = h->kfs[succ[k]];
  }
  for (int l = 0; l < L; ++l) {
    auto lm = std::make_shared<Landmark>();
    lm->id_ = {(size_t)l, 0};
    for (int o = lm_obs_ptr[l]; o < lm_obs_ptr[l + 1]; ++o) {
      KeyframePtr kf = h->kfs[obs_kf[o]];
      lm->AddObservation(kf, kf->landmarks_.size());
      kf->landmarks_.push_back(lm);
    }
    if (lm_invalid[l]) lm->SetInvalid();
    h->map->landmarks_[lm->id_] = lm;
  }
  return h;
}

void prune_free(PruneHandle* h) { delete h; }
void prune_shutdown() { covins_gpu::OptimizationT<Types>::Shutdown(); }

// Map::RemoveRedundantData through the facade; max_kfs < 0: the reference's numeric_limits<size_t>::max(). Returns the count; the rounds
// go to round_kf / round_action [K] as table indices of prune_build.
int prune_facade(PruneHandle* h, double th_red, int max_kfs, double max_time_dist, int* round_kf, int* round_action, int* num_rounds) {
  Prune::max_time_dist() = max_time_dist;
  const size_t n = max_kfs < 0 ? Prune::RemoveRedundantData(h->map, h->db, th_red)
                               : Prune::RemoveRedundantData(h->map, h->db, th_red, (size_t)max_kfs);
  const auto& rounds = Prune::last_rounds();
  *num_rounds = (int)rounds.size();
  for (size_t r = 0; r < rounds.size(); ++r) { round_kf[r] = h->index[rounds[r].kf.get()]; round_action[r] = rounds[r].action; }
  return (int)n;
}

// The serial restatement on the same classes. Returns the count; *ms is the wall time of the loop.
int prune_serial(PruneHandle* h, double th_red, int max_kfs, double max_time_dist, int* round_kf, int* round_action, int* num_rounds,
                 double* ms) {
  const auto t0 = std::chrono::steady_clock::now();
  Map& map = *h->map;
  map.Clean();
  std::vector<KeyframePtr> kfs;
  for (const auto& p : map.keyframes_) {
    const KeyframePtr& kf = p.second;
    if (kf->IsInvalid() || kf->id_.first == 0 || !kf->GetPredecessor() || !kf->GetSuccessor()) continue;
    kfs.push_back(kf);
  }
  int removed = 0, rounds = 0;
  std::vector<std::pair<double, KeyframePtr>> val;
  auto valid_kfs = [&] { size_t n = 0; for (const auto& p : map.keyframes_) n += !p.second->IsInvalid(); return n; };
  size_t valid = valid_kfs();
  while (!kfs.empty() && (max_kfs < 0 || valid > (size_t)max_kfs)) {
    val.clear();
    for (const auto& kf : kfs) val.emplace_back(redundancy_value(*kf), kf);
    std::stable_sort(val.begin(), val.end(), [](const auto& a, const auto& b) { return a.first > b.first; });
    for (size_t i = 0; i < kfs.size(); ++i) kfs[i] = val[i].second;
    if (max_kfs < 0 && !(val[0].first >= th_red)) break;
    const KeyframePtr kf = kfs[0];
    int action = 0;
    if (kf->GetSuccessor()->timestamp_ - kf->GetPredecessor()->timestamp_ >= max_time_dist) action = 1;
    else if (kf->is_loop_kf_) action = 2;
    else if (kf->not_erase_) action = 3;
    if (action == 0 || action == 3) {
      if (map.EraseKeyframeWithDatabase(kf, false, h->db)) --valid;
      ++removed;
    }
    round_kf[rounds] = h->index[kf.get()]; round_action[rounds] = action; ++rounds;
    kfs.erase(kfs.begin());
  }
  *num_rounds = rounds;
  *ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return removed;
}

// the map as the erases left it, in the table order of prune_build
void prune_state(PruneHandle* h, unsigned char* invalid, int* pred, int* succ, int* imu_count, double* imu_dt_sum, double* imu_first,
                 int* num_landmarks, int* db_erased) {
  for (size_t k = 0; k < h->kfs.size(); ++k) {
    const Keyframe& kf = *h->kfs[k];
    invalid[k] = kf.IsInvalid();
    auto idx = [&](const KeyframePtr& p) { return p ? h->index[p.get()] : -1; };
    pred[k] = idx(kf.GetPredecessor()); succ[k] = idx(kf.GetSuccessor());
    imu_count[k] = (int)kf.imu_.size();
    double s = 0;
    for (const auto& smp : kf.imu_) s += smp[0];
    imu_dt_sum[k] = s;
    for (int i = 0; i < 3; ++i) { imu_first[6 * k + i] = kf.acc0_[i]; imu_first[6 * k + 3 + i] = kf.gyr0_[i]; }
    num_landmarks[k] = (int)kf.landmarks_.size();
  }
  *db_erased = (int)h->db->erased.size();
}

}  // extern "C"
