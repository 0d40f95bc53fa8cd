// facade_refresh_shim.cpp — C entry points for tests/test_lmrefresh_host.py, tests/test_gpu_lmrefresh.py and tools/lmrefresh_bench.py:
// LandmarkRefreshT of include/covins_gpu/optimization_gpu.hpp on the stand-in classes of standin_refresh.hpp, and a plain serial
// restatement of the reference's two member functions on the same classes, in their literal arithmetic: Landmark::ComputeDescriptor
// (landmark_be.cpp:49-92: a double matrix of pairwise Hamming distances, std::sort of a copy of every row, the element at index
// 0.5 * (n - 1), the first row whose median is `<` the best so far) and Landmark::UpdateNormal (:185-220: normal = normal + v / v.norm()
// over the valid observers, divided by their number; dist * pow(scale_factor, level), and that divided by pow(scale_factor,
// num_octaves - 1)). It iterates the observations in the stand-in's given order. It is the CPU check of tests/lmrefresh_ref.py and the
// timing baseline. Two things favour the baseline over the reference: it copies no observation map and takes no mutex.
// Where the reference exits or divides 0 by 0 the restatement reports the status bits of covgpu_landmark_refresh_t instead.
// Compiled with -ffp-contract=off: every double operation is rounded on its own.
#include <chrono>
#include <climits>

#include "../../include/covins_gpu/optimization_gpu.hpp"
#include "standin_refresh.hpp"

using namespace standin_refresh;
using Refresh = covins_gpu::LandmarkRefreshT<Types>;

struct RefreshHandle {
  std::shared_ptr<Map> map;
  std::vector<KeyframePtr> kfs;     // table order of refresh_build
  std::vector<LandmarkPtr> lms;
};

namespace {

int hamming256(const uint8_t* a, const uint8_t* b) {   // cv::norm(a, b, cv::NORM_HAMMING) of two 32-byte rows
  int d = 0;
  for (int i = 0; i < 32; ++i) d += __builtin_popcount((unsigned)(a[i] ^ b[i]));
  return d;
}

double norm3(const double* v) { return std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }   // Eigen's norm(): ((x x + y y) + z z)

}  // namespace

extern "C" {

// Keyframe k's descriptor matrix and keypoints hold one row per observation of it, in order of appearance (feature index = that order).
// lm_ref_obs: position of the reference keyframe's observation in the landmark's list, -1 = no reference keyframe.
RefreshHandle* refresh_build(int K, const unsigned char* kf_invalid, const double* kf_center, int L, const unsigned char* lm_invalid,
                             const double* lm_pos, const int* lm_ref_obs, const int* lm_obs_ptr, const int* obs_kf,
                             const unsigned char* obs_desc, const int* obs_octave) {
  RefreshHandle* h = new RefreshHandle();
  h->map = std::make_shared<Map>();
  for (int k = 0; k < K; ++k) {
    auto kf = std::make_shared<Keyframe>();
    kf->id_ = {(size_t)k, 0};
    if (kf_invalid[k]) kf->MarkInvalid();
    kf->SetCenter(kf_center + 3 * k);
    h->kfs.push_back(kf);
    h->map->keyframes_[kf->id_] = kf;
  }
  for (int l = 0; l < L; ++l) {
    auto lm = std::make_shared<Landmark>();
    lm->id_ = {(size_t)l, 0};
    Vec3 p; for (int i = 0; i < 3; ++i) p[i] = lm_pos[3 * l + i];
    lm->SetWorldPos(p);
    for (int o = lm_obs_ptr[l]; o < lm_obs_ptr[l + 1]; ++o) {
      Keyframe& kf = *h->kfs[obs_kf[o]];
      lm->AddObservation(h->kfs[obs_kf[o]], kf.keypoints_aors_.size());
      kf.keypoints_aors_.push_back({0.f, (float)obs_octave[o], 0.f, 0.f});
      kf.desc_store_.insert(kf.desc_store_.end(), obs_desc + 32 * (size_t)o, obs_desc + 32 * (size_t)o + 32);
    }
    if (lm_ref_obs[l] >= 0) lm->SetReferenceKeyframe(h->kfs[obs_kf[lm_obs_ptr[l] + lm_ref_obs[l]]]);
    if (lm_invalid[l]) lm->MarkInvalid();
    h->lms.push_back(lm);
    h->map->landmarks_[lm->id_] = lm;
  }
  for (auto& kf : h->kfs) { kf->descriptors_.rows = (int)kf->keypoints_aors_.size(); kf->descriptors_.data = kf->desc_store_.data(); }
  return h;
}

void refresh_free(RefreshHandle* h) { delete h; }
void refresh_shutdown() { covins_gpu::OptimizationT<Types>::Shutdown(); }

// Landmark::ComputeDescriptor + UpdateNormal of every landmark through the facade (one covgpu_landmark_refresh call); forms [6]
void refresh_facade(RefreshHandle* h, double scale_factor, int num_octaves, int* forms) {
  Refresh::params().scale_factor = scale_factor; Refresh::params().num_octaves = num_octaves;
  Refresh::Refresh(h->map);
  for (int f = 0; f < COVGPU_LMR_FORMS; ++f) forms[f] = Refresh::last_forms()[f];
}

// the landmarks' derived members as they are now
void refresh_state(RefreshHandle* h, unsigned char* has_desc, unsigned char* desc, double* normal, double* mind, double* maxd) {
  for (size_t l = 0; l < h->lms.size(); ++l) {
    has_desc[l] = Types::landmark_descriptor(*h->lms[l], desc + 32 * l);
    Types::landmark_scale(*h->lms[l], normal + 3 * l, mind + l, maxd + l);
  }
}

// The serial restatement, landmark by landmark; outputs as covgpu_landmark_refresh_t's. *ms is the wall time of the loop.
void refresh_serial(RefreshHandle* h, double scale_factor, int num_octaves, int* desc_obs, unsigned char* desc, double* normal,
                    double* mind, double* maxd, int* status, double* ms) {
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<const uint8_t*> cand;
  std::vector<int> cand_pos;
  std::vector<double> dm, row;
  for (size_t l = 0; l < h->lms.size(); ++l) {
    const Landmark& lm = *h->lms[l];
    desc_obs[l] = -1; status[l] = 0; mind[l] = maxd[l] = 0.0;
    std::fill(desc + 32 * l, desc + 32 * l + 32, 0);
    std::fill(normal + 3 * l, normal + 3 * l + 3, 0.0);
    if (lm.IsInvalid()) { status[l] = 4; continue; }
    const Landmark::KfObservations obs = lm.GetObservations();
    // ---- ComputeDescriptor
    cand.clear(); cand_pos.clear();
    for (size_t i = 0; i < obs.size(); ++i) {
      if (obs[i].first->IsInvalid()) continue;
      cand.push_back(obs[i].first->descriptors_.data + 32 * obs[i].second);
      cand_pos.push_back((int)i);
    }
    if (!cand.empty()) {
      const int num_desc = (int)cand.size();
      dm.assign((size_t)num_desc * num_desc, 0.0);
      for (int i = 0; i < num_desc; ++i) {
        dm[(size_t)i * num_desc + i] = 0;
        for (int j = i + 1; j < num_desc; ++j) {
          const double dist_ij = (double)hamming256(cand[i], cand[j]);
          dm[(size_t)i * num_desc + j] = dist_ij; dm[(size_t)j * num_desc + i] = dist_ij;
        }
      }
      double best_median = INT_MAX;
      int best_idx = -1;
      for (int i = 0; i < num_desc; ++i) {
        row.assign(dm.begin() + (size_t)i * num_desc, dm.begin() + (size_t)(i + 1) * num_desc);
        std::sort(row.begin(), row.end());
        const double median = row[0.5 * (num_desc - 1)];
        if (median < best_median) { best_median = median; best_idx = i; }
      }
      desc_obs[l] = cand_pos[best_idx];
      std::memcpy(desc + 32 * l, cand[best_idx], 32);
    }
    // ---- UpdateNormal
    double nrm[3] = {0.0, 0.0, 0.0};
    int n = 0;
    const Vec3 pw = lm.GetWorldPos();
    for (const auto& o : obs) {
      if (o.first->IsInvalid()) continue;
      const Mat4 T = o.first->GetPoseTwc();
      const double v[3] = {pw[0] - T(0, 3), pw[1] - T(1, 3), pw[2] - T(2, 3)};
      const double len = norm3(v);
      for (int i = 0; i < 3; ++i) nrm[i] = nrm[i] + v[i] / len;
      n++;
    }
    if (n == 0) status[l] |= 1;
    else for (int i = 0; i < 3; ++i) normal[3 * l + i] = nrm[i] / n;
    const KeyframePtr ref = lm.GetReferenceKeyframe();
    if (!ref) { status[l] |= 2; continue; }
    const Mat4 T = ref->GetPoseTwc();
    const double pc[3] = {pw[0] - T(0, 3), pw[1] - T(1, 3), pw[2] - T(2, 3)};
    const double dist = norm3(pc);
    size_t feat = 0;
    for (const auto& o : obs) if (o.first == ref) { feat = o.second; break; }   // observations_[reference_kf_]
    const int level = (int)ref->keypoints_aors_[feat][1];
    const double levelScaleFactor = std::pow(scale_factor, level);
    maxd[l] = dist * levelScaleFactor;
    mind[l] = maxd[l] / std::pow(scale_factor, num_octaves - 1);
  }
  *ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

}  // extern "C"
