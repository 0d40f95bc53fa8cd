// facade_ncrelpose_shim.cpp — the C++ facade's 17-point stage (RelPoseSolverT: computeNonCentralRelPose, ComputeNonCentralRelPoseBatch;
// include/covins_gpu/optimization_gpu.hpp) on a stand-in shaped like COVINS-G's keyframe, without traits: the classes
// of standin_fivept.hpp plus the extrinsics the stage reads. tests/test_gpu_ncrelpose_chain.py drives it.
#include <cstdint>
#include <cstring>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../include/covins_gpu/optimization_gpu.hpp"
#include "standin_fivept.hpp"

namespace standin17 {
using standin5::Landmark;
using standin5::LandmarkPtr;
using standin5::Mat;
using standin5::Mat4;
using standin5::Vec3;

class Keyframe {
 public:
  LandmarkPtr GetLandmark(int) { return LandmarkPtr(); }
  std::shared_ptr<Keyframe> GetPredecessor() { return pred_.lock(); }
  Mat4 GetPoseTwc() { return T_wc_; }
  Mat4 GetPoseTcw() { return T_cw_; }
  Mat4 GetStateExtrinsics() { return T_sc_; }
  std::pair<size_t, size_t> id_;
  Mat descriptors_, descriptors_add_;
  std::vector<Vec3> bearings_add_;
  std::weak_ptr<Keyframe> pred_;
  std::vector<unsigned char> store_;
  Mat4 T_wc_, T_cw_, T_sc_;
};
using KeyframePtr = std::shared_ptr<Keyframe>;
class Map;
struct Types {   // no traits
  using Map = standin17::Map;
  using Keyframe = standin17::Keyframe;
  using Landmark = standin17::Landmark;
  using TransformType = Mat4;
  using Vector3Type = Vec3;
};
struct Mat6 {
  double m[36];
  double& operator()(int r, int c) { return m[6 * r + c]; }
};
}  // namespace standin17

namespace {
using standin17::KeyframePtr;
using Solver = covins_gpu::RelPoseSolverT<standin17::Types>;
struct Handle { std::vector<KeyframePtr> kfs; };

Solver make_solver(int min_inliers5, int max_iter5, int min_img_matches, float img_thres, float ratio, const double* nc) {
  Solver solver(min_inliers5, 0.5, max_iter5, min_img_matches);
  solver.setMatchParams("ORB", img_thres, ratio);
  Solver::NonCentralParams p;
  p.rp_error = nc[0]; p.rp_error_cov = nc[1]; p.min_inliers = (int)nc[2]; p.max_iters = (int)nc[3]; p.cov_thres = nc[4]; p.cov_iters = (int)nc[5];
  p.cov_max_iters = (int)nc[6];
  solver.setNonCentralParams(p);
  return solver;
}
}  // namespace

extern "C" {

// as f5_build of facade_fivept_shim.cpp, plus the extrinsics T_sc[k] (row-major 4x4)
void* n17_build(int nk, const int* row_ptr, const unsigned char* desc, const double* bearing, const int* client, const int* pred, const double* T_wc,
                const double* T_cw, const double* T_sc) {
  auto* h = new Handle;
  for (int k = 0; k < nk; ++k) {
    auto kf = std::make_shared<standin17::Keyframe>();
    const int n = row_ptr[k + 1] - row_ptr[k];
    kf->store_.assign(desc + 32 * (size_t)row_ptr[k], desc + 32 * (size_t)row_ptr[k + 1]);
    kf->descriptors_add_.rows = n; kf->descriptors_add_.cols = 32; kf->descriptors_add_.data = kf->store_.data();
    kf->bearings_add_.resize(n);
    for (int i = 0; i < n; ++i) for (int c = 0; c < 3; ++c) kf->bearings_add_[i][c] = bearing[3 * ((size_t)row_ptr[k] + i) + c];
    kf->id_ = {(size_t)k, (size_t)client[k]};
    std::memcpy(kf->T_wc_.m, T_wc + 16 * k, sizeof(double) * 16);
    std::memcpy(kf->T_cw_.m, T_cw + 16 * k, sizeof(double) * 16);
    std::memcpy(kf->T_sc_.m, T_sc + 16 * k, sizeof(double) * 16);
    h->kfs.push_back(kf);
  }
  for (int k = 0; k < nk; ++k) if (pred[k] >= 0) h->kfs[k]->pred_ = h->kfs[pred[k]];
  return h;
}
void n17_free(void* h) { delete static_cast<Handle*>(h); }
void n17_shutdown() { covins_gpu::OptimizationT<standin17::Types>::Shutdown(); }

unsigned long long n17_seed(void* hv, int a, int b) {
  auto* h = static_cast<Handle*>(hv);
  return covins_gpu::detail::ncrelpose_seed(h->kfs[a].get(), h->kfs[b].get());
}

// ComputeNonCentralRelPoseBatch of query q against nc candidates; nc7 = rp_error, rp_error_cov, min_inliers, max_iters, cov_thres,
// cov_iters, cov_max_iters. Per candidate: found, status (-1: the grid ended early), inliers, Tc1c2 and Ts1s2 (row-major 4x4), cov (6x6).
void n17_batch(void* hv, int q, int nc, const int* cand, double threshold, int min_inliers5, int max_iter5, int min_img_matches, float img_thres,
               float ratio, const double* nc7, unsigned char* found, int* status, int* inliers, double* Tc16, double* Ts16, double* cov36) {
  auto* h = static_cast<Handle*>(hv);
  std::vector<KeyframePtr> c;
  for (int i = 0; i < nc; ++i) c.push_back(h->kfs[cand[i]]);
  const Solver solver = make_solver(min_inliers5, max_iter5, min_img_matches, img_thres, ratio, nc7);
  const std::vector<Solver::NonCentralResult> res = solver.ComputeNonCentralRelPoseBatch(h->kfs[q], c, threshold);
  for (int i = 0; i < nc; ++i) {
    found[i] = res[i].found ? 1 : 0; status[i] = res[i].status; inliers[i] = res[i].inliers;
    if (res[i].status == 0 || res[i].status >= 4) {
      std::memcpy(Tc16 + 16 * i, res[i].Tc1c2.m, sizeof(double) * 16);
      std::memcpy(Ts16 + 16 * i, res[i].Ts1s2.m, sizeof(double) * 16);
    }
    std::memcpy(cov36 + 36 * i, res[i].cov_loop, sizeof(double) * 36);
  }
}

// computeNonCentralRelPose with the reference's signature
int n17_single(void* hv, int q, int c, double threshold, int min_inliers5, int max_iter5, int min_img_matches, float img_thres, float ratio,
               const double* nc7, double* Tc16, double* cov36) {
  auto* h = static_cast<Handle*>(hv);
  const Solver solver = make_solver(min_inliers5, max_iter5, min_img_matches, img_thres, ratio, nc7);
  standin17::Mat4 T;
  std::memcpy(T.m, Tc16, sizeof(T.m));
  standin17::Mat6 cov;
  const bool ok = solver.computeNonCentralRelPose(h->kfs[q], h->kfs[c], threshold, T, cov);
  std::memcpy(Tc16, T.m, sizeof(T.m));
  std::memcpy(cov36, cov.m, sizeof(cov.m));
  return ok ? 1 : 0;
}

}  // extern "C"
