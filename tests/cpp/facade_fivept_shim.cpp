// facade_fivept_shim.cpp — the C++ facade's five-point stage (RelPoseSolverT: computePose, ComputePoseGrid;
// include/covins_gpu/optimization_gpu.hpp) on the COVINS-G-shaped classes of standin_fivept.hpp, without traits.
// tests/test_gpu_fivept.py drives it and compares with the Python calls on the same flat data.
#include <cstdint>
#include <cstring>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../include/covins_gpu/optimization_gpu.hpp"
#include "standin_fivept.hpp"

namespace {
using standin5::KeyframePtr;
using Solver = covins_gpu::RelPoseSolverT<standin5::Types>;
struct Handle { std::vector<KeyframePtr> kfs; };
}  // namespace

extern "C" {

// nk keyframes: keyframe k owns rows [row_ptr[k], row_ptr[k+1]) of desc (32 bytes each) and of bearing (3 doubles each, any length),
// has id (k, client[k]), predecessor pred[k] (-1: none) and pose T_wc[k] (row-major 4x4; T_cw is given too).
void* f5_build(int nk, const int* row_ptr, const unsigned char* desc, const double* bearing, const int* client, const int* pred, const double* T_wc,
               const double* T_cw) {
  auto* h = new Handle;
  for (int k = 0; k < nk; ++k) {
    auto kf = std::make_shared<standin5::Keyframe>();
    const int n = row_ptr[k + 1] - row_ptr[k];
    kf->store_.assign(desc + 32 * (size_t)row_ptr[k], desc + 32 * (size_t)row_ptr[k + 1]);
    kf->descriptors_add_.rows = n; kf->descriptors_add_.cols = 32; kf->descriptors_add_.data = kf->store_.data();
    kf->bearings_add_.resize(n);
    for (int i = 0; i < n; ++i) for (int c = 0; c < 3; ++c) kf->bearings_add_[i][c] = bearing[3 * ((size_t)row_ptr[k] + i) + c];
    kf->id_ = {(size_t)k, (size_t)client[k]};
    std::memcpy(kf->T_wc_.m, T_wc + 16 * k, sizeof(double) * 16);
    std::memcpy(kf->T_cw_.m, T_cw + 16 * k, sizeof(double) * 16);
    h->kfs.push_back(kf);
  }
  for (int k = 0; k < nk; ++k) if (pred[k] >= 0) h->kfs[k]->pred_ = h->kfs[pred[k]];
  return h;
}
void f5_free(void* h) { delete static_cast<Handle*>(h); }
void f5_shutdown() { covins_gpu::OptimizationT<standin5::Types>::Shutdown(); }

unsigned long long f5_seed(void* hv, int a, int b, int cell) {
  auto* h = static_cast<Handle*>(hv);
  return covins_gpu::detail::fivept_seed(h->kfs[a].get(), h->kfs[b].get(), (uint64_t)cell);
}

// computePose of keyframes a, b on nm matches (idxA, idxB): T16 row-major (untouched unless found), inliers (ascending) and their count
int f5_compute_pose(void* hv, int a, int b, int nm, const int* idx, double threshold, int min_inliers, int max_iter, double* T16, int* inliers,
                    int* n_inliers) {
  auto* h = static_cast<Handle*>(hv);
  Solver::Matches m(nm);
  for (int i = 0; i < nm; ++i) { m[i].idxA = (size_t)idx[2 * i]; m[i].idxB = (size_t)idx[2 * i + 1]; m[i].distance = 0.0; }
  Solver solver(min_inliers, 0.5, max_iter);   // ransacProb is stored and not used, as in the reference
  standin5::Mat4 T;
  std::memcpy(T.m, T16, sizeof(T.m));
  std::vector<int> inl;
  const bool found = solver.computePose(h->kfs[a], h->kfs[b], m, threshold, T, inl);
  std::memcpy(T16, T.m, sizeof(T.m));
  *n_inliers = (int)inl.size();
  for (size_t i = 0; i < inl.size(); ++i) inliers[i] = inl[i];
  return found ? 1 : 0;
}

// ComputePoseGrid of query q against nc candidates (2 x 3 cells each). Per candidate: ok[c]; per cell (6 per candidate, query-major):
// the number of matches and of inliers, T_init16 of the candidate, TF (5 transforms: 2 of the query chain, 3 of the candidate's). The
// matches (idxA, idxB) and the inlier indices of all cells of all ok candidates are concatenated into midx / iidx (up to cap entries).
int f5_grid(void* hv, int q, int nc, const int* cand, double threshold, int min_inliers, int max_iter, int min_img_matches, float img_thres,
            float ratio, unsigned char* ok, int* n_matches, int* n_inliers, double* T_init16, double* TF16, int* midx, int* iidx, int cap) {
  auto* h = static_cast<Handle*>(hv);
  std::vector<KeyframePtr> c;
  for (int i = 0; i < nc; ++i) c.push_back(h->kfs[cand[i]]);
  Solver solver(min_inliers, 0.5, max_iter, min_img_matches);
  solver.setMatchParams("ORB", img_thres, ratio);
  const std::vector<Solver::GridResult> res = solver.ComputePoseGrid(h->kfs[q], c, threshold);
  int nm = 0, ni = 0;
  for (int i = 0; i < nc; ++i) {
    const Solver::GridResult& g = res[i];
    ok[i] = g.ok ? 1 : 0;
    for (int k = 0; k < 6; ++k) { n_matches[6 * i + k] = 0; n_inliers[6 * i + k] = 0; }
    if (!g.ok) continue;
    std::memcpy(T_init16 + 16 * i, g.T_init.m, sizeof(double) * 16);
    for (int k = 0; k < 2; ++k) std::memcpy(TF16 + 16 * (5 * i + k), g.TF_vect[0][k].m, sizeof(double) * 16);
    for (int k = 0; k < 3; ++k) std::memcpy(TF16 + 16 * (5 * i + 2 + k), g.TF_vect[1][k].m, sizeof(double) * 16);
    for (int a = 0; a < 2; ++a)
      for (int b = 0; b < 3; ++b) {
        const auto& m = g.match_vect[a][b];
        const auto& in = g.inliers_vect[a][b];
        n_matches[6 * i + 3 * a + b] = (int)m.size();
        n_inliers[6 * i + 3 * a + b] = g.inliers_size[3 * a + b];
        for (const auto& e : m) { if (nm < cap) { midx[2 * nm] = (int)e.idxA; midx[2 * nm + 1] = (int)e.idxB; } ++nm; }
        for (int e : in) { if (ni < cap) iidx[ni] = e; ++ni; }
      }
  }
  return nm > cap || ni > cap ? -1 : nm;
}

}  // extern "C"
