// ncrelpose_check.hpp — the argument checks of the 17-point batch (covgpu_ncrelpose_batch, covgpu_ncrelpose_solve_batch; DESIGN.md
// §4.24), beside fivept_check.hpp and to its rules: plain C++17 over covgpu.h and the standard library, no HIP call and no HIP type, so
// the checks compile and run (under sanitizers too) without a device: tests/cpp/ncrelpose_check_main.cpp. Every check is a pure function
// of its arguments that returns the message of the first violation, or nullptr; what it derives on the way goes into the plan.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/covgpu.h"

namespace covgpu {

constexpr int kNcrelposeMaxIterations = 100000;
constexpr int kNcrelposeMaxCells = 16;
constexpr int kNcrelposeMaxCovIters = 256;
constexpr int kNcrelposeMaxRows = 64;

struct NcrelposePlan {
  size_t corr = 0, cams = 0;
  int max_n = 0;
  double threshold = 0.0, th_cov = 0.0;         // 2 (1 - cos atan(rp_error / 800)) (RelNonCentralPosSolver.cpp:48-49)
  std::vector<unsigned long long> seeds;
};

inline double ncrelpose_threshold(double rp_error) { return 2.0 * (1.0 - std::cos(std::atan(rp_error * 1 / 800.0))); }

inline const char* ncrelpose_check(const covgpu_ncrelpose_batch_t* bt, const covgpu_ncrelpose_opts* o, NcrelposePlan& P) {
  if (!bt || !o) return "NULL batch or options";
  if (bt->num < 0) return "num < 0";
  if (o->max_iterations < 1 || o->max_iterations > kNcrelposeMaxIterations) return "max_iterations outside 1..100000";
  if (o->cov_iters < 2 || o->cov_iters > kNcrelposeMaxCovIters) return "cov_iters outside 2..256";
  if (o->cov_max_iters < 0) return "cov_max_iters < 0";
  if (o->min_inliers < 0) return "min_inliers < 0";
  if (o->stage_cap < 0) return "stage_cap < 0";
  if (!(o->probability > 0.0 && o->probability < 1.0)) return "probability outside (0, 1)";
  if (!std::isfinite(o->rp_error) || !(o->rp_error > 0.0)) return "rp_error not finite or not positive";
  if (!std::isfinite(o->rp_error_cov) || !(o->rp_error_cov > 0.0)) return "rp_error_cov not finite or not positive";
  if (std::isnan(o->cov_thres)) return "cov_thres is NaN";
  P.threshold = ncrelpose_threshold(o->rp_error);
  P.th_cov = ncrelpose_threshold(o->rp_error_cov);
  const size_t B = (size_t)bt->num;
  if (B == 0) return nullptr;
  if (bt->cells < 1 || bt->cells > kNcrelposeMaxCells) return "cells outside 1..16";
  if (!bt->corr_ptr || !bt->cell_ptr || !bt->cam_ptr || !bt->T_sc_q || !bt->T_sc_c || !bt->T_c1c2 || !bt->T_c1c2_ransac || !bt->T_s1s2 || !bt->cov ||
      !bt->inliers || !bt->status || !bt->iterations || !bt->best_draw || !bt->cov_rows || !bt->cov_draws)
    return "NULL array";
  if (bt->corr_ptr[0] != 0) return "corr_ptr[0] != 0";
  if (bt->cam_ptr[0] != 0) return "cam_ptr[0] != 0";
  const size_t nc = (size_t)bt->cells + 1;
  for (size_t b = 0; b < B; ++b) {
    if (bt->corr_ptr[b + 1] < bt->corr_ptr[b]) return "corr_ptr not monotone";
    if (bt->cam_ptr[b + 1] < bt->cam_ptr[b]) return "cam_ptr not monotone";
    const int n = bt->corr_ptr[b + 1] - bt->corr_ptr[b];
    P.max_n = std::max(P.max_n, n);
    const int32_t* c = bt->cell_ptr + b * nc;
    if (c[0] != 0 || c[bt->cells] != n) return "cell_ptr does not span the job";
    for (int j = 0; j < bt->cells; ++j)
      if (c[j + 1] < c[j]) return "cell_ptr not monotone";
  }
  P.corr = (size_t)bt->corr_ptr[B];
  P.cams = (size_t)bt->cam_ptr[B];
  if (P.cams > 0 && !bt->cam) return "NULL camera table";
  for (size_t i = 0; i < 12 * P.cams; ++i)
    if (!std::isfinite(bt->cam[i])) return "non-finite camera table";
  for (size_t i = 0; i < 7 * B; ++i)
    if (!std::isfinite(bt->T_sc_q[i]) || !std::isfinite(bt->T_sc_c[i])) return "non-finite extrinsics";
  for (size_t b = 0; b < B; ++b) {
    const double *q = bt->T_sc_q + 7 * b, *c = bt->T_sc_c + 7 * b;
    if (!(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3] > 0.0) || !(c[0] * c[0] + c[1] * c[1] + c[2] * c[2] + c[3] * c[3] > 0.0))
      return "zero quaternion in the extrinsics";
  }
  if (P.corr > 0 && (!bt->bearing1 || !bt->bearing2 || !bt->cam1 || !bt->cam2 || !bt->inlier)) return "NULL correspondence array";
  for (size_t i = 0; i < 3 * P.corr; ++i)
    if (!std::isfinite(bt->bearing1[i]) || !std::isfinite(bt->bearing2[i])) return "non-finite bearing";
  for (size_t b = 0; b < B; ++b) {
    const int32_t m = bt->cam_ptr[b + 1] - bt->cam_ptr[b];
    for (int32_t i = bt->corr_ptr[b]; i < bt->corr_ptr[b + 1]; ++i)
      if (bt->cam1[i] < 0 || bt->cam1[i] >= m || bt->cam2[i] < 0 || bt->cam2[i] >= m) return "camera index out of range";
  }
  P.seeds.resize(B);
  for (size_t b = 0; b < B; ++b) P.seeds[b] = bt->seed ? bt->seed[b] : o->seed + (uint64_t)b;
  return nullptr;
}

inline const char* ncrelpose_solve_check(int32_t n, int32_t N, const double* ray1, const double* ray2, const double* T, const int32_t* ok, const double* sv) {
  if (n < 0) return "n < 0";
  if (N < 17 || N > kNcrelposeMaxRows) return "N outside 17..64";
  if (n == 0) return nullptr;
  if (!ray1 || !ray2 || !T || !ok || !sv) return "NULL array";
  for (size_t i = 0; i < 6 * (size_t)n * (size_t)N; ++i)
    if (!std::isfinite(ray1[i]) || !std::isfinite(ray2[i])) return "non-finite ray";
  return nullptr;
}

}  // namespace covgpu
