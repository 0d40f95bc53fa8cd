// fivept_check.hpp — the argument checks of the five-point relative-pose batch (covgpu_fivept_ransac_batch, covgpu_fivept_solve_batch;
// DESIGN.md §4.23), beside batch_check.hpp and to its rules: plain C++17 over covgpu.h and the standard library, no HIP call and no HIP
// type, so the checks compile and run (under sanitizers too) without a device: tests/cpp/fivept_check_main.cpp. Every check is a pure
// function of its arguments that returns the message of the first violation, or nullptr; what it derives on the way goes into the plan.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/covgpu.h"

namespace covgpu {

constexpr int kFiveptMaxIterations = 100000;    // a job makes up to 11 max_iterations + 1 draws in one launch

struct FiveptPlan {
  size_t corr = 0;
  int max_n = 0;                                // the longest job
  std::vector<unsigned long long> seeds;        // (the kernel's type for the 64-bit seeds)
};

inline const char* fivept_check(const covgpu_fivept_batch_t* bt, const covgpu_fivept_opts* opts, FiveptPlan& P) {
  if (!bt || !opts) return "NULL batch or options";
  if (bt->num < 0) return "num < 0";
  if (opts->max_iterations <= 0) return "max_iterations <= 0";
  if (opts->max_iterations > kFiveptMaxIterations) return "max_iterations > 100000 (a job makes up to 11 max_iterations draws in one launch)";
  if (!(opts->probability > 0.0 && opts->probability < 1.0)) return "probability outside (0, 1)";
  if (!std::isfinite(opts->threshold) || !(opts->threshold > 0.0)) return "threshold not finite or not positive";
  if (!std::isfinite(opts->sigma) || !(opts->sigma > 0.0)) return "sigma not finite or not positive";
  const size_t B = (size_t)bt->num;
  if (B == 0) return nullptr;
  if (!bt->corr_ptr || !bt->T_12 || !bt->inliers || !bt->status) return "NULL array";
  if (bt->corr_ptr[0] != 0) return "corr_ptr[0] != 0";
  for (size_t b = 0; b < B; ++b) {
    if (bt->corr_ptr[b + 1] < bt->corr_ptr[b]) return "corr_ptr not monotone";
    P.max_n = std::max(P.max_n, bt->corr_ptr[b + 1] - bt->corr_ptr[b]);
  }
  P.corr = (size_t)bt->corr_ptr[B];
  if (P.corr > 0 && (!bt->bearing1 || !bt->bearing2 || !bt->inlier)) return "NULL correspondence array";
  for (size_t i = 0; i < 3 * P.corr; ++i)
    if (!std::isfinite(bt->bearing1[i]) || !std::isfinite(bt->bearing2[i])) return "non-finite bearing";
  P.seeds.resize(B);
  for (size_t b = 0; b < B; ++b) P.seeds[b] = bt->seed ? bt->seed[b] : opts->seed + (uint64_t)b;
  return nullptr;
}

inline const char* fivept_solve_check(int32_t n, const double* f1, const double* f2, const double* E, const int32_t* nsol, const double* T,
                                      const int32_t* chosen) {
  if (n < 0) return "n < 0";
  if (n == 0) return nullptr;
  if (!f1 || !f2 || !E || !nsol || !T || !chosen) return "NULL array";
  for (size_t i = 0; i < 24 * (size_t)n; ++i)
    if (!std::isfinite(f1[i]) || !std::isfinite(f2[i])) return "non-finite bearing";
  return nullptr;
}

}  // namespace covgpu
