// ncrelpose.hpp — what k_ncrelpose.hip offers its host side ncrelpose.hip: the launch of the batch, of the solve-only
// test kernel, and the limits the kernel was built with.
#pragma once
#include <hip/hip_runtime.h>

namespace covgpu {

struct NcRelposeArgs {
  int num, cells, max_n, stage_cap;                 // stage_cap: 0 = the kernel's own, else the smaller of the two
  const int *ptr, *cell;                            // [num+1], [num][cells+1]
  const double *f1, *f2;                            // [C][3]
  const int *cam1, *cam2, *cam_ptr;                 // [C], [C], [num+1]
  const double *cam, *Tq, *Tc;                      // [M][12], [num][7], [num][7]
  const unsigned long long* seed;                   // [num]
  double *T, *Tr, *Ts, *cov;                        // [num][7] x 3, [num][36]
  unsigned char* inlier;                            // [C]
  int* list;                                        // [C] scratch
  int *inliers, *status, *iterations, *best_draw, *cov_rows, *cov_draws;
  int min_inliers, max_iterations, cov_iters, cov_max_iters;
  double probability, threshold, th_cov, cov_thres;
};

// LDS staging cap, draws per pass, sample size, largest max_iterations, most cells, most covariance rows, most rows of a solve, polish steps
void ncrelpose_limits(int out[8]);
hipError_t launch_ncrelpose(const NcRelposeArgs& a, hipStream_t st);
hipError_t launch_ncrelpose_solve(int num, int N, const double* ray1, const double* ray2, double* T, int* ok, double* sv, hipStream_t st);

}  // namespace covgpu
