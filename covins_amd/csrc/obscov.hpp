// obscov.hpp — what the observation pass of covgpu_observation_covariance (k_obscov.hip) and its host side (obscov.hip) share.
#pragma once
#include "lmcov.hpp"
#include "obscov_check.hpp"

namespace covgpu {

// Everything is in the landmark-major observation order of the resident problem. `vx` is pass 1's store of V_a and pass 2's cross block:
// the lane that wrote V_a of an observation reads it back and overwrites it with Sigma_al = -V_a R^T.
struct ObscovArgs {
  LmcovArgs lm;          // Sigma, the tables and the landmark outputs of the landmark pass
  double* vx;            // [O][18]
  double* obs_cov;       // [O][4]
  double* obs_res;       // [O][2]
  uint8_t* obs_ok;       // [O]
};
void launch_obscov(const DevProblem& P, const ObscovArgs& a, hipStream_t st);   // one launch; P.L > 0

}  // namespace covgpu
