// lmcov.hpp — what the landmark pass of covgpu_landmark_covariance (k_lmcov.hip) and its host side (lmcov.hip) share: the per-call tables.
#pragma once
#include "common.hpp"
#include "lmcov_check.hpp"

namespace covgpu {

// Where a 6x6 pose-pose block of Sigma lies in the sweep's buffer (laid out like the fronts): element offset of its first entry and the
// leading dimension of the square that holds it.
struct LmcovBlock { long long off; int ld, pad; };
static_assert(sizeof(LmcovBlock) == 16, "one 16-byte load per block");

// Two numberings meet here, and every table says which it uses:
//   keyframe   index of the problem (obs_kf, fixed, perm; the solution index of its pose rows is D * keyframe)
//   position   chain-major position perm[keyframe] (pair_i, pair_j of the covisible pair list)
struct LmcovArgs {
  const double* S;               // Sigma
  const LmcovBlock* kf_blk;      // [K] by KEYFRAME: the diagonal pose block (only its lower triangle is read); off < 0: constant pose
  const LmcovBlock* pair_blk;    // [npairs] by ENTRY of the covisible pair list: Sigma[pose rows of position pair_i][pose rows of position pair_j]
  const int* row_ptr;            // [K + 1] by POSITION i: first entry of the pair list with pair_i >= i (the list is sorted by (i, j), i > j)
  double* lm_cov;                // [L][9]
  uint8_t* lm_ok;                // [L]
};
void launch_lmcov(const DevProblem& P, const LmcovArgs& a, hipStream_t st);   // one launch; P.L > 0

}  // namespace covgpu
