// lmcov.hpp — what the landmark pass of covgpu_landmark_covariance (k_lmcov.hip) and its host side (lmcov.hip) share: the per-call tables.
#pragma once
#include <vector>

#include "common.hpp"
#include "lmcov_check.hpp"

struct covgpu_context;
struct DeviceScratch;   // host.hpp

namespace covgpu {
struct SelPlan;         // selinv.hpp

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

// ---- host side (lmcov.hip), shared with the observation pass (obscov.hip)
// The tables of a landmark pass, on the host and on the device. lmcov_lists reads what the plan needs of the resident problem; lmcov_prepare
// runs inside sel_factor_and_sweep's `prepare` (plans the tables against the sweep's plan, allocates their device copies and the
// landmark outputs in U, adds their size to `bytes`; nothing is enqueued); lmcov_upload enqueues the copies and fills `a` but its S.
struct LmcovTables {
  std::vector<uint8_t> fixed;               // [K] by keyframe
  std::vector<int> pair_i, pair_j, pos_kf;  // the resident pair list (positions, sorted by (i, j), i > j) | position -> keyframe
  std::vector<LmcovBlock> kf_blk, pair_blk; // as LmcovArgs
  std::vector<int> row_ptr;
  LmcovBlock *d_kf = nullptr, *d_pair = nullptr;
  int* d_row = nullptr;
  double* d_lm_cov = nullptr; uint8_t* d_lm_ok = nullptr;
};
int lmcov_lists(const char* fn, covgpu_context* c, LmcovTables& t);
int lmcov_prepare(const char* fn, const covgpu_context* c, const SelPlan& pl, ::DeviceScratch& U, LmcovTables& t, size_t& bytes);
int lmcov_upload(covgpu_context* c, const LmcovTables& t, LmcovArgs& a);
// the refusals that depend on the context: sharded, nothing uploaded, a pose graph, off the elimination tree, no landmarks
int lmcov_context_check(const char* fn, const covgpu_context* c);

}  // namespace covgpu
