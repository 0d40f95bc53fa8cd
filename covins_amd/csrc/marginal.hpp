// marginal.hpp — what the sweep of the marginal covariances (k_marginal.hip) and its host side (marginal.hip) share: the per-call tables.
#pragma once
#include "common.hpp"
#include "marginal_check.hpp"

namespace covgpu {

// One front on the paths from the chosen unknowns to the root. Its active columns are the contiguous range [c0, c1) of the columns in
// sweep order (the post-order of their owners); W is the working matrix [rows][mp] of right-hand sides, one row per own unknown of every
// such front (a front's rows rounded up to 16: the padding rows stay zero under the identity the factor holds there).
struct MargFront {
  long long moff, linv;   // element offset of the front in nd_M | of its block inverses in nd_Linv
  int ld, nI, own, st;    // leading dimension | padded interior order of its level (where the border rows start) | own | border unknowns
  int nbo, wbase;         // 16-row blocks of its own unknowns | its first row in W
  int c0, c1;             // active columns
  int bmap, pad;          // first entry of its border rows' map (border scalar -> row of W)
};
// One workgroup of a step: x = front, y = panel (128 own columns), z = kind (0: substitute the panel's own rows | 1: update the 16 own rows of
// block w, below the panel | 2: update the 16 border rows of block w)
struct MargArgs {
  const double *M, *Linv;
  double* W; int mp;
  const MargFront* fr; const int* bmap; const int4* items;
};
void launch_marg_seed(double* W, int mp, int m, const int* seed_row, hipStream_t st);
void launch_marg_step(const MargArgs& a, int item0, int count, bool mfma, hipStream_t st);
void launch_marg_gram(const double* W, int mp, const MargFront* fr, int nf, const int* perm, int m, double* cov, hipStream_t st);

}  // namespace covgpu
