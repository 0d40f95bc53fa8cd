// k_lmcov.hip — the landmark pass behind covgpu_landmark_covariance: the 3x3 covariance of every landmark from what a build at
// mu leaves resident and the selected inverse of the reduced camera system (k_selinv.hip).
//
// With H_ll^-1 = R R^T (DevProblem::lmRT) and Z_a = (J_p^T J_l) R of observation a (DevProblem::obsZ, slot obs_zpos[o]), both written by k_lm_lin:
//   Sigma_l = H_ll^-1 + H_ll^-1 H_lp Sigma_pp H_pl H_ll^-1 = R (I + sum over a, b of Z_a^T Sigma_ab Z_b) R^T
// over the observations a, b of l by keyframes with a free pose; Sigma_ab is the 6x6 pose-pose block of Sigma between the two observers. Any
// two observers of a landmark are covisible, so the block lies on the structure of L, in the buffer the sweep filled; the host side (lmcov.hip)
// says where, per entry of the covisible pair list and per keyframe.
//
// Landmark-major like k_lm_lin, k_lm_backsub and k_lm_outliers: one G-lane group per landmark, G = DevProblem::lm_group. Lane a takes
// observations a, a + G, ..; for each it forms V_a = sum_b Sigma_ab Z_b, b over ALL free observers in landmark order, then M_a = Z_a^T V_a; the
// lanes' M_a are summed by the shuffle butterfly of k_lm_lin's H_ll (group_sum). Every sum has one order, nothing is accumulated with
// atomics, every output entry has one writer: two calls return the same bits.
// Block (a, b) of two different keyframes is entry e of the pair list with (pair_i, pair_j) = (larger, smaller position): a binary search of
// pair_j inside the row of the larger position. The list holds Sigma[rows of i][rows of j]; the other orientation reads the same 36 numbers
// transposed (the sweep stores both halves of Sigma from one computed value, so that IS Sigma_ji bit for bit). A diagonal block is read
// through its lower triangle. A block that is not found (the list is built from the same observation stream, and the host plan resolves every
// entry of it: it does not happen) is not skipped in silence: the landmark gets lm_ok = 0 and a zero block, never a covariance that is too small.
// The sum over the observer pairs and the landmark's block are in lmcov_dev.hpp, which k_obscov.hip shares.
#include "lmcov_dev.hpp"

namespace covgpu {
using namespace covdev;

template <int G>
__global__ __launch_bounds__(kLmcovThreads) void k_lmcov(DevProblem P, LmcovArgs A) {
  constexpr int GROUPS = kLmcovThreads / G;
  const int lane = threadIdx.x % G, grp = threadIdx.x / G;
  const int l = blockIdx.x * GROUPS + grp;
  const bool live = l < P.L;
  const int o0 = live ? P.lm_obs_ptr[l] : 0;
  const int nobs = live ? P.lm_obs_ptr[l + 1] - o0 : 0;
  const double2* Zrec = reinterpret_cast<const double2*>(P.obsZ);

  double M[9];
  int missing = 0;   // a term whose block of Sigma was not found: the sum would come out too small, so the landmark is not served
#pragma unroll
  for (int k = 0; k < 9; ++k) M[k] = 0.0;
  for (int a = lane; a < nobs; a += G) {
    const int ka = P.obs_kf[o0 + a];
    if (P.fixed[ka]) continue;   // a constant pose has no rows in Sigma
    double Za[18], V[18];
    lmcov_load_z(Zrec, P.obs_zpos[o0 + a], Za);
    lmcov_gather_v(P, A, Zrec, o0, nobs, ka, P.perm[ka], V, missing);
    lmcov_add_m(Za, V, M);
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) M[k] = group_sum<G>(M[k]);
#pragma unroll
  for (int off = G / 2; off >= 1; off >>= 1) missing |= __shfl_xor(missing, off, G);
  if (!live || lane != 0) return;

  double out[9];
  const bool ok = lmcov_block(P.lmRT + 9 * (size_t)l, M, missing, out);
  double* dst = A.lm_cov + 9 * (size_t)l;
#pragma unroll
  for (int k = 0; k < 9; ++k) dst[k] = ok ? out[k] : 0.0;
  A.lm_ok[l] = ok ? 1 : 0;
}

void launch_lmcov(const DevProblem& P, const LmcovArgs& a, hipStream_t st) {
  if (P.L <= 0) return;
  const int g = P.lm_group == 4 || P.lm_group == 8 ? P.lm_group : 16;
  const int nblk = (P.L + kLmcovThreads / g - 1) / (kLmcovThreads / g);
  if (g == 4) hipLaunchKernelGGL(k_lmcov<4>, dim3(nblk), dim3(kLmcovThreads), 0, st, P, a);
  else if (g == 8) hipLaunchKernelGGL(k_lmcov<8>, dim3(nblk), dim3(kLmcovThreads), 0, st, P, a);
  else hipLaunchKernelGGL(k_lmcov<16>, dim3(nblk), dim3(kLmcovThreads), 0, st, P, a);
}

}  // namespace covgpu
