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
#include "dev_math.hpp"
#include "lmcov.hpp"

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
    const int pa = P.perm[ka];
    double Za[18], V[18];
    {
      const double2* z = Zrec + 9 * (size_t)P.obs_zpos[o0 + a];
#pragma unroll
      for (int k = 0; k < 9; ++k) { const double2 t = z[k]; Za[2 * k] = t.x; Za[2 * k + 1] = t.y; }
    }
#pragma unroll
    for (int k = 0; k < 18; ++k) V[k] = 0.0;
    for (int b = 0; b < nobs; ++b) {
      const int kb = P.obs_kf[o0 + b];
      if (P.fixed[kb]) continue;
      const int pb = P.perm[kb];
      LmcovBlock B;
      int sr, sc;             // strides of Sigma_ab's rows and columns in the stored block
      const bool diag = pa == pb;
      if (diag) { B = A.kf_blk[ka]; sr = B.ld; sc = 1; }
      else {
        const int hi = pa > pb ? pa : pb, lo = pa > pb ? pb : pa;
        int e0 = A.row_ptr[hi], e1 = A.row_ptr[hi + 1];
        while (e0 < e1) { const int m = (e0 + e1) >> 1; if (P.pair_j[m] < lo) e0 = m + 1; else e1 = m; }
        if (e0 >= A.row_ptr[hi + 1] || P.pair_j[e0] != lo) { missing = 1; continue; }   // (two observers of a landmark are a pair of the list: not taken)
        B = A.pair_blk[e0];
        sr = pa > pb ? B.ld : 1; sc = pa > pb ? 1 : B.ld;
      }
      if (B.off < 0) { missing = 1; continue; }   // (the host plan resolves every entry: not taken)
      const double* Sb = A.S + B.off;
      double Zb[18];
      {
        const double2* z = Zrec + 9 * (size_t)P.obs_zpos[o0 + b];
#pragma unroll
        for (int k = 0; k < 9; ++k) { const double2 t = z[k]; Zb[2 * k] = t.x; Zb[2 * k + 1] = t.y; }
      }
#pragma unroll
      for (int r = 0; r < 6; ++r) {
        double s[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) {
          const bool up = diag && c > r;   // a diagonal block through its lower triangle
          s[c] = Sb[(size_t)(up ? c : r) * sr + (size_t)(up ? r : c) * sc];
        }
#pragma unroll
        for (int c = 0; c < 6; ++c) {
          V[3 * r] += s[c] * Zb[3 * c]; V[3 * r + 1] += s[c] * Zb[3 * c + 1]; V[3 * r + 2] += s[c] * Zb[3 * c + 2];
        }
      }
    }
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        M[3 * p] += Za[3 * r + p] * V[3 * r]; M[3 * p + 1] += Za[3 * r + p] * V[3 * r + 1]; M[3 * p + 2] += Za[3 * r + p] * V[3 * r + 2];
      }
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) M[k] = group_sum<G>(M[k]);
#pragma unroll
  for (int off = G / 2; off >= 1; off >>= 1) missing |= __shfl_xor(missing, off, G);
  if (!live || lane != 0) return;

  // Sigma_l = R T R^T, T = I + (M + M^T) / 2 (M is symmetric up to rounding), R = (r00 r10 r11 r20 r21 r22) lower: one triangle, stored twice
  const double* rt = P.lmRT + 9 * (size_t)l;
  const double R[3][3] = {{rt[0], 0.0, 0.0}, {rt[1], rt[2], 0.0}, {rt[3], rt[4], rt[5]}};
  double T[3][3];
#pragma unroll
  for (int p = 0; p < 3; ++p)
#pragma unroll
    for (int q = 0; q <= p; ++q) { const double t = 0.5 * (M[3 * p + q] + M[3 * q + p]) + (p == q ? 1.0 : 0.0); T[p][q] = t; T[q][p] = t; }
  double Y[3][3], out[9];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int q = 0; q < 3; ++q) Y[r][q] = R[r][0] * T[0][q] + R[r][1] * T[1][q] + R[r][2] * T[2][q];
  // k_lm_lin leaves a zero pivot in R (chol3) for an H_ll it could not accept as positive definite: no covariance
  bool ok = R[0][0] > 0.0 && R[1][1] > 0.0 && R[2][2] > 0.0 && missing == 0;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c <= r; ++c) {
      const double v = Y[r][0] * R[c][0] + Y[r][1] * R[c][1] + Y[r][2] * R[c][2];
      ok = ok && isfinite(v);
      out[3 * r + c] = v; out[3 * c + r] = v;
    }
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
