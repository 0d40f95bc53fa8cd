// lmcov_dev.hpp — the device functions the two landmark passes behind the selected inverse share: k_lmcov.hip (covgpu_landmark_covariance,
// DESIGN.md §4.21) and k_obscov.hip (covgpu_observation_covariance, §4.22). One text for the sum over the observer pairs of a landmark and
// for the landmark's block, so both kernels return the same bits of lm_cov.
#pragma once
#include "dev_math.hpp"
#include "lmcov.hpp"

namespace covgpu {
using namespace covdev;

// the 144-byte record Z = (J_p^T J_l) R of the observation in slot zpos (6x3 row-major)
COV_DEV void lmcov_load_z(const double2* Zrec, int zpos, double* Z) {
  const double2* z = Zrec + 9 * (size_t)zpos;
#pragma unroll
  for (int k = 0; k < 9; ++k) { const double2 t = z[k]; Z[2 * k] = t.x; Z[2 * k + 1] = t.y; }
}

// V_a = sum_b Sigma_ab Z_b (6x3 row-major) for the free observer at position pa (keyframe ka), b over ALL free observers of the landmark whose
// observations are o0 .. o0 + nobs - 1, in landmark order. Block (a, b) of two different keyframes is entry e of the pair list with
// (pair_i, pair_j) = (larger, smaller position): a binary search of pair_j inside the row of the larger position. The list holds
// Sigma[rows of i][rows of j]; the other orientation reads the same 36 numbers transposed. A diagonal block is read through its lower triangle.
// A block that is not found sets `missing` and is left out.
COV_DEV void lmcov_gather_v(const DevProblem& P, const LmcovArgs& A, const double2* Zrec, int o0, int nobs, int ka, int pa, double* V, int& missing) {
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
    lmcov_load_z(Zrec, P.obs_zpos[o0 + b], Zb);
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
}

// M += Z_a^T V_a
COV_DEV void lmcov_add_m(const double* Za, const double* V, double* M) {
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int p = 0; p < 3; ++p) {
      M[3 * p] += Za[3 * r + p] * V[3 * r]; M[3 * p + 1] += Za[3 * r + p] * V[3 * r + 1]; M[3 * p + 2] += Za[3 * r + p] * V[3 * r + 2];
    }
}

// a0 b0 + a1 b1 + a2 b2 with its roundings spelled out: fma(a2, b2, fma(a0, b0, a1 * b1)), or with `first` the first product rounded on
// its own, fma(a2, b2, fma(a1, b1, a0 * b0)). Left to the compiler, which product of such a sum is fused depends on the code around it
// (how often a product is used): written as plain sums, lmcov_block came out with other bits in k_obscov than in k_lmcov. It names for
// every sum the form k_lmcov had when the sums were plain (read off its instruction selection: Y[2][1] and entry (2, 1) of the block
// round the first product, the thirteen others the second), so k_lmcov returns the bits it always returned and k_obscov the same.
template <bool first = false>
COV_DEV double lmcov_dot3(double a0, double b0, double a1, double b1, double a2, double b2) {
  return first ? fma(a2, b2, fma(a1, b1, a0 * b0)) : fma(a2, b2, fma(a0, b0, a1 * b1));
}

// Sigma_l = R T R^T, T = I + (M + M^T) / 2 (M is symmetric up to rounding), R = (r00 r10 r11 r20 r21 r22) lower = rt[0..5]: one triangle, stored
// twice. Returns whether the landmark is served; out (9) is the block, not yet zeroed where it is not.
COV_DEV bool lmcov_block(const double* rt, const double* M, int missing, double* out) {
  const double R[3][3] = {{rt[0], 0.0, 0.0}, {rt[1], rt[2], 0.0}, {rt[3], rt[4], rt[5]}};
  double T[3][3];
#pragma unroll
  for (int p = 0; p < 3; ++p)
#pragma unroll
    for (int q = 0; q <= p; ++q) { const double t = fma(M[3 * p + q] + M[3 * q + p], 0.5, p == q ? 1.0 : 0.0); T[p][q] = t; T[q][p] = t; }
  double Y[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int q = 0; q < 3; ++q)
      Y[r][q] = r == 2 && q == 1 ? lmcov_dot3<true>(R[r][0], T[0][q], R[r][1], T[1][q], R[r][2], T[2][q])
                                 : lmcov_dot3(R[r][0], T[0][q], R[r][1], T[1][q], R[r][2], T[2][q]);
  // k_lm_lin leaves a zero pivot in R (chol3) for an H_ll it could not accept as positive definite: no covariance
  bool ok = R[0][0] > 0.0 && R[1][1] > 0.0 && R[2][2] > 0.0 && missing == 0;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c <= r; ++c) {
      const double v = r == 2 && c == 1 ? lmcov_dot3<true>(Y[r][0], R[c][0], Y[r][1], R[c][1], Y[r][2], R[c][2])
                                        : lmcov_dot3(Y[r][0], R[c][0], Y[r][1], R[c][1], Y[r][2], R[c][2]);
      ok = ok && isfinite(v);
      out[3 * r + c] = v; out[3 * c + r] = v;
    }
  return ok;
}

}  // namespace covgpu
