// k_obscov.hip — the observation pass behind covgpu_observation_covariance: for every observation o = (a, l) the 2x2 block
// C_o = J_o Sigma J_o^T of the hat matrix and the pose-landmark cross block Sigma_al, from what a build at mu leaves resident and the selected
// inverse of the reduced camera system; and the landmark's own block exactly as k_lmcov.hip writes it.
//
// With H_ll^-1 = R R^T (DevProblem::lmRT), Z_b = (J_p^T J_l) R of observation b (DevProblem::obsZ), V_a = sum_b Sigma_ab Z_b over the free
// observers b of l, M = sum_a Z_a^T V_a and Y = J_l R (2x3):
//   Sigma_al = -V_a R^T
//   C_o      = [J_p -Y] [[Sigma_aa, V_a], [V_a^T, (M + M^T) / 2]] [J_p -Y]^T + Y Y^T
// a quadratic form of a matrix that is positive semi-definite in exact arithmetic plus a positive semi-definite term — the same algebra as
// J Sigma J^T with Sigma_l = R (I + M) R^T, without the subtraction of the large J_l Sigma_l J_l^T from the cross terms.
//
// Landmark-major, one G-lane group per landmark (G = DevProblem::lm_group), lane a takes observations a, a + G, ..
//   pass 1  k_lmcov's loop (lmcov_dev.hpp), unchanged in order; each lane also stores the V_a it formed (18 doubles per observation, args.vx).
//           group_sum gives every lane M; every lane forms the landmark's block (lane 0 writes it), so every lane knows whether it is served.
//   pass 2  the same lane over the same observations: reads back the V_a IT stored (its own plain stores, program order: no barrier, no
//           flag — the idiom of k_selinv.hip), evaluates the observation at the resident estimate (eval_obs), loads Sigma_aa through
//           kf_blk (lower triangle) and writes obs_cov, obs_res, obs_ok and, over V_a, the cross block.
// No atomics, one summation order, one writer per output entry: two calls return the same bits. C_o's off-diagonal entry is computed once
// and stored twice.
#include "lmcov_dev.hpp"
#include "obscov.hpp"
#include "visual_dev.hpp"

namespace covgpu {
using namespace covdev;

template <int G, bool UNI>
__global__ __launch_bounds__(kObscovThreads) void k_obscov(DevProblem P, ObscovArgs A) {
  constexpr int GROUPS = kObscovThreads / G;
  const int lane = threadIdx.x % G, grp = threadIdx.x / G;
  const int l = blockIdx.x * GROUPS + grp;
  const bool live = l < P.L;
  const int o0 = live ? P.lm_obs_ptr[l] : 0;
  const int nobs = live ? P.lm_obs_ptr[l + 1] - o0 : 0;
  const double2* Zrec = reinterpret_cast<const double2*>(P.obsZ);

  // ---- pass 1
  double M[9];
  int missing = 0;   // a term whose block of Sigma was not found: the landmark and its observations are not served
#pragma unroll
  for (int k = 0; k < 9; ++k) M[k] = 0.0;
  for (int a = lane; a < nobs; a += G) {
    const int ka = P.obs_kf[o0 + a];
    if (P.fixed[ka]) continue;   // a constant pose has no rows in Sigma
    double Za[18], V[18];
    lmcov_load_z(Zrec, P.obs_zpos[o0 + a], Za);
    lmcov_gather_v(P, A.lm, Zrec, o0, nobs, ka, P.perm[ka], V, missing);
    lmcov_add_m(Za, V, M);
    double* vs = A.vx + 18 * (size_t)(o0 + a);
#pragma unroll
    for (int k = 0; k < 18; ++k) vs[k] = V[k];
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) M[k] = group_sum<G>(M[k]);
#pragma unroll
  for (int off = G / 2; off >= 1; off >>= 1) missing |= __shfl_xor(missing, off, G);
  if (!live) return;

  const double* rt = P.lmRT + 9 * (size_t)l;
  double out[9];
  const bool ok = lmcov_block(rt, M, missing, out);
  if (lane == 0) {
    double* dst = A.lm.lm_cov + 9 * (size_t)l;
#pragma unroll
    for (int k = 0; k < 9; ++k) dst[k] = ok ? out[k] : 0.0;
    A.lm.lm_ok[l] = ok ? 1 : 0;
  }

  // ---- pass 2
  const double r00 = rt[0], r10 = rt[1], r11 = rt[2], r20 = rt[3], r21 = rt[4], r22 = rt[5];
  double Ms[6];   // (M + M^T) / 2: xx xy xz yy yz zz
  Ms[0] = M[0]; Ms[1] = 0.5 * (M[1] + M[3]); Ms[2] = 0.5 * (M[2] + M[6]); Ms[3] = M[4]; Ms[4] = 0.5 * (M[5] + M[7]); Ms[5] = M[8];
  for (int a = lane; a < nobs; a += G) {
    const int o = o0 + a, ka = P.obs_kf[o];
    ObsLin e;
    eval_obs<true, UNI>(P, P.pose, P.lm, o, ka, l, e);   // (a constant pose: J_p = 0)
    const bool fx = P.fixed[ka] != 0;
    double* vs = A.vx + 18 * (size_t)o;
    double V[18], S[6][6];
    if (!fx) {
#pragma unroll
      for (int k = 0; k < 18; ++k) V[k] = vs[k];
      const LmcovBlock B = A.lm.kf_blk[ka];
      const double* Sb = A.lm.S + (B.off < 0 ? 0 : B.off);   // (off < 0: pass 1 set `missing`, nothing of this block is used)
#pragma unroll
      for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c <= r; ++c) { const double v = B.off < 0 ? 0.0 : Sb[(size_t)r * B.ld + c]; S[r][c] = v; S[c][r] = v; }
    } else {
#pragma unroll
      for (int k = 0; k < 18; ++k) V[k] = 0.0;
#pragma unroll
      for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) S[r][c] = 0.0;
    }
    double Y[2][3];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      Y[i][0] = e.jl[3 * i] * r00 + e.jl[3 * i + 1] * r10 + e.jl[3 * i + 2] * r20;
      Y[i][1] = e.jl[3 * i + 1] * r11 + e.jl[3 * i + 2] * r21;
      Y[i][2] = e.jl[3 * i + 2] * r22;
    }
    // t_j = Q u_j, u_j = [J_p row j; -Y row j], Q = [[Sigma_aa, V], [V^T, Ms]]
    double top[2][6], bot[2][3];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
      for (int r = 0; r < 6; ++r) {
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < 6; ++c) s += S[r][c] * e.jp[6 * j + c];
        top[j][r] = s - (V[3 * r] * Y[j][0] + V[3 * r + 1] * Y[j][1] + V[3 * r + 2] * Y[j][2]);
      }
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        double s = 0.0;
#pragma unroll
        for (int r = 0; r < 6; ++r) s += V[3 * r + p] * e.jp[6 * j + r];
        const double m0 = p == 0 ? Ms[0] : (p == 1 ? Ms[1] : Ms[2]), m1 = p == 0 ? Ms[1] : (p == 1 ? Ms[3] : Ms[4]), m2 = p == 0 ? Ms[2] : (p == 1 ? Ms[4] : Ms[5]);
        bot[j][p] = s - (m0 * Y[j][0] + m1 * Y[j][1] + m2 * Y[j][2]);
      }
    }
    double c[3];   // C_o: (0,0) (0,1) (1,1); entry (i, j) = u_i^T t_j + Y_i . Y_j
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const int i = q == 2 ? 1 : 0, j = q == 0 ? 0 : 1;
      double s = 0.0;
#pragma unroll
      for (int r = 0; r < 6; ++r) s += e.jp[6 * i + r] * top[j][r];
      s -= Y[i][0] * bot[j][0] + Y[i][1] * bot[j][1] + Y[i][2] * bot[j][2];
      c[q] = s + (Y[i][0] * Y[j][0] + Y[i][1] * Y[j][1] + Y[i][2] * Y[j][2]);
    }
    double* oc = A.obs_cov + 4 * (size_t)o;
    oc[0] = ok ? c[0] : 0.0; oc[1] = ok ? c[1] : 0.0; oc[2] = ok ? c[1] : 0.0; oc[3] = ok ? c[2] : 0.0;
    A.obs_res[2 * (size_t)o] = e.r0; A.obs_res[2 * (size_t)o + 1] = e.r1;
    A.obs_ok[o] = ok ? 1 : 0;
    // Sigma_al = -V R^T over V (a constant pose: zeros)
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      const double v0 = V[3 * r], v1 = V[3 * r + 1], v2 = V[3 * r + 2];
      vs[3 * r] = ok ? -(v0 * r00) : 0.0;
      vs[3 * r + 1] = ok ? -(v0 * r10 + v1 * r11) : 0.0;
      vs[3 * r + 2] = ok ? -(v0 * r20 + v1 * r21 + v2 * r22) : 0.0;
    }
  }
}

void launch_obscov(const DevProblem& P, const ObscovArgs& a, hipStream_t st) {
  if (P.L <= 0) return;
  const int g = P.lm_group == 4 || P.lm_group == 8 ? P.lm_group : 16;
  const int nblk = (P.L + kObscovThreads / g - 1) / (kObscovThreads / g);
  auto go = [&](auto G, auto U) {
    hipLaunchKernelGGL((k_obscov<decltype(G)::value, decltype(U)::value>), dim3(nblk), dim3(kObscovThreads), 0, st, P, a);
  };
  auto width = [&](auto U) {
    if (g == 4) go(std::integral_constant<int, 4>(), U); else if (g == 8) go(std::integral_constant<int, 8>(), U); else go(std::integral_constant<int, 16>(), U);
  };
  if (P.uni) width(std::true_type()); else width(std::false_type());
}

}  // namespace covgpu
