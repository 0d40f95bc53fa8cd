// k_selinv.hip — the sweep behind covgpu_selected_inverse: Sigma = S^-1 on the structure of L, from the factored fronts of
// the multifrontal solve (k_front.hip) as launch_nd_solve left them, root to leaves.
//
// For a front with own unknowns O and border B (L_OO, L_BO in nd_M), with Sigma_BB known from the ancestors:
//   W = L_OO^-1            block column by block column with the 16x16 block inverses of nd_Linv (the chain of k_marg_step's kind 0)
//   T = L_BO W
//   Sigma_BO = -Sigma_BB T
//   Sigma_OO = W^T W - Sigma_OB T      (= L_OO^-T (L_OO^-1 - L_BO^T Sigma_BO), written as a sum of two positive semi-definite terms)
// A level's fronts share a fixed sequence of launches: the gather of Sigma_BB out of the ancestor's finished square through the row map,
// then the four steps above in the matrix-core form, and the vector form's one launch. Launch boundaries are the only ordering: no gates,
// no flags, no atomics, and every sum runs in one fixed order.
// Sigma's square and the temporaries W / T live in two scratch buffers laid out like nd_M (selinv.hpp); both start zeroed, so the padding
// rows and columns of a front (own .. 16 nbo, st .. the next multiple of 128) read as zeros and a product may run over whole 16-blocks.
// Matrix-core form (v_mfma_f64_16x16x4_f64, operands as in k_panel.hip / k_marginal.hip: A lane n carries logical row 4 (n & 3) + (n >> 2),
// k-slot (lane >> 4, s) carries k = 4 (lane >> 4) + s, so an A operand that is contiguous along k is one 32-byte load and the accumulator
// of one product is the B operand of the next): a workgroup of a product owns 16 rows x 128 columns, its four waves two 16-column chunks
// each, so the rows of Sigma_BB are read once per panel of 128 own columns.
// Vector form: one workgroup per front, thread per entry, for the many small fronts of the bottom levels.
// Both halves of every symmetric block are stored (an entry is computed once and stored twice), so a child's gather may read either.
#include "selinv.hpp"

namespace covgpu {

typedef double v4f64 __attribute__((ext_vector_type(4)));

// Sigma_BB(f)[a][b] = Sigma(p)[map a][map b]: one workgroup per 16 border rows
__global__ __launch_bounds__(256) void k_selinv_gather(SelArgs a, int item0) {
  const int4 it = a.items[item0 + (int)blockIdx.x];
  const SelFront f = a.fr[it.x];
  const int r = 16 * it.z + (threadIdx.x >> 4);
  if (r >= f.st) return;
  const int* gm = a.gmap + f.gmap;
  const double* src = a.S + f.pmoff + (size_t)gm[r] * f.pld;
  double* dst = a.S + f.moff + (size_t)(f.nI + r) * f.ld + f.nI;
  for (int c = threadIdx.x & 15; c < f.st; c += 16) dst[c] = src[gm[c]];
}

// ---- matrix-core form
// kind 1: columns [16 c, 16 c + 16) of W = L_OO^-1, one wave per chunk c. A lane reads back only what it stored itself.
__device__ __forceinline__ void sel_winv_mfma(const SelArgs& a, const SelFront& f, int cg) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, fk = lane >> 4, pr = 4 * (n & 3) + (n >> 2);
  const int c = 4 * cg + wave;
  if (c >= f.nbo) return;
  const double* L = a.M + f.moff;
  const double* D = a.Linv + f.linv;
  double* Xc = a.X + f.moff + 16 * c + n;
  for (int i = c; i < f.nbo; ++i) {
    v4f64 acc;
#pragma unroll
    for (int s = 0; s < 4; ++s) acc[s] = (i == c && 4 * fk + s == n) ? 1.0 : 0.0;
    for (int j = c; j < i; ++j) {
      const v4f64 l4 = *reinterpret_cast<const v4f64*>(L + (size_t)(16 * i + pr) * f.ld + 16 * j + 4 * fk);
#pragma unroll
      for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-l4[s], Xc[(size_t)(16 * j + 4 * fk + s) * f.ld], acc, 0, 0, 0);
    }
    const v4f64 d4 = *reinterpret_cast<const v4f64*>(D + (size_t)(i >> 3) * kTile * kTile + (i & 7) * 256 + pr * 16 + 4 * fk);
    v4f64 z = v4f64{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < 4; ++s) z = __builtin_amdgcn_mfma_f64_16x16x4f64(d4[s], acc[s], z, 0, 0, 0);
#pragma unroll
    for (int s = 0; s < 4; ++s) Xc[(size_t)(16 * i + 4 * fk + s) * f.ld] = z[s];
  }
}

// kinds 2 .. 4: 16 rows x 128 columns of a product, wave w the 16-column chunks 8 ch + 2 w and + 1
//   2  T[border block b]         =  L_BO[b, :] W
//   3  Sigma_BO[border block b]  = -Sigma_BB[b, :] T                      (stored at both places)
//   4  Sigma_OO[own block b]     =  W[:, b]^T W - Sigma_OB[b, :] T        (chunks up to the diagonal; an entry on or below it stored at both places)
template <int KIND>
__device__ __forceinline__ void sel_prod_mfma(const SelArgs& a, const SelFront& f, int b, int ch) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, fk = lane >> 4, pr = 4 * (n & 3) + (n >> 2);
  const int jb0 = 8 * ch + 2 * wave;
  if (jb0 >= f.nbo || (KIND == 4 && jb0 > b)) return;
  const bool two = jb0 + 1 < f.nbo && (KIND != 4 || jb0 + 1 <= b);
  const size_t ld = (size_t)f.ld;
  const double* X = a.X + f.moff;
  const double* Xb = X + 16 * jb0 + n;   // the B operand's column (chunk jb0; chunk jb0 + 1 is 16 further)
  v4f64 acc0 = v4f64{0.0, 0.0, 0.0, 0.0}, acc1 = acc0;
  if (KIND == 2) {
    const double* Lr = a.M + f.moff + (size_t)(f.nI + min(16 * b + pr, f.st - 1)) * ld + 4 * fk;
    for (int kb = 8 * ch; kb < f.nbo; ++kb) {   // (W is lower triangular: nothing above the panel's first block row)
      const v4f64 l4 = *reinterpret_cast<const v4f64*>(Lr + 16 * kb);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const double* xr = Xb + (size_t)(16 * kb + 4 * fk + s) * ld;
        acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(l4[s], xr[0], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(l4[s], two ? xr[16] : 0.0, acc1, 0, 0, 0);
      }
    }
  } else {
    if (KIND == 4) {
      for (int kb = b; kb < f.nbo; ++kb) {      // (column block b of W starts at block row b)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const size_t k = (size_t)(16 * kb + 4 * fk + s) * ld;
          const double w = X[k + 16 * b + pr];
          acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(w, Xb[k], acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(w, two ? Xb[k + 16] : 0.0, acc1, 0, 0, 0);
        }
      }
    }
    // the rows of Sigma this lane carries as the A operand: border row (kind 3) or own row (kind 4: the mirrored Sigma_OB) x border columns
    const int arow = KIND == 3 ? f.nI + min(16 * b + pr, f.st - 1) : 16 * b + pr;
    const double* Sr = a.S + f.moff + (size_t)arow * ld + f.nI + 4 * fk;
    const double* Tb = Xb + (size_t)f.nI * ld;
    const int nkb = (f.st + 15) / 16;
    for (int kb = 0; kb < nkb; ++kb) {
      const v4f64 g4 = *reinterpret_cast<const v4f64*>(Sr + 16 * kb);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const double* tr = Tb + (size_t)(16 * kb + 4 * fk + s) * ld;
        acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(-g4[s], tr[0], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(-g4[s], two ? tr[16] : 0.0, acc1, 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int i = 16 * b + 4 * fk + s;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      if (t == 1 && !two) continue;
      const int j = 16 * (jb0 + t) + n;
      const double v = t ? acc1[s] : acc0[s];
      if (KIND == 2) {
        if (i < f.st) a.X[f.moff + (size_t)(f.nI + i) * ld + j] = v;
      } else if (KIND == 3) {
        if (i < f.st) { a.S[f.moff + (size_t)(f.nI + i) * ld + j] = v; a.S[f.moff + (size_t)j * ld + f.nI + i] = v; }
      } else if (j <= i) {
        a.S[f.moff + (size_t)i * ld + j] = v; a.S[f.moff + (size_t)j * ld + i] = v;
      }
    }
  }
}

// ---- vector form: the whole front in one workgroup; the phases are ordered by the workgroup's barriers
__device__ __forceinline__ void sel_front_vec(const SelArgs& a, const SelFront& f) {
  const int tid = threadIdx.x, n = f.own, st = f.st;
  const size_t ld = (size_t)f.ld;
  const double* L = a.M + f.moff;
  const double* D = a.Linv + f.linv;
  double* X = a.X + f.moff;
  double* S = a.S + f.moff;
  // W: thread per column, block row by block row with the block inverses
  for (int c = tid; c < n; c += 256) {
    for (int i = c >> 4; i < f.nbo; ++i) {
      double v[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        double s = 16 * i + r == c ? 1.0 : 0.0;
        const double* Lr = L + (size_t)(16 * i + r) * ld;
        for (int k = c; k < 16 * i; ++k) s -= Lr[k] * X[(size_t)k * ld + c];
        v[r] = s;
      }
      const double* Di = D + (size_t)(i >> 3) * kTile * kTile + (i & 7) * 256;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        double y = 0.0;
#pragma unroll
        for (int q = 0; q < 16; ++q) y += Di[r * 16 + q] * v[q];
        X[(size_t)(16 * i + r) * ld + c] = y;
      }
    }
  }
  __syncthreads();
  for (int e = tid; e < st * n; e += 256) {   // T = L_BO W
    const int t = e / n, c = e - t * n;
    const double* Lr = L + (size_t)(f.nI + t) * ld;
    double s = 0.0;
    for (int k = c; k < n; ++k) s += Lr[k] * X[(size_t)k * ld + c];
    X[(size_t)(f.nI + t) * ld + c] = s;
  }
  __syncthreads();
  for (int e = tid; e < st * n; e += 256) {   // Sigma_BO = -Sigma_BB T
    const int t = e / n, c = e - t * n;
    const double* Gr = S + (size_t)(f.nI + t) * ld + f.nI;
    double s = 0.0;
    for (int k = 0; k < st; ++k) s -= Gr[k] * X[(size_t)(f.nI + k) * ld + c];
    S[(size_t)(f.nI + t) * ld + c] = s;
    S[(size_t)c * ld + f.nI + t] = s;
  }
  __syncthreads();
  for (int e = tid; e < n * n; e += 256) {    // Sigma_OO = W^T W - Sigma_OB T
    const int i = e / n, j = e - i * n;
    if (j > i) continue;
    double s = 0.0;
    for (int k = i; k < n; ++k) s += X[(size_t)k * ld + i] * X[(size_t)k * ld + j];
    const double* Gr = S + (size_t)i * ld + f.nI;
    for (int k = 0; k < st; ++k) s -= Gr[k] * X[(size_t)(f.nI + k) * ld + j];
    S[(size_t)i * ld + j] = s;
    S[(size_t)j * ld + i] = s;
  }
}

template <int KIND>
__global__ __launch_bounds__(256) void k_selinv_step(SelArgs a, int item0) {
  const int4 it = a.items[item0 + (int)blockIdx.x];
  const SelFront f = a.fr[it.x];
  if (KIND == 1) sel_winv_mfma(a, f, it.z);
  else if (KIND == 5) sel_front_vec(a, f);
  else sel_prod_mfma<KIND>(a, f, it.z, it.w);
}

// out[e] = Sigma[src[e]] (src < 0: an entry that is not stored, or of a constant pose: zero)
__global__ __launch_bounds__(256) void k_selinv_read(const double* __restrict__ S, const long long* __restrict__ src, double* __restrict__ out, long long n) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) out[e] = src[e] >= 0 ? S[src[e]] : 0.0;
}

void launch_selinv_gather(const SelArgs& a, int item0, int count, hipStream_t st) {
  if (count > 0) hipLaunchKernelGGL(k_selinv_gather, dim3(count), dim3(256), 0, st, a, item0);
}
void launch_selinv_step(const SelArgs& a, int item0, int count, int kind, hipStream_t st) {
  if (count <= 0) return;
  switch (kind) {
    case 1: hipLaunchKernelGGL(k_selinv_step<1>, dim3(count), dim3(256), 0, st, a, item0); break;
    case 2: hipLaunchKernelGGL(k_selinv_step<2>, dim3(count), dim3(256), 0, st, a, item0); break;
    case 3: hipLaunchKernelGGL(k_selinv_step<3>, dim3(count), dim3(256), 0, st, a, item0); break;
    case 4: hipLaunchKernelGGL(k_selinv_step<4>, dim3(count), dim3(256), 0, st, a, item0); break;
    default: hipLaunchKernelGGL(k_selinv_step<5>, dim3(count), dim3(256), 0, st, a, item0); break;
  }
}
void launch_selinv_read(const double* S, const long long* src, double* out, long long n, hipStream_t st) {
  if (n > 0) hipLaunchKernelGGL(k_selinv_read, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, S, src, out, n);
}

}  // namespace covgpu
