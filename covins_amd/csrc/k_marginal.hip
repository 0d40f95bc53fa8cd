// k_marginal.hip — the sweep behind covgpu_marginal_covariance: columns of L^-1 E for the unit columns E of the chosen
// unknowns, through the factored fronts of the multifrontal solve (k_front.hip) as launch_nd_solve left them, and their Gram matrix.
//
// L^-1 e_j is non-zero only on the fronts of the path from the front that owns unknown j to the root, so with the columns in the post-order
// of their owners every front works on ONE contiguous range of columns, and at a level of the tree no two fronts touch the same column: the
// update of a front's border rows never meets a sibling's — plain stores, no atomics, one summation order.
// A front of `own` own unknowns is swept in panels of 128 columns, each panel in two launches shared by all fronts of the level:
//   kind 0   Y_p = L_pp^-1 V_p: the panel's rows, block row by block row with the 16x16 block inverses the factorisation left (the mirror of
//            k_bwd_step_sub); one workgroup per front, its waves take the 16-column chunks of the range — a chunk's chain is independent of
//            the others', and the front's tile of L comes from HBM once for all of them
//   kind 1/2 V[rows below] -= L[rows, panel] Y_p: one workgroup per 16 rows (own rows below the panel | border rows, which live in the
//            ancestors' part of the working matrix), every tile of L read once for all columns of the range
// Two forms of both: ranges of 16 columns and more run on v_mfma_f64_16x16x4_f64 (operands as in k_panel.hip: A lane n carries logical row
// 4 (n & 3) + (n >> 2), k-slot (lane >> 4, s) carries k = 4 (lane >> 4) + s, so every A operand is one 32-byte load and the accumulator of one
// product is the B operand of the next); narrower ranges stage the 16 x 128 block of L and the panel of Y in LDS through whole-line loads and
// run one thread per (row, column).
// The front layout read here is the one k_bwd_step_sub / k_bwd_front read: full squares at the front's (offset, leading dimension), own rows
// first, border rows from the level's padded interior order nI on, eight 16x16 block inverses per 128-tile in nd_Linv. Leaf fronts factored
// by k_potrf_leaf have the same layout in memory (leaf_front.hpp).
#include "marginal.hpp"

namespace covgpu {

typedef double v4f64 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void k_marg_seed(double* __restrict__ W, int mp, int m, const int* __restrict__ seed_row) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s < m) W[(size_t)seed_row[s] * mp + s] = 1.0;
}

// ---- matrix-core form
__device__ __forceinline__ void marg_diag_mfma(const MargArgs& a, const MargFront& f, int p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, fk = lane >> 4, pr = 4 * (n & 3) + (n >> 2);
  const int k0 = p * kMargPanel, nb = min(8, f.nbo - 8 * p), mp = a.mp;
  const double* Lp = a.M + f.moff + (size_t)k0 * f.ld + k0;          // the panel's diagonal tile
  const double* Dp = a.Linv + f.linv + (size_t)p * kTile * kTile;    // its eight block inverses
  double* Wp = a.W + (size_t)(f.wbase + k0) * mp;
  const int nch = (f.c1 - f.c0 + kMargBlock - 1) / kMargBlock;
  for (int ch = wave; ch < nch; ch += 4) {
    const int col = f.c0 + kMargBlock * ch + n;
    const bool ok = col < f.c1;
    v4f64 y[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (i < nb) {
        v4f64 acc;
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[s] = ok ? Wp[(size_t)(16 * i + 4 * fk + s) * mp + col] : 0.0;
#pragma unroll
        for (int j = 0; j < i; ++j) {
          const v4f64 l4 = *reinterpret_cast<const v4f64*>(Lp + (size_t)(16 * i + pr) * f.ld + 16 * j + 4 * fk);
#pragma unroll
          for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-l4[s], y[j][s], acc, 0, 0, 0);
        }
        const v4f64 d4 = *reinterpret_cast<const v4f64*>(Dp + i * 256 + pr * 16 + 4 * fk);
        v4f64 z = v4f64{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < 4; ++s) z = __builtin_amdgcn_mfma_f64_16x16x4f64(d4[s], acc[s], z, 0, 0, 0);
        y[i] = z;
        if (ok) {
#pragma unroll
          for (int s = 0; s < 4; ++s) Wp[(size_t)(16 * i + 4 * fk + s) * mp + col] = z[s];
        }
      } else y[i] = v4f64{0.0, 0.0, 0.0, 0.0};
    }
  }
}

// rows: kind 1 the own rows of block `blk` | kind 2 the border rows of block `blk`
__device__ __forceinline__ void marg_update_mfma(const MargArgs& a, const MargFront& f, int p, int kind, int blk) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, fk = lane >> 4, pr = 4 * (n & 3) + (n >> 2);
  const int k0 = p * kMargPanel, nb = min(8, f.nbo - 8 * p), mp = a.mp;
  const double* Wp = a.W + (size_t)(f.wbase + k0) * mp;
  // the row of L this lane carries as the A operand (a border row past the front's last one: any real row, its results are not stored)
  const int lrow = kind == 1 ? 16 * blk + pr : f.nI + min(16 * blk + pr, f.st - 1);
  const double* Lr = a.M + f.moff + (size_t)lrow * f.ld + k0 + 4 * fk;
  long long wr[4];   // rows of W behind the four accumulator entries (-1: none)
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int i = 16 * blk + 4 * fk + s;
    wr[s] = kind == 1 ? (long long)(f.wbase + i) : (i < f.st ? (long long)a.bmap[f.bmap + i] : -1ll);
  }
  const int nch = (f.c1 - f.c0 + kMargBlock - 1) / kMargBlock;
  for (int ch = wave; ch < nch; ch += 4) {
    const int col = f.c0 + kMargBlock * ch + n;
    const bool ok = col < f.c1;
    v4f64 acc;
#pragma unroll
    for (int s = 0; s < 4; ++s) acc[s] = (ok && wr[s] >= 0) ? a.W[(size_t)wr[s] * mp + col] : 0.0;
    for (int j = 0; j < nb; ++j) {
      const v4f64 l4 = *reinterpret_cast<const v4f64*>(Lr + 16 * j);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const double b = ok ? Wp[(size_t)(16 * j + 4 * fk + s) * mp + col] : 0.0;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-l4[s], b, acc, 0, 0, 0);
      }
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) if (ok && wr[s] >= 0) a.W[(size_t)wr[s] * mp + col] = acc[s];
  }
}

// ---- vector form (ranges of fewer than 16 columns): thread (r, cn) owns entry (row r of the block, column c0 + cn)
struct MargLds { double Y[kMargPanel][17]; double L[16][kMargPanel + 1]; double D[16][17]; double V[16][17]; };

__device__ __forceinline__ void marg_diag_vec(const MargArgs& a, const MargFront& f, int p, MargLds& S) {
  const int tid = threadIdx.x, r = tid >> 4, cn = tid & 15;
  const int k0 = p * kMargPanel, nb = min(8, f.nbo - 8 * p), mp = a.mp;
  const double* Lp = a.M + f.moff + (size_t)k0 * f.ld + k0;
  const double* Dp = a.Linv + f.linv + (size_t)p * kTile * kTile;
  double* Wp = a.W + (size_t)(f.wbase + k0) * mp;
  const int col = f.c0 + cn;
  const bool ok = col < f.c1;
  for (int i = 0; i < nb; ++i) {
    const int w = 16 * i;   // columns of block row i left of its diagonal block
    for (int e = tid; e < 16 * w; e += 256) { const int rr = e / w, kk = e - rr * w; S.L[rr][kk] = Lp[(size_t)(16 * i + rr) * f.ld + kk]; }
    S.D[r][cn] = Dp[i * 256 + r * 16 + cn];
    double v = ok ? Wp[(size_t)(16 * i + r) * mp + col] : 0.0;
    __syncthreads();
    for (int k = 0; k < w; ++k) v -= S.L[r][k] * S.Y[k][cn];
    S.V[r][cn] = v;
    __syncthreads();
    double y = 0.0;
#pragma unroll
    for (int k = 0; k < 16; ++k) y += S.D[r][k] * S.V[k][cn];
    S.Y[16 * i + r][cn] = y;
    if (ok) Wp[(size_t)(16 * i + r) * mp + col] = y;
    __syncthreads();
  }
}

__device__ __forceinline__ void marg_update_vec(const MargArgs& a, const MargFront& f, int p, int kind, int blk, MargLds& S) {
  const int tid = threadIdx.x, r = tid >> 4, cn = tid & 15;
  const int k0 = p * kMargPanel, kw = 16 * min(8, f.nbo - 8 * p), mp = a.mp;
  const double* Wp = a.W + (size_t)(f.wbase + k0) * mp;
  const int col = f.c0 + cn;
  const bool ok = col < f.c1;
  const int nrow = kind == 1 ? 16 : max(0, min(16, f.st - 16 * blk));   // real rows of the block
  const size_t row0 = kind == 1 ? (size_t)16 * blk : (size_t)f.nI + 16 * blk;
  const double* Lb = a.M + f.moff + row0 * f.ld + k0;
  for (int e = tid; e < 16 * kw; e += 256) { const int rr = e / kw, kk = e - rr * kw; S.L[rr][kk] = rr < nrow ? Lb[(size_t)rr * f.ld + kk] : 0.0; }
  for (int e = tid; e < 16 * kw; e += 256) { const int k = e >> 4, c = e & 15; S.Y[k][c] = f.c0 + c < f.c1 ? Wp[(size_t)k * mp + f.c0 + c] : 0.0; }
  __syncthreads();
  if (!ok || r >= nrow) return;
  const size_t wrow = kind == 1 ? (size_t)(f.wbase + 16 * blk + r) : (size_t)a.bmap[f.bmap + 16 * blk + r];
  double v = a.W[wrow * mp + col];
  for (int k = 0; k < kw; ++k) v -= S.L[r][k] * S.Y[k][cn];
  a.W[wrow * mp + col] = v;
}

template <bool MFMA>
__global__ __launch_bounds__(256) void k_marg_step(MargArgs a, int item0) {
  const int4 it = a.items[item0 + (int)blockIdx.x];
  const MargFront f = a.fr[it.x];
  if (MFMA) {
    if (it.z == 0) marg_diag_mfma(a, f, it.y); else marg_update_mfma(a, f, it.y, it.z, it.w);
  } else {
    __shared__ MargLds S;
    if (it.z == 0) marg_diag_vec(a, f, it.y, S); else marg_update_vec(a, f, it.y, it.z, it.w, S);
  }
}

// cov[perm[a]][perm[b]] = sum over the rows of W of W[row][a] W[row][b], fronts in level order, rows in order; a front outside whose range one
// of the two columns lies holds zeros there and is skipped. One workgroup per 16x16 tile of the lower triangle; an entry below the diagonal is
// stored at both places.
__global__ __launch_bounds__(256) void k_marg_gram(const double* __restrict__ W, int mp, const MargFront* __restrict__ fr, int nf,
                                                    const int* __restrict__ perm, int m, double* __restrict__ cov) {
  int ta = 0;
  while ((ta + 1) * (ta + 2) / 2 <= (int)blockIdx.x) ++ta;
  const int tb = (int)blockIdx.x - ta * (ta + 1) / 2;
  const int a = 16 * ta + (threadIdx.x >> 4), b = 16 * tb + (threadIdx.x & 15);
  double acc = 0.0;
  for (int q = 0; q < nf; ++q) {
    const int c0 = fr[q].c0, c1 = fr[q].c1;
    if (c0 >= 16 * tb + 16 || c1 <= 16 * tb || c0 >= 16 * ta + 16 || c1 <= 16 * ta) continue;
    const double* Wr = W + (size_t)fr[q].wbase * mp;
    const int own = fr[q].own;
    for (int r = 0; r < own; ++r) acc += Wr[(size_t)r * mp + a] * Wr[(size_t)r * mp + b];
  }
  if (a < m && b <= a) {
    const size_t pa = (size_t)perm[a], pb = (size_t)perm[b];
    cov[pa * m + pb] = acc;
    cov[pb * m + pa] = acc;
  }
}

void launch_marg_seed(double* W, int mp, int m, const int* seed_row, hipStream_t st) {
  hipLaunchKernelGGL(k_marg_seed, dim3((m + 255) / 256), dim3(256), 0, st, W, mp, m, seed_row);
}
void launch_marg_step(const MargArgs& a, int item0, int count, bool mfma, hipStream_t st) {
  if (count <= 0) return;
  if (mfma) hipLaunchKernelGGL(k_marg_step<true>, dim3(count), dim3(256), 0, st, a, item0);
  else hipLaunchKernelGGL(k_marg_step<false>, dim3(count), dim3(256), 0, st, a, item0);
}
void launch_marg_gram(const double* W, int mp, const MargFront* fr, int nf, const int* perm, int m, double* cov, hipStream_t st) {
  const int T = mp / kMargBlock;
  hipLaunchKernelGGL(k_marg_gram, dim3(T * (T + 1) / 2), dim3(256), 0, st, W, mp, fr, nf, perm, m, cov);
}

}  // namespace covgpu
