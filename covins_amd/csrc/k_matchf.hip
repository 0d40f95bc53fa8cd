// k_matchf.hip — batched brute-force L2 matching of float (SIFT) descriptors for COVINS-G's loop candidates: the exact
// search behind cv::BFMatcher(NORM_L2).knnMatch(k = 2) + distance and ratio tests (placerec_gen_be.cpp:82-114 and
// RelNonCentralPosSolver.cpp:303-340, feat.type SIFT), with d2(a, b) = max(0, (|a|^2 + |b|^2) - 2 dot(a, b)) in float32.
//
// k_matchf_norms: |x|^2 of every row once, a k-ordered fmaf chain.
// k_matchf_scan<KP>: a 256-thread workgroup owns 128 query ("A") rows of one job, 32 per wave. dot(a, b) runs on
// v_mfma_f32_32x32x2_f32, which is bit for bit the k-ordered fmaf chain from 0: the wave's 32 query rows are the column operand and stay
// in KP registers (lane (r, h) holds the dimensions of parity h of row r), the job's train ("B") rows stream through LDS in chunks of 64
// as the row operand, stored dimension-major so that a wave's operand read is one conflict-free ds_read_b32. A lane then holds 16
// train-row distances of ONE query row (col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)) in ascending row order, and
// keeps its running top-2 by (d2, index) in registers; the two half-waves are merged once at the end (the order is total, so the merge
// is exact), and threshold, ratio test, match, dist and nmatches finish in the same launch. The next chunk's rows are loaded into
// registers before the scan of the current chunk and written to LDS after it, so the scan hides their latency. KP (dimension pairs held, 32 / 64 / 128)
// covers dim <= 64 / 128 / 256; dimensions past dim are zero in both operands and the k loop ends at dim rounded up to 32.
#include <cmath>

#include "common.hpp"

namespace covgpu {

namespace {

constexpr int kScanThreadsF = 256;
constexpr int kQTile = kMatchFloatTileRows;     // query rows per workgroup: 4 waves of 32
constexpr int kBChunk = kMatchFloatChunkRows;   // train rows staged per chunk: two 32-row MFMA blocks
static_assert(kQTile == 32 * (kScanThreadsF / 64) && kBChunk == 64, "k_matchf_scan's index arithmetic");

using f32x16 = __attribute__((ext_vector_type(16))) float;

struct MatchFArgs {
  const float* desc;                  // [rows][dim]
  const float* norm;                  // [rows] |x|^2
  const int* row_ptr;
  const int* set_a;
  const int* set_b;
  const int* out_off;                 // [num_jobs] first output row of job j
  int* match;                         // [sum nA]
  float* dist;                        // [sum nA] or nullptr
  int* nmatches;                      // [num_jobs], zeroed before the launch
  int dim;
  int tiles;                          // A tiles per job
  float thr, ratio;
};

__global__ __launch_bounds__(kScanThreadsF) void k_matchf_norms(const float* __restrict__ desc, float* __restrict__ norm, int rows, int dim) {
  const int r = blockIdx.x * kScanThreadsF + (int)threadIdx.x;
  if (r >= rows) return;
  const float4* p = reinterpret_cast<const float4*>(desc + (size_t)r * dim);
  float s = 0.0f;
  for (int t = 0; t < dim / 4; ++t) {
    const float4 v = p[t];
    s = fmaf(v.x, v.x, s); s = fmaf(v.y, v.y, s); s = fmaf(v.z, v.z, s); s = fmaf(v.w, v.w, s);
  }
  norm[r] = s;
}

// (d, e) before (od, oe) in the order by (distance, index)
__device__ __forceinline__ bool before(float d, int e, float od, int oe) { return d < od || (d == od && e < oe); }

template <int KP>
__global__ __launch_bounds__(kScanThreadsF) void k_matchf_scan(MatchFArgs M) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* sB = smem;                                      // [2 KP][64]: dimension k, train row j at k * 64 + (j ^ 32 (k & 1))
  float* sN = smem + 2 * KP * kBChunk;                    // [64] |b|^2, +inf for the padding past the chunk's end
  const int job = blockIdx.x / M.tiles, tile = blockIdx.x % M.tiles;
  const int a0 = M.row_ptr[M.set_a[job]], nA = M.row_ptr[M.set_a[job] + 1] - a0;
  const int b0 = M.row_ptr[M.set_b[job]], nB = M.row_ptr[M.set_b[job] + 1] - b0;
  if (tile * kQTile >= nA) return;                        // uniform over the workgroup
  const int dim = M.dim, dimp = (dim + 31) & ~31;        // the k loop runs in groups of 32 dimensions, zero past dim
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const int ia = tile * kQTile + wave * 32 + r;
  const bool live = ia < nA;
  const bool wave_live = tile * kQTile + wave * 32 < nA;  // uniform over the wave
  // the query row's dimensions of parity h: q[s] = a[2 s + h], the B operand of k step s
  float q[KP];
  {
    const float4* qa = reinterpret_cast<const float4*>(M.desc + (size_t)(a0 + (live ? ia : 0)) * dim);
#pragma unroll
    for (int t = 0; t < KP / 2; ++t) {
      float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (live && 4 * t < dim) v = qa[t];
      q[2 * t] = h ? v.y : v.x; q[2 * t + 1] = h ? v.w : v.z;
    }
  }
  const float na = live ? M.norm[a0 + ia] : 0.0f;
  const float inf = __builtin_inff();
  float d0 = inf, d1 = inf;                              // squared distances of the best and the second best, (d2, index) ascending
  int e0 = -1, e1 = -1;
  const int srow = tid & 63, st0 = tid >> 6;             // staging: a wave writes 64 consecutive rows of one dimension (conflict-free)
  // the next chunk's rows travel through registers: loaded before the scan of the current chunk, written to LDS after it
  float4 pre[KP / 8];
  float pren = inf;
  auto fetch = [&](int c) {
    const int nc = min(kBChunk, nB - c);
    const float4* pb = reinterpret_cast<const float4*>(M.desc + (size_t)(b0 + c + (srow < nc ? srow : 0)) * dim);
#pragma unroll
    for (int i = 0; i < KP / 8; ++i) {
      const int t = st0 + (kScanThreadsF / 64) * i;
      pre[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);      // padding rows are zero: their dot stays finite, their norm makes them +inf
      if (srow < nc && 4 * t < dim) pre[i] = pb[t];
    }
    if (tid < kBChunk) pren = tid < nc ? M.norm[b0 + c + tid] : inf;
  };
  if (nB > 0) fetch(0);
  for (int c = 0; c < nB; c += kBChunk) {
    const int nc = min(kBChunk, nB - c);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < KP / 8; ++i) {
      const int t = st0 + (kScanThreadsF / 64) * i;
      if (4 * t < dimp) {
        float* o = sB + 4 * t * kBChunk;
        o[srow] = pre[i].x; o[kBChunk + (srow ^ 32)] = pre[i].y; o[2 * kBChunk + srow] = pre[i].z; o[3 * kBChunk + (srow ^ 32)] = pre[i].w;
      }
    }
    if (tid < kBChunk) sN[tid] = pren;
    __syncthreads();
    if (c + kBChunk < nB) fetch(c + kBChunk);
    if (!wave_live) continue;
    for (int blk = 0; blk * 32 < nc; ++blk) {
      f32x16 acc;
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
      const float* p = sB + h * kBChunk + ((blk * 32 + r) ^ (h * 32));
#pragma unroll
      for (int g = 0; g < KP / 16; ++g) {
        if (32 * g < dim) {                              // uniform: the k loop ends at dim rounded up to 32
#pragma unroll
          for (int s = 16 * g; s < 16 * g + 16; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(p[2 * s * kBChunk], q[s], acc, 0, 0, 0);
        }
      }
      float dd[16];
      float m = inf;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 nb = *reinterpret_cast<const float4*>(sN + blk * 32 + 8 * g + 4 * h);
        dd[4 * g + 0] = fmaxf(0.0f, (na + nb.x) - 2.0f * acc[4 * g + 0]);
        dd[4 * g + 1] = fmaxf(0.0f, (na + nb.y) - 2.0f * acc[4 * g + 1]);
        dd[4 * g + 2] = fmaxf(0.0f, (na + nb.z) - 2.0f * acc[4 * g + 2]);
        dd[4 * g + 3] = fmaxf(0.0f, (na + nb.w) - 2.0f * acc[4 * g + 3]);
        m = fminf(m, fminf(fminf(dd[4 * g], dd[4 * g + 1]), fminf(dd[4 * g + 2], dd[4 * g + 3])));
      }
      if (!(m < d1)) continue;                           // the rare inserts, in ascending row order: an equal distance never displaces
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float d = dd[i];
        const int j = c + blk * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
        if (d < d1) {
          if (d < d0) { e1 = e0; d1 = d0; e0 = j; d0 = d; } else { e1 = j; d1 = d; }
        }
      }
    }
  }
  if (!wave_live) return;
  // lanes r and r + 32 hold disjoint train rows of the same query row: merge the two sorted pairs
  {
    const float od0 = __shfl_xor(d0, 32), od1 = __shfl_xor(d1, 32);
    const int oe0 = __shfl_xor(e0, 32), oe1 = __shfl_xor(e1, 32);
    if (before(od0, oe0, d0, e0)) {
      const bool mine = before(d0, e0, od1, oe1);
      d1 = mine ? d0 : od1; e1 = mine ? e0 : oe1;
      d0 = od0; e0 = oe0;
    } else if (before(od0, oe0, d1, e1)) {
      d1 = od0; e1 = oe0;
    }
  }
  const float f0 = sqrtf(d0), f1 = sqrtf(d1);
  const bool ok = live && h == 0 && nB >= 2 && f0 <= M.thr && f0 < M.ratio * f1;
  if (live && h == 0) {
    const size_t o = (size_t)M.out_off[job] + ia;
    M.match[o] = ok ? e0 : -1;
    if (M.dist) M.dist[o] = ok ? f0 : -1.0f;
  }
  const unsigned long long bal = __ballot(ok);
  if (lane == 0 && bal) atomicAdd(&M.nmatches[job], (int)__popcll(bal));
}

template <int KP>
void launch_scan(const MatchFArgs& M, dim3 grid, hipStream_t st) {
  const size_t lds = matchf_lds_bytes(KP);
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_matchf_scan<KP>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(k_matchf_scan<KP>, grid, dim3(kScanThreadsF), lds, st, M);
}

}  // namespace

size_t matchf_lds_bytes(int kp) { return sizeof(float) * ((size_t)2 * kp * kBChunk + kBChunk); }

void launch_matchf_norms(int rows, int dim, const float* desc, float* norm, hipStream_t st) {
  if (rows <= 0) return;
  hipLaunchKernelGGL(k_matchf_norms, dim3((unsigned)((rows + kScanThreadsF - 1) / kScanThreadsF)), dim3(kScanThreadsF), 0, st, desc, norm, rows, dim);
}

void launch_matchf(int num_jobs, int maxA, int dim, const float* desc, const float* norm, const int* row_ptr, const int* set_a,
                   const int* set_b, const int* out_off, int* match, float* dist, int* nmatches, float thr, float ratio, hipStream_t st) {
  if (num_jobs <= 0 || maxA <= 0) return;
  const int tiles = (maxA + kQTile - 1) / kQTile;
  const MatchFArgs M{desc, norm, row_ptr, set_a, set_b, out_off, match, dist, nmatches, dim, tiles, thr, ratio};
  const dim3 grid((unsigned)((int64_t)num_jobs * tiles));           // covgpu_match_float_batch keeps num_jobs * tiles <= 2^31 - 1
  if (dim <= 64) launch_scan<32>(M, grid, st);
  else if (dim <= 128) launch_scan<64>(M, grid, st);
  else launch_scan<128>(M, grid, st);
}

}  // namespace covgpu
