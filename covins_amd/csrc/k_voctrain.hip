// k_voctrain.hip — one level of DBoW2's hierarchical k-means (TemplatedVocabulary::HKmeansStep / initiateClustersKMpp, FORB::meanValue /
// distance) for every node of the level at once, and the per-set unique word count behind setNodeWeights.
//
// The rows of the level are a permutation grouped by node ("segment"); a tile is a run of positions of one segment that one group of
// threads works. Every kernel takes its group size from blockDim.x, so the same code serves both forms: a workgroup of kVtThreads per
// tile of at most kVtTile rows (a segment above kVtWaveMax rows; above kVtTile it spreads over several workgroups), and one wavefront
// per segment of at most kVtWaveMax rows. All arithmetic is integer, every atomic is an integer atomic, and every loop is bounded by a
// data size: nothing waits on another workgroup. The host (voctrain.hip) drives the rounds and reads one word per k-means iteration.
#include "common.hpp"

namespace covgpu {

namespace {

constexpr int kMaxG = kVtThreads;
constexpr int kRedraws = 64;                      // draws of one cut_d (D1)

__device__ __forceinline__ unsigned long long vt_mix(unsigned long long x) {   // splitmix64, as in k_abspose.hip
  unsigned long long z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// draw j of the node with this key, in [0, 1)
__device__ __forceinline__ double vt_unit(unsigned long long key, int j) {
  const unsigned long long r = vt_mix(vt_mix(key) + (unsigned long long)j);
  return (double)(r >> 11) * 0x1.0p-53;
}

__device__ __forceinline__ int vt_hamming(const uint4& a0, const uint4& a1, const uint4& b0, const uint4& b1) {
  return __builtin_popcount(a0.x ^ b0.x) + __builtin_popcount(a0.y ^ b0.y) + __builtin_popcount(a0.z ^ b0.z) +
         __builtin_popcount(a0.w ^ b0.w) + __builtin_popcount(a1.x ^ b1.x) + __builtin_popcount(a1.y ^ b1.y) +
         __builtin_popcount(a1.z ^ b1.z) + __builtin_popcount(a1.w ^ b1.w);
}

// the sum of v over the workgroup, in every thread (s: kMaxG ints of LDS)
__device__ __forceinline__ unsigned vt_block_sum(unsigned v, unsigned* s) {
  const int tid = (int)threadIdx.x, G = (int)blockDim.x;
  s[tid] = v;
  __syncthreads();
  for (int off = G >> 1; off > 0; off >>= 1) {
    if (tid < off) s[tid] += s[tid + off];
    __syncthreads();
  }
  const unsigned r = s[0];
  __syncthreads();
  return r;
}

// One thread per segment. A segment of at most k rows is its own result: one cluster per row, in order. Any other gets its first centre.
__global__ __launch_bounds__(kVtThreads) void k_vt_begin(VocTrainDev D) {
  const int s = blockIdx.x * kVtThreads + (int)threadIdx.x;
  if (s >= D.num_seg) return;
  const int n = D.seg_n[s], beg = D.seg_beg[s];
  D.changed[s] = 0; D.iters[s] = 0;
  uint4* cent = D.cent + (size_t)s * D.k * 2;
  if (n <= D.k) {
    for (int i = 0; i < n; ++i) {
      const size_t r = (size_t)D.perm[beg + i];
      cent[2 * i] = D.desc[2 * r]; cent[2 * i + 1] = D.desc[2 * r + 1];
      D.sizes[(size_t)s * D.k + i] = 1;
    }
    D.ncent[s] = n; D.draws[s] = 0; D.seed_done[s] = 1; D.done[s] = 1;
    return;
  }
  int idx = (int)(vt_unit(D.seg_key[s], 0) * (double)n);
  if (idx > n - 1) idx = n - 1;
  const size_t r = (size_t)D.perm[beg + idx];
  cent[0] = D.desc[2 * r]; cent[1] = D.desc[2 * r + 1];
  D.ncent[s] = 1; D.draws[s] = 1; D.seed_done[s] = 0; D.done[s] = 0;
}

// min_dists against the newest centre and their sum over the tile
__global__ __launch_bounds__(kVtThreads) void k_vt_seed_dist(VocTrainDev D, int tile0, int first_round) {
  __shared__ unsigned sRed[kMaxG];
  const int t = tile0 + (int)blockIdx.x;
  const int4 T = D.tiles[t];
  if (D.seed_done[T.x]) return;
  const uint4* c = D.cent + ((size_t)T.x * D.k + (D.ncent[T.x] - 1)) * 2;
  const uint4 c0 = c[0], c1 = c[1];
  unsigned sum = 0;
  for (int p = T.y + (int)threadIdx.x; p < T.z; p += (int)blockDim.x) {
    const size_t r = (size_t)D.perm[p];
    int d = vt_hamming(D.desc[2 * r], D.desc[2 * r + 1], c0, c1);
    if (!first_round) d = min(d, D.min_d[p]);
    D.min_d[p] = d;
    sum += (unsigned)d;
  }
  sum = vt_block_sum(sum, sRed);                  // at most kVtTile * 256 < 2^32
  if (threadIdx.x == 0) D.tile_sum[t] = sum;
}

// One thread per segment: dist_sum over the segment's tiles, cut_d, and the tile in which the prefix sum crosses it.
__global__ __launch_bounds__(kVtThreads) void k_vt_seed_cut(VocTrainDev D) {
  const int s = blockIdx.x * kVtThreads + (int)threadIdx.x;
  if (s >= D.num_seg || D.seed_done[s]) return;
  const int t0 = D.seg_tile0[s], nt = D.seg_ntiles[s];
  unsigned long long total = 0;
  for (int t = 0; t < nt; ++t) total += D.tile_sum[t0 + t];
  if (total == 0) {                               // every row equals a centre: fewer than k clusters
    D.seed_done[s] = 1;
    atomicAdd((unsigned long long*)&D.stats[4], 1ull);
    return;
  }
  int j = D.draws[s];
  double cut = 0.0;
  for (int tries = 0; tries < kRedraws; ++tries) {
    cut = vt_unit(D.seg_key[s], j++) * (double)total;
    if (cut != 0.0) break;
  }
  D.draws[s] = j;
  unsigned long long run = 0;
  int pick = nt - 1;
  for (int t = 0; t < nt; ++t) {
    const unsigned long long next = run + D.tile_sum[t0 + t];
    if ((double)next >= cut) { pick = t; break; }
    if (t < nt - 1) run = next;                   // (no crossing at all: the last tile, entered with the sum before it)
  }
  D.cut[s] = cut; D.pick_tile[s] = t0 + pick; D.pick_base[s] = run;
}

// The tile that holds the crossing scans its rows and appends the picked row as the segment's next centre.
__global__ __launch_bounds__(kVtThreads) void k_vt_seed_pick(VocTrainDev D, int tile0) {
  __shared__ unsigned sScan[kMaxG];
  __shared__ int sFound;
  const int t = tile0 + (int)blockIdx.x, tid = (int)threadIdx.x, G = (int)blockDim.x;
  const int4 T = D.tiles[t];
  const int s = T.x;
  if (D.seed_done[s] || D.pick_tile[s] != t) return;
  const double cut = D.cut[s];
  const int nc = D.ncent[s];
  unsigned long long run = D.pick_base[s];
  if (tid == 0) sFound = INT32_MAX;
  __syncthreads();
  for (int p0 = T.y; p0 < T.z; p0 += G) {
    const int p = p0 + tid;
    const unsigned v = p < T.z ? (unsigned)D.min_d[p] : 0u;
    sScan[tid] = v;
    __syncthreads();
    for (int off = 1; off < G; off <<= 1) {       // inclusive scan
      const unsigned a = tid >= off ? sScan[tid - off] : 0u;
      __syncthreads();
      sScan[tid] += a;
      __syncthreads();
    }
    if (p < T.z && (double)(run + sScan[tid]) >= cut) atomicMin(&sFound, p);
    run += sScan[G - 1];
    __syncthreads();
    if (sFound != INT32_MAX) break;               // uniform: read after the barrier
    __syncthreads();
  }
  const int pick = sFound != INT32_MAX ? sFound : T.z - 1;
  if (nc >= D.k) return;
  if (tid < 2) D.cent[((size_t)s * D.k + nc) * 2 + tid] = D.desc[2 * (size_t)D.perm[pick] + tid];
  if (tid == 0) { D.ncent[s] = nc + 1; if (nc + 1 >= D.k) D.seed_done[s] = 1; }
}

// Each row to the centre of least distance, the lowest index winning a tie; raises changed[seg] where a row moved.
__global__ __launch_bounds__(kVtThreads) void k_vt_assoc(VocTrainDev D, int tile0, int first) {
  __shared__ uint4 sC[kVtMaxK][2];
  const int t = tile0 + (int)blockIdx.x, tid = (int)threadIdx.x, G = (int)blockDim.x;
  const int4 T = D.tiles[t];
  const int s = T.x;
  if (D.done[s]) return;
  const int nc = D.ncent[s];
  for (int i = tid; i < 2 * nc; i += G) sC[i >> 1][i & 1] = D.cent[(size_t)s * D.k * 2 + i];
  __syncthreads();
  int moved = 0;
  for (int p = T.y + tid; p < T.z; p += G) {
    const size_t r = (size_t)D.perm[p];
    const uint4 q0 = D.desc[2 * r], q1 = D.desc[2 * r + 1];
    int best = 0, best_d = vt_hamming(q0, q1, sC[0][0], sC[0][1]);
    for (int c = 1; c < nc; ++c) {
      const int d = vt_hamming(q0, q1, sC[c][0], sC[c][1]);
      if (d < best_d) { best_d = d; best = c; }
    }
    if (!first && D.assoc[p] != best) moved = 1;
    D.assoc[p] = best;
  }
  if (moved) D.changed[s] = 1;                    // every writer stores the same value
}

// One thread per segment, after an association: count it, and retire the segment whose association repeated.
__global__ __launch_bounds__(kVtThreads) void k_vt_flags(VocTrainDev D, int first) {
  const int s = blockIdx.x * kVtThreads + (int)threadIdx.x;
  if (s >= D.num_seg || D.done[s]) return;
  D.iters[s] += 1;
  if (!first && !D.changed[s]) D.done[s] = 1;
  else *D.any = 1;
  D.changed[s] = 0;
}

// FORB::meanValue from 256 bit counters: a bit is set iff its count >= n / 2 + n % 2; an empty group keeps its centre (D2).
__device__ __forceinline__ unsigned vt_majority(const int* cnt, int n) {
  const int th = n / 2 + n % 2;
  unsigned w = 0;
  for (int b = 0; b < 32; ++b) w |= (unsigned)(cnt[b] >= th) << b;
  return w;
}

// Bit counts of each cluster over the tile: column j of the counters belongs to one thread, so the LDS adds need no atomics. A tile
// that is its whole segment writes the new centres itself; the tiles of a wider segment add into the segment's global counters.
__global__ __launch_bounds__(kVtThreads) void k_vt_means(VocTrainDev D, int tile0) {
  extern __shared__ int sDyn[];                   // [k][256] counters, [k] sizes, [G][8] rows, [G] clusters
  const int t = tile0 + (int)blockIdx.x, tid = (int)threadIdx.x, G = (int)blockDim.x;
  const int4 T = D.tiles[t];
  const int s = T.x;
  if (D.done[s]) return;
  const int nc = D.ncent[s];
  int* sCnt = sDyn;
  int* sN = sCnt + D.k * 256;
  unsigned* sRow = (unsigned*)(sN + D.k);
  int* sA = (int*)(sRow + G * 8);
  for (int i = tid; i < nc * 256; i += G) sCnt[i] = 0;
  for (int i = tid; i < nc; i += G) sN[i] = 0;
  __syncthreads();
  for (int p0 = T.y; p0 < T.z; p0 += G) {
    const int p = p0 + tid, m = min(G, T.z - p0);
    if (p < T.z) {
      const size_t r = (size_t)D.perm[p];
      const uint4 q0 = D.desc[2 * r], q1 = D.desc[2 * r + 1];
      unsigned* row = sRow + tid * 8;
      row[0] = q0.x; row[1] = q0.y; row[2] = q0.z; row[3] = q0.w; row[4] = q1.x; row[5] = q1.y; row[6] = q1.z; row[7] = q1.w;
      const int c = D.assoc[p];
      sA[tid] = c;
      atomicAdd(&sN[c], 1);
    }
    __syncthreads();
    for (int col = tid; col < 256; col += G) {
      const int w = col >> 5, b = col & 31;
      for (int i = 0; i < m; ++i) sCnt[sA[i] * 256 + col] += (int)((sRow[i * 8 + w] >> b) & 1u);
    }
    __syncthreads();
  }
  const int slot = D.seg_slot[s];
  if (slot < 0) {
    unsigned* cent = (unsigned*)(D.cent + (size_t)s * D.k * 2);
    for (int i = tid; i < nc * 8; i += G) {
      const int c = i >> 3, n = sN[c];
      if (n == 0) { if ((i & 7) == 0) atomicAdd((unsigned long long*)&D.stats[3], 1ull); continue; }
      cent[i] = vt_majority(sCnt + c * 256 + (i & 7) * 32, n);
    }
  } else {
    for (int i = tid; i < nc * 256; i += G) if (sCnt[i]) atomicAdd(&D.gcnt[(size_t)slot * D.k * 256 + i], sCnt[i]);
    for (int i = tid; i < nc; i += G) if (sN[i]) atomicAdd(&D.gsize[(size_t)slot * D.k + i], sN[i]);
  }
}

// One thread per (slot, cluster, dword) of the segments wider than a tile.
__global__ __launch_bounds__(kVtThreads) void k_vt_means_final(VocTrainDev D) {
  const int i = blockIdx.x * kVtThreads + (int)threadIdx.x;
  if (i >= D.num_slots * D.k * 8) return;
  const int slot = i / (D.k * 8), c = (i >> 3) % D.k, w = i & 7, s = D.slot_seg[slot];
  if (D.done[s] || c >= D.ncent[s]) return;
  const int n = D.gsize[(size_t)slot * D.k + c];
  if (n == 0) { if (w == 0) atomicAdd((unsigned long long*)&D.stats[3], 1ull); return; }
  ((unsigned*)(D.cent + (size_t)s * D.k * 2))[c * 8 + w] = vt_majority(D.gcnt + ((size_t)slot * D.k + c) * 256 + w * 32, n);
}

// Stable partition of every segment by cluster, in three steps: the tiles' cluster counts, ...
__global__ __launch_bounds__(kVtThreads) void k_vt_part_count(VocTrainDev D, int tile0) {
  __shared__ int sN[kVtMaxK];
  const int t = tile0 + (int)blockIdx.x, tid = (int)threadIdx.x, G = (int)blockDim.x;
  const int4 T = D.tiles[t];
  for (int i = tid; i < D.k; i += G) sN[i] = 0;
  __syncthreads();
  for (int p = T.y + tid; p < T.z; p += G) atomicAdd(&sN[D.assoc[p]], 1);
  __syncthreads();
  for (int i = tid; i < D.k; i += G) D.tile_cnt[(size_t)t * D.k + i] = sN[i];
}

// ... one thread per segment turns them into each tile's first output position per cluster, and the cluster sizes, ...
__global__ __launch_bounds__(kVtThreads) void k_vt_part_offsets(VocTrainDev D) {
  const int s = blockIdx.x * kVtThreads + (int)threadIdx.x;
  if (s >= D.num_seg || D.seg_n[s] <= D.k) return;
  const int t0 = D.seg_tile0[s], nt = D.seg_ntiles[s];
  int run = D.seg_beg[s];
  for (int c = 0; c < D.k; ++c) {
    const int at = run;
    for (int t = 0; t < nt; ++t) {
      int* e = D.tile_cnt + (size_t)(t0 + t) * D.k + c;
      const int n = *e;
      *e = run; run += n;
    }
    D.sizes[(size_t)s * D.k + c] = run - at;
  }
}

// ... and the rows move, each behind the rows of its cluster that precede it.
__global__ __launch_bounds__(kVtThreads) void k_vt_part_scatter(VocTrainDev D, int tile0) {
  __shared__ int sBase[kVtMaxK];
  __shared__ int sA[kMaxG];
  const int t = tile0 + (int)blockIdx.x, tid = (int)threadIdx.x, G = (int)blockDim.x;
  const int4 T = D.tiles[t];
  for (int i = tid; i < D.k; i += G) sBase[i] = D.tile_cnt[(size_t)t * D.k + i];
  __syncthreads();
  for (int p0 = T.y; p0 < T.z; p0 += G) {
    const int p = p0 + tid, m = min(G, T.z - p0);
    const int c = p < T.z ? D.assoc[p] : -1;
    sA[tid] = c;
    __syncthreads();
    if (c >= 0) {
      int rank = 0;
      for (int i = 0; i < tid; ++i) rank += sA[i] == c;
      D.perm_out[sBase[c] + rank] = D.perm[p];
    }
    __syncthreads();
    for (int i = tid; i < D.k; i += G) {
      int n = 0;
      for (int e = 0; e < m; ++e) n += sA[e] == i;
      sBase[i] += n;
    }
    __syncthreads();
  }
}

// setNodeWeights: Ni[w] += 1 for every (set, word) pair met first, through one bitmap row per set of the chunk [set0, set0 + sets).
__global__ __launch_bounds__(kVtThreads) void k_vt_unique_words(const int* row_set, const int* row_word, int r0, int r1, int set0,
                                                                int words32, unsigned* bitmap, int* ni) {
  const int r = r0 + blockIdx.x * kVtThreads + (int)threadIdx.x;
  if (r >= r1) return;
  const int w = row_word[r];
  const unsigned bit = 1u << (w & 31);
  const unsigned old = atomicOr(&bitmap[(size_t)(row_set[r] - set0) * words32 + (w >> 5)], bit);
  if (!(old & bit)) atomicAdd(&ni[w], 1);
}

inline unsigned blocks(size_t n) { return (unsigned)((n + kVtThreads - 1) / kVtThreads); }

}  // namespace

size_t vt_means_lds_bytes(int k, int group) { return ((size_t)k * 257 + (size_t)group * 9) * 4; }

void launch_vt_begin(const VocTrainDev& D, hipStream_t st) {
  hipLaunchKernelGGL(k_vt_begin, dim3(blocks(D.num_seg)), dim3(kVtThreads), 0, st, D);
}

// `wide` tiles [0, wide) are worked by workgroups of kVtThreads, the `narrow` ones behind them by one wavefront each
void launch_vt_seed_round(const VocTrainDev& D, int wide, int narrow, int first_round, hipStream_t st) {
  if (wide) hipLaunchKernelGGL(k_vt_seed_dist, dim3(wide), dim3(kVtThreads), 0, st, D, 0, first_round);
  if (narrow) hipLaunchKernelGGL(k_vt_seed_dist, dim3(narrow), dim3(64), 0, st, D, wide, first_round);
  hipLaunchKernelGGL(k_vt_seed_cut, dim3(blocks(D.num_seg)), dim3(kVtThreads), 0, st, D);
  if (wide) hipLaunchKernelGGL(k_vt_seed_pick, dim3(wide), dim3(kVtThreads), 0, st, D, 0);
  if (narrow) hipLaunchKernelGGL(k_vt_seed_pick, dim3(narrow), dim3(64), 0, st, D, wide);
}

void launch_vt_means(const VocTrainDev& D, int wide, int narrow, hipStream_t st) {
  if (wide) hipLaunchKernelGGL(k_vt_means, dim3(wide), dim3(kVtThreads), vt_means_lds_bytes(D.k, kVtThreads), st, D, 0);
  if (narrow) hipLaunchKernelGGL(k_vt_means, dim3(narrow), dim3(64), vt_means_lds_bytes(D.k, 64), st, D, wide);
  if (D.num_slots) hipLaunchKernelGGL(k_vt_means_final, dim3(blocks((size_t)D.num_slots * D.k * 8)), dim3(kVtThreads), 0, st, D);
}

void launch_vt_assoc(const VocTrainDev& D, int wide, int narrow, int first, hipStream_t st) {
  if (wide) hipLaunchKernelGGL(k_vt_assoc, dim3(wide), dim3(kVtThreads), 0, st, D, 0, first);
  if (narrow) hipLaunchKernelGGL(k_vt_assoc, dim3(narrow), dim3(64), 0, st, D, wide, first);
  hipLaunchKernelGGL(k_vt_flags, dim3(blocks(D.num_seg)), dim3(kVtThreads), 0, st, D, first);
}

void launch_vt_partition(const VocTrainDev& D, int wide, int narrow, hipStream_t st) {
  if (wide) hipLaunchKernelGGL(k_vt_part_count, dim3(wide), dim3(kVtThreads), 0, st, D, 0);
  if (narrow) hipLaunchKernelGGL(k_vt_part_count, dim3(narrow), dim3(64), 0, st, D, wide);
  hipLaunchKernelGGL(k_vt_part_offsets, dim3(blocks(D.num_seg)), dim3(kVtThreads), 0, st, D);
  if (wide) hipLaunchKernelGGL(k_vt_part_scatter, dim3(wide), dim3(kVtThreads), 0, st, D, 0);
  if (narrow) hipLaunchKernelGGL(k_vt_part_scatter, dim3(narrow), dim3(64), 0, st, D, wide);
}

void launch_vt_unique_words(const int* row_set, const int* row_word, int r0, int r1, int set0, int words32, unsigned* bitmap, int* ni,
                            hipStream_t st) {
  if (r1 > r0) hipLaunchKernelGGL(k_vt_unique_words, dim3(blocks((size_t)(r1 - r0))), dim3(kVtThreads), 0, st, row_set, row_word, r0, r1,
                                  set0, words32, bitmap, ni);
}

}  // namespace covgpu
