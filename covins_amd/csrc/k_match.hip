// k_match.hip — batched brute-force Hamming matching of 32-byte ORB descriptors for the loop candidates:
// COVINS's LandmarkMatchingAlgorithm + estd2::DenseMatcher (placerec_be.cpp:84-90, mode DENSE) and COVINS-G's
// cv::BFMatcher(NORM_HAMMING).knnMatch(k = 2) + distance and ratio tests (placerec_gen_be.cpp:82-114, mode KNN2).
//
// Phase 1 (k_match_scan): one thread per query ("A") row, its descriptor in 8 VGPRs; a 256-thread workgroup covers 256 A rows of one
// job and streams the job's B rows through LDS in chunks of 256, every lane reading the same row (a broadcast). Each lane scans the B
// rows in ascending index order, as the reference's inner loop does: DENSE's 4-entry list depends on that order, so
// the B range is never split. KNN2's top-2 and tests finish in the same pass. Phase 2 (k_match_assign, DENSE only): one 64-thread
// workgroup per job stages the job's lists in LDS and its lane 0 replays DenseMatcher::assignbest in the single-thread order.
#include "common.hpp"

namespace covgpu {

namespace {

constexpr int kScanThreads = kMatchScanRows;   // A rows per workgroup = B rows staged per chunk
constexpr int kAssignThreads = 64;
constexpr int kBig = 1 << 20;          // above every distance: skipped and padding rows never enter a list

struct MatchArgs {
  const uint4* desc;                  // [rows][2] (32 B per row)
  const unsigned char* skip;          // [rows] or nullptr
  const int* row_ptr;
  const int* set_a;
  const int* set_b;
  const int* out_off;                 // [num_jobs] first output row of job j
  int* lists;                         // DENSE: [sum nA][4] entry (b << 16) | d, -1 = empty
  int* match;                         // [sum nA]
  int* dist;                          // [sum nA]
  int* nmatches;                      // [num_jobs], zeroed before the launch (KNN2 adds into it)
  int tiles;                          // A tiles per job
  int dcut;                           // DENSE: d is accepted iff d < dcut (<=> (float)d < dist_threshold)
  float thr, ratio;                   // KNN2
};

__device__ __forceinline__ int hamming(const uint4& a0, const uint4& a1, const uint4& b0, const uint4& b1) {
  int d = __builtin_popcount(a0.x ^ b0.x);
  d += __builtin_popcount(a0.y ^ b0.y);
  d += __builtin_popcount(a0.z ^ b0.z);
  d += __builtin_popcount(a0.w ^ b0.w);
  d += __builtin_popcount(a1.x ^ b1.x);
  d += __builtin_popcount(a1.y ^ b1.y);
  d += __builtin_popcount(a1.z ^ b1.z);
  d += __builtin_popcount(a1.w ^ b1.w);
  return d;
}

template <bool kDense>
__global__ __launch_bounds__(kScanThreads) void k_match_scan(MatchArgs M) {
  __shared__ uint4 sB[kScanThreads][2];
  __shared__ int sPen[kScanThreads];                     // 0, or kBig for a skipped row and for the padding past the chunk's end
  const int job = blockIdx.x / M.tiles, tile = blockIdx.x % M.tiles;
  const int a0 = M.row_ptr[M.set_a[job]], nA = M.row_ptr[M.set_a[job] + 1] - a0;
  const int b0 = M.row_ptr[M.set_b[job]], nB = M.row_ptr[M.set_b[job] + 1] - b0;
  if (tile * kScanThreads >= nA) return;                 // uniform over the workgroup
  const int ia = tile * kScanThreads + (int)threadIdx.x;
  const bool live = ia < nA;
  const bool active = live && !(kDense && M.skip && M.skip[a0 + ia]);
  uint4 q0 = make_uint4(0, 0, 0, 0), q1 = q0;
  if (live) { q0 = M.desc[2 * (size_t)(a0 + ia)]; q1 = M.desc[2 * (size_t)(a0 + ia) + 1]; }
  // DENSE list, sorted by distance (ties: later B row first); KNN2 top-2 by (d, index). A distance is at most 256 < kBig.
  int e0 = -1, e1 = -1, e2 = -1, e3 = -1;
  int d0 = kDense ? M.dcut : kBig, d1 = d0, d2 = d0, d3 = d0;
  for (int c = 0; c < nB; c += kScanThreads) {
    const int nc = min(kScanThreads, nB - c);
    __syncthreads();
    if ((int)threadIdx.x < nc) {
      const size_t r = (size_t)(b0 + c + (int)threadIdx.x);
      sB[threadIdx.x][0] = M.desc[2 * r]; sB[threadIdx.x][1] = M.desc[2 * r + 1];
      sPen[threadIdx.x] = (kDense && M.skip && M.skip[r]) ? kBig : 0;
    } else {
      sPen[threadIdx.x] = kBig;
    }
    __syncthreads();
    if (!active) continue;
    // four rows at a time: their distances without a branch (the LDS reads issue together), then the rare inserts in row order
    for (int j0 = 0; j0 < nc; j0 += 4) {
      int d[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) d[u] = hamming(q0, q1, sB[j0 + u][0], sB[j0 + u][1]) + sPen[j0 + u];
      if (min(min(d[0], d[1]), min(d[2], d[3])) >= (kDense ? d3 : d1)) continue;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int dd = d[u], j = c + j0 + u;
        if (kDense) {
          if (dd < d3) {                                 // listBIteration: tmpdist < aiBest[numBest-1].distance
            const int e = (j << 16) | dd;                // lower_bound: in front of the first entry with distance >= d
            if (dd <= d2) {
              e3 = e2; d3 = d2;
              if (dd <= d1) {
                e2 = e1; d2 = d1;
                if (dd <= d0) { e1 = e0; d1 = d0; e0 = e; d0 = dd; } else { e1 = e; d1 = dd; }
              } else { e2 = e; d2 = dd; }
            } else { e3 = e; d3 = dd; }
          }
        } else {
          if (dd < d1) {                                 // batchDistance K-best: after the entries with distance <= d
            if (dd < d0) { e1 = e0; d1 = d0; e0 = j; d0 = dd; } else { e1 = j; d1 = dd; }
          }
        }
      }
    }
  }
  if (!live) return;
  const size_t o = (size_t)M.out_off[job] + ia;
  if (kDense) {
    int4 l = make_int4(active ? e0 : -1, active ? e1 : -1, active ? e2 : -1, active ? e3 : -1);
    reinterpret_cast<int4*>(M.lists)[o] = l;
  } else {
    const bool ok = nB >= 2 && (float)d0 <= M.thr && (float)d0 < M.ratio * (float)d1;
    M.match[o] = ok ? e0 : -1;
    if (M.dist) M.dist[o] = ok ? d0 : -1;
    const unsigned long long bal = __ballot(ok);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(&M.nmatches[job], (int)__popcll(bal));
  }
}

// DenseMatcher::assignbest (DenseMatcher.cpp:62-104), iteratively, in the single-thread order. LDS: lists [nA][4], holder [nB]
// ((a << 16) | d, -1 = free, vpairs of matchBody), held [nA] (the B row A holds, -1 = none), cand [nA] (the A rows with a
// non-empty list, ascending: assignbest does nothing for the others).
__global__ __launch_bounds__(kAssignThreads) void k_match_assign(MatchArgs M, int maxA, int maxB) {
  extern __shared__ int smem[];
  const int job = blockIdx.x;
  const int a0 = M.row_ptr[M.set_a[job]], nA = M.row_ptr[M.set_a[job] + 1] - a0;
  const int nB = M.row_ptr[M.set_b[job] + 1] - M.row_ptr[M.set_b[job]];
  int* L = smem;                      // [maxA * 4]
  int* held = L + 4 * maxA;           // [maxA]
  int* vp = held + maxA;              // [nB]
  int* cand = vp + maxB;              // [nA]
  const size_t o = (size_t)M.out_off[job];
  for (int i = threadIdx.x; i < 4 * nA; i += kAssignThreads) L[i] = M.lists[4 * o + i];
  for (int i = threadIdx.x; i < nA; i += kAssignThreads) held[i] = -1;
  for (int i = threadIdx.x; i < nB; i += kAssignThreads) vp[i] = -1;
  __syncthreads();
  const int lane = (int)threadIdx.x;
  int ncand = 0;                                         // the same in every lane: built from ballots
  for (int base = 0; base < nA; base += kAssignThreads) {
    const bool has = base + lane < nA && L[4 * (base + lane)] >= 0;
    const unsigned long long bal = __ballot(has);
    if (has) cand[ncand + __popcll(bal & ((1ull << lane) - 1))] = base + lane;
    ncand += __popcll(bal);
  }
  __syncthreads();
  if (lane == 0) {
    int count = 0;
    for (int i = 0; i < ncand; ++i) {
      int cur = cand[i], idx = 0;
      while (idx < 4) {
        const int e = L[4 * cur + idx];
        if (e < 0) break;                                // aiBest[index].indexA == -1 ends the loop
        const int b = e >> 16, d = e & 0xffff;
        const int h = vp[b];
        if (h < 0) { vp[b] = (cur << 16) | d; held[cur] = b; ++count; break; }
        if (d < (h & 0xffff)) {                          // strictly better: steal, re-assign the loser from its entry 1
          const int old = h >> 16;
          vp[b] = (cur << 16) | d; held[cur] = b; held[old] = -1;
          cur = old; idx = 1;                            // terminates: every steal lowers vp[b]'s distance, an integer >= 0
          continue;
        }
        ++idx;
      }
    }
    M.nmatches[job] = count;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nA; i += kAssignThreads) {
    const int b = held[i];
    M.match[o + i] = b;
    if (M.dist) M.dist[o + i] = b < 0 ? -1 : (vp[b] & 0xffff);
  }
}

}  // namespace

size_t match_assign_lds_bytes(int maxA, int maxB) { return 4 * (6 * (size_t)maxA + (size_t)maxB); }

void launch_match(int mode, int num_jobs, int maxA, int maxB, const unsigned char* desc, const unsigned char* skip, const int* row_ptr,
                  const int* set_a, const int* set_b, const int* out_off, int* lists, int* match, int* dist, int* nmatches, int dcut,
                  float thr, float ratio, hipStream_t st) {
  if (num_jobs <= 0 || maxA <= 0) return;
  const int tiles = (maxA + kScanThreads - 1) / kScanThreads;
  MatchArgs M{reinterpret_cast<const uint4*>(desc), skip, row_ptr, set_a, set_b, out_off, lists, match, dist, nmatches, tiles, dcut, thr, ratio};
  const dim3 grid((unsigned)((int64_t)num_jobs * tiles));          // covgpu_match_batch keeps num_jobs * tiles <= 2^31 - 1
  if (mode == COVGPU_MATCH_DENSE) {
    hipLaunchKernelGGL(k_match_scan<true>, grid, dim3(kScanThreads), 0, st, M);
    const size_t lds = match_assign_lds_bytes(maxA, maxB);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_match_assign), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(k_match_assign, dim3(num_jobs), dim3(kAssignThreads), lds, st, M, maxA, maxB);
  } else {
    hipLaunchKernelGGL(k_match_scan<false>, grid, dim3(kScanThreads), 0, st, M);
  }
}

}  // namespace covgpu
