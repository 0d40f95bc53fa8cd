// k_lmrefresh.hip — Landmark::ComputeDescriptor (landmark_be.cpp:49-92) and Landmark::UpdateNormal (:185-220) for every landmark of a
// map in one pass. Per landmark: the candidates are its observations with a valid keyframe, in the order given; the
// representative descriptor is the candidate whose row of pairwise Hamming distances has the smallest median (rank (n-1)/2, the
// self-distance included), the lowest list position among equals; the normal is the mean of the unit vectors keyframe centre -> landmark,
// added in list order; the distances come from the reference observation's keyframe and octave. Integers for the descriptor, correctly
// rounded f64 operations without contraction for the rest, so the result does not depend on the form that computed it.
//
// Two forms, picked per landmark by the host from the length m of its observation list (which bounds the candidate count):
//   k_lmr_group<G>, G = 4 | 8 | 16 | 32 | 64 lanes per landmark, m <= G: lane i holds observation i — its descriptor in eight registers
//     and its unit vector. Descriptor j goes round the group by shuffles and lane i writes d(i, j) into its own 16-bit LDS row (a
//     distance can be 256); the median is found by nine bisection steps over the value, each counting the row's entries <= mid — no
//     sort, no array indexed at run time. The argmin is a shuffle minimum over (median << 16) | i. The unit vectors go round the group
//     the same way and every lane adds them in list order; lane 0 writes.
//   k_lmr_long, one 256-thread workgroup per landmark, m > 64: the first kLmrStage descriptors are staged in LDS, the rest is read from
//     global memory. One wavefront per row: its lanes stride over the row's entries into a 257-bin LDS histogram, a wave scan finds the
//     bin of rank (n-1)/2; the argmin is a minimum over (median << 32) | i, per wavefront and then over the four. The unit vectors are
//     computed 256 at a time into LDS and thread 0 adds each chunk in list order.
// No global atomics; every loop is bounded by a list length or a constant.
#include "common.hpp"

namespace covgpu {

namespace {

constexpr int kGroupThreads = 256;
constexpr int kHistBins = 320;                    // 257 values, five bins per lane
constexpr unsigned kNoKey = 0xffffffffu;
constexpr unsigned long long kNoKey64 = ~0ull;

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

__device__ __forceinline__ uint4 shfl4(const uint4& v, int src) {
  return make_uint4(__shfl(v.x, src), __shfl(v.y, src), __shfl(v.z, src), __shfl(v.w, src));
}

// Eigen's norm() of a 3-vector: sqrt((x x + y y) + z z), no fused multiply-add
__device__ __forceinline__ double norm3(double x, double y, double z) {
#pragma clang fp contract(off)
  return __dsqrt_rn((x * x + y * y) + z * z);
}

// (p - c) / |p - c|
__device__ __forceinline__ void unit_to(const double* p, const double* c, double& ux, double& uy, double& uz) {
#pragma clang fp contract(off)
  const double x = p[0] - c[0], y = p[1] - c[1], z = p[2] - c[2];
  const double n = norm3(x, y, z);
  ux = x / n; uy = y / n; uz = z / n;
}

__device__ __forceinline__ bool kf_valid(const LmRefreshDev& D, int o) { return !(D.kf_invalid && D.kf_invalid[D.obs_kf[o]]); }

// normal, distances and status of landmark l from the ordered sum (sx, sy, sz) of its n unit vectors; one thread
__device__ __forceinline__ void write_geometry(const LmRefreshDev& D, int l, int p0, int n, double sx, double sy, double sz) {
#pragma clang fp contract(off)
  int status = 0;
  double nx = 0.0, ny = 0.0, nz = 0.0, mind = 0.0, maxd = 0.0;
  if (n == 0) status |= 1;
  else { const double dn = (double)n; nx = sx / dn; ny = sy / dn; nz = sz / dn; }
  const int ref = D.ref_obs[l];
  if (ref < 0) status |= 2;
  else {
    const int o = p0 + ref;
    const double* c = D.center + 3 * (size_t)D.obs_kf[o];
    const double* p = D.pos + 3 * (size_t)l;
    const double dist = norm3(p[0] - c[0], p[1] - c[1], p[2] - c[2]);
    maxd = dist * D.scale[D.obs_octave[o]];
    mind = maxd / D.scale[D.num_octaves - 1];
  }
  D.normal[3 * (size_t)l] = nx; D.normal[3 * (size_t)l + 1] = ny; D.normal[3 * (size_t)l + 2] = nz;
  D.min_dist[l] = mind; D.max_dist[l] = maxd; D.status[l] = status;
}

// an invalid landmark: skipped, every output 0 / -1; one thread
__device__ __forceinline__ void write_skipped(const LmRefreshDev& D, int l) {
  if (D.obs_desc) { D.desc_obs[l] = -1; D.desc[2 * (size_t)l] = make_uint4(0, 0, 0, 0); D.desc[2 * (size_t)l + 1] = make_uint4(0, 0, 0, 0); }
  D.normal[3 * (size_t)l] = 0.0; D.normal[3 * (size_t)l + 1] = 0.0; D.normal[3 * (size_t)l + 2] = 0.0;
  D.min_dist[l] = 0.0; D.max_dist[l] = 0.0; D.status[l] = 4;
}

template <int G>
__global__ __launch_bounds__(kGroupThreads) void k_lmr_group(LmRefreshDev D, const int* __restrict__ list, int count) {
  static_assert(G >= 4 && G <= 64 && (G & (G - 1)) == 0, "lane groups are powers of two inside one wavefront");
  __shared__ unsigned short sRow[G * kGroupThreads];       // d(i, j) of the lane t that holds i: sRow[j * kGroupThreads + t]
  const int t = threadIdx.x;
  const int i = t % G;                                     // list position held by this lane
  const int base = (t & 63) - i;                           // first lane of the group inside the wavefront
  const int slot = blockIdx.x * (kGroupThreads / G) + t / G;
  const bool have = slot < count;
  const int l = have ? list[slot] : 0;
  const bool skip = have && D.lm_invalid && D.lm_invalid[l];
  const int p0 = have ? D.lm_ptr[l] : 0;
  const int m = have && !skip ? min(D.lm_ptr[l + 1] - p0, G) : 0;   // (<= G by the host's bucketing)
  bool valid = false;
  uint4 a = make_uint4(0, 0, 0, 0), b = a;
  double ux = 0.0, uy = 0.0, uz = 0.0;
  if (i < m && kf_valid(D, p0 + i)) {
    valid = true;
    if (D.obs_desc) { a = D.obs_desc[2 * (size_t)(p0 + i)]; b = D.obs_desc[2 * (size_t)(p0 + i) + 1]; }
    unit_to(D.pos + 3 * (size_t)l, D.center + 3 * (size_t)D.obs_kf[p0 + i], ux, uy, uz);
  }
  const unsigned long long gm = (__ballot(valid) >> base) & (G == 64 ? ~0ull : (1ull << (G & 63)) - 1ull);   // the group's candidates
  const int n = __popcll(gm);

  if (D.obs_desc) {   // (uniform)
    for (int j = 0; j < G; ++j) {
      const uint4 ja = shfl4(a, base + j), jb = shfl4(b, base + j);
      sRow[j * kGroupThreads + t] = (unsigned short)(((gm >> j) & 1ull) ? hamming(a, b, ja, jb) : 0xffff);
    }
    const int r = (n - 1) >> 1;
    int lo = 0, hi = 256;
    for (int s = 0; s < 9; ++s) {                          // 257 values: nine halvings
      const int mid = (lo + hi) >> 1;
      int c = 0;
      for (int j = 0; j < G; ++j) c += (int)sRow[j * kGroupThreads + t] <= mid;
      if (lo < hi) { if (c > r) hi = mid; else lo = mid + 1; }
    }
    unsigned key = valid ? ((unsigned)lo << 16) | (unsigned)i : kNoKey;
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) key = min(key, (unsigned)__shfl_xor((int)key, off));
    const int best = key == kNoKey ? -1 : (int)(key & 0xffffu);
    if (have && !skip) {
      if (i == 0) D.desc_obs[l] = best;
      if (i == best || (best < 0 && i == 0)) { D.desc[2 * (size_t)l] = a; D.desc[2 * (size_t)l + 1] = b; }   // (lane 0 without candidates holds zeros)
    }
  }

  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (int j = 0; j < G; ++j) {
    const double vx = __shfl(ux, base + j), vy = __shfl(uy, base + j), vz = __shfl(uz, base + j);
    if ((gm >> j) & 1ull) { sx = sx + vx; sy = sy + vy; sz = sz + vz; }
  }
  if (have && i == 0) {
    if (skip) write_skipped(D, l);
    else write_geometry(D, l, p0, n, sx, sy, sz);
  }
}

__global__ __launch_bounds__(kLmrLongThreads) void k_lmr_long(LmRefreshDev D, const int* __restrict__ list) {
  __shared__ uint4 sDesc[2 * kLmrStage];
  __shared__ unsigned char sValid[kLmrStage];
  __shared__ int sHist[kLmrLongThreads / 64][kHistBins];
  __shared__ unsigned long long sKey[kLmrLongThreads / 64];
  __shared__ int sCount[kLmrLongThreads / 64];
  __shared__ double sU[kLmrLongThreads][3];
  __shared__ unsigned char sUV[kLmrLongThreads];
  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  const int l = list[blockIdx.x];
  if (D.lm_invalid && D.lm_invalid[l]) {   // (the whole workgroup)
    if (t == 0) write_skipped(D, l);
    return;
  }
  const int p0 = D.lm_ptr[l], m = D.lm_ptr[l + 1] - p0;

  int cnt = 0;
  for (int j = t; j < m; j += kLmrLongThreads) {
    const bool v = kf_valid(D, p0 + j);
    cnt += v;
    if (j < kLmrStage) {
      sValid[j] = v;
      if (D.obs_desc) { sDesc[2 * j] = D.obs_desc[2 * (size_t)(p0 + j)]; sDesc[2 * j + 1] = D.obs_desc[2 * (size_t)(p0 + j) + 1]; }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
  if (lane == 0) sCount[w] = cnt;
  __syncthreads();
  int n = 0;
  for (int k = 0; k < kLmrLongThreads / 64; ++k) n += sCount[k];

  auto is_valid = [&](int j) -> bool { return j < kLmrStage ? sValid[j] != 0 : kf_valid(D, p0 + j); };

  if (D.obs_desc) {   // (uniform)
    const int r = (n - 1) >> 1;
    unsigned long long best = kNoKey64;                    // of this wavefront's rows; the same in all its lanes
    for (int i0 = 0; i0 < m; i0 += kLmrLongThreads / 64) { // the same trip count in every wavefront: the barriers are uniform
      const int i = i0 + w;
      const bool act = i < m && is_valid(i);
      for (int q = lane; q < kHistBins; q += 64) sHist[w][q] = 0;
      __syncthreads();
      if (act) {
        const uint4 ia = i < kLmrStage ? sDesc[2 * i] : D.obs_desc[2 * (size_t)(p0 + i)];
        const uint4 ib = i < kLmrStage ? sDesc[2 * i + 1] : D.obs_desc[2 * (size_t)(p0 + i) + 1];
        for (int j = lane; j < m; j += 64) {               // every entry of the row, strided: any length
          if (!is_valid(j)) continue;
          const uint4 ja = j < kLmrStage ? sDesc[2 * j] : D.obs_desc[2 * (size_t)(p0 + j)];
          const uint4 jb = j < kLmrStage ? sDesc[2 * j + 1] : D.obs_desc[2 * (size_t)(p0 + j) + 1];
          atomicAdd(&sHist[w][hamming(ia, ib, ja, jb)], 1);
        }
      }
      __syncthreads();
      if (act) {
        const int* h = &sHist[w][5 * lane];
        const int h0 = h[0], h1 = h[1], h2 = h[2], h3 = h[3], h4 = h[4];
        const int own = h0 + h1 + h2 + h3 + h4;
        int incl = own;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) { const int up = __shfl_up(incl, off); if (lane >= off) incl += up; }
        const int excl = incl - own;
        int med = -1;                                      // the bin of rank r lies in exactly one lane's five
        if (excl <= r && r < incl) {
          int c = excl + h0;
          if (c > r) med = 5 * lane;
          else if ((c += h1) > r) med = 5 * lane + 1;
          else if ((c += h2) > r) med = 5 * lane + 2;
          else if ((c += h3) > r) med = 5 * lane + 3;
          else med = 5 * lane + 4;
        }
        const unsigned long long who = __ballot(med >= 0);
        med = __shfl(med, who ? __ffsll((long long)who) - 1 : 0);
        const unsigned long long key = ((unsigned long long)(unsigned)med << 32) | (unsigned)i;
        best = key < best ? key : best;
      }
      __syncthreads();
    }
    if (lane == 0) sKey[w] = best;
    __syncthreads();
    unsigned long long key = sKey[0];
    for (int k = 1; k < kLmrLongThreads / 64; ++k) key = sKey[k] < key ? sKey[k] : key;
    const int pick = key == kNoKey64 ? -1 : (int)(unsigned)(key & 0xffffffffull);
    if (t == 0) D.desc_obs[l] = pick;
    if (t < 2) D.desc[2 * (size_t)l + t] = pick < 0 ? make_uint4(0, 0, 0, 0) : D.obs_desc[2 * (size_t)(p0 + pick) + t];
  }

  double sx = 0.0, sy = 0.0, sz = 0.0;                     // thread 0's
  for (int c0 = 0; c0 < m; c0 += kLmrLongThreads) {
    const int j = c0 + t;
    const bool v = j < m && is_valid(j);
    sUV[t] = v;
    if (v) unit_to(D.pos + 3 * (size_t)l, D.center + 3 * (size_t)D.obs_kf[p0 + j], sU[t][0], sU[t][1], sU[t][2]);
    __syncthreads();
    if (t == 0) {
      const int nc = min(kLmrLongThreads, m - c0);
      for (int q = 0; q < nc; ++q) if (sUV[q]) { sx = sx + sU[q][0]; sy = sy + sU[q][1]; sz = sz + sU[q][2]; }
    }
    __syncthreads();
  }
  if (t == 0) write_geometry(D, l, p0, n, sx, sy, sz);
}

}  // namespace

void launch_lm_refresh(const LmRefreshDev& D, int lanes, const int* list, int count, hipStream_t st) {
  if (count <= 0) return;
  auto blocks = [count](int g) { const int per = kGroupThreads / g; return (count + per - 1) / per; };
  switch (lanes) {
    case 4: k_lmr_group<4><<<blocks(4), kGroupThreads, 0, st>>>(D, list, count); break;
    case 8: k_lmr_group<8><<<blocks(8), kGroupThreads, 0, st>>>(D, list, count); break;
    case 16: k_lmr_group<16><<<blocks(16), kGroupThreads, 0, st>>>(D, list, count); break;
    case 32: k_lmr_group<32><<<blocks(32), kGroupThreads, 0, st>>>(D, list, count); break;
    case 64: k_lmr_group<64><<<blocks(64), kGroupThreads, 0, st>>>(D, list, count); break;
    default: k_lmr_long<<<count, kLmrLongThreads, 0, st>>>(D, list); break;
  }
}

}  // namespace covgpu
