// k_guided.hip — batched guided matching for the loop candidates: COVINS's FeatureMatcher::SearchBySE3
// (feature_matcher_be.cpp:293-498) and FeatureMatcher::SearchByProjection (:168-291). Both project landmarks into a keyframe, collect the
// keypoints inside a radius (KeyframeBase::GetFeaturesInArea, keyframe_base.cpp:262-318), keep the levels [predicted - 1, predicted]
// (LandmarkBase::PredictScale, landmark_base.cpp:120-133) and take the smallest Hamming distance with `<` (the first visited wins).
//
// Scan (k_guided_se3_scan, k_guided_proj_scan): one thread per point, its target pixel, radius, level and 32-byte descriptor in
// registers; a 256-thread workgroup covers one tile of up to 256 points of one job (and direction) and streams the keyframe's keypoints
// through LDS in chunks of 256 as {x, y, level, visiting rank}, every lane reading the same entry (a broadcast). The float radius test and
// the level window run per entry; only a keypoint that passes both has its descriptor fetched from global memory. A candidate is the key
// (distance << 24) | (visiting rank << 12) | row, so `min` over the keys is "smallest distance, first visited".
// SE3: the scan runs both directions in one launch; k_guided_agree applies the agreement test and counts. PROJECTION: the scan keeps the
// kGuidedListCap smallest keys with distance <= th_low per point plus their true number, and k_guided_proj_replay (one wavefront per job)
// replays the points in order against a claim bitmap in LDS; a point whose list was cut short and whose stored entries are all claimed
// is rescanned by the whole wavefront.
#include "common.hpp"
#include "dev_math.hpp"

namespace covgpu {

namespace {

using namespace covdev;

constexpr int kT = kGuidedScanPoints;
constexpr int kCap = kGuidedListCap;
constexpr int kReplayThreads = 64;
constexpr unsigned kNone = 0xffffffffu;          // above every key: a distance in a key is at most 255
constexpr int kStage = kCap + 3;                 // replay LDS row: keys, count, existing_idx, distance to the existing keypoint

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

// GetFeaturesInArea's test (keyframe_base.cpp:277-278, 308-309): float differences, float32 norm without a fused multiply-add, compared
// as a double with the radius
__device__ __forceinline__ bool in_area(float kx, float ky, float tx, float ty, double radius) {
#pragma clang fp contract(off)
  const float dx = kx - tx, dy = ky - ty;
  const float d = sqrtf(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)));
  return (double)d <= radius;
}

// KeyframeBase::IsInImage (keyframe_base.cpp:414-416); false for a NaN
__device__ __forceinline__ bool in_image(double u, double v, const double* b) { return u >= b[0] && u < b[1] && v >= b[2] && v < b[3]; }

// LandmarkBase::PredictScale (landmark_base.cpp:120-133): the distance arrives through a const float&
__device__ __forceinline__ int predict_scale(double dist, double max_distance, const GuidedOptsDev& O) {
  if (O.num_octaves == 1) return 0;              // both clamps end at 0
  const double ratio = max_distance / (double)(float)dist;
  const double n = ceil(log(ratio) / O.log_sf);
  return n < 0.0 ? 0 : (n >= (double)O.num_octaves ? O.num_octaves - 1 : (int)n);
}

// The keypoints [k0, k0 + nK) against this thread's point: keys[] = the kN smallest keys with distance <= dmax, ascending; cnt = how
// many there are. Every thread of the workgroup calls it (it synchronises); inactive threads only help staging.
template <int kN>
__device__ __forceinline__ void scan_set(const GuidedSets& S, int k0, int nK, bool active, float tx, float ty, double radius, int lvl,
                                         const uint4& q0, const uint4& q1, int dmax, unsigned (&keys)[kN], int& cnt, int4* sK) {
  for (int c = 0; c < nK; c += kT) {
    const int nc = min(kT, nK - c);
    __syncthreads();
    if ((int)threadIdx.x < nc) sK[threadIdx.x] = S.kpr[(size_t)k0 + c + threadIdx.x];
    __syncthreads();
    if (!active) continue;
    for (int j = 0; j < nc; ++j) {
      const int4 e = sK[j];
      if (e.z < lvl - 1 || e.z > lvl) continue;  // a taken keypoint has level INT_MIN
      if (!in_area(__int_as_float(e.x), __int_as_float(e.y), tx, ty, radius)) continue;
      const size_t r = (size_t)k0 + c + j;
      const int d = hamming(q0, q1, S.kdesc[2 * r], S.kdesc[2 * r + 1]);
      if (d > dmax) continue;
      ++cnt;
      const unsigned key = ((unsigned)d << 24) | ((unsigned)e.w << 12) | (unsigned)(c + j);
      if (key < keys[kN - 1]) {
        keys[kN - 1] = key;
#pragma unroll
        for (int u = kN - 1; u > 0; --u)
          if (keys[u] < keys[u - 1]) { const unsigned t = keys[u]; keys[u] = keys[u - 1]; keys[u - 1] = t; }
      }
    }
  }
}

__global__ __launch_bounds__(kT) void k_guided_se3_scan(GuidedSe3Args A, GuidedOptsDev O, const int4* tiles) {
  __shared__ int4 sK[kT];
  const int4 t = tiles[blockIdx.x];              // {job, direction, first row, rows}
  const int job = t.x, dir = t.y;
  const int s1 = A.set_1[job], s2 = A.set_2[job];
  const int src = dir ? s2 : s1, dst = dir ? s1 : s2;
  const int r0 = A.S.row_ptr[src], k0 = A.S.row_ptr[dst], nK = A.S.row_ptr[dst + 1] - k0;
  const int i = t.z + (int)threadIdx.x;
  const bool live = (int)threadIdx.x < t.w;
  bool active = live && A.lm_free[r0 + i] != 0;
  float tx = 0.f, ty = 0.f;
  double radius = 1.0;
  int lvl = 0;
  uint4 q0 = make_uint4(0, 0, 0, 0), q1 = q0;
  if (active) {
    const V3 p = ld3(A.lm_pos + 3 * (size_t)(r0 + i));
    const double* T = A.T12 + 7 * (size_t)job;
    const M3 R = qrot(ldq(T));
    const V3 t12 = ld3(T + 4);
    const V3 pc = dir ? mul(R, p) + t12 : mulT(R, p - t12);     // :423 / :344 (T21 = T12^-1)
    const double* K = A.K + 4 * (size_t)dst;
    const double u = (K[0] * pc.x + K[2] * pc.z) / pc.z, v = (K[1] * pc.y + K[3] * pc.z) / pc.z;   // K p / z, :351-352, :431-432
    // z < 0 skips (:347, :426); z == 0 gives inf or NaN and fails or passes IsInImage as IEEE has it. The bounds are keyframe 2's in
    // both directions (:355, :433).
    if (pc.z < 0.0 || !in_image(u, v, A.S.bounds + 4 * (size_t)s2)) {
      active = false;
    } else {
      lvl = predict_scale(sqrt(dot(pc, pc)), A.lm_maxd[r0 + i], O);
      radius = ldexp(O.radius, lvl);             // th * 2.0^level, :366, :443
      tx = (float)u; ty = (float)v;
      q0 = A.lm_desc[2 * (size_t)(r0 + i)]; q1 = A.lm_desc[2 * (size_t)(r0 + i) + 1];
    }
  }
  unsigned keys[1] = {kNone};
  int cnt = 0;
  scan_set<1>(A.S, k0, nK, active, tx, ty, radius, lvl, q0, q1, dir ? O.th_low - 1 : O.th_low, keys, cnt, sK);   // <= :403, < :479
  if (!live) return;
  (dir ? A.m2 + A.off2[job] : A.m1 + A.off1[job])[i] = keys[0] == kNone ? -1 : (int)(keys[0] & 4095u);
}

// :485-495. One workgroup per job; nfound is zeroed before the launch.
__global__ __launch_bounds__(kT) void k_guided_agree(GuidedSe3Args A, int agreement) {
  const int job = blockIdx.x;
  const int s1 = A.set_1[job], s2 = A.set_2[job];
  const int n1 = A.S.row_ptr[s1 + 1] - A.S.row_ptr[s1], n2 = A.S.row_ptr[s2 + 1] - A.S.row_ptr[s2];
  const int* m1 = A.m1 + A.off1[job];
  const int* m2 = A.m2 + A.off2[job];
  int* out = A.match + A.off1[job];
  for (int base = 0; base < n1; base += kT) {
    const int i = base + (int)threadIdx.x;
    bool ok = false;
    if (i < n1) {
      const int idx2 = m1[i];                    // a row of set 2: idx2 < n2
      if (idx2 >= 0) ok = agreement ? m2[idx2] == i : (i < n2 && m2[i] == i);
      out[i] = ok ? idx2 : -1;
    }
    const unsigned long long bal = __ballot(ok);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(&A.nfound[job], (int)__popcll(bal));
  }
}

__global__ __launch_bounds__(kT) void k_guided_proj_scan(GuidedProjArgs A, GuidedOptsDev O, const int4* tiles) {
  __shared__ int4 sK[kT];
  const int4 t = tiles[blockIdx.x];              // {job, 0, first point, points}
  const int job = t.x, set = A.set[job];
  const int k0 = A.S.row_ptr[set], nK = A.S.row_ptr[set + 1] - k0;
  const size_t p = (size_t)A.point_ptr[job] + t.z + threadIdx.x;
  const bool live = (int)threadIdx.x < t.w;
  bool active = live && !(A.skip && A.skip[p]);
  float tx = 0.f, ty = 0.f;
  double radius = 1.0;
  int lvl = 0, dold = -1;
  uint4 q0 = make_uint4(0, 0, 0, 0), q1 = q0;
  if (active) {
    const double* T = A.T_cw + 7 * (size_t)job;
    const M3 R = qrot(ldq(T));
    const V3 tcw = ld3(T + 4), pw = ld3(A.p_w + 3 * p);
    const V3 pc = mul(R, pw) + tcw;                              // :192
    double u = 0.0, v = 0.0;
    const double* cam = A.cam + 8 * (size_t)set;
    active = !(pc.z < 0.0) &&                                    // :195
             project_camera(pc, A.cam_model ? A.cam_model[set] : COVGPU_CAM_PINHOLE, A.cam_model ? A.xi[set] : 0.0, cam, cam + 4,
                            A.dist_type[set], u, v, nullptr) &&
             in_image(u, v, A.S.bounds + 4 * (size_t)set);       // :204
    if (active) {
      const V3 PO = pw + mulT(R, tcw);                           // p_w - O_w, O_w = -R^T t (:172, :210)
      const double dist = sqrt(dot(PO, PO));
      const double mind = 0.8 * A.min_d[p], maxd = 1.2 * A.max_d[p];   // landmark_base.cpp:68-76
      if (dist < mind || dist > maxd || dot(PO, ld3(A.normal + 3 * p)) < 0.5 * dist) {   // :213, :220
        active = false;
      } else {
        lvl = predict_scale(dist, A.max_d[p], O);
        radius = O.radius * pow(O.scale_factor, (double)lvl);    // :227
        tx = (float)u; ty = (float)v;
        q0 = A.p_desc[2 * p]; q1 = A.p_desc[2 * p + 1];
        const int ex = A.existing ? A.existing[p] : -1;
        if (ex >= 0) dold = hamming(q0, q1, A.S.kdesc[2 * (size_t)(k0 + ex)], A.S.kdesc[2 * (size_t)(k0 + ex) + 1]);   // :264-265
      }
    }
  }
  unsigned keys[kCap];
#pragma unroll
  for (int u = 0; u < kCap; ++u) keys[u] = kNone;
  int cnt = 0;
  scan_set<kCap>(A.S, k0, nK, active, tx, ty, radius, lvl, q0, q1, O.th_low, keys, cnt, sK);
  if (!live) return;
  static_assert(kCap == 8, "the list is stored as two int4");
  reinterpret_cast<int4*>(A.lists)[2 * p] = make_int4((int)keys[0], (int)keys[1], (int)keys[2], (int)keys[3]);
  reinterpret_cast<int4*>(A.lists)[2 * p + 1] = make_int4((int)keys[4], (int)keys[5], (int)keys[6], (int)keys[7]);
  A.cnt[p] = cnt;
  A.target[2 * p] = tx; A.target[2 * p + 1] = ty;
  A.rad[p] = radius;
  A.lvl[p] = lvl;
  A.dold[p] = dold;
}

// What :258-287 does with a point's best unclaimed key (kNone: nothing within th_low). Returns 1 for a claim.
__device__ __forceinline__ int replay_finish(const GuidedProjArgs& A, size_t p, unsigned best, int existing, int dold, unsigned* sClaim) {
  int claimed = -1, remap = -1, bd = -1, got = 0;
  if (best != kNone) {
    const int row = (int)(best & 4095u);
    bd = (int)(best >> 24);
    if (existing != -1) {
      if (!(dold < bd)) remap = row;             // :267-281; the dist_newplace test compares bestDist with itself
    } else {
      sClaim[row >> 5] |= 1u << (row & 31);      // :284
      claimed = row; got = 1;
    }
  }
  A.claimed[p] = claimed;
  A.remap_to[p] = remap;
  if (A.best_dist) A.best_dist[p] = bd;
  return got;
}

// One wavefront per job: lane 0 replays the points in order from their lists (staged 64 points at a time); the wavefront rescans a
// point whose list was cut short and is used up.
__global__ __launch_bounds__(kReplayThreads) void k_guided_proj_replay(GuidedProjArgs A, GuidedOptsDev O) {
  __shared__ unsigned sClaim[COVGPU_MATCH_MAX_ROWS / 32];
  __shared__ int sL[kReplayThreads][kStage];
  __shared__ int sNext;
  const int job = blockIdx.x, set = A.set[job], lane = (int)threadIdx.x;
  const int k0 = A.S.row_ptr[set], nK = A.S.row_ptr[set + 1] - k0;
  const size_t P0 = (size_t)A.point_ptr[job];
  const int nP = A.point_ptr[job + 1] - A.point_ptr[job];
  for (int w = lane; w < COVGPU_MATCH_MAX_ROWS / 32; w += kReplayThreads) sClaim[w] = 0u;
  int count = 0;                                 // lane 0's
  for (int base = 0; base < nP; base += kReplayThreads) {
    const int n = min(kReplayThreads, nP - base);
    __syncthreads();
    if (lane < n) {
      const size_t p = P0 + base + lane;
#pragma unroll
      for (int u = 0; u < kCap; ++u) sL[lane][u] = A.lists[kCap * p + u];
      sL[lane][kCap] = A.cnt[p];
      sL[lane][kCap + 1] = A.existing ? A.existing[p] : -1;
      sL[lane][kCap + 2] = A.dold[p];
    }
    __syncthreads();
    int i = 0;                                   // the same in every lane at each synchronisation
    while (true) {
      if (lane == 0) {
        for (; i < n; ++i) {
          const int c = sL[i][kCap];
          unsigned best = kNone;
          for (int u = 0; u < min(c, kCap); ++u) {
            const unsigned key = (unsigned)sL[i][u];
            const int row = (int)(key & 4095u);
            if (!((sClaim[row >> 5] >> (row & 31)) & 1u)) { best = key; break; }
          }
          if (best == kNone && c > kCap) break;  // entries beyond the stored ones exist: rescan
          count += replay_finish(A, P0 + base + i, best, sL[i][kCap + 1], sL[i][kCap + 2], sClaim);
        }
        sNext = i;
      }
      __syncthreads();
      i = sNext;
      if (i >= n) break;
      const size_t p = P0 + base + i;
      const float tx = A.target[2 * p], ty = A.target[2 * p + 1];
      const double radius = A.rad[p];
      const int lvl = A.lvl[p];
      const uint4 q0 = A.p_desc[2 * p], q1 = A.p_desc[2 * p + 1];
      unsigned best = kNone;
      for (int k = lane; k < nK; k += kReplayThreads) {
        const int4 e = A.S.kpr[(size_t)k0 + k];
        if (e.z < lvl - 1 || e.z > lvl) continue;
        if ((sClaim[k >> 5] >> (k & 31)) & 1u) continue;
        if (!in_area(__int_as_float(e.x), __int_as_float(e.y), tx, ty, radius)) continue;
        const int d = hamming(q0, q1, A.S.kdesc[2 * ((size_t)k0 + k)], A.S.kdesc[2 * ((size_t)k0 + k) + 1]);
        if (d <= O.th_low) best = min(best, ((unsigned)d << 24) | ((unsigned)e.w << 12) | (unsigned)k);
      }
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) best = min(best, (unsigned)__shfl_xor((int)best, off, 64));
      __syncthreads();                           // every lane has read sNext and the claims
      if (lane == 0) count += replay_finish(A, p, best, sL[i][kCap + 1], sL[i][kCap + 2], sClaim);
      ++i;
    }
  }
  if (lane == 0) A.nmatches[job] = count;
}

}  // namespace

void launch_guided_se3(const GuidedSe3Args& A, const GuidedOptsDev& O, int num_jobs, const int4* tiles, int num_tiles, hipStream_t st) {
  if (num_jobs <= 0) return;
  if (num_tiles > 0) hipLaunchKernelGGL(k_guided_se3_scan, dim3((unsigned)num_tiles), dim3(kT), 0, st, A, O, tiles);
  hipLaunchKernelGGL(k_guided_agree, dim3((unsigned)num_jobs), dim3(kT), 0, st, A, O.agreement);
}

void launch_guided_projection(const GuidedProjArgs& A, const GuidedOptsDev& O, int num_jobs, const int4* tiles, int num_tiles,
                              hipStream_t st) {
  if (num_jobs <= 0) return;
  if (num_tiles > 0) hipLaunchKernelGGL(k_guided_proj_scan, dim3((unsigned)num_tiles), dim3(kT), 0, st, A, O, tiles);
  hipLaunchKernelGGL(k_guided_proj_replay, dim3((unsigned)num_jobs), dim3(kReplayThreads), 0, st, A, O);
}

}  // namespace covgpu
