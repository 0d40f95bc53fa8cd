// k_visual.hip — reprojection residual blocks on gfx950: linearisation fused with landmark elimination.
//
// Replaces, for the problems assembled at covins_backend/src/covins_backend/optimization_be.cpp:432-530,
//   R4 robopt::reprojection::GlobalEuclideanReprError<PinholeCamera, RadTan|Equidistant>  (opt_be.cpp:487-525)
//   R5 aslam::PinholeCamera::project3 + distortion Jacobian
//   R6 ceres::CauchyLoss(1.0) corrector                                                   (opt_be.cpp:302,523)
// and the landmark half of Ceres' SPARSE_SCHUR (opt_be.cpp:561): H_ll, g_l, S -= W H_ll^-1 W^T, b += W H_ll^-1 g_l
// (SURVEY.md A.2, A.5, A.6). None of these have a reference source in-tree; the contract is SURVEY.md Appendix A.
//
// Kernel shapes — three deterministic, atomic-free passes:
//   k_lm_lin       one G-lane sub-wave group per landmark (G = 16: tracks average ~10 observations), lane = observation.
//                  Jacobians live in VGPRs only; H_ll / g_l are reduced with shuffle butterflies inside the group. With the
//                  Cholesky factor of the damped inverse, H_ll^-1 = R R^T, ONE 6x3 record per observation goes to HBM:
//                  Z = (Jp^T Jl) R — then W H_ll^-1 W'^T = Z Z'^T for any two observations of the landmark. (Rounds 1-2 wrote
//                  W, Y = W H_ll^-1 and a 39-double pose-side record: 600 B per observation instead of 144.)
//   k_kf_reduce    one wave per keyframe, lanes over its observations: every observation is RE-LINEARISED (pose and landmark
//                  rows are cache resident, the flops are free next to the 312-B record this replaces), D = Jp^T Jp - Z Z^T,
//                  gradient and right-hand side terms summed in a fixed order -> diagonal 6x6 block, gradient, reduced
//                  right-hand side, diag(J^T J).
//   k_pair_blocks  sixteen lanes per covisible keyframe pair (host-built lists, static per problem), lanes over the common
//                  landmarks: C[i,j] = -sum Z_i Z_j^T with plain stores. Every entry has exactly one writer and a fixed
//                  summation order: two solves of the same problem are bit-identical. The sixteen lanes load a trip's records together,
//                  consecutive lanes consecutive 16 bytes, through LDS; the pairs of an XCD chunk are dealt to its slots by falling
//                  length (DevProblem::pair_order). k_lm_lin writes the records the same way, through a per-wave LDS tile.
//                  (The first version accumulated the
//                  6x6 blocks with FP64 atomics: 11.1 ms and run-to-run rounding differences; these three passes take
//                  0.66 ms on the 5-agent map.)
//   obs_*          one thread per observation over the SoA stream (cost, J*v products, test dumps).
// All writes to the pose system go through c_entry (common.hpp): the fronts of the multifrontal solve (nd_entry), or the dense
// matrix of the per-kernel test entry points.
#include <type_traits>

#include "common.hpp"
#include "dev_math.hpp"
#include "reduce.hpp"
#include "visual_dev.hpp"

namespace covgpu {
using namespace covdev;

COV_DEV void group_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

// symmetric 3x3 inverse; h = xx xy xz yy yz zz
COV_DEV void inv3sym(const double* h, double* o) {
  const double c00 = h[3] * h[5] - h[4] * h[4], c01 = h[2] * h[4] - h[1] * h[5], c02 = h[1] * h[4] - h[2] * h[3];
  const double det = h[0] * c00 + h[1] * c01 + h[2] * c02;
  const double id = (fabs(det) > 0.0) ? 1.0 / det : 0.0;
  o[0] = c00 * id; o[1] = c01 * id; o[2] = c02 * id;
  o[3] = (h[0] * h[5] - h[2] * h[2]) * id; o[4] = (h[1] * h[2] - h[0] * h[4]) * id; o[5] = (h[0] * h[3] - h[1] * h[1]) * id;
}

constexpr int kBuildThreads = 256;

// ------------------------------------------------------------------------------------------------------------
// Landmark elimination in three deterministic, atomic-free passes:
//   k_lm_lin      (landmark-major) per landmark H_ll, g_l reduced in-group, damped inverse; per observation a
//                 record {W_a = Jp^T Jl, Y_a = W_a Hinv, D_a = Jp^T Jp - Y_a W_a^T, diag(Jp^T Jp), Jp^T r, Y_a g_l}
//   k_kf_reduce   (keyframe-major) one wave per keyframe sums its observations' records in a fixed order (lane = observation,
//                 partial sums through LDS) -> diagonal block of C, gradient, reduced right-hand side, diag(J^T J)
//   k_pair_blocks (covisible keyframe pair-major) sixteen lanes per pair (i > j in chain-major order), lane = common landmark:
//                 C[i,j] = -sum over common landmarks of Y_i W_j^T, written with plain stores
// Every entry of C is produced by exactly one wave in a fixed summation order: run-to-run bit-identical
// (SURVEY.md §7 "irregular graph": determinism needed for parity tests) and no FP64 atomic contention.
// ------------------------------------------------------------------------------------------------------------
constexpr int kRec = 39;  // per-keyframe sums of k_kf_reduce: D(21, lower row-major) hd(6) gp(6) yg(6)

// lower Cholesky factor of the symmetric positive definite 3x3 h = (xx xy xz yy yz zz): r = (r00 r10 r11 r20 r21 r22); a
// non-positive pivot (never for a damped inverse) gives zeros
COV_DEV void chol3(const double* h, double* r) {
  const double r00 = h[0] > 0.0 ? sqrt(h[0]) : 0.0, i00 = r00 > 0.0 ? 1.0 / r00 : 0.0;
  const double r10 = h[1] * i00, r20 = h[2] * i00;
  const double d1 = h[3] - r10 * r10, r11 = d1 > 0.0 ? sqrt(d1) : 0.0, i11 = r11 > 0.0 ? 1.0 / r11 : 0.0;
  const double r21 = (h[4] - r20 * r10) * i11;
  const double d2 = h[5] - r20 * r20 - r21 * r21, r22 = d2 > 0.0 ? sqrt(d2) : 0.0;
  r[0] = r00; r[1] = r10; r[2] = r11; r[3] = r20; r[4] = r21; r[5] = r22;
}
// Z = W R for W = Jp^T Jl (6x3) and the lower factor R
COV_DEV void z_of(const ObsLin& e, const double* R, double* Z) {
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    const double w0 = e.jp[r] * e.jl[0] + e.jp[6 + r] * e.jl[3], w1 = e.jp[r] * e.jl[1] + e.jp[6 + r] * e.jl[4], w2 = e.jp[r] * e.jl[2] + e.jp[6 + r] * e.jl[5];
    Z[3 * r] = w0 * R[0] + w1 * R[1] + w2 * R[3];
    Z[3 * r + 1] = w1 * R[2] + w2 * R[4];
    Z[3 * r + 2] = w2 * R[5];
  }
}

template <int G, bool UNI>
__global__ __launch_bounds__(kBuildThreads) void k_lm_lin(DevProblem P, double mu, DevSignal sig) {
  constexpr int GROUPS = kBuildThreads / G;
  // "everything before this kernel on its stream is complete" (the previous iteration's state update, the preintegration): the side stream's
  // kernels of this pass start from it — published here instead of by a launch in front of the pass's critical path
  if (sig.flag != nullptr && blockIdx.x == 0 && threadIdx.x == 0) __hip_atomic_store(sig.flag, sig.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const int lane = threadIdx.x % G, grp = threadIdx.x / G;
  const int l = blockIdx.x * GROUPS + grp;
  const bool lm_ok = l < P.L;
  const int o0 = lm_ok ? P.lm_obs_ptr[l] : 0;
  const int nobs = lm_ok ? P.lm_obs_ptr[l + 1] - o0 : 0;
  const int nchunk = (nobs + G - 1) / G;

  double h[6] = {0, 0, 0, 0, 0, 0}, gl[3] = {0, 0, 0}, cost = 0.0;
  ObsLin e;
  int kf = 0;
  for (int c = 0; c < nchunk; ++c) {
    const int a = c * G + lane;
    if (a < nobs) {
      kf = P.obs_kf[o0 + a];
      eval_obs<true, UNI>(P, P.pose, P.lm, o0 + a, kf, l, e);
      h[0] += e.jl[0] * e.jl[0] + e.jl[3] * e.jl[3];
      h[1] += e.jl[0] * e.jl[1] + e.jl[3] * e.jl[4];
      h[2] += e.jl[0] * e.jl[2] + e.jl[3] * e.jl[5];
      h[3] += e.jl[1] * e.jl[1] + e.jl[4] * e.jl[4];
      h[4] += e.jl[1] * e.jl[2] + e.jl[4] * e.jl[5];
      h[5] += e.jl[2] * e.jl[2] + e.jl[5] * e.jl[5];
      gl[0] += e.jl[0] * e.r0 + e.jl[3] * e.r1;
      gl[1] += e.jl[1] * e.r0 + e.jl[4] * e.r1;
      gl[2] += e.jl[2] * e.r0 + e.jl[5] * e.r1;
      cost += e.cost;
    }
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) h[k] = group_sum<G>(h[k]);
#pragma unroll
  for (int k = 0; k < 3; ++k) gl[k] = group_sum<G>(gl[k]);
  double hi[6];
  {
    double hd[6] = {h[0], h[1], h[2], h[3], h[4], h[5]};
    const double d0 = clamp_diag(h[0]), d1 = clamp_diag(h[3]), d2 = clamp_diag(h[5]);
    hd[0] += mu * d0 * d0; hd[3] += mu * d1 * d1; hd[5] += mu * d2 * d2;
    inv3sym(hd, hi);
  }
  double R[6];
  chol3(hi, R);
  if (lm_ok && lane == 0) {
    double* gg = P.grad + P.n + 3 * (size_t)l;
    double* hh = P.hdiag + P.n + 3 * (size_t)l;
    gg[0] = gl[0]; gg[1] = gl[1]; gg[2] = gl[2];
    hh[0] = h[0]; hh[1] = h[3]; hh[2] = h[5];
    double* hv = P.HllInv + 6 * (size_t)l;
#pragma unroll
    for (int k = 0; k < 6; ++k) hv[k] = hi[k];
    double* rt = P.lmRT + 9 * (size_t)l;  // R (6) | t = R^T g_l (3): what k_kf_reduce needs of this landmark
#pragma unroll
    for (int k = 0; k < 6; ++k) rt[k] = R[k];
    rt[6] = R[0] * gl[0] + R[1] * gl[1] + R[3] * gl[2];
    rt[7] = R[2] * gl[1] + R[4] * gl[2];
    rt[8] = R[5] * gl[2];
  }
  // per-block cost partial (summed in a fixed order by k_cost_finish)
  cost = wave_sum(cost);
  __shared__ double scost[kBuildThreads / 64];
  if ((threadIdx.x & 63) == 0) scost[threadIdx.x >> 6] = cost;
  __syncthreads();
  if (threadIdx.x == 0) {
    double c4 = 0.0;
#pragma unroll
    for (int k = 0; k < kBuildThreads / 64; ++k) c4 += scost[k];
    P.cost_part[blockIdx.x] = c4;
  }

  // The records leave as whole cache lines: every lane puts its Z into the wave's LDS tile (64 records of 144 B), then lane q of the wave
  // stores 16-byte segment 64 m + q (m = 0..8) of the tile — part (64 m + q) % 9 of the record of lane (64 m + q) / 9, consecutive lanes
  // on consecutive 16 bytes — to that record's slot, handed round by shuffle; lanes without an observation hand out -1 and their
  // segments are skipped. The groups of a wave walk their chunks in step (wave barriers): as many as its longest landmark has.
  // (Before: nine 16-byte stores per lane to its own scattered record — 64 partial lines per store instruction; same bytes.)
  __shared__ __attribute__((aligned(16))) double2 ztile[kBuildThreads / 64][64 * 9];
  double2* tile = ztile[threadIdx.x >> 6];
  const int wl = threadIdx.x & 63;
  int wchunk = nchunk;
#pragma unroll
  for (int off = G; off < 64; off <<= 1) wchunk = max(wchunk, __shfl_xor(wchunk, off, 64));
  for (int c = 0; c < wchunk; ++c) {
    const int a = c * G + lane;
    int zp = -1;
    if (a < nobs) {
      if (nchunk > 1) {  // multi-chunk landmark: this chunk's Jacobians were overwritten above
        kf = P.obs_kf[o0 + a];
        eval_obs<true, UNI>(P, P.pose, P.lm, o0 + a, kf, l, e);
      }
      double Z[18];
      z_of(e, R, Z);
      zp = P.obs_zpos[o0 + a];  // 144-byte record, 16-byte aligned, in its keyframe's block
#pragma unroll
      for (int k = 0; k < 9; ++k) tile[9 * wl + k] = double2{Z[2 * k], Z[2 * k + 1]};
    }
    group_sync();
#pragma unroll
    for (int m = 0; m < 9; ++m) {
      const int s2 = 64 * m + wl, rec = s2 / 9, part = s2 - 9 * rec;
      const int zr = __shfl(zp, rec, 64);
      if (zr >= 0) reinterpret_cast<double2*>(P.obsZ)[9 * (size_t)zr + part] = tile[s2];
    }
    group_sync();   // the tile is free for the next chunk
  }
}

// cost = sum of the per-block partials in index order (deterministic), added to the cost scalar
__global__ __launch_bounds__(256) void k_cost_finish(DevProblem P, int nparts) {
  __shared__ double sc[256];
  double acc = 0.0;
  for (int k = threadIdx.x; k < nparts; k += 256) acc += P.cost_part[k];
  sc[threadIdx.x] = acc;
  __syncthreads();
  for (int s2 = 128; s2 > 0; s2 >>= 1) {
    if (threadIdx.x < s2) sc[threadIdx.x] += sc[threadIdx.x + s2];
    __syncthreads();
  }
  if (threadIdx.x == 0) P.part[(size_t)SC_COST * P.part_n + 0] = sc[0];
}

// One wave (= one workgroup) per keyframe: fixed-order sum over its observations. Lanes run over the OBSERVATIONS (lane l takes
// observations l, l+64, ...), each re-linearised from the cache-resident pose / landmark rows plus the landmark's factor R and
// t = R^T g_l (72 B); the 39 partial sums of every lane go through LDS and lane k adds column k in lane order.
template <bool UNI>
__global__ __launch_bounds__(64) void k_kf_reduce(DevProblem P) {
  __shared__ double sp[kRec][65];
  const int kf = blockIdx.x, lane = threadIdx.x;
  if (P.fixed[kf]) return;  // constant pose block: rows stay empty, finalize_diag turns them into identity
  const int o0 = P.kf_obs_ptr[kf], o1 = P.kf_obs_ptr[kf + 1];
  double part[kRec];
#pragma unroll
  for (int k = 0; k < kRec; ++k) part[k] = 0.0;
  for (int t = o0 + lane; t < o1; t += 64) {
    const int l = P.kobs_lm[t];
    const double* uvs = P.kobs + 3 * (size_t)t;
    ObsLin e;
    eval_obs_uvs<true, UNI>(P, P.pose, P.lm, uvs[0], uvs[1], uvs[2], kf, l, e);
    const double* rt = P.lmRT + 9 * (size_t)l;
    double R[6], Z[18];
#pragma unroll
    for (int k = 0; k < 6; ++k) R[k] = rt[k];
    const double t0 = rt[6], t1 = rt[7], t2 = rt[8];
    z_of(e, R, Z);
    int q = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int cc = 0; cc <= r; ++cc)
        part[q++] += e.jp[r] * e.jp[cc] + e.jp[6 + r] * e.jp[6 + cc] - (Z[3 * r] * Z[3 * cc] + Z[3 * r + 1] * Z[3 * cc + 1] + Z[3 * r + 2] * Z[3 * cc + 2]);
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      part[21 + r] += e.jp[r] * e.jp[r] + e.jp[6 + r] * e.jp[6 + r];
      part[27 + r] += e.jp[r] * e.r0 + e.jp[6 + r] * e.r1;
      part[33 + r] += Z[3 * r] * t0 + Z[3 * r + 1] * t1 + Z[3 * r + 2] * t2;
    }
  }
#pragma unroll
  for (int k = 0; k < kRec; ++k) sp[k][lane] = part[k];
  __syncthreads();
  double acc = 0.0;
  if (lane < kRec) {
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll
    for (int t = 0; t < 64; t += 4) { a0 += sp[lane][t]; a1 += sp[lane][t + 1]; a2 += sp[lane][t + 2]; a3 += sp[lane][t + 3]; }
    acc = (a0 + a1) + (a2 + a3);
  }
  const double gp = __shfl(acc, (lane >= 33 && lane < 39) ? lane - 6 : lane, 64);  // lanes 33..38 hold yg; fetch the matching gp
  const size_t base = (size_t)P.D * kf;
  const int pos = P.perm[kf];
  if (lane < 21) {
    int r = 0;
    while ((r + 1) * (r + 2) / 2 <= lane) ++r;
    const int c = lane - r * (r + 1) / 2;
    *c_entry(P, pos, pos, r, c) = acc;
  } else if (lane < 27) {
    P.hdiag[base + lane - 21] = acc;
  } else if (lane < 33) {
    P.grad[base + lane - 27] = acc;
  } else if (lane < 39) {
    P.bred[base + lane - 33] = acc - gp;
  }
}

// Sixteen lanes per covisible keyframe pair (eight pairs per workgroup): C[i,j] = -sum over the common landmarks of Z_i Z_j^T.
// Lanes run over the common LANDMARKS (lane g takes terms g, g+16, ...: each a 6x3 times 3x6 product of two 144-byte records),
// the 36 partial sums of every lane go through LDS and lane g adds entries g, g+16, g+32 in lane order.
// The records travel as whole cache lines: a trip is sixteen terms, its record list the (up to) sixteen records of the row
// keyframe followed by the sixteen of the column keyframe, and lane q of the pair's sixteen loads 16-byte segment 16 m + q
// (m = 0..8) of either half — part (16 m + q) % 9 of record (16 m + q) / 9, consecutive lanes on consecutive 16 bytes — into
// registers, from there into LDS, and every lane reads its own two records back (144-byte stride). The slots of the trip are read
// coalesced (lane q: term q) and handed round by shuffle. The next trip's segments are in flight while this one is multiplied.
// The staging buffer is the pair's own slice of sp, which is needed behind the loop only: only the pair's lanes (one wave) touch it.
// (Before: every lane fetched its own records as nine 16-byte loads each — 64 lanes of a load instruction in 64 different
//  records; same terms, same order of additions, same bits.)
// (The first version had lane = block entry, 36 of 64 lanes busy, every lane walking all common landmarks in sequence:
// 0.78 ms on the 5-agent map, the longest kernel of the linearisation.)
constexpr int kPairLanes = 16, kPairsPerWg = 8;
constexpr int kPairChunk = 64;   // consecutive workgroups (of kPairsPerWg pairs) that one XCD takes together
constexpr int kPairSeg = 9 * kPairLanes;   // 16-byte segments of one half (sixteen records) of a trip's record list
static_assert(2 * kPairSeg * 2 <= 36 * (kPairLanes + 1), "a trip's records fit the pair's slice of the reduction buffer");
static_assert((36 * (kPairLanes + 1)) % 2 == 0, "the slices are 16-byte aligned");
// the trips of one pair as lane g of its sixteen sees them
constexpr int kPairSort = kPairChunk * kPairsPerWg;   // slots that are sorted together: the pairs of one XCD chunk (its keyframe blocks stay the same)
// upload: DevProblem::pair_order. One workgroup per kPairSort consecutive pairs of the list: slot r of the chunk gets the pair of rank r by falling number of
// common landmarks (ties: list order); slots behind the last pair get -1. Every pair keeps its own terms and order of additions: its block does not depend
// on the slot that computes it.
__global__ __launch_bounds__(kPairSort) void k_pair_order(DevProblem P) {
  __shared__ int cnt[kPairSort];
  const int t = threadIdx.x, p = blockIdx.x * kPairSort + t;
  const int mine = p < P.npairs ? P.pair_ptr[p + 1] - P.pair_ptr[p] : -1;
  cnt[t] = mine;
  __syncthreads();
  int rank = 0;
  for (int u = 0; u < kPairSort; ++u) { const int o = cnt[u]; rank += (o > mine || (o == mine && u < t)) ? 1 : 0; }
  P.pair_order[blockIdx.x * kPairSort + rank] = p < P.npairs ? p : -1;
}
struct PairTrips {
  const int *pair_oa, *pair_ob;
  const double2* Zs;   // record of slot z: segments 9 z .. 9 z + 8
  int e0, e1, g;
  // this lane's term of trip t: its two slots (-> the shuffles of fetch)
  COV_DEV void slots(int t, int& oa, int& ob) const {
    const int e = e0 + kPairLanes * t + g;
    oa = e < e1 ? pair_oa[e] : 0; ob = e < e1 ? pair_ob[e] : 0;
  }
  // issues this lane's segments of trip t, only segments of whole valid records (terms below e1); returns the segments per half
  COV_DEV int fetch(int t, int oa, int ob, double2 (&ra)[9], double2 (&rb)[9]) const {
    const int left = e1 - e0 - kPairLanes * t;
    const int nseg = 9 * (left < 0 ? 0 : (left > kPairLanes ? kPairLanes : left));
#pragma unroll
    for (int m = 0; m < 9; ++m) {
      const int s = kPairLanes * m + g, rec = s / 9, part = s - 9 * rec;
      const int za = __shfl(oa, rec, kPairLanes), zb = __shfl(ob, rec, kPairLanes);
      ra[m] = s < nseg ? Zs[9 * (size_t)za + part] : double2{0.0, 0.0};
      rb[m] = s < nseg ? Zs[9 * (size_t)zb + part] : double2{0.0, 0.0};
    }
    return nseg;
  }
};
__global__ __launch_bounds__(kPairLanes * kPairsPerWg, 2) void k_pair_blocks(DevProblem P) {
  __shared__ __attribute__((aligned(16))) double sp[kPairsPerWg][36][kPairLanes + 1];
  const int grp = threadIdx.x / kPairLanes, g = threadIdx.x % kPairLanes;
  // XCD-aware order (round 5): workgroup b runs on XCD b % 8 (observed dispatch order; placement affects speed only). The pair list is sorted by
  // (row keyframe, column keyframe) in chain order, and the two keyframes' record blocks (60 KB each) are what a pair reads: with consecutive
  // pair groups dealt round-robin every XCD's L2 fetched every keyframe's block — eight copies of the 125 MB record array per pass. Each XCD
  // now takes contiguous CHUNKS of the list: its L2 holds the keyframe blocks around the row keyframes it is working on.
  // (contiguous EIGHTHS of the list were 36 us slower than the round-robin order — 314 against 279 us — although they cut the fetches 4.7x: the
  //  pairs' work is uneven along the list, one XCD finished last. Chunks of kPairChunk consecutive workgroups, dealt round-robin to the XCDs:
  //  a chunk spans ~10 row keyframes, an XCD gets every eighth chunk.)
  const int nblk = (P.npairs + kPairsPerWg - 1) / kPairsPerWg;
  const int kx = (int)blockIdx.x >> 3, xcd = (int)blockIdx.x & 7;
  const int lb = ((kx / kPairChunk) * 8 + xcd) * kPairChunk + kx % kPairChunk;
  // which pair this slot works on: inside every kPairSort consecutive slots the pairs are dealt by falling length (k_pair_order), so that the four pairs of
  // a wave, which walk their trips in step, and the two waves of a workgroup, which holds its LDS until both are through, are of a length
  const int p = lb < nblk ? P.pair_order[lb * kPairsPerWg + grp] : -1;
  const bool ok = p >= 0;
  const int e0 = ok ? P.pair_ptr[p] : 0, e1 = ok ? P.pair_ptr[p + 1] : 0;
  double acc[36];
#pragma unroll
  for (int k = 0; k < 36; ++k) acc[k] = 0.0;
  // the trips of the four pairs of a wave run in step (wave barriers): as many as its longest pair has, a pair that is through idles
  int ntrip = (e1 - e0 + kPairLanes - 1) / kPairLanes;
  ntrip = max(ntrip, __shfl_xor(ntrip, 16, 64));
  ntrip = max(ntrip, __shfl_xor(ntrip, 32, 64));
  double2* stage = reinterpret_cast<double2*>(&sp[grp][0][0]);   // [2][kPairSeg]: row keyframe's records, column keyframe's
  double2 ra[9], rb[9];
  const PairTrips T{P.pair_oa, P.pair_ob, reinterpret_cast<const double2*>(P.obsZ), e0, e1, g};
  int oa = 0, ob = 0, nseg = 0;
  if (ntrip > 0) {
    T.slots(0, oa, ob);
    nseg = T.fetch(0, oa, ob, ra, rb);
    T.slots(1, oa, ob);
  }
  for (int t = 0; t < ntrip; ++t) {
#pragma unroll
    for (int m = 0; m < 9; ++m) {
      const int s = kPairLanes * m + g;
      if (s < nseg) { stage[s] = ra[m]; stage[kPairSeg + s] = rb[m]; }
    }
    group_sync();
    const bool mine = 9 * g < nseg;   // this lane has a term in this trip
    if (t + 1 < ntrip) {
      nseg = T.fetch(t + 1, oa, ob, ra, rb);
      T.slots(t + 2, oa, ob);
    }
    if (mine) {
      const double2* y = stage + 9 * g;
      const double* w = reinterpret_cast<const double*>(stage + kPairSeg + 9 * g);
      double yv[18];
#pragma unroll
      for (int k = 0; k < 9; ++k) { const double2 a2 = y[k]; yv[2 * k] = a2.x; yv[2 * k + 1] = a2.y; }
      // (the column keyframe's record in two halves of three rows: the whole of it beside the next trip's segments costs registers the kernel does not have)
#pragma unroll
      for (int hc = 0; hc < 6; hc += 3) {
        double wv[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) wv[k] = w[3 * hc + k];
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
          for (int c = 0; c < 3; ++c) acc[6 * r + hc + c] += yv[3 * r] * wv[3 * c] + yv[3 * r + 1] * wv[3 * c + 1] + yv[3 * r + 2] * wv[3 * c + 2];
      }
    }
    group_sync();   // every lane has read its records: the next trip (or the partial sums) may overwrite them
  }
#pragma unroll
  for (int k = 0; k < 36; ++k) sp[grp][k][g] = acc[k];
  __syncthreads();
  if (!ok) return;
  const int pi = P.pair_i[p], pj = P.pair_j[p];
  for (int k = g; k < 36; k += kPairLanes) {
    double a0 = 0.0, a1 = 0.0;
#pragma unroll
    for (int t = 0; t < kPairLanes; t += 2) { a0 += sp[grp][k][t]; a1 += sp[grp][k][t + 1]; }
    *c_entry(P, pi, pj, k / 6, k % 6) = -(a0 + a1);
  }
}

// (Measured, round 8, 5-agent map, kernel trace of 70 passes, beside k_kf_reduce on the side stream: 270-272 us before; 264 us with the cooperative
//  gathers alone — the 144-byte records straddle two 128-byte lines each whoever loads them, and the nine partial reads of a lane mostly hit in L1:
//  the pass moves the same lines and was not waiting for the load instructions; 244-252 us with the pairs of a chunk dealt by falling length as well:
//  in list order a wave walks as many trips as its longest pair has — 128 000 wave-trips on this map where 101 000 do — and a workgroup holds its
//  39 KB of LDS until its longest pair is through.)
// (Measured and dropped, round 4: one workgroup per keyframe i with i's records staged once in LDS (57.6 KB) so that only the partner's
//  records travel per common landmark — bit-identical, half the scattered reads, and SLOWER: 0.52 instead of 0.27 ms. One or two
//  workgroups per CU (77 KB of LDS each) cannot keep enough partner reads in flight; eight waves per CU with every read in flight can.)
// back-substitution: dl = Hinv (-g_l - sum_a W_a^T dp[kf_a]); written to out_all[n + 3l ..]
template <int G, bool UNI>
__global__ __launch_bounds__(kBuildThreads) void k_lm_backsub(DevProblem P, const double* __restrict__ dp, double* __restrict__ out_all) {
  constexpr int GROUPS = kBuildThreads / G;
  const int lane = threadIdx.x % G, grp = threadIdx.x / G;
  const int l = blockIdx.x * GROUPS + grp;
  const bool lm_ok = l < P.L;
  const int o0 = lm_ok ? P.lm_obs_ptr[l] : 0;
  const int nobs = lm_ok ? P.lm_obs_ptr[l + 1] - o0 : 0;
  double t[3] = {0, 0, 0};
  for (int a = lane; a < nobs; a += G) {
    ObsLin e;
    const int kf = P.obs_kf[o0 + a];
    eval_obs<true, UNI>(P, P.pose, P.lm, o0 + a, kf, l, e);
    const double* d = dp + (size_t)P.D * kf;
    // (W^T d)_c = sum_r (Jp^T Jl)[r][c] d[r] = sum_k Jl[k][c] (Jp[k] . d)
    const double s0 = e.jp[0] * d[0] + e.jp[1] * d[1] + e.jp[2] * d[2] + e.jp[3] * d[3] + e.jp[4] * d[4] + e.jp[5] * d[5];
    const double s1 = e.jp[6] * d[0] + e.jp[7] * d[1] + e.jp[8] * d[2] + e.jp[9] * d[3] + e.jp[10] * d[4] + e.jp[11] * d[5];
    t[0] += e.jl[0] * s0 + e.jl[3] * s1;
    t[1] += e.jl[1] * s0 + e.jl[4] * s1;
    t[2] += e.jl[2] * s0 + e.jl[5] * s1;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) t[k] = group_sum<G>(t[k]);
  if (lm_ok && lane == 0) {
    const double* gl = P.grad + P.n + 3 * (size_t)l;
    const double* hi = P.HllInv + 6 * (size_t)l;
    const double x = -gl[0] - t[0], y = -gl[1] - t[1], z = -gl[2] - t[2];
    double* o = out_all + P.n + 3 * (size_t)l;
    o[0] = hi[0] * x + hi[1] * y + hi[2] * z;
    o[1] = hi[1] * x + hi[3] * y + hi[4] * z;
    o[2] = hi[2] * x + hi[4] * y + hi[5] * z;
  }
}

// sum over observations of |Jp v_p[kf] + Jl v_l[lm]|^2
template <bool UNI>
__global__ __launch_bounds__(256) void k_obs_jvp(DevProblem P, const double* __restrict__ v_all) {
  double acc = 0.0;
  for (int o = blockIdx.x * blockDim.x + threadIdx.x; o < P.O; o += gridDim.x * blockDim.x) {
    ObsLin e;
    const int kf = P.obs_kf[o], l = P.obs_lm[o];
    eval_obs<true, UNI>(P, P.pose, P.lm, o, kf, l, e);
    const double* vp = v_all + (size_t)P.D * kf;
    const double* vl = v_all + P.n + 3 * (size_t)l;
    double s0 = e.jl[0] * vl[0] + e.jl[1] * vl[1] + e.jl[2] * vl[2];
    double s1 = e.jl[3] * vl[0] + e.jl[4] * vl[1] + e.jl[5] * vl[2];
#pragma unroll
    for (int k = 0; k < 6; ++k) { s0 += e.jp[k] * vp[k]; s1 += e.jp[6 + k] * vp[k]; }
    acc += s0 * s0 + s1 * s1;
  }
  acc = wave_sum(acc);
  part_put(P, SC_JV2, blockIdx.x * 4 + (threadIdx.x >> 6), acc);
}

template <bool UNI>
__global__ __launch_bounds__(256) void k_obs_cost(DevProblem P, const double* __restrict__ pose, const double* __restrict__ lm) {
  double acc = 0.0;
  for (int o = blockIdx.x * blockDim.x + threadIdx.x; o < P.O; o += gridDim.x * blockDim.x) {
    ObsLin e;
    eval_obs<false, UNI>(P, pose, lm, o, P.obs_kf[o], P.obs_lm[o], e);
    acc += e.cost;
  }
  acc = wave_sum(acc);
  part_put(P, SC_COST, blockIdx.x * 4 + (threadIdx.x >> 6), acc);
}

template <bool UNI>
__global__ __launch_bounds__(256) void k_obs_linearize(DevProblem P, double* r, double* Jp, double* Jl, double* cost) {
  const int o = blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= P.O) return;
  ObsLin e;
  eval_obs<true, UNI>(P, P.pose, P.lm, o, P.obs_kf[o], P.obs_lm[o], e);
  r[2 * o] = e.r0; r[2 * o + 1] = e.r1; cost[o] = e.cost;
  for (int k = 0; k < 12; ++k) Jp[12 * (size_t)o + k] = e.jp[k];
  for (int k = 0; k < 6; ++k) Jl[6 * (size_t)o + k] = e.jl[k];
}

template <bool UNI>
__global__ __launch_bounds__(256) void k_obs_norms(DevProblem P, double* norms) {
  const int o = blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= P.O) return;
  ObsLin e;
  eval_obs<false, UNI>(P, P.pose, P.lm, o, P.obs_kf[o], P.obs_lm[o], e);
  norms[o] = sqrt(e.r0 * e.r0 + e.r1 * e.r1);
}

static inline int stream_grid(int n) {
  const int b = (n + 255) / 256;
  return b < 1 ? 1 : (b > 2048 ? 2048 : b);  // memory-bound streams: cap at 8 blocks x 256 CUs, grid-stride the rest
}

// lanes per landmark of the landmark-major kernels (k_lm_lin, k_lm_backsub, k_lm_outliers): DevProblem::lm_group, chosen at upload from the map's mean
// track length (round 6) — the 5-agent map's tracks average 10 observations (16 lanes: 63 % of the lanes busy), configs[4]'s 4.1 (16 lanes: 25 %)
template <typename F> static void with_group(int g, F&& f) {
  if (g == 4) f(std::integral_constant<int, 4>()); else if (g == 8) f(std::integral_constant<int, 8>()); else f(std::integral_constant<int, 16>());
}
// unified cameras in the problem (DevProblem::uni): the UNI = true instantiations, else the pinhole-only ones
template <typename F> static void with_uni(const DevProblem& P, F&& f) {
  if (P.uni) f(std::true_type()); else f(std::false_type());
}
static int lm_blocks(const DevProblem& P) { const int g = P.lm_group == 4 || P.lm_group == 8 ? P.lm_group : 16; const int groups = kBuildThreads / g; return (P.L + groups - 1) / groups; }

// side != nullptr: the per-keyframe reduction (diagonal blocks, gradient, right-hand side: compute-heavy re-linearisation) runs on the
// side stream beside the pair pass (off-diagonal blocks: L2-bound record reads) — both follow the landmark pass only and write
// disjoint entries; whatever comes next on `st` follows both.
// first pass alone (per-observation records, per-landmark blocks, cost partials: touches nothing of the pose system) — the caller
// enqueues it ahead of the clearing of the fronts
void launch_lm_lin(const DevProblem& P, double mu, hipStream_t st, DevSignal sig) {
  if (P.L == 0) return;
  const int nblk = lm_blocks(P);
  with_uni(P, [&](auto U) { with_group(P.lm_group, [&](auto G) {
    hipLaunchKernelGGL((k_lm_lin<decltype(G)::value, decltype(U)::value>), dim3(nblk), dim3(kBuildThreads), 0, st, P, mu, sig); }); });
}
// the two passes that write the pose system, behind launch_lm_lin on `st`
void launch_lm_build(const DevProblem& P, double mu, hipStream_t st, hipEvent_t pose_system_cleared, hipStream_t side, hipEvent_t ev_lin, hipEvent_t ev_kf, CholAux* ax) {
  // (ordering through the context's device flags when the caller passes its CholAux, through HIP events otherwise: common.hpp)
  auto record = [&](hipEvent_t e, hipStream_t s) { if (ax) ax->record(e, s); else (void)hipEventRecord(e, s); };
  auto wait = [&](hipStream_t s, hipEvent_t e0, hipEvent_t e1 = nullptr) { if (ax) ax->wait(s, e0, e1); else { if (e0) (void)hipStreamWaitEvent(s, e0, 0); if (e1) (void)hipStreamWaitEvent(s, e1, 0); } };
  if (P.L == 0) { if (pose_system_cleared) wait(st, pose_system_cleared); return; }
  const int nblk = lm_blocks(P);
  const bool fork = side != nullptr && ev_lin != nullptr && ev_kf != nullptr && P.npairs > 0;
  hipStream_t s2 = fork ? side : st;
  // the side stream follows the landmark linearisation; the first writers of the pose system (both streams) follow the clearing of the fronts
  // (one gate for both on the side stream: the clearing ends long before the landmark pass)
  if (fork) { record(ev_lin, st); wait(s2, ev_lin, pose_system_cleared); if (pose_system_cleared) wait(st, pose_system_cleared); }
  else if (pose_system_cleared) wait(s2, pose_system_cleared);
  hipLaunchKernelGGL(k_cost_finish, dim3(1), dim3(256), 0, s2, P, nblk);
  with_uni(P, [&](auto U) { hipLaunchKernelGGL(k_kf_reduce<decltype(U)::value>, dim3(P.K), dim3(64), 0, s2, P); });
  if (P.npairs) {
    const int nblk = (P.npairs + kPairsPerWg - 1) / kPairsPerWg;
    const int nchunk8 = (nblk + 8 * kPairChunk - 1) / (8 * kPairChunk);   // rounds of eight chunks
    hipLaunchKernelGGL(k_pair_blocks, dim3(nchunk8 * 8 * kPairChunk), dim3(kPairLanes * kPairsPerWg), 0, st, P);
  }
  // (fork: the caller joins the side stream back — it has more on it)
}
// upload: keyframe-major copies of the observation stream (DevProblem::kobs), the Z slot of every observation, and the covisible-pair
// entries turned from observation indices into Z slots
__global__ __launch_bounds__(256) void k_kobs_build(DevProblem P) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= P.O) return;
  const int o = P.kf_obs_idx[t];
  P.kobs[3 * (size_t)t] = P.obs_u[o]; P.kobs[3 * (size_t)t + 1] = P.obs_v[o]; P.kobs[3 * (size_t)t + 2] = P.obs_sigma[o];
  P.kobs_lm[t] = P.obs_lm[o];
  P.obs_zpos[o] = t;
}
__global__ __launch_bounds__(256) void k_remap_idx(size_t n, int* __restrict__ a, int* __restrict__ b, const int* __restrict__ map) {
  const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (q < n) { a[q] = map[a[q]]; b[q] = map[b[q]]; }
}
void launch_kobs_build(const DevProblem& P, int* pair_oa, int* pair_ob, size_t nent, hipStream_t st) {
  if (P.O == 0) return;
  hipLaunchKernelGGL(k_kobs_build, dim3((P.O + 255) / 256), dim3(256), 0, st, P);
  if (nent > 0) hipLaunchKernelGGL(k_remap_idx, dim3((unsigned)((nent + 255) / 256)), dim3(256), 0, st, nent, pair_oa, pair_ob, (const int*)P.obs_zpos);
  if (P.npairs > 0) hipLaunchKernelGGL(k_pair_order, dim3((unsigned)(pair_order_slots(P.npairs) / kPairSort)), dim3(kPairSort), 0, st, P);
}
size_t pair_order_slots(int npairs) { return ((size_t)npairs + kPairSort - 1) / kPairSort * kPairSort; }
void launch_lm_backsub(const DevProblem& P, const double* dp, double* out_all, hipStream_t st) {
  if (P.L == 0) return;
  with_uni(P, [&](auto U) { with_group(P.lm_group, [&](auto G) {
    hipLaunchKernelGGL((k_lm_backsub<decltype(G)::value, decltype(U)::value>), dim3(lm_blocks(P)), dim3(kBuildThreads), 0, st, P, dp, out_all); }); });
}
void launch_obs_jvp(const DevProblem& P, const double* v_all, hipStream_t st) {
  if (P.O == 0) return;
  with_uni(P, [&](auto U) { hipLaunchKernelGGL(k_obs_jvp<decltype(U)::value>, dim3(stream_grid(P.O)), dim3(256), 0, st, P, v_all); });
}
void launch_obs_cost(const DevProblem& P, const double* pose, const double* lm, hipStream_t st) {
  if (P.O == 0) return;
  with_uni(P, [&](auto U) { hipLaunchKernelGGL(k_obs_cost<decltype(U)::value>, dim3(stream_grid(P.O)), dim3(256), 0, st, P, pose, lm); });
}
void launch_obs_linearize(const DevProblem& P, double* r, double* Jp, double* Jl, double* cost, hipStream_t st) {
  if (P.O == 0) return;
  with_uni(P, [&](auto U) { hipLaunchKernelGGL(k_obs_linearize<decltype(U)::value>, dim3((P.O + 255) / 256), dim3(256), 0, st, P, r, Jp, Jl, cost); });
}
// Map maintenance after the outlier round, on the device (optimization_be.cpp:270-290 + Map::Clean / RemoveLandmarkOutliers,
// map_be.cpp:448-454, 698-743): per observation "loss-corrected whitened residual norm > threshold -> erase", per landmark
// the number of observations it keeps; a landmark left with fewer than two is what RemoveLandmarkOutliers drops. One
// sub-wave group per landmark like the linearisation, the residual evaluated in place: only O bytes + L ints go back to
// the host instead of O doubles. counts[0] += erased observations, counts[1] += landmarks left with < 2.
template <int G, bool UNI>
__global__ __launch_bounds__(kBuildThreads) void k_lm_outliers(DevProblem P, double th, unsigned char* __restrict__ erase, int* __restrict__ left,
                                                               unsigned long long* __restrict__ counts) {
  constexpr int GROUPS = kBuildThreads / G;
  const int lane = threadIdx.x % G, grp = threadIdx.x / G;
  const int l = blockIdx.x * GROUPS + grp;
  const bool lm_ok = l < P.L;
  const int o0 = lm_ok ? P.lm_obs_ptr[l] : 0;
  const int nobs = lm_ok ? P.lm_obs_ptr[l + 1] - o0 : 0;
  double kept = 0.0, bad = 0.0;
  for (int a = lane; a < nobs; a += G) {
    ObsLin e;
    eval_obs<false, UNI>(P, P.pose, P.lm, o0 + a, P.obs_kf[o0 + a], l, e);
    const bool out = sqrt(e.r0 * e.r0 + e.r1 * e.r1) > th;
    erase[o0 + a] = out ? 1 : 0;
    kept += out ? 0.0 : 1.0; bad += out ? 1.0 : 0.0;
  }
  kept = group_sum<G>(kept); bad = group_sum<G>(bad);
  if (lm_ok && lane == 0) {
    left[l] = (int)kept;
    if (bad > 0.0) atomicAdd(&counts[0], (unsigned long long)bad);   // integer counters: order-independent
    if (kept < 2.0) atomicAdd(&counts[1], 1ull);
  }
}
void launch_lm_outliers(const DevProblem& P, double th, unsigned char* erase, int* left, unsigned long long* counts, hipStream_t st) {
  if (P.L == 0) return;
  with_uni(P, [&](auto U) { with_group(P.lm_group, [&](auto G) {
    hipLaunchKernelGGL((k_lm_outliers<decltype(G)::value, decltype(U)::value>), dim3(lm_blocks(P)), dim3(kBuildThreads), 0, st, P, th, erase, left, counts); }); });
}

void launch_obs_norms(const DevProblem& P, double* norms, hipStream_t st) {
  if (P.O == 0) return;
  with_uni(P, [&](auto U) { hipLaunchKernelGGL(k_obs_norms<decltype(U)::value>, dim3((P.O + 255) / 256), dim3(256), 0, st, P, norms); });
}

}  // namespace covgpu
