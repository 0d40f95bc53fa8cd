// k_prune.hip — Map::RemoveRedundantData (map_be.cpp:745-811) as an exact integer rule. A landmark with n live
// observations is worth v(n) tenths (0, 0, 0, 4, 7, 9, 10 for n = 0..6 and above: Keyframe::ComputeRedundancyValue,
// keyframe_be.cpp:228-256); a keyframe carries num = sum of v(n) and den = count over its live observations of valid landmarks with
// n >= 2, and its redundancy value is num / (10 den).
//
// Set-up, on the whole GPU: k_prune_init (keyframe flags), k_prune_count (live observations per landmark, observations per keyframe),
// k_prune_scan (one workgroup: the keyframe-major row pointers), k_prune_scatter (the keyframe-major landmark lists, num and den).
// The greedy loop: k_prune_loop, ONE workgroup of 1024 threads that runs every round. Per round: an argmax over the candidates on the
// total order (value by cross-multiplication in int64, den == 0 last, lowest index); thread 0 takes the stop and gate decisions,
// writes the round record and relinks the chain; on an erase the waves split the keyframe's landmarks, and a landmark whose count goes
// from o to o - 1 with o in 2..6 adds v(o-1) - v(o) to the num of every other live observer (and takes 1 off its den at o == 2) with
// int32 atomics. No workgroup waits on another, and every round takes one keyframe off the candidate list, so the loop ends.
// Everything the loop both writes and reads again (candidate and live flags, num, den) is read with agent-scope relaxed atomic
// loads and written with atomics or agent-scope atomic stores: the adds resolve in L2, and a plain load of the next round could hit
// a line this CU's L1 still holds. pred / succ and the valid count are thread 0's alone.
#include "common.hpp"

namespace covgpu {

namespace {

constexpr int kSetupThreads = 256;
constexpr int kNone = 0x7fffffff;   // "no candidate" in the argmax

__device__ __forceinline__ int ld_agent(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_agent(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void add_agent(int* p, int v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int tenths(int n) { return n <= 2 ? 0 : n == 3 ? 4 : n == 4 ? 7 : n == 5 ? 9 : 10; }

__global__ __launch_bounds__(kSetupThreads) void k_prune_init(PruneDev P) {
  const int k = blockIdx.x * kSetupThreads + threadIdx.x;
  if (k >= P.K) return;
  const int live = !(P.kf_invalid && P.kf_invalid[k]);
  P.live[k] = live;
  P.cand[k] = live && !(P.kf_first && P.kf_first[k]) && P.pred[k] >= 0 && P.succ[k] >= 0;
  P.num[k] = 0; P.den[k] = 0; P.cnt[k] = 0;
  P.out_num[k] = 0; P.out_den[k] = -1;   // -1: not handled by a round (k_prune_finish fills it in)
}

__global__ __launch_bounds__(kSetupThreads) void k_prune_count(PruneDev P) {
  const int l = blockIdx.x * kSetupThreads + threadIdx.x;
  if (l >= P.L) return;
  int n = 0;
  for (int j = P.lm_ptr[l]; j < P.lm_ptr[l + 1]; ++j) {
    const int k = P.obs_kf[j];
    n += P.live[k];
    atomicAdd(&P.cnt[k], 1);
  }
  P.lm_nobs[l] = n;
}

// exclusive scan of cnt [K] into kf_ptr [K+1]: one workgroup, a contiguous chunk per thread
__global__ __launch_bounds__(1024) void k_prune_scan(PruneDev P) {
  __shared__ int s[1024];
  const int t = threadIdx.x, chunk = (P.K + 1023) / 1024;
  const int k0 = min(t * chunk, P.K), k1 = min(k0 + chunk, P.K);
  int sum = 0;
  for (int k = k0; k < k1; ++k) sum += P.cnt[k];
  s[t] = sum;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {
    const int v = t >= d ? s[t - d] : 0;
    __syncthreads();
    s[t] += v;
    __syncthreads();
  }
  int run = s[t] - sum;
  for (int k = k0; k < k1; ++k) { P.kf_ptr[k] = run; run += P.cnt[k]; }
  if (t == 1023) P.kf_ptr[P.K] = s[1023];
}

__global__ __launch_bounds__(kSetupThreads) void k_prune_scatter(PruneDev P) {
  const int l = blockIdx.x * kSetupThreads + threadIdx.x;
  if (l >= P.L) return;
  const int n = P.lm_nobs[l];
  const bool counts = n >= 2 && !(P.lm_invalid && P.lm_invalid[l]);
  const int v = tenths(n);
  for (int j = P.lm_ptr[l]; j < P.lm_ptr[l + 1]; ++j) {
    const int k = P.obs_kf[j];
    const int slot = atomicSub(&P.cnt[k], 1) - 1;    // cnt[k] counts down from the keyframe's row length: every slot once
    P.kf_lm[P.kf_ptr[k] + slot] = l;
    if (counts && P.live[k]) { atomicAdd(&P.num[k], v); atomicAdd(&P.den[k], 1); }
  }
}

struct Pick { int num, den, k; };

// a ranks before b: larger num / den (both den > 0), den > 0 before den == 0, then the lower index. A total order on distinct k.
__device__ __forceinline__ bool before(const Pick& a, const Pick& b) {
  if (a.k == kNone) return false;
  if (b.k == kNone) return true;
  if ((a.den > 0) != (b.den > 0)) return a.den > 0;
  if (a.den > 0) {
    const long long l = (long long)a.num * b.den, r = (long long)b.num * a.den;
    if (l != r) return l > r;
  }
  return a.k < b.k;
}

__global__ __launch_bounds__(1024) void k_prune_loop(PruneDev P, PruneOptsDev O) {
  __shared__ Pick s_pick[16];
  __shared__ int s_k, s_action, s_stop;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  int valid = O.valid0, removed = 0;   // thread 0's
  int round = 0;
  for (;; ++round) {
    Pick best{0, 0, kNone};
    for (int k = t; k < P.K; k += 1024) {
      if (!ld_agent(P.cand + k)) continue;
      const Pick c{ld_agent(P.num + k), ld_agent(P.den + k), k};
      if (before(c, best)) best = c;
    }
    for (int d = 32; d >= 1; d >>= 1) {
      const Pick o{__shfl_xor(best.num, d, 64), __shfl_xor(best.den, d, 64), __shfl_xor(best.k, d, 64)};
      if (before(o, best)) best = o;
    }
    if (lane == 0) s_pick[wave] = best;
    __syncthreads();
    if (t == 0) {
      for (int w = 1; w < 16; ++w) if (before(s_pick[w], best)) best = s_pick[w];
      int stop = -1, action = 0;
      const int k = best.k;
      if (O.max_kfs >= 0 && valid <= O.max_kfs) stop = 2;
      else if (k == kNone) stop = 0;
      else if (O.max_kfs < 0 && (best.den == 0 || (double)best.num / (double)(10LL * best.den) < O.th_red)) stop = 1;
      else if (round == O.max_rounds) stop = 3;
      else {
        const int p = P.pred[k], s = P.succ[k];
        action = P.time[s] - P.time[p] >= O.max_time_dist ? 1 : (P.kf_loop && P.kf_loop[k]) ? 2 : (P.kf_not_erase && P.kf_not_erase[k]) ? 3 : 0;
        if (round < P.cap) { P.round_kf[round] = k; P.round_action[round] = action; }
        st_agent(P.cand + k, 0);
        P.out_num[k] = best.num; P.out_den[k] = best.den;
        removed += action == 0 || action == 3;
        if (action == 0) {
          st_agent(P.live + k, 0);
          --valid;
          P.succ[p] = s; P.pred[s] = p;
        }
      }
      s_k = k; s_action = action; s_stop = stop;
    }
    __syncthreads();
    if (s_stop >= 0) break;
    if (s_action == 0) {
      const int k = s_k;
      for (int i = P.kf_ptr[k] + wave; i < P.kf_ptr[k + 1]; i += 16) {
        const int l = P.kf_lm[i];
        int o = 0;
        if (lane == 0) o = __hip_atomic_fetch_add(P.lm_nobs + l, -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        o = __shfl(o, 0, 64);
        if (o < 2 || o > 6 || (P.lm_invalid && P.lm_invalid[l])) continue;
        const int delta = tenths(o - 1) - tenths(o);
        for (int j = P.lm_ptr[l] + lane; j < P.lm_ptr[l + 1]; j += 64) {
          const int k2 = P.obs_kf[j];
          if (k2 == k || !ld_agent(P.live + k2)) continue;
          if (delta) add_agent(P.num + k2, delta);
          if (o == 2) add_agent(P.den + k2, -1);
        }
      }
      __threadfence();   // the adds have reached L2 before any thread of the next round loads
    }
    __syncthreads();
  }
  if (t == 0) { P.result[0] = round; P.result[1] = removed; P.result[2] = s_stop; }
}

__global__ __launch_bounds__(kSetupThreads) void k_prune_finish(PruneDev P) {
  const int k = blockIdx.x * kSetupThreads + threadIdx.x;
  if (k >= P.K) return;
  if (P.out_den[k] < 0) { P.out_num[k] = P.num[k]; P.out_den[k] = P.den[k]; }
}

inline int blocks_for(int n) { return (n + kSetupThreads - 1) / kSetupThreads; }

}  // namespace

void launch_prune_setup(const PruneDev& P, hipStream_t st) {
  hipLaunchKernelGGL(k_prune_init, dim3(blocks_for(P.K)), dim3(kSetupThreads), 0, st, P);
  if (P.L > 0) hipLaunchKernelGGL(k_prune_count, dim3(blocks_for(P.L)), dim3(kSetupThreads), 0, st, P);
  hipLaunchKernelGGL(k_prune_scan, dim3(1), dim3(1024), 0, st, P);
  if (P.L > 0) hipLaunchKernelGGL(k_prune_scatter, dim3(blocks_for(P.L)), dim3(kSetupThreads), 0, st, P);
}

void launch_prune_loop(const PruneDev& P, const PruneOptsDev& O, hipStream_t st) {
  hipLaunchKernelGGL(k_prune_loop, dim3(1), dim3(1024), 0, st, P, O);
}

void launch_prune_finish(const PruneDev& P, hipStream_t st) {
  hipLaunchKernelGGL(k_prune_finish, dim3(blocks_for(P.K)), dim3(kSetupThreads), 0, st, P);
}

}  // namespace covgpu
