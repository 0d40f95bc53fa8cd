// k_bwd.hip — the backward substitution x = L^-T y of the dense FP64 Cholesky (k_chol.hip schedules it), every form of it:
//   k_bwd_step_sub  one launch per 128-tile: x_p = L_pp^-T y_p with the 16x16 block inverses k_potrf_panel (k_panel.hip) left behind,
//                   then y[cols left of the tile] -= L[tile rows, cols]^T x_p
//   k_bwd_given     all GIVEN tile rows of a front at once (the ancestors' unknowns, the border of an arrow block)
//   k_bwd_front     a whole multifrontal front of at most four interior tiles in one launch (ticket counter)
//   k_bwd_pipe      a level of fronts with many interior tiles in one launch: a pipeline of workgroups, the data words are the flags
//   k_bwd_pipe64    ... its form with 64x64 inverses for the few fronts at the top of the tree
//   k_bwd_tree      several levels in one launch of k_bwd_pipe's workgroups; k_bwd_tree64: of k_bwd_pipe64's
// The steps these forms share — the eight-step tile solve, the border product, the border's share in chunk order, a front's
// addressing, the column tile load, the publish and restore steps of the pipeline — are written once, above the kernels.
#include <cstdio>
#include <cstdlib>

#include <algorithm>

#include "common.hpp"
#include "dev_math.hpp"
#include "chain_dev.hpp"

namespace covgpu {

// Where front `batch` of a batched launch keeps its matrix and vectors: M / ld from the transfer table if there is one
template <class PM, class PY, class PX>   // (the kernels' pointers, __restrict__ and all)
COV_DEV void batch_operands(PM& M, size_t& ld, PY& y, PX& x, int batch, size_t bsM, size_t bsR, const long long* btab) {
  if (btab != nullptr) { M += (size_t)btab[2 * batch]; ld = (size_t)btab[2 * batch + 1]; }
  else M += (size_t)batch * bsM;
  y += (size_t)batch * bsR; x += (size_t)batch * bsR;
}

// ---- x_p = L_pp^-T v with the 16x16 block inverses -------------------------------------------------------------------
// Thread c < 128 (act) owns unknown c of the tile: row cl of its block's inverse ...
COV_DEV void load_block_inverse(double (&dv)[PB], const double* Dinv, bool act, int c) {
  const int jbc = c >> 4, cl = c & 15;
#pragma unroll
  for (int r = 0; r < PB; ++r) dv[r] = act ? Dinv[jbc * 256 + r * PB + cl] : 0.0;
}
// ... and every entry of L_pp it will need (rows of the blocks below its own), loaded up front: one memory latency
COV_DEV void load_blocks_below(double (&Lc)[7][PB], const double* M, size_t ld, int k0, bool act, int c) {
  const int jbc = c >> 4;
#pragma unroll
  for (int jb = 1; jb < 8; ++jb)
#pragma unroll
    for (int r = 0; r < PB; ++r) Lc[jb - 1][r] = (act && jbc < jb) ? M[(size_t)(k0 + PB * jb + r) * ld + k0 + c] : 0.0;
}
// Eight block steps of two barriers each, from the last block to the first: the block's v through `sv`, its x = Dinv^T v into `sx`,
// then v -= L[block jb rows, c] x for the unknowns left of it. blocks(jb, r): entry (PB jb + r, c) of the tile, jb >= 1; sx holds x_p at the end.
template <class Blocks, class Barrier>
COV_DEV void tile_backsolve(double v, const double (&dv)[PB], Blocks blocks, double* sx, double* sv, bool act, int c, Barrier barrier) {
  const int jbc = c >> 4;
#pragma unroll
  for (int jb = 7; jb >= 0; --jb) {
    if (act && jbc == jb) sv[c] = v;
    barrier();
    if (act && jbc == jb) {
      double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll
      for (int r = 0; r < PB; r += 4) {
        s0 += dv[r] * sv[PB * jb + r]; s1 += dv[r + 1] * sv[PB * jb + r + 1];
        s2 += dv[r + 2] * sv[PB * jb + r + 2]; s3 += dv[r + 3] * sv[PB * jb + r + 3];
      }
      sx[c] = (s0 + s1) + (s2 + s3);
    }
    barrier();
    if (jb > 0 && act && jbc < jb) {
      double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll
      for (int r = 0; r < PB; r += 4) {
        s0 += blocks(jb, r) * sx[PB * jb + r]; s1 += blocks(jb, r + 1) * sx[PB * jb + r + 1];
        s2 += blocks(jb, r + 2) * sx[PB * jb + r + 2]; s3 += blocks(jb, r + 3) * sx[PB * jb + r + 3];
      }
      v -= (s0 + s1) + (s2 + s3);
    }
  }
}

// ---- border product ----------------------------------------------------------------------------------------------------
// One wave's share of sum_r L[r][col, col + 1] x[r]: rows r_begin, r_begin + 4, .. below r_end (the four waves of the workgroup take every
// fourth row), eight double2 rows in flight. Lp: row 0 at this lane's column pair; sxg[r - x0] is the unknown of row r.
COV_DEV double2 border_rows_product(const double* Lp, size_t ld, const double* sxg, int x0, int r_begin, int r_end) {
  double2 acc = {0.0, 0.0};
  int r = r_begin;
  for (; r + 28 < r_end; r += 32) {
    double2 v[8]; double xv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) { v[u] = *reinterpret_cast<const double2*>(Lp + (size_t)(r + 4 * u) * ld); xv[u] = sxg[r + 4 * u - x0]; }
#pragma unroll
    for (int u = 0; u < 8; ++u) { acc.x += v[u].x * xv[u]; acc.y += v[u].y * xv[u]; }
  }
  for (; r < r_end; r += 4) { const double2 v = *reinterpret_cast<const double2*>(Lp + (size_t)r * ld); const double xv = sxg[r - x0]; acc.x += v.x * xv; acc.y += v.y * xv; }
  return acc;
}
// the four waves' partial sums added in wave order: deterministic
COV_DEV double2 sum_four_waves(const double2 (*part)[64], int lane) {
  const double2 a = part[0][lane], b = part[1][lane], c = part[2][lane], d = part[3][lane];
  return double2{((a.x + b.x) + c.x) + d.x, ((a.y + b.y) + c.y) + d.y};
}

// The border's share of a tile's right-hand side: v -= slot(q) for the chunks q < nch of the border, in chunk order.
// (eight partial sums in flight, subtracted in chunk order: one at a time each load was a dependent ~1.5 us round trip past the L2 —
//  10 chunks x 4 tiles = 60 us of a 69 us launch on the 5-agent map's upper levels)
template <class Slot>
COV_DEV void take_border_share(double& v, int nch, Slot slot) {
  for (int q0 = 0; q0 < nch; q0 += 8) {
    double t[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) t[u] = q0 + u < nch ? slot(q0 + u) : 0.0;
#pragma unroll
    for (int u = 0; u < 8; ++u) v -= t[u];
  }
}

// Backward substitution step for tile p with the 16x16 block inverses (Dinv == nullptr: x_p is given):
//   x_p = L_pp^-T y_p ; y[cols left of the tile] -= L[tile rows, cols]^T x_p.
// Every workgroup of the launch repeats the tile solve (cheaper than a separate launch on a launch-bound chain); the column
// update is split over the workgroups as before.
__global__ __launch_bounds__(256) void k_bwd_step_sub(const double* __restrict__ M, size_t ld, int p, const double* __restrict__ Dinv,
                                                       double* __restrict__ y, double* __restrict__ x, int ncol, size_t bsM, size_t bsL, size_t bsR,
                                                       const long long* __restrict__ btab, const int* __restrict__ live, int tI, BwdXfer xf) {
  if (live != nullptr) {  // padding tile of this front: x_p = 0 contributes nothing (GemmArgs::live)
    const int nI = live[2 * blockIdx.y], nO = live[2 * blockIdx.y + 1];
    if (!(p < nI || (p >= tI && p - tI < nO))) return;
  }
  batch_operands(M, ld, y, x, blockIdx.y, bsM, bsR, btab);
  if (Dinv != nullptr) Dinv += (size_t)blockIdx.y * bsL;
  __shared__ double sx[kTile];
  __shared__ double sv[kTile];
  __shared__ double part[8][33];
  const int tid = threadIdx.x, k0 = p * kTile;
  if (Dinv == nullptr) {
    if (tid < kTile) sx[tid] = x[k0 + tid];
    __syncthreads();
  } else {
    const int c = tid & 127;
    const bool act = tid < kTile;
    const double v = act ? y[k0 + c] : 0.0;
    double dv[PB], Lc[7][PB];
    load_block_inverse(dv, Dinv, act, c);
    load_blocks_below(Lc, M, ld, k0, act, c);
    tile_backsolve(v, dv, [&](int jb, int r) { return Lc[jb - 1][r]; }, sx, sv, act, c, [] { __syncthreads(); });
    if (blockIdx.x == 0 && tid < kTile) x[k0 + tid] = sx[tid];
    if (xf.gidx != nullptr && blockIdx.x == 0) {  // last step of a multifrontal front: its own unknowns -> solution vector
      const int node = xf.first + blockIdx.y, n = xf.own_dims[node];
      const int* gi = xf.gidx + xf.own_g[node];
      for (int i = tid; i < n; i += 256) xf.x[gi[i]] = (i < kTile) ? sx[i] : x[i];   // (tile 0 from LDS: p == 0 here)
    }
  }
  const int cl = tid & 31, rg = tid >> 5;
  const int col = blockIdx.x * 32 + cl;
  double acc = 0.0;
  if (col < ncol) {
    const double* Lc2 = M + (size_t)(k0 + 16 * rg) * ld + col;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc += Lc2[(size_t)r * ld] * sx[16 * rg + r];
  }
  part[rg][cl] = acc;
  __syncthreads();
  if (rg == 0 && col < ncol) {
    double t = 0.0;
#pragma unroll
    for (int g2 = 0; g2 < 8; ++g2) t += part[g2][cl];
    y[col] -= t;
  }
}

// Backward substitution, all GIVEN tile rows of a front at once (the ancestors' unknowns of a multifrontal front, the border
// of an arrow block): y[c] -= sum_{r in [r0, r1)} L[r][c] x[r] for the factored columns c < ncol. One workgroup per 128
// columns; its four waves take every fourth row (a row segment = 1 KiB, 16 rows in flight per wave), partial sums are added in
// wave order: deterministic. Replaces one launch per given tile (12 dependent launches for a 1.5k-row border).
__global__ __launch_bounds__(256) void k_bwd_given(const double* __restrict__ M, size_t ld, int r0, int r1, double* __restrict__ y,
                                                    const double* __restrict__ x, int ncol, size_t bsM, size_t bsR, const long long* __restrict__ btab,
                                                    const int* __restrict__ live, int tI, BwdXfer xf) {
  const int batch = blockIdx.y;
  if (live != nullptr) {  // rows beyond the front's real border are padding (x = 0); a front without interior columns has nothing to update
    r1 = min(r1, (tI + live[2 * batch + 1]) * kTile);
    if (live[2 * batch] == 0) return;
  }
  batch_operands(M, ld, y, x, batch, bsM, bsR, btab);
  __shared__ double2 part[4][64];
  extern __shared__ double sxg[];  // [r1 - r0] the given unknowns, staged once (a gather through the index list inside the row loop doubled its latency)
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int col = blockIdx.x * 128 + 2 * lane;
  // multifrontal front: the given unknowns come straight from the solution vector (row r0 + i = border scalar i of the front)
  if (xf.gidx != nullptr) {
    const int node = xf.first + batch;
    const int* gi = xf.gidx + xf.st_g[node];
    r1 = min(r1, r0 + xf.st_dims[node]);
    for (int i = threadIdx.x; i < r1 - r0; i += 256) sxg[i] = xf.x[gi[i]];
  } else {
    for (int i = threadIdx.x; i < r1 - r0; i += 256) sxg[i] = x[r0 + i];
  }
  __syncthreads();
  double2 acc = {0.0, 0.0};
  if (col < ncol) acc = border_rows_product(M + col, ld, sxg, r0, r0 + wv, r1);
  part[wv][lane] = acc;
  __syncthreads();
  if (wv == 0 && col < ncol) {
    const double2 t = sum_four_waves(part, lane);
    y[col] -= t.x;
    y[col + 1] -= t.y;
  }
}

// Backward substitution of a whole multifrontal front in ONE launch (fronts of at most four interior tiles: every level below
// the top of the tree). Workgroup (column tile ct, row chunk k) of a front forms the partial sums of
//   y[c] -= sum_r L[r][c] x[r]   over ITS 256 given rows (the ancestors' unknowns, read straight from the solution vector)
// for the 128 interior columns of tile ct and parks them in `scr`; the workgroup of the front that finishes LAST (ticket
// counter; nobody waits for anybody: no co-residency assumption) adds them in chunk order and solves the interior tiles from
// the last to the first: x_p = L_pp^-T y_p with the block inverses, y[cols left of the tile] -= L[tile rows, cols]^T x_p.
// Replaces 1 + (interior tiles) dependent launches per level whose first streamed a whole border through one workgroup per
// column tile (latency-bound: ~50 us for a 1.5k-row border).
__global__ __launch_bounds__(256) void k_bwd_front(const double* __restrict__ M, int tI, int nchunk, double* __restrict__ y, const double* __restrict__ Dinv_all,
                                                    size_t bsL, size_t bsR, const long long* __restrict__ btab, const int* __restrict__ live, BwdXfer xf,
                                                    int* __restrict__ cnt, double* __restrict__ scr) {
  const int batch = blockIdx.y, tid = threadIdx.x;
  const int ct = blockIdx.x / nchunk, k = blockIdx.x % nchunk;
  const int nIt = live[2 * batch];            // real interior tiles of this front
  const int node = xf.first + batch;
  const int nst = xf.st_dims[node];
  const int nch = max(1, (nst + 255) / 256);  // row chunks of this front
  if (ct >= nIt || k >= nch) return;
  M += (size_t)btab[2 * batch];
  const size_t ld = (size_t)btab[2 * batch + 1];
  y += (size_t)batch * bsR;
  const double* Dinv_f = Dinv_all + (size_t)batch * bsL;
  double* scr_f = scr + (size_t)batch * gridDim.x * kTile;   // [tile][chunk][128]
  __shared__ double2 part[4][64];
  __shared__ int s_ticket;
  __shared__ double sx[kTile], sv[kTile], sxg[256];
  {
    const int r0 = tI * kTile + 256 * k, nr = min(256, nst - 256 * k);   // this chunk's rows [r0, r0 + nr)
    const int* gi = xf.gidx + xf.st_g[node] + 256 * k;
    if (tid < nr) sxg[tid] = xf.x[gi[tid]];
    __syncthreads();
    const int lane = tid & 63, wv = tid >> 6;
    const int col = ct * kTile + 2 * lane;
    part[wv][lane] = border_rows_product(M + (size_t)r0 * ld + col, ld, sxg, 0, wv, nr);
    __syncthreads();
    if (wv == 0) {
      const double2 t = sum_four_waves(part, lane);
      double* dst = scr_f + ((size_t)ct * nchunk + k) * kTile + 2 * lane;
      __hip_atomic_store(dst, t.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(dst + 1, t.y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  // ---- ticket: the last workgroup of the front goes on. The partial sums travel through device-scope accesses (they bypass the
  //      per-XCD L2, which is not coherent across XCDs) and are complete (vmcnt) before the ticket is drawn; a device-scope FENCE
  //      here would write back and INVALIDATE the XCD's whole L2 under every workgroup that still streams its rows of L (measured:
  //      the sweep got slower than the separate launches).
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (a workgroup-scope release fence does not wait for the write-through stores)
  __syncthreads();
  if (tid == 0) s_ticket = __hip_atomic_fetch_add(&cnt[batch], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  if (s_ticket != nIt * nch - 1) return;
  if (tid == 0) __hip_atomic_store(&cnt[batch], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (next launch: ordered by the stream)
  for (int p = nIt - 1; p >= 0; --p) {
    const int k0 = p * kTile;
    const double* Dinv = Dinv_f + (size_t)p * kTile * kTile;
    {
      const int c = tid & 127;
      const bool act = tid < kTile;
      double v = act ? y[k0 + c] : 0.0;
      if (act)
        take_border_share(v, nch, [&](int q) { return __hip_atomic_load(scr_f + ((size_t)p * nchunk + q) * kTile + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); });
      double dv[PB], Lc[7][PB];
      load_block_inverse(dv, Dinv, act, c);
      load_blocks_below(Lc, M, ld, k0, act, c);
      tile_backsolve(v, dv, [&](int jb, int r) { return Lc[jb - 1][r]; }, sx, sv, act, c, [] { __syncthreads(); });
    }
    // own unknowns of this tile -> solution vector
    {
      const int n = xf.own_dims[node];
      const int* gi = xf.gidx + xf.own_g[node];
      if (tid < kTile && k0 + tid < n) xf.x[gi[k0 + tid]] = sx[tid];
    }
    // y[cols left of the tile] -= L[tile rows, cols]^T x_p: two groups of 64 rows per 128 columns, added in group order
    if (p > 0) {
      __shared__ double part2[2][kTile];
      const int cl = tid & 127, rg = tid >> 7;
      for (int c0 = 0; c0 < k0; c0 += kTile) {
        const double* Lc2 = M + (size_t)(k0 + 64 * rg) * ld + c0 + cl;
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll 4
        for (int r = 0; r < 64; r += 4) {
          a0 += Lc2[(size_t)r * ld] * sx[64 * rg + r]; a1 += Lc2[(size_t)(r + 1) * ld] * sx[64 * rg + r + 1];
          a2 += Lc2[(size_t)(r + 2) * ld] * sx[64 * rg + r + 2]; a3 += Lc2[(size_t)(r + 3) * ld] * sx[64 * rg + r + 3];
        }
        part2[rg][cl] = (a0 + a1) + (a2 + a3);
        __syncthreads();
        if (rg == 0) y[c0 + cl] -= part2[0][cl] + part2[1][cl];
        __syncthreads();
      }
    }
  }
}

// ---- Backward substitution of fronts with MANY interior tiles as ONE launch: a pipeline of workgroups (round 6) -----------------------------------
// The top of the elimination tree holds single fronts of 4 .. 16 interior tiles; one launch per tile (k_bwd_step_sub) costs 8.8 us a tile — a launch
// boundary (3.6 us under load) and two dependent memory latencies around 1 us of arithmetic — 141 us for the 5-agent map's root. Here every interior
// tile p has its own workgroup, all in one launch:
//   helpers     (tile ct, 256-row chunk k of the border): partial sums of y_ct -= L[border rows, ct]^T x_border, as in k_bwd_front
//   pipeline p  v = y_p - (its helpers' sums) - sum_{q > p} L[q, p]^T x_q, taking the x_q in the order they are solved (q = last .. p + 1; tile L[q, p]
//               is in registers before x_q arrives), then x_p = L_pp^-T v with the block inverses, publishes x_p, writes it to the solution vector.
// Hand-over between workgroups: the DATA WORDS are the flags. Every slot of `scr` / `xpub` holds kPipeEmpty (a NaN payload no arithmetic produces)
// between launches; the producer stores its values with agent-scope stores, the consumer polls the word it needs until it differs
// (tools/pipe_probe.hip: 0.6 us per hand-over across XCDs, against 1.15 for flag + data and 3.6 for a launch boundary). A helper's slot has one
// reader, which puts kPipeEmpty back; x_q is read by every pipeline workgroup p < q, the LAST of which (p = 0) restores the front's slots — by
// induction over the chain every other read has completed when workgroup 0 holds x_1. No counters, no clearing launch.
// Forward progress: a workgroup only waits for workgroups with a LOWER linear index (helpers first, then the tiles from the last to the first),
// which the dispatcher has started before it — no co-residency assumption. A wait beyond `limit` raises the gate's dead flag (CholAux::gate_failed:
// the solve is repeated on the launch-per-tile path and the context stays there).
static constexpr unsigned long long kPipeEmpty = 0x7ff8c0f6a11d0e5full;
struct BwdPipeArgs {
  const double* M; int tI, T, nchunk; double* y; const double* Dinv_all; size_t bsL, bsR; const long long* btab; const int* live; BwdXfer xf;
  double *scr, *xpub; int *dead, *dead_h; long long limit; int check;   // check: polls between two looks at the clock, minus one (a power of two)
  int fault;   // dev aid (COVGPU_PIPE_FAULT=1, tests): the first tile of every chain withholds its result — whoever waits for it runs into the limit
  int tree;    // k_bwd_tree (several levels in one launch): the ancestors' unknowns are POLLED in the solution vector (its entries of the merged levels
               // hold kPipeEmpty since k_nd_assemble), a front's own unknowns go there with agent-scope stores
};
COV_DEV double pipe_take(double* slot, const BwdPipeArgs& g, bool restore) {
  unsigned long long* w = reinterpret_cast<unsigned long long*>(slot);
  unsigned long long v;
  long long t0 = 0; int spins = 0;
  while ((v = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == kPipeEmpty) {
    __builtin_amdgcn_s_sleep(1);
    if ((++spins & g.check) == 0) {
      if (t0 == 0) t0 = wall_clock64();
      else if (wall_clock64() - t0 > g.limit || __hip_atomic_load(g.dead, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) {
        if (atomicExch(g.dead, 1) == 0) { g.dead_h[1] = -2; g.dead_h[2] = (int)blockIdx.x; g.dead_h[3] = (int)blockIdx.y; __threadfence_system(); g.dead_h[0] = 1; }
        v = 0ull; break;
      }
    }
  }
  if (restore) __hip_atomic_store(w, kPipeEmpty, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return __longlong_as_double((long long)v);
}
// What workgroup bx of front `batch` works on (helpers first: bx = tile * nchunk + chunk, then the tiles from the last to the first).
// p, k0 and Dinv are those of a tile workgroup; a helper (bx < T nchunk) gets p >= T and uses none of the three.
struct PipeFront {
  int nIt;                 // real interior tiles of this front
  int node, nst;
  int nch;                 // row chunks of this front's border (0: the root)
  const double* M; size_t ld;
  double* scr_f;           // [tile][chunk][128]
  double* xpub_f;          // [tile][128]
  double* y; const double* Dinv;
  int p, k0;
};
COV_DEV PipeFront pipe_front(const BwdPipeArgs& g, int bx, int batch) {
  PipeFront f;
  f.nIt = g.live[2 * batch];
  f.node = g.xf.first + batch;
  f.nst = g.xf.st_dims[f.node];
  f.nch = (f.nst + kPipeChunk - 1) / kPipeChunk;
  f.M = g.M + (size_t)g.btab[2 * batch];
  f.ld = (size_t)g.btab[2 * batch + 1];
  f.scr_f = g.scr + (size_t)batch * g.T * g.nchunk * kTile;
  f.xpub_f = g.xpub + (size_t)batch * g.T * kTile;
  f.p = g.T - 1 - (bx - g.T * g.nchunk);
  f.k0 = f.p * kTile;
  f.y = g.y + (size_t)batch * g.bsR;
  f.Dinv = g.Dinv_all + (size_t)batch * g.bsL + (size_t)f.p * kTile * kTile;
  return f;
}
// rows 64 h .. 64 h + 63 of tile L[q, p], column c: the part of the product with x_q this lane forms
COV_DEV void load_column_tile(double (&Lq)[64], const PipeFront& f, int q, int h, int c) {
  const double* src = f.M + (size_t)(q * kTile + 64 * h) * f.ld + f.k0 + c;
#pragma unroll
  for (int r = 0; r < 64; ++r) Lq[r] = src[(size_t)r * f.ld];
}
// unknown idx of tile p is solved: to the tiles that wait for it, and to entry gi of the solution vector (gi < 0: beyond the front's own unknowns)
COV_DEV void publish_x(const BwdPipeArgs& g, const PipeFront& f, int idx, double value, int gi) {
  if (f.p > 0 && !(g.fault && f.p == f.nIt - 1)) __hip_atomic_store(f.xpub_f + (size_t)f.p * kTile + idx, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (gi >= 0) {   // own unknowns of this tile -> solution vector
    if (g.tree) __hip_atomic_store(g.xf.x + gi, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else g.xf.x[gi] = value;
  }
}
// the last tile of the chain has seen every x_q of the front, and so has everybody else by then: the slots are free again
COV_DEV void restore_xpub(const PipeFront& f, int tid) {
  if (f.p == 0)
    for (int i = kTile + tid; i < f.nIt * kTile; i += 256)
      __hip_atomic_store(reinterpret_cast<unsigned long long*>(f.xpub_f + i), kPipeEmpty, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// helper workgroup hx = tile * nchunk + chunk of front `batch`: its kPipeChunk border rows' share of y_tile, into its slot of `scr`.
// ALL its rows of L are in registers (32 double2 a lane) before the ancestors' unknowns are gathered: what follows their arrival is arithmetic only.
// (First form: 256 rows a workgroup in eight batches of eight loads — eight dependent memory latencies, ~10 us of every level's ~20.)
COV_DEV void bwd_pipe_helper(const BwdPipeArgs& g, int hx, int batch, double* sxg /* [kPipeChunk] */, double2 (*part)[64]) {
  const int tid = threadIdx.x;
  const PipeFront f = pipe_front(g, hx, batch);
  const int ct = hx / g.nchunk, k = hx % g.nchunk;
  if (ct >= f.nIt || k >= f.nch) return;
  const int r0 = g.tI * kTile + kPipeChunk * k, nr = min(kPipeChunk, f.nst - kPipeChunk * k);
  const int lane = tid & 63, wv = tid >> 6;
  const int col = ct * kTile + 2 * lane;
  const double* Lp = f.M + (size_t)r0 * f.ld + col;
  static_assert(kPipeChunk == 128, "32 rows a wave");
  double2 v[32];
#pragma unroll
  for (int u = 0; u < 32; ++u) v[u] = (wv + 4 * u < nr) ? *reinterpret_cast<const double2*>(Lp + (size_t)(wv + 4 * u) * f.ld) : double2{0.0, 0.0};
  const int* gi = g.xf.gidx + g.xf.st_g[f.node] + kPipeChunk * k;
  if (tid < kPipeChunk) sxg[tid] = tid < nr ? (g.tree ? pipe_take(g.xf.x + gi[tid], g, false) : g.xf.x[gi[tid]]) : 0.0;
  __syncthreads();
  double2 a0 = {0.0, 0.0}, a1 = {0.0, 0.0};
#pragma unroll
  for (int u = 0; u < 32; u += 2) {
    const double x0 = sxg[wv + 4 * u], x1 = sxg[wv + 4 * u + 4];
    a0.x += v[u].x * x0; a0.y += v[u].y * x0; a1.x += v[u + 1].x * x1; a1.y += v[u + 1].y * x1;
  }
  part[wv][lane] = double2{a0.x + a1.x, a0.y + a1.y};
  __syncthreads();
  if (wv == 0) {
    const double2 t = sum_four_waves(part, lane);
    double* dst = f.scr_f + ((size_t)ct * g.nchunk + k) * kTile + 2 * lane;
    __hip_atomic_store(dst, t.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(dst + 1, t.y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}
constexpr size_t kPipeLds = (size_t)128 * 7 * 8 * sizeof(double);   // the packed blocks of the diagonal tile
COV_DEV void bwd_pipe_body(const BwdPipeArgs& g, const int bx, const int batch) {   // bx: the workgroup's index inside its front (helpers first)
  const int tid = threadIdx.x;
  __shared__ double2 part[4][64];
  __shared__ double sx[kTile], sv[kTile], sxq[2][kTile], part2[2][kTile];
  if (bx < g.T * g.nchunk) { bwd_pipe_helper(g, bx, batch, &sxq[0][0], part); return; }
  const PipeFront f = pipe_front(g, bx, batch);
  if (f.p >= f.nIt) return;
  const int c = tid & 127, h = tid >> 7;
  const bool act = tid < kTile;
  // ---- everything this tile will need that is already there: the first tile of its column, y_p, the diagonal tile
  double v = act ? f.y[f.k0 + c] : 0.0;
  const int n_own = g.xf.own_dims[f.node];
  const int gi_own = (act && f.k0 + c < n_own) ? g.xf.gidx[g.xf.own_g[f.node] + f.k0 + c] : -1;   // (loaded here, not between the last sum and its store)
  double dv[PB];
  load_block_inverse(dv, f.Dinv, act, c);
  // (the diagonal tile's blocks below the block diagonal go to LDS, packed by block row jb = 1 .. 7: [16 rows][16 jb columns] at 128 jb (jb - 1) —
  //  in registers, as k_bwd_step_sub holds them, they and the column tile above exceed the register file)
  extern __shared__ double sLc[];
#pragma unroll
  for (int jb = 1; jb < 8; ++jb)
#pragma unroll
    for (int rr = 0; rr < PB; rr += 2) {
      const int r = rr + h;
      if (c < PB * jb) sLc[128 * jb * (jb - 1) + r * PB * jb + c] = f.M[(size_t)(f.k0 + PB * jb + r) * f.ld + f.k0 + c];
    }
  // ---- the border's share (helpers), in chunk order
  if (act) take_border_share(v, f.nch, [&](int q) { return pipe_take(f.scr_f + ((size_t)f.p * g.nchunk + q) * kTile + c, g, true); });
  // ---- the tiles solved before this one, in the order they are solved
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#ifdef COVGPU_PIPE_PROBE
  long long tp0 = wall_clock64(), tp1 = 0, tp2 = 0, tp3 = 0, tp4 = 0;
#endif
  for (int q = f.nIt - 1; q > f.p; --q) {   // (tile L[q, p] is loaded at the top of its step, before the poll: see k_bwd_pipe64)
    double Lq[64];
    load_column_tile(Lq, f, q, h, c);
    if (act) sxq[q & 1][c] = pipe_take(f.xpub_f + (size_t)q * kTile + c, g, false);
    lds_barrier();
#ifdef COVGPU_PIPE_PROBE
    tp1 = wall_clock64();
#endif
    const double* xs = &sxq[q & 1][64 * h];
#pragma unroll
    for (int r = 0; r < 64; r += 4) { a0 += Lq[r] * xs[r]; a1 += Lq[r + 1] * xs[r + 1]; a2 += Lq[r + 2] * xs[r + 2]; a3 += Lq[r + 3] * xs[r + 3]; }
  }
  part2[h][c] = (a0 + a1) + (a2 + a3);
  lds_barrier();
  if (act) v -= part2[0][c] + part2[1][c];
#ifdef COVGPU_PIPE_PROBE
  tp2 = wall_clock64();
#endif
  // ---- x_p = L_pp^-T v (block inverses)
  tile_backsolve(v, dv, [&](int jb, int r) { return sLc[128 * jb * (jb - 1) + r * PB * jb + c]; }, sx, sv, act, c, [] { lds_barrier(); });
#ifdef COVGPU_PIPE_PROBE
  tp3 = wall_clock64();
#endif
  if (act) publish_x(g, f, c, sx[c], gi_own);
#ifdef COVGPU_PIPE_PROBE
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  tp4 = wall_clock64();
  if (tid == 0 && f.nst == 0) printf("pipe tile %2d: start %lld  last x in +%lld  gemv+reduce +%lld  solve +%lld  published +%lld (10 ns ticks)\n", f.p, tp0 % 100000000ll, tp1 - tp0, tp2 - tp1, tp3 - tp2, tp4 - tp3);
#endif
  restore_xpub(f, tid);
}
__global__ __launch_bounds__(256) void k_bwd_pipe(BwdPipeArgs g) { bwd_pipe_body(g, (int)blockIdx.x, (int)blockIdx.y); }
// The same pipeline for the FEW fronts at the top of the tree (at most 128 interior tiles in the launch), where the chain of tiles is the whole cost:
// measured on the 5-agent map's root, a tile of k_bwd_pipe costs 4.4 us — 0.6 hand-over, 1.0 the product with the newest x_q, 2.8 the eight-step
// substitution with the 16x16 block inverses (two barriers a step). Here every tile's workgroup first forms the INVERSES OF THE TWO 64x64 DIAGONAL
// BLOCKS of its tile by two doubling steps from the 16x16 inverses ([[A,0],[B,C]]^-1 = [[A^-1,0],[-C^-1 B A^-1, C^-1]]; ~2 us, while the chain is
// still far away for all but the first tile), and the substitution becomes three products of 16 terms a lane with wave-local sums:
//   x_hi = C^-T v_hi;  x_lo = A^-T (v_lo - B^T x_hi)        (three barriers instead of sixteen)
// and the product with x_q sums inside a wave too (column c's two half sums sit 32 lanes apart). The order of the workgroups is k_bwd_pipe's (helpers
// first): a workgroup takes a whole CU (111 KB of LDS), and with the tile workgroups first two contexts running this launch at once (virtual ranks of a
// sharded solve on one GPU) could fill every CU with tile workgroups that wait for helpers which find no room. Launches of more than 128 tile workgroups
// use k_bwd_pipe (eight to a CU).
constexpr int kP64W = 0, kP64S1 = 2 * 64 * 65, kP64S2 = kP64S1 + 4 * 16 * 17, kP64Y = kP64S2 + 2 * 32 * 33, kP64V = kP64Y + 2 * 32 * 33, kP64Doubles = kP64V + 128 + 128 + 64 + 256;
constexpr size_t kPipe64Lds = (size_t)kP64Doubles * sizeof(double);
COV_DEV void bwd_pipe64_body(const BwdPipeArgs& g, const int bx, const int batch) {
  extern __shared__ __attribute__((aligned(16))) double sm64[];
  const int tid = threadIdx.x;
  if (bx < g.T * g.nchunk) { bwd_pipe_helper(g, bx, batch, sm64, reinterpret_cast<double2(*)[64]>(sm64 + 256)); return; }
  const PipeFront f = pipe_front(g, bx, batch);
  if (f.p >= f.nIt) return;
  const double* M = f.M;
  const size_t ld = f.ld;
  const int k0 = f.k0;
  double (*W)[64][65] = reinterpret_cast<double (*)[64][65]>(sm64 + kP64W);     // the two 64x64 inverses (lower; zeros above the diagonal)
  double (*S1)[16][17] = reinterpret_cast<double (*)[16][17]>(sm64 + kP64S1);  // L blocks (2t+1, 2t) of the tile, t < 4
  double (*S2)[32][33] = reinterpret_cast<double (*)[32][33]>(sm64 + kP64S2);  // L blocks rows 64u+32.., cols 64u.., u < 2
  double (*Y2)[32][33] = reinterpret_cast<double (*)[32][33]>(sm64 + kP64Y);
  double (*Y1)[16][17] = reinterpret_cast<double (*)[16][17]>(sm64 + kP64Y);
  double* sx = sm64 + kP64V; double* sv = sx + 128; double* svlo = sv + 128; double* sxq = svlo + 64;   // sxq: [2][128]
  const int w = tid >> 6, l = tid & 63;
  const int c = 32 * w + (l & 31), h = l >> 5;      // product with x_q: column c, row half h
  const bool vh = h == 0;                           // ... and the lane that holds v[c]
  const int cc = 16 * w + (l & 15), gq = l >> 4;    // substitution: column cc of a 64-block, row group gq
  // ---- loads of everything that is already there: what the inverses need first (loads return in order), then the first tile of the column, y_p, B.
  //      (Every barrier below orders LDS traffic only: __syncthreads() would also wait for the loads and stores in flight — a memory latency each)
  double dreg[8], s1reg[4], s2reg[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) dreg[i] = f.Dinv[tid + 256 * i];
#pragma unroll
  for (int i = 0; i < 4; ++i) { const int e = tid + 256 * i, t = e >> 8, rr = (e >> 4) & 15, cx = e & 15; s1reg[i] = M[(size_t)(k0 + 32 * t + 16 + rr) * ld + k0 + 32 * t + cx]; }
#pragma unroll
  for (int i = 0; i < 8; ++i) { const int e = tid + 256 * i, u = e >> 10, rr = (e >> 5) & 31, cx = e & 31; s2reg[i] = M[(size_t)(k0 + 64 * u + 32 + rr) * ld + k0 + 64 * u + cx]; }
  double v = vh ? f.y[k0 + c] : 0.0;
  // (where this tile's unknowns go in the solution vector: the index loads would sit between the sums and the stores of the last steps)
  const int n_own = g.xf.own_dims[f.node];
  const int* gi = g.xf.gidx + g.xf.own_g[f.node];
  const int gi_hi = (gq == 0 && k0 + 64 + cc < n_own) ? gi[k0 + 64 + cc] : -1, gi_lo = (gq == 0 && k0 + cc < n_own) ? gi[k0 + cc] : -1;
  {
    for (int i = tid; i < 2 * 64 * 65; i += 256) sm64[kP64W + i] = 0.0;
    lds_barrier();
#pragma unroll
    for (int i = 0; i < 8; ++i) { const int e = tid + 256 * i, blk = e >> 8, rr = (e >> 4) & 15, cx = e & 15; W[blk >> 2][16 * (blk & 3) + rr][16 * (blk & 3) + cx] = dreg[i]; }
#pragma unroll
    for (int i = 0; i < 4; ++i) { const int e = tid + 256 * i; S1[e >> 8][(e >> 4) & 15][e & 15] = s1reg[i]; }
#pragma unroll
    for (int i = 0; i < 8; ++i) { const int e = tid + 256 * i; S2[e >> 10][(e >> 5) & 31][e & 31] = s2reg[i]; }
    lds_barrier();
  }
  double bb[16];   // (B of this tile: needed last, loaded once the staging registers are free)
#pragma unroll
  for (int i = 0; i < 16; ++i) bb[i] = M[(size_t)(k0 + 64 + 16 * gq + i) * ld + k0 + cc];
  {  // ---- 16 -> 32: four pairs, one per wave
    const int t = w, u = t >> 1, o = 32 * (t & 1), c1 = l & 15, r0 = 4 * (l >> 4);
    double yv[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const double d = W[u][o + k][o + c1];
#pragma unroll
      for (int i = 0; i < 4; ++i) yv[i] += S1[t][r0 + i][k] * d;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) Y1[t][r0 + i][c1] = yv[i];
    lds_barrier();
    double xv[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const double yk = Y1[t][k][c1];
#pragma unroll
      for (int i = 0; i < 4; ++i) xv[i] -= W[u][o + 16 + r0 + i][o + 16 + k] * yk;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) W[u][o + 16 + r0 + i][o + c1] = xv[i];
    lds_barrier();
  }
  {  // ---- 32 -> 64: two pairs, two waves each
    const int u = tid >> 7, l2 = tid & 127, c2 = l2 & 31, r0 = 8 * (l2 >> 5);
    double yv[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll 8
    for (int k = 0; k < 32; ++k) {
      const double d = W[u][k][c2];
#pragma unroll
      for (int i = 0; i < 8; ++i) yv[i] += S2[u][r0 + i][k] * d;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) Y2[u][r0 + i][c2] = yv[i];
    lds_barrier();
    double xv[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll 8
    for (int k = 0; k < 32; ++k) {
      const double yk = Y2[u][k][c2];
#pragma unroll
      for (int i = 0; i < 8; ++i) xv[i] -= W[u][32 + r0 + i][32 + k] * yk;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) W[u][32 + r0 + i][c2] = xv[i];
    lds_barrier();
  }
  double w1[16], w0[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) { w1[i] = W[1][16 * gq + i][cc]; w0[i] = W[0][16 * gq + i][cc]; }
  // ---- the border's share (helpers), in chunk order
  if (vh) take_border_share(v, f.nch, [&](int q) { return pipe_take(f.scr_f + ((size_t)f.p * g.nchunk + q) * kTile + c, g, true); });
  // ---- the tiles solved before this one, in the order they are solved
  // (tile L[q, p] is loaded at the top of the step that uses it, before x_q is polled — loads return in order, so the poll comes back behind it;
  //  a workgroup that keeps up with the chain spends that latency waiting for x_q anyway. Prefetching it a step ahead into the same registers made
  //  the compiler rotate 128 registers through copies every step: 1 us of a 3.8 us step)
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#ifdef COVGPU_PIPE_PROBE
  long long tp0 = wall_clock64(), tp1 = 0, tp2 = 0, tp3 = 0, tp4 = 0;
#endif
  for (int q = f.nIt - 1; q > f.p; --q) {
    double Lq[64];
    load_column_tile(Lq, f, q, h, c);
    if (vh) sxq[128 * (q & 1) + c] = pipe_take(f.xpub_f + (size_t)q * kTile + c, g, false);
    lds_barrier();
#ifdef COVGPU_PIPE_PROBE
    tp1 = wall_clock64();
#endif
    const double2* xs = reinterpret_cast<const double2*>(sxq + 128 * (q & 1) + 64 * h);
#pragma unroll
    for (int r = 0; r < 32; r += 2) {
      const double2 x0 = xs[r], x1 = xs[r + 1];
      a0 += Lq[2 * r] * x0.x; a1 += Lq[2 * r + 1] * x0.y; a2 += Lq[2 * r + 2] * x1.x; a3 += Lq[2 * r + 3] * x1.y;
    }
  }
  {
    double acc = (a0 + a1) + (a2 + a3);
    acc += __shfl_xor(acc, 32, 64);
    if (vh) { v -= acc; sv[c] = v; }
  }
  lds_barrier();
#ifdef COVGPU_PIPE_PROBE
  tp2 = wall_clock64();
#endif
  {  // x_hi = C^-T v_hi
    double s0 = 0.0, s1 = 0.0;
#pragma unroll
    for (int i = 0; i < 16; i += 2) { s0 += w1[i] * sv[64 + 16 * gq + i]; s1 += w1[i + 1] * sv[64 + 16 * gq + i + 1]; }
    double sum = s0 + s1;
    sum += __shfl_xor(sum, 16, 64); sum += __shfl_xor(sum, 32, 64);
    if (gq == 0) {
      sx[64 + cc] = sum;
      publish_x(g, f, 64 + cc, sum, gi_hi);
    }
  }
  lds_barrier();
  {  // v_lo - B^T x_hi
    double s0 = 0.0, s1 = 0.0;
#pragma unroll
    for (int i = 0; i < 16; i += 2) { s0 += bb[i] * sx[64 + 16 * gq + i]; s1 += bb[i + 1] * sx[64 + 16 * gq + i + 1]; }
    double sum = s0 + s1;
    sum += __shfl_xor(sum, 16, 64); sum += __shfl_xor(sum, 32, 64);
    if (gq == 0) svlo[cc] = sv[cc] - sum;
  }
  lds_barrier();
  {  // x_lo = A^-T (...)
    double s0 = 0.0, s1 = 0.0;
#pragma unroll
    for (int i = 0; i < 16; i += 2) { s0 += w0[i] * svlo[16 * gq + i]; s1 += w0[i + 1] * svlo[16 * gq + i + 1]; }
    double sum = s0 + s1;
    sum += __shfl_xor(sum, 16, 64); sum += __shfl_xor(sum, 32, 64);
    if (gq == 0) publish_x(g, f, cc, sum, gi_lo);
  }
#ifdef COVGPU_PIPE_PROBE
  tp3 = wall_clock64();
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  tp4 = wall_clock64();
  if (tid == 0 && f.nch == 0) printf("pipe64 tile %2d: start %lld  last x in +%lld  product +%lld  solve +%lld  stores done +%lld (10 ns ticks)\n", f.p, tp0 % 100000000ll, tp1 - tp0, tp2 - tp1, tp3 - tp2, tp4 - tp3);
#endif
  restore_xpub(f, tid);
}
__global__ __launch_bounds__(256) void k_bwd_pipe64(BwdPipeArgs g) { bwd_pipe64_body(g, (int)blockIdx.x, (int)blockIdx.y); }
// SEVERAL LEVELS of the tree in one launch (the bottom levels: hundreds of fronts of one or two interior tiles, ~20 us a level as launches of their
// own — a boundary, the gather of the ancestors' unknowns, the rows of L, the sums, the tile, the scatter, each a dependent memory latency). The
// levels stand in the grid from the highest to the lowest; a front's helpers POLL its ancestors' unknowns in the solution vector, whose entries of the
// merged levels k_nd_assemble filled with kPipeEmpty at the start of the solve (entries of higher levels hold values long since: the poll falls
// through), and the tile workgroups publish a front's own unknowns there with agent-scope stores. A workgroup still only waits for workgroups with a
// lower linear index. What a level loads that does not depend on the levels above — its rows of L, its block inverses — is in flight while it waits.
struct BwdTreeArgs { BwdPipeArgs base; BwdTreeLevel lev[kBwdTreeMax]; int wg0[kBwdTreeMax + 1]; int nlev; };
// the level this workgroup belongs to -> the arguments of that level's pipeline, the workgroup's index inside its front and the front
COV_DEV BwdPipeArgs tree_level(const BwdTreeArgs& a, int& bx, int& batch) {
  int l = 0;
  while (l + 1 < a.nlev && (int)blockIdx.x >= a.wg0[l + 1]) ++l;
  const BwdTreeLevel& L = a.lev[l];
  BwdPipeArgs g = a.base;
  g.tI = L.tI; g.T = L.T; g.nchunk = L.nchunk; g.y = L.y; g.Dinv_all = L.Dinv; g.bsL = L.bsL; g.bsR = L.bsR; g.btab = L.btab; g.live = L.live; g.xf.first = L.first;
  g.scr = a.base.scr + L.scr_off; g.xpub = a.base.scr + L.xpub_off; g.tree = 1;
  const int per = L.T * L.nchunk + L.T, local = (int)blockIdx.x - a.wg0[l];
  bx = local % per; batch = local / per;
  return g;
}
__global__ __launch_bounds__(256) void k_bwd_tree(BwdTreeArgs a) {
  int bx, batch;
  const BwdPipeArgs g = tree_level(a, bx, batch);
  bwd_pipe_body(g, bx, batch);
}
// ... and the TOP levels of the tree in one launch of k_bwd_pipe64's form (at most 128 tile workgroups in all)
__global__ __launch_bounds__(256) void k_bwd_tree64(BwdTreeArgs a) {
  int bx, batch;
  const BwdPipeArgs g = tree_level(a, bx, batch);
  bwd_pipe64_body(g, bx, batch);
}
__global__ void k_pipe_fill(unsigned long long* p, size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) p[i] = kPipeEmpty;
}
unsigned long long pipe_empty_word() { return kPipeEmpty; }
void launch_pipe_fill(double* buf, size_t n, hipStream_t st) {
  if (n > 0) hipLaunchKernelGGL(k_pipe_fill, dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, st, reinterpret_cast<unsigned long long*>(buf), n);
}

// ---- launch wrappers (k_chol.hip schedules them) ----------------------------------------------------------------------
// what every pipelined launch passes: the hand-over scratch, the dead flag, the limit of a wait and the two dev aids of the environment
static BwdPipeArgs pipe_args(const double* M, BwdXfer xf, double* pipe, int* dead, int* dead_h, double timeout_s, int tree) {
  static const int check = std::max(1, env_int("COVGPU_PIPE_SPIN_CHECK", 2048));   // (the test of the fallback: 1)
  static const int fault = env_int("COVGPU_PIPE_FAULT", 0);
  return BwdPipeArgs{M, 0, 0, 0, nullptr, nullptr, 0, 0, nullptr, nullptr, xf, pipe, pipe, dead, dead_h, (long long)(timeout_s * 1e8), check - 1, fault, tree};
}
static void set_pipe_attributes() {
  static std::atomic<unsigned long long> seen{0};
  if (!first_use_on_device(seen)) return;
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_bwd_pipe), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPipeLds);
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_bwd_tree), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPipeLds);
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_bwd_pipe64), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPipe64Lds);
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_bwd_tree64), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPipe64Lds);
}
void launch_bwd_tree(const double* M, const BwdTreeLevel* lev, int nlev, BwdXfer xf, double* pipe, int* dead, int* dead_h, double timeout_s, hipStream_t st, bool form64) {
  BwdTreeArgs a;
  a.base = pipe_args(M, xf, pipe, dead, dead_h, timeout_s, 1);
  a.nlev = nlev; a.wg0[0] = 0;
  size_t off = 0;
  for (int l = 0; l < nlev; ++l) {
    a.lev[l] = lev[l];
    a.lev[l].scr_off = off; off += (size_t)lev[l].nbt * lev[l].T * lev[l].nchunk * kTile;
    a.lev[l].xpub_off = off; off += (size_t)lev[l].nbt * lev[l].T * kTile;
    a.wg0[l + 1] = a.wg0[l] + lev[l].nbt * (lev[l].T * lev[l].nchunk + lev[l].T);
  }
  set_pipe_attributes();
  form_hit(form64 ? KF_BWD_TREE64 : KF_BWD_TREE);
  if (form64) hipLaunchKernelGGL(k_bwd_tree64, dim3(a.wg0[nlev]), dim3(256), kPipe64Lds, st, a);
  else hipLaunchKernelGGL(k_bwd_tree, dim3(a.wg0[nlev]), dim3(256), kPipeLds, st, a);
}
void launch_bwd_pipe(const double* S, int tI, int ntiles, int nchunk, double* y, const double* Linv, int nbt, size_t sL, size_t sR, hipStream_t st,
                     const long long* btab, const int* live, BwdXfer xf, double* pipe, int* dead, int* dead_h, double timeout_s) {
  BwdPipeArgs g = pipe_args(S, xf, pipe, dead, dead_h, timeout_s, 0);
  g.tI = tI; g.T = ntiles; g.nchunk = nchunk; g.y = y; g.Dinv_all = Linv; g.bsL = sL; g.bsR = sR; g.btab = btab; g.live = live;
  g.xpub = pipe + (size_t)nbt * ntiles * nchunk * kTile;
  set_pipe_attributes();
  // few tiles in the launch: the form with the 64x64 inverses (a whole CU per tile workgroup)
  constexpr int kPipe64Max = 128;
  const bool form64 = nbt * ntiles <= kPipe64Max;
  form_hit(form64 ? KF_BWD_PIPE64 : KF_BWD_PIPE);
  if (form64) hipLaunchKernelGGL(k_bwd_pipe64, dim3(ntiles * nchunk + ntiles, nbt), dim3(256), kPipe64Lds, st, g);
  else hipLaunchKernelGGL(k_bwd_pipe, dim3(ntiles * nchunk + ntiles, nbt), dim3(256), kPipeLds, st, g);
}

void launch_bwd_given(const double* S, size_t ld, int r0, int r1, double* y, double* x, int ncol, int nbt, size_t sM, size_t sR, hipStream_t st,
                      const long long* btab, const int* live, int tI, BwdXfer xf) {
  if (r1 <= r0 || ncol <= 0) return;
  form_hit(KF_BWD_GIVEN);
  hipLaunchKernelGGL(k_bwd_given, dim3((ncol + 127) / 128, nbt), dim3(256), (size_t)(r1 - r0) * sizeof(double), st, S, ld, r0, r1, y, (const double*)x, ncol, sM,
                     sR, btab, live, tI, xf);
}

void launch_bwd_front(const double* S, int tI, int ntiles, int nchunk, double* y, const double* Linv, int nbt, size_t sL, size_t sR, hipStream_t st,
                      const long long* btab, const int* live, BwdXfer xf, int* cnt, double* scr) {
  form_hit(KF_BWD_FRONT);
  hipLaunchKernelGGL(k_bwd_front, dim3(ntiles * nchunk, nbt), dim3(256), 0, st, S, tI, nchunk, y, Linv, sL, sR, btab, live, xf, cnt, scr);
}

void launch_bwd_step_sub(const double* S, size_t ld, int p, const double* Linv_p, double* y, double* x, int ncol, int nblocks, int nbt, size_t sM,
                         size_t sL, size_t sR, hipStream_t st, const long long* btab, const int* live, int tI, BwdXfer xf) {
  form_hit(KF_BWD_STEP_SUB);
  hipLaunchKernelGGL(k_bwd_step_sub, dim3(nblocks, nbt), dim3(256), 0, st, S, ld, p, Linv_p, y, x, ncol, sM, sL, sR, btab, live, tI, xf);
}

}  // namespace covgpu
