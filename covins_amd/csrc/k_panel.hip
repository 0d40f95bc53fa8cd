// k_panel.hip — the serial chain of the dense FP64 Cholesky (k_chol.hip), 256 columns per step.
//
// Replaces, like k_chol.hip, the linear-algebra half of ceres::Solve(SPARSE_SCHUR) (optimization_be.cpp:560-567,
// 1024-1031). With the fronts of the elimination tree the factorisation of the 5-agent map is 15 serial
// panels of pure latency. In round 2a a 256-column panel was potrf(128) -> TRSM -> rank-128 update -> potrf(128) -> TRSM ->
// next-diagonal update, six dependent launches of 20-80 us each with a 128x128 explicit inverse in the middle. Here the
// same panel is three launches and no large inverse:
//   k_potrf_panel   ONE workgroup (16 waves) factors the whole 256x256 diagonal block. The trailing 16x16 tiles live in
//                   REGISTERS in the MFMA accumulator layout for the whole kernel (119 tiles over the twelve waves of SIMDs
//                   1-3); only the current 16-column panel travels through LDS (double-buffered). Two barriers per block
//                   column: wave 0 carries the serial chain alone (diagonal block + its inverse in one sweep IN REGISTERS,
//                   rows exchanged by DPP row broadcasts -> the tile below it -> the next diagonal tile), the tile waves solve
//                   the rest of the panel against the block inverse on the matrix core and apply the panel to every trailing
//                   tile; L / y leave by whoever has the time. The right-hand side rides along as one more row. Leaves L in
//                   place, y = L^-1 b, and the INVERSES OF THE SIXTEEN 16x16 DIAGONAL BLOCKS. (Round 3: 8 waves, the sweep
//                   through LDS round trips, 87 us per launch; round 4: 60 us. tools/panel_probe.hip, tools/valu_probe.hip.)
//   k_trsm_sub4     X = A L^-T for 16-row slabs below the panel, FOUR waves per slab (one per SIMD): block forward
//                   substitution on Z = X^T kept in accumulator layout — a finished 16x16 block Z_j IS the B operand of the
//                   trailing updates acc_i -= L_ij Z_j (the C/D layout of v_mfma_f64_16x16x4 equals its B layout), and
//                   Z_j = Dinv_j acc_j needs only the small block inverses. Exact substitution between blocks: better
//                   conditioned than the product with a 128x128 explicit inverse it replaces. (Round 4's one wave per slab,
//                   bound by one SIMD's matrix pipe, is retired.)
// The backward substitution with the same block inverses has a file of its own: k_bwd.hip.
// A logical row permutation makes every MFMA operand a contiguous 32-byte load: hardware k-slot (lane>>4, step s) carries
// logical index 4*(lane>>4)+s instead of (lane>>4)+4*s — consistently for A and B, so products are unchanged.
#include <cstdio>
#include <cstdlib>

#include <algorithm>

#include "common.hpp"
#include "dev_math.hpp"
#include "chain_dev.hpp"
#include "leaf_front.hpp"

namespace covgpu {

typedef double v4f64 __attribute__((ext_vector_type(4)));

#ifdef COVGPU_PROBE
__device__ long long g_pprobe[8];
__device__ long long g_pstep[4][16];   // per step: wave 0 sweep done, wave 0 past X, wave 0 past Y, probed tile wave's updates done (relative to kernel start)
#define PSTEP(k, j, t0) do { if ((threadIdx.x & 63) == 0) g_pstep[k][j] = clock64() - (t0); } while (0)
__device__ long long g_parr[16][16];   // arrival of every wave at barrier X(j)
#define PARR(j, t0) do { if ((threadIdx.x & 63) == 0) g_parr[threadIdx.x >> 6][j] = clock64() - (t0); } while (0)
#ifndef PPROBE_WAVE
#define PPROBE_WAVE 1
#endif
// (accumulated in registers and written once: a global read-modify-write per phase costs more than the phases themselves)
#define PPROBE_DECL() long long pacc[8] = {0, 0, 0, 0, 0, 0, 0, 0}
#define PPROBE_ACC(i, t0) do { pacc[i] += clock64() - (t0); } while (0)
#define PPROBE_T0() clock64()
#define PPROBE_FLUSH() do { if (threadIdx.x == 0) for (int i_ = 1; i_ < 6; ++i_) g_pprobe[i_] = pacc[i_]; if (threadIdx.x == 64 * PPROBE_WAVE) { g_pprobe[6] = pacc[6]; g_pprobe[7] = pacc[7]; } } while (0)
#else
#define PPROBE_DECL() do {} while (0)
#define PPROBE_ACC(i, t0) do {} while (0)
#define PPROBE_T0() 0
#define PPROBE_FLUSH() do {} while (0)
#define PSTEP(k, j, t0) do {} while (0)
#define PARR(j, t0) do {} while (0)
#define PPROBE_WAVE 1
#endif

constexpr int PP = 18;                 // LDS pitch of a panel row (16 doubles + 2): rows 16-byte aligned, and the 16 lanes of a quarter wave
                                       // reading 32 bytes of 16 consecutive rows hit all 64 banks once (ds_read_b128, conflict-free)
constexpr int PROWS = 256;
constexpr int NW = 16;                 // waves of the panel workgroup: wave 0 carries the serial chain, waves 1..15 own the trailing tiles
constexpr int NSLOT = 10;              // tile slots per wave: 119 tiles (i, k), 1 <= k <= i <= 15 except (1,1), ~30 per SIMD, SIMD 0 with three tile waves
constexpr size_t kPanelLds = (size_t)(2 * PROWS * PP + 256 + 256 + 32 + 16 * PP) * sizeof(double);
// the four-wave form for fronts of at most 128 real columns in the panel (round 6): one chain wave + three tile waves, 128 panel rows
constexpr int PROWS4 = 128;
constexpr size_t kPanelLds4 = (size_t)(2 * PROWS4 * PP + 256 + PROWS4 + 32 + 16 * PP) * sizeof(double);

// lane id from the hardware, inside a volatile asm: it is re-issued where it is used (two VALU instructions) instead of being
// computed once, hoisted out of the step loop and reloaded from scratch — a memory latency on the serial chain per reload
COV_DEV int hw_lane_id() {
  int l;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
  return l;
}

// DPP row_newbcast (gfx90a+, the one DPP control 64-bit operations take): lane C of every 16-lane row to the whole row.
// Written as inline assembly because the compiler does not fold v_mov_b64_dpp into the multiply-add (a dependent pair per element, twice
// the instructions on the chain) — and therefore WITHOUT the compiler's hazard handling: a DPP source written by a VALU instruction needs
// two wait states (five after an EXEC write). diag_sweep keeps that distance by construction: the broadcast of the pivot carries its own
// s_nop, every multiply-add reads the register its predecessor of the PREVIOUS pivot wrote (>= 4 instructions earlier, asm volatile
// statements keep their order), and dpp_fence() separates the sweep from whatever wrote the registers before it.
template <int C> COV_DEV double dpp_bcast(double v) {
  double d;
  asm volatile("s_nop 1\n\tv_mov_b64_dpp %0, %1 row_newbcast:%2 row_mask:0xf bank_mask:0xf" : "=v"(d) : "v"(v), "n"(C));
  return d;
}
// acc += (acc of lane C of this row) * m
template <int C> COV_DEV void dpp_fmac(double& acc, double m) {
  asm volatile("v_fmac_f64_dpp %0, %0, %1 row_newbcast:%2 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(m), "n"(C));
}
COV_DEV void dpp_fence(double (&a)[16], double (&w)[4]) {
  asm volatile("s_nop 4" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]), "+v"(a[7]), "+v"(a[8]), "+v"(a[9]),
               "+v"(a[10]), "+v"(a[11]), "+v"(a[12]), "+v"(a[13]), "+v"(a[14]), "+v"(a[15]), "+v"(w[0]), "+v"(w[1]), "+v"(w[2]), "+v"(w[3]));
}

// Pivots C .. 15 of the diagonal-block sweep of k_potrf_panel's wave 0 (see there), unrolled by recursion: the DPP control is an immediate
template <int C> COV_DEV void diag_sweep(double (&a)[16], double (&w)[4], int r, bool& bad, double& rsr) {
  if constexpr (C < 16) {
    int rr = r;
    asm volatile("" : "+v"(rr));  // (lane masks recomputed per pivot instead of sixteen hoisted SGPR pairs)
    const double d = dpp_bcast<C>(a[C]);
    bad = bad || !(d > 0.0);  // (a non-positive pivot poisons the block with inf/NaN: flagged, the caller discards the solve)
    // 1/d: hardware estimate + two Newton steps arranged as r1 = r + r e, r2 = r1 + r1 e^2 (e = 1 - d r): three dependent
    // operations after the estimate instead of four
    const double r0 = __builtin_amdgcn_rcp(d);
    const double e0 = fma(-d, r0, 1.0);
    const double r1 = fma(r0, e0, r0), e1 = e0 * e0;
    const double rinv = fma(r1, e1, r1);
    const double nt = -(a[C] * rinv);
#pragma unroll
    for (int cc = C + 1; cc < 16; ++cc) dpp_fmac<C>(a[cc], nt);
    const double ntw = (rr > C) ? nt : 0.0;  // rows <= C of W are final rows of the inverse
#pragma unroll
    for (int e = 0; e < 4; ++e) dpp_fmac<C>(w[e], ntw);
    rsr = (rr == C) ? d : rsr;   // the lane's own pivot
    diag_sweep<C + 1>(a, w, r, bad, rsr);
  }
}

// acc (tile (i,k), accumulator layout: row = (lane>>4) + 4 reg, col = lane & 15) -= P_i P_k^T for the 16-column panel `pan`
COV_DEV v4f64 tile_update(v4f64 acc, const double* pan, int i, int k, int fr, int fk) {
  const double* pa = pan + (PB * i + fr) * PP + 4 * fk;
  const double* pb = pan + (PB * k + fr) * PP + 4 * fk;
  const double2 a01 = *reinterpret_cast<const double2*>(pa), a23 = *reinterpret_cast<const double2*>(pa + 2);
  const double2 b01 = *reinterpret_cast<const double2*>(pb), b23 = *reinterpret_cast<const double2*>(pb + 2);
  acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-a01.x, b01.x, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-a01.y, b01.y, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-a23.x, b23.x, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-a23.y, b23.y, acc, 0, 0, 0);
  return acc;
}

// the 119 trailing tiles (i, k), 1 <= k <= i <= 15 except (1,1), in column-major order, packed i | k << 8
struct PanelTileTab { int v[119]; };
constexpr PanelTileTab make_panel_tiles() {
  PanelTileTab t{};
  int u = 0;
  for (int k = 1; k < 16; ++k)
    for (int i = k; i < 16; ++i) { if (i == 1 && k == 1) continue; t.v[u++] = i | (k << 8); }
  return t;
}
__constant__ PanelTileTab kPanelTile = make_panel_tiles();
// the 27 trailing tiles of an 8-block panel (i, k), 1 <= k <= i <= 7 except (1,1), column-major (the four-wave form)
struct PanelTileTab8 { int v[27]; };
constexpr PanelTileTab8 make_panel_tiles8() {
  PanelTileTab8 t{};
  int u = 0;
  for (int k = 1; k < 8; ++k)
    for (int i = k; i < 8; ++i) { if (i == 1 && k == 1) continue; t.v[u++] = i | (k << 8); }
  return t;
}
__constant__ PanelTileTab8 kPanelTile8 = make_panel_tiles8();

// Panel j (LDS, complete: block column j of the factor from row o = 16 j on, raw diagonal block + its column factors `rs`) leaves for
// memory, and the right-hand side below it takes y_j (in sRhs[o ..)): thread u of NT, half rows of 64 bytes.
// LEAF (the one-launch leaf form, potrf_panel_body): logical rows from `nown` on are the front's border rows, `bshift` rows further down in
// memory; bo != nullptr (the last step): their right-hand side, now complete, leaves for bo[physical row].
template <int NT, bool LEAF = false>
COV_DEV void panel_out(const double* pan, double* sRhs, const double* rs, double* Mg, size_t ld, int o, int n, int u, double* yo, int nown = 0, int bshift = 0,
                       double* bo = nullptr) {
  for (int row = o + PB + (u >> 1); row < n; row += NT / 2) {
    const double2* src = reinterpret_cast<const double2*>(pan + row * PP + 8 * (u & 1));
    double2* dst = reinterpret_cast<double2*>(Mg + (size_t)(LEAF ? leaf_phys_row(row, nown, bshift) : row) * ld + o + 8 * (u & 1));
    const double2 v0 = src[0], v1 = src[1], v2 = src[2], v3 = src[3];
    dst[0] = v0; dst[1] = v1; dst[2] = v2; dst[3] = v3;
  }
  for (int e = NT - 1 - u; e < 256; e += NT) {  // the block's own rows: lower part, scaled by column (from the other end of the threads than the half rows)
    const int rr = e >> 4, cc = e & 15;
    if (cc <= rr) Mg[(size_t)(o + rr) * ld + o + cc] = pan[(o + rr) * PP + cc] * rs[cc];
  }
  for (int row = o + PB + (NT - 1 - u); row < n; row += NT) {
    double t0 = 0.0, t1 = 0.0, t2 = 0.0, t3 = 0.0;
#pragma unroll
    for (int c = 0; c < PB; c += 4) {
      t0 += sRhs[o + c] * pan[row * PP + c]; t1 += sRhs[o + c + 1] * pan[row * PP + c + 1];
      t2 += sRhs[o + c + 2] * pan[row * PP + c + 2]; t3 += sRhs[o + c + 3] * pan[row * PP + c + 3];
    }
    const double bv = sRhs[row] - ((t0 + t1) + (t2 + t3));
    sRhs[row] = bv;
    if (LEAF && bo != nullptr && row >= nown) bo[row + bshift] = bv;
  }
  if (yo != nullptr && u < PB) yo[o + u] = sRhs[o + u];
}

// Factor the (16 nb)-order diagonal block at (k0, k0), nb = 16 (a 256-column panel) or fewer (the last panel of a front).
// Dinv_out: block j at Dinv_out + (j >> 3) * 128*128 + (j & 7) * 256, [16][16] row-major (zeros above the diagonal).
//
// Sixteen waves, two roles, each a loop of its own (a wave's registers are then either the sweep's or the tiles'), two
// workgroup barriers per block column j:
//   wave 0 (the chain)    (a) diagonal block j  ->  X(j+1,j) = T(j+1,j) Dinv_j^T  ->  T(j+1,j+1) -= X X^T  ->  (a) diagonal block j+1 ...
//   waves on SIMDs 1-3    (twelve; wave w runs on SIMD w & 3) own the 119 trailing 16x16 tiles in REGISTERS in the MFMA accumulator
//                         layout, dealt round-robin in column-major order: between barriers X(j) and Y(j) they solve the remaining tiles of
//                         panel j (i >= j+2) against Dinv_j; between Y(j) and X(j+1) — while wave 0 already factors block j+1 — they apply
//                         panel j to block column j+1 (handed on through LDS), to the diagonal tile (j+2,j+2) (handed to wave 0 through sDg
//                         one step ahead) and to the rest of their tiles. The matrix pipe runs one v_mfma_f64_16x16x4 in 64 cycles,
//                         dependent or not (tools/valu_probe.hip): 680 tile updates of 4 are 24 us of three matrix pipes, and the first
//                         eight steps are bound by them, the last eight by wave 0's chain.
//                         L and y leave ONE STEP BEHIND (panel_out), in the solve phase.
//   waves 4, 8, 12        (SIMD 0, beside the chain wave, which takes every issue slot there during its sweep) help to fill LDS and exit.
// The diagonal-block sweep of wave 0 is described at its place in the loop; the rest of the panel is X_ij = T_ij Dinv_j^T, 4 MFMAs per
// tile. (What round 1 found too inaccurate for this system was ITS wide inverse: 128x128, formed inside the factorisation and applied
// to every row below. That finding is about that inverse, not about wide explicit inverses as such: the backward pass applies 64x64 inverses
// built from these 16x16 ones by two doubling steps — k_bwd_pipe64 — and holds the same tests. A 16x16 block inverse formed by substitution
// is the standard blocked-TRSM building block; tests/test_gpu_parity.py::test_mfma_cholesky_ill_conditioned_blocks and the full-size
// parity tests hold with it.)
// Round 6: (i) every front factors only ITS OWN real 16-column blocks of the panel (`own`: the launch-wide nb is the widest front's; a front's
// further blocks are identity padding — L = I, block inverses = I, y = 0 are in place and stay), and a launch lists only the fronts that have
// a real column in this panel (`list`): on the 12-agent map a level mixes 1 000-2 000 fronts of 9 .. 700 unknowns, and every one of them ran all
// the steps of the widest in every panel of the level — 16 of that map's 38 ms per iteration. (ii) NWV = 4: the same kernel with ONE chain wave and
// THREE tile waves (27 trailing tiles of an 8-block panel, 128 panel rows, 42 KB of LDS) for fronts of at most 128 real columns in the panel — the
// speed-bias segments and the small pose fronts, thousands per level: three workgroups per CU instead of one. The arithmetic of a front is the
// same in both forms (same tile updates in the same order).
// The one-launch LEAF form (LEAF, sixteen waves; leaf_front.hpp says which fronts take it): the working set is a WHOLE front of at most 256 rows, its
// own blocks 0 .. nbo-1 followed at once by its border blocks (in memory the border starts at row nI: leaf_phys_row), and the step loop stops
// behind the own blocks. The border rows of the panels are then L21, the right-hand side that rides along is y on the own rows and the updated
// right-hand side on the border rows, and the tiles left in the registers are the front's Schur complement: no substitution kernel, no update kernel
// and no round trip of L21 through memory between them. The border x border tiles are never cleared between iterations (k_nd_zero skips them, the
// first trailing update of the other route starts them from zero: GemmArgs::beta0) — their accumulators START FROM ZERO here and are never loaded.
// The complement leaves as the lower 16x16 tiles of the border x border block (diagonal tiles whole, both triangles, as the quadrant kernel leaves
// them): the extend-add reads max(row, column), min(row, column) only.
template <int NWV, bool LEAF = false>
COV_DEV void potrf_panel_body(double* __restrict__ M, size_t ld, int k0, int nb, double* __restrict__ Dinv_out, int* flag,
                              const double* __restrict__ rhs, double* __restrict__ yout, size_t bsM, size_t bsL, size_t bsR,
                              const long long* __restrict__ btab, const int* __restrict__ own, const int* __restrict__ list,
                              const int* __restrict__ stdim = nullptr, int nI = 0) {
  static_assert(!LEAF || NWV == 16, "the leaf form is a sixteen-wave form");
  constexpr int PROWS = (NWV == 16) ? 256 : PROWS4;   // (shadows the 16-wave constant)
  constexpr int NTW = (NWV == 16) ? 12 : 3;           // tile waves
  const int front = list != nullptr ? list[blockIdx.x] : (int)blockIdx.x;
  if (own != nullptr) {
    const int real = __builtin_amdgcn_readfirstlane(own[front]) - k0;
    nb = min(nb, (real + PB - 1) / PB);
    if (nb <= 0) return;   // (workgroup-uniform) no real column of this front in the panel
  }
  // block columns to factor | LEAF: logical rows from nown on are border rows, bshift rows further down in memory; nb becomes ALL blocks of the front
  const int nsteps = nb;
  int nown = 0, bshift = 0;
  if constexpr (LEAF) {
    nown = PB * nsteps; bshift = leaf_border_shift(nsteps, nI);
    nb = min(nsteps + leaf_blocks(__builtin_amdgcn_readfirstlane(stdim[front])), PROWS / PB);
  }
  if (btab != nullptr) { M += (size_t)btab[2 * front]; ld = (size_t)btab[2 * front + 1]; }  // fronts of unequal order (GemmArgs::btab)
  else M += (size_t)front * bsM;
  Dinv_out += (size_t)front * bsL;
  if (rhs != nullptr) { rhs += (size_t)front * bsR; yout += (size_t)front * bsR; }
  extern __shared__ __attribute__((aligned(16))) double sP[];  // panel[2][PROWS][PP] | sDv[16][16] | sRhs[PROWS] | sdd[2][16] | sDg[16][PP]
  double* sDv = sP + 2 * PROWS * PP;
  double* sRhs = sDv + 256;
  double* sdd = sRhs + PROWS;   // [2][16] 1/sqrt of the block's 16 pivots
  double* sDg = sdd + 32;       // [16][PP] the diagonal tile wave 0 takes over next (panels before the current one applied)
  const int tid0 = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid0 >> 6);
  const int n = PB * nb;
  double* Mg = M + (size_t)k0 * ld + k0;
  const long long tp0 = PPROBE_T0();

  // ---- block column 0 (its diagonal tile SYMMETRIC: an entry above the diagonal is read from its mirror image — the sweep of wave 0
  // wants whole rows), the diagonal tile (1,1) and the right-hand side go to LDS: by the four waves of SIMD 0 (a row per thread), which
  // own no tiles. The tile waves only ISSUE the loads of their tiles before the barrier behind the prologue (first needed at the end of
  // step 0) and go on to barrier X(0): the chain wave starts its sweep one memory round trip after the launch, beside them.
  auto fill_lds = [&]() {
    const int fid = (NWV == 16) ? 64 * (wave >> 2) + (tid0 & 63) : tid0;   // 0 .. 255 (four-wave form: every wave fills, then the tile waves load their tiles)
    double fv[PB], frhs = 0.0, fdg = 0.0;
#pragma unroll
    for (int c = 0; c < PB; ++c) fv[c] = 0.0;
    if (fid < n) {
      const int prow = LEAF ? leaf_phys_row(fid, nown, bshift) : fid;
      if (fid >= PB) {
#pragma unroll
        for (int c = 0; c < PB; c += 2) { const double2 v = *reinterpret_cast<const double2*>(Mg + (size_t)prow * ld + c); fv[c] = v.x; fv[c + 1] = v.y; }
      } else {
#pragma unroll
        for (int c = 0; c < PB; ++c) fv[c] = Mg[(size_t)(c > fid ? c : fid) * ld + (c > fid ? fid : c)];
      }
      if (rhs != nullptr) frhs = rhs[k0 + prow];
    }
    if (nb > 1 && (!LEAF || nsteps > 1)) {  // diagonal tile (1,1): wave 0 takes it over at step 0 (see below). LEAF, one own block: a border tile, from zero
      const int rr = fid >> 4, cc = fid & 15;
      fdg = Mg[(size_t)(PB + (cc <= rr ? rr : cc)) * ld + PB + (cc <= rr ? cc : rr)];
    }
    if (fid < n) {
#pragma unroll
      for (int c = 0; c < PB; c += 2) *reinterpret_cast<double2*>(sP + fid * PP + c) = double2{fv[c], fv[c + 1]};
    }
    if (fid < PROWS) sRhs[fid] = frhs;
    if (nb > 1) sDg[(fid >> 4) * PP + (fid & 15)] = fdg;
    // (no barrier of its own: the first one everybody meets is X(0); before it the chain wave only reads rows 0..15 of block column 0,
    //  which its own lanes have just written)
  };

  if (wave == 0) {
    // ================================================================ the chain
    PPROBE_DECL();
    fill_lds();
    PPROBE_ACC(4, tp0);
    __builtin_amdgcn_s_setprio(3);
    for (int j = 0; j < nsteps; ++j) {
      double* cur = sP + (j & 1) * PROWS * PP;          // block column j, rows 16 j .. n
      double* oth = sP + ((j + 1) & 1) * PROWS * PP;    // block column j+1 (being assembled)
      double* dv = sDv;
      const int o = PB * j;
      const long long tq0 = PPROBE_T0();
      // ---- (a): factor the diagonal block and form its inverse.
      // The sweep lives in REGISTERS, one matrix row per lane, and what a pivot needs of another row arrives by DPP row_newbcast (lane c
      // of every 16-lane row to the whole row) — no LDS round trip on the chain. Lane (r, g): a[0..15] = row r of the SYMMETRIC block (the
      // four 16-lane rows carry identical copies), w[0..3] = W[r][4g..4g+3] (W starts as I). Pivot c: d = a_c[c], t_r = a_r[c] / d (the
      // lane's own register), a_r[cc] -= t_r a_c[cc] for cc > c (both triangles: row c' must still be whole when its turn comes; rows <= c
      // turn into leftovers nobody reads), W_r: -= t_r W_c: for r > c — the forward substitution L X = I in outer-product form with the
      // same multipliers. L = A diag(d)^-1/2 and X = diag(d)^-1/2 W are scaled once at the end.
      const int ln = hw_lane_id();
      const int r = ln & 15, g = ln >> 4;
      double a[PB], w[4];
#pragma unroll
      for (int e = 0; e < PB; e += 2) { const double2 v = *reinterpret_cast<const double2*>(cur + (o + r) * PP + e); a[e] = v.x; a[e + 1] = v.y; }
#pragma unroll
      for (int e = 0; e < 4; ++e) w[e] = (4 * g + e == r) ? 1.0 : 0.0;
      bool bad = false;
      double rsr = 1.0;
      dpp_fence(a, w);
      diag_sweep<0>(a, w, r, bad, rsr);
      if (bad && ln == 0) atomicOr(flag, 1);
      // 1/sqrt(d_r), once per lane: X = diag(d)^-1/2 W (by row) here; L = A diag(d)^-1/2 (by column) is applied by the threads that store
      // L_jj (nobody reads it from LDS before): the raw columns and the sixteen factors go to LDS
      {
        const double dvv = (rsr > 0.0) ? rsr : 1.0;
        double rs = __builtin_amdgcn_rsq(dvv);
        rs = rs * (1.5 - 0.5 * dvv * rs * rs);
        rs = rs * (1.5 - 0.5 * dvv * rs * rs);
        rsr = rs;
      }
      if (ln < PB) {
        sdd[PB * (j & 1) + r] = rsr;   // (two buffers: the storing threads of step j run beside the sweep of step j + 1)
#pragma unroll
        for (int e = 0; e < PB; e += 2) *reinterpret_cast<double2*>(cur + (o + r) * PP + e) = double2{a[e], a[e + 1]};   // (above the diagonal: leftovers nobody reads)
      }
      double* dst = Dinv_out + (size_t)(j >> 3) * kTile * kTile + (size_t)(j & 7) * 256 + r * PB + 4 * g;
      double xv[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        xv[e] = (4 * g + e <= r) ? w[e] * rsr : 0.0;
        asm volatile("" : "+v"(xv[e]));  // selects, not a branch around the stores
        dv[r * PB + 4 * g + e] = xv[e];
        dst[e] = xv[e];
      }
      PPROBE_ACC(5, tq0);
      PSTEP(0, j, tp0);
      lds_barrier();  // ---- X(j): L_jj, Dinv_j in LDS; block column j complete in `cur`; trailing tiles carry panels < j
      PPROBE_ACC(1, tq0);
      PSTEP(1, j, tp0);
      const long long tq1 = PPROBE_T0();
      if (j + 1 < nb) {
        // X(j+1,j) = T(j+1,j) Dinv_j^T, formed TRANSPOSED — X^T = Dinv_j T^T, the operands of the same four instructions swapped (Dinv_j[r][4g..4g+3]
        // is what this lane holds) —: lane (r, g) then holds X[r][g], X[r][g+4], X[r][g+8], X[r][g+12], which IS an operand of the next diagonal
        // tile's update T(j+1,j+1) -= X X^T under the k-slot assignment (g, s) <-> column g + 4 s (any assignment does, taken for both
        // operands): no LDS round trip between the two products. The tile waves get X in row layout through `cur`, the next sweep the
        // updated tile through `oth`.
        double* tp = cur + (o + PB + r) * PP + 4 * g;
        const double2 ta = *reinterpret_cast<const double2*>(tp), tc = *reinterpret_cast<const double2*>(tp + 2);
        v4f64 dg;
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) dg[rg] = sDg[(g + 4 * rg) * PP + r];
        v4f64 xt = v4f64{0.0, 0.0, 0.0, 0.0};
        xt = __builtin_amdgcn_mfma_f64_16x16x4f64(xv[0], ta.x, xt, 0, 0, 0);
        xt = __builtin_amdgcn_mfma_f64_16x16x4f64(xv[1], ta.y, xt, 0, 0, 0);
        xt = __builtin_amdgcn_mfma_f64_16x16x4f64(xv[2], tc.x, xt, 0, 0, 0);
        xt = __builtin_amdgcn_mfma_f64_16x16x4f64(xv[3], tc.y, xt, 0, 0, 0);
#pragma unroll
        for (int s2 = 0; s2 < 4; ++s2) dg = __builtin_amdgcn_mfma_f64_16x16x4f64(-xt[s2], xt[s2], dg, 0, 0, 0);
#pragma unroll
        for (int s2 = 0; s2 < 4; ++s2) cur[(o + PB + r) * PP + g + 4 * s2] = xt[s2];
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) oth[(o + PB + g + 4 * rg) * PP + r] = dg[rg];
        if (LEAF && j + 1 == nsteps) {   // the first border tile of the Schur complement is this wave's: it leaves from here
          double* sc = Mg + (size_t)(nI + g) * ld + nI + r;
#pragma unroll
          for (int rg = 0; rg < 4; ++rg) sc[(size_t)(4 * rg) * ld] = dg[rg];
        }
      }
      lds_barrier();  // ---- Y(j): panel j complete in `cur`, the next diagonal tile in `oth`
      PPROBE_ACC(2, tq1);
      PSTEP(2, j, tp0);
    }
    __builtin_amdgcn_s_setprio(0);
    PPROBE_FLUSH();
    return;
  }

  // steps before it are bound by the matrix pipes (the chain wave waits), the last eight by the chain. LEAF: the loop ends after at most eight steps
  // with the border x border tiles still in the registers — every step is the matrix pipes', and the tile waves have the epilogue to run: all of SIMD 0's
  const int jsplit = LEAF ? nsteps : (NWV == 16 && nb > 8) ? nb - 8 : 0;
  double* const bout = LEAF ? const_cast<double*>(rhs) : nullptr;   // LEAF: the border rows' right-hand side goes back in place
  if (NWV == 16 && (wave & 3) == 0) {
    // ================================================================ SIMD 0's other waves: y_j, and the way out of panel j while the steps
    // are bound by the matrix pipes (the chain wave, which takes every issue slot of this SIMD during its sweep, then waits for the tiles)
    fill_lds();
    const int lq = tid0 & 63;
    for (int j = 0; j < nsteps; ++j) {
      const double* cur = sP + (j & 1) * PROWS * PP;
      const int o = PB * j;
      PARR(j, tp0);
      lds_barrier();  // ---- X(j)
      if (wave == 4 && lq < PB) {  // y_j = Dinv_j b_j
        double y0 = 0.0, y1 = 0.0, y2 = 0.0, y3 = 0.0;
#pragma unroll
        for (int k = 0; k < PB; k += 4) {
          y0 += sDv[lq * PB + k] * sRhs[o + k]; y1 += sDv[lq * PB + k + 1] * sRhs[o + k + 1];
          y2 += sDv[lq * PB + k + 2] * sRhs[o + k + 2]; y3 += sDv[lq * PB + k + 3] * sRhs[o + k + 3];
        }
        sRhs[o + lq] = (y0 + y1) + (y2 + y3);
      }
      lds_barrier();  // ---- Y(j)
      if (j < jsplit)
        panel_out<192, LEAF>(cur, sRhs, sdd + PB * (j & 1), Mg, ld, o, n, 64 * ((wave >> 2) - 1) + lq, yout != nullptr ? yout + k0 : nullptr, nown, bshift,
                             j + 1 == nsteps ? bout : nullptr);
      if (wave == PPROBE_WAVE) PSTEP(3, j, tp0);
    }
    return;
  }


  // ================================================================ the tile waves
  PPROBE_DECL();
  const int lane0 = tid0 & 63, fr0 = lane0 & 15, fk0 = lane0 >> 4;
  const int tw = (NWV == 16) ? 3 * (wave >> 2) + (wave & 3) - 1 : wave - 1;   // 0 .. NTW-1
  if (NWV != 16) fill_lds();
  // ---- tile slots of this wave (wave-uniform, packed i | k << 8; k = 99: none): the 119 tiles (i, k), 1 <= k <= i <= 15 except (1,1), in
  // column-major order, round-robin: every SIMD carries the same number of tiles at every step
  int tik[NSLOT];
#pragma unroll
  for (int s = 0; s < NSLOT; ++s) {
    const int u = NTW * s + tw;
    constexpr int NTILE = (NWV == 16) ? 119 : 27;
    const int pk = (NWV == 16) ? kPanelTile.v[u < NTILE ? u : 0] : kPanelTile8.v[u < NTILE ? u : 0];   // (a table: the search for the column was ~1 us of scalar loops per wave)
    tik[s] = (u < NTILE && (pk & 255) < nb) ? pk : (99 << 8);
  }
  // ---- the wave's trailing tiles into registers: the loads are only ISSUED here (see above): addresses from four per-lane offsets (and
  // four mirrored ones for the diagonal tiles, kept symmetric) and a wave-uniform base per tile; a slot without a tile loads tile (1,1)
  // and never looks at it again (a select would wait for the load)
  unsigned offn[4], offm[4];
#pragma unroll
  for (int rg = 0; rg < 4; ++rg) {
    const int rw = fk0 + 4 * rg;
    offn[rg] = (unsigned)rw * (unsigned)ld + (unsigned)fr0;
    offm[rg] = fr0 > rw ? (unsigned)fr0 * (unsigned)ld + (unsigned)rw : offn[rg];
  }
  v4f64 acc[NSLOT];
#pragma unroll
  for (int s = 0; s < NSLOT; ++s) {
    const bool on = (tik[s] >> 8) != 99;
    const int ii = on ? (tik[s] & 255) : 1, kk = on ? (tik[s] >> 8) : 1;
    if (LEAF && (!on || kk >= nsteps)) {   // (wave-uniform) a border x border tile: never cleared, never read — the complement starts from zero
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) acc[s][rg] = 0.0;
      continue;
    }
    const double* base = Mg + (size_t)(LEAF ? leaf_phys_row(PB * ii, nown, bshift) : PB * ii) * ld + PB * kk;   // (LEAF: kk is an own block here)
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) acc[s][rg] = base[ii == kk ? offm[rg] : offn[rg]];
  }
  // (The first step is as long as the tile loads take to issue, ~5 us: 244 KB into ONE CU at ~50 GB/s. Measured and dropped: half of them
  //  behind barrier X(0) — the conditional load inside the step loop costs 38 spilled registers —; 16-byte loads by lane pairs with a DPP
  //  swap behind X(0): half the instructions, the same time.)
  for (int j = 0; j < nsteps; ++j) {
    double* cur = sP + (j & 1) * PROWS * PP;
    double* oth = sP + ((j + 1) & 1) * PROWS * PP;
    const double* dv = sDv;
    // every per-lane constant of the step is rebuilt from the hardware lane id here: kept across the loop they are spilled
    // (the accumulator tiles take the registers) and every reload is a memory latency
    const int lq = hw_lane_id();
    const int fr = lq & 15, fk = lq >> 4;
    PARR(j, tp0);
    lds_barrier();  // ---- X(j)
    if (NWV != 16 && tw == 0 && lq < PB) {  // y_j = Dinv_j b_j (the 16-wave form: wave 4)
      const int o = PB * j;
      double y0 = 0.0, y1 = 0.0, y2 = 0.0, y3 = 0.0;
#pragma unroll
      for (int k = 0; k < PB; k += 4) {
        y0 += sDv[lq * PB + k] * sRhs[o + k]; y1 += sDv[lq * PB + k + 1] * sRhs[o + k + 1];
        y2 += sDv[lq * PB + k + 2] * sRhs[o + k + 2]; y3 += sDv[lq * PB + k + 3] * sRhs[o + k + 3];
      }
      sRhs[o + lq] = (y0 + y1) + (y2 + y3);
    }
    for (int i = j + 2 + tw; i < nb; i += NTW) {  // X(i,j) for i >= j+2
      double* tp = cur + (PB * i + fr) * PP + 4 * fk;
      const double* dp = dv + fr * PB + 4 * fk;
      const double2 ta = *reinterpret_cast<const double2*>(tp), tc = *reinterpret_cast<const double2*>(tp + 2);
      const double2 tb = *reinterpret_cast<const double2*>(dp), td = *reinterpret_cast<const double2*>(dp + 2);
      v4f64 x = v4f64{0.0, 0.0, 0.0, 0.0};
      x = __builtin_amdgcn_mfma_f64_16x16x4f64(ta.x, tb.x, x, 0, 0, 0);
      x = __builtin_amdgcn_mfma_f64_16x16x4f64(ta.y, tb.y, x, 0, 0, 0);
      x = __builtin_amdgcn_mfma_f64_16x16x4f64(tc.x, td.x, x, 0, 0, 0);
      x = __builtin_amdgcn_mfma_f64_16x16x4f64(tc.y, td.y, x, 0, 0, 0);
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) cur[(PB * i + fk + 4 * rg) * PP + fr] = x[rg];
    }
    lds_barrier();  // ---- Y(j): panel j complete in `cur`, the next diagonal tile in `oth`
    const long long tq2 = PPROBE_T0();
    // panel j onto every trailing tile of this wave; block column j+1 goes on to `oth` and the diagonal tile (j+2,j+2) to sDg on the way.
    // Tile (j+1,j+1) is wave 0's already.
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) {
      int pk = tik[s];
      asm volatile("" : "+s"(pk));  // keeps the LDS row addresses of all slots from being hoisted out of the j loop (spills)
      const int i = pk & 255, k = pk >> 8;
      if (k >= j + 1 && k != 99 && !(k == j + 1 && i == k)) {
        acc[s] = tile_update(acc[s], cur, i, k, fr, fk);
        if (k == j + 1 || (k == j + 2 && i == k)) {
          double* dstp = (i == k) ? sDg + fk * PP + fr : oth + (PB * i + fk) * PP + fr;
#pragma unroll
          for (int rg = 0; rg < 4; ++rg) dstp[4 * rg * PP] = acc[s][rg];
        }
      }
    }
    PPROBE_ACC(6, tq2);
    if (wave == PPROBE_WAVE) PSTEP(3, j, tp0);
    const long long tq3 = PPROBE_T0();
    if (j >= jsplit) panel_out<64 * NTW>(cur, sRhs, sdd + PB * (j & 1), Mg, ld, PB * j, n, 64 * tw + lq, yout != nullptr ? yout + k0 : nullptr);   // (the tile waves have the time now)
    PPROBE_ACC(7, tq3);
  }
  if constexpr (LEAF) {
    // ---- the Schur complement leaves: every tile of this wave with both blocks in the border, every panel applied. Tile (nsteps, nsteps) is wave 0's.
    const int lq = hw_lane_id();
    const int fr = lq & 15, fk = lq >> 4;
    double* const sc = Mg + (size_t)(bshift + fk) * ld + bshift + fr;
#pragma unroll
    for (int s = 0; s < NSLOT; ++s) {
      const int i = tik[s] & 255, k = tik[s] >> 8;
      if (k != 99 && k >= nsteps && !(i == k && k == nsteps)) {
        double* dstp = sc + (size_t)(PB * i) * ld + PB * k;
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) dstp[(size_t)(4 * rg) * ld] = acc[s][rg];
      }
    }
  }
  PPROBE_FLUSH();
}

__global__ __launch_bounds__(64 * NW) void k_potrf_panel(double* __restrict__ M, size_t ld, int k0, int nb, double* __restrict__ Dinv_out, int* flag,
                                                         const double* __restrict__ rhs, double* __restrict__ yout, size_t bsM, size_t bsL, size_t bsR,
                                                         const long long* __restrict__ btab, const int* __restrict__ own, const int* __restrict__ list) {
  potrf_panel_body<16>(M, ld, k0, nb, Dinv_out, flag, rhs, yout, bsM, bsL, bsR, btab, own, list);
}
// (three workgroups per CU: 42 KB of LDS each; at most 168 registers per wave)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) void k_potrf_panel4(double* __restrict__ M, size_t ld, int k0, int nb, double* __restrict__ Dinv_out, int* flag,
                                                         const double* __restrict__ rhs, double* __restrict__ yout, size_t bsM, size_t bsL, size_t bsR,
                                                         const long long* __restrict__ btab, const int* __restrict__ own, const int* __restrict__ list) {
  potrf_panel_body<4>(M, ld, k0, nb, Dinv_out, flag, rhs, yout, bsM, bsL, bsR, btab, own, list);
}
// the one-launch leaf form: workgroup = front of the batch, whole (own: up to eight blocks | stdim: the border's order | nI: where the border starts)
__global__ __launch_bounds__(64 * NW) void k_potrf_leaf(double* __restrict__ M, double* __restrict__ Dinv_out, int* flag, double* __restrict__ rhs,
                                                        double* __restrict__ yout, size_t bsL, size_t bsR, const long long* __restrict__ btab,
                                                        const int* __restrict__ own, const int* __restrict__ stdim, int nI) {
  potrf_panel_body<16, true>(M, 0, 0, PROWS / 2 / PB, Dinv_out, flag, rhs, yout, 0, bsL, bsR, btab, own, nullptr, stdim, nI);
}

struct TrsmSubArgs {
  double* M; size_t ld;
  int k0;                 // first column of the panel
  int r0;                 // first row (multiple of 16); workgroup x handles rows r0 + 16 x ..
  const double* Dinv;     // block inverses of the panel's first tile (second tile 128*128 further)
  double* rhs; const double* yvec;   // forward substitution riding along: rhs[rows] -= X[rows, :] y[k0 ..)
  size_t bsM, bsL, bsR;
  const int* live; int tI;           // see GemmArgs (k_chol.hip)
  int chain;                         // 1: launched on the serial chain — its waves raise their issue priority over the bulk update's
  const long long* btab;             // see GemmArgs (k_chol.hip)
  const int* own;                    // [batch] real interior order of every front (nullptr: the launch-wide NB applies to all)
};

// X = A L^-T on a 16-row slab, L = the (16 NB)-order factor at (k0, k0), with FOUR waves per slab, one per SIMD: a single wave (round 4's form,
// retired) is bound by ITS matrix pipe (544 v_mfma_f64_16x16x4 of 64 cycles, dependent or not: 14.5 us before any load latency), and on the serial
// chain sixteen slabs are all there is to run. Wave w owns the blocks i = w, w + 4, ... of Z. Nobody waits at a barrier: block j of Z goes through LDS (all sixteen kept) behind a counter the
// other waves poll, and the wave that owns block j + 1 applies L(j+1, j) to it FIRST, publishes Z_{j+1} = Dinv_{j+1} acc_{j+1} and only
// then catches up on its other blocks — the chain is (read Z_j, 4 MFMAs, 4 MFMAs, write Z_{j+1}) per step, everything else fills in behind.
// The L tiles of a wave stream through a ring of registers in a FIXED order (step-major; its slot of the next owner's block row is fetched
// and dropped when it lies on or above the diagonal: ring positions stay compile-time constants).
#ifdef COVGPU_PROBE
__device__ long long g_tprobe[4][24];
#define TPROBE(k) do { if (lane == 0 && blockIdx.x == 0 && blockIdx.y == 0) g_tprobe[wave][k] = clock64() - tstart; } while (0)
#else
#define TPROBE(k) do {} while (0)
#endif
template <int NB>
COV_DEV void trsm_sub4_body(const TrsmSubArgs& g, v4f64 (*zall)[64], int* zcount, double (*spart)[16]) {
  constexpr int MB = NB / 4;
  const int batch = blockIdx.y, lane = threadIdx.x & 63, n = lane & 15, fk = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int row0 = g.r0 + PB * (int)blockIdx.x;
#ifdef COVGPU_PROBE
  const long long tstart = clock64();
#endif
  if (g.chain) __builtin_amdgcn_s_setprio(3);
  double* Mb = g.M + (g.btab != nullptr ? (size_t)g.btab[2 * batch] : (size_t)batch * g.bsM);
  const size_t ld = g.btab != nullptr ? (size_t)g.btab[2 * batch + 1] : g.ld;
  const double* Db = g.Dinv + (size_t)batch * g.bsL;
  const int pr = 4 * (n & 3) + (n >> 2);  // logical row carried by A-operand lane n
  double* Arow = Mb + (size_t)(row0 + n) * ld + g.k0 + 4 * fk;
  const double* Lrow = Mb + (size_t)(g.k0 + pr) * ld + g.k0 + 4 * fk;
  const double* Drow = Db + pr * PB + 4 * fk;
  auto Ltile = [&](int i, int j) { return *reinterpret_cast<const v4f64*>(Lrow + (size_t)(PB * i) * ld + PB * j); };
  auto Dblk = [&](int j) { return *reinterpret_cast<const v4f64*>(Drow + (size_t)(j >> 3) * kTile * kTile + (j & 7) * 256); };
  v4f64 acc[MB];
#pragma unroll
  for (int m = 0; m < MB; ++m) acc[m] = *reinterpret_cast<const v4f64*>(Arow + PB * (4 * m + wave));
  v4f64 dmine[MB];   // the block inverses of this wave's blocks
#pragma unroll
  for (int m = 0; m < MB; ++m) dmine[m] = Dblk(4 * m + wave);
  constexpr int RING = 8;
  v4f64 ring[RING];
  // fetch cursor over the fixed sequence: for j = 0 .. NB-2, for m = (j + 1) / 4 .. MB-1 -> tile (4 m + wave, j)
  int pj = 0, pm = 0, pt = 0;
  auto fetch = [&]() {
    if (pj < NB - 1) {
      ring[pt % RING] = Ltile(4 * pm + wave, pj); ++pt;
      if (++pm >= MB) { ++pj; pm = (pj + 1) >> 2; }
    }
  };
#pragma unroll
  for (int k = 0; k < RING - 1; ++k) fetch();
  auto publish = [&](int j, int m) {   // Z_j = Dinv_j acc_j: final block of X, and -Z_j for everybody
    v4f64 Z = v4f64{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < 4; ++s) Z = __builtin_amdgcn_mfma_f64_16x16x4f64(dmine[m][s], acc[m][s], Z, 0, 0, 0);
    acc[m] = Z;
    zall[j][lane] = -Z;
    if (lane == 0) __hip_atomic_store(zcount, j + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);   // (LDS operations of a wave execute in order)
  };
  if (wave == 0) publish(0, 0);
  int t = 0;
#pragma unroll
  for (int j = 0; j + 1 < NB; ++j) {
    const int o1 = (j + 1) & 3, m1 = (j + 1) >> 2;
    if (wave != (j & 3)) {   // (the publisher itself need not look)
      int spins = 0;
      while (__hip_atomic_load(zcount, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < j + 1 && ++spins < (1 << 22)) __builtin_amdgcn_s_sleep(1);
    }
    const v4f64 Zn = zall[j][lane];
    if (NB == 16) TPROBE(j);
#pragma unroll
    for (int m = m1; m < MB; ++m) {
      fetch();
      if (m > m1 || wave >= o1) {
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[m] = __builtin_amdgcn_mfma_f64_16x16x4f64(ring[t % RING][s], Zn[s], acc[m], 0, 0, 0);
      }
      ++t;
      if (m == m1 && wave == o1) publish(j + 1, m1);
    }
  }
  if (NB == 16) TPROBE(16);
#pragma unroll
  for (int m = 0; m < MB; ++m) *reinterpret_cast<v4f64*>(Arow + PB * (4 * m + wave)) = acc[m];
  if (g.rhs != nullptr) {  // rhs[row0 + n] -= sum_k X[n][k] y[k]: lane partial, fixed butterfly over the four lanes sharing n, waves in order
    const double* yv = g.yvec + (size_t)batch * g.bsR + g.k0 + 4 * fk;
    double part = 0.0;
#pragma unroll
    for (int m = 0; m < MB; ++m) {
      const v4f64 y4 = *reinterpret_cast<const v4f64*>(yv + PB * (4 * m + wave));
#pragma unroll
      for (int s = 0; s < 4; ++s) part += acc[m][s] * y4[s];
    }
    part += __shfl_xor(part, 16, 64);
    part += __shfl_xor(part, 32, 64);
    if (fk == 0) spart[wave][n] = part;
    lds_barrier();
    if (wave == 0 && fk == 0) g.rhs[(size_t)batch * g.bsR + row0 + n] -= ((spart[0][n] + spart[1][n]) + spart[2][n]) + spart[3][n];
  }
}

template <int NB>
__global__ __launch_bounds__(256) void k_trsm_sub4(TrsmSubArgs g) {
  __shared__ v4f64 zall[16][64];
  __shared__ double spart[4][16];
  __shared__ int zcount;
  if (g.live != nullptr) {
    const int batch = blockIdx.y, row0 = g.r0 + PB * (int)blockIdx.x;
    const int nI = g.live[2 * batch], nO = g.live[2 * batch + 1];
    const int tp = g.k0 / kTile, tr = row0 / kTile;
    if (!(tp < nI || (tp >= g.tI && tp - g.tI < nO))) return;
    if (!(tr < nI || (tr >= g.tI && tr - g.tI < nO))) return;
  }
  int nbf = NB;
  if (g.own != nullptr) {
    const int real = g.own[blockIdx.y] - g.k0;
    if (real <= 0) return;
    nbf = (real + PB - 1) / PB;
  }
  if (threadIdx.x == 0) zcount = 0;
  __syncthreads();
  if (NB > 4 && nbf <= 4) { trsm_sub4_body<4>(g, zall, &zcount, spart); return; }
  if (NB > 8 && nbf <= 8) { trsm_sub4_body<8>(g, zall, &zcount, spart); return; }
  if (NB > 12 && nbf <= 12) { trsm_sub4_body<12>(g, zall, &zcount, spart); return; }
  trsm_sub4_body<NB>(g, zall, &zcount, spart);
}

// (Measured and dropped, round 4 — both bit-identical to this kernel: (i) four slabs per workgroup with the factor streamed through LDS
//  by block columns, two block columns ahead: 36 us instead of 25 on the chain, a two-step prefetch distance does not cover a memory
//  latency and every step then pays one; (ii) this kernel with a ring of TWENTY tiles and one wave per SIMD: no change at all — the slab
//  is bound by its 544 dependent-issue MFMAs on one SIMD (16 Z chains of four dependent instructions each), not by the tile loads.)
// (Measured and dropped, round 4: a panel PIPELINE for multi-panel fronts — the factorisation publishing its block columns through
//  device-scope flags, a second launch on another stream following it in lock step with the substitution of the next panel's rows and
//  the update of the next diagonal block. Correct, but a root panel took ~250 us instead of 159: a device-scope load / store
//  acknowledgement costs ~4 us here, as long as a whole factorisation step. profiles/r04_ab_experiments.txt; the code is in the history
//  of this file, commit 5ecf8c0.)

// ---- launch wrappers (k_chol.hip schedules them) ----------------------------------------------------------------------
void launch_potrf_panel(double* S, size_t ld, int t0, int w, double* Linv, int* flag, double* b, int npad, int nbt, size_t sM, size_t sL, size_t sR,
                        hipStream_t st, const long long* btab, int nb, const int* own, const int* list, int n_big, int n_small) {
  if (nb < 0) nb = 8 * w;
  if (nb == 0) { form_hit(KF_POTRF_SKIPPED); return; }  // an all-padding panel of every front of the batch: L = I, Dinv = I, y = 0 are in place
  static std::atomic<unsigned long long> seen{0};
  if (first_use_on_device(seen)) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_potrf_panel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPanelLds);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_potrf_panel4), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPanelLds4);
  }
  double* Lp = Linv + (size_t)t0 * kTile * kTile;
  const double* yb = b ? b + npad : nullptr;
  if (list == nullptr) {   // every front of the batch in the sixteen-wave form (arrow blocks of the pose graph, the dense solve)
    form_hit(KF_POTRF_PANEL); form_hit(KF_POTRF_PANEL_FRONTS, nbt);
    hipLaunchKernelGGL(k_potrf_panel, dim3(nbt), dim3(64 * NW), kPanelLds, st, S, ld, t0 * kTile, nb, Lp, flag, (const double*)b, (double*)yb, sM, sL, sR, btab, own, list);
    return;
  }
  // list[0 .. n_big): fronts with more than 128 real columns in this panel | list[n_big .. n_big + n_small): the others that have any (four waves)
  // The four-wave form runs three fronts per CU on the same three matrix pipes: per front it is slower (one tile wave per SIMD instead of four), so it
  // only pays when the small fronts outnumber the CUs — 5-agent map, 182 speed-bias segments: 245 it/s with it against 250 without.
  constexpr int kSmallMin = 384;
  if (n_small <= kSmallMin) { n_big += n_small; n_small = 0; }
  if (n_big > 0) { form_hit(KF_POTRF_PANEL); form_hit(KF_POTRF_PANEL_FRONTS, n_big); }
  if (n_small > 0) { form_hit(KF_POTRF_PANEL4); form_hit(KF_POTRF_PANEL4_FRONTS, n_small); }
  if (n_big > 0) hipLaunchKernelGGL(k_potrf_panel, dim3(n_big), dim3(64 * NW), kPanelLds, st, S, ld, t0 * kTile, nb, Lp, flag, (const double*)b, (double*)yb, sM, sL, sR, btab, own, list);
  if (n_small > 0)
    hipLaunchKernelGGL(k_potrf_panel4, dim3(n_small), dim3(256), kPanelLds4, st, S, ld, t0 * kTile, std::min(nb, 8), Lp, flag, (const double*)b, (double*)yb, sM, sL, sR, btab, own,
                       list + n_big);
}

// a level of leaf fronts (leaf_front.hpp: leaf_level_eligible) factored whole in one launch: L, the block inverses, y, the border rows' right-hand
// side and the Schur complements are all in place behind it. Counted as k_potrf_panel's: it is that kernel's sixteen-wave form
void launch_potrf_leaf(double* S, double* Linv, int* flag, double* b, int npad, int nbt, size_t sL, size_t sR, hipStream_t st, const long long* btab,
                       const int* own, const int* stdim, int nI) {
  static std::atomic<unsigned long long> seen{0};
  if (first_use_on_device(seen)) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_potrf_leaf), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPanelLds);
  form_hit(KF_POTRF_PANEL); form_hit(KF_POTRF_PANEL_FRONTS, nbt); form_hit(KF_POTRF_LEAF, nbt);
  hipLaunchKernelGGL(k_potrf_leaf, dim3(nbt), dim3(64 * NW), kPanelLds, st, S, Linv, flag, b, b + npad, sL, sR, btab, own, stdim, nI);
}

void launch_trsm_sub(double* S, size_t ld, int t0, int w, int r0, int r1, const double* Linv, double* b, int npad, int nbt, size_t sM, size_t sL,
                     size_t sR, const int* live, int tI, hipStream_t st, bool chain, const long long* btab, int nb, const int* own) {
  if (r1 <= r0 || nb == 0) return;
  TrsmSubArgs g{S, ld, t0 * kTile, r0 * kTile, Linv + (size_t)t0 * kTile * kTile, b, b ? b + npad : nullptr, sM, sL, sR, live, tI, chain ? 1 : 0, btab, own};
  const dim3 grid((r1 - r0) * (kTile / PB), nbt);
  // nb: 16-column blocks of the panel that hold real columns (the rest is identity padding with zeros below: X = A there)
  const int need = nb > 0 ? std::min(nb, 8 * w) : 8 * w;
  form_hit(need <= 4 ? KF_TRSM_SUB4_4 : need <= 8 ? KF_TRSM_SUB4_8 : need <= 12 ? KF_TRSM_SUB4_12 : KF_TRSM_SUB4_16);
  if (need <= 4) hipLaunchKernelGGL(k_trsm_sub4<4>, grid, dim3(256), 0, st, g);
  else if (need <= 8) hipLaunchKernelGGL(k_trsm_sub4<8>, grid, dim3(256), 0, st, g);
  else if (need <= 12) hipLaunchKernelGGL(k_trsm_sub4<12>, grid, dim3(256), 0, st, g);
  else hipLaunchKernelGGL(k_trsm_sub4<16>, grid, dim3(256), 0, st, g);
}

}  // namespace covgpu
