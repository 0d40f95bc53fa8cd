// k_front.hip — multifrontal FP64 Cholesky of the whole reduced camera system: the linear solve of
// ceres::Solve(SPARSE_SCHUR) (optimization_be.cpp:560-567) in the elimination order of nd_plan.hpp.
//
// The reduced camera system (poses 6 + speed-bias 9 per keyframe, A.6) is sparse: covisibility reaches +-20 keyframes along
// an agent's trajectory, loop closures and fused landmarks add local patches, IMU factors couple chain neighbours. Every node
// of the nested-dissection tree owns a dense FRONT [own unknowns | coupled ancestor unknowns]; the linearisation kernels write
// the system straight into the fronts (nd_entry, common.hpp — no global matrix exists). Per tree level, bottom-up:
//   extend-add   a parent's front += the Schur complements its children left in their trailing blocks (one gather launch:
//                every entry sums its children in child order — deterministic, no atomics)
//   partial factorisation of ALL fronts of the level in one batch on the FP64 matrix cores (k_chol.hip / k_panel.hip; fronts
//                of unequal order share the launches through a per-front (offset, leading dimension) table; the forward
//                substitution rides along)
// then top-down one backward substitution per level with the ancestors' unknowns given. Same arithmetic as a dense Cholesky
// of the 15K-order system up to the elimination order. Replaces round 2's IMU-chain elimination + per-agent dense blocks:
// 5-agent map 1.2e11 -> 2.7e10 flops, single-agent maps no longer factor a dense 6K system.
// This file: the kernels and their launchers; launch_nd_solve is the sequence of the steps of struct FrontRun. The host tables the kernels and
// the launchers read (NdDev, NdLevel) are built by nd_tables.hip.
#include <algorithm>

#include "common.hpp"
#include "dev_math.hpp"

namespace covgpu {

// ------------------------------------------------------------------------------------------------ device kernels
struct NdLevArgs {
  int first, n, nI, ntot;
  double* rhs;  // the level's right-hand sides: [n][2 ntot]
  const int *own_dims, *st_dims, *own_g, *st_g, *gidx, *inv_off, *inv;
};

// clear the tiles the factorisation will touch and put the identity on the interior padding rows. One workgroup per 128x128
// tile; dead tiles exit at once. Touched: the lower triangle over [interior tiles up to the last big panel that holds a real
// column | real border tiles] (a half-padded 256-column panel is read whole by the panel kernels), and the 2x2 diagonal
// tiles of the all-padding panels (k_potrf_panel factors every panel of every front of the batch).
// (ONE launch over the tiles of all levels — a level per launch was seven dependent host enqueues at the head of every linearisation,
//  with the chip idle behind them: blocks [blk0[l], blk0[l + 1]) belong to level l, tile (tr, tc) of its front number `fz`)
struct NdZeroArgs { int nlev; int first[24], n[24], nI[24], T[24]; long long blk0[25]; const int *own_dims, *st_dims, *bb_off, *bb; int first_top; };
__global__ __launch_bounds__(256) void k_nd_zero(DevProblem P, NdZeroArgs z) {
  int l = 0;
  while (l + 1 < z.nlev && (long long)blockIdx.x >= z.blk0[l + 1]) ++l;
  const int T = z.T[l];
  const int q = (int)((long long)blockIdx.x - z.blk0[l]);
  const int fz = q / (T * T), rem = q - fz * T * T, tr = rem / T, tc = rem - tr * T;
  if (tc > tr) return;
  const int node = z.first[l] + fz;
  // (a front of at most 128 unknowns: nothing reads its second tile column below the panel's own 2x2 tiles — the panel factorisation, the
  //  substitutions and the rank updates all stop at the front's own last real 16-column block)
  const int own_n = z.own_dims[node];
  const int nIt = z.nI[l] / kTile, lo2 = own_n <= kTile ? 1 : 2 * ((own_n + 2 * kTile - 1) / (2 * kTile)), lb = (z.st_dims[node] + kTile - 1) / kTile;
  auto live = [&](int t) { return t < lo2 || (t >= nIt && t - nIt < lb); };
  const bool pad_diag = tr >= lo2 && tr < nIt && tc >= (tr & ~1);
  if (!((live(tr) && live(tc)) || pad_diag)) return;
  // a border x border tile no child adds into: the first panel's trailing update starts it from zero itself (GemmArgs::beta0); one that a child
  // does add into is written whole by the extend-add (round 6: store_border) — except in the replicated top fronts of a sharded solve, which are
  // summed over the ranks as they stand
  if (z.bb != nullptr && tc >= nIt && (node < z.first_top || !z.bb[z.bb_off[node] + (tr - nIt) * (tr - nIt + 1) / 2 + (tc - nIt)])) return;
  const size_t ld = (size_t)P.nd_ntab[2 * node + 1];
  double* M = P.nd_M + P.nd_ntab[2 * node] + (size_t)tr * kTile * ld + (size_t)tc * kTile;
  const int own = z.own_dims[node];
  for (int e = threadIdx.x; e < kTile * kTile / 2; e += 256) {
    const int r = e / (kTile / 2), c2 = 2 * (e - r * (kTile / 2));
    double2 v = {0.0, 0.0};
    if (tr == tc && tr < nIt) {  // interior diagonal tile: identity on the padding rows
      const int gr = tr * kTile + r;
      if (gr >= own) { if (c2 == r) v.x = 1.0; if (c2 + 1 == r) v.y = 1.0; }
    }
    *reinterpret_cast<double2*>(M + (size_t)r * ld + c2) = v;
  }
}

// speed-bias part of the system (block-tridiagonal rows Ad / Ae and their couplings Bp / Bs / Bn to the poses, filled by the
// inertial kernels and damped by k_finalize_diag) and the right-hand side -> fronts. One thread per entry.
// part: 0 everything | 1 what is final as soon as the speed-bias part of the system is — every matrix entry (Ad .. Bn are the inertial kernels' alone)
// and the right-hand side of the bottom level's fronts (nodes < nleaf in level order: speed-bias rows only) —, written early, beside the landmark pass,
// where that level is factored there (launch_nd_leaves) | 2 the rest: the "empty" words and the other fronts' right-hand sides. Every entry belongs to
// one part.
__global__ __launch_bounds__(256) void k_nd_assemble(DevProblem P, const int* __restrict__ rhs_off, double* __restrict__ x, const int* __restrict__ fill, int nfill,
                                                      unsigned long long empty, int part, int nleaf) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  // (the solution vector's entries of the levels whose backward substitution is ONE launch start a solve "empty": k_bwd.hip, k_bwd_tree)
  if (t < nfill) reinterpret_cast<unsigned long long*>(x)[fill[t]] = empty;
  if (P.vi && part != 2) {
    const int pos = t / 324, e = t - 324 * pos;
    if (pos < P.K) {
      const int vs = 2 * pos + 1;
      const bool head = pos == P.pos_chain_begin[pos], tail = pos + 1 == P.pos_chain_end[pos];
      if (e < 81) {
        const int r = e / 9, c = e - 9 * r;
        if (c <= r) *nd_entry(P, vs, vs, r, c) = P.Ad[(size_t)81 * pos + e];
      } else if (e < 162) {
        const int q = e - 81, r = q / 9, c = q - 9 * r;
        if (!head) *nd_entry(P, vs, vs - 2, r, c) = P.Ae[(size_t)81 * pos + q];
      } else {
        const int q = e - 162, w = q / 54, k = q - 54 * w, r = k / 6, c = k - 6 * r;
        if (w == 0) *nd_entry(P, vs, 2 * pos, r, c) = P.Bs[(size_t)54 * pos + k];
        else if (w == 1) { if (!head) *nd_entry(P, vs, 2 * (pos - 1), r, c) = P.Bp[(size_t)54 * pos + k]; }
        else if (!tail) *nd_entry(P, vs, 2 * (pos + 1), r, c) = P.Bn[(size_t)54 * pos + k];
      }
    }
  }
  if (t < P.n) {  // right-hand side: own rows of every front (the border rows start at zero and collect the children's parts)
    const int kf = t / P.D, r = t - kf * P.D, pos = P.perm[kf];
    const int v = r < 6 ? 2 * pos : 2 * pos + 1, rr = r < 6 ? r : r - 6;
    const int node = P.nd_vnode[v];
    if (node >= 0 && (part == 0 || (node < nleaf) == (part == 1))) P.nd_rhs[rhs_off[node] + P.nd_voff[v] + rr] = P.bred[t];  // (node < 0: an unknown of another rank's subtree)
  }
}

// parent front += children's Schur complements, parent right-hand side += children's reduced right-hand sides, in child order.
// One workgroup per 64x64 tile of a host-built list (only tiles some child contributes to); a thread owns a 4x4 sub-grid.
// Round 5: tile and child descriptors flattened on the host (NdDev::extw / extc): tile -> child entry -> row map -> value, with the child entry two
// and the row maps one child ahead of the gather — the kernel is a chain of dependent loads on the critical path of every level transition.
__global__ __launch_bounds__(256) void k_nd_extend(DevProblem P, NdLevArgs a, const int* __restrict__ work, const int* __restrict__ child, int second_pass, int store_border, DevSignal sig) {
  // ("the chain's stream has finished the level below": published by this launch's first thread instead of a launch of its own — CholAux::publish_handle)
  if (sig.flag != nullptr && blockIdx.x == 0 && threadIdx.x == 0) __hip_atomic_store(sig.flag, sig.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const int4 w0 = reinterpret_cast<const int4*>(work)[2 * (size_t)blockIdx.x], w1 = reinterpret_cast<const int4*>(work)[2 * (size_t)blockIdx.x + 1];
  const size_t foff = (size_t)(unsigned)w0.x | ((size_t)(unsigned)w0.y << 32);
  const size_t ld = (size_t)w0.z;
  const int rhs_p = w0.w, tr = w1.x, tc = w1.y, kbeg = w1.z, kend = w1.w;
  const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
  double* F = P.nd_M + foff;
  const int nrow = (int)ld;
  int rr[4], cc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) { rr[i] = 64 * tr + ty + 16 * i; cc[i] = 64 * tc + tx + 16 * i; }
  struct Ch { size_t moff; int ldc, rhs, inv; };
  auto load_ch = [&](int k) {
    const int2* q = reinterpret_cast<const int2*>(child) + 3 * (size_t)k;
    const int2 a0 = q[0], a1 = q[1], a2 = q[2];
    Ch c; c.moff = (size_t)(unsigned)a0.x | ((size_t)(unsigned)a0.y << 32); c.ldc = a1.x; c.rhs = a1.y; c.inv = a2.x;
    return c;
  };
  Ch c1 = {0, 0, 0, 0}, c2 = {0, 0, 0, 0};   // entries of child k + 1 | k + 2
  if (kbeg < kend) c1 = load_ch(kbeg);
  if (kbeg + 1 < kend) c2 = load_ch(kbeg + 1);
  // what the front holds already: only columns of the front's OWN unknowns carry original entries (a border x border entry
  // belongs to an ancestor's front) — those are read up front, beside the index loads, the rest starts from zero
  double v[4][4], rv[4] = {0.0, 0.0, 0.0, 0.0};
  bool hit[4][4];
  // (second_pass: the top fronts of a sharded solve take their top children after the all-reduce — everything is read then)
  const bool own_cols = second_pass != 0 || 64 * tc < a.nI;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[i][j] = (own_cols && rr[i] < nrow && cc[j] <= rr[i]) ? F[(size_t)rr[i] * ld + cc[j]] : 0.0;
      hit[i][j] = false;
    }
  // children in child order (deterministic sums); the row maps of child k + 1 are fetched before the entries of child k are gathered
  int irn[4], icn[4];
  auto load_maps = [&](const Ch& c) {
    const int* inv = a.inv + c.inv;
#pragma unroll
    for (int i = 0; i < 4; ++i) { irn[i] = rr[i] < nrow ? inv[rr[i]] : -1; icn[i] = cc[i] < nrow ? inv[cc[i]] : -1; }
  };
  if (kbeg < kend) load_maps(c1);
  for (int k = kbeg; k < kend; ++k) {
    const Ch c = c1;
    c1 = c2;
    if (k + 2 < kend) c2 = load_ch(k + 2);
    const double* C = P.nd_M + c.moff;
    const size_t ldc = (size_t)c.ldc;
    int ir[4], ic[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { ir[i] = irn[i]; ic[i] = icn[i]; }
    if (k + 1 < kend) load_maps(c1);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (ir[i] < 0) continue;
      if (tr == tc && tx == 0) rv[i] += P.nd_rhs[c.rhs + ir[i]];  // (diagonal tiles: lane tx == 0 of a row folds the right-hand side)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (ic[j] < 0 || cc[j] > rr[i]) continue;
        v[i][j] += C[(size_t)(ir[i] > ic[j] ? ir[i] : ic[j]) * ldc + (ir[i] > ic[j] ? ic[j] : ir[i])];
        hit[i][j] = true;
      }
    }
  }
  // border x border tiles (no original entries, never cleared: k_nd_zero): EVERY entry of the lower part is stored — what no child reaches is zero
  const bool store_all = !own_cols && store_border != 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) if (hit[i][j] || (store_all && rr[i] < nrow && cc[j] <= rr[i])) F[(size_t)rr[i] * ld + cc[j]] = v[i][j];
    if (rv[i] != 0.0) P.nd_rhs[rhs_p + rr[i]] += rv[i];
  }
}

// The same extend-add reading RECORDS (nd_tables: NdDev::extr): the level transitions sit on the serial chain with a dozen workgroups each, and a
// workgroup of k_nd_extend is a chain of six dependent loads under a chip full of trailing updates (tile -> child entries -> row maps -> values, a
// child at a time, then the right-hand side's read-modify-write) — 35-50 us for ten tiles. Here: record (header, first child and its maps: one
// address, known from the tile index) -> values (and the overflow records of further children) -> store. Bit-identical to k_nd_extend.
__global__ __launch_bounds__(256) void k_nd_extend_rec(DevProblem P, NdLevArgs a, const int* __restrict__ recs, const int* __restrict__ over, int second_pass, int store_border, DevSignal sig) {
  if (sig.flag != nullptr && blockIdx.x == 0 && threadIdx.x == 0) __hip_atomic_store(sig.flag, sig.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const int* rec = recs + (size_t)kExtRec * blockIdx.x;
  const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
  const int4 w0 = reinterpret_cast<const int4*>(rec)[0], w1 = reinterpret_cast<const int4*>(rec)[1];
  int4 chn = reinterpret_cast<const int4*>(rec)[2];
  int irn[4], icn[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) { irn[i] = rec[16 + ty + 16 * i]; icn[i] = rec[80 + tx + 16 * i]; }
  const size_t foff = (size_t)(unsigned)w0.x | ((size_t)(unsigned)w0.y << 32);
  const size_t ld = (size_t)w0.z;
  const int rhs_p = w0.w, tr = w1.x, tc = w1.y, nrec = w1.z, next = w1.w;
  double* F = P.nd_M + foff;
  const int nrow = (int)ld;
  int rr[4], cc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) { rr[i] = 64 * tr + ty + 16 * i; cc[i] = 64 * tc + tx + 16 * i; }
  double v[4][4], rv[4] = {0.0, 0.0, 0.0, 0.0};
  bool hit[4][4];
  const bool own_cols = second_pass != 0 || 64 * tc < a.nI;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[i][j] = (own_cols && rr[i] < nrow && cc[j] <= rr[i]) ? F[(size_t)rr[i] * ld + cc[j]] : 0.0;
      hit[i][j] = false;
    }
  for (int k = 0; k < nrec; ++k) {
    const double* C = P.nd_M + ((size_t)(unsigned)chn.x | ((size_t)(unsigned)chn.y << 32));
    const size_t ldc = (size_t)chn.z;
    const int crhs = chn.w;
    int ir[4], ic[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { ir[i] = irn[i]; ic[i] = icn[i]; }
    if (k + 1 < nrec) {   // the next child's record is in flight while this one's entries are gathered
      const int* r2 = over + (size_t)kExtRec * (next + k);
      chn = reinterpret_cast<const int4*>(r2)[2];
#pragma unroll
      for (int i = 0; i < 4; ++i) { irn[i] = r2[16 + ty + 16 * i]; icn[i] = r2[80 + tx + 16 * i]; }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (ir[i] < 0) continue;
      if (tr == tc && tx == 0) rv[i] += P.nd_rhs[crhs + ir[i]];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (ic[j] < 0 || cc[j] > rr[i]) continue;
        v[i][j] += C[(size_t)(ir[i] > ic[j] ? ir[i] : ic[j]) * ldc + (ir[i] > ic[j] ? ic[j] : ir[i])];
        hit[i][j] = true;
      }
    }
  }
  const bool store_all = !own_cols && store_border != 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) if (hit[i][j] || (store_all && rr[i] < nrow && cc[j] <= rr[i])) F[(size_t)rr[i] * ld + cc[j]] = v[i][j];
    if (rv[i] != 0.0) P.nd_rhs[rhs_p + rr[i]] += rv[i];
  }
}

// block inverses of the padding columns are the identity once and for all (the panel kernel never writes them: DenseBatch::own_max)
__global__ __launch_bounds__(256) void k_nd_linv_init(double* __restrict__ Linv, size_t n) {
  const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (q < n) { const int e = (int)(q & 255); Linv[q] = ((e >> 4) == (e & 15)) ? 1.0 : 0.0; }
}

// sharded solve: [grad | hdiag] of the top unknowns <-> the tail of the all-reduced range (dir 0: pack, 1: unpack)
__global__ __launch_bounds__(256) void k_nd_gh(DevProblem P, const int* __restrict__ top_g, int ntop, double* __restrict__ buf, int dir) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ntop) return;
  const int q = top_g[i];
  if (dir == 0) { buf[i] = P.grad[q]; buf[ntop + i] = P.hdiag[q]; }
  else { P.grad[q] = buf[i]; P.hdiag[q] = buf[ntop + i]; }
}
// sharded solve: the live lower tiles of the top fronts <-> the packed exchange buffer (dir 0: pack, 1: unpack). One workgroup per tile.
__global__ __launch_bounds__(256) void k_nd_top_pack(DevProblem P, const int* __restrict__ tiles, double* __restrict__ pack, int dir) {
  const int node = tiles[3 * blockIdx.x], tr = tiles[3 * blockIdx.x + 1], tc = tiles[3 * blockIdx.x + 2];
  const size_t ld = (size_t)P.nd_ntab[2 * node + 1];
  double* M = P.nd_M + P.nd_ntab[2 * node] + (size_t)tr * kTile * ld + (size_t)tc * kTile;
  double* B = pack + (size_t)blockIdx.x * kTile * kTile;
  for (int e = threadIdx.x; e < kTile * kTile / 2; e += 256) {
    const int r = e / (kTile / 2), c2 = 2 * (e - r * (kTile / 2));
    double2* m = reinterpret_cast<double2*>(M + (size_t)r * ld + c2);
    double2* b = reinterpret_cast<double2*>(B + (size_t)r * kTile + c2);
    if (dir == 0) *b = *m; else *m = *b;
  }
}
// sharded solve: trust-region damping of the top unknowns, applied to the all-reduced top fronts with the all-reduced
// diag(J^T J) (k_finalize_diag leaves them out: every rank holds only its part of their rows before the exchange).
// Distributed top (shard policy 1): the fronts are still sums over the ranks' copies — the lead rank adds the damping, the others
// clear the row of an unknown without any observation (the lead's 1 on the diagonal is then the sum)
__global__ __launch_bounds__(256) void k_nd_top_damp(DevProblem P, const int* __restrict__ top_var, const int* __restrict__ top_r,
                                                      const int* __restrict__ top_g, int ntop, const int* __restrict__ rhs_off, double mu, int lead) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ntop) return;
  const int v = top_var[i], r = top_r[i];
  const double h = P.hdiag[top_g[i]];
  double* d = nd_entry(P, v, v, r, r);
  if (h == 0.0) { *d = lead ? 1.0 : 0.0; P.nd_rhs[rhs_off[P.nd_vnode[v]] + P.nd_voff[v] + r] = 0.0; }
  else if (lead) { const double c = covdev::clamp_diag(h); *d += mu * c * c; }
}
// Distributed top (shard policy 1): one panel's column tiles and right-hand-side rows of a batch of top fronts <-> the contiguous reduce
// buffer, dir 0 pack | 1 unpack. Entries {front, tile row | first row, tile column | rows, 0 tile | 1 right-hand side}: the first ntile are
// 128x128 tiles (buffer [ntile][128][128], full squares at the front's own leading dimension), the rest right-hand-side segments of up to
// 256 rows (buffer [.][256] behind the tiles). One workgroup per entry, 16-byte accesses along the rows.
// The interior padding rows of a front carry an identity diagonal on EVERY rank's copy (k_nd_zero): only the lead rank's copy counts.
__global__ __launch_bounds__(256) void k_nd_panel_xfer(DevProblem P, const int4* __restrict__ ent, int ntile, double* __restrict__ buf,
                                                        const int* __restrict__ rhs_node, const int* __restrict__ own_dims, int dir, int lead) {
  const int4 e = ent[blockIdx.x];
  if ((int)blockIdx.x < ntile) {
    const size_t ld = (size_t)P.nd_ntab[2 * e.x + 1];
    double* M = P.nd_M + P.nd_ntab[2 * e.x] + (size_t)e.y * kTile * ld + (size_t)e.z * kTile;
    double* B = buf + (size_t)blockIdx.x * kTile * kTile;
    const int pad0 = (dir == 0 && !lead && e.y == e.z && e.y * kTile < P.nd_nI[e.x]) ? own_dims[e.x] - e.y * kTile : kTile;   // first padding row of the tile
    for (int q = threadIdx.x; q < kTile * kTile / 2; q += 256) {
      const int r = q / (kTile / 2), c2 = 2 * (q - r * (kTile / 2));
      double2* m = reinterpret_cast<double2*>(M + (size_t)r * ld + c2);
      double2* b = reinterpret_cast<double2*>(B + (size_t)r * kTile + c2);
      if (dir == 0) *b = r < pad0 ? *m : double2{0.0, 0.0};
      else *m = *b;
    }
  } else {
    double* R = P.nd_rhs + rhs_node[e.x] + e.y;
    double* B = buf + (size_t)ntile * kTile * kTile + (size_t)(blockIdx.x - ntile) * 256;
    const int t = threadIdx.x;
    if (t < e.z) { if (dir == 0) B[t] = R[t]; else R[t] = B[t]; }
  }
}

// ------------------------------------------------------------------------------------------------ launchers
// the switches of the driver, read once when the library loads
static const bool kLookahead = env_int("COVGPU_ND_LOOKAHEAD", 1) != 0;   // look-ahead across the levels of the tree (FrontRun::run_levels)
static const bool kFusedBwd = env_int("COVGPU_ND_BWD_FUSED", 1) != 0;    // backward substitution as one launch per level (0: one per tile)
static const bool kBwdTree = env_int("COVGPU_BWD_TREE", 1) != 0;         // ... and as one launch per group of levels (0: a launch per level)
static const bool kExtRecords = env_int("COVGPU_EXT_RECORDS", 1) != 0;   // extend-add from records (0: through the round-5 tables, k_nd_extend)
// COVGPU_BETA0 (on unless 0): the first rank update of a border x border tile no child adds into starts it from zero (GemmArgs::beta0), and the
// extend-add stores the tiles a child does add into whole — k_nd_zero clears neither. Off: k_nd_zero clears every border tile (round 5's form).
static const bool kBeta0 = env_int("COVGPU_BETA0", 1) != 0;
// COVGPU_LEAF_ONE (on unless 0): a bottom level of speed-bias leaf fronts is factored whole in one launch (k_potrf_leaf). Off: the panel route
// (k_potrf_panel, k_trsm_sub4 and the trailing update through their gates) — kept for the A/B of the two and for the test that compares them.
// 2: the one-launch form, left on the chain at the level's old place instead of beside the landmark pass (the other half of the A/B).
static int env_leaf_one() { static const int v = env_int("COVGPU_LEAF_ONE", 1); return v; }
static const bool kLeafOne = env_leaf_one() != 0;

static NdLevArgs lev_args(const DevProblem& P, const NdDev& nd, int l) {
  const NdLevel& L = nd.lev[l];
  return NdLevArgs{L.first, L.n, L.nI, L.ntot, P.nd_rhs + L.rhs_off, nd.own_dims, nd.st_dims, nd.own_g, nd.st_g, nd.gidx, nd.inv_off, nd.inv};
}

void launch_nd_init(const DevProblem& P, const NdDev& nd, hipStream_t st) {
  if (nd.linv_elems) hipLaunchKernelGGL(k_nd_linv_init, dim3((unsigned)((nd.linv_elems + 255) / 256)), dim3(256), 0, st, P.nd_Linv, nd.linv_elems);
}

void launch_nd_zero(const DevProblem& P, const NdDev& nd, hipStream_t st) {
  NdZeroArgs z;
  z.nlev = 0; z.blk0[0] = 0; z.own_dims = nd.own_dims; z.st_dims = nd.st_dims; z.bb_off = nd.bb_off; z.bb = kBeta0 ? nd.bb : nullptr;
  // nodes are numbered in level order: the first node of the first top level (sharded solve) — below it the extend-add stores the border tiles
  z.first_top = !kBeta0 ? 0 : (nd.top_lev0 < (int)nd.lev.size() ? nd.lev[nd.top_lev0].first : nd.nnodes);
  auto flush = [&] {
    if (z.nlev > 0 && z.blk0[z.nlev] > 0) hipLaunchKernelGGL(k_nd_zero, dim3((unsigned)z.blk0[z.nlev]), dim3(256), 0, st, P, z);
    z.nlev = 0; z.blk0[0] = 0;
  };
  for (size_t l = 0; l < nd.lev.size(); ++l) {
    const NdLevel& L = nd.lev[l];
    if (L.n == 0) continue;
    const int T = L.ntot / kTile;
    const long long nb = (long long)T * T * L.n;
    if (z.nlev == 24 || z.blk0[z.nlev] + nb > 0x7fffff00ll) flush();   // (more than 24 levels / 2^31 blocks: another launch)
    z.first[z.nlev] = L.first; z.n[z.nlev] = L.n; z.nI[z.nlev] = L.nI; z.T[z.nlev] = T;
    z.blk0[z.nlev + 1] = z.blk0[z.nlev] + nb;
    ++z.nlev;
  }
  flush();
}

// One linear solve as steps: what launch_nd_solve's arguments and the steps share. Every enqueue of the solve is made by one of the members; the order
// of the members in launch_nd_solve is the order on the stream.
struct FrontRun {
  const DevProblem& P; NdDev& nd; double* dst; const double mu; hipStream_t st; CholAux& ax;
  const int nlev, ltop;   // levels | first top level (== nlev: none)
  bool tree_on = false, tree_top_on = false;   // the bottom | top levels' backward substitution as one launch (set by ensure_scratch)
  FrontRun(const DevProblem& P_, NdDev& nd_, double* dst_, double mu_, hipStream_t st_, CholAux& ax_)
      : P(P_), nd(nd_), dst(dst_), mu(mu_), st(st_), ax(ax_), nlev((int)nd_.lev.size()), ltop(nd_.top_lev0) {}
  // leaves both scratches of the backward substitution large enough for this tree, and tree_on / tree_top_on. false: allocation failed, nothing enqueued
  bool ensure_scratch() {
    {  // scratch of the one-launch backward substitution (k_bwd_front): [fronts][interior tiles <= 4][256-row chunks of the border][128]
      size_t need = 0;
      for (const NdLevel& L : nd.lev)
        need = std::max(need, (size_t)L.n * std::min(kBwdFrontMaxTiles, (L.own_max + kTile - 1) / kTile) * std::max(1, (L.ntot - L.nI + 255) / 256) * kTile);
      if (need > ax.bwd_scr_elems) {
        if (ax.bwd_scr) (void)hipFree(ax.bwd_scr);
        ax.bwd_scr = nullptr; ax.bwd_scr_elems = 0;
        if (hipMalloc((void**)&ax.bwd_scr, need * sizeof(double)) != hipSuccess) { ax.bwd_scr = nullptr; return false; }   // (nothing enqueued yet)
        ax.bwd_scr_elems = need;
      }
    }
    if (!ax.pipe_broken && ax.gate_dead != nullptr && ax.gate_dead_h != nullptr) {  // scratch of the pipelined backward substitution (k_bwd_pipe): [fronts][interior tiles][chunks + 1][128], filled once
      size_t need = 0, tree = 0, tree2 = 0;   // a level of its own | the bottom | the top levels in one launch
      for (int l = 0; l < nlev; ++l) {
        const NdLevel& L = nd.lev[l];
        if (L.n > 0 && bwd_pipe_on() && L.interior_tiles() >= kBwdPipeMinTiles) need = std::max(need, L.pipe_scratch_elems());
        if (l < nd.tree_levels) tree += L.pipe_scratch_elems();
        if (l >= nd.tree_top0) tree2 += L.pipe_scratch_elems();
      }
      need = std::max(need, std::max(tree, tree2));
      if (need > ax.bwd_pipe_elems) {
        if (ax.bwd_pipe) { (void)hipDeviceSynchronize(); (void)hipFree(ax.bwd_pipe); }
        ax.bwd_pipe = nullptr; ax.bwd_pipe_elems = 0;
        if (hipMalloc((void**)&ax.bwd_pipe, need * sizeof(double)) == hipSuccess) {
          ax.bwd_pipe_elems = need;
          launch_pipe_fill(ax.bwd_pipe, need, st);   // (stream-ordered before the first use)
        } else ax.bwd_pipe = nullptr;                // (launch per tile)
      }
    }
    // the bottom levels' backward substitution as one launch (k_bwd_tree): needs the pipeline (not COVGPU_BWD_PIPE=0), its scratch and the give-up word
    const bool tree_ok = kBwdTree && kFusedBwd && nd.tree_fill != nullptr && !ax.pipe_broken && ax.bwd_pipe != nullptr && ax.gate_dead != nullptr && bwd_pipe_on();
    tree_on = tree_ok && nd.tree_levels >= 2;
    tree_top_on = tree_ok && nd.tree_top0 < nlev;
    return true;
  }
  // leaves the speed-bias part of the system and the right-hand side in the fronts, and the one-launch levels' entries of dst "empty"
  // (the right-hand sides were cleared on the head stream of the build, beside the fronts: solver.hip enqueue_build)
  // leaves_early: the speed-bias system and the bottom level's right-hand sides are in place already (launch_nd_leaves) — the rest
  void assemble(bool leaves_early) {
    ax.mark(st, -1);
    const int nfill = (tree_on || tree_top_on) ? (int)nd.h_tree_fill.size() : 0;
    const int cnt = std::max(std::max(P.vi && !leaves_early ? 324 * P.K : 0, P.n), nfill);
    hipLaunchKernelGGL(k_nd_assemble, dim3((cnt + 255) / 256), dim3(256), 0, st, P, (const int*)nd.rhs_node, dst, (const int*)nd.tree_fill, nfill, pipe_empty_word(),
                       leaves_early ? 2 : 0, leaves_early ? nd.lev[0].n : 0);
    ax.mark(st, -2);
  }
  // the early share of the assembly on stream s: the speed-bias system (all of it) and the right-hand sides of the bottom level's fronts
  void assemble_leaves(hipStream_t s) {
    const int cnt = std::max(P.vi ? 324 * P.K : 0, P.n);
    hipLaunchKernelGGL(k_nd_assemble, dim3((cnt + 255) / 256), dim3(256), 0, s, P, (const int*)nd.rhs_node, (double*)nullptr, (const int*)nullptr, 0, 0ull, 1, nd.lev[0].n);
  }
  // level l's fronts as a batch of the dense factorisation
  DenseBatch batch(int l) const {
    const NdLevel& L = nd.lev[l];
    DenseBatch bt;
    bt.n = L.n; bt.sM = 0; bt.sL = (size_t)L.nI * kTile; bt.sR = (size_t)2 * L.ntot;
    bt.live = L.live; bt.tI = L.nI / kTile; bt.live_h = L.live_h.data();
    if (kBeta0 && nd.bb != nullptr) { bt.beta0_off = nd.bb_off + L.first; bt.beta0 = nd.bb; }
    if (L.plist != nullptr) { bt.plist = L.plist; bt.pbig_h = L.pbig.data(); bt.psmall_h = L.psmall.data(); }
    bt.tab = P.nd_ntab + 2 * (size_t)L.first; bt.tri_slot = l; bt.own_max = L.own_max; bt.own_dims = nd.own_dims + L.first; bt.own_dims_h = nd.h_own_dims.data() + L.first;
    return bt;
  }
  // fronts <-> solution vector for a batch whose first front is `first`: the ancestors' unknowns are read from dst by the first launch of a
  // level's backward substitution, the fronts' own unknowns are written there by its last
  BwdXfer xfer(int first) const {
    BwdXfer xf;
    xf.gidx = nd.gidx; xf.own_g = nd.own_g; xf.st_g = nd.st_g; xf.own_dims = nd.own_dims; xf.st_dims = nd.st_dims; xf.x = dst; xf.first = first;
    return xf;
  }
  // extend-add into level l's fronts from their children of one kind, on stream s2. part: 0 all tiles | 1 the tiles of the fronts' first 256 rows |
  // 2 the others. true: something was enqueued
  bool extend(int l, bool top_children, int part, hipStream_t s2, DevSignal sig = DevSignal()) {
    const NdLevel& L = nd.lev[l];
    int first = top_children ? L.ext2_first : L.ext_first, count = top_children ? L.ext2_count : L.ext_count;
    const int countA = top_children ? L.ext2_countA : L.ext_countA;
    if (part == 1) count = countA;
    if (part == 2) { first += countA; count -= countA; }
    const bool records = kExtRecords && nd.extr != nullptr;
    const int store_border = (!top_children && l < ltop && kBeta0) ? 1 : 0;
    if (count > 0) { form_hit(records ? KF_ND_EXTEND_REC : KF_ND_EXTEND); if (part != 0) form_hit(KF_ND_EXTEND_SPLIT); }
    if (count > 0 && records)
      hipLaunchKernelGGL(k_nd_extend_rec, dim3(count), dim3(256), 0, s2, P, lev_args(P, nd, l), (const int*)(nd.extr + (size_t)kExtRec * first),
                         (const int*)(nd.extr + (size_t)kExtRec * nd.ext_over), top_children ? 1 : 0, store_border, sig);
    else if (count > 0)
      hipLaunchKernelGGL(k_nd_extend, dim3(count), dim3(256), 0, s2, P, lev_args(P, nd, l), (const int*)(nd.extw + 8 * (size_t)first),
                         (const int*)(top_children ? nd.extc2 : nd.extc), top_children ? 1 : 0, store_border, sig);
    return count > 0;
  }
  // level l is the bottom level of speed-bias leaf fronts that the one-launch form takes (NdLevel::leaf_one; COVGPU_LEAF_ONE=0: the panel route)
  bool leaf_one(int l) const { return kLeafOne && l == 0 && nd.lev[0].leaf_one && nd.lev[0].n > 0; }
  // the bottom level whole on stream s: one launch, no gate inside (k_panel.hip: k_potrf_leaf)
  void leaf_launch(hipStream_t s) {
    const NdLevel& L = nd.lev[0];
    launch_potrf_leaf(P.nd_M, P.nd_Linv + L.linv_off, P.flag, P.nd_rhs + L.rhs_off, L.ntot, L.n, (size_t)L.nI * kTile, (size_t)2 * L.ntot, s,
                      P.nd_ntab + 2 * (size_t)L.first, nd.own_dims + L.first, nd.st_dims + L.first, L.nI);
  }
  // partial factorisation of level l's fronts. split: the trailing update of this level's last panel is split for the look-ahead into the next
  // level (DenseBatch::split_ta)
  void factor(int l, bool split, hipEvent_t pre_trsm) {
    const NdLevel& L = nd.lev[l];
    ax.mark(st, -3);
    if (leaf_one(l)) leaf_launch(st);
    else if (L.n > 0) {
      DenseBatch bt = batch(l);
      bt.split_ta = split ? L.split_ta : 0; bt.pre_trsm = pre_trsm;
      dense_cholesky_solve_raw(P.nd_M, P.nd_rhs + L.rhs_off, P.nd_Linv + L.linv_off, P.flag, L.ntot, st, ax, L.nI / kTile, false, bt);
    }
    ax.mark(st, -4);
  }
  // Levels [l0, l1) one after the other, with a look-ahead across the level boundary: of level l's last trailing update only the
  // tiles its parents' first panel receives run on the chain's stream, followed by that part of the extend-add and the parents'
  // first panel; the rest of the update and of the extend-add run beside it on the bulk stream (ax.aux).
  // leaves_early: level l0 = 0 was factored beside the landmark pass (launch_nd_leaves; the chain's stream has waited for it: enqueue_build) — the
  // chain starts at level 1, whose extend-add keeps its two halves as behind a split update
  void run_levels(int l0, int l1, bool top_children, bool leaves_early = false) {
    bool prev_split = false;
    for (int l = l0; l < l1; ++l) {
      if (leaves_early && l == 0) { prev_split = kLookahead && l + 1 < l1 && nd.lev[1].n > 0 && nd.lev[0].split_ta > 0; continue; }
      hipEvent_t pre = nullptr;
      if (prev_split) {
        // (the bulk stream already follows the level below through its own update; this also covers a batch that declined the split. Round 6: the
        //  record rides with the first half of the extend-add — published by its first thread — when that launch exists)
        DevSignal sig = ax.publish_handle(ax.ev_xa, st, 5);
        const int cntA = top_children ? nd.lev[l].ext2_countA : nd.lev[l].ext_countA;
        if (sig.flag == nullptr || cntA <= 0) { if (sig.flag != nullptr) ax.record_handle(sig, st); else ax.record(ax.ev_xa, st, 5); sig = DevSignal(); }
        extend(l, top_children, 1, st, sig);
        ax.wait(ax.aux, ax.ev_xa);
        extend(l, top_children, 2, ax.aux);
        ax.record(ax.ev_xb, ax.aux, 6);
        pre = ax.ev_xb;
      } else extend(l, top_children, 0, st);
      const NdLevel& L = nd.lev[l];
      const bool split = kLookahead && l + 1 < l1 && L.n > 0 && nd.lev[l + 1].n > 0 && L.split_ta > 0;
      factor(l, split, pre);
      prev_split = split;
    }
  }
  // sharded solve, either policy: gradient and diag(J^T J) of the top unknowns summed over the ranks — packed behind the top right-hand sides, the
  // policy's all-reduce, unpacked — then the damping of the top unknowns (lead: this rank's copy takes it; the replicated top: every rank's)
  void top_gh_damp(bool lead) {
    double* gh = P.nd_rhs + nd.gh_off;
    const unsigned nb = (unsigned)((nd.ntop + 255) / 256);
    if (nd.ntop > 0) { form_hit(KF_ND_GH, 2); form_hit(KF_ND_TOP_DAMP); }
    if (nd.ntop > 0) hipLaunchKernelGGL(k_nd_gh, dim3(nb), dim3(256), 0, st, P, (const int*)nd.top_g, nd.ntop, gh, 0);
    if (!nd.dist) reduce_top_replicated();
    else if (nd.ntop > 0 && ax.reduce != nullptr) ax.reduce(ax.reduce_ctx, gh, 2 * (size_t)nd.ntop, 0, st);
    if (nd.ntop > 0) {
      hipLaunchKernelGGL(k_nd_gh, dim3(nb), dim3(256), 0, st, P, (const int*)nd.top_g, nd.ntop, gh, 1);
      hipLaunchKernelGGL(k_nd_top_damp, dim3(nb), dim3(256), 0, st, P, (const int*)nd.top_var, (const int*)nd.top_r, (const int*)nd.top_g, nd.ntop,
                         (const int*)nd.rhs_node, mu, lead ? 1 : 0);
    }
  }
  // Agent-sharded solve: the top fronts so far hold THIS rank's residuals and subtrees only. ONE all-reduce of [live lower tiles
  // of the top fronts, packed | top right-hand sides | grad, hdiag of the top unknowns] (the last two contiguous in nd_rhs): the fronts are stored
  // as full squares, of which the exchange needs half (33.6 -> 17.9 MB for the 5-agent map's root). From here on every rank runs the top of the
  // tree redundantly, with no further exchange.
  void reduce_top_replicated() {
    if (ax.reduce == nullptr) return;
    if (nd.n_top_tiles > 0) form_hit(KF_ND_TOP_PACK, 2);
    const size_t ntile = (size_t)nd.n_top_tiles * kTile * kTile, nvec = nd.rhs_top + 2 * (size_t)nd.ntop;
    if (nd.n_top_tiles > 0) hipLaunchKernelGGL(k_nd_top_pack, dim3(nd.n_top_tiles), dim3(256), 0, st, P, (const int*)nd.top_tiles, nd.top_pack, 0);
    if (nvec > 0) (void)hipMemcpyAsync(nd.top_pack + ntile, P.nd_rhs, nvec * sizeof(double), hipMemcpyDeviceToDevice, st);
    ax.reduce(ax.reduce_ctx, nd.top_pack, ntile + nvec, 0, st);
    if (nd.n_top_tiles > 0) hipLaunchKernelGGL(k_nd_top_pack, dim3(nd.n_top_tiles), dim3(256), 0, st, P, (const int*)nd.top_tiles, nd.top_pack, 1);
    if (nvec > 0) (void)hipMemcpyAsync(P.nd_rhs, nd.top_pack + ntile, nvec * sizeof(double), hipMemcpyDeviceToDevice, st);
  }
  // distributed top: panel Pp of level x.L becomes the panel — its column block and right-hand-side rows all-reduced (DistPanels::exchange)
  struct XCtx { FrontRun* run; const NdLevel* L; };
  static void exchange_panel(void* vc, int Pp) {
    const XCtx& x = *static_cast<XCtx*>(vc);
    const FrontRun& r = *x.run;
    const NdLevel& L = *x.L;
    const int nt = L.dx_nt[Pp], ne = nt + L.dx_nr[Pp];
    if (ne == 0 || r.ax.reduce == nullptr) return;
    const int4* ent = reinterpret_cast<const int4*>(r.nd.dist_ent) + L.dx_first[Pp];
    const size_t n = (size_t)nt * kTile * kTile + (size_t)L.dx_nr[Pp] * 256;
    const int lead = r.nd.dist_lead ? 1 : 0;
    form_hit(KF_ND_PANEL_XFER, 2);
    hipLaunchKernelGGL(k_nd_panel_xfer, dim3(ne), dim3(256), 0, r.st, r.P, ent, nt, r.nd.dist_buf, (const int*)r.nd.rhs_node, (const int*)r.nd.own_dims, 0, lead);
    r.ax.reduce(r.ax.reduce_ctx, r.nd.dist_buf, n, 0, r.st);
    hipLaunchKernelGGL(k_nd_panel_xfer, dim3(ne), dim3(256), 0, r.st, r.P, ent, nt, r.nd.dist_buf, (const int*)r.nd.rhs_node, (const int*)r.nd.own_dims, 1, lead);
  }
  // Distributed top (shard policy 1): the top fronts stay SUMS over the ranks' copies. Per top level the extend-add of the top
  // children (partial sums added to partial sums) and the panels one at a time — each panel's column block and right-hand-side rows all-reduced
  // when it becomes the panel (dense_cholesky_dist). Everything of the top runs on this one stream: the subtree levels above joined it, so no
  // gate on another stream waits for anything enqueued behind an all-reduce.
  void dist_levels() {
    for (int l = ltop; l < nlev; ++l) {
      extend(l, true, 0, st);
      const NdLevel& L = nd.lev[l];
      ax.mark(st, -3);
      if (L.n > 0) {
        XCtx xc{this, &L};
        DistPanels d;
        d.np = (int)L.dx_nt.size(); d.tri = L.dt_dev.data(); d.tri_cnt = L.dt_cnt.data(); d.lead = nd.dist_lead; d.exchange = exchange_panel; d.ctx = &xc;
        DenseBatch bt = batch(l);
        bt.beta0 = nullptr; bt.beta0_off = nullptr;   // (top fronts: every border tile is cleared and read)
        dense_cholesky_dist(P.nd_M, P.nd_rhs + L.rhs_off, P.nd_Linv + L.linv_off, P.flag, L.ntot, st, ax, L.nI / kTile, bt, d);
      }
      ax.mark(st, -4);
    }
  }
  // backward substitution of levels l_hi .. l_lo (downwards) in one launch
  void tree_launch(int l_hi, int l_lo, bool form64) {
    BwdTreeLevel tl[kBwdTreeMax];
    int nq = 0;
    for (int l = l_hi; l >= l_lo; --l) {
      const NdLevel& L = nd.lev[l];
      BwdTreeLevel& t = tl[nq++];
      t.nbt = L.n; t.T = L.interior_tiles(); t.nchunk = L.pipe_chunks(); t.tI = L.nI / kTile; t.first = L.first;
      t.y = P.nd_rhs + L.rhs_off + L.ntot; t.bsR = (size_t)2 * L.ntot; t.Dinv = P.nd_Linv + L.linv_off; t.bsL = (size_t)L.nI * kTile;
      t.btab = P.nd_ntab + 2 * (size_t)L.first; t.live = L.live; t.scr_off = t.xpub_off = 0;
    }
    launch_bwd_tree(P.nd_M, tl, nq, xfer(0), ax.bwd_pipe, ax.gate_dead, ax.gate_dead_h, ax.gate_timeout_s, st, form64);
    ax.mark(st, -5);
  }
  // backward substitution, top-down: the top group in one launch, the levels between the groups one by one, the bottom group in one launch
  void backward() {
    if (tree_top_on) tree_launch(nlev - 1, nd.tree_top0, true);
    for (int l = (tree_top_on ? nd.tree_top0 : nlev) - 1; l >= (tree_on ? nd.tree_levels : 0); --l) {
      const NdLevel& L = nd.lev[l];
      if (L.n == 0) continue;
      DenseBatch bt = batch(l);
      bt.xfer = xfer(L.first);
      bt.bwd_cnt = kFusedBwd ? ax.bwd_cnt : nullptr; bt.bwd_scr = ax.bwd_scr;
      if (kFusedBwd && !ax.pipe_broken && ax.bwd_pipe != nullptr) { bt.bwd_pipe = ax.bwd_pipe; bt.pipe_dead = ax.gate_dead; bt.pipe_dead_h = ax.gate_dead_h; bt.pipe_timeout_s = ax.gate_timeout_s; }
      dense_backward_solve(P.nd_M, P.nd_rhs + L.rhs_off, P.nd_Linv + L.linv_off, L.ntot, st, L.nI / kTile, L.ntot / kTile, bt);
      ax.mark(st, -5);
    }
    if (tree_on) tree_launch(nd.tree_levels - 1, 0, false);   // levels tree_levels - 1 .. 0 in one launch
    ax.mark(st, -6);
  }
};

// The bottom level of speed-bias leaf fronts, assembled and factored on stream s as soon as the speed-bias part of the system is final and the fronts
// are cleared — beside the landmark pass (solver.hip: enqueue_build), one launch each and no gate inside. false: this tree has no such level (or
// COVGPU_LEAF_ONE is 0, or 2: the one-launch form at the level's old place on the chain) and nothing was enqueued; the solve then runs level 0 itself.
bool nd_leaves_beside_pass(const NdDev& nd) { return kLeafOne && env_leaf_one() != 2 && !nd.lev.empty() && nd.lev[0].leaf_one && nd.lev[0].n > 0 && nd.top_lev0 == (int)nd.lev.size(); }
bool launch_nd_leaves(const DevProblem& P, NdDev& nd, hipStream_t s, CholAux& ax) {
  if (!nd_leaves_beside_pass(nd)) return false;
  FrontRun r(P, nd, nullptr, 0.0, s, ax);
  r.assemble_leaves(s);
  r.leaf_launch(s);
  nd.leaves_done = true;
  return true;
}

bool launch_nd_solve(const DevProblem& P, NdDev& nd, double* dst, double mu, hipStream_t st, CholAux& ax) {
  FrontRun r(P, nd, dst, mu, st, ax);
  ax.init();
  if (!r.ensure_scratch()) return false;
  const bool leaves_early = nd.leaves_done;   // (of THIS system: enqueue_build's launch_nd_leaves)
  nd.leaves_done = false;
  r.assemble(leaves_early);
  r.run_levels(0, r.ltop, false, leaves_early);   // the subtrees of this rank (single GPU: the whole tree), level by level
  if (r.ltop < r.nlev) {            // sharded solve: the top fronts take their subtree children, then the exchange of the shard policy
    for (int l = r.ltop; l < r.nlev; ++l) r.extend(l, false, 0, st);
    r.top_gh_damp(nd.dist ? nd.dist_lead : true);
    if (nd.dist) r.dist_levels(); else r.run_levels(r.ltop, r.nlev, true);
  }
  r.backward();
  return true;
}

}  // namespace covgpu
