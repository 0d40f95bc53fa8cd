// nd_tables.hip — host tables of the multifrontal solve (k_front.hip) from the elimination tree of nd_plan.hpp: level order, front and right-hand-side
// layout, ancestor rows, row maps, the extend-add lists in their three encodings, border maps, the one-launch backward groups and the distributed
// top's exchange and ownership lists. Host index arithmetic only — no kernel, no HIP call. struct FrontTables holds what the steps share; every step
// states what it leaves behind; nd_tables at the end of the file is the sequence of the steps, and NdDev is complete when it returns (upload.hip
// only copies it to the device).
#include <algorithm>

#include "common.hpp"
#include "leaf_front.hpp"
#include "nd_plan.hpp"

namespace covgpu {
namespace {

enum ChildKind { kSubtreeChild = 0, kTopChild = 1 };   // NdDev: subtree children | top children (top fronts of a sharded solve only)

// tile t of a front is live (as in k_nd_zero): one of its first n_int interior tiles, or one of the n_border tiles behind the tI padded interior tiles
bool live(int t, int n_int, int tI, int n_border) { return t < n_int || (t >= tI && t - tI < n_border); }

struct FrontTables {
  const NdHostPlan& hp; const int* pos_kf; const int D, rank; NdDev& dev;
  const bool sh;                          // agent-sharded solve
  int Hs = 0, nlev = 0, nl = 0;           // subtree levels | levels | local nodes
  std::vector<std::vector<int>> lnodes;   // per level: its local nodes (plan ids)
  std::vector<int> order, newid, ld;      // local id -> plan id | plan id -> local id (-1: foreign) | local id -> front order
  // working tables no one outside needs: children by kind (CSR over local ids) and the extend-add tiles (node, tile row, tile column) with their kind
  std::vector<int> cptr[2], cidx[2], ext, ext_kind;
  FrontTables(const NdHostPlan& hp_, const int* pos_kf_, int D_, int rank_, NdDev& dev_)
      : hp(hp_), pos_kf(pos_kf_), D(D_), rank(rank_), dev(dev_), sh(!hp_.node_rank.empty()) {}
  // rank: this context's rank in an agent-sharded solve (hp.node_rank non-empty); fronts exist for the rank's own subtrees and for the TOP nodes (replicated)
  bool is_top(int n) const { return sh && hp.node_rank[n] < 0; }
  bool is_local(int n) const { return !sh || hp.node_rank[n] < 0 || hp.node_rank[n] == rank; }
  int gidx_of(int v, int r) const { return D * pos_kf[v >> 1] + ((v & 1) ? 6 + r : r); }
  // calls hit(t) for every tile row t of front i — `count` tiles of `tile` rows from row `row0` on — in which child ch's row map has an entry
  template <class F> void reached_tiles(int i, int ch, int row0, int tile, int count, F&& hit) const {
    const int* inv = dev.h_inv.data() + dev.h_inv_off[ch];
    for (int t = 0; t < count; ++t) {
      bool any = false;
      for (int r = row0 + tile * t; r < std::min(ld[i], row0 + tile * t + tile) && !any; ++r) any = inv[r] >= 0;
      if (any) hit(t);
    }
  }
  // leaves Hs / nlev / lnodes, the local nodes renumbered in level order (order, newid) and dev.nnodes / top_lev0 / plan_flops.
  // Batches = levels: subtree nodes by height, then the top nodes by their height inside the top.
  void level_order() {
    const int nn = hp.nnodes;
    for (int n = 0; n < nn; ++n) if (!is_top(n)) Hs = std::max(Hs, hp.level[n] + 1);
    std::vector<int> lev(nn), toph(nn, 0);
    for (int n = nn - 1; n >= 0; --n) if (is_top(n)) for (int c : hp.child[n]) if (is_top(c)) toph[n] = std::max(toph[n], toph[c] + 1);
    nlev = Hs;
    for (int n = 0; n < nn; ++n) { lev[n] = is_top(n) ? Hs + toph[n] : hp.level[n]; nlev = std::max(nlev, lev[n] + 1); }
    lnodes.assign(nlev, {});
    for (int n = 0; n < nn; ++n) if (is_local(n)) lnodes[lev[n]].push_back(n);
    // local nodes renumbered in level order: a level's slice of nd_ntab is its batch table; foreign nodes have no id
    newid.assign(nn, -1);
    for (int l = 0; l < nlev; ++l) for (int n : lnodes[l]) { newid[n] = (int)order.size(); order.push_back(n); }
    nl = (int)order.size();
    dev.nnodes = nl; dev.top_lev0 = Hs; dev.plan_flops = hp.flops;
  }
  // leaves per variable its front, offset and ordinal there, and who owns it (h_vnode / h_voff / h_vord / h_vown: 0 foreign | 1 subtree | 2 top)
  void variable_maps() {
    const int K = hp.K;
    dev.h_vnode.assign(2 * (size_t)K, -1); dev.h_voff.assign(2 * (size_t)K, 0); dev.h_vord.assign(2 * (size_t)K, 0); dev.h_vown.assign(2 * (size_t)K, 0);
    for (int v = 0; v < 2 * K; ++v)
      if (hp.vnode[v] >= 0) {
        const int n = hp.vnode[v];
        dev.h_vnode[v] = newid[n]; dev.h_voff[v] = hp.voff[v]; dev.h_vord[v] = hp.vord[v];
        dev.h_vown[v] = !is_local(n) ? 0 : (is_top(n) ? 2 : 1);
      }
  }
  // leaves front i = node n of level L at element `moff`: its row of every per-node table, its solution indices, its live counts, and — a top
  // front — its exchanged tile triples and the list of its scalar unknowns
  void lay_front(NdLevel& L, int n, int i, size_t& moff) {
    const int nO = ((hp.st_dims[n] + kTile - 1) / kTile) * kTile;
    ld[i] = L.nI + nO;
    L.ntot = std::max(L.ntot, ld[i]);
    dev.h_ndepth[i] = hp.depth[n]; dev.h_nI[i] = L.nI;
    dev.h_ntab[2 * (size_t)i] = (long long)moff; dev.h_ntab[2 * (size_t)i + 1] = ld[i];
    moff += (size_t)ld[i] * ld[i];
    dev.h_own_dims[i] = hp.own_dims[n]; dev.h_st_dims[i] = hp.st_dims[n];
    dev.h_own_g[i] = (int)dev.h_gidx.size();
    for (int v : hp.own[n]) for (int r = 0; r < NdHostPlan::vdim(v); ++r) dev.h_gidx.push_back(gidx_of(v, r));
    dev.h_st_g[i] = (int)dev.h_gidx.size();
    for (int v : hp.strct[n]) for (int r = 0; r < NdHostPlan::vdim(v); ++r) dev.h_gidx.push_back(gidx_of(v, r));
    L.live_h.push_back((hp.own_dims[n] + kTile - 1) / kTile); L.live_h.push_back(nO / kTile);
    if (!is_top(n)) return;
    // live lower-triangular tiles of a replicated front: what a sharded solve exchanges (whole 256-column panels of the interior)
    const int nIt = L.nI / kTile, lo2 = 2 * ((hp.own_dims[n] + 2 * kTile - 1) / (2 * kTile)), lb = (hp.st_dims[n] + kTile - 1) / kTile;
    const int Tn = ld[i] / kTile;
    for (int tr = 0; tr < Tn; ++tr)
      for (int tc = 0; tc <= tr; ++tc)
        if (live(tr, lo2, nIt, lb) && live(tc, lo2, nIt, lb)) { dev.h_top_tiles.push_back(i); dev.h_top_tiles.push_back(tr); dev.h_top_tiles.push_back(tc); }
    for (int v : hp.own[n]) for (int r = 0; r < NdHostPlan::vdim(v); ++r) { dev.h_top_var.push_back(v); dev.h_top_r.push_back(r); dev.h_top_g.push_back(gidx_of(v, r)); }
  }
  // leaves the front lists of the panel factorisation (NdLevel::plist / pbig / psmall)
  void panel_lists(NdLevel& L) {
    L.plist_h.resize(L.n);
    for (int k = 0; k < L.n; ++k) L.plist_h[k] = k;
    std::stable_sort(L.plist_h.begin(), L.plist_h.end(), [&](int a, int b) { return dev.h_own_dims[L.first + a] > dev.h_own_dims[L.first + b]; });
    const int np = L.nI / 256;
    L.pbig.assign(np, 0); L.psmall.assign(np, 0);
    for (int k = 0; k < L.n; ++k)
      for (int P = 0; P < np; ++P) {
        const int real = dev.h_own_dims[L.first + k] - 256 * P;
        if (real > 128) ++L.pbig[P]; else if (real > 0) ++L.psmall[P];
      }
  }
  // whether the one-launch leaf form takes the bottom level `nodes` (NdLevel::leaf_one): a level below other levels of an unsharded tree (a sharded
  // solve keeps the panel route: its ranks' bottom levels differ, and its schedule is not this one's) that leaf_level_eligible accepts
  bool leaf_one_level(const std::vector<int>& nodes) const {
    if (sh || nlev < 2) return false;
    std::vector<int> od, sd, ptr{0}, var;
    for (int n : nodes) {
      od.push_back(hp.own_dims[n]); sd.push_back(hp.st_dims[n]);
      var.insert(var.end(), hp.own[n].begin(), hp.own[n].end());
      ptr.push_back((int)var.size());
    }
    return leaf_level_eligible((int)nodes.size(), od.data(), sd.data(), ptr.data(), var.data());
  }
  // leaves the level shapes (dev.lev: n, first, nI, ntot, own_max, linv_off, live counts, panel lists), the fronts laid out one behind the other
  // (ld, h_ntab, the per-node tables of lay_front) and the totals M_sub / M_elems / linv_elems / ntop / n_top_tiles
  void front_layout() {
    dev.h_ndepth.resize(nl); dev.h_nI.resize(nl); dev.h_ntab.resize(2 * (size_t)nl);
    dev.h_own_dims.resize(nl); dev.h_st_dims.resize(nl); dev.h_own_g.resize(nl); dev.h_st_g.resize(nl);
    dev.lev.resize(nlev);
    ld.resize(nl);
    size_t moff = 0, loff = 0;
    for (int l = 0, i = 0; l < nlev; ++l) {
      NdLevel& L = dev.lev[l];
      L.n = (int)lnodes[l].size(); L.first = i; L.own_max = 0;
      for (int n : lnodes[l]) L.own_max = std::max(L.own_max, hp.own_dims[n]);
      L.nI = std::max(256, ((L.own_max + 255) / 256) * 256);
      L.ntot = L.nI;
      if (l == Hs) dev.M_sub = moff;
      for (int n : lnodes[l]) lay_front(L, n, i++, moff);
      L.linv_off = loff; loff += (size_t)L.n * L.nI * kTile;
      panel_lists(L);
      if (l == 0) L.leaf_one = leaf_one_level(lnodes[l]);
    }
    if (Hs >= nlev) dev.M_sub = moff;
    dev.M_elems = moff; dev.linv_elems = loff;
    dev.ntop = (int)dev.h_top_g.size(); dev.n_top_tiles = (int)(dev.h_top_tiles.size() / 3);
  }
  // leaves the right-hand sides laid out: [top levels | grad, hdiag of the top unknowns | subtree levels] — with the top fronts right in front of
  // them (upload.hip puts both in ONE allocation) the whole all-reduced region is contiguous
  void rhs_layout() {
    dev.h_rhs_node.assign(nl, 0);
    size_t roff = 0;
    auto place = [&](int l) {
      NdLevel& L = dev.lev[l];
      L.rhs_off = roff;
      for (int k = 0; k < L.n; ++k) dev.h_rhs_node[L.first + k] = (int)(roff + (size_t)k * 2 * L.ntot);
      roff += (size_t)L.n * 2 * L.ntot;
    };
    for (int l = Hs; l < nlev; ++l) place(l);
    dev.rhs_top = roff; dev.gh_off = roff; roff += 2 * dev.h_top_g.size();
    for (int l = 0; l < Hs; ++l) place(l);
    dev.rhs_elems = roff;
  }
  // leaves the front row of every ancestor variable a node's subtree couples to: nd_fidx[nd_abase[node][depth of the ancestor] + ordinal]
  void ancestor_rows() {
    dev.h_abase.assign((size_t)nl * hp.maxdepth, -1);
    for (int i = 0; i < nl; ++i) {
      const int n = order[i];
      for (int a = hp.parent[n]; a >= 0; a = hp.parent[a]) {
        dev.h_abase[(size_t)i * hp.maxdepth + hp.depth[a]] = (int)dev.h_fidx.size();
        dev.h_fidx.resize(dev.h_fidx.size() + hp.own[a].size(), -1);
      }
      int row = dev.h_nI[i];
      for (int v : hp.strct[n]) {
        const int a = hp.vnode[v];
        dev.h_fidx[dev.h_abase[(size_t)i * hp.maxdepth + hp.depth[a]] + hp.vord[v]] = row;
        row += NdHostPlan::vdim(v);
      }
    }
  }
  // leaves the children of every front by kind (cptr / cidx) and the map (parent front row -> child front row) the extend-add gathers through
  // (h_inv_off / h_inv)
  void children_and_row_maps() {
    for (int kind = 0; kind < 2; ++kind) cptr[kind].assign(nl + 1, 0);
    dev.h_inv_off.assign(nl, -1);
    for (int i = 0; i < nl; ++i) {
      const int n = order[i];
      for (int kind = 0; kind < 2; ++kind) cptr[kind][i + 1] = cptr[kind][i];
      for (int c : hp.child[n]) {
        if (!is_local(c)) continue;   // another rank's subtree: its contribution arrives through the all-reduce of the top fronts
        const int kind = is_top(c) ? kTopChild : kSubtreeChild;
        cidx[kind].push_back(newid[c]); ++cptr[kind][i + 1];
      }
      const int p = hp.parent[n];
      if (p < 0) continue;
      const int ip = newid[p];   // (a local node's parent is local: own subtree or top)
      dev.h_inv_off[i] = (int)dev.h_inv.size();
      dev.h_inv.resize(dev.h_inv.size() + ld[ip], -1);
      int* inv = dev.h_inv.data() + dev.h_inv_off[i];
      int row = dev.h_nI[i];
      for (int v : hp.strct[n]) {
        // the variable's row in the parent's front: own column there, or one of the parent's border rows
        const int prow = hp.vnode[v] == p ? hp.voff[v] : dev.h_fidx[dev.h_abase[(size_t)ip * hp.maxdepth + hp.depth[hp.vnode[v]]] + hp.vord[v]];
        for (int r = 0; r < NdHostPlan::vdim(v); ++r) inv[prow + r] = row + r;
        row += NdHostPlan::vdim(v);
      }
    }
  }
  // Round 6: the border x border part of a front is never cleared (k_nd_zero) — the extend-add STORES every entry of the 64-tiles it visits there
  // (children's sum, or zero), so it must visit every lower 64-tile of each 128-tile some child reaches (NdDev::bb marks those for the first
  // trailing update, which reads them; the others it starts from zero itself). Leaves those 64-tiles marked, from tile t0 on.
  static void whole_border_tiles(std::vector<char>& mark, int T, int t0) {
    for (int A = t0; A < T; A += 2)
      for (int B = t0; B <= A; B += 2) {
        bool any = false;
        for (int a = A; a < std::min(T, A + 2); ++a) for (int b = B; b < std::min(T, B + 2); ++b) if (b <= a && mark[(size_t)a * T + b]) any = true;
        if (any) for (int a = A; a < std::min(T, A + 2); ++a) for (int b = B; b < std::min(T, B + 2); ++b) if (b <= a) mark[(size_t)a * T + b] = 1;
      }
  }
  // leaves level l's extend-add work list for its children of one kind appended to ext / ext_kind: the 64x64 tiles of the parents' fronts that
  // receive something from such a child, and its place (first, count, countA) in the level
  void extend_tiles(int l, ChildKind kind, int& first, int& count, int& countA) {
    const NdLevel& L = dev.lev[l];
    first = (int)ext.size() / 3;
    std::vector<int> tiles;
    for (int k = 0; k < L.n; ++k) {
      const int i = L.first + k;
      const int T = (ld[i] + 63) / 64;
      std::vector<char> mark((size_t)T * T, 0);
      for (int q = cptr[kind][i]; q < cptr[kind][i + 1]; ++q) {
        std::vector<int> rows;
        reached_tiles(i, cidx[kind][q], 0, 64, T, [&](int t) { rows.push_back(t); });
        for (int a : rows) for (int b : rows) if (b <= a) mark[(size_t)a * T + b] = 1;
      }
      if (kind == kSubtreeChild && !is_top(order[i])) whole_border_tiles(mark, T, dev.h_nI[i] / 64);
      for (int a = 0; a < T; ++a) for (int b = 0; b <= a; ++b) if (mark[(size_t)a * T + b]) { tiles.push_back(i); tiles.push_back(a); tiles.push_back(b); }
    }
    // tiles of the fronts' first 256 rows (what the first panel's factorisation needs) first: NdLevel::ext_countA
    countA = 0;
    for (int pass = 0; pass < 2; ++pass)
      for (size_t q = 0; q < tiles.size(); q += 3)
        if ((tiles[q + 1] < 4) == (pass == 0)) {
          ext.insert(ext.end(), tiles.begin() + q, tiles.begin() + q + 3); countA += pass == 0 ? 1 : 0;
          ext_kind.push_back(kind);
        }
    count = (int)ext.size() / 3 - first;
  }
  // leaves NdLevel::split_ta: the border tiles of level l's fronts that carry unknowns of the parents' first 256 columns (a front's border lists
  // its parent's unknowns first, in the parent's own order)
  void split_ta(int l) {
    NdLevel& L = dev.lev[l];
    L.split_ta = 0;
    for (int k = 0; k < L.n; ++k) {
      const int n = order[L.first + k], p = hp.parent[n];
      if (p < 0) continue;
      int d = 0;
      for (int v : hp.strct[n]) if (hp.vnode[v] == p && hp.voff[v] < 256) d += NdHostPlan::vdim(v);
      L.split_ta = std::max(L.split_ta, (d + kTile - 1) / kTile);
    }
  }
  // front / child descriptor shared by the three encodings: {offset lo, hi | leading dimension | right-hand side offset}
  void put_front(int* w, int node) const {
    const unsigned long long mo = (unsigned long long)dev.h_ntab[2 * (size_t)node];
    w[0] = (int)(unsigned)(mo & 0xffffffffull); w[1] = (int)(unsigned)(mo >> 32); w[2] = (int)dev.h_ntab[2 * (size_t)node + 1]; w[3] = dev.h_rhs_node[node];
  }
  // leaves the flattened work / child lists of k_nd_extend (NdDev::extw / extc / extc2)
  void flat_lists() {
    for (int kind = 0; kind < 2; ++kind) {
      std::vector<int>& out = kind == kTopChild ? dev.h_extc2 : dev.h_extc;
      out.resize(6 * cidx[kind].size());
      for (size_t k = 0; k < cidx[kind].size(); ++k) {
        int* c = out.data() + 6 * k;
        put_front(c, cidx[kind][k]); c[4] = dev.h_inv_off[cidx[kind][k]]; c[5] = 0;
      }
    }
    const size_t nt = ext.size() / 3;
    dev.h_extw.resize(8 * nt);
    for (size_t q = 0; q < nt; ++q) {
      const int node = ext[3 * q];
      const std::vector<int>& cp = cptr[ext_kind[q]];
      int* w = dev.h_extw.data() + 8 * q;
      put_front(w, node);
      w[4] = ext[3 * q + 1]; w[5] = ext[3 * q + 2]; w[6] = cp[node]; w[7] = cp[node + 1];
    }
  }
  // Round 6, the same lists as RECORDS of kExtRec ints (k_nd_extend_rec): per tile ONE record {header | first contributing child | that child's row
  // maps for the tile's 64 rows and 64 columns}, found by the tile's index alone, and one overflow record per further contributing child. The kernel's
  // chain of dependent loads is record -> values instead of tile -> child entries -> row maps -> values; children that reach neither the tile's rows
  // nor its columns are not visited at all (their terms were zero: same sums, same order). Leaves h_extr / ext_over.
  void records() {
    const size_t nt = ext.size() / 3;
    dev.h_extr.assign((size_t)kExtRec * nt, -1);
    dev.ext_over = nt;
    for (size_t q = 0; q < nt; ++q) {
      const int node = ext[3 * q], a = ext[3 * q + 1], b = ext[3 * q + 2], kind = ext_kind[q];
      int nrec = 0;
      const size_t next = dev.h_extr.size() / kExtRec - nt;
      for (int k = cptr[kind][node]; k < cptr[kind][node + 1]; ++k) {
        const int ch = cidx[kind][k];
        bool anyr = false, anyc = false;
        reached_tiles(node, ch, 64 * a, 64, 1, [&](int) { anyr = true; });
        reached_tiles(node, ch, 64 * b, 64, 1, [&](int) { anyc = true; });
        if (!anyr || !anyc) continue;
        if (nrec > 0) dev.h_extr.resize(dev.h_extr.size() + kExtRec, -1);
        int* r = nrec == 0 ? dev.h_extr.data() + (size_t)kExtRec * q : dev.h_extr.data() + dev.h_extr.size() - kExtRec;
        put_front(r + 8, ch);
        const int* inv = dev.h_inv.data() + dev.h_inv_off[ch];
        for (int e = 0; e < 64; ++e) {
          const int rr = 64 * a + e, cc = 64 * b + e;
          r[16 + e] = rr < ld[node] ? inv[rr] : -1; r[80 + e] = cc < ld[node] ? inv[cc] : -1;
        }
        ++nrec;
      }
      int* w = dev.h_extr.data() + (size_t)kExtRec * q;
      for (int e = 0; e < 6; ++e) w[e] = dev.h_extw[8 * q + e];
      w[6] = nrec; w[7] = (int)next;
    }
  }
  // leaves the border x border 128-tiles that receive something from a child (NdDev::bb): only those are cleared per iteration and read by the first
  // panel's trailing update. A top front of a sharded solve is summed over the ranks as it stands: all its tiles count as contributed to.
  void border_maps() {
    dev.h_bb_off.assign(nl, 0);
    for (int i = 0; i < nl; ++i) {
      const int nI = dev.h_nI[i], lb = (ld[i] - nI + kTile - 1) / kTile;
      dev.h_bb_off[i] = (int)dev.h_bb.size();
      dev.h_bb.resize(dev.h_bb.size() + (size_t)lb * (lb + 1) / 2, is_top(order[i]) ? 1 : 0);
      if (is_top(order[i]) || lb == 0) continue;
      int* bb = dev.h_bb.data() + dev.h_bb_off[i];
      for (int kind = 0; kind < 2; ++kind)
        for (int q = cptr[kind][i]; q < cptr[kind][i + 1]; ++q) {
          std::vector<int> rows;
          reached_tiles(i, cidx[kind][q], nI, kTile, lb, [&](int t) { rows.push_back(t); });
          for (int a : rows) for (int b : rows) if (b <= a) bb[a * (a + 1) / 2 + b] = 1;
        }
    }
  }
  // leaves the groups of levels whose backward substitution runs as one launch (tree_levels / tree_top0) and the solution indices of their
  // fronts' own unknowns (h_tree_fill)
  void backward_groups() {
    // bottom levels (k_bwd.hip: k_bwd_tree): while a level's fronts hold at most two interior tiles
    int ls = 0;
    const int lmax = std::min(std::min(nlev, Hs), kBwdTreeMax);
    while (ls < lmax && dev.lev[ls].n > 0 && dev.lev[ls].n <= 65535 && (dev.lev[ls].own_max + kTile - 1) / kTile <= 2) ++ls;
    dev.tree_levels = ls >= 2 ? ls : 0;
    // the top levels, from the root down while the tile workgroups stay within 128 (k_bwd_tree64: a workgroup takes a whole CU) and every front has two
    // interior tiles or more somewhere in the level
    int lt = nlev, wgs = 0;
    while (lt > dev.tree_levels && nlev - lt < kBwdTreeMax) {
      const NdLevel& L = dev.lev[lt - 1];
      const int T = L.interior_tiles();
      if (L.n <= 0 || T < 2 || wgs + L.n * T > 128) break;
      wgs += L.n * T; --lt;
    }
    dev.tree_top0 = nlev - lt >= 2 ? lt : nlev;
    for (int l = 0; l < nlev; ++l)
      if (l < dev.tree_levels || l >= dev.tree_top0)
        for (int i = dev.lev[l].first; i < dev.lev[l].first + dev.lev[l].n; ++i)
          for (int q = 0; q < dev.h_own_dims[i]; ++q) dev.h_tree_fill.push_back(dev.h_gidx[dev.h_own_g[i] + q]);
  }
  // leaves panel P's exchange entries appended to h_dist_ent (NdLevel::dx_*): the live tiles of the panel's real tile columns, from the diagonal
  // down, then 256 right-hand-side rows, of every front whose interior reaches the panel (the others hold identity padding there, the same on
  // every rank); and the reduce buffer's sizes
  void dist_exchange(NdLevel& L, int P) {
    const int t0 = 2 * P, tI = L.nI / kTile;
    L.dx_first[P] = (int)dev.h_dist_ent.size() / 4;
    for (int pass = 0; pass < 2; ++pass)
      for (int k = 0; k < L.n; ++k) {
        const int i = L.first + k, nIr = L.live_h[2 * k], nO = L.live_h[2 * k + 1], Tn = ld[i] / kTile;
        if (t0 >= nIr) continue;
        if (pass == 1) {
          const int rows = std::min(256, ld[i] - t0 * kTile);
          dev.h_dist_ent.insert(dev.h_dist_ent.end(), {i, t0 * kTile, rows, 1});
          ++L.dx_nr[P];
          continue;
        }
        for (int c = t0; c < std::min(t0 + 2, nIr); ++c)
          for (int t = c; t < Tn; ++t)
            if (live(t, nIr, tI, nO)) { dev.h_dist_ent.insert(dev.h_dist_ent.end(), {i, t, c, 0}); ++L.dx_nt[P]; }
      }
    const size_t elems = (size_t)L.dx_nt[P] * kTile * kTile + (size_t)L.dx_nr[P] * 256;
    dev.dist_buf_elems = std::max(dev.dist_buf_elems, elems);
    dev.dist_solve_elems += elems;
  }
  // leaves panel P's owned trailing-update tiles (i, j), j <= i, relative to tile tb, appended to h_dist_tri (NdLevel::dt_*): tile row owner by
  // nd_tile_owner on the front's compact rows (real interior tiles, then border tiles); XCD-balanced as k_chol.hip's live_tile_list (whole 8x8
  // supertiles of a front to the shortest of 8 queues, interleaved)
  void dist_owned_tiles(NdLevel& L, int P) {
    const int world = std::max(hp.world, 1);
    const int t0 = 2 * P, tb = t0 + 2, T = L.ntot / kTile, tI = L.nI / kTile;
    std::vector<int> q[8];
    for (int k = 0; k < L.n; ++k) {
      const int i = L.first + k, nIr = L.live_h[2 * k], nO = L.live_h[2 * k + 1], node = order[i];
      if (t0 >= nIr) continue;
      auto mine = [&](int t) { return nd_tile_owner(node, t < tI ? t : nIr + (t - tI), world) == rank; };
      const int nt = T - tb, Ts = (nt + 7) / 8;
      for (int si = 0; si < Ts; ++si)
        for (int sj = 0; sj <= si; ++sj) {
          std::vector<int> grp;
          for (int a = 8 * si; a < std::min(nt, 8 * si + 8); ++a) {
            if (!live(tb + a, nIr, tI, nO) || !mine(tb + a)) continue;
            for (int b = 8 * sj; b < std::min(a + 1, 8 * sj + 8); ++b) if (live(tb + b, nIr, tI, nO)) grp.push_back((k << 20) | (a << 10) | b);
          }
          if (grp.empty()) continue;
          int best = 0;
          for (int x = 1; x < 8; ++x) if (q[x].size() < q[best].size()) best = x;
          q[best].insert(q[best].end(), grp.begin(), grp.end());
        }
    }
    size_t longest = 0;
    for (int x = 0; x < 8; ++x) longest = std::max(longest, q[x].size());
    L.dt_first[P] = (int)dev.h_dist_tri.size();
    L.dt_cnt[P] = (int)(8 * longest);
    dev.h_dist_tri.resize(dev.h_dist_tri.size() + 8 * longest, -1);
    for (int x = 0; x < 8; ++x) for (size_t e = 0; e < q[x].size(); ++e) dev.h_dist_tri[L.dt_first[P] + 8 * e + x] = q[x][e];
  }
  // shard policy 1 (distributed top): leaves, per panel of every top level, what is exchanged and which trailing-update tiles this rank applies
  void dist_panels() {
    dev.dist = sh && hp.shard_policy == 1;
    dev.dist_lead = rank == 0;
    if (!dev.dist) return;
    for (int l = Hs; l < nlev; ++l) {
      NdLevel& L = dev.lev[l];
      const int np = L.nI / 256;
      L.dx_first.assign(np, 0); L.dx_nt.assign(np, 0); L.dx_nr.assign(np, 0); L.dt_first.assign(np, 0); L.dt_cnt.assign(np, 0);
      for (int P = 0; P < np; ++P) { dist_exchange(L, P); dist_owned_tiles(L, P); }
    }
    dev.dist_solve_elems += 2 * dev.h_top_g.size();   // gradient and diag(J^T J) of the top unknowns
  }
};

}  // namespace

void nd_tables(const NdHostPlan& hp, const int* pos_kf, int D, int rank, NdDev& dev) {
  dev = NdDev();
  FrontTables t(hp, pos_kf, D, rank, dev);
  t.level_order();
  t.variable_maps();
  t.front_layout();
  t.rhs_layout();
  t.ancestor_rows();
  t.children_and_row_maps();
  for (int l = 0; l < t.nlev; ++l) {
    NdLevel& L = dev.lev[l];
    t.extend_tiles(l, kSubtreeChild, L.ext_first, L.ext_count, L.ext_countA);
    t.extend_tiles(l, kTopChild, L.ext2_first, L.ext2_count, L.ext2_countA);
    t.split_ta(l);
  }
  t.flat_lists();
  t.records();
  t.border_maps();
  t.backward_groups();
  t.dist_panels();
  dev.active = true;
}

}  // namespace covgpu
