// nd_tables_dump.hip — every host table of the multifrontal solve (nd_tables: covins_amd/csrc/nd_tables.hip) for a fixed set of small plans, written
// to a file: two builds of the table builder are compared byte for byte through their dumps (profiles/front_tables_compare.txt). Host only, no GPU.
//   hipcc -O2 -std=c++17 -I covins_amd/csrc tools/nd_tables_dump.hip covins_amd/csrc/nd_plan.o covins_amd/csrc/nd_tables.o -pthread -o nd_tables_dump
//   nd_tables_dump OUT          the dump; prints per plan how often each branch of the builder ran, exit 1 if one of them never ran in the whole set
//   nd_tables_dump --time N     mean milliseconds of N calls of nd_tables on the largest plan of the set
// The plans are chain graphs: `nch` agents of `len` keyframes, covisibility `w` keyframes along a chain, every `loop`-th keyframe covisible with the
// same position of the next agent; visual-inertial. world > 0: sharded over that many ranks (policy 0 replicated | 1 distributed top), every rank dumped.
#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "common.hpp"
#include "nd_plan.hpp"

using namespace covgpu;

struct PlanSpec { const char* name; int nch, len, w, loop, leaf, world, policy, min_order; };
static const PlanSpec kPlans[] = {
    {"one_agent", 1, 300, 30, 0, 0, 0, 0, 0},              // the planner's own leaf size, merged levels; separators of 30 keyframes: the top one-launch group
    {"three_agents_wide_leaves", 3, 120, 45, 6, 600, 0, 0, 0},   // leaf regions of up to 600 unknowns under wide separators
    {"three_agents_small_leaves", 3, 100, 4, 9, 120, 0, 0, 0},   // a deep tree of small fronts: the bottom one-launch group
    {"four_agents_replicated", 4, 100, 6, 7, 150, 2, 0, 0},
    {"five_agents_replicated", 5, 80, 6, 5, 200, 3, 0, 0},
    {"four_agents_distributed", 4, 100, 6, 7, 150, 2, 1, 300},
    {"five_agents_distributed", 5, 80, 12, 3, 200, 3, 1, 400},
};
constexpr int kNumPlans = (int)(sizeof(kPlans) / sizeof(kPlans[0]));

static bool build_plan(const PlanSpec& s, NdHostPlan& hp, std::vector<int>& pos_kf) {
  const int K = s.nch * s.len;
  std::vector<int> chain_ptr(s.nch + 1), pi, pj;
  for (int c = 0; c <= s.nch; ++c) chain_ptr[c] = c * s.len;
  for (int c = 0; c < s.nch; ++c)
    for (int q = 0; q < s.len; ++q) {
      const int i = c * s.len + q;
      for (int d = 1; d <= s.w && q - d >= 0; ++d) { pi.push_back(i); pj.push_back(i - d); }
      if (s.loop > 0 && c + 1 < s.nch && q % s.loop == 0) { pi.push_back(i + s.len); pj.push_back(i); }
    }
  if (!nd_plan_build(K, true, s.nch, chain_ptr.data(), (int)pi.size(), pi.data(), pj.data(), 0, nullptr, nullptr, s.leaf, hp, s.world > 0 ? 0 : -1)) return false;
  if (s.world > 0 && s.policy == 0) nd_shard_assign(hp, s.world);
  if (s.world > 0 && s.policy == 1) nd_shard_assign_dist(hp, s.world, 48.0 * 1048576.0, s.min_order);
  pos_kf.resize(K);
  for (int q = 0; q < K; ++q) pos_kf[q] = (7 * q + 3) % K;   // (K is no multiple of 7 in any plan: a permutation)
  return true;
}

static FILE* g_out = nullptr;
template <class T> static void put(const char* name, const std::vector<T>& v) {
  std::fprintf(g_out, "%s %zu:", name, v.size());
  for (const T& x : v) std::fprintf(g_out, " %lld", (long long)x);
  std::fprintf(g_out, "\n");
}
static void put(const char* name, long long x) { std::fprintf(g_out, "%s %lld\n", name, x); }

static void dump(const NdDev& d) {
  put("active", d.active); put("nnodes", d.nnodes); put("top_lev0", d.top_lev0); put("tree_levels", d.tree_levels); put("tree_top0", d.tree_top0);
  put("ext_over", (long long)d.ext_over); put("ntop", d.ntop); put("n_top_tiles", d.n_top_tiles); put("M_sub", (long long)d.M_sub);
  put("rhs_top", (long long)d.rhs_top); put("gh_off", (long long)d.gh_off); put("dist", d.dist); put("dist_lead", d.dist_lead);
  put("dist_buf_elems", (long long)d.dist_buf_elems); put("dist_solve_elems", (long long)d.dist_solve_elems); put("M_elems", (long long)d.M_elems);
  put("rhs_elems", (long long)d.rhs_elems); put("linv_elems", (long long)d.linv_elems);
  std::fprintf(g_out, "plan_flops %.17g\n", d.plan_flops);
  put("h_tree_fill", d.h_tree_fill); put("h_extw", d.h_extw); put("h_extc", d.h_extc); put("h_extc2", d.h_extc2); put("h_extr", d.h_extr);
  put("h_top_tiles", d.h_top_tiles); put("h_vnode", d.h_vnode); put("h_voff", d.h_voff); put("h_vord", d.h_vord); put("h_vown", d.h_vown);
  put("h_ndepth", d.h_ndepth); put("h_nI", d.h_nI); put("h_abase", d.h_abase); put("h_fidx", d.h_fidx); put("h_own_dims", d.h_own_dims);
  put("h_st_dims", d.h_st_dims); put("h_own_g", d.h_own_g); put("h_st_g", d.h_st_g); put("h_gidx", d.h_gidx); put("h_inv_off", d.h_inv_off);
  put("h_inv", d.h_inv); put("h_rhs_node", d.h_rhs_node); put("h_top_var", d.h_top_var); put("h_top_r", d.h_top_r); put("h_top_g", d.h_top_g);
  put("h_bb_off", d.h_bb_off); put("h_bb", d.h_bb); put("h_ntab", d.h_ntab); put("h_dist_ent", d.h_dist_ent); put("h_dist_tri", d.h_dist_tri);
  for (size_t l = 0; l < d.lev.size(); ++l) {
    const NdLevel& L = d.lev[l];
    std::fprintf(g_out, "level %zu\n", l);
    put("n", L.n); put("nI", L.nI); put("ntot", L.ntot); put("first", L.first); put("rhs_off", (long long)L.rhs_off); put("linv_off", (long long)L.linv_off);
    put("own_max", L.own_max); put("ext_first", L.ext_first); put("ext_count", L.ext_count); put("ext_countA", L.ext_countA); put("split_ta", L.split_ta);
    put("ext2_first", L.ext2_first); put("ext2_count", L.ext2_count); put("ext2_countA", L.ext2_countA);
    put("live_h", L.live_h); put("plist_h", L.plist_h); put("pbig", L.pbig); put("psmall", L.psmall);
    put("dx_first", L.dx_first); put("dx_nt", L.dx_nt); put("dx_nr", L.dx_nr); put("dt_first", L.dt_first); put("dt_cnt", L.dt_cnt);
  }
}

// how often the branches of the builder ran: every column must be non-zero somewhere in the set
enum { C_TOP_NODES, C_TOP_CHILDREN, C_OVERFLOW, C_TREE_BOTTOM, C_TREE_TOP, C_WIDE_LEVEL, C_BORDER_UNTOUCHED, C_DIST_PANEL, C_COUNT };
static const char* const kCover[C_COUNT] = {"top_nodes", "top_children", "overflow_records", "tree_levels>=2", "tree_top0<levels", "level_nI>256",
                                            "h_bb_zero", "dist_panel_xchg_and_tiles"};
static void cover(const NdDev& d, long long* c) {
  const int nlev = (int)d.lev.size();
  c[C_TOP_NODES] += nlev > d.top_lev0 ? d.nnodes - d.lev[d.top_lev0].first : 0;
  c[C_OVERFLOW] += (long long)(d.h_extr.size() / kExtRec) - (long long)d.ext_over;
  c[C_TREE_BOTTOM] += d.tree_levels >= 2;
  c[C_TREE_TOP] += d.tree_top0 < nlev;
  for (int b : d.h_bb) c[C_BORDER_UNTOUCHED] += b == 0;
  for (const NdLevel& L : d.lev) {
    c[C_TOP_CHILDREN] += L.ext2_count;
    c[C_WIDE_LEVEL] += L.nI > 256;
    for (size_t P = 0; P < L.dx_nt.size(); ++P) c[C_DIST_PANEL] += d.dist && L.dx_nt[P] > 0 && L.dt_cnt[P] > 0;
  }
}

int main(int argc, char** argv) {
  if (argc == 3 && std::strcmp(argv[1], "--time") == 0) {
    const int reps = std::max(1, std::atoi(argv[2]));
    int big = 0;
    for (int p = 1; p < kNumPlans; ++p) if (kPlans[p].nch * kPlans[p].len > kPlans[big].nch * kPlans[big].len) big = p;
    NdHostPlan hp; std::vector<int> pos_kf;
    if (!build_plan(kPlans[big], hp, pos_kf)) return 2;
    NdDev d;
    nd_tables(hp, pos_kf.data(), 15, 0, d);
    const auto t0 = std::chrono::steady_clock::now();
    for (int r = 0; r < reps; ++r) nd_tables(hp, pos_kf.data(), 15, 0, d);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / reps;
    std::printf("%s: nd_tables %.4f ms (mean of %d)\n", kPlans[big].name, ms, reps);
    return 0;
  }
  if (argc != 2) { std::fprintf(stderr, "usage: %s OUT | --time N\n", argv[0]); return 2; }
  g_out = std::fopen(argv[1], "w");
  if (g_out == nullptr) { std::perror(argv[1]); return 2; }
  long long total[C_COUNT] = {0};
  std::printf("%-28s", "plan");
  for (int k = 0; k < C_COUNT; ++k) std::printf(" %s", kCover[k]);
  std::printf("\n");
  for (const PlanSpec& s : kPlans) {
    NdHostPlan hp; std::vector<int> pos_kf;
    if (!build_plan(s, hp, pos_kf)) { std::fprintf(stderr, "%s: no plan\n", s.name); return 2; }
    long long c[C_COUNT] = {0};
    for (int rank = 0; rank < std::max(s.world, 1); ++rank) {
      NdDev d;
      nd_tables(hp, pos_kf.data(), 15, rank, d);
      if (d.ntop != (int)d.h_top_g.size() || d.n_top_tiles != (int)(d.h_top_tiles.size() / 3)) {
        std::fprintf(stderr, "%s rank %d: ntop / n_top_tiles not set by the builder\n", s.name, rank); return 3;
      }
      std::fprintf(g_out, "plan %s rank %d nodes %d\n", s.name, rank, hp.nnodes);
      dump(d);
      cover(d, c);
    }
    std::printf("%-28s", s.name);
    for (int k = 0; k < C_COUNT; ++k) { std::printf(" %lld", c[k]); total[k] += c[k]; }
    std::printf("\n");
  }
  std::fclose(g_out);
  bool all = true;
  for (int k = 0; k < C_COUNT; ++k) if (total[k] == 0) { std::fprintf(stderr, "never ran: %s\n", kCover[k]); all = false; }
  return all ? 0 : 1;
}
