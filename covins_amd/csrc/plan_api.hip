// plan_api.hip — the host-only plan entry points of libcovgpu: the keyframe order an upload and a plan share (build_chains,
// build_chains_pgo), covgpu_nd_plan_* (the nested-dissection plan of nd_plan.hip for inspection and the CPU tests),
// covgpu_shard_plan (the multi-GPU split of one map) and covgpu_pgo_partition. Nothing here touches a device.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "host.hpp"

using namespace covgpu;

bool plan_timing_on() { return getenv("COVGPU_PLAN_TIMING") != nullptr; }

// IMU chains (one per agent: predecessor -> successor factors, optimization_be.cpp:369-416) laid out back to back:
// perm[kf] = chain-major position, pos_kf = inverse, chain_ptr = positions of each chain. Without IMU factors every
// keyframe is its own position (identity order, one "chain").
int build_chains(const covgpu_problem* p, bool vi, std::vector<int>& perm, std::vector<int>& pos_kf, std::vector<int>& chain_ptr) {
  const int K = p->num_kf, I = vi ? p->num_imu : 0;
  perm.assign(K, 0); pos_kf.assign(K, 0); chain_ptr.assign(1, 0);
  if (vi) {
    std::vector<int> succ(K, -1), has_pred(K, 0);
    for (int f = 0; f < I; ++f) {
      const int i = p->imu_kf_i[f], j = p->imu_kf_j[f];
      if (i == j || succ[i] != -1 || has_pred[j]) { g_err = "invalid problem: IMU factors must form simple predecessor chains"; return COVGPU_ERR_INVALID_ARG; }
      succ[i] = j; has_pred[j] = 1;
    }
    int pos = 0;
    for (int k = 0; k < K; ++k) {
      if (has_pred[k]) continue;
      for (int c = k; c != -1; c = succ[c]) { perm[c] = pos; pos_kf[pos] = c; ++pos; }
      chain_ptr.push_back(pos);
    }
    if (pos != K) { g_err = "invalid problem: IMU factors contain a cycle"; return COVGPU_ERR_INVALID_ARG; }
  } else {
    for (int k = 0; k < K; ++k) { perm[k] = k; pos_kf[k] = k; }
    chain_ptr.push_back(K);
  }
  return COVGPU_OK;
}

// Pose graph (round 6: the multifrontal solve of k_front.hip serves PoseGraphOptimization too): there are no IMU factors to read an agent's
// time axis from, and the map hands keyframes over agent-interleaved (typedefs_base.hpp:178) — index distance says nothing. The edge list does:
// an edge whose endpoints share no neighbour is a bridge between otherwise unrelated parts of the graph, a loop closure
// (optimization_be.cpp:912-944); the odometry edges of one agent (every keyframe tied to its five predecessors, :947-1021) always share
// neighbours. "Chains" = connected components of the graph without its bridges, each laid out in breadth-first order from a pseudo-peripheral
// keyframe — along an odometry chain that IS the time axis up to a few places, and nd_plan's halving of a chain then cuts ~5 keyframes.
void build_chains_pgo(const covgpu_problem* p, std::vector<int>& perm, std::vector<int>& pos_kf, std::vector<int>& chain_ptr) {
  const int K = p->num_kf, E = p->num_edge;
  perm.assign(K, 0); pos_kf.assign(K, 0); chain_ptr.assign(1, 0);
  std::vector<std::vector<int>> adj(K);
  for (int e = 0; e < E; ++e) if (p->edge_i[e] != p->edge_j[e]) { adj[p->edge_i[e]].push_back(p->edge_j[e]); adj[p->edge_j[e]].push_back(p->edge_i[e]); }
  for (auto& a : adj) { std::sort(a.begin(), a.end()); a.erase(std::unique(a.begin(), a.end()), a.end()); }
  auto bridge = [&](int u, int v) {
    const std::vector<int>&A = adj[u], &B = adj[v];
    for (size_t x = 0, y = 0; x < A.size() && y < B.size();) { if (A[x] == B[y]) return false; if (A[x] < B[y]) ++x; else ++y; }
    return A.size() > 1 || B.size() > 1;
  };
  std::vector<std::vector<int>> nb(K);   // neighbours over non-bridge edges
  for (int u = 0; u < K; ++u) for (int v : adj[u]) if (!bridge(u, v)) nb[u].push_back(v);
  std::vector<int> level(K, -1), queue;
  std::vector<char> placed(K, 0);
  auto bfs = [&](int start) {
    queue.assign(1, start); level[start] = 0;
    for (size_t h = 0; h < queue.size(); ++h) { const int u = queue[h]; for (int v : nb[u]) if (level[v] < 0) { level[v] = level[u] + 1; queue.push_back(v); } }
    return queue.back();
  };
  int pos = 0;
  for (int k = 0; k < K; ++k) {
    if (placed[k]) continue;
    const int far = bfs(k);
    for (int v : queue) level[v] = -1;
    bfs(far);   // second sweep from a pseudo-peripheral keyframe: its breadth-first order is the layout
    for (int v : queue) { level[v] = -1; placed[v] = 1; perm[v] = pos; pos_kf[pos] = v; ++pos; }
    chain_ptr.push_back(pos);
  }
}

// unique covisible pairs (free keyframes only) and edge pairs, as chain-major positions i > j (host-only plan functions;
// upload_impl builds the same pair list with the per-pair observation lists the device needs)
static bool host_pairs(const covgpu_problem* p, const std::vector<int>& perm, std::vector<int>& pi, std::vector<int>& pj, std::vector<int>& ei,
                       std::vector<int>& ej) {
  std::vector<long long> keys;
  for (int l = 0; l < p->num_lm; ++l)
    for (int a = p->lm_obs_ptr[l]; a < p->lm_obs_ptr[l + 1]; ++a) {
      if (p->kf_fixed[p->obs_kf[a]]) continue;
      for (int b = p->lm_obs_ptr[l]; b < p->lm_obs_ptr[l + 1]; ++b) {
        if (p->kf_fixed[p->obs_kf[b]]) continue;
        const int pa = perm[p->obs_kf[a]], pb = perm[p->obs_kf[b]];
        if (pb < pa) keys.push_back(((long long)pa << 32) | (unsigned)pb);
      }
    }
  std::sort(keys.begin(), keys.end()); keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
  pi.resize(keys.size()); pj.resize(keys.size()); ei.clear(); ej.clear();
  for (size_t q = 0; q < keys.size(); ++q) { pi[q] = (int)(keys[q] >> 32); pj[q] = (int)(keys[q] & 0xffffffffll); }
  for (int e = 0; e < p->num_edge; ++e) {
    const int a = perm[p->edge_i[e]], b = perm[p->edge_j[e]];
    if (a == b) return false;
    ei.push_back(std::max(a, b)); ej.push_back(std::min(a, b));
  }
  return true;
}

// Host-only: the nested-dissection plan of the reduced camera system (nd_plan.hpp, k_front.hip) for inspection and the CPU
// tests (tests/test_nd_plan.py replays the elimination in numpy on the oracle's system).
int nd_leaf_dims(int requested) {   // 0: nd_plan_build chooses among its candidates (nd_plan.hip)
  if (requested > 0) return requested;
  const char* e = getenv("COVGPU_ND_LEAF");
  const int v = e ? atoi(e) : 0;
  return v > 0 ? v : 0;
}
static int nd_plan_create_mode(const covgpu_options* opt, const covgpu_problem* p, int32_t leaf_dims, covgpu_nd_plan** out, int top_mode);
extern "C" int covgpu_nd_plan_create(const covgpu_options* opt, const covgpu_problem* p, int32_t leaf_dims, covgpu_nd_plan** out) { return nd_plan_create_mode(opt, p, leaf_dims, out, -1); }
static int nd_plan_create_mode(const covgpu_options* opt, const covgpu_problem* p, int32_t leaf_dims, covgpu_nd_plan** out, int top_mode) {
  return guarded([&] {
    const bool vi = !opt->visual_only;
    *out = nullptr;
    RC(validate(p, false, vi));
    std::vector<int> perm, pos_kf, chain_ptr, pi, pj, ei, ej;
    RC(build_chains(p, vi, perm, pos_kf, chain_ptr));
    if (!host_pairs(p, perm, pi, pj, ei, ej)) { g_err = "invalid problem: self edge"; return (int)COVGPU_ERR_INVALID_ARG; }
    covgpu_nd_plan* pl = new covgpu_nd_plan();
    pl->pos_kf = pos_kf;
    const auto t_pl = std::chrono::steady_clock::now();
    struct PT { std::chrono::steady_clock::time_point t0; ~PT() { if (plan_timing_on()) std::fprintf(stderr, "[covgpu] nd_plan_build %.1f ms\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() * 1e3); } } pt{t_pl};
    if (!nd_plan_build(p->num_kf, vi, (int)chain_ptr.size() - 1, chain_ptr.data(), (int)pi.size(), pi.data(), pj.data(), (int)ei.size(), ei.data(), ej.data(),
                       nd_leaf_dims(leaf_dims), pl->hp, top_mode)) {
      delete pl; g_err = "nested-dissection plan: a coupling joins two branches"; return (int)COVGPU_ERR_INVALID_ARG;
    }
    *out = pl;
    return (int)COVGPU_OK;
  });
}
// Host-only: the plan PoseGraphOptimization's solve runs on (round 6): 6-dof blocks, chains read from the edge graph (build_chains_pgo), couplings = the edge pairs
extern "C" int covgpu_nd_plan_create_pgo(const covgpu_options* opt, const covgpu_problem* p, int32_t leaf_dims, covgpu_nd_plan** out) {
  (void)opt;
  return guarded([&] {
    *out = nullptr;
    RC(validate(p, true, false));
    std::vector<int> perm, pos_kf, chain_ptr;
    build_chains_pgo(p, perm, pos_kf, chain_ptr);
    std::vector<uint64_t> keys;
    for (int e = 0; e < p->num_edge; ++e) {
      const int a = perm[p->edge_i[e]], b = perm[p->edge_j[e]];
      if (a == b) { g_err = "invalid problem: self edge"; return (int)COVGPU_ERR_INVALID_ARG; }
      keys.push_back(((uint64_t)(uint32_t)std::max(a, b) << 32) | (uint32_t)std::min(a, b));
    }
    std::sort(keys.begin(), keys.end()); keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    std::vector<int> ei(keys.size()), ej(keys.size());
    for (size_t q = 0; q < keys.size(); ++q) { ei[q] = (int)(keys[q] >> 32); ej[q] = (int)(keys[q] & 0xffffffffull); }
    covgpu_nd_plan* pl = new covgpu_nd_plan();
    pl->pos_kf = pos_kf;
    if (!nd_plan_build(p->num_kf, false, (int)chain_ptr.size() - 1, chain_ptr.data(), 0, nullptr, nullptr, (int)ei.size(), ei.data(), ej.data(), nd_leaf_dims(leaf_dims), pl->hp, -1, false)) {
      delete pl; g_err = "nested-dissection plan: a coupling joins two branches"; return (int)COVGPU_ERR_INVALID_ARG;
    }
    *out = pl;
    return (int)COVGPU_OK;
  });
}
extern "C" void covgpu_nd_plan_destroy(covgpu_nd_plan* pl) { delete pl; }
// out[16] = { nodes, levels, depth, own entries, front-structure entries, front elements (all batches), flops, largest own dims,
//             largest border dims, root own dims, 0 ... }
extern "C" void covgpu_nd_plan_info(const covgpu_nd_plan* pl, int64_t* out) {
  for (int i = 0; i < 16; ++i) out[i] = 0;
  const NdHostPlan& h = pl->hp;
  out[0] = h.nnodes; out[1] = h.nlev; out[2] = h.maxdepth;
  for (int n = 0; n < h.nnodes; ++n) {
    out[3] += (int64_t)h.own[n].size(); out[4] += (int64_t)h.strct[n].size();
    out[7] = std::max<int64_t>(out[7], h.own_dims[n]); out[8] = std::max<int64_t>(out[8], h.st_dims[n]);
    if (h.parent[n] < 0) out[9] = std::max<int64_t>(out[9], h.own_dims[n]);
  }
  out[5] = (int64_t)h.front_elems; out[6] = (int64_t)h.flops;
  out[10] = h.top_mode; out[11] = h.leaf; out[12] = h.group_frac100;   // which candidate tree (nd_plan_build): COVGPU_ND_TOP / COVGPU_ND_LEAF / COVGPU_ND_GROUP_FRAC (= out[12] / 100) reproduce it before the amalgamation: a shard plan and every plan with a forced leaf size exactly, a merged default plan not (a forced leaf size is never merged)
  out[13] = h.shard_policy;                                               // shard plans: 0 replicated top | 1 distributed top
}
extern "C" int32_t covgpu_nd_plan_rank_flops(const covgpu_nd_plan* pl, double* out) {
  const NdHostPlan& h = pl->hp;
  const int world = h.node_rank.empty() ? 1 : std::max(h.world, 1);
  NdShardAcct a;
  nd_shard_account(h, world, a);
  for (int r = 0; r < world; ++r) out[r] = a.rank_fl[r];
  return world;
}
extern "C" void covgpu_nd_plan_exchange(const covgpu_nd_plan* pl, int64_t* out) {
  const NdHostPlan& h = pl->hp;
  const int world = h.node_rank.empty() ? 1 : std::max(h.world, 1);
  NdShardAcct a;
  nd_shard_account(h, world, a);
  out[0] = (int64_t)a.bytes; out[1] = a.collectives; out[2] = world; out[3] = h.shard_policy;
}
// per node: parent, level, own_ptr / st_ptr [nodes + 1]; variables as 2 * IR keyframe + (0 pose | 1 speed-bias)
extern "C" void covgpu_nd_plan_arrays(const covgpu_nd_plan* pl, int32_t* parent, int32_t* level, int32_t* own_ptr, int32_t* own_var, int32_t* st_ptr,
                                      int32_t* st_var) {
  const NdHostPlan& h = pl->hp;
  int o = 0, s = 0;
  auto ir = [&](int v) { return 2 * pl->pos_kf[v >> 1] + (v & 1); };
  for (int n = 0; n < h.nnodes; ++n) {
    parent[n] = h.parent[n]; level[n] = h.level[n]; own_ptr[n] = o; st_ptr[n] = s;
    for (int v : h.own[n]) own_var[o++] = ir(v);
    for (int v : h.strct[n]) st_var[s++] = ir(v);
  }
  own_ptr[h.nnodes] = o; st_ptr[h.nnodes] = s;
}

// Host-only: the multi-GPU split of ONE map = the nested-dissection plan of the FULL problem
// plus, per tree node, the rank that owns it (nd_shard_assign: top of the tree replicated, subtrees dealt to the ranks), and
// the owner of every landmark / IMU factor / between factor: the rank of the DEEPEST tree node among the unknowns the
// residual touches (those unknowns form a clique of the coupling graph, so they lie on one root path: everything a residual
// contributes lands in fronts of its owner's subtrees or in top fronts — the only part that is all-reduced); residuals that
// touch top unknowns only are dealt round-robin. Returns the number of subtrees (0: nothing to split).
extern "C" int32_t covgpu_shard_plan(const covgpu_options* opt, const covgpu_problem* p, int32_t world, covgpu_nd_plan** plan_out, int32_t* lm_rank,
                                     int32_t* imu_rank, int32_t* edge_rank) {
  *plan_out = nullptr;
  if (world < 1) return 0;
  // Candidates (round 5): the tree with ONE separator of all agents at the top (its children, one region per agent, are the subtrees) and the tree with two
  // groups of agents at the top, each with the replicated top capped at 48 MiB (round 4's cap) and at 512 MiB of fronts; the cheapest by nd_shard_cost —
  // (replicated top + busiest rank's subtrees) at the flop rate of nd_plan.hip's cost model + the panel chains by its chain formula + the ring all-reduce of the top — is kept. On the corrected 5-agent map the
  // one-separator top is 3 726 unknowns = 61 % of the flops on every rank; the two-groups tree gives two ranks a 1 968-order top (10 %) and, with its two
  // second-level separators opened, four ranks a top of 45 %. COVGPU_SHARD_TREE = 0 / 1 forces the tree, COVGPU_SHARD_CAP_MIB the cap. Deterministic.
  // shard policy (options, COVGPU_SHARD_POLICY overrides for A/B runs): 0 the top replicated and all-reduced whole | 1 the top distributed — its fronts
  // stay sums over the ranks, all-reduced a panel at a time (nd_shard_assign_dist)
  int policy = opt->shard_policy;
  if (const char* e = getenv("COVGPU_SHARD_POLICY")) policy = atoi(e);
  if (policy != 0 && policy != 1) { g_err = "covgpu_shard_plan: shard_policy must be 0 or 1"; return 0; }
  covgpu_nd_plan* pl = nullptr;
  {
    const char* e_tree = getenv("COVGPU_SHARD_TREE");
    const char* e_cap = getenv("COVGPU_SHARD_CAP_MIB");
    std::vector<int> modes = e_tree ? std::vector<int>{atoi(e_tree) != 0 ? 1 : 0} : std::vector<int>{0, 1};
    std::vector<double> caps = e_cap ? std::vector<double>{atof(e_cap)} : std::vector<double>{48.0, 512.0};
    double best_cost = 0.0;
    for (int mode : modes) {
      covgpu_nd_plan* cand = nullptr;
      if (nd_plan_create_mode(opt, p, 0, &cand, mode) != COVGPU_OK) continue;
      for (double cap : caps) {
        NdHostPlan trial = cand->hp;
        if (policy == 1) nd_shard_assign_dist(trial, world, cap * 1048576.0);
        else nd_shard_assign(trial, world, cap * 1048576.0);
        if (trial.nsub == 0) continue;
        const double cost = nd_shard_cost(trial, world);
        if (pl == nullptr || cost < best_cost) {
          if (pl == nullptr) { pl = new covgpu_nd_plan(); pl->pos_kf = cand->pos_kf; }
          pl->hp = std::move(trial); best_cost = cost;
        }
      }
      delete cand;
    }
    if (pl == nullptr) return 0;
  }
  NdHostPlan& hp = pl->hp;
  const bool vi = !opt->visual_only;
  std::vector<int> perm(p->num_kf);
  for (int q = 0; q < p->num_kf; ++q) perm[pl->pos_kf[q]] = q;
  // owner of a set of variables (position-based ids): rank of the deepest node, -1 if they are all top
  auto owner = [&](std::initializer_list<int> vars) {
    int best = -1, depth = -1;
    for (int v : vars) { const int n = hp.vnode[v]; if (n >= 0 && hp.depth[n] > depth) { depth = hp.depth[n]; best = n; } }
    return best < 0 ? -1 : hp.node_rank[best];
  };
  for (int l = 0; l < p->num_lm; ++l) {
    int best = -1, depth = -1;
    for (int o = p->lm_obs_ptr[l]; o < p->lm_obs_ptr[l + 1]; ++o) {
      const int kf = p->obs_kf[o];
      if (p->kf_fixed[kf]) continue;  // (a constant keyframe has no pose unknown: it binds nobody)
      const int n = hp.vnode[2 * perm[kf]];
      if (hp.depth[n] > depth) { depth = hp.depth[n]; best = n; }
    }
    const int r = best < 0 ? -1 : hp.node_rank[best];
    lm_rank[l] = r >= 0 ? r : l % world;
  }
  for (int f = 0; f < p->num_imu; ++f) {
    const int a = perm[p->imu_kf_i[f]], b = perm[p->imu_kf_j[f]];
    const int r = vi ? owner({2 * a, 2 * a + 1, 2 * b, 2 * b + 1}) : -1;
    imu_rank[f] = r >= 0 ? r : f % world;
  }
  for (int e = 0; e < p->num_edge; ++e) {
    const int r = owner({2 * perm[p->edge_i[e]], 2 * perm[p->edge_j[e]]});
    edge_rank[e] = r >= 0 ? r : e % world;
  }
  *plan_out = pl;
  return hp.nsub;
}
extern "C" void covgpu_nd_plan_ranks(const covgpu_nd_plan* pl, int32_t* node_rank) {  // per tree node: owning rank, -1 = top (replicated); all 0 without an assignment
  for (int n = 0; n < pl->hp.nnodes; ++n) node_rank[n] = pl->hp.node_rank.empty() ? 0 : pl->hp.node_rank[n];
}
// after a sharded solve: which rank's download holds keyframe k's pose / speed-bias (-1: a top unknown — identical on every rank)
extern "C" void covgpu_nd_plan_owner(const covgpu_nd_plan* pl, int32_t* pose_rank, int32_t* sb_rank) {
  const NdHostPlan& hp = pl->hp;
  for (int q = 0; q < hp.K; ++q) {
    const int kf = pl->pos_kf[q];
    const int np = hp.vnode[2 * q], ns = hp.vnode[2 * q + 1];
    pose_rank[kf] = (np >= 0 && !hp.node_rank.empty()) ? hp.node_rank[np] : -1;
    sb_rank[kf] = (ns >= 0 && !hp.node_rank.empty()) ? hp.node_rank[ns] : -1;
  }
}

extern "C" int32_t covgpu_pgo_partition(int32_t num_kf, int32_t num_edge, const int32_t* edge_i, const int32_t* edge_j, int32_t* block_of_kf) {
  for (int k = 0; k < num_kf; ++k) block_of_kf[k] = -1;
  for (int e = 0; e < num_edge; ++e)
    if (edge_i[e] < 0 || edge_i[e] >= num_kf || edge_j[e] < 0 || edge_j[e] >= num_kf) return 0;
  PgoHostPlan hp;
  if (!pgo_plan_analyse(num_kf, num_edge, edge_i, edge_j, hp)) return 0;
  for (size_t a = 0; a < hp.block_kf.size(); ++a)
    for (int kf : hp.block_kf[a]) block_of_kf[kf] = (int32_t)a;
  return (int32_t)hp.block_kf.size();
}
