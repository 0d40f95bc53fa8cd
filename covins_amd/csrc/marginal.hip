// marginal.hip — covgpu_marginal_covariance / covgpu_marginal_resident (include/covgpu.h): the host side of the sweep of
// k_marginal.hip. A call linearises, builds and factors through the product's own enqueue_build / enqueue_solve (as covgpu_gn_step does), then
// plans the sweep on the host from the front tables the upload left in NdDev — which fronts lie on the paths, the order of the columns, the
// working matrix, the steps — and runs it on the context's stream behind the solve. It reads the factor and writes only its own scratch.
#include <algorithm>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "host.hpp"
#include "marginal.hpp"

using namespace covgpu;

namespace {

struct MargLaunch { int first, count; bool mfma; };
struct MargPlan {
  int m = 0, mp = 0, rows = 0;
  std::vector<MargFront> fronts;     // level order (= the order of the Gram sums)
  std::vector<int> bmap, seed_row, perm;
  std::vector<int4> items;
  std::vector<MargLaunch> launches;  // stream order
};

// The fronts that a unit column of the chosen unknowns reaches, the columns in the post-order of their owners, and the steps. Everything comes
// from the host tables of the upload: the own / border solution indices of every front (h_gidx) say who owns a border row, the deepest owner
// among a front's border rows is the next front on its path (the front's parent in the tree, or the first ancestor it couples to).
const char* marg_plan(const covgpu_context* c, const covgpu_marginal_t* mg, MargPlan& pl) {
  const NdDev& nd = c->nd;
  const DevProblem& P = c->P;
  const int D = P.D, d = mg->block ? D : 6, q = mg->num_kf, nn = nd.nnodes;
  pl.m = q * d; pl.mp = ((pl.m + kMargBlock - 1) / kMargBlock) * kMargBlock;
  std::vector<int> gnode((size_t)P.n, -1), goff((size_t)P.n, 0);
  for (int i = 0; i < nn; ++i)
    for (int t = 0; t < nd.h_own_dims[i]; ++t) { const int g = nd.h_gidx[nd.h_own_g[i] + t]; gnode[g] = i; goff[g] = t; }
  std::vector<int> col_g(pl.m);
  for (int t = 0; t < q; ++t) for (int r = 0; r < d; ++r) col_g[t * d + r] = D * mg->kf[t] + r;
  for (int g : col_g) if (gnode[g] < 0) return "an unknown of the selection has no front";
  // visited fronts: closed under "owner of a border row"
  std::vector<char> vis(nn, 0);
  std::vector<int> eparent(nn, -1), stack;
  for (int g : col_g) if (!vis[gnode[g]]) { vis[gnode[g]] = 1; stack.push_back(gnode[g]); }
  while (!stack.empty()) {
    const int i = stack.back(); stack.pop_back();
    int best = -1;
    for (int t = 0; t < nd.h_st_dims[i]; ++t) {
      const int a = gnode[nd.h_gidx[nd.h_st_g[i] + t]];
      if (a < 0) return "a border row of a front has no owner";
      if (best < 0 || nd.h_ndepth[a] > nd.h_ndepth[best]) best = a;
      if (!vis[a]) { vis[a] = 1; stack.push_back(a); }
    }
    eparent[i] = best;
  }
  // the forest of the visited fronts, children in front order, and the columns in its post-order
  std::vector<std::vector<int>> child(nn), cols_of(nn);
  std::vector<int> roots, c0(nn, 0), c1(nn, 0);
  for (int i = 0; i < nn; ++i) if (vis[i]) { if (eparent[i] >= 0) child[eparent[i]].push_back(i); else roots.push_back(i); }
  for (int j = 0; j < pl.m; ++j) cols_of[gnode[col_g[j]]].push_back(j);
  pl.perm.clear(); pl.perm.reserve(pl.m);
  std::function<void(int)> dfs = [&](int i) {
    c0[i] = (int)pl.perm.size();
    for (int ch : child[i]) dfs(ch);
    for (int j : cols_of[i]) pl.perm.push_back(j);
    c1[i] = (int)pl.perm.size();
  };
  for (int r : roots) dfs(r);
  if ((int)pl.perm.size() != pl.m) return "the paths of the selection do not form a forest";
  // fronts (ids are in level order), the working matrix's rows, the border maps
  std::vector<int> fid(nn, -1), wrow((size_t)P.n, -1), lev_of(nn, 0);
  for (size_t l = 0; l < nd.lev.size(); ++l) for (int k = 0; k < nd.lev[l].n; ++k) lev_of[nd.lev[l].first + k] = (int)l;
  int rows = 0;
  for (int i = 0; i < nn; ++i) {
    if (!vis[i] || c1[i] == c0[i]) continue;
    const NdLevel& L = nd.lev[lev_of[i]];
    MargFront f;
    f.moff = nd.h_ntab[2 * (size_t)i]; f.ld = (int)nd.h_ntab[2 * (size_t)i + 1];
    f.linv = (long long)(L.linv_off + (size_t)(i - L.first) * L.nI * kTile);
    f.nI = L.nI; f.own = nd.h_own_dims[i]; f.st = nd.h_st_dims[i];
    f.nbo = (f.own + kMargBlock - 1) / kMargBlock; f.wbase = rows;
    f.c0 = c0[i]; f.c1 = c1[i]; f.bmap = 0; f.pad = 0;
    for (int t = 0; t < f.own; ++t) wrow[nd.h_gidx[nd.h_own_g[i] + t]] = rows + t;
    rows += kMargBlock * f.nbo;
    fid[i] = (int)pl.fronts.size();
    pl.fronts.push_back(f);
  }
  pl.rows = rows;
  for (int i = 0; i < nn; ++i) {
    if (fid[i] < 0) continue;
    MargFront& f = pl.fronts[fid[i]];
    f.bmap = (int)pl.bmap.size();
    for (int t = 0; t < f.st; ++t) {
      const int w = wrow[nd.h_gidx[nd.h_st_g[i] + t]];
      if (w < 0) return "a border row of a visited front lies outside the working matrix";
      const int a = gnode[nd.h_gidx[nd.h_st_g[i] + t]];   // its owner works on every column this front hands it
      if (c0[a] > f.c0 || c1[a] < f.c1) return "the owner of a border row is not on the front's path";
      pl.bmap.push_back(w);
    }
  }
  pl.seed_row.resize(pl.m);
  for (int s = 0; s < pl.m; ++s) pl.seed_row[s] = wrow[col_g[pl.perm[s]]];
  // steps: per level, per panel: the panels' own rows, then the rows below — each in the matrix-core form and in the vector form
  for (size_t l = 0; l < nd.lev.size(); ++l) {
    const NdLevel& L = nd.lev[l];
    int maxp = 0;
    for (int k = 0; k < L.n; ++k) if (fid[L.first + k] >= 0) maxp = std::max(maxp, (pl.fronts[fid[L.first + k]].nbo + 7) / 8);
    for (int p = 0; p < maxp; ++p)
      for (int phase = 0; phase < 2; ++phase)
        for (int form = 0; form < 2; ++form) {   // form 0: matrix cores
          const int first = (int)pl.items.size();
          for (int k = 0; k < L.n; ++k) {
            const int x = fid[L.first + k];
            if (x < 0) continue;
            const MargFront& f = pl.fronts[x];
            if (8 * p >= f.nbo || ((f.c1 - f.c0 >= COVGPU_MARGINAL_MFMA_COLS) != (form == 0))) continue;
            if (phase == 0) pl.items.push_back(int4{x, p, 0, 0});
            else {
              for (int b = 8 * p + 8; b < f.nbo; ++b) pl.items.push_back(int4{x, p, 1, b});
              for (int b = 0; b < (f.st + kMargBlock - 1) / kMargBlock; ++b) pl.items.push_back(int4{x, p, 2, b});
            }
          }
          const int count = (int)pl.items.size() - first;
          if (count > 0) pl.launches.push_back(MargLaunch{first, count, form == 0});
        }
  }
  return nullptr;
}

int bad_arg(const char* fn, const std::string& m) { g_err = std::string(fn) + ": " + m; return COVGPU_ERR_INVALID_ARG; }

// the refusals that depend on the context: the sweep reads the fronts of ONE device's elimination tree
int context_check(const char* fn, const covgpu_context* c) {
  if (c->sharded) return bad_arg(fn, "a sharded context holds one rank's share of the factor");
  if (!c->have) return bad_arg(fn, "no problem uploaded");
  if (!c->P.nd) return bad_arg(fn, "the pose graph of this context is off the elimination tree (COVGPU_PGO_ND=0)");
  return COVGPU_OK;
}

// linearise at the resident estimate, build and factor at mu (the steps of covgpu_gn_step behind its upload), then the sweep
int factor_and_sweep(const char* fn, covgpu_context* c, const covgpu_marginal_t* mg) {
  launch_preintegrate(c->P, c->st);
  enqueue_build(c, mg->mu);
  enqueue_solve(c, c->P.gn);
  RC(read_scalars(c));
  if (chol_failed(c)) { g_err = std::string(fn) + ": reduced system is not positive definite"; return COVGPU_ERR_NUMERIC; }
  MargPlan pl;
  if (const char* e = marg_plan(c, mg, pl)) { g_err = std::string(fn) + ": " + e; return COVGPU_ERR_INVALID_ARG; }
  const size_t wel = (size_t)pl.rows * pl.mp, cel = (size_t)pl.m * pl.m;
  DeviceScratch U(c->st);
  MargArgs a;
  a.M = c->P.nd_M; a.Linv = c->P.nd_Linv; a.mp = pl.mp;
  int *seed = nullptr, *perm = nullptr; double* cov = nullptr;
  HIPCHK(U.zeroed(&a.W, wel));
  HIPCHK(U.upload(&a.fr, pl.fronts.data(), pl.fronts.size())); HIPCHK(U.upload(&a.bmap, pl.bmap.data(), pl.bmap.size()));
  HIPCHK(U.upload(&a.items, pl.items.data(), pl.items.size()));
  HIPCHK(U.upload(&seed, pl.seed_row.data(), pl.seed_row.size())); HIPCHK(U.upload(&perm, pl.perm.data(), pl.perm.size()));
  HIPCHK(U.alloc(&cov, cel));
  launch_marg_seed(a.W, pl.mp, pl.m, seed, c->st);
  long long n_mfma = 0, n_vec = 0;
  for (const MargLaunch& L : pl.launches) { launch_marg_step(a, L.first, L.count, L.mfma, c->st); ++(L.mfma ? n_mfma : n_vec); }
  launch_marg_gram(a.W, pl.mp, a.fr, (int)pl.fronts.size(), perm, pl.m, cov, c->st);
  HIPCHK(U.fetch(mg->cov, (const double*)cov, cel));
  HIPCHK(hipStreamSynchronize(c->st));
  HIPCHK(hipGetLastError());
  if (mg->stats) {
    int64_t* s = mg->stats;
    s[0] = pl.m; s[1] = (int64_t)pl.fronts.size(); s[2] = n_mfma + n_vec + 2; s[3] = n_mfma; s[4] = n_vec;
    s[5] = (int64_t)((wel + cel) * sizeof(double) + pl.fronts.size() * sizeof(MargFront) + pl.items.size() * sizeof(int4) +
                     (pl.bmap.size() + pl.seed_row.size() + pl.perm.size()) * sizeof(int));
    s[6] = s[7] = 0;
  }
  return COVGPU_OK;
}

int covariance_impl(covgpu_context* c, const covgpu_options* opt, const covgpu_problem* p, int pgo, const covgpu_marginal_t* mg) {
  const char* fn = "covgpu_marginal_covariance";
  if (const char* e = marginal_check(p, opt, mg)) return bad_arg(fn, e);
  if (c->sharded) return bad_arg(fn, "a sharded context holds one rank's share of the factor");
  RC(upload_impl(c, opt, p, pgo != 0));
  RC(context_check(fn, c));
  RC(reset_state(c));
  return factor_and_sweep(fn, c, mg);
}

int resident_impl(covgpu_context* c, const covgpu_options* opt, const covgpu_marginal_t* mg) {
  const char* fn = "covgpu_marginal_resident";
  if (!opt) return bad_arg(fn, "NULL options");
  RC(context_check(fn, c));
  HIPCHK(hipSetDevice(c->device));
  std::vector<uint8_t> fixed((size_t)std::max(c->P.K, 1), 0);
  HIPCHK(hipMemcpy(fixed.data(), c->P.fixed, (size_t)c->P.K, hipMemcpyDeviceToHost));
  if (const char* e = marginal_selection_check(c->P.K, fixed.data(), mg)) return bad_arg(fn, e);
  c->P.reproj_loss_a = opt->reproj_loss_a;   // (as every solve of the resident problem takes it)
  if (!c->state_set) RC(reset_state(c));     // an upload alone: the estimate is the uploaded one
  return factor_and_sweep(fn, c, mg);
}

}  // namespace

extern "C" void covgpu_marginal_limits(int32_t out[4]) {
  out[0] = COVGPU_MARGINAL_MAX_KF; out[1] = COVGPU_MARGINAL_MAX_COLS; out[2] = COVGPU_MARGINAL_MFMA_COLS; out[3] = kMargPanel;
}
extern "C" int covgpu_marginal_check(const covgpu_problem* p, const covgpu_options* o, const covgpu_marginal_t* m) {
  return check_export("covgpu_marginal_check", [&] { return marginal_check(p, o, m); });
}
extern "C" int covgpu_marginal_covariance(covgpu_context* c, const covgpu_options* opt, const covgpu_problem* p, int32_t pgo, const covgpu_marginal_t* mg) {
  if (!c) { g_err = "covgpu_marginal_covariance: NULL context"; return COVGPU_ERR_INVALID_ARG; }
  return guarded([&] { return covariance_impl(c, opt, p, pgo, mg); });
}
extern "C" int covgpu_marginal_resident(covgpu_context* c, const covgpu_options* opt, const covgpu_marginal_t* mg) {
  if (!c) { g_err = "covgpu_marginal_resident: NULL context"; return COVGPU_ERR_INVALID_ARG; }
  return guarded([&] { return resident_impl(c, opt, mg); });
}
