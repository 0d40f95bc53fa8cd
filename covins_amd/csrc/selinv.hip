// selinv.hip — covgpu_selected_inverse / covgpu_selected_inverse_resident (include/covgpu.h): the host side of the sweep of
// k_selinv.hip. A call linearises, builds and factors through the product's own enqueue_build / enqueue_solve (as covgpu_marginal_covariance
// does), plans the sweep on the host from the front tables the upload left in NdDev — every front's ancestor, the map of its border rows into
// the ancestor's square, the steps per level, where every requested block lies — and runs it on the context's stream behind the solve. It
// reads the factor and writes only its own scratch; nothing is kept per upload. A call is two named steps: sel_factor_and_sweep leaves Sigma in
// the scratch (covgpu_landmark_covariance, lmcov.hip, starts with the same step), the read-out copies the requested entries out of it.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "host.hpp"
#include "selinv.hpp"

using namespace covgpu;

static int bad_arg(const char* fn, const std::string& m) { g_err = std::string(fn) + ": " + m; return COVGPU_ERR_INVALID_ARG; }

namespace covgpu {

// The rule of the read-out, per pair of variables (the pose rows 0 .. 5 and the speed-bias rows 6 .. 14 of a keyframe may have different
// owners): the block lies in the square of whichever of the two owners is lower in the tree, if the other variable is in its border.
bool sel_want(const SelPlan& pl, int grow, int nrow, int gcol, int ncol, int sym, size_t out, std::vector<SelReq>& reqs) {
  const int fa = pl.gnode[grow], fb = pl.gnode[gcol];
  if (fa < 0 || fb < 0) return false;
  if (fa != fb && pl.lev_of[fa] == pl.lev_of[fb]) return false;
  reqs.push_back(SelReq{pl.lev_of[fa] <= pl.lev_of[fb] ? fa : fb, grow, nrow, gcol, ncol, sym, out, -1, 0});
  return true;
}

// A variable's rows are contiguous in a front (nd_tables lays a front out variable by variable), which the resolution checks. The position of
// a solution index in the square of front p goes through one scratch array that is filled and cleared per front.
const char* sel_locate(const covgpu_context* c, const SelPlan& pl, std::vector<SelReq>& reqs) {
  const NdDev& nd = c->nd;
  std::vector<int> pos((size_t)c->P.n, -1);
  auto fill = [&](int p, bool on) {
    for (int t = 0; t < nd.h_own_dims[p]; ++t) pos[nd.h_gidx[nd.h_own_g[p] + t]] = on ? t : -1;
    for (int t = 0; t < nd.h_st_dims[p]; ++t) pos[nd.h_gidx[nd.h_st_g[p] + t]] = on ? pl.fronts[p].nI + t : -1;
  };
  std::stable_sort(reqs.begin(), reqs.end(), [](const SelReq& a, const SelReq& b) { return a.front < b.front; });
  for (size_t i = 0; i < reqs.size();) {
    const int p = reqs[i].front;
    const SelFront& f = pl.fronts[p];
    fill(p, true);
    for (; i < reqs.size() && reqs[i].front == p; ++i) {
      SelReq& R = reqs[i];
      const int r0 = pos[R.grow], q0 = pos[R.gcol];
      if (r0 < 0 || q0 < 0) continue;
      if (pos[R.grow + R.nrow - 1] != r0 + R.nrow - 1 || pos[R.gcol + R.ncol - 1] != q0 + R.ncol - 1) { fill(p, false); return "the rows of a variable are not contiguous in a front"; }
      R.off = f.moff + (long long)r0 * f.ld + q0; R.ld = f.ld;
    }
    fill(p, false);
  }
  return nullptr;
}

namespace {
// Everything comes from the host tables of the upload: the own / border solution indices of every front (h_gidx) say who owns a border row;
// the deepest owner among a front's border rows is its ancestor p, and struct(f) \ own(p) must lie in struct(p) (the fill property).
const char* sel_plan_tree(const covgpu_context* c, SelPlan& pl) {
  const NdDev& nd = c->nd;
  const DevProblem& P = c->P;
  const int nn = nd.nnodes;
  std::vector<int>& gnode = pl.gnode; std::vector<int>& goff = pl.goff; std::vector<int>& lev_of = pl.lev_of;
  gnode.assign((size_t)P.n, -1); goff.assign((size_t)P.n, 0); lev_of.assign(nn, 0);
  for (int i = 0; i < nn; ++i)
    for (int t = 0; t < nd.h_own_dims[i]; ++t) { const int g = nd.h_gidx[nd.h_own_g[i] + t]; gnode[g] = i; goff[g] = t; }
  for (size_t l = 0; l < nd.lev.size(); ++l) for (int k = 0; k < nd.lev[l].n; ++k) lev_of[nd.lev[l].first + k] = (int)l;
  // fronts and their ancestors
  pl.fronts.resize(nn);
  std::vector<int> parent(nn, -1);
  for (int i = 0; i < nn; ++i) {
    const NdLevel& L = nd.lev[lev_of[i]];
    SelFront& f = pl.fronts[i];
    f.moff = nd.h_ntab[2 * (size_t)i]; f.ld = (int)nd.h_ntab[2 * (size_t)i + 1];
    f.linv = (long long)(L.linv_off + (size_t)(i - L.first) * L.nI * kTile);
    f.nI = L.nI; f.own = nd.h_own_dims[i]; f.st = nd.h_st_dims[i];
    f.nbo = (f.own + kSelBlock - 1) / kSelBlock;
    f.pmoff = -1; f.pld = 0; f.gmap = 0; f.pad = 0;
    if (16 * f.nbo > f.nI || f.nI + f.st > f.ld) return "a front's shape does not fit its square";
    int best = -1;
    for (int t = 0; t < f.st; ++t) {
      const int a = gnode[nd.h_gidx[nd.h_st_g[i] + t]];
      if (a < 0) return "a border row of a front has no owner";
      if (lev_of[a] <= lev_of[i]) return "the owner of a border row is not above the front";
      if (best < 0 || nd.h_ndepth[a] > nd.h_ndepth[best]) best = a;
    }
    parent[i] = best;
  }
  // position of a solution index in the square of front p, through one scratch array that is filled and cleared per front
  std::vector<int> pos((size_t)P.n, -1);
  auto fill = [&](int p, bool on) {
    for (int t = 0; t < nd.h_own_dims[p]; ++t) pos[nd.h_gidx[nd.h_own_g[p] + t]] = on ? t : -1;
    for (int t = 0; t < nd.h_st_dims[p]; ++t) pos[nd.h_gidx[nd.h_st_g[p] + t]] = on ? pl.fronts[p].nI + t : -1;
  };
  std::vector<std::vector<int>> child(nn);
  for (int i = 0; i < nn; ++i) if (parent[i] >= 0) child[parent[i]].push_back(i);
  for (int p = 0; p < nn; ++p) {
    if (child[p].empty()) continue;
    fill(p, true);
    for (int i : child[p]) {
      SelFront& f = pl.fronts[i];
      f.pmoff = pl.fronts[p].moff; f.pld = pl.fronts[p].ld; f.gmap = (int)pl.gmap.size();
      for (int t = 0; t < f.st; ++t) {
        const int w = pos[nd.h_gidx[nd.h_st_g[i] + t]];
        if (w < 0) return "a border row of a front lies outside its ancestor's square";
        pl.gmap.push_back(w);
      }
    }
    fill(p, false);
  }
  // steps: root level first; per level the gather of all its fronts, the four steps of the matrix-core form, the vector form
  for (int l = (int)nd.lev.size() - 1; l >= 0; --l) {
    const NdLevel& L = nd.lev[l];
    for (int kind = 0; kind <= 5; ++kind) {
      const int first = (int)pl.items.size();
      for (int k = 0; k < L.n; ++k) {
        const int x = L.first + k;
        const SelFront& f = pl.fronts[x];
        const bool mfma = f.own + f.st >= COVGPU_SELINV_MFMA_ROWS;
        const int nbb = (f.st + kSelBlock - 1) / kSelBlock, npan = (f.nbo + 7) / 8;
        if (kind == 0) for (int b = 0; b < nbb; ++b) pl.items.push_back(int4{x, 0, b, 0});
        else if (kind == 5) { if (!mfma) pl.items.push_back(int4{x, 5, 0, 0}); }
        else if (!mfma) continue;
        else if (kind == 1) for (int g = 0; g < (f.nbo + 3) / 4; ++g) pl.items.push_back(int4{x, 1, g, 0});
        else if (kind == 4) { for (int b = 0; b < f.nbo; ++b) for (int p = 0; 8 * p <= b; ++p) pl.items.push_back(int4{x, 4, b, p}); }
        else for (int b = 0; b < nbb; ++b) for (int p = 0; p < npan; ++p) pl.items.push_back(int4{x, kind, b, p});
      }
      const int count = (int)pl.items.size() - first;
      if (count > 0) pl.launches.push_back(SelLaunch{first, count, kind});
    }
  }
  return nullptr;
}
}  // namespace

// read-out of the keyframes' diagonal blocks and of the requested pairs, per pair of variables
const char* sel_plan_readout(const covgpu_context* c, const covgpu_selinv_t* rq, const uint8_t* fixed, SelPlan& pl) {
  const DevProblem& P = c->P;
  const int D = P.D, d = rq->block ? D : 6, K = P.K;
  pl.d = d;
  const int64_t np = rq->num_pairs;
  const size_t dd = (size_t)d * d;
  pl.src.assign(((size_t)K + (size_t)np) * dd, -1);
  pl.pair_ok.assign((size_t)np, 1);
  pl.served = 0;
  std::vector<SelReq> reqs;   // sym: a diagonal block's part, stored at both places
  const int nparts = d > 6 ? 2 : 1, part0[2] = {0, 6}, partn[2] = {6, d - 6};
  auto want = [&](int ki, int a, int kj, int b, int sym, size_t base) -> bool {
    return sel_want(pl, D * ki + part0[a], partn[a], D * kj + part0[b], partn[b], sym, base + (size_t)part0[a] * d + part0[b], reqs);
  };
  for (int k = 0; k < K; ++k) {
    if (fixed[k]) continue;
    for (int a = 0; a < nparts; ++a)
      for (int b = 0; b <= a; ++b)   // one triangle, stored twice
        if (!want(k, a, k, b, 1, (size_t)k * dd)) return "an unknown of a free keyframe has no front";
  }
  for (int64_t e = 0; e < np; ++e)
    for (int a = 0; a < nparts && pl.pair_ok[e]; ++a)
      for (int b = 0; b < nparts; ++b)
        if (!want(rq->pair_i[e], a, rq->pair_j[e], b, 0, ((size_t)K + (size_t)e) * dd)) { pl.pair_ok[e] = 0; break; }
  if (const char* e = sel_locate(c, pl, reqs)) return e;
  for (const SelReq& R : reqs) {
    if (R.off < 0) continue;
    for (int r = 0; r < R.nrow; ++r)
      for (int q = 0; q < (R.sym && R.grow == R.gcol ? r + 1 : R.ncol); ++q) {
        const long long s = R.off + (long long)r * R.ld + q;
        pl.src[R.out + (size_t)r * d + q] = s;
        if (R.sym) pl.src[R.out - (size_t)(R.grow - R.gcol) * d + (R.grow - R.gcol) + (size_t)q * d + r] = s;
      }
  }
  for (int k = 0; k < K; ++k)
    if (!fixed[k]) for (size_t e = 0; e < dd; ++e) if (pl.src[(size_t)k * dd + e] < 0) return "a diagonal block of a keyframe lies off the structure of L";
  for (int64_t e = 0; e < np; ++e) {
    long long* s = pl.src.data() + ((size_t)K + (size_t)e) * dd;
    for (size_t t = 0; t < dd && pl.pair_ok[e]; ++t) if (s[t] < 0) pl.pair_ok[e] = 0;
    if (!pl.pair_ok[e]) std::fill(s, s + dd, -1ll);
    pl.served += pl.pair_ok[e];
  }
  return nullptr;
}

int sel_context_check(const char* fn, const covgpu_context* c) {
  if (c->sharded) return bad_arg(fn, "a sharded context holds one rank's share of the factor");
  if (!c->have) return bad_arg(fn, "no problem uploaded");
  if (!c->P.nd) return bad_arg(fn, "the pose graph of this context is off the elimination tree (COVGPU_PGO_ND=0)");
  return COVGPU_OK;
}

// plan and scratch first (an allocation that fails leaves nothing enqueued), then linearise at the resident estimate, build and factor at mu
// (the steps of covgpu_gn_step behind its upload), then the sweep
int sel_factor_and_sweep(const char* fn, covgpu_context* c, double mu, DeviceScratch& U, SelSweep& sw, const std::function<int(SelPlan&)>& prepare) {
  SelPlan& pl = sw.pl;
  if (const char* e = sel_plan_tree(c, pl)) { g_err = std::string(fn) + ": " + e; return COVGPU_ERR_INVALID_ARG; }
  const size_t mel = c->nd.M_elems;
  SelArgs& a = sw.a;
  a.M = c->P.nd_M; a.Linv = c->P.nd_Linv;
  SelFront* fr = nullptr; int* gmap = nullptr; int4* items = nullptr;
  HIPCHK(U.alloc(&a.S, mel)); HIPCHK(U.alloc(&a.X, mel));
  HIPCHK(U.alloc(&fr, pl.fronts.size())); HIPCHK(U.alloc(&gmap, pl.gmap.size())); HIPCHK(U.alloc(&items, pl.items.size()));
  a.fr = fr; a.gmap = gmap; a.items = items;
  sw.bytes = 2 * mel * sizeof(double) + pl.fronts.size() * sizeof(SelFront) + pl.items.size() * sizeof(int4) + pl.gmap.size() * sizeof(int);
  RC(prepare(pl));

  launch_preintegrate(c->P, c->st);
  enqueue_build(c, mu);
  enqueue_solve(c, c->P.gn);
  RC(read_scalars(c));
  if (chol_failed(c)) { g_err = std::string(fn) + ": reduced system is not positive definite"; return COVGPU_ERR_NUMERIC; }

  HIPCHK(hipMemsetAsync(a.S, 0, mel * sizeof(double), c->st)); HIPCHK(hipMemsetAsync(a.X, 0, mel * sizeof(double), c->st));
  HIPCHK(hipMemcpyAsync(fr, pl.fronts.data(), pl.fronts.size() * sizeof(SelFront), hipMemcpyHostToDevice, c->st));
  if (!pl.gmap.empty()) HIPCHK(hipMemcpyAsync(gmap, pl.gmap.data(), pl.gmap.size() * sizeof(int), hipMemcpyHostToDevice, c->st));
  HIPCHK(hipMemcpyAsync(items, pl.items.data(), pl.items.size() * sizeof(int4), hipMemcpyHostToDevice, c->st));
  for (const SelLaunch& L : pl.launches) {
    if (L.kind == 0) { launch_selinv_gather(a, L.first, L.count, c->st); ++sw.n_gather; }
    else { launch_selinv_step(a, L.first, L.count, L.kind, c->st); ++(L.kind == 5 ? sw.n_vec : sw.n_mfma); }
  }
  return COVGPU_OK;
}

int sel_read_out(covgpu_context* c, const SelSweep& sw, long long* src, double* out) {
  const size_t nout = sw.pl.src.size();
  HIPCHK(hipMemcpyAsync(src, sw.pl.src.data(), nout * sizeof(long long), hipMemcpyHostToDevice, c->st));
  launch_selinv_read(sw.a.S, src, out, (long long)nout, c->st);
  return COVGPU_OK;
}

int sel_fetch_fixed(covgpu_context* c, std::vector<uint8_t>& fixed) {
  fixed.assign((size_t)std::max(c->P.K, 1), 0);
  HIPCHK(hipMemcpy(fixed.data(), c->P.fixed, (size_t)c->P.K, hipMemcpyDeviceToHost));
  return COVGPU_OK;
}

}  // namespace covgpu

namespace {

// the two steps of a call: Sigma into the sweep's scratch (with the read-out table planned and allocated before anything is enqueued), the read-out
int factor_and_sweep(const char* fn, covgpu_context* c, const covgpu_selinv_t* rq, const uint8_t* fixed) {
  DeviceScratch U(c->st);
  SelSweep sw;
  long long* src = nullptr; double* out = nullptr;
  RC(sel_factor_and_sweep(fn, c, rq->mu, U, sw, [&](SelPlan& pl) -> int {
    if (const char* e = sel_plan_readout(c, rq, fixed, pl)) { g_err = std::string(fn) + ": " + e; return COVGPU_ERR_INVALID_ARG; }
    HIPCHK(U.alloc(&src, pl.src.size())); HIPCHK(U.alloc(&out, pl.src.size()));
    return COVGPU_OK;
  }));
  const SelPlan& pl = sw.pl;
  const size_t kel = (size_t)c->P.K * pl.d * pl.d, nout = pl.src.size();
  RC(sel_read_out(c, sw, src, out));
  HIPCHK(U.fetch(rq->kf_cov, (const double*)out, kel));
  HIPCHK(U.fetch(rq->pair_cov, (const double*)(out + kel), nout - kel));
  HIPCHK(hipStreamSynchronize(c->st));
  HIPCHK(hipGetLastError());
  if (rq->num_pairs > 0) std::memcpy(rq->pair_ok, pl.pair_ok.data(), (size_t)rq->num_pairs);
  if (rq->stats) {
    int64_t* s = rq->stats;
    s[0] = (int64_t)pl.fronts.size(); s[1] = (int64_t)c->nd.lev.size(); s[2] = sw.n_mfma + sw.n_vec + sw.n_gather + 1; s[3] = sw.n_mfma; s[4] = sw.n_vec;
    s[5] = (int64_t)(sw.bytes + nout * sizeof(double) + nout * sizeof(long long));
    s[6] = pl.served; s[7] = 0;
  }
  return COVGPU_OK;
}

int inverse_impl(covgpu_context* c, const covgpu_options* opt, const covgpu_problem* p, int pgo, const covgpu_selinv_t* rq) {
  const char* fn = "covgpu_selected_inverse";
  if (const char* e = selinv_check(p, opt, rq)) return bad_arg(fn, e);
  if (c->sharded) return bad_arg(fn, "a sharded context holds one rank's share of the factor");
  RC(upload_impl(c, opt, p, pgo != 0));
  RC(sel_context_check(fn, c));
  RC(reset_state(c));
  std::vector<uint8_t> fixed;
  RC(sel_fetch_fixed(c, fixed));
  return factor_and_sweep(fn, c, rq, fixed.data());
}

int resident_impl(covgpu_context* c, const covgpu_options* opt, const covgpu_selinv_t* rq) {
  const char* fn = "covgpu_selected_inverse_resident";
  if (!opt) return bad_arg(fn, "NULL options");
  RC(sel_context_check(fn, c));
  HIPCHK(hipSetDevice(c->device));
  std::vector<uint8_t> fixed;
  RC(sel_fetch_fixed(c, fixed));
  if (const char* e = selinv_request_check(c->P.K, fixed.data(), rq)) return bad_arg(fn, e);
  c->P.reproj_loss_a = opt->reproj_loss_a;   // (as every solve of the resident problem takes it)
  if (!c->state_set) RC(reset_state(c));     // an upload alone: the estimate is the uploaded one
  return factor_and_sweep(fn, c, rq, fixed.data());
}

}  // namespace

extern "C" void covgpu_selinv_limits(int32_t out[4]) {
  out[0] = COVGPU_SELINV_MFMA_ROWS; out[1] = kSelPanel; out[2] = kSelBlock; out[3] = 0;
}
extern "C" int covgpu_selinv_check(const covgpu_problem* p, const covgpu_options* o, const covgpu_selinv_t* s) {
  return check_export("covgpu_selinv_check", [&] { return selinv_check(p, o, s); });
}
extern "C" int covgpu_selected_inverse(covgpu_context* c, const covgpu_options* opt, const covgpu_problem* p, int32_t pgo, const covgpu_selinv_t* rq) {
  if (!c) { g_err = "covgpu_selected_inverse: NULL context"; return COVGPU_ERR_INVALID_ARG; }
  return guarded([&] { return inverse_impl(c, opt, p, pgo, rq); });
}
extern "C" int covgpu_selected_inverse_resident(covgpu_context* c, const covgpu_options* opt, const covgpu_selinv_t* rq) {
  if (!c) { g_err = "covgpu_selected_inverse_resident: NULL context"; return COVGPU_ERR_INVALID_ARG; }
  return guarded([&] { return resident_impl(c, opt, rq); });
}
