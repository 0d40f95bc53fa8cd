// lmcov.hip — covgpu_landmark_covariance / covgpu_landmark_covariance_resident (include/covgpu.h): the host side of the
// landmark pass of k_lmcov.hip. A call starts with step one of covgpu_selected_inverse (selinv.hip: sel_factor_and_sweep leaves Sigma in its
// scratch), with its own plan and scratch made before anything is enqueued: where the 6x6 pose-pose block of Sigma lies for every entry of
// the resident covisible pair list and for every free keyframe. The blocks are found by the rule of the selected inverse's read-out
// (sel_want / sel_locate); nothing is kept per upload. The tables and the context's refusals are exported through lmcov.hpp: the
// observation pass (obscov.hip) runs on the same ones.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "host.hpp"
#include "lmcov.hpp"
#include "selinv.hpp"

using namespace covgpu;

namespace {

int bad_arg(const char* fn, const std::string& m) { g_err = std::string(fn) + ": " + m; return COVGPU_ERR_INVALID_ARG; }

// The tables of the landmark pass. Two numberings meet: sel_want / sel_locate work in SOLUTION indices (D * keyframe of the problem + component),
// the covisible pair list (pair_i, pair_j) in chain-major POSITIONS (perm[keyframe]).
const char* lmcov_plan(const covgpu_context* c, const SelPlan& pl, LmcovTables& lp) {
  const int K = c->P.K, D = c->P.D;
  const uint8_t* fixed = lp.fixed.data();
  const std::vector<int>&pair_i = lp.pair_i, &pair_j = lp.pair_j, &pos_kf = lp.pos_kf;
  const size_t np = pair_i.size();
  lp.kf_blk.assign((size_t)K, LmcovBlock{-1, 0, 0});
  lp.pair_blk.assign(np, LmcovBlock{-1, 0, 0});
  lp.row_ptr.assign((size_t)K + 1, 0);
  std::vector<SelReq> reqs;   // out: keyframe k -> k, pair entry e -> K + e; only the pose variable (rows 0 .. 5) of a keyframe is involved
  for (int k = 0; k < K; ++k)
    if (!fixed[k] && !sel_want(pl, D * k, 6, D * k, 6, 1, (size_t)k, reqs)) return "the pose of a free keyframe has no front";
  for (size_t e = 0; e < np; ++e) {
    const int pi = pair_i[e], pj = pair_j[e];
    if (pi < 0 || pi >= K || pj < 0 || pj >= pi) return "the covisible pair list is not in chain-major positions i > j";
    if (e > 0 && (pair_i[e - 1] > pi || (pair_i[e - 1] == pi && pair_j[e - 1] >= pj))) return "the covisible pair list is not sorted";
    const int ki = pos_kf[pi], kj = pos_kf[pj];
    if (fixed[ki] || fixed[kj]) return "a keyframe with a constant pose in the covisible pair list";
    if (!sel_want(pl, D * ki, 6, D * kj, 6, 0, (size_t)K + e, reqs)) return "a covisible pair of free keyframes lies off the structure of L";
    ++lp.row_ptr[(size_t)pi + 1];
  }
  for (int i = 0; i < K; ++i) lp.row_ptr[(size_t)i + 1] += lp.row_ptr[i];
  if (const char* m = sel_locate(c, pl, reqs)) return m;
  for (const SelReq& R : reqs) (R.out < (size_t)K ? lp.kf_blk[R.out] : lp.pair_blk[R.out - K]) = LmcovBlock{R.off, R.ld, 0};
  for (int k = 0; k < K; ++k) if (!fixed[k] && lp.kf_blk[k].off < 0) return "a diagonal block of a keyframe lies off the structure of L";
  for (size_t e = 0; e < np; ++e) if (lp.pair_blk[e].off < 0) return "a covisible pair of free keyframes lies off the structure of L";
  return nullptr;
}

}  // namespace

namespace covgpu {

int lmcov_lists(const char* fn, covgpu_context* c, LmcovTables& t) {
  const DevProblem& P = c->P;
  const int K = P.K;
  RC(sel_fetch_fixed(c, t.fixed));
  t.pair_i.assign((size_t)P.npairs, 0); t.pair_j.assign((size_t)P.npairs, 0); t.pos_kf.assign((size_t)K, 0);
  if (P.npairs > 0) {
    HIPCHK(hipMemcpy(t.pair_i.data(), P.pair_i, (size_t)P.npairs * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(t.pair_j.data(), P.pair_j, (size_t)P.npairs * sizeof(int), hipMemcpyDeviceToHost));
  }
  if ((int)c->h_perm.size() != K) return bad_arg(fn, "the context holds no chain-major order");
  for (int k = 0; k < K; ++k) {
    if (c->h_perm[k] < 0 || c->h_perm[k] >= K) return bad_arg(fn, "the chain-major order is not a permutation");
    t.pos_kf[c->h_perm[k]] = k;
  }
  return COVGPU_OK;
}

int lmcov_prepare(const char* fn, const covgpu_context* c, const SelPlan& pl, ::DeviceScratch& U, LmcovTables& t, size_t& bytes) {
  const int L = c->P.L;
  if (const char* m = lmcov_plan(c, pl, t)) return bad_arg(fn, m);
  HIPCHK(U.alloc(&t.d_kf, t.kf_blk.size())); HIPCHK(U.alloc(&t.d_pair, t.pair_blk.size())); HIPCHK(U.alloc(&t.d_row, t.row_ptr.size()));
  HIPCHK(U.alloc(&t.d_lm_cov, (size_t)9 * L)); HIPCHK(U.alloc(&t.d_lm_ok, (size_t)L));
  bytes += (t.kf_blk.size() + t.pair_blk.size()) * sizeof(LmcovBlock) + t.row_ptr.size() * sizeof(int) + (size_t)L * (9 * sizeof(double) + 1);
  return COVGPU_OK;
}

int lmcov_upload(covgpu_context* c, const LmcovTables& t, LmcovArgs& a) {
  HIPCHK(hipMemcpyAsync(t.d_kf, t.kf_blk.data(), t.kf_blk.size() * sizeof(LmcovBlock), hipMemcpyHostToDevice, c->st));
  if (!t.pair_blk.empty()) HIPCHK(hipMemcpyAsync(t.d_pair, t.pair_blk.data(), t.pair_blk.size() * sizeof(LmcovBlock), hipMemcpyHostToDevice, c->st));
  HIPCHK(hipMemcpyAsync(t.d_row, t.row_ptr.data(), t.row_ptr.size() * sizeof(int), hipMemcpyHostToDevice, c->st));
  a.kf_blk = t.d_kf; a.pair_blk = t.d_pair; a.row_ptr = t.d_row; a.lm_cov = t.d_lm_cov; a.lm_ok = t.d_lm_ok;
  return COVGPU_OK;
}

// the refusals that depend on the context
int lmcov_context_check(const char* fn, const covgpu_context* c) {
  if (c->sharded) return bad_arg(fn, "a sharded context holds one rank's share of the factor");
  if (!c->have && !c->second_round) return bad_arg(fn, "no problem uploaded");   // (second_round: what covgpu_gba_two_round left, host.hpp)
  if (c->pgo) return bad_arg(fn, "the context holds a pose graph: it has no landmarks");
  if (!c->P.nd) return bad_arg(fn, "the problem of this context is off the elimination tree");
  if (c->P.L <= 0 || c->P.O <= 0) return bad_arg(fn, "a problem without landmarks");
  return COVGPU_OK;
}

}  // namespace covgpu

namespace {

int sweep_and_pass(const char* fn, covgpu_context* c, const covgpu_lmcov_t* rq) {
  const DevProblem& P = c->P;
  const int L = P.L;
  LmcovTables lp;
  RC(lmcov_lists(fn, c, lp));

  DeviceScratch U(c->st);
  SelSweep sw;
  LmcovArgs a{};
  long long* src = nullptr; double* kf_out = nullptr;
  size_t own_bytes = 0;
  covgpu_selinv_t diag{};   // the read-out of kf_cov: the pose diagonal blocks as covgpu_selected_inverse at block 0 returns them
  diag.block = 0; diag.mu = rq->mu; diag.kf_cov = rq->kf_cov; diag.num_pairs = 0;
  RC(sel_factor_and_sweep(fn, c, rq->mu, U, sw, [&](SelPlan& pl) -> int {
    RC(lmcov_prepare(fn, c, pl, U, lp, own_bytes));
    if (rq->kf_cov) {
      if (const char* m = sel_plan_readout(c, &diag, lp.fixed.data(), pl)) return bad_arg(fn, m);
      HIPCHK(U.alloc(&src, pl.src.size())); HIPCHK(U.alloc(&kf_out, pl.src.size()));
      own_bytes += pl.src.size() * (sizeof(long long) + sizeof(double));
    }
    return COVGPU_OK;
  }));
  RC(lmcov_upload(c, lp, a));
  a.S = sw.a.S;
  launch_lmcov(P, a, c->st);
  if (rq->kf_cov) {
    RC(sel_read_out(c, sw, src, kf_out));
    HIPCHK(U.fetch(rq->kf_cov, (const double*)kf_out, sw.pl.src.size()));
  }
  HIPCHK(U.fetch(rq->lm_cov, (const double*)a.lm_cov, (size_t)9 * L));
  HIPCHK(U.fetch(rq->lm_ok, (const uint8_t*)a.lm_ok, (size_t)L));
  HIPCHK(hipStreamSynchronize(c->st));
  HIPCHK(hipGetLastError());
  if (rq->stats) {
    int64_t* s = rq->stats;
    int64_t bad = 0;
    for (int l = 0; l < L; ++l) bad += rq->lm_ok[l] ? 0 : 1;
    s[0] = (int64_t)sw.pl.fronts.size(); s[1] = (int64_t)c->nd.lev.size(); s[2] = sw.n_mfma + sw.n_vec + sw.n_gather + (rq->kf_cov ? 1 : 0); s[3] = 1;
    s[4] = P.lm_group == 4 || P.lm_group == 8 ? P.lm_group : 16;
    s[5] = (int64_t)(sw.bytes + own_bytes); s[6] = (int64_t)lp.pair_blk.size(); s[7] = bad;
  }
  return COVGPU_OK;
}

int context_check(const char* fn, const covgpu_context* c) { return lmcov_context_check(fn, c); }

int covariance_impl(covgpu_context* c, const covgpu_options* opt, const covgpu_problem* p, const covgpu_lmcov_t* rq) {
  const char* fn = "covgpu_landmark_covariance";
  if (const char* e = lmcov_check(p, opt, rq)) return bad_arg(fn, e);
  if (c->sharded) return bad_arg(fn, "a sharded context holds one rank's share of the factor");
  RC(upload_impl(c, opt, p, false));
  RC(context_check(fn, c));
  RC(reset_state(c));
  return sweep_and_pass(fn, c, rq);
}

int resident_impl(covgpu_context* c, const covgpu_options* opt, const covgpu_lmcov_t* rq) {
  const char* fn = "covgpu_landmark_covariance_resident";
  if (!opt) return bad_arg(fn, "NULL options");
  if (const char* e = lmcov_request_check(rq)) return bad_arg(fn, e);
  RC(context_check(fn, c));
  HIPCHK(hipSetDevice(c->device));
  c->P.reproj_loss_a = opt->reproj_loss_a;   // (as every solve of the resident problem takes it)
  if (!c->state_set) RC(reset_state(c));     // an upload alone: the estimate is the uploaded one
  return sweep_and_pass(fn, c, rq);
}

}  // namespace

extern "C" void covgpu_lmcov_limits(int32_t out[4]) {
  out[0] = kLmcovMaxGroup; out[1] = kLmcovThreads; out[2] = 9; out[3] = 0;
}
extern "C" int covgpu_lmcov_check(const covgpu_problem* p, const covgpu_options* o, const covgpu_lmcov_t* s) {
  return check_export("covgpu_lmcov_check", [&] { return lmcov_check(p, o, s); });
}
extern "C" int covgpu_landmark_covariance(covgpu_context* c, const covgpu_options* opt, const covgpu_problem* p, const covgpu_lmcov_t* rq) {
  if (!c) { g_err = "covgpu_landmark_covariance: NULL context"; return COVGPU_ERR_INVALID_ARG; }
  return guarded([&] { return covariance_impl(c, opt, p, rq); });
}
extern "C" int covgpu_landmark_covariance_resident(covgpu_context* c, const covgpu_options* opt, const covgpu_lmcov_t* rq) {
  if (!c) { g_err = "covgpu_landmark_covariance_resident: NULL context"; return COVGPU_ERR_INVALID_ARG; }
  return guarded([&] { return resident_impl(c, opt, rq); });
}
