// obscov.hip — covgpu_observation_covariance / covgpu_observation_covariance_resident (include/covgpu.h): the host side of
// the observation pass of k_obscov.hip. A call is the landmark call's (lmcov.hip) with another kernel behind the sweep: step one of
// covgpu_selected_inverse (sel_factor_and_sweep leaves Sigma in its scratch), the landmark pass's tables (lmcov_lists / lmcov_prepare /
// lmcov_upload, shared, not copied), then ONE launch that writes the landmark blocks as k_lmcov does and the blocks of every observation.
// All scratch is allocated before anything is enqueued; nothing is kept per upload.
#include <string>
#include <vector>

#include "host.hpp"
#include "obscov.hpp"
#include "selinv.hpp"

using namespace covgpu;

namespace {

int bad_arg(const char* fn, const std::string& m) { g_err = std::string(fn) + ": " + m; return COVGPU_ERR_INVALID_ARG; }

int sweep_and_pass(const char* fn, covgpu_context* c, const covgpu_obscov_t* rq) {
  const DevProblem& P = c->P;
  const int L = P.L;
  const size_t O = (size_t)P.O;
  LmcovTables lp;
  RC(lmcov_lists(fn, c, lp));

  DeviceScratch U(c->st);
  SelSweep sw;
  ObscovArgs a{};
  long long* src = nullptr; double* kf_out = nullptr;
  size_t own_bytes = 0;
  covgpu_selinv_t diag{};   // the read-out of kf_cov, as the landmark call has it
  diag.block = 0; diag.mu = rq->mu; diag.kf_cov = rq->kf_cov; diag.num_pairs = 0;
  RC(sel_factor_and_sweep(fn, c, rq->mu, U, sw, [&](SelPlan& pl) -> int {
    RC(lmcov_prepare(fn, c, pl, U, lp, own_bytes));
    if (rq->kf_cov) {
      if (const char* m = sel_plan_readout(c, &diag, lp.fixed.data(), pl)) return bad_arg(fn, m);
      HIPCHK(U.alloc(&src, pl.src.size())); HIPCHK(U.alloc(&kf_out, pl.src.size()));
      own_bytes += pl.src.size() * (sizeof(long long) + sizeof(double));
    }
    HIPCHK(U.alloc(&a.vx, O * kObscovCrossDoubles)); HIPCHK(U.alloc(&a.obs_cov, O * kObscovBlockDoubles));
    HIPCHK(U.alloc(&a.obs_res, O * 2)); HIPCHK(U.alloc(&a.obs_ok, O));
    own_bytes += O * ((kObscovCrossDoubles + kObscovBlockDoubles + 2) * sizeof(double) + 1);
    return COVGPU_OK;
  }));
  RC(lmcov_upload(c, lp, a.lm));
  a.lm.S = sw.a.S;
  launch_obscov(P, a, c->st);
  if (rq->kf_cov) {
    RC(sel_read_out(c, sw, src, kf_out));
    HIPCHK(U.fetch(rq->kf_cov, (const double*)kf_out, sw.pl.src.size()));
  }
  HIPCHK(U.fetch(rq->lm_cov, (const double*)a.lm.lm_cov, (size_t)9 * L));
  HIPCHK(U.fetch(rq->lm_ok, (const uint8_t*)a.lm.lm_ok, (size_t)L));
  HIPCHK(U.fetch(rq->obs_cov, (const double*)a.obs_cov, O * kObscovBlockDoubles));
  HIPCHK(U.fetch(rq->cross_cov, (const double*)a.vx, O * kObscovCrossDoubles));
  HIPCHK(U.fetch(rq->obs_res, (const double*)a.obs_res, O * 2));
  HIPCHK(U.fetch(rq->obs_ok, (const uint8_t*)a.obs_ok, O));
  std::vector<int> obs_kf;
  if (rq->stats) {   // (the count of the observations by constant keyframes)
    obs_kf.resize(O);
    HIPCHK(U.fetch(obs_kf.data(), (const int*)P.obs_kf, O));
  }
  HIPCHK(hipStreamSynchronize(c->st));
  HIPCHK(hipGetLastError());
  if (rq->stats) {
    int64_t* s = rq->stats;
    int64_t bad = 0, constant = 0;
    for (size_t o = 0; o < O; ++o) { bad += rq->obs_ok[o] ? 0 : 1; constant += lp.fixed[(size_t)obs_kf[o]] ? 1 : 0; }
    s[0] = (int64_t)sw.pl.fronts.size(); s[1] = (int64_t)c->nd.lev.size(); s[2] = sw.n_mfma + sw.n_vec + sw.n_gather + (rq->kf_cov ? 1 : 0); s[3] = 1;
    s[4] = P.lm_group == 4 || P.lm_group == 8 ? P.lm_group : 16;
    s[5] = (int64_t)(sw.bytes + own_bytes); s[6] = bad; s[7] = constant;
  }
  return COVGPU_OK;
}

int covariance_impl(covgpu_context* c, const covgpu_options* opt, const covgpu_problem* p, const covgpu_obscov_t* rq) {
  const char* fn = "covgpu_observation_covariance";
  if (const char* e = obscov_check(p, opt, rq)) return bad_arg(fn, e);
  if (c->sharded) return bad_arg(fn, "a sharded context holds one rank's share of the factor");
  RC(upload_impl(c, opt, p, false));
  RC(lmcov_context_check(fn, c));
  RC(reset_state(c));
  return sweep_and_pass(fn, c, rq);
}

int resident_impl(covgpu_context* c, const covgpu_options* opt, const covgpu_obscov_t* rq) {
  const char* fn = "covgpu_observation_covariance_resident";
  if (!opt) return bad_arg(fn, "NULL options");
  if (const char* e = obscov_request_check(rq)) return bad_arg(fn, e);
  RC(lmcov_context_check(fn, c));
  HIPCHK(hipSetDevice(c->device));
  c->P.reproj_loss_a = opt->reproj_loss_a;   // (as every solve of the resident problem takes it)
  if (!c->state_set) RC(reset_state(c));     // an upload alone: the estimate is the uploaded one
  return sweep_and_pass(fn, c, rq);
}

}  // namespace

extern "C" void covgpu_obscov_limits(int32_t out[4]) {
  out[0] = kObscovMaxGroup; out[1] = kObscovThreads; out[2] = kObscovCrossDoubles; out[3] = kObscovBlockDoubles;
}
extern "C" int covgpu_obscov_check(const covgpu_problem* p, const covgpu_options* o, const covgpu_obscov_t* s) {
  return check_export("covgpu_obscov_check", [&] { return obscov_check(p, o, s); });
}
extern "C" int covgpu_observation_covariance(covgpu_context* c, const covgpu_options* opt, const covgpu_problem* p, const covgpu_obscov_t* rq) {
  if (!c) { g_err = "covgpu_observation_covariance: NULL context"; return COVGPU_ERR_INVALID_ARG; }
  return guarded([&] { return covariance_impl(c, opt, p, rq); });
}
extern "C" int covgpu_observation_covariance_resident(covgpu_context* c, const covgpu_options* opt, const covgpu_obscov_t* rq) {
  if (!c) { g_err = "covgpu_observation_covariance_resident: NULL context"; return COVGPU_ERR_INVALID_ARG; }
  return guarded([&] { return resident_impl(c, opt, rq); });
}
