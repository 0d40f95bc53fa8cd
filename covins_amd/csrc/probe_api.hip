// probe_api.hip — the test entry points of libcovgpu: each uploads a problem and reads back what ONE stage of the product path
// computes on it (residuals, Jacobians, preintegration, the reduced system, one Gauss-Newton step, the dense solve), for the
// parity tests against the oracle. They run the product's own upload_impl / enqueue_build / enqueue_solve (host.hpp); the
// extern "C" wrappers at the end of the file map host exceptions to status codes (guarded) as the product entry points do.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "host.hpp"

using namespace covgpu;

template <typename T>
static int fetch(covgpu_context* c, T* host, const T* dev, size_t count) {
  if (count) HIPCHK(hipMemcpyAsync(host, dev, count * sizeof(T), hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  return COVGPU_OK;
}

static int residual_norms_impl(covgpu_context* c, const covgpu_options* opt, const covgpu_problem* p, double* norms) {
  covgpu_options o = *opt; o.visual_only = 1;
  RC(upload_impl(c, &o, p, false)); RC(reset_state(c));
  double* d; RC(dev_alloc(c, &d, (size_t)c->P.O));
  launch_obs_norms(c->P, d, c->st);
  return fetch(c, norms, d, (size_t)c->P.O);
}

static int linearize_reprojection_impl(covgpu_context* c, const covgpu_options* opt, const covgpu_problem* p, double* r, double* Jp, double* Jl, double* cost) {
  covgpu_options o = *opt; o.visual_only = 1;
  RC(upload_impl(c, &o, p, false)); RC(reset_state(c));
  const size_t O = c->P.O;
  double *dr, *dJp, *dJl, *dc;
  RC(dev_alloc(c, &dr, 2 * O)); RC(dev_alloc(c, &dJp, 12 * O)); RC(dev_alloc(c, &dJl, 6 * O)); RC(dev_alloc(c, &dc, O));
  launch_obs_linearize(c->P, dr, dJp, dJl, dc, c->st);
  RC(fetch(c, r, dr, 2 * O)); RC(fetch(c, Jp, dJp, 12 * O)); RC(fetch(c, Jl, dJl, 6 * O));
  return fetch(c, cost, dc, O);
}

static int preintegrate_impl(covgpu_context* c, const covgpu_options* opt, const covgpu_problem* p, double* delta, double* J, double* Pm) {
  covgpu_options o = *opt; o.visual_only = 0;
  RC(upload_impl(c, &o, p, false)); RC(reset_state(c));
  launch_preintegrate(c->P, c->st);
  const size_t I = c->P.I;
  RC(fetch(c, delta, c->P.pre_delta, 11 * I)); RC(fetch(c, J, c->P.pre_J, 225 * I));
  return fetch(c, Pm, c->P.pre_P, 225 * I);
}

static int linearize_imu_impl(covgpu_context* c, const covgpu_options* opt, const covgpu_problem* p, double* r, double* J) {
  covgpu_options o = *opt; o.visual_only = 0;
  RC(upload_impl(c, &o, p, false)); RC(reset_state(c));
  launch_preintegrate(c->P, c->st);
  const size_t I = c->P.I;
  double *dr, *dJ;
  RC(dev_alloc(c, &dr, 15 * I)); RC(dev_alloc(c, &dJ, 450 * I));
  launch_imu_linearize(c->P, dr, dJ, c->st);
  RC(fetch(c, r, dr, 15 * I));
  return fetch(c, J, dJ, 450 * I);
}

static int linearize_between_impl(covgpu_context* c, const covgpu_options* opt, const covgpu_problem* p, double* r, double* J, double* cost) {
  RC(upload_impl(c, opt, p, true)); RC(reset_state(c));
  const size_t E = c->P.E;
  double *dr, *dJ, *dc;
  RC(dev_alloc(c, &dr, 6 * E)); RC(dev_alloc(c, &dJ, 72 * E)); RC(dev_alloc(c, &dc, E));
  launch_edge_linearize(c->P, dr, dJ, dc, c->st);
  RC(fetch(c, r, dr, 6 * E)); RC(fetch(c, J, dJ, 72 * E));
  return fetch(c, cost, dc, E);
}

static int schur_impl(covgpu_context* c, const covgpu_options* opt, const covgpu_problem* p, bool pgo, double mu, double* S, double* b, double* cost) {
  RC(upload_impl(c, opt, p, pgo, false)); RC(reset_state(c));  // dense form: the test reads C back as one matrix
  launch_preintegrate(c->P, c->st);
  enqueue_build(c, mu);
  RC(read_scalars(c));
  *cost = c->h_scal[SC_COST];
  // assemble the reduced system in IR layout (D rows per keyframe) from its structured parts
  const DevProblem& P = c->P;
  const int n = P.n, npad = P.npad, K = P.K, D = P.D;
  std::vector<double> C((size_t)npad * npad);
  std::vector<int> perm(K), pos_kf(K), cptr(P.nchains + 1);
  RC(fetch(c, C.data(), P.Sred, C.size()));
  RC(fetch(c, perm.data(), P.perm, (size_t)K)); RC(fetch(c, pos_kf.data(), P.pos_kf, (size_t)K));
  RC(fetch(c, cptr.data(), P.chain_ptr, cptr.size()));
  std::fill(S, S + (size_t)n * n, 0.0);
  auto Sat = [&](int r, int cc) -> double& { return S[(size_t)r * n + cc]; };
  for (int a = 0; a < K; ++a)
    for (int bq = 0; bq < K; ++bq) {
      const int ra = 6 * perm[a], rb = 6 * perm[bq];
      for (int r = 0; r < 6; ++r)
        for (int cc = 0; cc < 6; ++cc) {
          const int i = ra + r, j = rb + cc;
          Sat(D * a + r, D * bq + cc) = (j <= i) ? C[(size_t)i * npad + j] : C[(size_t)j * npad + i];
        }
    }
  if (P.vi) {
    std::vector<double> Ad(81 * (size_t)K), Ae(81 * (size_t)K), Bp(54 * (size_t)K), Bs(54 * (size_t)K), Bn(54 * (size_t)K);
    RC(fetch(c, Ad.data(), P.Ad, Ad.size())); RC(fetch(c, Ae.data(), P.Ae, Ae.size()));
    RC(fetch(c, Bp.data(), P.Bp, Bp.size())); RC(fetch(c, Bs.data(), P.Bs, Bs.size())); RC(fetch(c, Bn.data(), P.Bn, Bn.size()));
    std::vector<int> chain_of(K);
    for (int ch = 0; ch < P.nchains; ++ch) for (int q = cptr[ch]; q < cptr[ch + 1]; ++q) chain_of[q] = ch;
    for (int pos = 0; pos < K; ++pos) {
      const int a = pos_kf[pos], ch = chain_of[pos];
      for (int r = 0; r < 9; ++r)
        for (int cc = 0; cc < 9; ++cc) Sat(15 * a + 6 + r, 15 * a + 6 + cc) = Ad[81 * (size_t)pos + 9 * r + cc];
      auto put_b = [&](const std::vector<double>& B, int other_pos) {
        const int o = pos_kf[other_pos];
        for (int r = 0; r < 9; ++r)
          for (int cc = 0; cc < 6; ++cc) {
            const double v = B[54 * (size_t)pos + 6 * r + cc];
            Sat(15 * a + 6 + r, 15 * o + cc) = v; Sat(15 * o + cc, 15 * a + 6 + r) = v;
          }
      };
      put_b(Bs, pos);
      if (pos > cptr[ch]) {
        put_b(Bp, pos - 1);
        const int o = pos_kf[pos - 1];
        for (int r = 0; r < 9; ++r)
          for (int cc = 0; cc < 9; ++cc) {
            const double v = Ae[81 * (size_t)pos + 9 * r + cc];
            Sat(15 * a + 6 + r, 15 * o + 6 + cc) = v; Sat(15 * o + 6 + cc, 15 * a + 6 + r) = v;
          }
      }
      if (pos + 1 < cptr[ch + 1]) put_b(Bn, pos + 1);
    }
  }
  return fetch(c, b, P.bred, (size_t)n);
}

// one damped Gauss-Newton step at the uploaded estimate through the PRODUCT solve path (landmark elimination, multifrontal
// solve of the reduced camera system — sharded if a shard is set — and landmark back-substitution)
static int gn_step_impl(covgpu_context* c, const covgpu_options* opt, const covgpu_problem* p, double mu, double* dx, double* dl, double* cost) {
  RC(upload_impl(c, opt, p, false)); RC(reset_state(c));
  launch_preintegrate(c->P, c->st);
  enqueue_build(c, mu);
  enqueue_solve(c, c->P.gn);
  RC(read_scalars(c));
  if (chol_failed(c)) { g_err = "reduced system is not positive definite"; return COVGPU_ERR_NUMERIC; }
  if (cost) *cost = c->h_scal[SC_COST];
  RC(fetch(c, dx, c->P.gn, (size_t)c->P.n));
  return fetch(c, dl, c->P.gn + c->P.n, (size_t)3 * c->P.L);
}

static int solve_reduced_impl(covgpu_context* c, int32_t n, const double* S, const double* b, double* x) {
  HIPCHK(hipSetDevice(c->device));
  if (n <= 0) { g_err = "n <= 0"; return COVGPU_ERR_INVALID_ARG; }
  const int npad = ((n + kTile - 1) / kTile) * kTile;
  std::vector<double> Sp((size_t)npad * npad, 0.0), bp((size_t)2 * npad, 0.0);
  for (int r = 0; r < npad; ++r) {
    if (r < n) { std::memcpy(&Sp[(size_t)r * npad], S + (size_t)r * n, (size_t)(r + 1) * sizeof(double)); bp[r] = b[r]; }
    else Sp[(size_t)r * npad + r] = 1.0;
  }
  int flag = 0;   // (receives a fetch: declared, like Sp and bp, before the scratch)
  DeviceScratch U(c->st);
  double *dS = nullptr, *db = nullptr, *dL = nullptr; int* df = nullptr;
  HIPCHK(U.upload(&dS, Sp.data(), Sp.size())); HIPCHK(U.upload(&db, bp.data(), bp.size()));
  HIPCHK(U.alloc(&dL, (size_t)(npad / kTile) * kTile * kTile)); HIPCHK(U.zeroed(&df, 4));
  {
    FormScope census(&c->chol.forms);
    dense_cholesky_solve_raw(dS, db, dL, df, npad, c->st, c->chol);
  }
  HIPCHK(U.fetch(x, db, (size_t)n)); HIPCHK(U.fetch(&flag, df, 1));
  HIPCHK(hipStreamSynchronize(c->st));
  if (flag) { g_err = "reduced system is not positive definite"; return COVGPU_ERR_NUMERIC; }
  return COVGPU_OK;
}

// ---- the trust-region tail (k_tail.hip, k_dense.hip: k_tr_*)
static int fetch_tail_state_impl(covgpu_context* c, double* grad, double* hdiag, double* gn, double* vtmp, double* pose_c, double* sb_c, double* lm_c) {
  if (!c->have) { g_err = "covgpu_fetch_tail_state: no problem uploaded"; return COVGPU_ERR_INVALID_ARG; }
  HIPCHK(hipSetDevice(c->device));
  const DevProblem& P = c->P;
  DeviceScratch U(c->st);   // (fetch only: skips the outputs the caller did not ask for)
  HIPCHK(U.fetch(grad, (const double*)P.grad, (size_t)P.N)); HIPCHK(U.fetch(hdiag, (const double*)P.hdiag, (size_t)P.N));
  HIPCHK(U.fetch(gn, (const double*)P.gn, (size_t)P.N)); HIPCHK(U.fetch(vtmp, (const double*)P.vtmp, (size_t)P.N));
  HIPCHK(U.fetch(pose_c, (const double*)P.pose_c, (size_t)7 * P.K));
  if (P.vi) HIPCHK(U.fetch(sb_c, (const double*)P.sb_c, (size_t)9 * P.K));
  HIPCHK(U.fetch(lm_c, (const double*)P.lm_c, (size_t)3 * P.L));
  HIPCHK(hipStreamSynchronize(c->st));
  return COVGPU_OK;
}

// the step logic on a stub problem: nothing but the trust-region state, the scalars, the flags and the partial sums exist (K = L = 0:
// k_tr_accept behind k_tr_decide copies nothing)
static int tail_logic_probe_impl(covgpu_context* c, const covgpu_options* o, int kernel, int stage, int with_logic, int fresh, int flag0, double* tr,
                                 double* scal, const double* part, int part_n) {
  auto bad = [](const char* m) -> int { g_err = std::string("covgpu_tail_logic_probe: ") + m; return COVGPU_ERR_INVALID_ARG; };
  if (!o || !tr || !scal) return bad("NULL argument");
  if (kernel < 0 || kernel > 4) return bad("kernel must be 0 .. 4");
  if ((kernel == 0 || kernel == 1) && stage != 1 && stage != 2) return bad("stage must be 1 or 2");
  if (kernel == 1 && (!part || part_n < 1)) return bad("k_tail_finish needs part[COVGPU_SC_COUNT][part_n], part_n >= 1");
  HIPCHK(hipSetDevice(c->device));
  DevProblem P;
  std::memset(&P, 0, sizeof(P));
  const int flags[4] = {flag0, 0, 0, 0};
  DeviceScratch U(c->st);
  HIPCHK(U.upload(&P.tr, tr, (size_t)TR_COUNT)); HIPCHK(U.upload(&P.scal, scal, (size_t)SC_COUNT)); HIPCHK(U.upload(&P.flag, flags, 4));
  P.scal_r = P.scal; P.flag_r = P.flag;
  if (kernel == 1) { HIPCHK(U.upload(&P.part, part, (size_t)SC_COUNT * part_n)); P.part_n = part_n; }
  const TrConsts tc{o->strategy, o->max_radius, o->min_relative_decrease, o->function_tolerance, o->parameter_tolerance, o->gradient_tolerance};
  switch (kernel) {
    case 0: launch_tail_logic(P, tc, stage, fresh, c->st); break;
    case 1: launch_tail_finish(P, tc, stage, o->strategy == COVGPU_DOGLEG, with_logic != 0, fresh, c->st); break;
    case 2: launch_tr_after_solve(P, tc, fresh, c->st); break;
    case 3: launch_tr_after_model(P, tc, c->st); break;
    default: launch_tr_decide(P, tc, c->st); break;
  }
  HIPCHK(U.fetch(tr, (const double*)P.tr, (size_t)TR_COUNT)); HIPCHK(U.fetch(scal, (const double*)P.scal, (size_t)SC_COUNT));
  HIPCHK(hipStreamSynchronize(c->st));
  HIPCHK(hipGetLastError());
  return COVGPU_OK;
}

extern "C" int covgpu_fetch_tail_state(covgpu_context* c, double* grad, double* hdiag, double* gn, double* vtmp, double* pose_c, double* sb_c, double* lm_c) {
  if (!c) { g_err = "covgpu_fetch_tail_state: NULL context"; return COVGPU_ERR_INVALID_ARG; }
  return guarded([&] { return fetch_tail_state_impl(c, grad, hdiag, gn, vtmp, pose_c, sb_c, lm_c); });
}
extern "C" int covgpu_tail_logic_probe(covgpu_context* c, const covgpu_options* opt, int32_t kernel, int32_t stage, int32_t with_logic, int32_t fresh,
                                       int32_t flag0, double* tr, double* scal, const double* part, int32_t part_n) {
  if (!c) { g_err = "covgpu_tail_logic_probe: NULL context"; return COVGPU_ERR_INVALID_ARG; }
  return guarded([&] { return tail_logic_probe_impl(c, opt, kernel, stage, with_logic, fresh, flag0, tr, scal, part, part_n); });
}

extern "C" int covgpu_reprojection_residual_norms(covgpu_context* c, const covgpu_options* opt, const covgpu_problem* p, double* norms) {
  return guarded([&] { return residual_norms_impl(c, opt, p, norms); });
}
extern "C" int covgpu_linearize_reprojection(covgpu_context* c, const covgpu_options* opt, const covgpu_problem* p, double* r, double* Jp,
                                             double* Jl, double* cost) {
  return guarded([&] { return linearize_reprojection_impl(c, opt, p, r, Jp, Jl, cost); });
}
extern "C" int covgpu_preintegrate(covgpu_context* c, const covgpu_options* opt, const covgpu_problem* p, double* delta, double* J, double* Pm) {
  return guarded([&] { return preintegrate_impl(c, opt, p, delta, J, Pm); });
}
extern "C" int covgpu_linearize_imu(covgpu_context* c, const covgpu_options* opt, const covgpu_problem* p, double* r, double* J) {
  return guarded([&] { return linearize_imu_impl(c, opt, p, r, J); });
}
extern "C" int covgpu_linearize_between(covgpu_context* c, const covgpu_options* opt, const covgpu_problem* p, double* r, double* J, double* cost) {
  return guarded([&] { return linearize_between_impl(c, opt, p, r, J, cost); });
}
extern "C" int covgpu_schur(covgpu_context* c, const covgpu_options* opt, const covgpu_problem* p, double mu, double* S, double* b, double* cost) {
  return guarded([&] { return schur_impl(c, opt, p, false, mu, S, b, cost); });
}
extern "C" int covgpu_schur_pgo(covgpu_context* c, const covgpu_options* opt, const covgpu_problem* p, double mu, double* S, double* b, double* cost) {
  return guarded([&] { return schur_impl(c, opt, p, true, mu, S, b, cost); });
}
extern "C" int covgpu_gn_step(covgpu_context* c, const covgpu_options* opt, const covgpu_problem* p, double mu, double* dx, double* dl, double* cost) {
  return guarded([&] { return gn_step_impl(c, opt, p, mu, dx, dl, cost); });
}
extern "C" int covgpu_solve_reduced(covgpu_context* c, int32_t n, const double* S, const double* b, double* x) {
  return guarded([&] { return solve_reduced_impl(c, n, S, b, x); });
}
