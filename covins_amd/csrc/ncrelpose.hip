// ncrelpose.hip — host side of the 17-point batch (k_ncrelpose.hip): the extern "C" entry points, written as those of
// fivept.hip are: check (ncrelpose_check.hpp: a pure function that also fills the call's plan), hipSetDevice, uploads into one
// DeviceScratch (host.hpp), one launch, fetches and one synchronisation of the context's stream, at the end.
#include <vector>

#include "host.hpp"
#include "ncrelpose.hpp"
#include "ncrelpose_check.hpp"

using namespace covgpu;

extern "C" void covgpu_default_ncrelpose_opts(covgpu_ncrelpose_opts* o) {
  if (!o) return;
  o->rp_error = 1.5; o->rp_error_cov = 10.0; o->min_inliers = 100; o->max_iterations = 4000; o->cov_thres = 10.0; o->cov_iters = 30;   // config_backend.yaml:91-97
  o->cov_max_iters = 300; o->probability = 0.99; o->seed = 0; o->stage_cap = 0;
}

extern "C" void covgpu_ncrelpose_limits(int32_t out[8]) {
  if (!out) return;
  int v[8];
  ncrelpose_limits(v);
  for (int i = 0; i < 8; ++i) out[i] = v[i];
}

extern "C" int covgpu_ncrelpose_check(const covgpu_ncrelpose_batch_t* bt, const covgpu_ncrelpose_opts* opts) {
  return check_export("covgpu_ncrelpose_check", [&] { NcrelposePlan P; return ncrelpose_check(bt, opts, P); });
}

extern "C" int covgpu_ncrelpose_batch(covgpu_context* c, const covgpu_ncrelpose_batch_t* bt, const covgpu_ncrelpose_opts* opts) {
  return batch_entry("covgpu_ncrelpose_batch", c, [&](auto bad) -> int {
    NcrelposePlan P;
    if (const char* m = ncrelpose_check(bt, opts, P)) return bad(m);
    const size_t B = (size_t)bt->num, C = P.corr, M = P.cams;
    if (B == 0) return COVGPU_OK;
    HIPCHK(hipSetDevice(c->device));
    DeviceScratch U(c->st);
    NcRelposeArgs a{};
    a.num = (int)B; a.cells = bt->cells; a.max_n = P.max_n; a.stage_cap = opts->stage_cap;
    int *dptr_ = nullptr, *dcell = nullptr, *dc1 = nullptr, *dc2 = nullptr, *dcp = nullptr;
    double *df1 = nullptr, *df2 = nullptr, *dcam = nullptr, *dTq = nullptr, *dTc = nullptr;
    unsigned long long* dseed = nullptr;
    HIPCHK(U.upload(&dptr_, bt->corr_ptr, B + 1)); HIPCHK(U.upload(&dcell, bt->cell_ptr, B * ((size_t)bt->cells + 1)));
    HIPCHK(U.upload(&df1, bt->bearing1, 3 * C)); HIPCHK(U.upload(&df2, bt->bearing2, 3 * C));
    HIPCHK(U.upload(&dc1, bt->cam1, C)); HIPCHK(U.upload(&dc2, bt->cam2, C));
    HIPCHK(U.upload(&dcp, bt->cam_ptr, B + 1)); HIPCHK(U.upload(&dcam, bt->cam, 12 * M));
    HIPCHK(U.upload(&dTq, bt->T_sc_q, 7 * B)); HIPCHK(U.upload(&dTc, bt->T_sc_c, 7 * B));
    HIPCHK(U.upload(&dseed, P.seeds.data(), B));
    a.ptr = dptr_; a.cell = dcell; a.f1 = df1; a.f2 = df2; a.cam1 = dc1; a.cam2 = dc2; a.cam_ptr = dcp; a.cam = dcam; a.Tq = dTq; a.Tc = dTc; a.seed = dseed;
    HIPCHK(U.upload(&a.T, bt->T_c1c2, 7 * B)); HIPCHK(U.upload(&a.Tr, bt->T_c1c2_ransac, 7 * B));   // untouched rows come back as they went
    HIPCHK(U.upload(&a.Ts, bt->T_s1s2, 7 * B)); HIPCHK(U.upload(&a.cov, bt->cov, 36 * B));
    HIPCHK(U.alloc(&a.inlier, C)); HIPCHK(U.alloc(&a.list, C));
    HIPCHK(U.alloc(&a.inliers, B)); HIPCHK(U.alloc(&a.status, B)); HIPCHK(U.alloc(&a.iterations, B)); HIPCHK(U.alloc(&a.best_draw, B));
    HIPCHK(U.alloc(&a.cov_rows, B)); HIPCHK(U.alloc(&a.cov_draws, B));
    a.min_inliers = opts->min_inliers; a.max_iterations = opts->max_iterations; a.cov_iters = opts->cov_iters; a.cov_max_iters = opts->cov_max_iters;
    a.probability = opts->probability; a.threshold = P.threshold; a.th_cov = P.th_cov; a.cov_thres = opts->cov_thres;
    HIPCHK(launch_ncrelpose(a, c->st));
    HIPCHK(U.fetch(bt->T_c1c2, a.T, 7 * B)); HIPCHK(U.fetch(bt->T_c1c2_ransac, a.Tr, 7 * B)); HIPCHK(U.fetch(bt->T_s1s2, a.Ts, 7 * B));
    HIPCHK(U.fetch(bt->cov, a.cov, 36 * B)); HIPCHK(U.fetch(bt->inlier, a.inlier, C));
    HIPCHK(U.fetch(bt->inliers, a.inliers, B)); HIPCHK(U.fetch(bt->status, a.status, B)); HIPCHK(U.fetch(bt->iterations, a.iterations, B));
    HIPCHK(U.fetch(bt->best_draw, a.best_draw, B)); HIPCHK(U.fetch(bt->cov_rows, a.cov_rows, B)); HIPCHK(U.fetch(bt->cov_draws, a.cov_draws, B));
    HIPCHK(hipStreamSynchronize(c->st));
    return COVGPU_OK;
  });
}

extern "C" int covgpu_ncrelpose_solve_batch(covgpu_context* c, int32_t n, int32_t N, const double* ray1, const double* ray2, double* T, int32_t* ok,
                                            double* sv) {
  return batch_entry("covgpu_ncrelpose_solve_batch", c, [&](auto bad) -> int {
    if (const char* m = ncrelpose_solve_check(n, N, ray1, ray2, T, ok, sv)) return bad(m);
    if (n == 0) return COVGPU_OK;
    const size_t K = (size_t)n;
    HIPCHK(hipSetDevice(c->device));
    DeviceScratch U(c->st);
    double *d1, *d2, *dT, *dsv; int* dok;
    HIPCHK(U.upload(&d1, ray1, 6 * K * N)); HIPCHK(U.upload(&d2, ray2, 6 * K * N)); HIPCHK(U.upload(&dT, T, 7 * K));
    HIPCHK(U.alloc(&dok, K)); HIPCHK(U.alloc(&dsv, 3 * K));
    HIPCHK(launch_ncrelpose_solve(n, N, d1, d2, dT, dok, dsv, c->st));
    HIPCHK(U.fetch(T, dT, 7 * K)); HIPCHK(U.fetch(ok, dok, K)); HIPCHK(U.fetch(sv, dsv, 3 * K));
    HIPCHK(hipStreamSynchronize(c->st));
    return COVGPU_OK;
  });
}
