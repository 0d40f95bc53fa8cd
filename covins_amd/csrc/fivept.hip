// fivept.hip — host side of the five-point relative-pose batch (k_fivept.hip): the extern "C" entry points, written as
// those of batch.hip are: check (fivept_check.hpp: a pure function that also fills the call's plan), hipSetDevice, uploads into one
// DeviceScratch (host.hpp), one launch, fetches and one synchronisation of the context's stream, at the end. A file of its own beside
// batch.hip, as voctrain.hip is: tests/test_gpu_batch_errors.py lists the entry points of those two files one by one.
#include <vector>

#include "host.hpp"

using namespace covgpu;

extern "C" void covgpu_default_fivept_opts(covgpu_fivept_opts* o) {
  if (!o) return;
  o->min_inliers = 20; o->max_iterations = 200; o->probability = 0.99; o->threshold = 16.0; o->sigma = 4.5e-6; o->seed = 0;   // config_backend.yaml:100-102
}

extern "C" void covgpu_fivept_limits(int32_t out[4]) {
  if (!out) return;
  int v[4];
  fivept_limits(v);
  for (int i = 0; i < 4; ++i) out[i] = v[i];
}

extern "C" int covgpu_fivept_check(const covgpu_fivept_batch_t* bt, const covgpu_fivept_opts* opts) {
  return check_export("covgpu_fivept_check", [&] { FiveptPlan P; return fivept_check(bt, opts, P); });
}

extern "C" int covgpu_fivept_ransac_batch(covgpu_context* c, const covgpu_fivept_batch_t* bt, const covgpu_fivept_opts* opts) {
  return batch_entry("covgpu_fivept_ransac_batch", c, [&](auto bad) -> int {
    FiveptPlan P;
    if (const char* m = fivept_check(bt, opts, P)) return bad(m);
    const size_t B = (size_t)bt->num, C = P.corr;
    if (B == 0) return COVGPU_OK;
    HIPCHK(hipSetDevice(c->device));
    DeviceScratch U(c->st);
    int *dptr_ = nullptr, *din = nullptr, *dst = nullptr, *dit = nullptr, *dbd = nullptr;
    double *df1 = nullptr, *df2 = nullptr, *dT = nullptr;
    unsigned long long* dseed = nullptr;
    unsigned char* dmask = nullptr;
    HIPCHK(U.upload(&dptr_, bt->corr_ptr, B + 1));
    HIPCHK(U.upload(&df1, bt->bearing1, 3 * C)); HIPCHK(U.upload(&df2, bt->bearing2, 3 * C));
    HIPCHK(U.upload(&dseed, P.seeds.data(), B));
    HIPCHK(U.upload(&dT, bt->T_12, 7 * B));   // untouched rows come back as they went
    HIPCHK(U.alloc(&dmask, C)); HIPCHK(U.alloc(&din, B)); HIPCHK(U.alloc(&dst, B)); HIPCHK(U.alloc(&dit, B)); HIPCHK(U.alloc(&dbd, B));
    HIPCHK(launch_fivept((int)B, dptr_, df1, df2, dseed, dT, dmask, din, dst, dit, dbd, opts->min_inliers, opts->max_iterations, opts->probability,
                  opts->threshold, opts->sigma, P.max_n, c->st));   // raising the dynamic LDS limit, then the launch
    HIPCHK(U.fetch(bt->T_12, dT, 7 * B)); HIPCHK(U.fetch(bt->inliers, din, B)); HIPCHK(U.fetch(bt->status, dst, B));
    HIPCHK(U.fetch(bt->iterations, dit, B)); HIPCHK(U.fetch(bt->best_draw, dbd, B));
    HIPCHK(U.fetch(bt->inlier, dmask, C));
    HIPCHK(hipStreamSynchronize(c->st));
    return COVGPU_OK;
  });
}

extern "C" int covgpu_fivept_solve_batch(covgpu_context* c, int32_t n, const double* f1, const double* f2, double* E, int32_t* nsol, double* T,
                                         int32_t* chosen) {
  return batch_entry("covgpu_fivept_solve_batch", c, [&](auto bad) -> int {
    if (const char* m = fivept_solve_check(n, f1, f2, E, nsol, T, chosen)) return bad(m);
    if (n == 0) return COVGPU_OK;
    const size_t N = (size_t)n;
    HIPCHK(hipSetDevice(c->device));
    DeviceScratch U(c->st);
    double *d1, *d2, *dE, *dT; int *dn, *dc;
    HIPCHK(U.upload(&d1, f1, 24 * N)); HIPCHK(U.upload(&d2, f2, 24 * N)); HIPCHK(U.zeroed(&dE, 90 * N)); HIPCHK(U.upload(&dT, T, 7 * N));
    HIPCHK(U.alloc(&dn, N)); HIPCHK(U.alloc(&dc, N));
    HIPCHK(launch_fivept_solve(n, d1, d2, dE, dn, dT, dc, c->st));
    HIPCHK(U.fetch(E, dE, 90 * N)); HIPCHK(U.fetch(nsol, dn, N)); HIPCHK(U.fetch(T, dT, 7 * N)); HIPCHK(U.fetch(chosen, dc, N));
    HIPCHK(hipStreamSynchronize(c->st));
    return COVGPU_OK;
  });
}
