// batch.hip — host side of libcovgpu's stateless batch front end: the extern "C" entry points that take one batch of host arrays,
// run its kernels on the context's stream and hand the results back. Nothing here touches the resident problem of the solver
// (upload.hip, solver.hip): a context lends its device and its stream only. Serves DESIGN.md §4.9 (relative pose, k_relpose.hip; the landmark
// re-anchoring behind a pose-graph solve), §4.10 (P3P RANSAC, k_abspose.hip), §4.11 (descriptor matching, k_match.hip), §4.12
// (guided matching, k_guided.hip), §4.13 (bag-of-words transform, score and candidate query, k_bow.hip), §4.14 (redundant-keyframe
// pruning, k_prune.hip), §4.15 (landmark descriptors, normals and scale ranges, k_lmrefresh.hip) and §4.17 (float descriptor matching,
// k_matchf.hip).
// Every entry point checks all its arguments before its first device call, holds its device buffers in one DeviceScratch
// (host.hpp) and synchronises its stream once, at the end.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "host.hpp"

using namespace covgpu;

// The prologue of every device entry point of this file: a NULL context is an argument error, and no C++ exception leaves the call.
// `bad` is the body's argument-error return: "<function>: <message>".
template <typename F>
static int batch_entry(const char* fn, covgpu_context* c, F&& body) {
  auto bad = [fn](const char* m) -> int { g_err = std::string(fn) + ": " + m; return COVGPU_ERR_INVALID_ARG; };
  if (!c) return bad("NULL context");
  return guarded([&] { return body(bad); });
}

extern "C" int covgpu_relpose_batch(covgpu_context* c, const covgpu_relpose_batch_t* bt, double th_outlier, int32_t min_inliers) {
  return batch_entry("covgpu_relpose_batch", c, [&](auto bad) -> int {
    if (!bt || bt->num_pairs < 0 || (bt->num_pairs > 0 && (!bt->corr_ptr || !bt->T_ab || !bt->inliers || !bt->cam_a || !bt->cam_b || !bt->dist_type_a || !bt->dist_type_b)))
      return bad("NULL array");
    const size_t B = (size_t)bt->num_pairs;
    if (B == 0) return COVGPU_OK;
    for (size_t b = 0; b < B; ++b) if (bt->corr_ptr[b + 1] < bt->corr_ptr[b]) return bad("corr_ptr not monotone");
    for (const int32_t* m : {bt->cam_model_a, bt->cam_model_b}) if (m) for (size_t b = 0; b < B; ++b) {
      if (m[b] != COVGPU_CAM_PINHOLE && m[b] != COVGPU_CAM_UNIFIED) return bad("unknown camera model");
    }
    // per side: model and xi of every pair (xi 0 for pinhole rows); uploaded only if some camera of the batch is unified
    std::vector<int32_t> hmA(B, COVGPU_CAM_PINHOLE), hmB(B, COVGPU_CAM_PINHOLE);
    std::vector<double> hxA(B, 0.0), hxB(B, 0.0);
    bool uni = false;
    for (int side = 0; side < 2; ++side) {
      const int32_t* m = side ? bt->cam_model_b : bt->cam_model_a;
      const double* x = side ? bt->xi_b : bt->xi_a;
      std::vector<int32_t>& hm = side ? hmB : hmA;
      std::vector<double>& hx = side ? hxB : hxA;
      if (!m) continue;
      for (size_t b = 0; b < B; ++b) {
        if (m[b] != COVGPU_CAM_UNIFIED) continue;
        if (!x) return bad("unified camera without xi");
        if (!std::isfinite(x[b]) || x[b] < 0.0) return bad("xi of a unified camera is negative or not finite");
        hm[b] = COVGPU_CAM_UNIFIED; hx[b] = x[b]; uni = true;
      }
    }
    const size_t C = (size_t)bt->corr_ptr[B];
    if (C > 0 && (!bt->p_a || !bt->p_b || !bt->kp_a || !bt->kp_b || !bt->sigma_a || !bt->sigma_b || !bt->outlier)) return bad("NULL correspondence array");
    HIPCHK(hipSetDevice(c->device));
    DeviceScratch U(c->st);
    int *dptr_ = nullptr, *dda = nullptr, *ddb = nullptr, *din = nullptr, *dmA = nullptr, *dmB = nullptr;
    double *dpB = nullptr, *dpA = nullptr, *dkA = nullptr, *dkB = nullptr, *dsA = nullptr, *dsB = nullptr, *dcA = nullptr, *dcB = nullptr, *dT = nullptr;
    double *dxA = nullptr, *dxB = nullptr;
    unsigned char* dout = nullptr;
    HIPCHK(U.upload(&dptr_, bt->corr_ptr, B + 1));
    HIPCHK(U.upload(&dpB, bt->p_b, 3 * C)); HIPCHK(U.upload(&dpA, bt->p_a, 3 * C));
    HIPCHK(U.upload(&dkA, bt->kp_a, 2 * C)); HIPCHK(U.upload(&dkB, bt->kp_b, 2 * C));
    HIPCHK(U.upload(&dsA, bt->sigma_a, C)); HIPCHK(U.upload(&dsB, bt->sigma_b, C));
    HIPCHK(U.upload(&dcA, bt->cam_a, 8 * B)); HIPCHK(U.upload(&dcB, bt->cam_b, 8 * B));
    HIPCHK(U.upload(&dda, bt->dist_type_a, B)); HIPCHK(U.upload(&ddb, bt->dist_type_b, B));
    HIPCHK(U.upload(&dT, bt->T_ab, 7 * B));
    if (uni) {
      HIPCHK(U.upload(&dmA, hmA.data(), B)); HIPCHK(U.upload(&dmB, hmB.data(), B));
      HIPCHK(U.upload(&dxA, hxA.data(), B)); HIPCHK(U.upload(&dxB, hxB.data(), B));
    }
    HIPCHK(U.alloc(&din, B)); HIPCHK(U.alloc(&dout, C));
    launch_relpose((int)B, dptr_, dpB, dpA, dkA, dkB, dsA, dsB, dcA, dda, dcB, ddb, th_outlier, min_inliers, dT, dout, din, c->st, dmA, dxA, dmB, dxB);
    HIPCHK(U.fetch(bt->T_ab, dT, 7 * B)); HIPCHK(U.fetch(bt->inliers, din, B)); HIPCHK(U.fetch(bt->outlier, dout, C));
    HIPCHK(hipStreamSynchronize(c->st));
    return COVGPU_OK;
  });
}

extern "C" void covgpu_default_ransac_opts(covgpu_ransac_opts* o) {
  if (!o) return;
  o->min_inliers = 6; o->max_iterations = 300; o->probability = 0.99; o->threshold = 25.0; o->seed = 0;   // config_backend.yaml:85-88
}

extern "C" int covgpu_abspose_ransac_batch(covgpu_context* c, const covgpu_abspose_batch_t* bt, const covgpu_ransac_opts* opts) {
  return batch_entry("covgpu_abspose_ransac_batch", c, [&](auto bad) -> int {
    if (!bt || !opts) return bad("NULL batch or options");
    if (bt->num < 0) return bad("num < 0");
    if (opts->max_iterations <= 0) return bad("max_iterations <= 0");
    if (opts->max_iterations > 100000) return bad("max_iterations > 100000 (a candidate makes up to 11 max_iterations draws in one launch)");
    if (!(opts->probability > 0.0 && opts->probability < 1.0)) return bad("probability outside (0, 1)");
    if (!std::isfinite(opts->threshold) || !(opts->threshold > 0.0)) return bad("threshold not finite or not positive");
    const size_t B = (size_t)bt->num;
    if (B == 0) return COVGPU_OK;
    if (!bt->corr_ptr || !bt->T_wc || !bt->inliers) return bad("NULL array");
    if (bt->corr_ptr[0] != 0) return bad("corr_ptr[0] != 0");
    int max_n = 0;
    for (size_t b = 0; b < B; ++b) {
      if (bt->corr_ptr[b + 1] < bt->corr_ptr[b]) return bad("corr_ptr not monotone");
      max_n = std::max(max_n, bt->corr_ptr[b + 1] - bt->corr_ptr[b]);
    }
    const size_t C = (size_t)bt->corr_ptr[B];
    if (C > 0 && (!bt->bearing || !bt->point_w || !bt->sigma_angle || !bt->inlier)) return bad("NULL correspondence array");
    for (size_t i = 0; i < 3 * C; ++i)
      if (!std::isfinite(bt->bearing[i]) || !std::isfinite(bt->point_w[i])) return bad("non-finite bearing or point");
    std::vector<unsigned long long> seeds(B);   // (the kernel's type for the 64-bit seeds)
    for (size_t b = 0; b < B; ++b) seeds[b] = bt->seed ? bt->seed[b] : opts->seed + (uint64_t)b;
    HIPCHK(hipSetDevice(c->device));
    DeviceScratch U(c->st);
    int *dptr_ = nullptr, *din = nullptr, *dit = nullptr, *dbd = nullptr;
    double *df = nullptr, *dP = nullptr, *ds = nullptr, *dT = nullptr;
    unsigned long long* dseed = nullptr;
    unsigned char* dmask = nullptr;
    HIPCHK(U.upload(&dptr_, bt->corr_ptr, B + 1));
    HIPCHK(U.upload(&df, bt->bearing, 3 * C)); HIPCHK(U.upload(&dP, bt->point_w, 3 * C)); HIPCHK(U.upload(&ds, bt->sigma_angle, C));
    HIPCHK(U.upload(&dseed, seeds.data(), B));
    HIPCHK(U.upload(&dT, bt->T_wc, 7 * B));   // untouched rows come back as they went
    HIPCHK(U.alloc(&dmask, C)); HIPCHK(U.alloc(&din, B)); HIPCHK(U.alloc(&dit, B)); HIPCHK(U.alloc(&dbd, B));
    launch_abspose((int)B, dptr_, df, dP, ds, dseed, dT, dmask, din, dit, dbd, opts->min_inliers, opts->max_iterations, opts->probability, opts->threshold,
                   max_n, c->st);
    HIPCHK(hipGetLastError());
    HIPCHK(U.fetch(bt->T_wc, dT, 7 * B)); HIPCHK(U.fetch(bt->inliers, din, B));
    HIPCHK(U.fetch(bt->iterations, dit, B)); HIPCHK(U.fetch(bt->best_draw, dbd, B));
    HIPCHK(U.fetch(bt->inlier, dmask, C));
    HIPCHK(hipStreamSynchronize(c->st));
    return COVGPU_OK;
  });
}

extern "C" int covgpu_p3p_batch(covgpu_context* c, int32_t n, const double* f, const double* P, double* T, int32_t* nsol, int32_t* chosen) {
  return batch_entry("covgpu_p3p_batch", c, [&](auto bad) -> int {
    if (n < 0) return bad("n < 0");
    if (n == 0) return COVGPU_OK;
    if (!f || !P || !T || !nsol || !chosen) return bad("NULL array");
    const size_t N = (size_t)n;
    for (size_t i = 0; i < 12 * N; ++i)
      if (!std::isfinite(f[i]) || !std::isfinite(P[i])) return bad("non-finite bearing or point");
    HIPCHK(hipSetDevice(c->device));
    DeviceScratch U(c->st);
    double *df, *dP, *dT; int *dn, *dc;
    HIPCHK(U.upload(&df, f, 12 * N)); HIPCHK(U.upload(&dP, P, 12 * N)); HIPCHK(U.zeroed(&dT, 28 * N));
    HIPCHK(U.alloc(&dn, N)); HIPCHK(U.alloc(&dc, N));
    launch_p3p(n, df, dP, dT, dn, dc, c->st);
    HIPCHK(hipGetLastError());
    HIPCHK(U.fetch(T, dT, 28 * N)); HIPCHK(U.fetch(nsol, dn, N)); HIPCHK(U.fetch(chosen, dc, N));
    HIPCHK(hipStreamSynchronize(c->st));
    return COVGPU_OK;
  });
}

extern "C" void covgpu_default_match_opts(covgpu_match_opts* o, int32_t mode) {
  if (!o) return;
  o->mode = mode;
  o->dist_threshold = mode == COVGPU_MATCH_KNN2 ? 40.0f : 50.0f;   // img_match_thres (config_backend.yaml:38); LandmarkMatchingAlgorithm(50.0)
  o->ratio = 0.8f;                                                 // ratio_thres (config_backend.yaml:39), KNN2 only
}

extern "C" int covgpu_match_batch(covgpu_context* c, const covgpu_match_batch_t* bt, const covgpu_match_opts* opts) {
  return batch_entry("covgpu_match_batch", c, [&](auto bad) -> int {
    if (!bt || !opts) return bad("NULL batch or options");
    if (opts->mode != COVGPU_MATCH_DENSE && opts->mode != COVGPU_MATCH_KNN2) return bad("unknown mode");
    if (!std::isfinite(opts->dist_threshold) || !(opts->dist_threshold > 0.0f)) return bad("dist_threshold not finite or not positive");
    if (!std::isfinite(opts->ratio) || !(opts->ratio > 0.0f)) return bad("ratio not finite or not positive");
    const bool dense = opts->mode == COVGPU_MATCH_DENSE;
    if (bt->num_sets < 0 || bt->num_jobs < 0) return bad("num_sets or num_jobs < 0");
    if (!dense && bt->skip) return bad("skip must be NULL in KNN2");
    if (bt->num_sets > 0 && !bt->row_ptr) return bad("NULL row_ptr");
    if (bt->num_sets > 0 && bt->row_ptr[0] != 0) return bad("row_ptr[0] != 0");
    for (int s = 0; s < bt->num_sets; ++s) {
      if (bt->row_ptr[s + 1] < bt->row_ptr[s]) return bad("row_ptr not monotone");
      if (bt->row_ptr[s + 1] - bt->row_ptr[s] > COVGPU_MATCH_MAX_ROWS) return bad("a set holds more than COVGPU_MATCH_MAX_ROWS rows");
    }
    const size_t R = bt->num_sets > 0 ? (size_t)bt->row_ptr[bt->num_sets] : 0;
    if (R > 0 && !bt->desc) return bad("NULL desc");
    const int J = bt->num_jobs;
    if (J > 0 && (!bt->set_a || !bt->set_b || !bt->nmatches)) return bad("NULL job array");
    std::vector<int32_t> off(J > 0 ? J : 1, 0);
    size_t totalA = 0;
    int maxA = 0, maxB = 0;
    for (int j = 0; j < J; ++j) {
      if (bt->set_a[j] < 0 || bt->set_a[j] >= bt->num_sets || bt->set_b[j] < 0 || bt->set_b[j] >= bt->num_sets) return bad("set index out of range");
      const int nA = bt->row_ptr[bt->set_a[j] + 1] - bt->row_ptr[bt->set_a[j]];
      off[j] = (int32_t)totalA;
      totalA += (size_t)nA;
      if (totalA > (size_t)INT32_MAX) return bad("more than 2^31 - 1 output rows");
      maxA = std::max(maxA, nA);
      maxB = std::max(maxB, bt->row_ptr[bt->set_b[j] + 1] - bt->row_ptr[bt->set_b[j]]);
    }
    if (totalA > 0 && !bt->match) return bad("NULL match");
    if (J == 0) return COVGPU_OK;
    const int tiles = (maxA + kMatchScanRows - 1) / kMatchScanRows;  // scan workgroups per job (launch_match): one 1-D grid of J * tiles
    if ((int64_t)J * tiles > (int64_t)INT32_MAX) return bad("num_jobs * ceil(max query rows / 256) exceeds 2^31 - 1 workgroups");
    HIPCHK(hipSetDevice(c->device));
    int dcut = 0;                                                    // (float)d < dist_threshold  <=>  d < dcut, for d in 0..256
    while (dcut <= 256 && (float)dcut < opts->dist_threshold) ++dcut;
    DeviceScratch U(c->st);
    unsigned char *ddesc = nullptr, *dskip = nullptr;
    int *dptr_ = nullptr, *dsa = nullptr, *dsb = nullptr, *doff = nullptr, *dlist = nullptr, *dmatch = nullptr, *ddist = nullptr, *dn = nullptr;
    HIPCHK(U.upload(&ddesc, bt->desc, 32 * R));
    if (dense && bt->skip) HIPCHK(U.upload(&dskip, bt->skip, R));
    HIPCHK(U.upload(&dptr_, bt->row_ptr, (size_t)bt->num_sets + 1));
    HIPCHK(U.upload(&dsa, bt->set_a, (size_t)J)); HIPCHK(U.upload(&dsb, bt->set_b, (size_t)J)); HIPCHK(U.upload(&doff, off.data(), (size_t)J));
    if (dense) HIPCHK(U.alloc(&dlist, 4 * totalA));                  // the 4 best of every query row
    HIPCHK(U.alloc(&dmatch, totalA)); HIPCHK(U.alloc(&ddist, totalA)); HIPCHK(U.zeroed(&dn, (size_t)J));
    launch_match(opts->mode, J, maxA, maxB, ddesc, dskip, dptr_, dsa, dsb, doff, dlist, dmatch, ddist, dn, dcut, opts->dist_threshold, opts->ratio,
                 c->st);
    HIPCHK(hipGetLastError());
    HIPCHK(U.fetch(bt->match, dmatch, totalA)); HIPCHK(U.fetch(bt->dist, ddist, totalA)); HIPCHK(U.fetch(bt->nmatches, dn, (size_t)J));
    HIPCHK(hipStreamSynchronize(c->st));
    return COVGPU_OK;
  });
}

extern "C" void covgpu_default_match_float_opts(covgpu_match_opts* o) {
  if (!o) return;
  o->mode = COVGPU_MATCH_KNN2;
  o->dist_threshold = 500.0f;                                      // img_match_thres, "use 500 for SIFT" (config_backend.yaml:38)
  o->ratio = 0.8f;                                                 // ratio_thres (config_backend.yaml:39)
}

extern "C" void covgpu_match_float_limits(int32_t out[4]) {
  if (!out) return;
  out[0] = COVGPU_MATCH_MAX_ROWS; out[1] = kMatchFloatMaxDim; out[2] = kMatchFloatTileRows; out[3] = kMatchFloatChunkRows;
}

namespace {

// What covgpu_match_float_batch derives from its arguments while it checks them.
struct MatchFloatPlan { size_t rows = 0, total_a = 0; int max_a = 0; std::vector<int32_t> off; };

// All checks of covgpu_match_float_batch; the message of the first violation, or nullptr.
const char* match_float_check(const covgpu_match_float_batch_t* bt, const covgpu_match_opts* opts, MatchFloatPlan& P) {
  if (!bt || !opts) return "NULL batch or options";
  if (opts->mode != COVGPU_MATCH_KNN2) return "mode must be COVGPU_MATCH_KNN2";
  if (!std::isfinite(opts->dist_threshold) || !(opts->dist_threshold > 0.0f)) return "dist_threshold not finite or not positive";
  if (!std::isfinite(opts->ratio) || !(opts->ratio > 0.0f)) return "ratio not finite or not positive";
  if (bt->dim <= 0 || bt->dim % 4 != 0 || bt->dim > kMatchFloatMaxDim) return "dim must be a positive multiple of 4 up to 256";
  if (bt->num_sets < 0 || bt->num_jobs < 0) return "num_sets or num_jobs < 0";
  if (bt->num_sets > 0 && !bt->row_ptr) return "NULL row_ptr";
  if (bt->num_sets > 0 && bt->row_ptr[0] != 0) return "row_ptr[0] != 0";
  for (int s = 0; s < bt->num_sets; ++s) {
    if (bt->row_ptr[s + 1] < bt->row_ptr[s]) return "row_ptr not monotone";
    if (bt->row_ptr[s + 1] - bt->row_ptr[s] > COVGPU_MATCH_MAX_ROWS) return "a set holds more than COVGPU_MATCH_MAX_ROWS rows";
  }
  P.rows = bt->num_sets > 0 ? (size_t)bt->row_ptr[bt->num_sets] : 0;
  if (P.rows > 0 && !bt->desc) return "NULL desc";
  const int J = bt->num_jobs;
  if (J > 0 && (!bt->set_a || !bt->set_b || !bt->nmatches)) return "NULL job array";
  P.off.assign(J > 0 ? J : 1, 0);
  for (int j = 0; j < J; ++j) {
    if (bt->set_a[j] < 0 || bt->set_a[j] >= bt->num_sets || bt->set_b[j] < 0 || bt->set_b[j] >= bt->num_sets) return "set index out of range";
    const int nA = bt->row_ptr[bt->set_a[j] + 1] - bt->row_ptr[bt->set_a[j]];
    P.off[j] = (int32_t)P.total_a;
    P.total_a += (size_t)nA;
    if (P.total_a > (size_t)INT32_MAX) return "more than 2^31 - 1 output rows";
    P.max_a = std::max(P.max_a, nA);
  }
  if (P.total_a > 0 && !bt->match) return "NULL match";
  const int tiles = (P.max_a + kMatchFloatTileRows - 1) / kMatchFloatTileRows;   // scan workgroups per job (launch_matchf)
  if ((int64_t)J * tiles > (int64_t)INT32_MAX) return "num_jobs * ceil(max query rows / 128) exceeds 2^31 - 1 workgroups";
  // a NaN would leave the order by (distance, index) undefined, and |x|^2 has to stay finite in float32
  for (size_t i = 0; i < P.rows * (size_t)bt->dim; ++i)
    if (!(std::fabs(bt->desc[i]) <= kMatchFloatMaxAbs)) return "descriptor value not finite or above 1e18 in magnitude";
  return nullptr;
}

}  // namespace

extern "C" int covgpu_match_float_check(const covgpu_match_float_batch_t* bt, const covgpu_match_opts* opts) {
  return guarded([&]() -> int {
    MatchFloatPlan P;
    if (const char* m = match_float_check(bt, opts, P)) { g_err = std::string("covgpu_match_float_check: ") + m; return COVGPU_ERR_INVALID_ARG; }
    return COVGPU_OK;
  });
}

extern "C" int covgpu_match_float_batch(covgpu_context* c, const covgpu_match_float_batch_t* bt, const covgpu_match_opts* opts) {
  return batch_entry("covgpu_match_float_batch", c, [&](auto bad) -> int {
    MatchFloatPlan P;
    if (const char* m = match_float_check(bt, opts, P)) return bad(m);
    const int J = bt->num_jobs;
    if (J == 0) return COVGPU_OK;
    const size_t R = P.rows, totalA = P.total_a;
    HIPCHK(hipSetDevice(c->device));
    DeviceScratch U(c->st);
    float *ddesc = nullptr, *dnorm = nullptr, *ddist = nullptr;
    int *dptr_ = nullptr, *dsa = nullptr, *dsb = nullptr, *doff = nullptr, *dmatch = nullptr, *dn = nullptr;
    HIPCHK(U.upload(&ddesc, bt->desc, R * (size_t)bt->dim));         // every set once, however many jobs name it
    HIPCHK(U.alloc(&dnorm, R));
    HIPCHK(U.upload(&dptr_, bt->row_ptr, (size_t)bt->num_sets + 1));
    HIPCHK(U.upload(&dsa, bt->set_a, (size_t)J)); HIPCHK(U.upload(&dsb, bt->set_b, (size_t)J)); HIPCHK(U.upload(&doff, P.off.data(), (size_t)J));
    HIPCHK(U.alloc(&dmatch, totalA)); HIPCHK(U.alloc(&ddist, totalA)); HIPCHK(U.zeroed(&dn, (size_t)J));
    launch_matchf_norms((int)R, bt->dim, ddesc, dnorm, c->st);
    launch_matchf(J, P.max_a, bt->dim, ddesc, dnorm, dptr_, dsa, dsb, doff, dmatch, ddist, dn, opts->dist_threshold, opts->ratio, c->st);
    HIPCHK(hipGetLastError());
    HIPCHK(U.fetch(bt->match, dmatch, totalA)); HIPCHK(U.fetch(bt->dist, ddist, totalA)); HIPCHK(U.fetch(bt->nmatches, dn, (size_t)J));
    HIPCHK(hipStreamSynchronize(c->st));
    return COVGPU_OK;
  });
}

extern "C" void covgpu_default_guided_opts(covgpu_guided_opts* o, int32_t mode) {
  if (!o) return;
  o->th_low = 50;                                                  // desc_matching_th_low_ (feature_matcher_be.hpp)
  o->radius = mode == COVGPU_GUIDED_PROJECTION ? 10.0 : 9.5;       // config_backend.yaml:45-50
  o->scale_factor = 2.0; o->num_octaves = 1;                       // features::scale_factor, features::num_octaves
  o->agreement = 0;
}

namespace {

// Checks shared by the two guided entry points; the message of the first violation, or nullptr.
const char* guided_check(const covgpu_keypoint_sets_t& s, const covgpu_guided_opts* o) {
  if (!o) return "NULL options";
  if (o->th_low < 0 || o->th_low > 255) return "th_low outside [0, 255]";
  if (!std::isfinite(o->radius) || !(o->radius > 0.0)) return "radius not finite or not positive";
  if (o->num_octaves < 1) return "num_octaves < 1";
  if (o->num_octaves > 1 && (!std::isfinite(o->scale_factor) || !(o->scale_factor > 1.0))) return "scale_factor not finite or not above 1";
  if (o->agreement != 0 && o->agreement != 1) return "agreement is neither 0 nor 1";
  if (s.num_sets < 0) return "num_sets < 0";
  if (s.num_sets > 0 && !s.row_ptr) return "NULL row_ptr";
  if (s.num_sets > 0 && s.row_ptr[0] != 0) return "row_ptr[0] != 0";
  for (int i = 0; i < s.num_sets; ++i) {
    if (s.row_ptr[i + 1] < s.row_ptr[i]) return "row_ptr not monotone";
    if (s.row_ptr[i + 1] - s.row_ptr[i] > COVGPU_MATCH_MAX_ROWS) return "a set holds more than COVGPU_MATCH_MAX_ROWS rows";
  }
  if (s.num_sets > 0 && !s.bounds) return "NULL bounds";
  if (s.num_sets > 0 && s.row_ptr[s.num_sets] > 0 && (!s.kp || !s.level || !s.desc)) return "NULL keypoint array";
  return nullptr;
}

// Device records of the keypoints: {x, y, level, visiting rank}. Grid order is ascending (cell_x, cell_y, index) with the cell of
// AssignFeaturesToGrid (keyframe_base.cpp:134-139) clamped to the 64 x 48 grid; index order when the set has no grid. A taken keypoint
// (SearchByProjection's vpMatched[idx] != NULL) gets level INT_MIN and so fails every level window.
std::vector<int4> guided_records(const covgpu_keypoint_sets_t& s, const uint8_t* taken) {
  const size_t R = s.num_sets > 0 ? (size_t)s.row_ptr[s.num_sets] : 0;
  std::vector<int4> rec(R);
  std::vector<int> cell, order;
  for (int i = 0; i < s.num_sets; ++i) {
    const int r0 = s.row_ptr[i], n = s.row_ptr[i + 1] - r0;
    order.resize(n);
    for (int k = 0; k < n; ++k) order[k] = k;
    if (s.grid_inv && s.grid_inv[2 * i] > 0.0) {
      cell.resize(n);
      for (int k = 0; k < n; ++k) {
        const double cx = std::round((double)s.kp[2 * (size_t)(r0 + k)] * s.grid_inv[2 * i]);
        const double cy = std::round((double)s.kp[2 * (size_t)(r0 + k) + 1] * s.grid_inv[2 * i + 1]);
        const int ix = cx >= 0.0 ? (cx <= 63.0 ? (int)cx : 63) : 0, iy = cy >= 0.0 ? (cy <= 47.0 ? (int)cy : 47) : 0;   // (a NaN goes to cell 0)
        cell[k] = ix * 48 + iy;
      }
      std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return cell[a] < cell[b]; });
    }
    for (int rank = 0; rank < n; ++rank) {
      const size_t r = (size_t)r0 + order[rank];
      int4 e;
      std::memcpy(&e.x, &s.kp[2 * r], 4); std::memcpy(&e.y, &s.kp[2 * r + 1], 4);
      e.z = (taken && taken[r]) ? INT32_MIN : s.level[r];
      e.w = rank;
      rec[r] = e;
    }
  }
  return rec;
}

}  // namespace
// (the 32-byte descriptors below go up as the kernels read them: two uint4 a row)

extern "C" int covgpu_search_se3_batch(covgpu_context* c, const covgpu_search_se3_batch_t* bt, const covgpu_guided_opts* opts) {
  return batch_entry("covgpu_search_se3_batch", c, [&](auto bad) -> int {
    if (!bt) return bad("NULL batch");
    if (const char* m = guided_check(bt->sets, opts)) return bad(m);
    const covgpu_keypoint_sets_t& s = bt->sets;
    const int S = s.num_sets, J = bt->num_jobs;
    const size_t R = S > 0 ? (size_t)s.row_ptr[S] : 0;
    if (J < 0) return bad("num_jobs < 0");
    if (S > 0 && !bt->K) return bad("NULL K");
    if (R > 0 && (!bt->lm_pos || !bt->lm_max_distance || !bt->lm_desc || !bt->lm_free)) return bad("NULL landmark array");
    if (J > 0 && (!bt->set_1 || !bt->set_2 || !bt->T12 || !bt->nfound)) return bad("NULL job array");
    std::vector<int32_t> off1(J > 0 ? J : 1, 0), off2(J > 0 ? J : 1, 0);
    std::vector<int4> tiles;
    size_t tot1 = 0, tot2 = 0;
    for (int j = 0; j < J; ++j) {
      if (bt->set_1[j] < 0 || bt->set_1[j] >= S || bt->set_2[j] < 0 || bt->set_2[j] >= S) return bad("set index out of range");
      for (int k = 0; k < 7; ++k) if (!std::isfinite(bt->T12[7 * (size_t)j + k])) return bad("non-finite T12");
      const int n1 = s.row_ptr[bt->set_1[j] + 1] - s.row_ptr[bt->set_1[j]], n2 = s.row_ptr[bt->set_2[j] + 1] - s.row_ptr[bt->set_2[j]];
      off1[j] = (int32_t)tot1; off2[j] = (int32_t)tot2;
      tot1 += (size_t)n1; tot2 += (size_t)n2;
      if (tot1 > (size_t)INT32_MAX || tot2 > (size_t)INT32_MAX) return bad("more than 2^31 - 1 output rows");
      for (int dir = 0; dir < 2; ++dir)
        for (int f = 0, n = dir ? n2 : n1; f < n; f += kGuidedScanPoints) tiles.push_back(make_int4(j, dir, f, std::min(kGuidedScanPoints, n - f)));
      if (tiles.size() > (size_t)INT32_MAX) return bad("more than 2^31 - 1 scan workgroups");
    }
    if (tot1 > 0 && !bt->match) return bad("NULL match");
    if (J == 0) return COVGPU_OK;
    HIPCHK(hipSetDevice(c->device));
    const std::vector<int4> rec = guided_records(s, nullptr);
    const size_t Ss = (size_t)S, Js = (size_t)J;
    DeviceScratch U(c->st);
    GuidedSe3Args A{};
    HIPCHK(U.upload(&A.S.kpr, rec.data(), R)); HIPCHK(U.upload(&A.S.kdesc, (const uint4*)s.desc, 2 * R));
    HIPCHK(U.upload(&A.S.row_ptr, s.row_ptr, Ss + 1)); HIPCHK(U.upload(&A.S.bounds, s.bounds, 4 * Ss));
    HIPCHK(U.upload(&A.K, bt->K, 4 * Ss)); HIPCHK(U.upload(&A.lm_pos, bt->lm_pos, 3 * R));
    HIPCHK(U.upload(&A.lm_maxd, bt->lm_max_distance, R)); HIPCHK(U.upload(&A.lm_desc, (const uint4*)bt->lm_desc, 2 * R));
    HIPCHK(U.upload(&A.lm_free, bt->lm_free, R));
    HIPCHK(U.upload(&A.set_1, bt->set_1, Js)); HIPCHK(U.upload(&A.set_2, bt->set_2, Js));
    HIPCHK(U.upload(&A.T12, bt->T12, 7 * Js));
    HIPCHK(U.upload(&A.off1, off1.data(), Js)); HIPCHK(U.upload(&A.off2, off2.data(), Js));
    const int4* dtiles = nullptr;
    HIPCHK(U.upload(&dtiles, tiles.data(), tiles.size()));
    HIPCHK(U.alloc(&A.m1, tot1)); HIPCHK(U.alloc(&A.m2, tot2)); HIPCHK(U.alloc(&A.match, tot1));
    HIPCHK(U.zeroed(&A.nfound, Js));
    const GuidedOptsDev O{opts->th_low, opts->radius, opts->scale_factor, std::log(opts->scale_factor), opts->num_octaves, opts->agreement};
    launch_guided_se3(A, O, J, dtiles, (int)tiles.size(), c->st);
    HIPCHK(hipGetLastError());
    HIPCHK(U.fetch(bt->match, A.match, tot1)); HIPCHK(U.fetch(bt->match1, A.m1, tot1)); HIPCHK(U.fetch(bt->match2, A.m2, tot2));
    HIPCHK(U.fetch(bt->nfound, A.nfound, Js));
    HIPCHK(hipStreamSynchronize(c->st));
    return COVGPU_OK;
  });
}

extern "C" int covgpu_search_projection_batch(covgpu_context* c, const covgpu_search_projection_batch_t* bt, const covgpu_guided_opts* opts) {
  return batch_entry("covgpu_search_projection_batch", c, [&](auto bad) -> int {
    if (!bt) return bad("NULL batch");
    if (const char* m = guided_check(bt->sets, opts)) return bad(m);
    const covgpu_keypoint_sets_t& s = bt->sets;
    const int S = s.num_sets, J = bt->num_jobs;
    const size_t R = S > 0 ? (size_t)s.row_ptr[S] : 0;
    if (J < 0) return bad("num_jobs < 0");
    if (S > 0 && (!bt->cam || !bt->dist_type)) return bad("NULL camera array");
    for (int i = 0; i < S; ++i) {
      if (bt->dist_type[i] != COVGPU_DIST_RADTAN && bt->dist_type[i] != COVGPU_DIST_EQUIDISTANT) return bad("unknown distortion type");
      if (!bt->cam_model || bt->cam_model[i] == COVGPU_CAM_PINHOLE) continue;
      if (bt->cam_model[i] != COVGPU_CAM_UNIFIED) return bad("unknown camera model");
      if (!bt->xi) return bad("unified camera without xi");
      if (!std::isfinite(bt->xi[i]) || bt->xi[i] < 0.0) return bad("xi of a unified camera is negative or not finite");
    }
    if (J > 0 && (!bt->set || !bt->T_cw || !bt->point_ptr || !bt->nmatches)) return bad("NULL job array");
    if (J > 0 && bt->point_ptr[0] != 0) return bad("point_ptr[0] != 0");
    std::vector<int4> tiles;
    for (int j = 0; j < J; ++j) {
      if (bt->set[j] < 0 || bt->set[j] >= S) return bad("set index out of range");
      if (bt->point_ptr[j + 1] < bt->point_ptr[j]) return bad("point_ptr not monotone");
      for (int k = 0; k < 7; ++k) if (!std::isfinite(bt->T_cw[7 * (size_t)j + k])) return bad("non-finite T_cw");
      for (int f = 0, n = bt->point_ptr[j + 1] - bt->point_ptr[j]; f < n; f += kGuidedScanPoints)
        tiles.push_back(make_int4(j, 0, f, std::min(kGuidedScanPoints, n - f)));
    }
    const size_t P = J > 0 ? (size_t)bt->point_ptr[J] : 0;
    if (P > 0 && (!bt->p_w || !bt->normal || !bt->min_distance || !bt->max_distance || !bt->p_desc || !bt->claimed || !bt->remap_to))
      return bad("NULL point array");
    if (bt->existing_idx)
      for (int j = 0; j < J; ++j) {
        const int n = s.row_ptr[bt->set[j] + 1] - s.row_ptr[bt->set[j]];
        for (int p = bt->point_ptr[j]; p < bt->point_ptr[j + 1]; ++p)
          if (bt->existing_idx[p] < -1 || bt->existing_idx[p] >= n) return bad("existing_idx out of range");
      }
    if (J == 0) return COVGPU_OK;
    HIPCHK(hipSetDevice(c->device));
    const std::vector<int4> rec = guided_records(s, bt->taken);
    const size_t Ss = (size_t)S, Js = (size_t)J;
    DeviceScratch U(c->st);
    GuidedProjArgs A{};
    HIPCHK(U.upload(&A.S.kpr, rec.data(), R)); HIPCHK(U.upload(&A.S.kdesc, (const uint4*)s.desc, 2 * R));
    HIPCHK(U.upload(&A.S.row_ptr, s.row_ptr, Ss + 1)); HIPCHK(U.upload(&A.S.bounds, s.bounds, 4 * Ss));
    HIPCHK(U.upload(&A.cam, bt->cam, 8 * Ss)); HIPCHK(U.upload(&A.dist_type, bt->dist_type, Ss));
    std::vector<double> xi(S, 0.0);                                    // 0 for the pinhole rows, whose xi is not read
    if (bt->cam_model) {
      for (int i = 0; i < S; ++i) if (bt->cam_model[i] == COVGPU_CAM_UNIFIED) xi[i] = bt->xi[i];
      HIPCHK(U.upload(&A.cam_model, bt->cam_model, Ss)); HIPCHK(U.upload(&A.xi, xi.data(), Ss));
    }
    HIPCHK(U.upload(&A.set, bt->set, Js)); HIPCHK(U.upload(&A.T_cw, bt->T_cw, 7 * Js));
    HIPCHK(U.upload(&A.point_ptr, bt->point_ptr, Js + 1));
    HIPCHK(U.upload(&A.p_w, bt->p_w, 3 * P)); HIPCHK(U.upload(&A.normal, bt->normal, 3 * P));
    HIPCHK(U.upload(&A.min_d, bt->min_distance, P)); HIPCHK(U.upload(&A.max_d, bt->max_distance, P));
    HIPCHK(U.upload(&A.p_desc, (const uint4*)bt->p_desc, 2 * P));
    if (bt->skip) HIPCHK(U.upload(&A.skip, bt->skip, P));
    if (bt->existing_idx) HIPCHK(U.upload(&A.existing, bt->existing_idx, P));
    const int4* dtiles = nullptr;
    HIPCHK(U.upload(&dtiles, tiles.data(), tiles.size()));
    HIPCHK(U.alloc(&A.lists, kGuidedListCap * P)); HIPCHK(U.alloc(&A.cnt, P)); HIPCHK(U.alloc(&A.target, 2 * P));
    HIPCHK(U.alloc(&A.rad, P)); HIPCHK(U.alloc(&A.lvl, P)); HIPCHK(U.alloc(&A.dold, P));
    HIPCHK(U.alloc(&A.claimed, P)); HIPCHK(U.alloc(&A.remap_to, P)); HIPCHK(U.alloc(&A.best_dist, P));
    HIPCHK(U.alloc(&A.nmatches, Js));
    const GuidedOptsDev O{opts->th_low, opts->radius, opts->scale_factor, std::log(opts->scale_factor), opts->num_octaves, opts->agreement};
    launch_guided_projection(A, O, J, dtiles, (int)tiles.size(), c->st);
    HIPCHK(hipGetLastError());
    HIPCHK(U.fetch(bt->claimed, A.claimed, P)); HIPCHK(U.fetch(bt->remap_to, A.remap_to, P)); HIPCHK(U.fetch(bt->best_dist, A.best_dist, P));
    HIPCHK(U.fetch(bt->nmatches, A.nmatches, Js));
    HIPCHK(hipStreamSynchronize(c->st));
    return COVGPU_OK;
  });
}

extern "C" int covgpu_pgo_reanchor(covgpu_context* c, int32_t K, const double* pose_old, const double* pose_new, double* velocity, int32_t L,
                                   const int32_t* ref_kf, double* lm_pos) {
  return batch_entry("covgpu_pgo_reanchor", c, [&](auto bad) -> int {
    if (K < 0 || L < 0 || (K > 0 && (!pose_old || !pose_new)) || (L > 0 && (!ref_kf || !lm_pos))) return bad("NULL array");
    for (int l = 0; l < L; ++l) if (ref_kf[l] >= K) return bad("ref_kf out of range");
    HIPCHK(hipSetDevice(c->device));
    const size_t Ks = (size_t)K, Ls = (size_t)L;
    DeviceScratch U(c->st);
    double *dpo, *dpn, *dv = nullptr, *dl; int* dr;
    HIPCHK(U.upload(&dpo, pose_old, 7 * Ks)); HIPCHK(U.upload(&dpn, pose_new, 7 * Ks));
    HIPCHK(U.upload(&dl, lm_pos, 3 * Ls)); HIPCHK(U.upload(&dr, ref_kf, Ls));
    if (velocity) HIPCHK(U.upload(&dv, velocity, 3 * Ks));
    launch_reanchor(K, dpo, dpn, dv, L, dr, dl, c->st);
    HIPCHK(U.fetch(lm_pos, dl, 3 * Ls)); HIPCHK(U.fetch(velocity, dv, 3 * Ks));
    HIPCHK(hipStreamSynchronize(c->st));
    return COVGPU_OK;
  });
}

// ---- bag-of-words retrieval (k_bow.hip) ----
// (the two checks are shared with bowdb.hip: declared in host.hpp)

// The first violation of a bow CSR over `rows` rows (word ids ascending and duplicate-free, values finite), or nullptr.
const char* bow_csr_check(int rows, const int32_t* ptr, const int32_t* word, const double* value) {
  if (rows < 0) return "negative row count";
  if (rows == 0) return nullptr;
  if (!ptr) return "NULL bow_ptr";
  if (ptr[0] != 0) return "bow_ptr[0] != 0";
  for (int r = 0; r < rows; ++r) if (ptr[r + 1] < ptr[r]) return "bow_ptr not monotone";
  if (ptr[rows] > 0 && (!word || !value)) return "NULL word or value";
  for (int r = 0; r < rows; ++r)
    for (int i = ptr[r]; i < ptr[r + 1]; ++i) {
      if (word[i] < 0) return "negative word id";
      if (i > ptr[r] && word[i] <= word[i - 1]) return "word ids of a bow row not ascending and duplicate-free";
      if (!std::isfinite(value[i])) return "non-finite bow value";
    }
  return nullptr;
}

// The first violation of the vocabulary's tree shape, or nullptr.
const char* bow_vocab_check(const covgpu_bow_vocab_t* v) {
  if (!v) return "NULL vocabulary";
  if (v->scoring != COVGPU_BOW_L1_NORM) return "only L1_NORM scoring is supported";
  if (v->weighting < COVGPU_BOW_TF_IDF || v->weighting > COVGPU_BOW_BINARY) return "unknown weighting";
  const int N = v->num_nodes, W = v->num_words;
  if (N < 2) return "the vocabulary has no node below the root";
  if (W < 1 || W > COVGPU_BOW_MAX_WORDS) return "num_words is not in 1..COVGPU_BOW_MAX_WORDS";
  if (v->k < 1 || v->L < 0) return "k < 1 or L < 0";
  if (!v->parent || !v->child_ptr || !v->child || !v->desc || !v->word_id || !v->weight) return "NULL vocabulary array";
  if (v->parent[0] != -1) return "parent[0] != -1";
  for (int n = 1; n < N; ++n) if (v->parent[n] < 0 || v->parent[n] >= n) return "parent[n] is not in 0..n-1";
  if (v->child_ptr[0] != 0) return "child_ptr[0] != 0";
  for (int n = 0; n < N; ++n) if (v->child_ptr[n + 1] < v->child_ptr[n]) return "child_ptr not monotone";
  if (v->child_ptr[N] != N - 1) return "child_ptr[num_nodes] != num_nodes - 1";
  std::vector<uint8_t> seen(W, 0);
  for (int n = 0; n < N; ++n) {
    for (int i = v->child_ptr[n]; i < v->child_ptr[n + 1]; ++i) {
      const int c = v->child[i];
      if (c <= 0 || c >= N) return "child index out of range";
      if (v->parent[c] != n) return "child lists inconsistent with parent";
      if (i > v->child_ptr[n] && c <= v->child[i - 1]) return "children not in ascending (line) order";
    }
    const bool leaf = v->child_ptr[n + 1] == v->child_ptr[n];
    if (leaf != (v->word_id[n] >= 0)) return "leaves are not exactly the nodes with a word id";
    if (leaf) {
      if (v->word_id[n] >= W) return "word id out of range";
      if (seen[v->word_id[n]]) return "word ids are not a permutation of 0..num_words-1";
      seen[v->word_id[n]] = 1;
    }
    if (!std::isfinite(v->weight[n])) return "non-finite weight";
  }
  for (int w = 0; w < W; ++w) if (!seen[w]) return "word ids are not a permutation of 0..num_words-1";
  return nullptr;
}

extern "C" int covgpu_bow_transform_batch(covgpu_context* c, const covgpu_bow_vocab_t* v, const covgpu_bow_transform_batch_t* bt) {
  return batch_entry("covgpu_bow_transform_batch", c, [&](auto bad) -> int {
    if (!bt) return bad("NULL batch");
    if (const char* m = bow_vocab_check(v)) return bad(m);
    const int S = bt->num_sets;
    if (S < 0 || bt->capacity < 0) return bad("num_sets or capacity < 0");
    if (S > 0 && (!bt->row_ptr || !bt->bow_ptr)) return bad("NULL row_ptr or bow_ptr");
    if (S > 0 && bt->row_ptr[0] != 0) return bad("row_ptr[0] != 0");
    for (int s = 0; s < S; ++s) {
      if (bt->row_ptr[s + 1] < bt->row_ptr[s]) return bad("row_ptr not monotone");
      if (bt->row_ptr[s + 1] - bt->row_ptr[s] > COVGPU_MATCH_MAX_ROWS) return bad("a set holds more than COVGPU_MATCH_MAX_ROWS rows");
    }
    const size_t R = S > 0 ? (size_t)bt->row_ptr[S] : 0;
    if (R > 0 && !bt->desc) return bad("NULL desc");
    if (bt->capacity > 0 && (!bt->word || !bt->value)) return bad("NULL word or value");
    if (bt->total) *bt->total = 0;
    if (S == 0) return COVGPU_OK;
    const size_t N = (size_t)v->num_nodes, W = (size_t)v->num_words, Ss = (size_t)S;
    std::vector<double> ww(W);
    for (size_t n = 0; n < N; ++n) if (v->word_id[n] >= 0) ww[v->word_id[n]] = v->weight[n];
    // each set's words sit at its first row; the exact CSR is packed from one download (declared before the scratch that fills them)
    std::vector<int32_t> hw(R), hc(S);
    std::vector<double> hv(R);
    HIPCHK(hipSetDevice(c->device));
    DeviceScratch U(c->st);
    BowVocabDev V{};
    V.num_nodes = (int)N;
    HIPCHK(U.upload(&V.child_ptr, v->child_ptr, N + 1)); HIPCHK(U.upload(&V.child, v->child, N - 1));
    HIPCHK(U.upload(&V.desc, (const uint4*)v->desc, 2 * N)); HIPCHK(U.upload(&V.word_id, v->word_id, N));
    HIPCHK(U.upload(&V.word_weight, ww.data(), W));
    unsigned char* ddesc = nullptr;
    int *dptr_ = nullptr, *drw = nullptr, *drn = nullptr, *dow = nullptr, *dcnt = nullptr;
    double* dov = nullptr;
    HIPCHK(U.upload(&ddesc, bt->desc, 32 * R)); HIPCHK(U.upload(&dptr_, bt->row_ptr, Ss + 1));
    HIPCHK(U.alloc(&drw, R)); HIPCHK(U.alloc(&drn, R)); HIPCHK(U.alloc(&dow, R));
    HIPCHK(U.alloc(&dov, R)); HIPCHK(U.alloc(&dcnt, Ss));
    const int add_weight = v->weighting == COVGPU_BOW_TF_IDF || v->weighting == COVGPU_BOW_TF;
    launch_bow_transform(V, ddesc, dptr_, S, (int)R, v->L - bt->levelsup, add_weight, drw, drn, dow, dov, dcnt, c->st);
    HIPCHK(hipGetLastError());
    HIPCHK(U.fetch(hw.data(), dow, R)); HIPCHK(U.fetch(hv.data(), dov, R));
    HIPCHK(U.fetch(bt->row_word, drw, R)); HIPCHK(U.fetch(bt->row_node, drn, R));
    HIPCHK(U.fetch(hc.data(), dcnt, Ss));
    HIPCHK(hipStreamSynchronize(c->st));
    int64_t tot = 0;
    bt->bow_ptr[0] = 0;
    for (int s = 0; s < S; ++s) {
      const int64_t room = std::max<int64_t>(0, std::min<int64_t>(hc[s], (int64_t)bt->capacity - tot));
      if (room > 0) {
        std::memcpy(bt->word + tot, hw.data() + bt->row_ptr[s], 4 * (size_t)room);
        std::memcpy(bt->value + tot, hv.data() + bt->row_ptr[s], 8 * (size_t)room);
      }
      tot += hc[s];
      bt->bow_ptr[s + 1] = (int32_t)tot;                                // tot <= rows <= 2^31 - 1
    }
    if (bt->total) *bt->total = tot;
    return COVGPU_OK;
  });
}

extern "C" int covgpu_bow_score_pairs(covgpu_context* c, int32_t num_vec, const int32_t* bow_ptr, const int32_t* word, const double* value,
                                      int32_t num_pairs, const int32_t* a, const int32_t* b, double* score) {
  return batch_entry("covgpu_bow_score_pairs", c, [&](auto bad) -> int {
    if (const char* m = bow_csr_check(num_vec, bow_ptr, word, value)) return bad(m);
    if (num_pairs < 0) return bad("num_pairs < 0");
    if (num_pairs > 0 && (!a || !b || !score)) return bad("NULL pair array");
    for (int i = 0; i < num_pairs; ++i)
      if (a[i] < 0 || a[i] >= num_vec || b[i] < 0 || b[i] >= num_vec) return bad("pair index out of range");
    if (num_pairs == 0) return COVGPU_OK;
    HIPCHK(hipSetDevice(c->device));
    const size_t nnz = (size_t)bow_ptr[num_vec], P = (size_t)num_pairs;
    DeviceScratch U(c->st);
    int *dp = nullptr, *dw = nullptr, *da = nullptr, *db = nullptr;
    double *dv = nullptr, *ds = nullptr;
    HIPCHK(U.upload(&dp, bow_ptr, (size_t)num_vec + 1)); HIPCHK(U.upload(&dw, word, nnz)); HIPCHK(U.upload(&dv, value, nnz));
    HIPCHK(U.upload(&da, a, P)); HIPCHK(U.upload(&db, b, P)); HIPCHK(U.alloc(&ds, P));
    launch_bow_score_pairs(dp, dp + 1, dw, dv, num_pairs, da, db, ds, c->st);
    HIPCHK(hipGetLastError());
    HIPCHK(U.fetch(score, ds, P));
    HIPCHK(hipStreamSynchronize(c->st));
    return COVGPU_OK;
  });
}

extern "C" void covgpu_default_detect_opts(covgpu_detect_opts* o, int32_t mode) {
  if (!o) return;
  o->min_score_factor = mode == COVGPU_DETECT_COVINS_G ? 0.7 : 0.8;  // placerec_gen_be.cpp / placerec_be.cpp:389
  o->min_loop_dist = 100;                                            // config_backend.yaml:72-78
  o->exclude_kfs_with_id_less_than = 7;
  o->inter_map_matches_only = 0;
  o->scratch_kib = 0;
}

extern "C" int covgpu_detect_candidates_batch(covgpu_context* c, const covgpu_detect_batch_t* bt, const covgpu_detect_opts* opts) {
  return batch_entry("covgpu_detect_candidates_batch", c, [&](auto bad) -> int {
    if (!bt || !opts) return bad("NULL batch or options");
    if (!std::isfinite(opts->min_score_factor)) return bad("non-finite min_score_factor");
    if (opts->scratch_kib < 0) return bad("scratch_kib < 0");
    const int N = bt->num_kf, M = bt->num_db, Q = bt->num_queries, cap = bt->cap;
    if (N < 0 || M < 0 || Q < 0 || cap < 0) return bad("negative count");
    if (N > 0 && (!bt->id || !bt->client || !bt->nb_ptr)) return bad("NULL keyframe array");
    for (int k = 0; k < N; ++k) if (bt->id[k] < 0) return bad("negative keyframe id");
    if (const char* m = bow_csr_check(N, bt->bow_ptr, bt->word, bt->value)) return bad(m);
    if (N > 0 && bt->nb_ptr[0] != 0) return bad("nb_ptr[0] != 0");
    for (int k = 0; k < N; ++k) if (bt->nb_ptr[k + 1] < bt->nb_ptr[k]) return bad("nb_ptr not monotone");
    const size_t NB = N > 0 ? (size_t)bt->nb_ptr[N] : 0;
    if (NB > 0 && !bt->nb) return bad("NULL nb");
    for (size_t i = 0; i < NB; ++i) if (bt->nb[i] < 0 || bt->nb[i] >= N) return bad("neighbour index out of range");
    if (M > 0 && !bt->db_order) return bad("NULL db_order");
    std::vector<int32_t> pos_of(N > 0 ? N : 1, -1);
    for (int p = 0; p < M; ++p) {
      const int k = bt->db_order[p];
      if (k < 0 || k >= N) return bad("db_order index out of range");
      if (pos_of[k] >= 0) return bad("db_order repeats a keyframe");
      pos_of[k] = p;
    }
    if (Q > 0 && (!bt->query_kf || !bt->db_visible || !bt->num_candidates)) return bad("NULL query array");
    if (Q > 0 && cap > 0 && !bt->candidates) return bad("NULL candidates");
    int max_words = 0;
    size_t num_pairs = 0;
    for (int q = 0; q < Q; ++q) {
      const int k = bt->query_kf[q];
      if (k < 0 || k >= N) return bad("query_kf out of range");
      if (bt->db_visible[q] < 0 || bt->db_visible[q] > M) return bad("db_visible is not in 0..num_db");
      if (bt->min_score_in && std::isnan(bt->min_score_in[q])) return bad("min_score_in is NaN");
      max_words = std::max(max_words, bt->bow_ptr[k + 1] - bt->bow_ptr[k]);
      num_pairs += (size_t)(bt->nb_ptr[k + 1] - bt->nb_ptr[k]);
    }
    if (num_pairs > (size_t)INT32_MAX) return bad("more than 2^31 - 1 query neighbours");
    if (Q == 0) return COVGPU_OK;
    // host side of the call: the reference-score pairs and the inverted index of the database (posting lists in insertion order)
    std::vector<int32_t> pa, pb, poff(Q + 1, 0);
    if (!bt->min_score_in) {
      pa.reserve(num_pairs); pb.reserve(num_pairs);
      for (int q = 0; q < Q; ++q) {
        const int k = bt->query_kf[q];
        for (int i = bt->nb_ptr[k]; i < bt->nb_ptr[k + 1]; ++i) {
          if (bt->invalid && bt->invalid[bt->nb[i]]) continue;
          pa.push_back(k); pb.push_back(bt->nb[i]);
        }
        poff[q + 1] = (int32_t)pa.size();
      }
    }
    int inv_words = 0;
    for (int p = 0; p < M; ++p) {
      const int k = bt->db_order[p];
      if (bt->bow_ptr[k + 1] > bt->bow_ptr[k]) inv_words = std::max(inv_words, bt->word[bt->bow_ptr[k + 1] - 1] + 1);
    }
    std::vector<int32_t> inv_ptr((size_t)inv_words + 1, 0);
    for (int p = 0; p < M; ++p) {
      const int k = bt->db_order[p];
      for (int i = bt->bow_ptr[k]; i < bt->bow_ptr[k + 1]; ++i) ++inv_ptr[bt->word[i] + 1];
    }
    for (int w = 0; w < inv_words; ++w) {
      if ((int64_t)inv_ptr[w + 1] + inv_ptr[w] > (int64_t)INT32_MAX) return bad("more than 2^31 - 1 database words");
      inv_ptr[w + 1] += inv_ptr[w];
    }
    std::vector<int32_t> inv_pos((size_t)inv_ptr[inv_words]), fill(inv_ptr.begin(), inv_ptr.end() - 1);
    for (int p = 0; p < M; ++p) {
      const int k = bt->db_order[p];
      for (int i = bt->bow_ptr[k]; i < bt->bow_ptr[k + 1]; ++i) inv_pos[fill[bt->word[i]]++] = p;
    }
    HIPCHK(hipSetDevice(c->device));
    DeviceScratch U(c->st);
    DetectDev D{};
    D.M = M; D.inv_words = inv_words;
    const size_t nnz = N > 0 ? (size_t)bt->bow_ptr[N] : 0, Ns = (size_t)N, Qs = (size_t)Q, caps = (size_t)cap;
    HIPCHK(U.upload(&D.id, bt->id, Ns)); HIPCHK(U.upload(&D.client, bt->client, Ns));
    HIPCHK(U.upload(&D.vec_beg, bt->bow_ptr, Ns + 1)); HIPCHK(U.upload(&D.word, bt->word, nnz));
    HIPCHK(U.upload(&D.value, bt->value, nnz)); HIPCHK(U.upload(&D.nb_beg, bt->nb_ptr, Ns + 1));
    HIPCHK(U.upload(&D.nb, bt->nb, NB));
    D.vec_end = D.vec_beg + 1; D.nb_end = D.nb_beg + 1;                // a CSR pointer array as (begin, end)
    D.con_beg = D.nb_beg; D.con_end = D.nb_end; D.con = D.nb;          // a query's connected list is its row of the table
    HIPCHK(U.upload(&D.db_order, bt->db_order, (size_t)M));
    HIPCHK(U.upload(&D.pos_of, pos_of.data(), Ns)); HIPCHK(U.upload(&D.inv_ptr, inv_ptr.data(), inv_ptr.size()));
    HIPCHK(U.upload(&D.inv_pos, inv_pos.data(), inv_pos.size())); HIPCHK(U.upload(&D.query_kf, bt->query_kf, Qs));
    HIPCHK(U.upload(&D.db_visible, bt->db_visible, Qs));
    if (bt->min_score_in) HIPCHK(U.upload(&D.min_score, bt->min_score_in, Qs)); else HIPCHK(U.alloc(&D.min_score, Qs));
    int* counters = nullptr;                                           // max_common, num_sharing, num_scored, num_candidates
    HIPCHK(U.zeroed(&counters, 4 * Qs));
    D.max_common = counters; D.num_sharing = counters + Qs; D.num_scored = counters + 2 * Qs; D.num_candidates = counters + 3 * Qs;
    HIPCHK(U.alloc(&D.candidates, Qs * caps)); HIPCHK(U.alloc(&D.acc_score, Qs * caps));
    if (cap > 0) { HIPCHK(hipMemsetAsync(D.candidates, 0xff, 4 * Qs * caps, c->st)); HIPCHK(hipMemsetAsync(D.acc_score, 0, 4 * Qs * caps, c->st)); }
    if (!bt->min_score_in) {
      int *dpa = nullptr, *dpb = nullptr, *dpo = nullptr;
      double* dps = nullptr;
      HIPCHK(U.upload(&dpa, pa.data(), pa.size())); HIPCHK(U.upload(&dpb, pb.data(), pb.size()));
      HIPCHK(U.upload(&dpo, poff.data(), poff.size())); HIPCHK(U.alloc(&dps, pa.size()));
      launch_bow_score_pairs(D.vec_beg, D.vec_end, D.word, D.value, (int)pa.size(), dpa, dpb, dps, c->st);
      launch_bow_min_score(D, Q, dpo, dps, opts->min_score_factor, c->st);
    }
    // per-query scratch is 28 B per database entry; queries run in chunks that keep it within the budget
    const size_t budget = (size_t)(opts->scratch_kib > 0 ? opts->scratch_kib : 65536) << 10;
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>(Qs, budget / (28 * std::max<size_t>(1, (size_t)M))));
    const size_t cm = (size_t)chunk * (size_t)M;
    const int hist_stride = max_words + 1;
    int *common = nullptr, *first = nullptr, *best = nullptr, *order = nullptr, *hist = nullptr;
    double* score = nullptr;
    float* acc = nullptr;
    HIPCHK(U.alloc(&common, cm)); HIPCHK(U.alloc(&first, cm)); HIPCHK(U.alloc(&score, cm));
    HIPCHK(U.alloc(&acc, cm)); HIPCHK(U.alloc(&best, cm)); HIPCHK(U.alloc(&order, cm));
    HIPCHK(U.alloc(&hist, (size_t)chunk * (size_t)hist_stride));
    const DetectOptsDev O{opts->min_loop_dist, opts->exclude_kfs_with_id_less_than, opts->inter_map_matches_only != 0};
    for (int q0 = 0; q0 < Q; q0 += chunk)
      launch_bow_detect_chunk(D, O, q0, std::min(chunk, Q - q0), cap, hist_stride, common, first, score, acc, best, order, hist, c->st);
    HIPCHK(hipGetLastError());
    HIPCHK(U.fetch(bt->num_candidates, D.num_candidates, Qs)); HIPCHK(U.fetch(bt->max_common_words, D.max_common, Qs));
    HIPCHK(U.fetch(bt->num_sharing, D.num_sharing, Qs)); HIPCHK(U.fetch(bt->num_scored, D.num_scored, Qs));
    HIPCHK(U.fetch(bt->min_score, D.min_score, Qs));
    HIPCHK(U.fetch(bt->candidates, D.candidates, Qs * caps)); HIPCHK(U.fetch(bt->acc_score, D.acc_score, Qs * caps));
    HIPCHK(hipStreamSynchronize(c->st));
    return COVGPU_OK;
  });
}

// ---- redundant-keyframe pruning (k_prune.hip) ----
extern "C" void covgpu_default_prune_opts(covgpu_prune_opts* o) {
  if (!o) return;
  o->th_red = 0.95; o->max_time_dist = 1.0;                            // config_backend.yaml:58-59
  o->max_kfs = -1; o->max_rounds = 0;
}

namespace {

// The first violation of a prune call's arguments, or nullptr.
const char* prune_check(const covgpu_prune_t* p, const covgpu_prune_opts* o) {
  if (!p || !o) return "NULL problem or options";
  if (!std::isfinite(o->th_red) || !std::isfinite(o->max_time_dist)) return "non-finite th_red or max_time_dist";
  const int K = p->num_kf, L = p->num_lm;
  if (K < 0 || L < 0 || p->capacity < 0) return "negative count";
  if (!p->lm_obs_ptr) return "NULL lm_obs_ptr";
  if (p->lm_obs_ptr[0] != 0) return "lm_obs_ptr[0] != 0";
  for (int l = 0; l < L; ++l) if (p->lm_obs_ptr[l + 1] < p->lm_obs_ptr[l]) return "lm_obs_ptr not monotone";
  const int O = p->lm_obs_ptr[L];
  if (O > 0 && !p->obs_kf) return "NULL obs_kf";
  for (int i = 0; i < O; ++i) if (p->obs_kf[i] < 0 || p->obs_kf[i] >= K) return "obs_kf out of range";
  if (K > 0 && (!p->kf_pred || !p->kf_succ || !p->kf_time)) return "NULL keyframe array";
  if (p->capacity > 0 && (!p->round_kf || !p->round_action)) return "NULL round array";
  for (int k = 0; k < K; ++k) {
    if (!std::isfinite(p->kf_time[k])) return "non-finite kf_time";
    if (p->kf_pred[k] < -1 || p->kf_pred[k] >= K || p->kf_succ[k] < -1 || p->kf_succ[k] >= K) return "kf_pred or kf_succ out of range";
  }
  for (int k = 0; k < K; ++k) {
    const int pr = p->kf_pred[k], su = p->kf_succ[k];
    if ((pr >= 0 && p->kf_succ[pr] >= 0 && p->kf_succ[pr] != k) || (su >= 0 && p->kf_pred[su] >= 0 && p->kf_pred[su] != k))
      return "kf_pred and kf_succ are not mutual";
  }
  return nullptr;
}

}  // namespace

extern "C" int covgpu_prune_check(const covgpu_prune_t* p, const covgpu_prune_opts* o) {
  return guarded([&]() -> int {
    if (const char* m = prune_check(p, o)) { g_err = std::string("covgpu_prune_check: ") + m; return COVGPU_ERR_INVALID_ARG; }
    return COVGPU_OK;
  });
}

extern "C" int covgpu_prune_redundant(covgpu_context* c, const covgpu_prune_t* p, const covgpu_prune_opts* o) {
  return batch_entry("covgpu_prune_redundant", c, [&](auto bad) -> int {
    if (const char* m = prune_check(p, o)) return bad(m);
    const int K = p->num_kf, L = p->num_lm;
    const size_t Ks = (size_t)K, Ls = (size_t)L, Os = (size_t)p->lm_obs_ptr[L];
    int valid0 = 0;
    for (int k = 0; k < K; ++k) valid0 += !(p->kf_invalid && p->kf_invalid[k]);
    if (p->loop_ms) *p->loop_ms = 0.0;
    if (K == 0) {   // nothing to rank (and no observation: obs_kf has no valid value)
      if (p->num_rounds) *p->num_rounds = 0;
      if (p->removed) *p->removed = 0;
      if (p->stop_reason) *p->stop_reason = o->max_kfs >= 0 ? 2 : 0;
      if (p->lm_nobs) std::fill(p->lm_nobs, p->lm_nobs + L, 0);
      return COVGPU_OK;
    }
    int32_t res[3] = {0, 0, 0};
    HIPCHK(hipSetDevice(c->device));
    struct Events {   // around the greedy loop, only when the caller asks for its time
      hipEvent_t a = nullptr, b = nullptr;
      ~Events() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
    } ev;
    DeviceScratch U(c->st);
    PruneDev D{};
    D.K = K; D.L = L;
    HIPCHK(U.upload(&D.lm_ptr, p->lm_obs_ptr, Ls + 1)); HIPCHK(U.upload(&D.obs_kf, p->obs_kf, Os));
    if (p->lm_invalid) HIPCHK(U.upload(&D.lm_invalid, p->lm_invalid, Ls));
    if (p->kf_invalid) HIPCHK(U.upload(&D.kf_invalid, p->kf_invalid, Ks));
    if (p->kf_first) HIPCHK(U.upload(&D.kf_first, p->kf_first, Ks));
    if (p->kf_loop) HIPCHK(U.upload(&D.kf_loop, p->kf_loop, Ks));
    if (p->kf_not_erase) HIPCHK(U.upload(&D.kf_not_erase, p->kf_not_erase, Ks));
    HIPCHK(U.upload(&D.time, p->kf_time, Ks));
    HIPCHK(U.upload(&D.pred, p->kf_pred, Ks)); HIPCHK(U.upload(&D.succ, p->kf_succ, Ks));
    HIPCHK(U.alloc(&D.kf_ptr, Ks + 1)); HIPCHK(U.alloc(&D.kf_lm, Os)); HIPCHK(U.alloc(&D.cnt, Ks));
    HIPCHK(U.alloc(&D.lm_nobs, Ls));
    HIPCHK(U.alloc(&D.num, Ks)); HIPCHK(U.alloc(&D.den, Ks)); HIPCHK(U.alloc(&D.live, Ks)); HIPCHK(U.alloc(&D.cand, Ks));
    HIPCHK(U.alloc(&D.out_num, Ks)); HIPCHK(U.alloc(&D.out_den, Ks));
    const int max_rounds = o->max_rounds > 0 ? std::min(o->max_rounds, K) : K;   // (a round takes a candidate: never more than K)
    D.cap = std::min(p->capacity, max_rounds);
    HIPCHK(U.alloc(&D.round_kf, (size_t)D.cap)); HIPCHK(U.alloc(&D.round_action, (size_t)D.cap));
    HIPCHK(U.zeroed(&D.result, 3));
    const PruneOptsDev OD{o->th_red, o->max_time_dist, o->max_kfs, o->max_rounds > 0 ? o->max_rounds : K, valid0};
    launch_prune_setup(D, c->st);
    if (p->loop_ms) { HIPCHK(hipEventCreate(&ev.a)); HIPCHK(hipEventCreate(&ev.b)); HIPCHK(hipEventRecord(ev.a, c->st)); }
    launch_prune_loop(D, OD, c->st);
    if (p->loop_ms) HIPCHK(hipEventRecord(ev.b, c->st));
    launch_prune_finish(D, c->st);
    HIPCHK(hipGetLastError());
    HIPCHK(U.fetch(res, D.result, 3));
    HIPCHK(U.fetch(p->round_kf, D.round_kf, (size_t)D.cap)); HIPCHK(U.fetch(p->round_action, D.round_action, (size_t)D.cap));
    HIPCHK(U.fetch(p->kf_pred_out, D.pred, Ks)); HIPCHK(U.fetch(p->kf_succ_out, D.succ, Ks));
    HIPCHK(U.fetch(p->lm_nobs, D.lm_nobs, Ls));
    HIPCHK(U.fetch(p->red_num, D.out_num, Ks)); HIPCHK(U.fetch(p->red_den, D.out_den, Ks));
    HIPCHK(hipStreamSynchronize(c->st));
    if (p->loop_ms) { float ms = 0.f; HIPCHK(hipEventElapsedTime(&ms, ev.a, ev.b)); *p->loop_ms = ms; }
    if (p->num_rounds) *p->num_rounds = res[0];
    if (p->removed) *p->removed = res[1];
    if (p->stop_reason) *p->stop_reason = res[2];
    return COVGPU_OK;
  });
}

// ---- landmark refresh (k_lmrefresh.hip) ----
extern "C" void covgpu_default_landmark_refresh_opts(covgpu_landmark_refresh_opts* o) {
  if (!o) return;
  o->scale_factor = 2.0; o->num_octaves = 1;                          // config_backend.yaml:31-32
}

extern "C" void covgpu_landmark_refresh_limits(int32_t out[4]) {
  if (!out) return;
  out[0] = kLmrGroupMax; out[1] = 64; out[2] = kLmrLongThreads; out[3] = kLmrStage;
}

static_assert(kLmrGroupMax == COVGPU_LMR_GROUP_MAX && kLmrLongThreads == COVGPU_LMR_LONG_THREADS && kLmrStage == COVGPU_LMR_STAGE &&
              kLmrForms == COVGPU_LMR_FORMS && COVGPU_LMR_WAVE == 64, "covgpu.h names the limits of k_lmrefresh.hip");

namespace {

// The first violation of a landmark-refresh call's arguments, or nullptr.
const char* lm_refresh_check(const covgpu_landmark_refresh_t* p, const covgpu_landmark_refresh_opts* o) {
  if (!p || !o) return "NULL problem or options";
  if (!std::isfinite(o->scale_factor) || !(o->scale_factor > 0.0)) return "scale_factor not finite or not positive";
  if (o->num_octaves < 1 || o->num_octaves > 64) return "num_octaves outside [1, 64]";
  const int K = p->num_kf, L = p->num_lm;
  if (K < 0 || L < 0) return "negative count";
  if (!p->lm_obs_ptr) return "NULL lm_obs_ptr";
  if (p->lm_obs_ptr[0] != 0) return "lm_obs_ptr[0] != 0";
  for (int l = 0; l < L; ++l) if (p->lm_obs_ptr[l + 1] < p->lm_obs_ptr[l]) return "lm_obs_ptr not monotone";
  const int O = p->lm_obs_ptr[L];
  if (O > 0 && (!p->obs_kf || !p->obs_octave)) return "NULL obs_kf or obs_octave";
  if (L > 0 && (!p->lm_ref_obs || !p->lm_pos)) return "NULL lm_ref_obs or lm_pos";
  if (K > 0 && !p->kf_center) return "NULL kf_center";
  for (int i = 0; i < O; ++i) if (p->obs_kf[i] < 0 || p->obs_kf[i] >= K) return "obs_kf out of range";
  for (int l = 0; l < L; ++l) {
    const int r = p->lm_ref_obs[l], m = p->lm_obs_ptr[l + 1] - p->lm_obs_ptr[l];
    if (r < -1 || r >= m) return "lm_ref_obs outside its landmark's list";
    if (r >= 0) { const int oc = p->obs_octave[p->lm_obs_ptr[l] + r]; if (oc < 0 || oc >= 64) return "octave of a reference observation outside [0, 64)"; }
  }
  for (size_t i = 0; i < 3 * (size_t)L; ++i) if (!std::isfinite(p->lm_pos[i])) return "non-finite lm_pos";
  for (size_t i = 0; i < 3 * (size_t)K; ++i) if (!std::isfinite(p->kf_center[i])) return "non-finite kf_center";
  return nullptr;
}

}  // namespace

extern "C" int covgpu_landmark_refresh_check(const covgpu_landmark_refresh_t* p, const covgpu_landmark_refresh_opts* o) {
  return guarded([&]() -> int {
    if (const char* m = lm_refresh_check(p, o)) { g_err = std::string("covgpu_landmark_refresh_check: ") + m; return COVGPU_ERR_INVALID_ARG; }
    return COVGPU_OK;
  });
}

extern "C" int covgpu_landmark_refresh(covgpu_context* c, const covgpu_landmark_refresh_t* p, const covgpu_landmark_refresh_opts* o) {
  return batch_entry("covgpu_landmark_refresh", c, [&](auto bad) -> int {
    if (const char* m = lm_refresh_check(p, o)) return bad(m);
    const int K = p->num_kf, L = p->num_lm;
    const size_t Ks = (size_t)K, Ls = (size_t)L, Os = (size_t)p->lm_obs_ptr[L];
    // the form of every landmark from the length of its list; an invalid landmark is skipped by the narrowest
    static const int kLanes[kLmrForms] = {4, 8, 16, 32, 64, 0};
    std::vector<int32_t> form(Ls), start(kLmrForms + 1, 0), list(Ls);
    for (int l = 0; l < L; ++l) {
      const int m = p->lm_invalid && p->lm_invalid[l] ? 0 : p->lm_obs_ptr[l + 1] - p->lm_obs_ptr[l];
      int f = 0;
      while (f < kLmrForms - 1 && m > kLanes[f]) ++f;
      form[l] = f; ++start[f + 1];
    }
    if (p->form_count) for (int f = 0; f < kLmrForms; ++f) p->form_count[f] = start[f + 1];
    if (p->kernel_ms) *p->kernel_ms = 0.0;
    if (L == 0) return COVGPU_OK;
    for (int f = 0; f < kLmrForms; ++f) start[f + 1] += start[f];
    { std::vector<int32_t> at(start.begin(), start.end() - 1); for (int l = 0; l < L; ++l) list[at[form[l]]++] = l; }
    double scale[64];
    for (int l = 0; l < 64; ++l) scale[l] = std::pow(o->scale_factor, l);   // the device never calls pow
    HIPCHK(hipSetDevice(c->device));
    struct Events {   // around the kernels, only when the caller asks for their time
      hipEvent_t a = nullptr, b = nullptr;
      ~Events() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
    } ev;
    DeviceScratch U(c->st);
    LmRefreshDev D{};
    int* dlist = nullptr;
    HIPCHK(U.upload(&D.lm_ptr, p->lm_obs_ptr, Ls + 1)); HIPCHK(U.upload(&D.obs_kf, p->obs_kf, Os));
    HIPCHK(U.upload(&D.obs_octave, p->obs_octave, Os));
    if (p->obs_desc) HIPCHK(U.upload(&D.obs_desc, reinterpret_cast<const uint4*>(p->obs_desc), 2 * Os));
    HIPCHK(U.upload(&D.ref_obs, p->lm_ref_obs, Ls)); HIPCHK(U.upload(&D.pos, p->lm_pos, 3 * Ls));
    HIPCHK(U.upload(&D.center, p->kf_center, 3 * Ks));
    if (p->kf_invalid) HIPCHK(U.upload(&D.kf_invalid, p->kf_invalid, Ks));
    if (p->lm_invalid) HIPCHK(U.upload(&D.lm_invalid, p->lm_invalid, Ls));
    HIPCHK(U.upload(&D.scale, scale, 64));
    D.num_octaves = o->num_octaves;
    HIPCHK(U.upload(&dlist, list.data(), Ls));
    HIPCHK(U.alloc(&D.desc_obs, Ls)); HIPCHK(U.alloc(&D.desc, 2 * Ls));
    HIPCHK(U.alloc(&D.normal, 3 * Ls)); HIPCHK(U.alloc(&D.min_dist, Ls)); HIPCHK(U.alloc(&D.max_dist, Ls)); HIPCHK(U.alloc(&D.status, Ls));
    if (p->kernel_ms) { HIPCHK(hipEventCreate(&ev.a)); HIPCHK(hipEventCreate(&ev.b)); HIPCHK(hipEventRecord(ev.a, c->st)); }
    for (int f = 0; f < kLmrForms; ++f) launch_lm_refresh(D, kLanes[f], dlist + start[f], start[f + 1] - start[f], c->st);
    if (p->kernel_ms) HIPCHK(hipEventRecord(ev.b, c->st));
    HIPCHK(hipGetLastError());
    if (p->obs_desc) {
      HIPCHK(U.fetch(p->lm_desc_obs, D.desc_obs, Ls));
      HIPCHK(U.fetch(reinterpret_cast<uint4*>(p->lm_desc), D.desc, 2 * Ls));
    }
    HIPCHK(U.fetch(p->lm_normal, D.normal, 3 * Ls)); HIPCHK(U.fetch(p->lm_min_distance, D.min_dist, Ls));
    HIPCHK(U.fetch(p->lm_max_distance, D.max_dist, Ls)); HIPCHK(U.fetch(p->lm_status, D.status, Ls));
    HIPCHK(hipStreamSynchronize(c->st));
    if (p->kernel_ms) { float ms = 0.f; HIPCHK(hipEventElapsedTime(&ms, ev.a, ev.b)); *p->kernel_ms = ms; }
    return COVGPU_OK;
  });
}
