// batch.hip — host side of libcovgpu's stateless batch front end: the extern "C" entry points that take one batch of host arrays,
// run its kernels on the context's stream and hand the results back. Nothing here touches the resident problem of the solver
// (upload.hip, solver.hip): a context lends its device and its stream only. Serves DESIGN.md §4.9 (relative pose, k_relpose.hip; the landmark
// re-anchoring behind a pose-graph solve), §4.10 (P3P RANSAC, k_abspose.hip), §4.11 (descriptor matching, k_match.hip), §4.12
// (guided matching, k_guided.hip), §4.13 (bag-of-words transform, score and candidate query, k_bow.hip), §4.14 (redundant-keyframe
// pruning, k_prune.hip), §4.15 (landmark descriptors, normals and scale ranges, k_lmrefresh.hip) and §4.17 (float descriptor matching,
// k_matchf.hip).
// Every entry point reads: check (batch_check.hpp: a pure function that also fills the call's plan), hipSetDevice, uploads into one
// DeviceScratch (host.hpp), launch, fetches and one synchronisation of its stream, at the end. The prologue (batch_entry) and the body of
// the covgpu_*_check exports (check_export) are in host.hpp.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "host.hpp"

using namespace covgpu;

extern "C" int covgpu_relpose_batch(covgpu_context* c, const covgpu_relpose_batch_t* bt, double th_outlier, int32_t min_inliers) {
  return batch_entry("covgpu_relpose_batch", c, [&](auto bad) -> int {
    RelposePlan P;
    if (const char* m = relpose_check(bt, P)) return bad(m);
    const size_t B = (size_t)bt->num_pairs, C = P.corr;
    if (B == 0) return COVGPU_OK;
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
    if (P.unified) {
      HIPCHK(U.upload(&dmA, P.model_a.data(), B)); HIPCHK(U.upload(&dmB, P.model_b.data(), B));
      HIPCHK(U.upload(&dxA, P.xi_a.data(), B)); HIPCHK(U.upload(&dxB, P.xi_b.data(), B));
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
    AbsposePlan P;
    if (const char* m = abspose_check(bt, opts, P)) return bad(m);
    const size_t B = (size_t)bt->num, C = P.corr;
    if (B == 0) return COVGPU_OK;
    HIPCHK(hipSetDevice(c->device));
    DeviceScratch U(c->st);
    int *dptr_ = nullptr, *din = nullptr, *dit = nullptr, *dbd = nullptr;
    double *df = nullptr, *dP = nullptr, *ds = nullptr, *dT = nullptr;
    unsigned long long* dseed = nullptr;
    unsigned char* dmask = nullptr;
    HIPCHK(U.upload(&dptr_, bt->corr_ptr, B + 1));
    HIPCHK(U.upload(&df, bt->bearing, 3 * C)); HIPCHK(U.upload(&dP, bt->point_w, 3 * C)); HIPCHK(U.upload(&ds, bt->sigma_angle, C));
    HIPCHK(U.upload(&dseed, P.seeds.data(), B));
    HIPCHK(U.upload(&dT, bt->T_wc, 7 * B));   // untouched rows come back as they went
    HIPCHK(U.alloc(&dmask, C)); HIPCHK(U.alloc(&din, B)); HIPCHK(U.alloc(&dit, B)); HIPCHK(U.alloc(&dbd, B));
    launch_abspose((int)B, dptr_, df, dP, ds, dseed, dT, dmask, din, dit, dbd, opts->min_inliers, opts->max_iterations, opts->probability, opts->threshold,
                   P.max_n, c->st);
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
    if (const char* m = p3p_check(n, f, P, T, nsol, chosen)) return bad(m);
    if (n == 0) return COVGPU_OK;
    const size_t N = (size_t)n;
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
    MatchPlan P;
    if (const char* m = match_check(bt, opts, P)) return bad(m);
    const int J = bt->num_jobs;
    if (J == 0) return COVGPU_OK;
    const bool dense = opts->mode == COVGPU_MATCH_DENSE;
    const size_t R = P.rows, totalA = P.total_a;
    HIPCHK(hipSetDevice(c->device));
    int dcut = 0;                                                    // (float)d < dist_threshold  <=>  d < dcut, for d in 0..256
    while (dcut <= 256 && (float)dcut < opts->dist_threshold) ++dcut;
    DeviceScratch U(c->st);
    unsigned char *ddesc = nullptr, *dskip = nullptr;
    int *dptr_ = nullptr, *dsa = nullptr, *dsb = nullptr, *doff = nullptr, *dlist = nullptr, *dmatch = nullptr, *ddist = nullptr, *dn = nullptr;
    HIPCHK(U.upload(&ddesc, bt->desc, 32 * R));
    if (dense && bt->skip) HIPCHK(U.upload(&dskip, bt->skip, R));
    HIPCHK(U.upload(&dptr_, bt->row_ptr, (size_t)bt->num_sets + 1));
    HIPCHK(U.upload(&dsa, bt->set_a, (size_t)J)); HIPCHK(U.upload(&dsb, bt->set_b, (size_t)J)); HIPCHK(U.upload(&doff, P.off.data(), (size_t)J));
    if (dense) HIPCHK(U.alloc(&dlist, 4 * totalA));                  // the 4 best of every query row
    HIPCHK(U.alloc(&dmatch, totalA)); HIPCHK(U.alloc(&ddist, totalA)); HIPCHK(U.zeroed(&dn, (size_t)J));
    launch_match(opts->mode, J, P.max_a, P.max_b, ddesc, dskip, dptr_, dsa, dsb, doff, dlist, dmatch, ddist, dn, dcut, opts->dist_threshold, opts->ratio,
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

extern "C" int covgpu_match_float_check(const covgpu_match_float_batch_t* bt, const covgpu_match_opts* opts) {
  return check_export("covgpu_match_float_check", [&] { MatchPlan P; return match_float_check(bt, opts, P); });
}

extern "C" int covgpu_match_float_batch(covgpu_context* c, const covgpu_match_float_batch_t* bt, const covgpu_match_opts* opts) {
  return batch_entry("covgpu_match_float_batch", c, [&](auto bad) -> int {
    MatchPlan P;
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

// The keypoint sets of a guided call on the device (the 32-byte descriptors go up as the kernels read them: two uint4 a row). `rec`
// stages the records: the caller declares it before the scratch, so that it outlives the copy.
int upload_guided_sets(DeviceScratch& U, const covgpu_keypoint_sets_t& s, const uint8_t* taken, std::vector<int4>& rec, GuidedSets& D) {
  const size_t R = s.num_sets > 0 ? (size_t)s.row_ptr[s.num_sets] : 0, S = (size_t)s.num_sets;
  rec = guided_records(s, taken);
  HIPCHK(U.upload(&D.kpr, rec.data(), R)); HIPCHK(U.upload(&D.kdesc, (const uint4*)s.desc, 2 * R));
  HIPCHK(U.upload(&D.row_ptr, s.row_ptr, S + 1)); HIPCHK(U.upload(&D.bounds, s.bounds, 4 * S));
  return COVGPU_OK;
}

// The scan tiles of a guided call on the device: the kernels read a GuidedTile as an int4 {job, direction, first point, points}.
static_assert(sizeof(GuidedTile) == sizeof(int4) && offsetof(GuidedTile, job) == offsetof(int4, x) && offsetof(GuidedTile, dir) == offsetof(int4, y) &&
              offsetof(GuidedTile, first) == offsetof(int4, z) && offsetof(GuidedTile, count) == offsetof(int4, w), "a GuidedTile is uploaded as an int4");
int upload_guided_tiles(DeviceScratch& U, const std::vector<GuidedTile>& tiles, const int4** d) {
  HIPCHK(U.upload(d, reinterpret_cast<const int4*>(tiles.data()), tiles.size()));
  return COVGPU_OK;
}

GuidedOptsDev guided_opts_dev(const covgpu_guided_opts* o) {
  return GuidedOptsDev{o->th_low, o->radius, o->scale_factor, std::log(o->scale_factor), o->num_octaves, o->agreement};
}

}  // namespace

extern "C" int covgpu_search_se3_batch(covgpu_context* c, const covgpu_search_se3_batch_t* bt, const covgpu_guided_opts* opts) {
  return batch_entry("covgpu_search_se3_batch", c, [&](auto bad) -> int {
    GuidedPlan P;
    if (const char* m = search_se3_check(bt, opts, P)) return bad(m);
    const int J = bt->num_jobs;
    if (J == 0) return COVGPU_OK;
    const size_t Ss = (size_t)bt->sets.num_sets, Js = (size_t)J, R = P.rows, tot1 = P.tot1, tot2 = P.tot2;
    HIPCHK(hipSetDevice(c->device));
    std::vector<int4> rec;
    DeviceScratch U(c->st);
    GuidedSe3Args A{};
    RC(upload_guided_sets(U, bt->sets, nullptr, rec, A.S));
    HIPCHK(U.upload(&A.K, bt->K, 4 * Ss)); HIPCHK(U.upload(&A.lm_pos, bt->lm_pos, 3 * R));
    HIPCHK(U.upload(&A.lm_maxd, bt->lm_max_distance, R)); HIPCHK(U.upload(&A.lm_desc, (const uint4*)bt->lm_desc, 2 * R));
    HIPCHK(U.upload(&A.lm_free, bt->lm_free, R));
    HIPCHK(U.upload(&A.set_1, bt->set_1, Js)); HIPCHK(U.upload(&A.set_2, bt->set_2, Js));
    HIPCHK(U.upload(&A.T12, bt->T12, 7 * Js));
    HIPCHK(U.upload(&A.off1, P.off1.data(), Js)); HIPCHK(U.upload(&A.off2, P.off2.data(), Js));
    const int4* dtiles = nullptr;
    RC(upload_guided_tiles(U, P.tiles, &dtiles));
    HIPCHK(U.alloc(&A.m1, tot1)); HIPCHK(U.alloc(&A.m2, tot2)); HIPCHK(U.alloc(&A.match, tot1));
    HIPCHK(U.zeroed(&A.nfound, Js));
    launch_guided_se3(A, guided_opts_dev(opts), J, dtiles, (int)P.tiles.size(), c->st);
    HIPCHK(hipGetLastError());
    HIPCHK(U.fetch(bt->match, A.match, tot1)); HIPCHK(U.fetch(bt->match1, A.m1, tot1)); HIPCHK(U.fetch(bt->match2, A.m2, tot2));
    HIPCHK(U.fetch(bt->nfound, A.nfound, Js));
    HIPCHK(hipStreamSynchronize(c->st));
    return COVGPU_OK;
  });
}

extern "C" int covgpu_search_projection_batch(covgpu_context* c, const covgpu_search_projection_batch_t* bt, const covgpu_guided_opts* opts) {
  return batch_entry("covgpu_search_projection_batch", c, [&](auto bad) -> int {
    GuidedPlan G;
    if (const char* m = search_projection_check(bt, opts, G)) return bad(m);
    const int J = bt->num_jobs;
    if (J == 0) return COVGPU_OK;
    const size_t Ss = (size_t)bt->sets.num_sets, Js = (size_t)J, P = G.points;
    HIPCHK(hipSetDevice(c->device));
    std::vector<int4> rec;
    DeviceScratch U(c->st);
    GuidedProjArgs A{};
    RC(upload_guided_sets(U, bt->sets, bt->taken, rec, A.S));
    HIPCHK(U.upload(&A.cam, bt->cam, 8 * Ss)); HIPCHK(U.upload(&A.dist_type, bt->dist_type, Ss));
    if (bt->cam_model) { HIPCHK(U.upload(&A.cam_model, bt->cam_model, Ss)); HIPCHK(U.upload(&A.xi, G.xi.data(), Ss)); }
    HIPCHK(U.upload(&A.set, bt->set, Js)); HIPCHK(U.upload(&A.T_cw, bt->T_cw, 7 * Js));
    HIPCHK(U.upload(&A.point_ptr, bt->point_ptr, Js + 1));
    HIPCHK(U.upload(&A.p_w, bt->p_w, 3 * P)); HIPCHK(U.upload(&A.normal, bt->normal, 3 * P));
    HIPCHK(U.upload(&A.min_d, bt->min_distance, P)); HIPCHK(U.upload(&A.max_d, bt->max_distance, P));
    HIPCHK(U.upload(&A.p_desc, (const uint4*)bt->p_desc, 2 * P));
    if (bt->skip) HIPCHK(U.upload(&A.skip, bt->skip, P));
    if (bt->existing_idx) HIPCHK(U.upload(&A.existing, bt->existing_idx, P));
    const int4* dtiles = nullptr;
    RC(upload_guided_tiles(U, G.tiles, &dtiles));
    HIPCHK(U.alloc(&A.lists, kGuidedListCap * P)); HIPCHK(U.alloc(&A.cnt, P)); HIPCHK(U.alloc(&A.target, 2 * P));
    HIPCHK(U.alloc(&A.rad, P)); HIPCHK(U.alloc(&A.lvl, P)); HIPCHK(U.alloc(&A.dold, P));
    HIPCHK(U.alloc(&A.claimed, P)); HIPCHK(U.alloc(&A.remap_to, P)); HIPCHK(U.alloc(&A.best_dist, P));
    HIPCHK(U.alloc(&A.nmatches, Js));
    launch_guided_projection(A, guided_opts_dev(opts), J, dtiles, (int)G.tiles.size(), c->st);
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
    if (const char* m = reanchor_check(K, pose_old, pose_new, L, ref_kf, lm_pos)) return bad(m);
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
// (the vocabulary and bow CSR checks are shared with bowdb.hip: batch_check.hpp)

extern "C" int covgpu_bow_transform_batch(covgpu_context* c, const covgpu_bow_vocab_t* v, const covgpu_bow_transform_batch_t* bt) {
  return batch_entry("covgpu_bow_transform_batch", c, [&](auto bad) -> int {
    size_t R = 0;
    if (const char* m = bow_transform_check(v, bt, R)) return bad(m);
    const int S = bt->num_sets;
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
    if (const char* m = bow_score_pairs_check(num_vec, bow_ptr, word, value, num_pairs, a, b, score)) return bad(m);
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
    DetectPlan P;
    if (const char* m = detect_check(bt, opts, P)) return bad(m);
    const int N = bt->num_kf, M = bt->num_db, Q = bt->num_queries, cap = bt->cap;
    if (Q == 0) return COVGPU_OK;
    HIPCHK(hipSetDevice(c->device));
    DeviceScratch U(c->st);
    DetectDev D{};
    D.M = M; D.inv_words = P.inv_words;
    const size_t nnz = N > 0 ? (size_t)bt->bow_ptr[N] : 0, Ns = (size_t)N, Qs = (size_t)Q, caps = (size_t)cap;
    HIPCHK(U.upload(&D.id, bt->id, Ns)); HIPCHK(U.upload(&D.client, bt->client, Ns));
    HIPCHK(U.upload(&D.vec_beg, bt->bow_ptr, Ns + 1)); HIPCHK(U.upload(&D.word, bt->word, nnz));
    HIPCHK(U.upload(&D.value, bt->value, nnz)); HIPCHK(U.upload(&D.nb_beg, bt->nb_ptr, Ns + 1));
    HIPCHK(U.upload(&D.nb, bt->nb, P.num_nb));
    D.vec_end = D.vec_beg + 1; D.nb_end = D.nb_beg + 1;                // a CSR pointer array as (begin, end)
    D.con_beg = D.nb_beg; D.con_end = D.nb_end; D.con = D.nb;          // a query's connected list is its row of the table
    HIPCHK(U.upload(&D.db_order, bt->db_order, (size_t)M));
    HIPCHK(U.upload(&D.pos_of, P.pos_of.data(), Ns)); HIPCHK(U.upload(&D.inv_ptr, P.inv_ptr.data(), P.inv_ptr.size()));
    HIPCHK(U.upload(&D.inv_pos, P.inv_pos.data(), P.inv_pos.size())); HIPCHK(U.upload(&D.query_kf, bt->query_kf, Qs));
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
      HIPCHK(U.upload(&dpa, P.pair_a.data(), P.pair_a.size())); HIPCHK(U.upload(&dpb, P.pair_b.data(), P.pair_b.size()));
      HIPCHK(U.upload(&dpo, P.pair_off.data(), P.pair_off.size())); HIPCHK(U.alloc(&dps, P.pair_a.size()));
      launch_bow_score_pairs(D.vec_beg, D.vec_end, D.word, D.value, (int)P.pair_a.size(), dpa, dpb, dps, c->st);
      launch_bow_min_score(D, Q, dpo, dps, opts->min_score_factor, c->st);
    }
    // per-query scratch is 28 B per database entry; queries run in chunks that keep it within the budget
    const size_t budget = (size_t)(opts->scratch_kib > 0 ? opts->scratch_kib : 65536) << 10;
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>(Qs, budget / (28 * std::max<size_t>(1, (size_t)M))));
    const size_t cm = (size_t)chunk * (size_t)M;
    const int hist_stride = P.max_words + 1;
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

extern "C" int covgpu_prune_check(const covgpu_prune_t* p, const covgpu_prune_opts* o) {
  return check_export("covgpu_prune_check", [&] { return prune_check(p, o); });
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
    EventPair ev;   // around the greedy loop, only when the caller asks for its time
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

extern "C" int covgpu_landmark_refresh_check(const covgpu_landmark_refresh_t* p, const covgpu_landmark_refresh_opts* o) {
  return check_export("covgpu_landmark_refresh_check", [&] { return lm_refresh_check(p, o); });
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
    EventPair ev;   // around the kernels, only when the caller asks for their time
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
