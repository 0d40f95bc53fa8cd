// batch_check.hpp — every argument check of the stateless batch front end (batch.hip, voctrain.hip) and the checks it shares with the
// resident database (bowdb.hip) and the solver's upload (upload.hip). Plain C++17: covgpu.h, the standard library and batch_limits.hpp;
// no HIP call and no HIP type, so the checks compile and run (under sanitizers too) without a device: tests/cpp/batch_check_main.cpp.
// Every check is a pure function of its arguments that returns the message of the first violation, or nullptr. What it derives on
// the way (offsets, totals, tiles, host-built tables) goes into a plan struct that the entry point then uses.
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/covgpu.h"
#include "batch_limits.hpp"

namespace covgpu {

// ---- primitives ----

// The two messages of a CSR pointer array, by the array's name.
struct CsrMsgs { const char *first, *monotone; };
constexpr CsrMsgs kRowPtr{"row_ptr[0] != 0", "row_ptr not monotone"}, kCorrPtr{"corr_ptr[0] != 0", "corr_ptr not monotone"},
    kPointPtr{"point_ptr[0] != 0", "point_ptr not monotone"}, kNbPtr{"nb_ptr[0] != 0", "nb_ptr not monotone"},
    kLmObsPtr{"lm_obs_ptr[0] != 0", "lm_obs_ptr not monotone"}, kBowPtr{"bow_ptr[0] != 0", "bow_ptr not monotone"},
    kChildPtr{"child_ptr[0] != 0", "child_ptr not monotone"};

// Row r of a CSR pointer array: not shorter than 0 and, with cap > 0, not longer than cap (the per-set limit of the matching kernels).
inline const char* csr_row_check(const int32_t* ptr, int r, const CsrMsgs& m, int cap = 0) {
  if (ptr[r + 1] < ptr[r]) return m.monotone;
  if (cap > 0 && ptr[r + 1] - ptr[r] > cap) return "a set holds more than COVGPU_MATCH_MAX_ROWS rows";
  return nullptr;
}

// The whole array ptr[0..n]: starts at 0, then row by row. *longest receives the longest row.
inline const char* csr_check(const int32_t* ptr, int n, const CsrMsgs& m, int cap = 0, int* longest = nullptr) {
  if (ptr[0] != 0) return m.first;
  for (int r = 0; r < n; ++r) {
    if (const char* e = csr_row_check(ptr, r, m, cap)) return e;
    if (longest) *longest = std::max(*longest, ptr[r + 1] - ptr[r]);
  }
  return nullptr;
}

// Descriptor sets (row_ptr of the matchers, the guided searches and the BoW transform): no sets are valid and read nothing.
inline const char* desc_sets_check(int num_sets, const int32_t* row_ptr) {
  if (num_sets <= 0) return nullptr;
  if (!row_ptr) return "NULL row_ptr";
  return csr_check(row_ptr, num_sets, kRowPtr, COVGPU_MATCH_MAX_ROWS);
}

// Camera i of a model / xi pair of arrays (model NULL: all pinhole). `no_xi` names the xi array of the call.
constexpr const char* kNoXi = "unified camera without xi";
constexpr const char* kNoCamXi = "unified camera without cam_xi";
inline const char* cam_model_check(const int32_t* model, size_t i) {
  return model && model[i] != COVGPU_CAM_PINHOLE && model[i] != COVGPU_CAM_UNIFIED ? "unknown camera model" : nullptr;
}
inline const char* cam_xi_check(const int32_t* model, const double* xi, size_t i, const char* no_xi) {
  if (!model || model[i] != COVGPU_CAM_UNIFIED) return nullptr;
  if (!xi) return no_xi;
  if (!std::isfinite(xi[i]) || xi[i] < 0.0) return "xi of a unified camera is negative or not finite";
  return nullptr;
}
inline const char* cam_check(const int32_t* model, const double* xi, size_t i, const char* no_xi) {
  if (const char* e = cam_model_check(model, i)) return e;
  return cam_xi_check(model, xi, i, no_xi);
}

// ---- relative pose and P3P ----

// Per side the model and xi of every pair (xi 0 for pinhole rows); uploaded only if some camera of the batch is unified.
struct RelposePlan {
  size_t corr = 0;
  bool unified = false;
  std::vector<int32_t> model_a, model_b;
  std::vector<double> xi_a, xi_b;
};

inline const char* relpose_check(const covgpu_relpose_batch_t* bt, RelposePlan& P) {
  if (!bt || bt->num_pairs < 0 || (bt->num_pairs > 0 && (!bt->corr_ptr || !bt->T_ab || !bt->inliers || !bt->cam_a || !bt->cam_b || !bt->dist_type_a || !bt->dist_type_b)))
    return "NULL array";
  const size_t B = (size_t)bt->num_pairs;
  if (B == 0) return nullptr;
  for (size_t b = 0; b < B; ++b) if (const char* e = csr_row_check(bt->corr_ptr, (int)b, kCorrPtr)) return e;   // (corr_ptr[0] is not required to be 0)
  for (const int32_t* m : {bt->cam_model_a, bt->cam_model_b}) for (size_t b = 0; b < B; ++b) if (const char* e = cam_model_check(m, b)) return e;
  P.model_a.assign(B, COVGPU_CAM_PINHOLE); P.model_b.assign(B, COVGPU_CAM_PINHOLE);
  P.xi_a.assign(B, 0.0); P.xi_b.assign(B, 0.0);
  for (int side = 0; side < 2; ++side) {
    const int32_t* m = side ? bt->cam_model_b : bt->cam_model_a;
    const double* x = side ? bt->xi_b : bt->xi_a;
    std::vector<int32_t>& hm = side ? P.model_b : P.model_a;
    std::vector<double>& hx = side ? P.xi_b : P.xi_a;
    if (!m) continue;
    for (size_t b = 0; b < B; ++b) {
      if (m[b] != COVGPU_CAM_UNIFIED) continue;
      if (const char* e = cam_xi_check(m, x, b, kNoXi)) return e;
      hm[b] = COVGPU_CAM_UNIFIED; hx[b] = x[b]; P.unified = true;
    }
  }
  P.corr = (size_t)bt->corr_ptr[B];
  if (P.corr > 0 && (!bt->p_a || !bt->p_b || !bt->kp_a || !bt->kp_b || !bt->sigma_a || !bt->sigma_b || !bt->outlier)) return "NULL correspondence array";
  return nullptr;
}

struct AbsposePlan {
  size_t corr = 0;
  int max_n = 0;                                // the longest candidate
  std::vector<unsigned long long> seeds;        // (the kernel's type for the 64-bit seeds)
};

inline const char* abspose_check(const covgpu_abspose_batch_t* bt, const covgpu_ransac_opts* opts, AbsposePlan& P) {
  if (!bt || !opts) return "NULL batch or options";
  if (bt->num < 0) return "num < 0";
  if (opts->max_iterations <= 0) return "max_iterations <= 0";
  if (opts->max_iterations > 100000) return "max_iterations > 100000 (a candidate makes up to 11 max_iterations draws in one launch)";
  if (!(opts->probability > 0.0 && opts->probability < 1.0)) return "probability outside (0, 1)";
  if (!std::isfinite(opts->threshold) || !(opts->threshold > 0.0)) return "threshold not finite or not positive";
  const size_t B = (size_t)bt->num;
  if (B == 0) return nullptr;
  if (!bt->corr_ptr || !bt->T_wc || !bt->inliers) return "NULL array";
  if (const char* e = csr_check(bt->corr_ptr, (int)B, kCorrPtr, 0, &P.max_n)) return e;
  P.corr = (size_t)bt->corr_ptr[B];
  if (P.corr > 0 && (!bt->bearing || !bt->point_w || !bt->sigma_angle || !bt->inlier)) return "NULL correspondence array";
  for (size_t i = 0; i < 3 * P.corr; ++i)
    if (!std::isfinite(bt->bearing[i]) || !std::isfinite(bt->point_w[i])) return "non-finite bearing or point";
  P.seeds.resize(B);
  for (size_t b = 0; b < B; ++b) P.seeds[b] = bt->seed ? bt->seed[b] : opts->seed + (uint64_t)b;
  return nullptr;
}

inline const char* p3p_check(int32_t n, const double* f, const double* P, const double* T, const int32_t* nsol, const int32_t* chosen) {
  if (n < 0) return "n < 0";
  if (n == 0) return nullptr;
  if (!f || !P || !T || !nsol || !chosen) return "NULL array";
  for (size_t i = 0; i < 12 * (size_t)n; ++i)
    if (!std::isfinite(f[i]) || !std::isfinite(P[i])) return "non-finite bearing or point";
  return nullptr;
}

// ---- descriptor matching ----

// Query rows per scan workgroup of a matcher and the message of its grid limit.
struct ScanTile { int rows; const char* too_many; };
constexpr ScanTile kMatchTile{kMatchScanRows, "num_jobs * ceil(max query rows / 256) exceeds 2^31 - 1 workgroups"},
    kMatchFloatTile{kMatchFloatTileRows, "num_jobs * ceil(max query rows / 128) exceeds 2^31 - 1 workgroups"};

// What a matching call derives from its sets and jobs: the rows of all sets, per job the first output row, their total, the
// longest query and the longest train set.
struct MatchPlan { size_t rows = 0, total_a = 0; int max_a = 0, max_b = 0; std::vector<int32_t> off; };

// Sets and job table of covgpu_match_batch_t / covgpu_match_float_batch_t (the same fields by name).
template <class Batch>
const char* match_table_check(const Batch* bt, const ScanTile& tile, MatchPlan& P) {
  if (const char* e = desc_sets_check(bt->num_sets, bt->row_ptr)) return e;
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
    P.max_b = std::max(P.max_b, bt->row_ptr[bt->set_b[j] + 1] - bt->row_ptr[bt->set_b[j]]);
  }
  if (P.total_a > 0 && !bt->match) return "NULL match";
  const int tiles = (P.max_a + tile.rows - 1) / tile.rows;   // scan workgroups per job: one 1-D grid of J * tiles
  if ((int64_t)J * tiles > (int64_t)INT32_MAX) return tile.too_many;
  return nullptr;
}

// dist_threshold and ratio of both matchers
inline const char* match_opts_check(const covgpu_match_opts* opts) {
  if (!std::isfinite(opts->dist_threshold) || !(opts->dist_threshold > 0.0f)) return "dist_threshold not finite or not positive";
  if (!std::isfinite(opts->ratio) || !(opts->ratio > 0.0f)) return "ratio not finite or not positive";
  return nullptr;
}

inline const char* match_check(const covgpu_match_batch_t* bt, const covgpu_match_opts* opts, MatchPlan& P) {
  if (!bt || !opts) return "NULL batch or options";
  if (opts->mode != COVGPU_MATCH_DENSE && opts->mode != COVGPU_MATCH_KNN2) return "unknown mode";
  if (const char* e = match_opts_check(opts)) return e;
  if (bt->num_sets < 0 || bt->num_jobs < 0) return "num_sets or num_jobs < 0";
  if (opts->mode != COVGPU_MATCH_DENSE && bt->skip) return "skip must be NULL in KNN2";
  return match_table_check(bt, kMatchTile, P);
}

inline const char* match_float_check(const covgpu_match_float_batch_t* bt, const covgpu_match_opts* opts, MatchPlan& P) {
  if (!bt || !opts) return "NULL batch or options";
  if (opts->mode != COVGPU_MATCH_KNN2) return "mode must be COVGPU_MATCH_KNN2";
  if (const char* e = match_opts_check(opts)) return e;
  if (bt->dim <= 0 || bt->dim % 4 != 0 || bt->dim > kMatchFloatMaxDim) return "dim must be a positive multiple of 4 up to 256";
  if (bt->num_sets < 0 || bt->num_jobs < 0) return "num_sets or num_jobs < 0";
  if (const char* e = match_table_check(bt, kMatchFloatTile, P)) return e;
  // a NaN would leave the order by (distance, index) undefined, and |x|^2 has to stay finite in float32
  for (size_t i = 0; i < P.rows * (size_t)bt->dim; ++i)
    if (!(std::fabs(bt->desc[i]) <= kMatchFloatMaxAbs)) return "descriptor value not finite or above 1e18 in magnitude";
  return nullptr;
}

// ---- guided matching ----

// A scan workgroup's share of a job: `count` (at most kGuidedScanPoints) points from `first`, in direction `dir`. The kernels read it as an int4.
struct GuidedTile { int32_t job, dir, first, count; };

struct GuidedPlan {
  size_t rows = 0, points = 0;                  // keypoint rows of all sets; points of all jobs (PROJECTION)
  size_t tot1 = 0, tot2 = 0;                    // SE3: output rows of the two directions
  std::vector<int32_t> off1, off2;              // SE3: per job the first output row of each direction
  std::vector<GuidedTile> tiles;
  std::vector<double> xi;                       // PROJECTION: per set, 0 for the pinhole rows, whose xi is not read
  void add_tiles(int job, int dir, int n) {
    for (int f = 0; f < n; f += kGuidedScanPoints) tiles.push_back(GuidedTile{job, dir, f, std::min(kGuidedScanPoints, n - f)});
  }
};

// Options and keypoint sets, shared by the two guided entry points.
inline const char* guided_check(const covgpu_keypoint_sets_t& s, const covgpu_guided_opts* o) {
  if (!o) return "NULL options";
  if (o->th_low < 0 || o->th_low > 255) return "th_low outside [0, 255]";
  if (!std::isfinite(o->radius) || !(o->radius > 0.0)) return "radius not finite or not positive";
  if (o->num_octaves < 1) return "num_octaves < 1";
  if (o->num_octaves > 1 && (!std::isfinite(o->scale_factor) || !(o->scale_factor > 1.0))) return "scale_factor not finite or not above 1";
  if (o->agreement != 0 && o->agreement != 1) return "agreement is neither 0 nor 1";
  if (s.num_sets < 0) return "num_sets < 0";
  if (const char* e = desc_sets_check(s.num_sets, s.row_ptr)) return e;
  if (s.num_sets > 0 && !s.bounds) return "NULL bounds";
  if (s.num_sets > 0 && s.row_ptr[s.num_sets] > 0 && (!s.kp || !s.level || !s.desc)) return "NULL keypoint array";
  return nullptr;
}

inline const char* search_se3_check(const covgpu_search_se3_batch_t* bt, const covgpu_guided_opts* opts, GuidedPlan& P) {
  if (!bt) return "NULL batch";
  if (const char* e = guided_check(bt->sets, opts)) return e;
  const covgpu_keypoint_sets_t& s = bt->sets;
  const int S = s.num_sets, J = bt->num_jobs;
  P.rows = S > 0 ? (size_t)s.row_ptr[S] : 0;
  if (J < 0) return "num_jobs < 0";
  if (S > 0 && !bt->K) return "NULL K";
  if (P.rows > 0 && (!bt->lm_pos || !bt->lm_max_distance || !bt->lm_desc || !bt->lm_free)) return "NULL landmark array";
  if (J > 0 && (!bt->set_1 || !bt->set_2 || !bt->T12 || !bt->nfound)) return "NULL job array";
  P.off1.assign(J > 0 ? J : 1, 0); P.off2.assign(J > 0 ? J : 1, 0);
  for (int j = 0; j < J; ++j) {
    if (bt->set_1[j] < 0 || bt->set_1[j] >= S || bt->set_2[j] < 0 || bt->set_2[j] >= S) return "set index out of range";
    for (int k = 0; k < 7; ++k) if (!std::isfinite(bt->T12[7 * (size_t)j + k])) return "non-finite T12";
    const int n1 = s.row_ptr[bt->set_1[j] + 1] - s.row_ptr[bt->set_1[j]], n2 = s.row_ptr[bt->set_2[j] + 1] - s.row_ptr[bt->set_2[j]];
    P.off1[j] = (int32_t)P.tot1; P.off2[j] = (int32_t)P.tot2;
    P.tot1 += (size_t)n1; P.tot2 += (size_t)n2;
    if (P.tot1 > (size_t)INT32_MAX || P.tot2 > (size_t)INT32_MAX) return "more than 2^31 - 1 output rows";
    P.add_tiles(j, 0, n1); P.add_tiles(j, 1, n2);
    if (P.tiles.size() > (size_t)INT32_MAX) return "more than 2^31 - 1 scan workgroups";
  }
  if (P.tot1 > 0 && !bt->match) return "NULL match";
  return nullptr;
}

inline const char* search_projection_check(const covgpu_search_projection_batch_t* bt, const covgpu_guided_opts* opts, GuidedPlan& P) {
  if (!bt) return "NULL batch";
  if (const char* e = guided_check(bt->sets, opts)) return e;
  const covgpu_keypoint_sets_t& s = bt->sets;
  const int S = s.num_sets, J = bt->num_jobs;
  P.rows = S > 0 ? (size_t)s.row_ptr[S] : 0;
  if (J < 0) return "num_jobs < 0";
  if (S > 0 && (!bt->cam || !bt->dist_type)) return "NULL camera array";
  for (int i = 0; i < S; ++i) {
    if (bt->dist_type[i] != COVGPU_DIST_RADTAN && bt->dist_type[i] != COVGPU_DIST_EQUIDISTANT) return "unknown distortion type";
    if (const char* e = cam_check(bt->cam_model, bt->xi, (size_t)i, kNoXi)) return e;
  }
  if (J > 0 && (!bt->set || !bt->T_cw || !bt->point_ptr || !bt->nmatches)) return "NULL job array";
  if (J > 0 && bt->point_ptr[0] != 0) return kPointPtr.first;
  for (int j = 0; j < J; ++j) {
    if (bt->set[j] < 0 || bt->set[j] >= S) return "set index out of range";
    if (const char* e = csr_row_check(bt->point_ptr, j, kPointPtr)) return e;
    for (int k = 0; k < 7; ++k) if (!std::isfinite(bt->T_cw[7 * (size_t)j + k])) return "non-finite T_cw";
    P.add_tiles(j, 0, bt->point_ptr[j + 1] - bt->point_ptr[j]);
  }
  P.points = J > 0 ? (size_t)bt->point_ptr[J] : 0;
  if (P.points > 0 && (!bt->p_w || !bt->normal || !bt->min_distance || !bt->max_distance || !bt->p_desc || !bt->claimed || !bt->remap_to))
    return "NULL point array";
  if (bt->existing_idx)
    for (int j = 0; j < J; ++j) {
      const int n = s.row_ptr[bt->set[j] + 1] - s.row_ptr[bt->set[j]];
      for (int p = bt->point_ptr[j]; p < bt->point_ptr[j + 1]; ++p)
        if (bt->existing_idx[p] < -1 || bt->existing_idx[p] >= n) return "existing_idx out of range";
    }
  P.xi.assign((size_t)S, 0.0);
  if (bt->cam_model) for (int i = 0; i < S; ++i) if (bt->cam_model[i] == COVGPU_CAM_UNIFIED) P.xi[i] = bt->xi[i];
  return nullptr;
}

inline const char* reanchor_check(int32_t K, const double* pose_old, const double* pose_new, int32_t L, const int32_t* ref_kf, const double* lm_pos) {
  if (K < 0 || L < 0 || (K > 0 && (!pose_old || !pose_new)) || (L > 0 && (!ref_kf || !lm_pos))) return "NULL array";
  for (int l = 0; l < L; ++l) if (ref_kf[l] >= K) return "ref_kf out of range";
  return nullptr;
}

// ---- bag-of-words retrieval ----

// A bow CSR over `rows` rows: word ids ascending and duplicate-free, values finite.
inline const char* bow_csr_check(int rows, const int32_t* ptr, const int32_t* word, const double* value) {
  if (rows < 0) return "negative row count";
  if (rows == 0) return nullptr;
  if (!ptr) return "NULL bow_ptr";
  if (const char* e = csr_check(ptr, rows, kBowPtr)) return e;
  if (ptr[rows] > 0 && (!word || !value)) return "NULL word or value";
  for (int r = 0; r < rows; ++r)
    for (int i = ptr[r]; i < ptr[r + 1]; ++i) {
      if (word[i] < 0) return "negative word id";
      if (i > ptr[r] && word[i] <= word[i - 1]) return "word ids of a bow row not ascending and duplicate-free";
      if (!std::isfinite(value[i])) return "non-finite bow value";
    }
  return nullptr;
}

// The vocabulary's tree shape.
inline const char* bow_vocab_check(const covgpu_bow_vocab_t* v) {
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
  if (const char* e = csr_check(v->child_ptr, N, kChildPtr)) return e;
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

// `rows` receives the descriptor rows of all sets.
inline const char* bow_transform_check(const covgpu_bow_vocab_t* v, const covgpu_bow_transform_batch_t* bt, size_t& rows) {
  if (!bt) return "NULL batch";
  if (const char* e = bow_vocab_check(v)) return e;
  const int S = bt->num_sets;
  if (S < 0 || bt->capacity < 0) return "num_sets or capacity < 0";
  if (S > 0 && (!bt->row_ptr || !bt->bow_ptr)) return "NULL row_ptr or bow_ptr";
  if (const char* e = desc_sets_check(S, bt->row_ptr)) return e;
  rows = S > 0 ? (size_t)bt->row_ptr[S] : 0;
  if (rows > 0 && !bt->desc) return "NULL desc";
  if (bt->capacity > 0 && (!bt->word || !bt->value)) return "NULL word or value";
  return nullptr;
}

inline const char* bow_score_pairs_check(int32_t num_vec, const int32_t* bow_ptr, const int32_t* word, const double* value, int32_t num_pairs,
                                         const int32_t* a, const int32_t* b, const double* score) {
  if (const char* e = bow_csr_check(num_vec, bow_ptr, word, value)) return e;
  if (num_pairs < 0) return "num_pairs < 0";
  if (num_pairs > 0 && (!a || !b || !score)) return "NULL pair array";
  for (int i = 0; i < num_pairs; ++i)
    if (a[i] < 0 || a[i] >= num_vec || b[i] < 0 || b[i] >= num_vec) return "pair index out of range";
  return nullptr;
}

// Host side of a detect call: keyframe -> database position, the reference-score pairs (query keyframe, valid neighbour) with their
// per-query offsets, and the inverted index of the database (posting lists in insertion order). Filled only for num_queries > 0.
struct DetectPlan {
  size_t num_nb = 0;
  int max_words = 0, inv_words = 0;             // longest query vector; words of the inverted index
  std::vector<int32_t> pos_of, pair_a, pair_b, pair_off, inv_ptr, inv_pos;
};

inline const char* detect_check(const covgpu_detect_batch_t* bt, const covgpu_detect_opts* opts, DetectPlan& P) {
  if (!bt || !opts) return "NULL batch or options";
  if (!std::isfinite(opts->min_score_factor)) return "non-finite min_score_factor";
  if (opts->scratch_kib < 0) return "scratch_kib < 0";
  const int N = bt->num_kf, M = bt->num_db, Q = bt->num_queries, cap = bt->cap;
  if (N < 0 || M < 0 || Q < 0 || cap < 0) return "negative count";
  if (N > 0 && (!bt->id || !bt->client || !bt->nb_ptr)) return "NULL keyframe array";
  for (int k = 0; k < N; ++k) if (bt->id[k] < 0) return "negative keyframe id";
  if (const char* e = bow_csr_check(N, bt->bow_ptr, bt->word, bt->value)) return e;
  if (N > 0) if (const char* e = csr_check(bt->nb_ptr, N, kNbPtr)) return e;
  P.num_nb = N > 0 ? (size_t)bt->nb_ptr[N] : 0;
  if (P.num_nb > 0 && !bt->nb) return "NULL nb";
  for (size_t i = 0; i < P.num_nb; ++i) if (bt->nb[i] < 0 || bt->nb[i] >= N) return "neighbour index out of range";
  if (M > 0 && !bt->db_order) return "NULL db_order";
  P.pos_of.assign(N > 0 ? N : 1, -1);
  for (int p = 0; p < M; ++p) {
    const int k = bt->db_order[p];
    if (k < 0 || k >= N) return "db_order index out of range";
    if (P.pos_of[k] >= 0) return "db_order repeats a keyframe";
    P.pos_of[k] = p;
  }
  if (Q > 0 && (!bt->query_kf || !bt->db_visible || !bt->num_candidates)) return "NULL query array";
  if (Q > 0 && cap > 0 && !bt->candidates) return "NULL candidates";
  size_t num_pairs = 0;
  for (int q = 0; q < Q; ++q) {
    const int k = bt->query_kf[q];
    if (k < 0 || k >= N) return "query_kf out of range";
    if (bt->db_visible[q] < 0 || bt->db_visible[q] > M) return "db_visible is not in 0..num_db";
    if (bt->min_score_in && std::isnan(bt->min_score_in[q])) return "min_score_in is NaN";
    P.max_words = std::max(P.max_words, bt->bow_ptr[k + 1] - bt->bow_ptr[k]);
    num_pairs += (size_t)(bt->nb_ptr[k + 1] - bt->nb_ptr[k]);
  }
  if (num_pairs > (size_t)INT32_MAX) return "more than 2^31 - 1 query neighbours";
  if (Q == 0) return nullptr;
  P.pair_off.assign((size_t)Q + 1, 0);
  if (!bt->min_score_in) {
    P.pair_a.reserve(num_pairs); P.pair_b.reserve(num_pairs);
    for (int q = 0; q < Q; ++q) {
      const int k = bt->query_kf[q];
      for (int i = bt->nb_ptr[k]; i < bt->nb_ptr[k + 1]; ++i) {
        if (bt->invalid && bt->invalid[bt->nb[i]]) continue;
        P.pair_a.push_back(k); P.pair_b.push_back(bt->nb[i]);
      }
      P.pair_off[q + 1] = (int32_t)P.pair_a.size();
    }
  }
  for (int p = 0; p < M; ++p) {
    const int k = bt->db_order[p];
    if (bt->bow_ptr[k + 1] > bt->bow_ptr[k]) P.inv_words = std::max(P.inv_words, bt->word[bt->bow_ptr[k + 1] - 1] + 1);
  }
  P.inv_ptr.assign((size_t)P.inv_words + 1, 0);
  for (int p = 0; p < M; ++p) {
    const int k = bt->db_order[p];
    for (int i = bt->bow_ptr[k]; i < bt->bow_ptr[k + 1]; ++i) ++P.inv_ptr[bt->word[i] + 1];
  }
  for (int w = 0; w < P.inv_words; ++w) {
    if ((int64_t)P.inv_ptr[w + 1] + P.inv_ptr[w] > (int64_t)INT32_MAX) return "more than 2^31 - 1 database words";
    P.inv_ptr[w + 1] += P.inv_ptr[w];
  }
  P.inv_pos.resize((size_t)P.inv_ptr[P.inv_words]);
  std::vector<int32_t> fill(P.inv_ptr.begin(), P.inv_ptr.end() - 1);
  for (int p = 0; p < M; ++p) {
    const int k = bt->db_order[p];
    for (int i = bt->bow_ptr[k]; i < bt->bow_ptr[k + 1]; ++i) P.inv_pos[fill[bt->word[i]]++] = p;
  }
  return nullptr;
}

// ---- map maintenance ----

inline const char* prune_check(const covgpu_prune_t* p, const covgpu_prune_opts* o) {
  if (!p || !o) return "NULL problem or options";
  if (!std::isfinite(o->th_red) || !std::isfinite(o->max_time_dist)) return "non-finite th_red or max_time_dist";
  const int K = p->num_kf, L = p->num_lm;
  if (K < 0 || L < 0 || p->capacity < 0) return "negative count";
  if (!p->lm_obs_ptr) return "NULL lm_obs_ptr";
  if (const char* e = csr_check(p->lm_obs_ptr, L, kLmObsPtr)) return e;
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

inline const char* lm_refresh_check(const covgpu_landmark_refresh_t* p, const covgpu_landmark_refresh_opts* o) {
  if (!p || !o) return "NULL problem or options";
  if (!std::isfinite(o->scale_factor) || !(o->scale_factor > 0.0)) return "scale_factor not finite or not positive";
  if (o->num_octaves < 1 || o->num_octaves > 64) return "num_octaves outside [1, 64]";
  const int K = p->num_kf, L = p->num_lm;
  if (K < 0 || L < 0) return "negative count";
  if (!p->lm_obs_ptr) return "NULL lm_obs_ptr";
  if (const char* e = csr_check(p->lm_obs_ptr, L, kLmObsPtr)) return e;
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

// ---- vocabulary training ----

// k^L, or 0 if it exceeds COVGPU_BOW_MAX_WORDS
inline int64_t voc_full_words(int k, int L) {
  int64_t w = 1;
  for (int l = 0; l < L; ++l) { w *= k; if (w > COVGPU_BOW_MAX_WORDS) return 0; }
  return w;
}

inline const char* voc_train_check(const covgpu_voc_train_t* p, const covgpu_voc_train_opts* o) {
  if (!p || !o) return "NULL problem or options";
  if (o->k < 2) return "k < 2";
  if (o->k > COVGPU_VOCTRAIN_MAX_K) return "k > COVGPU_VOCTRAIN_MAX_K";
  if (o->L < 1) return "L < 1";
  const int64_t full = voc_full_words(o->k, o->L);
  if (!full) return "k^L > COVGPU_BOW_MAX_WORDS";
  if (o->weighting < COVGPU_BOW_TF_IDF || o->weighting > COVGPU_BOW_BINARY) return "unknown weighting";
  if (o->scoring != COVGPU_BOW_L1_NORM) return "only L1_NORM scoring is supported";
  if (o->max_iterations < 1) return "max_iterations < 1";
  if ((int64_t)o->scratch_kib * 8192 < full) return "scratch_kib below one set's word bitmap, ceil(k^L / 8192)";
  const int S = p->num_sets;
  if (S < 0 || p->node_capacity < 0) return "num_sets or node_capacity < 0";
  if (S == 0) return "no descriptor rows";
  if (!p->row_ptr) return "NULL row_ptr";
  if (const char* e = csr_check(p->row_ptr, S, kRowPtr)) return e;   // (no limit on the rows of a set)
  if (p->row_ptr[S] == 0) return "no descriptor rows";
  if (p->row_ptr[S] > INT32_MAX - COVGPU_VOCTRAIN_TILE) return "more than 2^31 - 1 - COVGPU_VOCTRAIN_TILE rows";   // a tile's position loop steps past its end
  if (!p->desc) return "NULL desc";
  if (!p->num_nodes || !p->num_words) return "NULL num_nodes or num_words";
  if (p->node_capacity > 0 && (!p->parent || !p->desc_out || !p->word_id || !p->weight)) return "NULL output array";
  return nullptr;
}

}  // namespace covgpu
