// optimization_gpu.hpp — header-only C++ facade: covins::Optimization::{GlobalBundleAdjustment,
// PoseGraphOptimization} re-implemented on top of the C ABI of libcovgpu (include/covgpu.h).
//
// Drop-in boundary. The reference declares, in covins_backend/include/covins/covins_backend/
// optimization_be.hpp:38-51,
//     static auto GlobalBundleAdjustment(MapPtr map, int interations_limit, double time_limit,
//                                        bool visual_only = false, bool outlier_removal = true,
//                                        bool estimate_bias = false) -> void;
//     static auto PoseGraphOptimization(MapPtr map, PoseMap corrected_poses) -> void;
// and callers link those symbols directly (backend.cpp:141-156, placerec_be.cpp:327, placerec_gen_be.cpp:250).
// `covins_gpu::OptimizationT<Types>` keeps both signatures verbatim. It walks Map / Keyframe / Landmark with the
// very accessors optimization_be.cpp uses (GetKeyframesVec, IsInvalid, UpdateCeresFromState-equivalent reads,
// GetObservations, GetPredecessor, GetLoopConstraints, ...), applies the same gating rules and constants, and
// replaces each `ceres::Problem` + `ceres::Solve` by one flat `covgpu_problem` + covgpu_gba_solve /
// covgpu_pgo_solve. Write-back and map maintenance follow optimization_be.cpp:572-614 and :1037-1083.
//
// The header is Eigen-free on purpose (no Eigen in this build image): 4x4 transforms, 3-vectors and 6x6
// matrices are only touched through operator()(r,c) / operator[](i), which Eigen types and the test stand-ins
// (tests/cpp/standin_map.hpp) both provide. `Types` names the map classes and the few operations whose
// spelling differs between the real COVINS classes and a stand-in (see INTEGRATION.md for the COVINS binding).
#pragma once
#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <map>
#include <unordered_map>
#include <memory>
#include <set>
#include <stdexcept>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../covgpu.h"

namespace covins_gpu {

// covins_params::opt / sys / placerec values read on this path (config/config_backend.yaml:8,115-140;
// config_backend.hpp:180-207). A plain struct instead of static-init globals.
struct Params {
  int gba_use_map_loop_constraints = 1;
  double th_gba_outlier_global = 0.92;
  int gba_fix_poses_loaded_maps = 0;
  int pgo_iteration_limit = 10;
  int use_nbr_kfs = 1;
  int use_robust_loss = 1;
  double robust_loss_th = 0.5;
  int pgo_fix_kfs_after_gba = 1;
  int pgo_fix_poses_loaded_maps = 0;
  double wt_kf_r = 10.0, wt_kf_t = 1.0, wt_kf_n1 = 10.0, wt_kf_n23 = 2.0, wt_kf_n45 = 3.0;
  double th_outlier_align = 1.3;   // opt.th_outlier_align (config_backend.yaml:117), OptimizeRelativePose
  std::string placerec_type = "COVINS";
  int strategy = COVGPU_DOGLEG;  // the reference runs DOGLEG (optimization_be.cpp:261,564,1028)
  int device = 0;
  // multi-GPU GlobalBundleAdjustment inside this one process (covgpu_gba_solve_multi): ranks > 1 shards the ONE map by sub-map
  // over `ranks` contexts; rank r runs on HIP device devices[r] (empty: devices 0 .. ranks-1). Ranks on different devices talk
  // over RCCL; ranks that share a device (a one-GPU box: the test form) over the library's in-process group.
  int n_gpus = 1;
  std::vector<int> devices;
  // how the sharded solve (n_gpus > 1) treats the top of the elimination tree: 0 replicated and all-reduced whole (default) | 1 distributed —
  // all-reduced a 256-column panel at a time, the trailing updates split over the ranks (covgpu_options::shard_policy)
  int shard_policy = 0;
  int flatten_threads = 0;  // host threads of the Map -> IR walk over landmarks; 0 = sys.threads_server-like default (hardware, <= 16)
  // GlobalBundleAdjustment with outlier removal: derive the second round's problem on the device from the resident first round
  // (covgpu_gba_two_round: ONE Map -> IR walk and ONE upload per call); 0: the reference's literal sequence — walk, solve, erase, walk, solve
  int device_second_round = 1;
  // Opt-in (0: the call ends with the reference's own map->Clean(), optimization_be.cpp:614). 1: the end of the two-round call reproduces what
  // Map::Clean's map check does (map_be.cpp:698-717: every landmark of the map whose observation map holds fewer than two entries is erased)
  // from counts the call already has — the Map -> IR walk visited every landmark's observations once, the device returned how many of them
  // each landmark kept — instead of copying every landmark's observation map AGAIN to read its size (50 ms of a 180 ms call on the 5-agent
  // map). NOT reproduced: Clean's second loop over every keyframe's landmark vector (:719-729), which only finds landmarks that a keyframe
  // references but the map does not list — none in a consistent map. tests/test_facade.py compares the two ends.
  int device_clean = 0;
  // loop-candidate geometric verification, Se3Solver (config_backend.yaml:85-88: placerec.ransac.*). ransac_probability: the reference's
  // Se3Solver stores its ransacProb but never hands it to opengv, which runs with its own default 0.99 — the facade's Se3Solver uses this
  // value, not the constructor's, so the default reproduces the reference
  int ransac_min_inliers = 6;
  double ransac_probability = 0.99;
  int ransac_max_iterations = 300;
  double ransac_class_threshold = 25;
  // (IMU noise and gravity are NOT parameters: every IMU factor carries its keyframe's own VICalibration values,
  //  Types::imu_calib, as the reference's per-keyframe preintegrators do — keyframe_be.cpp:187-195.)
};

namespace detail {

// f(keyframe, feature index) for every observation of a landmark: through Types::visit_observations(landmark, f) when the binding
// offers it (a walk under the landmark's lock, no copy), otherwise over the copy Landmark::GetObservations() returns — a
// std::map of smart pointers: one allocation and one atomic reference-count round trip per observation, 60 % of the walk.
template <class Types, class L, class F>
inline auto visit_observations(const L& lm, F&& f, int) -> decltype(Types::visit_observations(lm, f), void()) { Types::visit_observations(lm, f); }
template <class Types, class L, class F>
inline void visit_observations(const L& lm, F&& f, long) { const auto obs = lm.GetObservations(); for (auto& m : obs) f(m.first, m.second); }

// projection model of a keyframe's camera through the optional trait Types::camera_model(keyframe, &model, &xi) (COVGPU_CAM_*; false =
// unknown model); a binding without it has pinhole cameras only
template <class Types, class K>
inline auto camera_model(const K& kf, int* model, double* xi, int) -> decltype(Types::camera_model(kf, model, xi), bool()) {
  return Types::camera_model(kf, model, xi);
}
template <class Types, class K>
inline bool camera_model(const K&, int* model, double* xi, long) { *model = COVGPU_CAM_PINHOLE; *xi = 0.0; return true; }

// unit bearing of feature i of a keyframe through the optional trait Types::bearing(keyframe, i, out3) (false: i is past the keyframe's
// bearings_); without it keyframe_be.cpp:209-218 on keypoints_undistorted_ and the pinhole intrinsics of Types::camera
template <class Types, class K>
inline auto bearing(const K& kf, size_t i, double* out, int) -> decltype(Types::bearing(kf, i, out), bool()) {
  return Types::bearing(kf, i, out);
}
template <class Types, class K>
inline bool bearing(const K& kf, size_t i, double* out, long) {
  if (i >= kf.keypoints_undistorted_.size()) return false;
  double intr[4], dist[4]; int dt = 0;
  if (!Types::camera(kf, intr, dist, &dt)) return false;
  const double x = (kf.keypoints_undistorted_[i][0] - intr[2]) * (1.0 / intr[0]), y = (kf.keypoints_undistorted_[i][1] - intr[3]) * (1.0 / intr[1]);
  const double n = std::sqrt(x * x + y * y + 1.0);
  out[0] = x / n; out[1] = y / n; out[2] = 1.0 / n;
  return true;
}

// descriptor matrix of a keyframe (which = 0: descriptors_, the ORB rows of its keypoints; 1: descriptors_add_, COVINS-G's) through the
// optional trait Types::descriptors(keyframe, which, &rows, &data) (false: none); without it the cv::Mat fields rows / data, which hold
// 32-byte CV_8U rows back to back as ORB extraction leaves them. The keyframe is taken non-const: KeyframeBase's accessors are.
template <class Types, class K>
inline auto descriptors(K& kf, int which, int* rows, const uint8_t** data, int)
    -> decltype(Types::descriptors(kf, which, rows, data), bool()) {
  return Types::descriptors(kf, which, rows, data);
}
template <class Types, class K>
inline bool descriptors(K& kf, int which, int* rows, const uint8_t** data, long) {
  const auto& M = which == 0 ? kf.descriptors_ : kf.descriptors_add_;
  *rows = M.rows; *data = reinterpret_cast<const uint8_t*>(M.data);
  return true;
}

// landmark of feature k through the optional trait Types::landmark(keyframe, k); without it KeyframeBase::GetLandmark(k), which COVINS
// declares non-const (keyframe_base.hpp:124)
template <class Types, class K>
inline auto landmark(K& kf, size_t k, int) -> decltype(Types::landmark(kf, k)) { return Types::landmark(kf, k); }
template <class Types, class K>
inline auto landmark(K& kf, size_t k, long) -> decltype(kf.GetLandmark((int)k)) { return kf.GetLandmark((int)k); }

// ---- what the guided matching (LoopMatcherT::SearchBySE3Batch / SearchByProjection) reads beyond the above, each through an optional
//      trait with the COVINS member as the fallback.
// Landmark::GetDescriptor() (landmark_base.hpp:77), 32 bytes copied out: Types::landmark_descriptor(landmark, out32); false = none
template <class Types, class L>
inline auto landmark_descriptor(L& lm, uint8_t* out, int) -> decltype(Types::landmark_descriptor(lm, out), bool()) {
  return Types::landmark_descriptor(lm, out);
}
template <class Types, class L>
inline bool landmark_descriptor(L& lm, uint8_t* out, long) {
  const auto M = lm.GetDescriptor();
  if (M.cols * M.rows < 32) return false;
  std::memcpy(out, M.data, 32);
  return true;
}
// normal_, min_distance_, max_distance_ of a landmark: Types::landmark_scale(landmark, normal3, &min, &max). LandmarkBase keeps them
// protected; the fallback divides GetMinDistanceInvariance() / GetMaxDistanceInvariance() by their 0.8 / 1.2 (landmark_base.cpp:68-76),
// which can differ from the member in the last bit — a binding that wants the reference's decisions to the bit supplies the trait.
template <class Types, class L>
inline auto landmark_scale(L& lm, double* n, double* mn, double* mx, int) -> decltype(Types::landmark_scale(lm, n, mn, mx), void()) {
  Types::landmark_scale(lm, n, mn, mx);
}
template <class Types, class L>
inline void landmark_scale(L& lm, double* n, double* mn, double* mx, long) {
  const auto v = lm.GetNormal();
  n[0] = v[0]; n[1] = v[1]; n[2] = v[2];
  *mn = lm.GetMinDistanceInvariance() / 0.8; *mx = lm.GetMaxDistanceInvariance() / 1.2;
}
// IsInImage's bounds (xmin xmax ymin ymax, keyframe_base.cpp:414-416) and the grid state (grid_width_inv_, grid_height_inv_ when
// assigned_to_grid_, else 0 0 = brute-force order, :273): Types::keyframe_image(keyframe, bounds4, grid_inv2)
template <class Types, class K>
inline auto keyframe_image(K& kf, double* b, double* g, int) -> decltype(Types::keyframe_image(kf, b, g), void()) { Types::keyframe_image(kf, b, g); }
template <class Types, class K>
inline void keyframe_image(K& kf, double* b, double* g, long) {
  b[0] = kf.img_dim_x_min_; b[1] = kf.img_dim_x_max_; b[2] = kf.img_dim_y_min_; b[3] = kf.img_dim_y_max_;
  g[0] = kf.assigned_to_grid_ ? kf.grid_width_inv_ : 0.0; g[1] = kf.assigned_to_grid_ ? kf.grid_height_inv_ : 0.0;
}
// Keyframe::RemapLandmark(lm, now, new) (keyframe_be.cpp:484-495): Types::remap_landmark(keyframe_ptr, landmark_ptr, now, new)
template <class Types, class KP, class LP>
inline auto remap_landmark(const KP& kf, const LP& lm, size_t now, size_t to, int) -> decltype(Types::remap_landmark(kf, lm, now, to), void()) {
  Types::remap_landmark(kf, lm, now, to);
}
template <class Types, class KP, class LP>
inline void remap_landmark(const KP& kf, const LP& lm, size_t now, size_t to, long) { kf->RemapLandmark(lm, now, to); }

// ---- what LandmarkRefreshT writes and reads beyond the above.
// descriptor_ of a landmark (32 bytes): Types::set_landmark_descriptor(landmark, bytes32); normal_, min_distance_, max_distance_:
// Types::set_landmark_scale(landmark, normal3, min, max). LandmarkBase keeps these members protected and offers no setter, so there is
// no COVINS member to fall back on: a binding that instantiates LandmarkRefreshT supplies both.
template <class Types, class L>
inline auto set_landmark_descriptor(L& lm, const uint8_t* d, int) -> decltype(Types::set_landmark_descriptor(lm, d), void()) {
  Types::set_landmark_descriptor(lm, d);
}
template <class Types, class L>
inline void set_landmark_descriptor(L&, const uint8_t*, long) {
  static_assert(sizeof(L) == 0, "LandmarkRefreshT needs Types::set_landmark_descriptor(landmark, bytes32)");
}
template <class Types, class L>
inline auto set_landmark_scale(L& lm, const double* n, double mn, double mx, int) -> decltype(Types::set_landmark_scale(lm, n, mn, mx), void()) {
  Types::set_landmark_scale(lm, n, mn, mx);
}
template <class Types, class L>
inline void set_landmark_scale(L&, const double*, double, double, long) {
  static_assert(sizeof(L) == 0, "LandmarkRefreshT needs Types::set_landmark_scale(landmark, normal3, min, max)");
}
// camera centre of a keyframe, the translation of GetPoseTwc(): Types::camera_center(keyframe, out3), else the member
template <class Types, class K>
inline auto camera_center(K& kf, double* c, int) -> decltype(Types::camera_center(kf, c), void()) { Types::camera_center(kf, c); }
template <class Types, class K>
inline void camera_center(K& kf, double* c, long) { const auto T = kf.GetPoseTwc(); c[0] = T(0, 3); c[1] = T(1, 3); c[2] = T(2, 3); }

// RANSAC seed of a (query, candidate) keyframe pair from their ids: a candidate's draws do not depend on the batch it is verified in
template <class K>
inline uint64_t abspose_seed(const K* query, const K* cand) {
  auto id = [](const K* k) -> uint64_t { return k ? ((uint64_t)k->id_.first << 20) ^ (uint64_t)k->id_.second : 0; };
  return id(query) * 0x9E3779B97F4A7C15ull + id(cand);
}

// seed of cell `cell` of the five-point grid of a (query, candidate) keyframe pair: the pair's seed, moved by the cell
template <class K>
inline uint64_t fivept_seed(const K* kf1, const K* kf2, uint64_t cell) {
  return abspose_seed(kf1, kf2) + cell * 0xD1B54A32D192ED03ull;
}

// seed of the 17-point job of a (query, candidate) keyframe pair: the pair's seed, moved off every cell of its five-point grid
template <class K>
inline uint64_t ncrelpose_seed(const K* kf_query, const K* kf_cand) {
  return abspose_seed(kf_query, kf_cand) ^ 0x17D1B54A32D192EDull;
}

inline void fatal(const char* msg) {  // the reference prints COUTFATAL and exit(-1) (e.g. optimization_be.cpp:113-114)
  std::fprintf(stderr, "[covins_gpu] FATAL: %s\n", msg);
  std::exit(-1);
}

// unit bearing of additional feature i of a keyframe (COVINS-G: bearings_add_, frame-relative-adapter.cpp:27-38) through the optional
// trait Types::bearing_add(keyframe, i, out3); without it kf.bearings_add_[i], read by [0..2]. Normalised here, as the adapter does.
template <class Types, class K>
inline auto bearing_add_raw(K& kf, size_t i, double* out, int) -> decltype(Types::bearing_add(kf, i, out), void()) { Types::bearing_add(kf, i, out); }
template <class Types, class K>
inline void bearing_add_raw(K& kf, size_t i, double* out, long) {
  if (i >= kf.bearings_add_.size()) fatal("five-point: a match indexes past bearings_add_");
  const auto& b = kf.bearings_add_[i];
  out[0] = b[0]; out[1] = b[1]; out[2] = b[2];
}
template <class Types, class K>
inline void bearing_add(K& kf, size_t i, double* out) {
  bearing_add_raw<Types>(kf, i, out, 0);
  const double n = std::sqrt(out[0] * out[0] + out[1] * out[1] + out[2] * out[2]);
  out[0] /= n; out[1] /= n; out[2] /= n;
}

// float descriptor matrix of a keyframe (COVINS-G with feat.type SIFT: descriptors_add_ as `dim`-float rows) through the optional trait
// Types::descriptors_f32(keyframe, &rows, &dim, &data) (false: none); without it descriptors_add_ read as a continuous CV_32F cv::Mat
// (rows, cols, data). A non-empty matrix of another type is fatal: the reference's FLANN matcher throws on it.
template <class Types, class K>
inline auto descriptors_f32(K& kf, int* rows, int* dim, const float** data, int)
    -> decltype(Types::descriptors_f32(kf, rows, dim, data), bool()) {
  return Types::descriptors_f32(kf, rows, dim, data);
}
template <class Types, class K>
inline bool descriptors_f32(K& kf, int* rows, int* dim, const float** data, long) {
  const auto& M = kf.descriptors_add_;
  constexpr int kCv32F = 5;                                            // CV_32FC1 (opencv2/core/hal/interface.h)
  if (M.rows > 0 && (M.type() != kCv32F || !M.isContinuous())) fatal("descriptors_add_ is not a continuous CV_32F matrix (feat.type SIFT)");
  *rows = M.rows; *dim = M.cols; *data = reinterpret_cast<const float*>(M.data);
  return true;
}

// rotation matrix (rows/cols 0..2 of any (r,c)-indexable) -> Hamilton quaternion x,y,z,w (what Eigen::Quaterniond(R) yields)
template <class M>
inline void rot_to_quat(const M& T, double* q) {
  const double m00 = T(0, 0), m11 = T(1, 1), m22 = T(2, 2), tr = m00 + m11 + m22;
  double x, y, z, w;
  if (tr > 0) {
    const double s = std::sqrt(tr + 1.0) * 2;
    w = 0.25 * s; x = (T(2, 1) - T(1, 2)) / s; y = (T(0, 2) - T(2, 0)) / s; z = (T(1, 0) - T(0, 1)) / s;
  } else if (m00 > m11 && m00 > m22) {
    const double s = std::sqrt(1.0 + m00 - m11 - m22) * 2;
    w = (T(2, 1) - T(1, 2)) / s; x = 0.25 * s; y = (T(0, 1) + T(1, 0)) / s; z = (T(0, 2) + T(2, 0)) / s;
  } else if (m11 > m22) {
    const double s = std::sqrt(1.0 + m11 - m00 - m22) * 2;
    w = (T(0, 2) - T(2, 0)) / s; x = (T(0, 1) + T(1, 0)) / s; y = 0.25 * s; z = (T(1, 2) + T(2, 1)) / s;
  } else {
    const double s = std::sqrt(1.0 + m22 - m00 - m11) * 2;
    w = (T(1, 0) - T(0, 1)) / s; x = (T(0, 2) + T(2, 0)) / s; y = (T(1, 2) + T(2, 1)) / s; z = 0.25 * s;
  }
  const double n = std::sqrt(x * x + y * y + z * z + w * w);
  q[0] = x / n; q[1] = y / n; q[2] = z / n; q[3] = w / n;
}
// pose block [qx qy qz qw px py pz] from a 4x4 transform (keyframe_base.cpp:486-499)
template <class M>
inline void transform_to_pose(const M& T, double* p) {
  rot_to_quat(T, p);
  p[4] = T(0, 3); p[5] = T(1, 3); p[6] = T(2, 3);
}
// Utils::Ceres2Transform (utils_base.cpp:28-43): normalise q, fill a 4x4
template <class M>
inline void pose_to_transform(const double* p, M& T) {
  double x = p[0], y = p[1], z = p[2], w = p[3];
  const double n = std::sqrt(x * x + y * y + z * z + w * w);
  x /= n; y /= n; z /= n; w /= n;
  T(0, 0) = 1 - 2 * (y * y + z * z); T(0, 1) = 2 * (x * y - w * z);     T(0, 2) = 2 * (x * z + w * y);     T(0, 3) = p[4];
  T(1, 0) = 2 * (x * y + w * z);     T(1, 1) = 1 - 2 * (x * x + z * z); T(1, 2) = 2 * (y * z - w * x);     T(1, 3) = p[5];
  T(2, 0) = 2 * (x * z - w * y);     T(2, 1) = 2 * (y * z + w * x);     T(2, 2) = 1 - 2 * (x * x + y * y); T(2, 3) = p[6];
  T(3, 0) = 0; T(3, 1) = 0; T(3, 2) = 0; T(3, 3) = 1;
}
// [q,t] of Ta^-1 Tb for two 4x4 transforms (optimization_be.cpp:956-958, 1006-1008)
template <class M>
inline void relative_pose(const M& Ta, const M& Tb, double* out7) {
  double R[3][3], t[3];
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) {
      R[r][c] = 0;
      for (int k = 0; k < 3; ++k) R[r][c] += Ta(k, r) * Tb(k, c);
    }
    t[r] = 0;
    for (int k = 0; k < 3; ++k) t[r] += Ta(k, r) * (Tb(k, 3) - Ta(k, 3));
  }
  struct V { double (*R)[3]; double operator()(int r, int c) const { return R[r][c]; } } v{R};
  rot_to_quat(v, out7);
  out7[4] = t[0]; out7[5] = t[1]; out7[6] = t[2];
}
// upper-triangular chol(A^-1)^T of a 6x6 SPD matrix given row-major (optimization_be.cpp:922-923)
inline void sqrt_info_from_cov(const double* cov, double* S) {
  double A[6][12];
  for (int r = 0; r < 6; ++r) for (int c = 0; c < 6; ++c) { A[r][c] = cov[6 * r + c]; A[r][6 + c] = (r == c); }
  for (int c = 0; c < 6; ++c) {  // Gauss-Jordan with partial pivoting
    int p = c;
    for (int r = c + 1; r < 6; ++r) if (std::fabs(A[r][c]) > std::fabs(A[p][c])) p = r;
    for (int k = 0; k < 12; ++k) std::swap(A[c][k], A[p][k]);
    const double d = A[c][c];
    for (int k = 0; k < 12; ++k) A[c][k] /= d;
    for (int r = 0; r < 6; ++r) if (r != c) { const double f = A[r][c]; for (int k = 0; k < 12; ++k) A[r][k] -= f * A[c][k]; }
  }
  double L[6][6] = {};
  for (int j = 0; j < 6; ++j) {
    double d = A[j][6 + j];
    for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
    L[j][j] = std::sqrt(d);
    for (int i = j + 1; i < 6; ++i) {
      double s = A[i][6 + j];
      for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
      L[i][j] = s / L[j][j];
    }
  }
  for (int r = 0; r < 6; ++r) for (int c = 0; c < 6; ++c) S[6 * r + c] = L[c][r];
}

// C = A B for 4x4 transforms; p_cam = (T_w_c)^-1 p_w
template <class M>
inline void mat_mul(const M& A, const M& B, M& C) {
  for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) { double s = 0; for (int k = 0; k < 4; ++k) s += A(r, k) * B(k, c); C(r, c) = s; }
}
template <class M, class V>
inline void to_camera(const M& Twc, const V& pw, double* out3) {
  for (int r = 0; r < 3; ++r) { double s = 0; for (int k = 0; k < 3; ++k) s += Twc(k, r) * (pw[k] - Twc(k, 3)); out3[r] = s; }
}

struct Flat {  // owning storage behind one covgpu_problem
  std::vector<double> pose, sb, cam_extr, cam_intr, cam_dist, lm, uv, sigma, samples, first, noise, meas, info, loss;
  std::vector<uint8_t> fixed;
  std::vector<int32_t> kf_cam, cam_type, obs_ptr, obs_kf, imu_i, imu_j, imu_ptr, ei, ej;
  std::vector<int32_t> cam_model;   // [A] COVGPU_CAM_*
  std::vector<double> cam_xi;       // [A]
  covgpu_problem view() {
    covgpu_problem p{};
    p.num_kf = (int32_t)fixed.size(); p.num_cam = (int32_t)cam_type.size(); p.num_lm = (int32_t)(lm.size() / 3);
    p.num_obs = (int32_t)obs_kf.size(); p.num_imu = (int32_t)imu_i.size(); p.num_edge = (int32_t)ei.size();
    p.num_imu_samples = (int32_t)(samples.size() / 7);
    if (obs_ptr.empty()) obs_ptr.push_back(0);
    if (imu_ptr.empty()) imu_ptr.push_back(0);
    p.kf_pose = pose.data(); p.kf_speed_bias = sb.data(); p.kf_fixed = fixed.data(); p.kf_cam = kf_cam.data();
    p.cam_extr = cam_extr.data(); p.cam_intr = cam_intr.data(); p.cam_dist = cam_dist.data(); p.cam_dist_type = cam_type.data();
    p.lm_pos = lm.data(); p.lm_obs_ptr = obs_ptr.data(); p.obs_kf = obs_kf.data(); p.obs_uv = uv.data(); p.obs_sigma = sigma.data();
    p.imu_kf_i = imu_i.data(); p.imu_kf_j = imu_j.data(); p.imu_sample_ptr = imu_ptr.data(); p.imu_samples = samples.data();
    p.imu_first = first.data(); p.imu_noise = noise.data();
    p.edge_i = ei.data(); p.edge_j = ej.data(); p.edge_meas = meas.data(); p.edge_sqrt_info = info.data(); p.edge_loss_a = loss.data();
    bool uni = false;   // camera models only when some camera is unified (a pinhole-only map runs the pinhole kernels, NULL)
    for (int32_t m : cam_model) uni = uni || m == COVGPU_CAM_UNIFIED;
    if (uni && cam_model.size() == cam_type.size()) { p.cam_model = cam_model.data(); p.cam_xi = cam_xi.data(); }
    return p;
  }
};

// ---- what the bag-of-words retrieval (KeyframeDatabaseT) reads and writes, each through an optional trait with the COVINS member as
//      the fallback: bow_vec_ (DBoW2::BowVector, a std::map<WordId, WordValue>), feat_vec_ (DBoW2::FeatureVector, a std::map<NodeId,
//      std::vector<unsigned>>) and the covisibility neighbours in the reference's order.
template <class Types, class K, class F>
inline auto visit_bow(K& kf, F&& f, int) -> decltype(Types::visit_bow(kf, f), void()) { Types::visit_bow(kf, f); }
template <class Types, class K, class F>
inline void visit_bow(K& kf, F&& f, long) { for (const auto& e : kf.bow_vec_) f((int32_t)e.first, (double)e.second); }
template <class Types, class K>
inline auto set_bow(K& kf, size_t n, const int32_t* word, const double* value, int) -> decltype(Types::set_bow(kf, n, word, value), void()) {
  Types::set_bow(kf, n, word, value);
}
template <class Types, class K>
inline void set_bow(K& kf, size_t n, const int32_t* word, const double* value, long) {
  kf.bow_vec_.clear();
  for (size_t i = 0; i < n; ++i) kf.bow_vec_[word[i]] = value[i];
}
// per descriptor row its word (-1: stopped, no entry) and FeatureVector key: fv.addFeature(nid, i_feature) in row order
template <class Types, class K>
inline auto set_features(K& kf, size_t rows, const int32_t* row_word, const int32_t* row_node, int)
    -> decltype(Types::set_features(kf, rows, row_word, row_node), void()) {
  Types::set_features(kf, rows, row_word, row_node);
}
template <class Types, class K>
inline void set_features(K& kf, size_t rows, const int32_t* row_word, const int32_t* row_node, long) {
  kf.feat_vec_.clear();
  for (size_t i = 0; i < rows; ++i) if (row_word[i] >= 0) kf.feat_vec_[row_node[i]].push_back((unsigned)i);
}
// GetConnectedKeyframesByWeight(0) (COVINS) or GetConnectedNeighborKeyframes() (COVINS-G), as kf_database.cpp:50-54 chooses
template <class Types, class K>
inline auto connected_keyframes(K& kf, bool covins_g, int) -> decltype(Types::connected_keyframes(kf, covins_g)) {
  return Types::connected_keyframes(kf, covins_g);
}
template <class Types, class K>
inline auto connected_keyframes(K& kf, bool covins_g, long) -> decltype(kf.GetConnectedKeyframesByWeight(0)) {
  return covins_g ? kf.GetConnectedNeighborKeyframes() : kf.GetConnectedKeyframesByWeight(0);
}


}  // namespace detail

// `Types` must provide (see tests/cpp/standin_map.hpp and INTEGRATION.md):
//   typedefs  Map, Keyframe, Landmark, TransformType, Vector3Type
//   static bool camera(const Keyframe&, double intr[4], double dist[4], int* dist_type);   false = unknown model
//   optional: static bool camera_model(const Keyframe&, int* model, double* xi);   COVGPU_CAM_PINHOLE | COVGPU_CAM_UNIFIED and the
//             unified model's xi (intr[4] then holds fu fv cu cv); false = unknown model. Absent: every camera is pinhole.
//   static int  imu_count(const Keyframe&);
//   static void imu_sample(const Keyframe&, int i, double* dt, double acc[3], double gyr[3]);
//   static void imu_first(const Keyframe&, double acc0[3], double gyr0[3]);
//   static void imu_calib(const Keyframe&, double out5[5]);   sigma_a_c, sigma_g_c, sigma_aw_c, sigma_gw_c, g of the
//                                                             keyframe's VICalibration (keyframe_be.cpp:187-195)
template <class Types>
class OptimizationT {
 public:
  using Map = typename Types::Map;
  using Keyframe = typename Types::Keyframe;
  using Landmark = typename Types::Landmark;
  using MapPtr = std::shared_ptr<Map>;
  using KeyframePtr = std::shared_ptr<Keyframe>;
  using LandmarkPtr = std::shared_ptr<Landmark>;
  using TransformType = typename Types::TransformType;
  using Vector3Type = typename Types::Vector3Type;
  using idpair = std::pair<size_t, size_t>;
  using PoseMap = std::map<idpair, TransformType>;

  OptimizationT() = delete;  // static-only, like the reference class (optimization_be.hpp:36)

  static Params& params() { static Params p; return p; }

  // row k of the IR = kfs[k], landmark l = lms[l]; observation i of the IR (landmark-major, Flat::obs_ptr) = feature obs_feat[i] of
  // keyframe kfs[Flat::obs_kf[i]]. (No smart-pointer copies per observation: 0.87 M observations x four atomic reference-count
  // updates on the keyframes' control blocks, contended between the walking threads, were most of a 0.28 s walk.)
  struct Index {
    std::vector<KeyframePtr> kfs; std::vector<LandmarkPtr> lms; std::vector<size_t> obs_feat;
    // for Params::device_clean: per IR landmark the entries of its observation map that are NOT in the IR (invalid / null keyframes), and the
    // valid landmarks the gating left out whose observation map holds fewer than two entries (what Map::Clean erases whatever the solve does)
    std::vector<int32_t> lm_extra; std::vector<LandmarkPtr> short_lms;
  };

  // Map -> IR for one GBA round (optimization_be.cpp:74-254 round 1, :308-557 round 2)
  static void FlattenGBA(const MapPtr& map, bool visual_only, bool round2, detail::Flat& f, Index& ix) {
    const Params& prm = params();
    const bool tim = std::getenv("COVGPU_FLATTEN_TIMING") != nullptr;
    auto t_last = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
      if (!tim) return;
      const auto t = std::chrono::steady_clock::now();
      std::fprintf(stderr, "[covins_gpu] flatten %-28s %7.2f ms\n", what, std::chrono::duration<double, std::milli>(t - t_last).count());
      t_last = t;
    };
    auto keyframes = map->GetKeyframesVec();
    auto landmarks = map->GetLandmarksVec();
    lap("map vectors");
    std::unordered_map<const Keyframe*, int32_t> row;
    row.reserve(2 * keyframes.size() + 16);
    std::map<size_t, std::vector<int32_t>> cams_of_client;
    for (auto& kf : keyframes) {
      if (kf->IsInvalid()) continue;
      const int32_t k = (int32_t)ix.kfs.size();
      row[kf.get()] = k; ix.kfs.push_back(kf);
      double p7[7];
      detail::transform_to_pose(kf->GetPoseTws(), p7);  // UpdateCeresFromState (keyframe_base.cpp:486-499)
      f.pose.insert(f.pose.end(), p7, p7 + 7);
      const Vector3Type v = kf->GetStateVelocity();
      Vector3Type ba, bg;
      kf->GetStateBias(ba, bg);
      for (int i = 0; i < 3; ++i) f.sb.push_back(v[i]);
      for (int i = 0; i < 3; ++i) f.sb.push_back(ba[i]);
      for (int i = 0; i < 3; ++i) f.sb.push_back(bg[i]);
      bool fixed = (kf->id_.first == 0 && kf->id_.second == map->id_map_);                       // :88-89, 329-331
      if (round2 && kf->is_loaded_ && prm.gba_fix_poses_loaded_maps) fixed = true;                // :338-341
      f.fixed.push_back(fixed ? 1 : 0);
      // Extrinsics, intrinsics and distortion are constant parameter blocks OF THIS KEYFRAME (:336,349,352:
      // kf->ceres_extrinsics_ / camera_ of every keyframe). Identical rows are shared: normally one per agent, but a
      // keyframe whose calibration differs from its agent's earlier ones gets its own camera row.
      double intr[4], dist[4], e7[7], xi = 0.0; int dt = 0, model = COVGPU_CAM_PINHOLE;
      if (!Types::camera(*kf, intr, dist, &dt) || !detail::camera_model<Types>(*kf, &model, &xi, 0))
        detail::fatal("Unknown projection / distortion type.");  // :104-115, 187-221
      detail::transform_to_pose(kf->GetStateExtrinsics(), e7);
      std::vector<int32_t>& cands = cams_of_client[kf->id_.second];
      int32_t cam = -1;
      for (int32_t c : cands) {
        bool same = f.cam_type[c] == dt && f.cam_model[c] == model && f.cam_xi[c] == xi;
        for (int i = 0; same && i < 7; ++i) same = f.cam_extr[7 * c + i] == e7[i];
        for (int i = 0; same && i < 4; ++i) same = f.cam_intr[4 * c + i] == intr[i] && f.cam_dist[4 * c + i] == dist[i];
        if (same) { cam = c; break; }
      }
      if (cam < 0) {
        cam = (int32_t)f.cam_type.size(); cands.push_back(cam);
        f.cam_extr.insert(f.cam_extr.end(), e7, e7 + 7); f.cam_intr.insert(f.cam_intr.end(), intr, intr + 4);
        f.cam_dist.insert(f.cam_dist.end(), dist, dist + 4); f.cam_type.push_back(dt);
        f.cam_model.push_back(model); f.cam_xi.push_back(xi);
      }
      f.kf_cam.push_back(cam);
    }
    lap("keyframes");
    // IMU factors (:117-144 / :367-420)
    f.imu_ptr.assign(1, 0);
    if (!visual_only)
      for (auto& kf : ix.kfs) {
        KeyframePtr pred = kf->GetPredecessor();
        if (!pred || pred->IsInvalid()) {
          if (kf->id_.first != 0) detail::fatal("keyframe without predecessor");  // :121-124, 371-374
          continue;
        }
        const int n = Types::imu_count(*kf);
        if (round2 && n == 0) continue;  // "0 IMU measurements - skip IMU factor" (:382-385)
        f.imu_i.push_back(row.at(pred.get())); f.imu_j.push_back(row.at(kf.get()));
        double a0[3], g0[3];
        Types::imu_first(*kf, a0, g0);
        f.first.insert(f.first.end(), a0, a0 + 3); f.first.insert(f.first.end(), g0, g0 + 3);
        double nz[5];
        Types::imu_calib(*kf, nz);  // the preintegrator of THIS keyframe was built from its own calibration (keyframe_be.cpp:187-195)
        if (!(nz[0] > 0 && nz[1] > 0 && nz[2] > 0 && nz[3] > 0) || nz[4] < 9.0) detail::fatal("IMU calibration unset (sigma <= 0 or g < 9)");  // keyframe_base.cpp:51-55
        f.noise.insert(f.noise.end(), nz, nz + 5);
        for (int i = 0; i < n; ++i) {
          double dt, a[3], g[3];
          Types::imu_sample(*kf, i, &dt, a, g);
          if (dt == 0.0) continue;  // "dt: 0 -- skip measurement" (keyframe_be.cpp:199-202): the buffer may hold the initial reading
          f.samples.push_back(dt); f.samples.insert(f.samples.end(), a, a + 3); f.samples.insert(f.samples.end(), g, g + 3);
        }
        f.imu_ptr.push_back((int32_t)(f.samples.size() / 7));
      }
    // landmarks + observations (:147-236 / :425-530). The walk is O(#observations) of pointer chasing and std::map
    // copies (GetObservations), the dominant host cost of a call once the solve runs on the GPU: landmark ranges go to
    // host threads, each filling its own Flat/Index slice; the slices are concatenated in landmark order, so the IR is
    // the same for any thread count. (The map is exclusively checked out for the call, backend.cpp:134; the accessors
    // take the per-object mutexes.)
    lap("IMU factors");
    const size_t th_min_observations = 2;
    int nth = prm.flatten_threads > 0 ? prm.flatten_threads : (int)std::thread::hardware_concurrency();
    nth = std::max(1, std::min(nth, 16));
    if (landmarks.size() < 4096) nth = 1;
    struct Slice { std::vector<double> lm, uv, sigma; std::vector<int32_t> obs_kf, nobs, extra; std::vector<LandmarkPtr> lms, shorts; std::vector<size_t> feat; };
    std::vector<Slice> slices(nth);
    auto walk = [&](int t) {
      Slice sl;   // (thread-local while it grows: the vectors' end pointers of neighbouring slices[] entries share cache lines)
      const size_t l0 = landmarks.size() * (size_t)t / nth, l1 = landmarks.size() * (size_t)(t + 1) / nth;
      sl.lm.reserve(3 * (l1 - l0)); sl.lms.reserve(l1 - l0); sl.nobs.reserve(l1 - l0);
      sl.obs_kf.reserve(12 * (l1 - l0)); sl.uv.reserve(24 * (l1 - l0)); sl.sigma.reserve(12 * (l1 - l0)); sl.feat.reserve(12 * (l1 - l0));
      for (size_t li = l0; li < l1; ++li) {
        const LandmarkPtr& lm = landmarks[li];
        if (lm->IsInvalid()) continue;
        // (emitted straight into the slice and rolled back if fewer than two valid observations remain: :150-160, 428-440)
        const size_t o_mark = sl.obs_kf.size();
        int32_t n = 0, total = 0;
        detail::visit_observations<Types>(*lm, [&](const KeyframePtr& kfx, size_t feat) {
          ++total;
          if (!kfx || kfx->IsInvalid()) return;
          sl.obs_kf.push_back(row.at(kfx.get()));
          sl.uv.push_back((double)kfx->keypoints_distorted_[feat][0]);  // float -> double (utils_base.hpp:76-80)
          sl.uv.push_back((double)kfx->keypoints_distorted_[feat][1]);
          sl.sigma.push_back(((double)kfx->keypoints_aors_[feat][1] + 1) * 2.0);  // :184, 478
          sl.feat.push_back(feat);
          ++n;
        }, 0);
        if ((size_t)n < th_min_observations) {
          sl.obs_kf.resize(o_mark); sl.uv.resize(2 * o_mark); sl.sigma.resize(o_mark); sl.feat.resize(o_mark);
          if (total < 2) sl.shorts.push_back(lm);
          continue;
        }
        const Vector3Type pw = lm->GetWorldPos();
        for (int i = 0; i < 3; ++i) sl.lm.push_back(pw[i]);
        sl.lms.push_back(lm);
        sl.nobs.push_back(n);
        sl.extra.push_back(total - n);
      }
      slices[t] = std::move(sl);
    };
    auto in_threads = [&](const std::function<void(int)>& fn) {
      std::vector<std::thread> th;
      for (int t = 1; t < nth; ++t) th.emplace_back(fn, t);
      fn(0);
      for (auto& x : th) x.join();
    };
    in_threads(walk);
    lap("landmark walk (threads)");
    // slices -> IR at their offsets (prefix sums), again in the threads: 35 MB of copies
    std::vector<size_t> lm0(nth + 1, 0), ob0(nth + 1, 0);
    for (int t = 0; t < nth; ++t) { lm0[t + 1] = lm0[t] + slices[t].lms.size(); ob0[t + 1] = ob0[t] + slices[t].obs_kf.size(); }
    f.lm.resize(3 * lm0[nth]); f.obs_ptr.resize(lm0[nth] + 1); ix.lms.resize(lm0[nth]); ix.lm_extra.resize(lm0[nth]);
    for (int t = 0; t < nth; ++t) ix.short_lms.insert(ix.short_lms.end(), slices[t].shorts.begin(), slices[t].shorts.end());
    f.uv.resize(2 * ob0[nth]); f.sigma.resize(ob0[nth]); f.obs_kf.resize(ob0[nth]); ix.obs_feat.resize(ob0[nth]);
    f.obs_ptr[0] = 0;
    in_threads([&](int t) {
      Slice& sl = slices[t];
      std::copy(sl.lm.begin(), sl.lm.end(), f.lm.begin() + 3 * lm0[t]);
      std::copy(sl.uv.begin(), sl.uv.end(), f.uv.begin() + 2 * ob0[t]);
      std::copy(sl.sigma.begin(), sl.sigma.end(), f.sigma.begin() + ob0[t]);
      std::copy(sl.obs_kf.begin(), sl.obs_kf.end(), f.obs_kf.begin() + ob0[t]);
      std::copy(sl.feat.begin(), sl.feat.end(), ix.obs_feat.begin() + ob0[t]);
      std::move(sl.lms.begin(), sl.lms.end(), ix.lms.begin() + lm0[t]);
      std::copy(sl.extra.begin(), sl.extra.end(), ix.lm_extra.begin() + lm0[t]);
      int32_t at = (int32_t)ob0[t];
      for (size_t q = 0; q < sl.nobs.size(); ++q) { at += sl.nobs[q]; f.obs_ptr[lm0[t] + q + 1] = at; }
      sl = Slice();
    });
    lap("slices -> IR");
    // loop edges (:238-254 / :534-557): sqrt_info = diag(100 I3, 1e4 I3); loss only in round 2
    if (!round2 || prm.gba_use_map_loop_constraints)
      for (auto& lc : map->GetLoopConstraints()) {
        auto a = row.find(lc.kf1.get()), b = row.find(lc.kf2.get());
        if (a == row.end() || b == row.end()) { std::fprintf(stderr, "[covins_gpu] Loop KF missing -- skip loop\n"); continue; }  // :546-549
        double m7[7];
        detail::transform_to_pose(lc.T_s1_s2, m7);
        f.ei.push_back(a->second); f.ej.push_back(b->second); f.meas.insert(f.meas.end(), m7, m7 + 7);
        for (int r = 0; r < 6; ++r) for (int c = 0; c < 6; ++c) f.info.push_back(r == c ? (r < 3 ? 100.0 : 1e4) : 0.0);
        f.loss.push_back(round2 ? 1.0 : 0.0);
      }
  }

  static covgpu_options Options(int max_it, bool visual_only) {
    const Params& prm = params();
    covgpu_options o;
    covgpu_default_options(&o);
    o.strategy = prm.strategy; o.max_iterations = max_it; o.visual_only = visual_only ? 1 : 0; o.device = prm.device;
    return o;
  }

  // One context per calling thread and device, created on first use and kept (streams, pinned buffers, the device context):
  // the reference calls these functions per loop closure (placerec_be.cpp:327) and per loop candidate (OptimizeRelativePose) —
  // creating and destroying a context for every call cost more than the single-pair solve it wrapped.
  struct ContextHolder {
    covgpu_context* ctx = nullptr; int device = -1;
    ~ContextHolder() { if (ctx) covgpu_destroy(ctx); }
  };
  static ContextHolder& Holder() {
    static thread_local ContextHolder h;
    return h;
  }
  // Explicit release of the calling thread's cached context (streams, pinned buffers, the last problem's device buffers): for callers
  // that do not want to rely on the thread_local destructor at thread / process teardown, or want the HBM back between calls.
  static void Shutdown() {
    ContextHolder& h = Holder();
    if (h.ctx != nullptr) { covgpu_destroy(h.ctx); h.ctx = nullptr; h.device = -1; }
  }
  static covgpu_context* Context() {
    ContextHolder& h = Holder();
    const int dev = params().device;
    if (h.ctx != nullptr && h.device != dev) { covgpu_destroy(h.ctx); h.ctx = nullptr; }
    if (h.ctx == nullptr) {
      covgpu_options o = Options(1, false);
      if (covgpu_create(&o, &h.ctx) != COVGPU_OK) detail::fatal(covgpu_last_error());
      h.device = dev;
    }
    return h.ctx;
  }
  // wall milliseconds of the stages of the calling thread's last GlobalBundleAdjustment call (measurement hook; no effect on the call)
  static std::vector<std::pair<std::string, double>>& last_stages() {
    static thread_local std::vector<std::pair<std::string, double>> v;
    return v;
  }
  // one GBA solve (+ optionally the outlier decisions at its estimate): one GPU through the thread's context, or sharded
  static void SolveGBA(covgpu_context* ctx, covgpu_options& o, covgpu_problem& p, covgpu_result& r, std::vector<uint8_t>* erase,
                       std::vector<int32_t>* lm_left, int64_t* counts) {
    const Params& prm = params();
    if (prm.n_gpus > 1) {
      std::vector<int32_t> dev(prm.n_gpus);
      for (int i = 0; i < prm.n_gpus; ++i) dev[i] = i < (int)prm.devices.size() ? prm.devices[i] : i;
      o.shard_policy = prm.shard_policy;
      if (covgpu_gba_solve_multi(&o, &p, &r, prm.n_gpus, dev.data(), prm.th_gba_outlier_global, erase ? erase->data() : nullptr,
                                 lm_left ? lm_left->data() : nullptr, counts) != COVGPU_OK)
        detail::fatal(covgpu_last_error());
      return;
    }
    if (covgpu_gba_solve(ctx, &o, &p, &r) != COVGPU_OK) detail::fatal(covgpu_last_error());
    // problem.Evaluate + threshold (:270-289) on the device at the estimate the solve left resident: flags come back
    if (erase && covgpu_outlier_pass(ctx, prm.th_gba_outlier_global, erase->data(), lm_left->data(), counts) != COVGPU_OK) detail::fatal(covgpu_last_error());
  }

  // ---- marginal covariances from the factor of the reduced camera system (covgpu_marginal_covariance). The reference has no
  // counterpart: it obtains the 6x6 covariance of a loop edge (LoopConstraint::cov_mat, optimization_be.cpp:922-923) from repeated 17-point
  // solves (RelNonCentralPosSolver.cpp:187-292). Here: the map's own view after GBA.
  // Joint covariance of the keyframes `ids` (id, client id; any order, distinct, none with a constant pose) at the map's estimate, on the problem
  // the SECOND round of GlobalBundleAdjustment solves (loop constraints with their loss): [m][m] row-major, m = ids.size() * d in the order of
  // `ids`, d = 6 (dtheta, dp: A.1's right perturbation) or — full_state on a visual-inertial problem — 15 (then dv, db_a, db_g). mu: damping
  // of the factored system, 0 = the covariance proper. stats: covgpu_marginal_t::stats or nullptr. Throws std::invalid_argument for an id the
  // problem does not hold and std::runtime_error with the library's message for a refused or failed call.
  static std::vector<double> MarginalCovariance(const MapPtr& map, const std::vector<idpair>& ids, bool visual_only = false, bool full_state = false,
                                                double mu = 0.0, int64_t* stats = nullptr) {
    detail::Flat f; Index ix;
    FlattenGBA(map, visual_only, true, f, ix);
    std::map<idpair, int32_t> row;
    for (size_t k = 0; k < ix.kfs.size(); ++k) row[ix.kfs[k]->id_] = (int32_t)k;
    std::vector<int32_t> kf;
    for (const idpair& id : ids) {
      auto it = row.find(id);
      if (it == row.end()) throw std::invalid_argument("MarginalCovariance: keyframe not in the problem");
      kf.push_back(it->second);
    }
    const int d = (full_state && !visual_only) ? 15 : 6;
    std::vector<double> cov((size_t)(kf.size() * d) * (kf.size() * d));
    covgpu_marginal_t mg;
    mg.num_kf = (int32_t)kf.size(); mg.kf = kf.data(); mg.block = full_state ? 1 : 0; mg.mu = mu; mg.cov = cov.data(); mg.stats = stats;
    covgpu_problem p = f.view();
    covgpu_options o = Options(1, visual_only);
    if (covgpu_marginal_covariance(Context(), &o, &p, 0, &mg) != COVGPU_OK) throw std::runtime_error(covgpu_last_error());
    return cov;
  }
  // Covariance of EVERY keyframe of the map in one call, and the cross blocks of the keyframe pairs `pairs` that lie on the structure of the
  // factor (covgpu_selected_inverse): covisible pairs, IMU neighbours and loop edges always do with the pose rows, IMU
  // neighbours with the full state. Same problem, tangent, d and mu as MarginalCovariance. kf: per keyframe id its [d][d] block (a keyframe
  // with a constant pose: zeros); pair: per entry of `pairs` its [d][d] block Sigma[rows of first][columns of second], zeroed where
  // pair_ok is 0 (such a pair comes from MarginalCovariance). stats: covgpu_selinv_t::stats.
  struct KeyframeCovarianceSet {
    int d = 6;
    std::map<idpair, std::vector<double>> kf;
    std::vector<std::vector<double>> pair;
    std::vector<uint8_t> pair_ok;
    int64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  };
  static KeyframeCovarianceSet KeyframeCovariances(const MapPtr& map, bool visual_only = false, bool full_state = false, double mu = 0.0,
                                                   const std::vector<std::pair<idpair, idpair>>& pairs = {}) {
    detail::Flat f; Index ix;
    FlattenGBA(map, visual_only, true, f, ix);
    std::map<idpair, int32_t> row;
    for (size_t k = 0; k < ix.kfs.size(); ++k) row[ix.kfs[k]->id_] = (int32_t)k;
    std::vector<int32_t> pi, pj;
    for (const auto& pr : pairs) {
      auto a = row.find(pr.first), b = row.find(pr.second);
      if (a == row.end() || b == row.end()) throw std::invalid_argument("KeyframeCovariances: keyframe not in the problem");
      pi.push_back(a->second); pj.push_back(b->second);
    }
    KeyframeCovarianceSet out;
    out.d = (full_state && !visual_only) ? 15 : 6;
    const size_t dd = (size_t)out.d * out.d, K = ix.kfs.size();
    std::vector<double> kc(K * dd), pc(pairs.size() * dd);
    out.pair_ok.assign(pairs.size(), 0);
    covgpu_selinv_t s;
    s.block = full_state ? 1 : 0; s.mu = mu; s.kf_cov = kc.data(); s.num_pairs = (int64_t)pairs.size();
    s.pair_i = pi.data(); s.pair_j = pj.data(); s.pair_cov = pc.data(); s.pair_ok = out.pair_ok.data(); s.stats = out.stats;
    covgpu_problem p = f.view();
    covgpu_options o = Options(1, visual_only);
    if (covgpu_selected_inverse(Context(), &o, &p, 0, &s) != COVGPU_OK) throw std::runtime_error(covgpu_last_error());
    for (size_t k = 0; k < K; ++k) out.kf[ix.kfs[k]->id_] = std::vector<double>(kc.begin() + k * dd, kc.begin() + (k + 1) * dd);
    for (size_t q = 0; q < pairs.size(); ++q) out.pair.emplace_back(pc.begin() + q * dd, pc.begin() + (q + 1) * dd);
    return out;
  }
  // Covariance of EVERY landmark of the map's problem in one call (covgpu_landmark_covariance): per landmark id its 3x3 block
  // of the inverse of the whole system at damping mu, world frame. Same problem and mu as KeyframeCovariances. A landmark whose H_ll is not
  // positive definite (lm_ok = 0) is left out of the map. Matrix3Type: any default-constructible 3x3 type written through operator()(r, c) —
  // Eigen::Matrix3d in COVINS (this header stays Eigen-free, see the top). stats (optional): covgpu_lmcov_t::stats.
  template <class Matrix3Type>
  static std::map<idpair, Matrix3Type> LandmarkCovariances(const MapPtr& map, bool visual_only = false, double mu = 0.0, int64_t* stats = nullptr) {
    detail::Flat f; Index ix;
    FlattenGBA(map, visual_only, true, f, ix);
    const size_t L = ix.lms.size();
    std::vector<double> lc(9 * L + 9);
    std::vector<uint8_t> ok(L + 1, 0);
    covgpu_lmcov_t s;
    s.mu = mu; s.lm_cov = lc.data(); s.lm_ok = ok.data(); s.kf_cov = nullptr; s.stats = stats;
    covgpu_problem p = f.view();
    covgpu_options o = Options(1, visual_only);
    if (covgpu_landmark_covariance(Context(), &o, &p, &s) != COVGPU_OK) throw std::runtime_error(covgpu_last_error());
    std::map<idpair, Matrix3Type> out;
    for (size_t l = 0; l < L; ++l) {
      if (!ok[l]) continue;
      Matrix3Type m;
      for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) m(r, c) = lc[9 * l + 3 * r + c];
      out[ix.lms[l]->id_] = m;
    }
    return out;
  }
  // Covariance of EVERY observation of the map's problem in one call (covgpu_observation_covariance), in the landmark-major
  // observation order of the problem: the 2x2 block C_o = J_o Sigma J_o^T of the hat matrix (row-major; the normalised residual of the
  // observation is r^T (I - C_o)^-1 r) and the 6x3 block Sigma_al, pose rows of the observer (dtheta, dp) by the landmark's world
  // coordinates. Same problem and mu as LandmarkCovariances; with a robust loss the blocks are in loss-corrected units. ok = 0: the
  // landmark is not served (LandmarkCovariances leaves it out), the blocks are zeros. stats (optional): covgpu_obscov_t::stats.
  struct ObservationCovariance {
    idpair lm, kf;
    double cov[4] = {0, 0, 0, 0};
    double cross[18] = {};
    uint8_t ok = 0;
  };
  static std::vector<ObservationCovariance> ObservationCovariances(const MapPtr& map, bool visual_only = false, double mu = 0.0, int64_t* stats = nullptr) {
    detail::Flat f; Index ix;
    FlattenGBA(map, visual_only, true, f, ix);
    const size_t L = ix.lms.size(), O = f.obs_kf.size();
    std::vector<double> oc(4 * O + 4), cc(18 * O + 18);
    std::vector<uint8_t> ok(O + 1, 0);
    covgpu_obscov_t s;
    s.mu = mu; s.obs_cov = oc.data(); s.cross_cov = cc.data(); s.obs_res = nullptr; s.obs_ok = ok.data();
    s.lm_cov = nullptr; s.lm_ok = nullptr; s.kf_cov = nullptr; s.stats = stats;
    covgpu_problem p = f.view();
    covgpu_options o = Options(1, visual_only);
    if (covgpu_observation_covariance(Context(), &o, &p, &s) != COVGPU_OK) throw std::runtime_error(covgpu_last_error());
    std::vector<ObservationCovariance> out(O);
    for (size_t l = 0; l < L; ++l)
      for (size_t i = (size_t)f.obs_ptr[l]; i < (size_t)f.obs_ptr[l + 1]; ++i) {
        ObservationCovariance& r = out[i];
        r.lm = ix.lms[l]->id_; r.kf = ix.kfs[f.obs_kf[i]]->id_; r.ok = ok[i];
        for (int k = 0; k < 4; ++k) r.cov[k] = oc[4 * i + k];
        for (int k = 0; k < 18; ++k) r.cross[k] = cc[18 * i + k];
      }
    return out;
  }
  // Covariance of the relative pose T_s1_s2 of two keyframes from their joint pose covariance cov12 ([12][12]: MarginalCovariance(map, {id1,
  // id2})): J cov12 J^T with J the 6x12 Jacobian of the between residual (R7) at zero residual and unit weight — [6][6] row-major, rotation
  // first and translation second, the order of LoopConstraint::cov_mat.
  static std::array<double, 36> RelativePoseCovariance(const std::vector<double>& cov12, const TransformType& Tws1, const TransformType& Tws2) {
    if (cov12.size() != 144) throw std::invalid_argument("RelativePoseCovariance: cov12 must be 12x12");
    double R1[9], R2[9], t[3], J[72] = {0};
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) { R1[3 * r + c] = Tws1(r, c); R2[3 * r + c] = Tws2(r, c); }
    for (int r = 0; r < 3; ++r) { t[r] = 0; for (int c = 0; c < 3; ++c) t[r] += R1[3 * c + r] * (Tws2(c, 3) - Tws1(c, 3)); }   // R1^T (p2 - p1)
    const double sk[9] = {0, -t[2], t[1], t[2], 0, -t[0], -t[1], t[0], 0};
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) {
        double a = 0;
        for (int k = 0; k < 3; ++k) a += R2[3 * k + r] * R1[3 * k + c];   // R2^T R1
        J[12 * r + c] = -a; J[12 * r + 6 + c] = r == c ? 1.0 : 0.0;
        J[12 * (3 + r) + c] = sk[3 * r + c]; J[12 * (3 + r) + 3 + c] = -R1[3 * c + r]; J[12 * (3 + r) + 9 + c] = R1[3 * c + r];
      }
    double JS[72];
    for (int r = 0; r < 6; ++r) for (int c = 0; c < 12; ++c) { double a = 0; for (int k = 0; k < 12; ++k) a += J[12 * r + k] * cov12[12 * k + c]; JS[12 * r + c] = a; }
    std::array<double, 36> out;
    for (int r = 0; r < 6; ++r)
      for (int c = 0; c <= r; ++c) { double a = 0; for (int k = 0; k < 12; ++k) a += JS[12 * r + k] * J[12 * c + k]; out[6 * r + c] = out[6 * c + r] = a; }
    return out;
  }

  // ---- optimization_be.cpp:56-618
  static auto GlobalBundleAdjustment(MapPtr map, int interations_limit, double time_limit, bool visual_only = false,
                                     bool outlier_removal = true, bool estimate_bias = false) -> void {
    (void)time_limit; (void)estimate_bias;  // never read by the reference either
    std::printf("+++ GBA: Start +++\n");
    const bool tim = std::getenv("COVGPU_FLATTEN_TIMING") != nullptr;   // per-stage wall times of the call on stderr
    auto t_last = std::chrono::steady_clock::now();
    last_stages().clear();
    auto lap = [&](const char* what) {   // (two clock reads per stage: kept for last_stages(), printed on request)
      const auto t = std::chrono::steady_clock::now();
      const double ms = std::chrono::duration<double, std::milli>(t - t_last).count();
      last_stages().emplace_back(what, ms);
      if (tim) std::fprintf(stderr, "[covins_gpu] GBA call %-34s %7.2f ms\n", what, ms);
      t_last = t;
    };
    covgpu_context* ctx = params().n_gpus > 1 ? nullptr : Context();   // (the sharded solve creates its own contexts, one per device)
    lap("context");
    if (outlier_removal && params().device_second_round) {
      // Both rounds behind one call. The first round's problem is walked once (:80-254); the outlier round, the erase decisions
      // (:270-290) and the rebuilt second-round problem (:296-557) stay on the device; the map is brought to the state the reference
      // leaves: observations erased (:281-289), the second round's estimate written back (:572-609), Map::Clean (:614).
      const Params& prm = params();
      detail::Flat f; Index ix;
      FlattenGBA(map, visual_only, false, f, ix);
      lap("Map -> IR (once)");
      std::vector<uint8_t> fixed2;
      if (prm.gba_fix_poses_loaded_maps) {   // :338-341
        fixed2.assign(f.fixed.begin(), f.fixed.end());
        for (size_t k = 0; k < ix.kfs.size(); ++k) if (ix.kfs[k]->is_loaded_) fixed2[k] = 1;
      }
      covgpu_two_round tr;
      tr.outlier_threshold = prm.th_gba_outlier_global; tr.round1_iterations = 5; tr.use_loops_round2 = prm.gba_use_map_loop_constraints ? 1 : 0;
      tr.loop_loss_round2 = 1.0; tr.kf_fixed_round2 = fixed2.empty() ? nullptr : fixed2.data();
      covgpu_problem p = f.view();
      covgpu_options o = Options(interations_limit, visual_only);
      covgpu_result r1, r2;
      std::vector<uint8_t> erase(f.obs_kf.size() + 1);
      std::vector<int32_t> lm_left(ix.lms.size() + 1);
      int64_t counts[2] = {0, 0};
      if (prm.n_gpus > 1) {   // (round 6) the sharded route: one upload per rank, the second round derived on every rank's device from its share
        std::vector<int32_t> dev(prm.n_gpus);
        for (int i = 0; i < prm.n_gpus; ++i) dev[i] = i < (int)prm.devices.size() ? prm.devices[i] : i;
        o.shard_policy = prm.shard_policy;
        if (covgpu_gba_two_round_multi(&o, &p, &tr, prm.n_gpus, dev.data(), erase.data(), lm_left.data(), counts, &r1, &r2) != COVGPU_OK) detail::fatal(covgpu_last_error());
      } else if (covgpu_gba_two_round(ctx, &o, &p, &tr, erase.data(), lm_left.data(), counts, &r1, &r2) != COVGPU_OK) detail::fatal(covgpu_last_error());
      lap("upload + both rounds on the device");
      size_t num_bad = 0, lms2 = 0;
      for (size_t l = 0; l < ix.lms.size(); ++l) {
        for (int32_t i = f.obs_ptr[l]; i < f.obs_ptr[l + 1]; ++i)
          if (erase[i]) {  // :281-289
            const KeyframePtr& kf = ix.kfs[f.obs_kf[i]];
            kf->EraseLandmark(ix.obs_feat[i]);
            ix.lms[l]->EraseObservation(kf);
            ++num_bad;
          }
        lms2 += lm_left[l] >= 2 ? 1 : 0;
      }
      std::printf("--> GBA removed %zu of %zu observations\n", num_bad, f.obs_kf.size() * 2);
      std::printf("--> KFs: %zu\n--> LMs: %zu\n", ix.kfs.size(), lms2);
      lap("erase observations");
      if (r2.termination == 4) std::fprintf(stderr, "[covins_gpu] GBA: linear solve failed, keeping the last accepted estimate (as ceres::Solve would)\n");
      if (r2.reserved > 0) std::fprintf(stderr, "[covins_gpu] GBA: %d IMU factors without a positive definite covariance carry no weight\n", r2.reserved);
      for (size_t k = 0; k < ix.kfs.size(); ++k) {  // :572-595
        KeyframePtr& kf = ix.kfs[k];
        TransformType T;
        detail::pose_to_transform(&f.pose[7 * k], T);
        kf->SetPoseTws(T);
        kf->SetPoseOptimized();
        if (!visual_only) {
          const double* s = &f.sb[9 * k];
          Vector3Type vel, bA, bG;
          for (int i = 0; i < 3; ++i) { vel[i] = s[i]; bA[i] = s[3 + i]; bG[i] = s[6 + i]; }
          kf->SetStateBias(bA, bG);
          kf->SetStateVelocity(vel);
          kf->SetVelBiasOptimized();
        }
        kf->is_gba_optimized_ = true;
      }
      for (size_t l = 0; l < ix.lms.size(); ++l) {  // :598-609 — the landmarks of the SECOND round (:428-440: two observations left)
        if (lm_left[l] < 2) continue;
        Vector3Type pw;
        for (int i = 0; i < 3; ++i) pw[i] = f.lm[3 * l + i];
        ix.lms[l]->SetWorldPos(pw);
        ix.lms[l]->SetOptimized();
        ix.lms[l]->is_gba_optimized_ = true;
      }
      lap("write-back");
      std::printf("--> Clean Map\n");
      if (prm.device_clean) {
        // Map::Clean's map check (map_be.cpp:698-717) from the counts at hand: entries left = kept by the device + entries outside the IR
        size_t removed = 0;
        for (size_t l = 0; l < ix.lms.size(); ++l) if (lm_left[l] + ix.lm_extra[l] < 2) { map->EraseLandmark(ix.lms[l]); ++removed; }
        for (auto& lm : ix.short_lms) { map->EraseLandmark(lm); ++removed; }
        std::printf("----> Done: Removed %zu Landmarks (counts of the call; Params::device_clean)\n", removed);
        lap("Map::Clean (from the call's counts)");
      } else {
        map->Clean();  // :614
        lap("Map::Clean");
      }
      std::printf("--> done.\n+++ GBA: End +++\n");
      return;
    }
    if (outlier_removal) {  // first round (:62-293)
      detail::Flat f; Index ix;
      FlattenGBA(map, visual_only, false, f, ix);
      lap("round 1: Map -> IR");
      covgpu_problem p = f.view();
      covgpu_options o = Options(5, visual_only);  // max_num_iterations = 5 (:262)
      covgpu_result r;
      std::vector<uint8_t> erase(f.obs_kf.size() + 1);
      std::vector<int32_t> lm_left(ix.lms.size() + 1);
      int64_t counts[2] = {0, 0};
      SolveGBA(ctx, o, p, r, &erase, &lm_left, counts);
      lap("round 1: upload + solve + outlier pass");
      size_t num_bad = 0;
      for (size_t l = 0; l < ix.lms.size(); ++l)
        for (int32_t i = f.obs_ptr[l]; i < f.obs_ptr[l + 1]; ++i)
          if (erase[i]) {  // :281-289
            const KeyframePtr& kf = ix.kfs[f.obs_kf[i]];
            kf->EraseLandmark(ix.obs_feat[i]);
            ix.lms[l]->EraseObservation(kf);
            ++num_bad;
          }
      std::printf("--> GBA removed %zu of %zu observations\n", num_bad, f.obs_kf.size() * 2);
      lap("round 1: erase observations");
    }
    lap("round 1: release IR");
    {  // second round (:296-610)
      detail::Flat f; Index ix;
      FlattenGBA(map, visual_only, true, f, ix);
      lap("round 2: Map -> IR");
      std::printf("--> KFs: %zu\n--> LMs: %zu\n", ix.kfs.size(), ix.lms.size());
      covgpu_problem p = f.view();
      covgpu_options o = Options(interations_limit, visual_only);
      covgpu_result r;
      SolveGBA(ctx, o, p, r, nullptr, nullptr, nullptr);
      lap("round 2: upload + solve");
      if (r.termination == 4) std::fprintf(stderr, "[covins_gpu] GBA: linear solve failed, keeping the last accepted estimate (as ceres::Solve would)\n");
      if (r.reserved > 0) std::fprintf(stderr, "[covins_gpu] GBA: %d IMU factors without a positive definite covariance carry no weight\n", r.reserved);
      for (size_t k = 0; k < ix.kfs.size(); ++k) {  // :572-595
        KeyframePtr& kf = ix.kfs[k];
        TransformType T;
        detail::pose_to_transform(&f.pose[7 * k], T);
        kf->SetPoseTws(T);
        kf->SetPoseOptimized();
        if (!visual_only) {
          const double* s = &f.sb[9 * k];
          Vector3Type vel, bA, bG;
          for (int i = 0; i < 3; ++i) { vel[i] = s[i]; bA[i] = s[3 + i]; bG[i] = s[6 + i]; }
          kf->SetStateBias(bA, bG);
          kf->SetStateVelocity(vel);
          kf->SetVelBiasOptimized();
        }
        kf->is_gba_optimized_ = true;
      }
      for (size_t l = 0; l < ix.lms.size(); ++l) {  // :598-609
        Vector3Type pw;
        for (int i = 0; i < 3; ++i) pw[i] = f.lm[3 * l + i];
        ix.lms[l]->SetWorldPos(pw);
        ix.lms[l]->SetOptimized();
        ix.lms[l]->is_gba_optimized_ = true;
      }
      lap("round 2: write-back");
    }
    lap("round 2: release IR");
    std::printf("--> Clean Map\n");
    map->Clean();  // :614
    lap("Map::Clean");
    std::printf("--> done.\n+++ GBA: End +++\n");
  }

  // ---- optimization_be.cpp:833-1086
  static auto PoseGraphOptimization(MapPtr map, PoseMap corrected_poses) -> void {
    const Params& prm = params();
    const bool tim = std::getenv("COVGPU_FLATTEN_TIMING") != nullptr;
    auto t_last = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
      if (!tim) return;
      const auto t = std::chrono::steady_clock::now();
      std::fprintf(stderr, "[covins_gpu] flatten %-28s %7.2f ms\n", what, std::chrono::duration<double, std::milli>(t - t_last).count());
      t_last = t;
    };
    auto keyframes = map->GetKeyframesVec();
    auto landmarks = map->GetLandmarksVec();
    detail::Flat f;
    std::vector<KeyframePtr> kfs;
    std::map<Keyframe*, int32_t> row;
    for (auto& kf : keyframes) {  // :850-882
      if (kf->IsInvalid()) continue;
      row[kf.get()] = (int32_t)kfs.size(); kfs.push_back(kf);
      double p7[7];
      auto mit = corrected_poses.find(kf->id_);
      if (mit != corrected_poses.end()) detail::transform_to_pose(mit->second, p7);
      else detail::transform_to_pose(kf->GetPoseTws(), p7);
      f.pose.insert(f.pose.end(), p7, p7 + 7);
      for (int i = 0; i < 9; ++i) f.sb.push_back(0.0);
      bool fixed = (kf->id_.first == 0 && kf->id_.second == map->id_map_);
      if (kf->is_gba_optimized_ && prm.pgo_fix_kfs_after_gba) fixed = true;
      else if (kf->is_loaded_ && prm.pgo_fix_poses_loaded_maps) fixed = true;
      f.fixed.push_back(fixed ? 1 : 0);
      f.kf_cam.push_back(0);
    }
    f.cam_type.push_back(0);
    f.cam_extr.assign(7, 0.0); f.cam_extr[3] = 1.0; f.cam_intr.assign(4, 1.0); f.cam_dist.assign(4, 0.0);
    double W1[36] = {}, W23[36] = {}, W45[36] = {};  // :889-902
    for (int i = 0; i < 6; ++i) {
      W1[7 * i] = (i < 3 ? prm.wt_kf_r : prm.wt_kf_t) * prm.wt_kf_n1;
      W23[7 * i] = W1[7 * i] / prm.wt_kf_n23; W45[7 * i] = W1[7 * i] / prm.wt_kf_n45;
    }
    auto add_edge = [&](int32_t a, int32_t b, const double* m7, const double* S, double loss) {
      f.ei.push_back(a); f.ej.push_back(b); f.meas.insert(f.meas.end(), m7, m7 + 7); f.info.insert(f.info.end(), S, S + 36); f.loss.push_back(loss);
    };
    for (auto& lc : map->GetLoopConstraints()) {  // :912-944
      double S[36], m7[7];
      if (prm.placerec_type == "COVINS") for (int i = 0; i < 36; ++i) S[i] = W1[i];
      else {
        double cov[36];
        for (int r = 0; r < 6; ++r) for (int c = 0; c < 6; ++c) cov[6 * r + c] = lc.cov_mat(r, c);
        detail::sqrt_info_from_cov(cov, S);
      }
      detail::transform_to_pose(lc.T_s1_s2, m7);
      auto a = row.find(lc.kf1.get()), b = row.find(lc.kf2.get());  // an invalidated loop keyframe must not take the server down
      if (a == row.end() || b == row.end()) { std::fprintf(stderr, "[covins_gpu] PGO: loop KF missing -- skip loop\n"); continue; }
      add_edge(a->second, b->second, m7, S, prm.use_robust_loss ? prm.robust_loss_th : 0.0);
    }
    std::set<std::pair<Keyframe*, Keyframe*>> inserted;
    for (auto& kf : kfs) {  // successor edges from the VIO poses (:947-972)
      KeyframePtr succ = kf->GetSuccessor();
      if (!succ) continue;
      auto sr = row.find(succ.get());
      if (sr == row.end()) continue;  // successor invalid / not in the map: no parameter block to tie to
      if (!inserted.insert({kf.get(), succ.get()}).second) continue;
      double m7[7];
      detail::relative_pose(kf->GetPoseTws_vio(), succ->GetPoseTws_vio(), m7);
      add_edge(row.at(kf.get()), sr->second, m7, W1, 0.0);
    }
    if (prm.use_nbr_kfs)  // five previous neighbours (:976-1021)
      for (auto& kf : kfs) {
        std::vector<KeyframePtr> connections;
        KeyframePtr temp = kf;
        for (int j = 1; j < 6; ++j)
          if (int(kf->id_.first) - j > 0) {
            temp = temp ? temp->GetPredecessor() : KeyframePtr();  // a chain shorter than id_.first suggests (culled keyframes) ends here
            if (!temp) break;
            connections.push_back(temp);
          }
        size_t k = 0;
        for (auto& kfc : connections) {
          k++;
          const double* S = (k <= 1) ? W1 : (k <= 3 ? W23 : W45);
          auto cr = row.find(kfc.get());
          if (cr == row.end()) continue;
          if (!inserted.insert({kf.get(), kfc.get()}).second) continue;
          double m7[7];
          detail::relative_pose(kf->GetPoseTws_vio(), kfc->GetPoseTws_vio(), m7);
          add_edge(row.at(kf.get()), cr->second, m7, S, 0.0);
        }
      }
    covgpu_problem p = f.view();
    covgpu_options o = Options(prm.pgo_iteration_limit, false);
    covgpu_context* ctx = Context();
    covgpu_result r;
    if (covgpu_pgo_solve(ctx, &o, &p, &r) != COVGPU_OK) detail::fatal(covgpu_last_error());
    // recover (:1033-1083): poses, velocity rotation, landmark re-anchoring on the device
    std::vector<double> pose_old(7 * kfs.size()), vel(3 * kfs.size());
    for (size_t k = 0; k < kfs.size(); ++k) {
      detail::transform_to_pose(kfs[k]->GetPoseTws(), &pose_old[7 * k]);
      const Vector3Type v = kfs[k]->GetStateVelocity();
      for (int i = 0; i < 3; ++i) vel[3 * k + i] = v[i];
    }
    std::vector<LandmarkPtr> lms;
    std::vector<int32_t> ref;
    std::vector<double> lmp;
    for (auto& lm : landmarks) {
      if (lm->IsInvalid()) continue;
      KeyframePtr kf_ref = lm->GetReferenceKeyframe();
      if (!kf_ref) { if (!lm->GetObservations().empty()) map->EraseLandmark(lm); continue; }  // :1059-1065
      auto it = row.find(kf_ref.get());
      if (it == row.end()) { map->EraseLandmark(lm); continue; }                              // :1069-1073
      const Vector3Type pw = lm->GetWorldPos();
      lms.push_back(lm); ref.push_back(it->second);
      for (int i = 0; i < 3; ++i) lmp.push_back(pw[i]);
    }
    if (covgpu_pgo_reanchor(ctx, (int32_t)kfs.size(), pose_old.data(), f.pose.data(), vel.data(), (int32_t)lms.size(), ref.data(),
                            lmp.data()) != COVGPU_OK)
      detail::fatal(covgpu_last_error());
    for (size_t k = 0; k < kfs.size(); ++k) {
      TransformType T;
      detail::pose_to_transform(&f.pose[7 * k], T);
      kfs[k]->SetPoseTws(T);  // UpdateFromCeres (:1045)
      Vector3Type v;
      for (int i = 0; i < 3; ++i) v[i] = vel[3 * k + i];
      kfs[k]->SetStateVelocity(v);
      kfs[k]->SetPoseOptimized();
    }
    for (size_t l = 0; l < lms.size(); ++l) {
      Vector3Type pw;
      for (int i = 0; i < 3; ++i) pw[i] = lmp[3 * l + i];
      lms[l]->SetWorldPos(pw);
      lms[l]->SetOptimized();
    }
    std::printf("--> PGO END \n");
  }

  // ---- optimization_be.cpp:620-831, batched: one entry per loop candidate (placerec_be.cpp:116-165 verifies them one by
  //      one; a batch goes to the device in ONE launch, covgpu_relpose_batch). Semantics per entry are the reference's:
  //      matches1[i] is reset for removed correspondences, T12 is updated unless fewer than 12 inliers are left, the
  //      return value is the inlier count (0 = rejected).
  using LandmarkVector = std::vector<LandmarkPtr>;
  struct RelPoseJob { KeyframePtr kf1, kf2; LandmarkVector* matches1; TransformType* T12; int result = 0; };
  static void OptimizeRelativePoseBatch(std::vector<RelPoseJob>& jobs) {
    const size_t B = jobs.size();
    if (B == 0) return;
    std::vector<int32_t> ptr(1, 0), dA(B), dB(B), inl(B), mA(B), mB(B);
    std::vector<double> pB, pA, kA, kB, sA, sB, camA(8 * B), camB(8 * B), T(7 * B), xA(B), xB(B);
    bool uni = false;
    std::vector<std::vector<int>> index(B);   // correspondence -> position in matches1
    for (size_t b = 0; b < B; ++b) {
      RelPoseJob& j = jobs[b];
      int da = 0, db = 0;
      if (!Types::camera(*j.kf1, &camA[8 * b], &camA[8 * b + 4], &da) || !Types::camera(*j.kf2, &camB[8 * b], &camB[8 * b + 4], &db) ||
          !detail::camera_model<Types>(*j.kf1, &mA[b], &xA[b], 0) || !detail::camera_model<Types>(*j.kf2, &mB[b], &xB[b], 0))
        detail::fatal("Unknown projection / distortion type.");  // :668-671, 676-752
      dA[b] = da; dB[b] = db;
      uni = uni || mA[b] == COVGPU_CAM_UNIFIED || mB[b] == COVGPU_CAM_UNIFIED;
      detail::transform_to_pose(*j.T12, &T[7 * b]);
      // TcwA = (Tws1 Tsc1)^-1, TcwB = (Tws2 Tsc1)^-1 — the reference uses kf1's extrinsics for both (:640-641)
      TransformType TwcA, TwcB;
      detail::mat_mul(j.kf1->GetPoseTws(), j.kf1->GetStateExtrinsics(), TwcA);
      detail::mat_mul(j.kf2->GetPoseTws(), j.kf1->GetStateExtrinsics(), TwcB);
      const auto lmsA = j.kf1->GetLandmarks();
      const int N = (int)j.matches1->size();
      for (int i = 0; i < N; ++i) {
        const LandmarkPtr& mb = (*j.matches1)[i];
        if (!mb) continue;
        const LandmarkPtr ma = i < (int)lmsA.size() ? lmsA[i] : LandmarkPtr();
        const int iB = mb->GetFeatureIndex(j.kf2);
        if (!ma || ma->IsInvalid() || mb->IsInvalid() || iB < 0) continue;        // :648-651
        double a3[3], b3[3];
        detail::to_camera(TwcA, ma->GetWorldPos(), a3); detail::to_camera(TwcB, mb->GetWorldPos(), b3);   // :652-656
        pA.insert(pA.end(), a3, a3 + 3); pB.insert(pB.end(), b3, b3 + 3);
        kA.push_back((double)j.kf1->keypoints_distorted_[i][0]); kA.push_back((double)j.kf1->keypoints_distorted_[i][1]);
        kB.push_back((double)j.kf2->keypoints_distorted_[iB][0]); kB.push_back((double)j.kf2->keypoints_distorted_[iB][1]);
        sA.push_back(((double)j.kf1->keypoints_aors_[i][1] + 1) * 2.0); sB.push_back(((double)j.kf2->keypoints_aors_[iB][1] + 1) * 2.0);   // :658, 717
        index[b].push_back(i);
      }
      ptr.push_back((int32_t)sA.size());
    }
    std::vector<uint8_t> out(sA.size() + 1);
    covgpu_relpose_batch_t bt{};
    bt.num_pairs = (int32_t)B; bt.corr_ptr = ptr.data(); bt.p_b = pB.data(); bt.p_a = pA.data(); bt.kp_a = kA.data(); bt.kp_b = kB.data();
    bt.sigma_a = sA.data(); bt.sigma_b = sB.data(); bt.cam_a = camA.data(); bt.cam_b = camB.data(); bt.dist_type_a = dA.data(); bt.dist_type_b = dB.data();
    bt.T_ab = T.data(); bt.outlier = out.data(); bt.inliers = inl.data();
    if (uni) { bt.cam_model_a = mA.data(); bt.cam_model_b = mB.data(); bt.xi_a = xA.data(); bt.xi_b = xB.data(); }
    covgpu_context* ctx = Context();
    if (covgpu_relpose_batch(ctx, &bt, params().th_outlier_align, 12) != COVGPU_OK) detail::fatal(covgpu_last_error());
    for (size_t b = 0; b < B; ++b) {
      RelPoseJob& j = jobs[b];
      for (size_t c = 0; c < index[b].size(); ++c)
        if (out[ptr[b] + c]) (*j.matches1)[index[b][c]].reset();   // "matches1[i] = NULL" (:807; the reference indexes by residual, a quirk not copied)
      j.result = inl[b];
      if (inl[b] > 0) detail::pose_to_transform(&T[7 * b], *j.T12);  // :820
    }
  }
  // same signature as the reference (th2 is unused there too)
  static auto OptimizeRelativePose(KeyframePtr kf1, KeyframePtr kf2, LandmarkVector& matches1, TransformType& T12, const double th2) -> int {
    (void)th2;
    std::vector<RelPoseJob> jobs(1);
    jobs[0].kf1 = kf1; jobs[0].kf2 = kf2; jobs[0].matches1 = &matches1; jobs[0].T12 = &T12;
    OptimizeRelativePoseBatch(jobs);
    return jobs[0].result;
  }
};

// ---- Se3Solver (Se3Solver.h / Se3Solver.cpp:59-110): the 3D-2D RANSAC of a loop candidate, batched (covgpu_abspose_ransac_batch,
//      DESIGN.md §4.10). Drop-in for covins::Se3Solver: same constructor, setRansacParams and projectiveAlignment; Tws is the query
//      camera in the world (opengv's transformation_t, what placerec_be.cpp:132 uses as Twc1). ProjectiveAlignmentBatch verifies many
//      candidates with ONE library call per distinct threshold (placerec_be.cpp:116-139 runs them one by one).
template <class Types>
class Se3SolverT {
 public:
  using Keyframe = typename Types::Keyframe;
  using Landmark = typename Types::Landmark;
  using KeyframePtr = std::shared_ptr<Keyframe>;
  using LandmarkPtr = std::shared_ptr<Landmark>;
  using LandmarkVector = std::vector<LandmarkPtr>;
  using TransformType = typename Types::TransformType;

  // the reference's defaults (Se3Solver.h); callers pass covins_params::placerec::ransac::* (Params::ransac_*)
  Se3SolverT(const size_t minInliers = 30, const double ransacProb = 0.999, const size_t maxIter = 300)
      : mMinInliers(minInliers), mRansacProb(ransacProb), mMaxIter(maxIter) {}
  void setRansacParams(const int minInliers, const double ransacProb, const int maxIter) {
    mMinInliers = (size_t)minInliers; mRansacProb = ransacProb; mMaxIter = (size_t)maxIter;
  }

  // one loop candidate: matches[i] = the landmark matched to feature i of kf (NULL: none). kf_candidate only seeds the draws.
  struct AbsPoseJob {
    KeyframePtr kf, kf_candidate;
    LandmarkVector* matches = nullptr;
    double threshold = 25.0;
    TransformType* Tws = nullptr;
    bool found = false;   // out: projectiveAlignment's return value
    int inliers = 0;      // out
  };

  void ProjectiveAlignmentBatch(std::vector<AbsPoseJob>& jobs) const {
    std::vector<double> ths;
    for (const AbsPoseJob& j : jobs) if (std::find(ths.begin(), ths.end(), j.threshold) == ths.end()) ths.push_back(j.threshold);
    for (double th : ths) run(jobs, th);
  }

  bool projectiveAlignment(const KeyframePtr keyframePtr, LandmarkVector& mapPointMatches, const double threshold, TransformType& Tws) const {
    std::vector<AbsPoseJob> jobs(1);
    jobs[0].kf = keyframePtr; jobs[0].matches = &mapPointMatches; jobs[0].threshold = threshold; jobs[0].Tws = &Tws;
    ProjectiveAlignmentBatch(jobs);
    return jobs[0].found;
  }

 private:
  size_t mMinInliers;
  double mRansacProb;   // stored, not used: see Params::ransac_probability
  size_t mMaxIter;

  void run(std::vector<AbsPoseJob>& jobs, double th) const {
    std::vector<size_t> sel;
    for (size_t b = 0; b < jobs.size(); ++b) if (jobs[b].threshold == th) sel.push_back(b);
    const size_t B = sel.size();
    std::vector<int32_t> ptr(1, 0);
    std::vector<double> f, P, sg, T(7 * B, 0.0);
    std::vector<uint64_t> seed(B);
    std::vector<std::vector<size_t>> indMap(B);
    for (size_t s = 0; s < B; ++s) {
      AbsPoseJob& j = jobs[sel[s]];
      const LandmarkVector& m = *j.matches;
      for (size_t i = 0; i < m.size(); ++i) if (m[i] && !m[i]->IsInvalid()) indMap[s].push_back(i);   // Se3Solver.cpp:66-75
      double intr[4], dist[4]; int dt = 0;
      if (!Types::camera(*j.kf, intr, dist, &dt)) detail::fatal("Unknown projection / distortion type.");
      const double fu = (intr[0] + intr[1]) / 2.0;
      // FrameNoncentralAbsoluteAdapter: i < min(bearings_.size(), matches.size()), null / invalid matches skipped
      for (size_t i = 0; i < m.size(); ++i) {
        double b3[3];
        if (!detail::bearing<Types>(*j.kf, i, b3, 0)) break;
        if (!m[i] || m[i]->IsInvalid()) continue;
        const auto pw = m[i]->GetWorldPos();
        const double sd = 0.8 * ((double)j.kf->keypoints_aors_[i][1] + 1);
        f.insert(f.end(), b3, b3 + 3);
        for (int k = 0; k < 3; ++k) P.push_back(pw[k]);
        sg.push_back(std::sqrt(2) * sd * sd / (fu * fu));
      }
      ptr.push_back((int32_t)sg.size());
      seed[s] = detail::abspose_seed(j.kf.get(), j.kf_candidate.get());
    }
    std::vector<uint8_t> mask(sg.size() + 1);
    std::vector<int32_t> inl(B);
    covgpu_abspose_batch_t bt{};
    bt.num = (int32_t)B; bt.corr_ptr = ptr.data(); bt.bearing = f.data(); bt.point_w = P.data(); bt.sigma_angle = sg.data(); bt.seed = seed.data();
    bt.T_wc = T.data(); bt.inlier = mask.data(); bt.inliers = inl.data();
    covgpu_ransac_opts o;
    covgpu_default_ransac_opts(&o);
    o.min_inliers = (int32_t)mMinInliers; o.max_iterations = (int32_t)mMaxIter; o.threshold = th;
    o.probability = OptimizationT<Types>::params().ransac_probability;
    if (covgpu_abspose_ransac_batch(OptimizationT<Types>::Context(), &bt, &o) != COVGPU_OK) detail::fatal(covgpu_last_error());
    for (size_t s = 0; s < B; ++s) {
      AbsPoseJob& j = jobs[sel[s]];
      j.inliers = inl[s]; j.found = inl[s] > 0;
      if (!j.found) continue;                                        // :81-83: matches and Tws untouched
      LandmarkVector& m = *j.matches;
      std::vector<bool> keep(m.size(), false);
      for (int32_t c = ptr[s]; c < ptr[s + 1]; ++c) if (mask[c]) keep[indMap[s][c - ptr[s]]] = true;   // :85-93
      for (size_t i = 0; i < m.size(); ++i) if (!keep[i]) m[i].reset();                               // :94-98
      detail::pose_to_transform(&T[7 * s], *j.Tws);                                                   // :100-102
    }
  }
};


// ---- descriptor matching of the loop candidates (covgpu_match_batch): ComputeSE3's first step for all candidates of a
//      query keyframe in ONE library call. MatchLandmarksBatch is COVINS's LandmarkMatchingAlgorithm(50) + estd2::DenseMatcher(8)
//      over descriptors_ (placerec_be.cpp:84-90; rows without a valid landmark skipped, as LandmarkMatchingAlgorithm::doSetup does);
//      MatchImagesBatch is COVINS-G's BFMatcher(NORM_HAMMING).knnMatch(k = 2) + distance and ratio tests over descriptors_add_
//      (placerec_gen_be.cpp:82-114); MatchImagesFloatBatch is its SIFT branch (L2 over float rows, covgpu_match_float_batch, DESIGN.md
//      §4.17) and MatchImagePairsBatch takes any list of keyframe pairs, for both feature types. Each returns, per candidate, the match list in the reference's order (ascending idxB for the
//      former, ascending idxA for the latter); its size is ComputeSE3's nmatches. Invalid candidates are the caller's to drop first.
template <class Types>
class LoopMatcherT {
 public:
  using Keyframe = typename Types::Keyframe;
  using KeyframePtr = std::shared_ptr<Keyframe>;
  struct Match {   // covins::Match (matcher/MatchingAlgorithm.h): idxA in the query, idxB in the candidate
    size_t idxA, idxB;
    double distance;
  };
  using Matches = std::vector<Match>;

  using Landmark = typename Types::Landmark;
  using LandmarkPtr = std::shared_ptr<Landmark>;
  using LandmarkVector = std::vector<LandmarkPtr>;
  using TransformType = typename Types::TransformType;

  // ---- guided matching (covgpu_search_se3_batch / covgpu_search_projection_batch). The reference's constants:
  //      desc_matching_th_low_ and covins_params::features::scale_factor / num_octaves; agreement 0 = SearchBySE3's literal agreement
  //      test (feature_matcher_be.cpp:486-495), 1 = match2[match1[i]] == i.
  //      The three entry points are member templates only so that an explicit instantiation of LoopMatcherT on a binding without the
  //      members they read (keypoints_aors_, GetFeatureIndex, ...) still compiles; call them without template arguments.
  struct GuidedParams { int th_low = 50; double scale_factor = 2.0; int num_octaves = 1; int agreement = 0; };
  static GuidedParams& guided_params() { static GuidedParams p; return p; }

  // FeatureMatcher::SearchBySE3 (feature_matcher_be.cpp:293-498) for many (kf1, kf2, T12) in ONE library call: matches12[i] =
  // kf2->GetLandmarks()[match] for every agreed row, found = the return value. matches12 holds the matches so far (alreadyMatched).
  struct Se3SearchJob { KeyframePtr kf1, kf2; LandmarkVector* matches12 = nullptr; const TransformType* T12 = nullptr; int found = 0; };
  template <class Binding = Types>
  static void SearchBySE3Batch(std::vector<Se3SearchJob>& jobs, double th = 9.5) {
    const size_t J = jobs.size();
    if (J == 0) return;
    KpSets S;
    std::vector<double> K, pos, maxd, T(7 * J);
    std::vector<uint8_t> ldesc, lfree;
    std::vector<int32_t> s1(J), s2(J), off(J + 1, 0);
    std::vector<LandmarkVector> lms2(J);
    for (size_t j = 0; j < J; ++j) {
      Se3SearchJob& job = jobs[j];
      const LandmarkVector lms1 = job.kf1->GetLandmarks();
      lms2[j] = job.kf2->GetLandmarks();
      const size_t n1 = lms1.size(), n2 = lms2[j].size();
      if (job.matches12->size() < n1) job.matches12->resize(n1);
      std::vector<bool> already1(n1, false), already2(n2, false);                     // :313-324
      for (size_t i = 0; i < n1; ++i) {
        const LandmarkPtr& m = (*job.matches12)[i];
        if (!m) continue;
        already1[i] = true;
        const int idx2 = m->GetFeatureIndex(job.kf2);
        if (idx2 >= 0 && idx2 < (int)n2) already2[idx2] = true;
      }
      for (int side = 0; side < 2; ++side) {
        Keyframe& kf = side ? *job.kf2 : *job.kf1;
        const LandmarkVector& lms = side ? lms2[j] : lms1;
        const std::vector<bool>& already = side ? already2 : already1;
        (side ? s2 : s1)[j] = S.add(kf, lms.size());
        double intr[4], dist[4]; int dt = 0;
        if (!Types::camera(kf, intr, dist, &dt)) detail::fatal("Unknown projection / distortion type.");
        K.insert(K.end(), intr, intr + 4);                                             // calibration_.K (:297-298)
        TransformType Twc;
        detail::mat_mul(kf.GetPoseTws(), kf.GetStateExtrinsics(), Twc);                // GetPoseTcw()^-1 (:301-302)
        for (size_t i = 0; i < lms.size(); ++i) {
          double p3[3] = {0, 0, 0}, mx = 1.0, mn = 0.0, nrm[3];
          uint8_t d[32] = {};
          const LandmarkPtr& lm = lms[i];
          bool free = lm && !already[i] && !lm->IsInvalid();                           // :334-339, :412-418
          if (free) {
            detail::to_camera(Twc, lm->GetWorldPos(), p3);                             // :342-343, :421-422
            detail::landmark_scale<Types>(*lm, nrm, &mn, &mx, 0);
            free = detail::landmark_descriptor<Types>(*lm, d, 0);                      // (descrMP.cols == 0: every candidate is skipped, :386)
          }
          pos.insert(pos.end(), p3, p3 + 3); maxd.push_back(mx); ldesc.insert(ldesc.end(), d, d + 32); lfree.push_back(free ? 1 : 0);
        }
      }
      detail::transform_to_pose(*job.T12, &T[7 * j]);
      off[j + 1] = off[j] + (int32_t)n1;
    }
    std::vector<int32_t> match((size_t)off[J] + 1), nf(J);
    covgpu_search_se3_batch_t bt{};
    bt.sets = S.view();
    bt.K = K.data(); bt.lm_pos = pos.data(); bt.lm_max_distance = maxd.data(); bt.lm_desc = ldesc.data(); bt.lm_free = lfree.data();
    bt.num_jobs = (int32_t)J; bt.set_1 = s1.data(); bt.set_2 = s2.data(); bt.T12 = T.data(); bt.match = match.data(); bt.nfound = nf.data();
    const covgpu_guided_opts o = guided_opts(COVGPU_GUIDED_SE3, th);
    if (covgpu_search_se3_batch(OptimizationT<Types>::Context(), &bt, &o) != COVGPU_OK) detail::fatal(covgpu_last_error());
    for (size_t j = 0; j < J; ++j) {
      for (int32_t i = off[j]; i < off[j + 1]; ++i)
        if (match[i] >= 0) (*jobs[j].matches12)[i - off[j]] = lms2[j][match[i]];      // :491
      jobs[j].found = nf[j];
    }
  }
  // same signature as the reference
  template <class Binding = Types>
  static auto SearchBySE3(KeyframePtr kf1, KeyframePtr kf2, LandmarkVector& matches12, const TransformType T12, const double th) -> int {
    std::vector<Se3SearchJob> jobs(1);
    jobs[0].kf1 = kf1; jobs[0].kf2 = kf2; jobs[0].matches12 = &matches12; jobs[0].T12 = &T12;
    SearchBySE3Batch(jobs, th);
    return jobs[0].found;
  }

  // FeatureMatcher::SearchByProjection (feature_matcher_be.cpp:168-291; placerec_be.cpp:194), the reference's signature and return
  // value: claims go into vpMatched, remap proposals through Keyframe::RemapLandmark in point order.
  template <class Binding = Types>
  static auto SearchByProjection(KeyframePtr kf, TransformType Tcw, const LandmarkVector& points, LandmarkVector& matched, double th) -> int {
    KpSets S;
    S.add(*kf, matched.size());
    const size_t n = matched.size(), P = points.size();
    std::vector<uint8_t> taken(n), pdesc(32 * P + 32), skip(P + 1);
    std::set<const Landmark*> found;                                                   // spAlreadyFound (:175-176)
    for (size_t i = 0; i < n; ++i) { taken[i] = matched[i] ? 1 : 0; if (matched[i]) found.insert(matched[i].get()); }
    double cam[8], xi = 0.0, T[7];
    int32_t dt = 0, model = COVGPU_CAM_PINHOLE, set0 = 0, pptr[2] = {0, (int32_t)P}, nm = 0;
    int dti = 0, mi = 0;
    if (!Types::camera(*kf, cam, cam + 4, &dti) || !detail::camera_model<Types>(*kf, &mi, &xi, 0)) detail::fatal("Unknown projection / distortion type.");
    dt = dti; model = mi;
    detail::transform_to_pose(Tcw, T);
    std::vector<double> pw(3 * P + 3), nrm(3 * P + 3), mn(P + 1), mx(P + 1);
    std::vector<int32_t> existing(P + 1, -1), claimed(P + 1), remap(P + 1);
    for (size_t p = 0; p < P; ++p) {
      const LandmarkPtr& lm = points[p];
      skip[p] = !lm || lm->IsInvalid() || found.count(lm.get()) || !detail::landmark_descriptor<Types>(*lm, &pdesc[32 * p], 0);   // :184
      if (skip[p]) continue;
      const auto w = lm->GetWorldPos();
      for (int k = 0; k < 3; ++k) pw[3 * p + k] = w[k];
      detail::landmark_scale<Types>(*lm, &nrm[3 * p], &mn[p], &mx[p], 0);
      const int e = lm->GetFeatureIndex(kf);                                           // :260
      existing[p] = e >= 0 && e < (int)n ? e : -1;
    }
    covgpu_search_projection_batch_t bt{};
    bt.sets = S.view();
    bt.taken = taken.data(); bt.cam = cam; bt.dist_type = &dt; bt.cam_model = &model; bt.xi = &xi;
    bt.num_jobs = 1; bt.set = &set0; bt.T_cw = T; bt.point_ptr = pptr;
    bt.p_w = pw.data(); bt.normal = nrm.data(); bt.min_distance = mn.data(); bt.max_distance = mx.data(); bt.p_desc = pdesc.data();
    bt.skip = skip.data(); bt.existing_idx = existing.data(); bt.claimed = claimed.data(); bt.remap_to = remap.data(); bt.nmatches = &nm;
    const covgpu_guided_opts o = guided_opts(COVGPU_GUIDED_PROJECTION, th);
    if (covgpu_search_projection_batch(OptimizationT<Types>::Context(), &bt, &o) != COVGPU_OK) detail::fatal(covgpu_last_error());
    for (size_t p = 0; p < P; ++p) {
      if (claimed[p] >= 0) matched[claimed[p]] = points[p];                            // :284
      if (remap[p] >= 0) detail::remap_landmark<Types>(kf, points[p], (size_t)existing[p], (size_t)remap[p], 0);   // :280
    }
    return nm;
  }

  static std::vector<Matches> MatchLandmarksBatch(const KeyframePtr& query, const std::vector<KeyframePtr>& candidates, float thr = 50.0f) {
    covgpu_match_opts o;
    covgpu_default_match_opts(&o, COVGPU_MATCH_DENSE);
    o.dist_threshold = thr;
    return run(query, candidates, o, 0);
  }
  static std::vector<Matches> MatchImagesBatch(const KeyframePtr& query, const std::vector<KeyframePtr>& candidates, float img_match_thres = 40.0f,
                                               float ratio_thres = 0.8f) {
    covgpu_match_opts o;
    covgpu_default_match_opts(&o, COVGPU_MATCH_KNN2);
    o.dist_threshold = img_match_thres; o.ratio = ratio_thres;
    return run(query, candidates, o, 1);
  }

  // ---- float (SIFT) descriptors and arbitrary pair lists (covgpu_match_float_batch). Member templates for the
  //      reason given above: the float path reads cols / type() / isContinuous() of descriptors_add_ unless the binding has the trait
  //      Types::descriptors_f32. Call them without template arguments.
  // The SIFT branch of ComputeSE3 (placerec_gen_be.cpp:86-114): knnMatch(k = 2) over descriptors_add_ under the L2 norm + distance and
  // ratio tests, the exact search that the reference's FlannBasedMatcher approximates. Returns what MatchImagesBatch returns.
  template <class Binding = Types>
  static std::vector<Matches> MatchImagesFloatBatch(const KeyframePtr& query, const std::vector<KeyframePtr>& candidates,
                                                    float img_match_thres = 500.0f, float ratio_thres = 0.8f) {
    std::vector<std::pair<KeyframePtr, KeyframePtr>> pairs;
    for (const KeyframePtr& c : candidates) pairs.emplace_back(query, c);
    return run_pairs<Binding>(pairs, true, img_match_thres, ratio_thres);
  }
  // Any list of (query, train) keyframe pairs in ONE library call, every distinct keyframe uploaded once: what
  // RelNonCentralPosSolver::findMatches needs for its grid of query / candidate predecessors (RelNonCentralPosSolver.cpp:82-144,
  // :303-340). feature_type is covins_params::features::type: "ORB" goes to covgpu_match_batch (mode KNN2), "SIFT" to
  // covgpu_match_float_batch; anything else is the reference's fatal path. One match list per pair, ascending idxA.
  template <class Binding = Types>
  static std::vector<Matches> MatchImagePairsBatch(const std::vector<std::pair<KeyframePtr, KeyframePtr>>& pairs, const std::string& feature_type,
                                                   float img_match_thres, float ratio_thres = 0.8f) {
    if (feature_type != "ORB" && feature_type != "SIFT") detail::fatal("Wrong Feature Type: Only ORB or SIFT is supported currently");
    return run_pairs<Binding>(pairs, feature_type == "SIFT", img_match_thres, ratio_thres);
  }

 private:
  // keypoint sets of the guided matching: keypoints_distorted_, (int)keypoints_aors_[i][1], descriptors_ rows, bounds and grid state
  struct KpSets {
    std::vector<int32_t> ptr{0}, level;
    std::vector<float> kp;
    std::vector<uint8_t> desc;
    std::vector<double> bounds, grid;
    template <class K>   // (a template: instantiated only for bindings that call the guided matching)
    int32_t add(K& kf, size_t n) {
      int rows = 0; const uint8_t* data = nullptr;
      if (!detail::descriptors<Types>(kf, 0, &rows, &data, 0)) rows = 0;
      if ((size_t)rows < n || kf.keypoints_distorted_.size() < n || kf.keypoints_aors_.size() < n)
        detail::fatal("guided matching: fewer keypoints or descriptors than landmark slots");
      for (size_t i = 0; i < n; ++i) {
        kp.push_back(kf.keypoints_distorted_[i][0]); kp.push_back(kf.keypoints_distorted_[i][1]);
        level.push_back((int32_t)kf.keypoints_aors_[i][1]);
      }
      desc.insert(desc.end(), data, data + 32 * n);
      double b[4], g[2];
      detail::keyframe_image<Types>(kf, b, g, 0);
      bounds.insert(bounds.end(), b, b + 4); grid.insert(grid.end(), g, g + 2);
      ptr.push_back(ptr.back() + (int32_t)n);
      return (int32_t)ptr.size() - 2;
    }
    covgpu_keypoint_sets_t view() {
      kp.reserve(1); level.reserve(1); desc.reserve(1);                                // non-NULL data() for empty sets
      covgpu_keypoint_sets_t s{};
      s.num_sets = (int32_t)ptr.size() - 1; s.row_ptr = ptr.data(); s.kp = kp.data(); s.level = level.data(); s.desc = desc.data();
      s.bounds = bounds.data(); s.grid_inv = grid.data();
      return s;
    }
  };
  static covgpu_guided_opts guided_opts(int mode, double th) {
    covgpu_guided_opts o;
    covgpu_default_guided_opts(&o, mode);
    const GuidedParams& g = guided_params();
    o.th_low = g.th_low; o.radius = th; o.scale_factor = g.scale_factor; o.num_octaves = g.num_octaves; o.agreement = g.agreement;
    return o;
  }

  template <class Binding>
  static std::vector<Matches> run_pairs(const std::vector<std::pair<KeyframePtr, KeyframePtr>>& pairs, bool is_float, float thr, float ratio) {
    const size_t J = pairs.size();
    std::vector<Matches> out(J);
    if (J == 0) return out;
    std::map<const Keyframe*, int32_t> set_of;                         // every distinct keyframe is one set
    std::vector<int32_t> ptr(1, 0), sa(J), sb(J), off(J + 1, 0);
    std::vector<uint8_t> desc8;
    std::vector<float> descf;
    int dim = 0;
    auto add = [&](Keyframe& kf) -> int32_t {
      const auto it = set_of.find(&kf);
      if (it != set_of.end()) return it->second;
      int rows = 0;
      if (is_float) {
        int d = 0; const float* data = nullptr;
        if (!detail::descriptors_f32<Binding>(kf, &rows, &d, &data, 0)) rows = 0;
        if (rows > 0) {
          if (dim == 0) dim = d;
          if (d != dim) detail::fatal("float descriptors of different lengths in one batch");
          descf.insert(descf.end(), data, data + (size_t)rows * (size_t)d);
        }
      } else {
        const uint8_t* data = nullptr;
        if (!detail::descriptors<Binding>(kf, 1, &rows, &data, 0)) rows = 0;
        desc8.insert(desc8.end(), data, data + 32 * (size_t)rows);
      }
      ptr.push_back(ptr.back() + rows);
      return set_of[&kf] = (int32_t)ptr.size() - 2;
    };
    for (size_t j = 0; j < J; ++j) {
      sa[j] = add(*pairs[j].first); sb[j] = add(*pairs[j].second);
      off[j + 1] = off[j] + (ptr[sa[j] + 1] - ptr[sa[j]]);
    }
    const size_t total = (size_t)off[J];
    std::vector<int32_t> match(total + 1), nm(J);
    std::vector<int32_t> disti(is_float ? 1 : total + 1);
    std::vector<float> distf(is_float ? total + 1 : 1);
    covgpu_match_opts o;
    int rc;
    if (is_float) {
      covgpu_default_match_float_opts(&o);
      o.dist_threshold = thr; o.ratio = ratio;
      descf.reserve(1);                                                // non-NULL data() for empty sets
      covgpu_match_float_batch_t bt{};
      bt.num_sets = (int32_t)ptr.size() - 1; bt.row_ptr = ptr.data(); bt.dim = dim > 0 ? dim : 4; bt.desc = descf.data();
      bt.num_jobs = (int32_t)J; bt.set_a = sa.data(); bt.set_b = sb.data(); bt.match = match.data(); bt.dist = distf.data(); bt.nmatches = nm.data();
      rc = covgpu_match_float_batch(OptimizationT<Types>::Context(), &bt, &o);
    } else {
      covgpu_default_match_opts(&o, COVGPU_MATCH_KNN2);
      o.dist_threshold = thr; o.ratio = ratio;
      desc8.reserve(1);
      covgpu_match_batch_t bt{};
      bt.num_sets = (int32_t)ptr.size() - 1; bt.row_ptr = ptr.data(); bt.desc = desc8.data(); bt.skip = nullptr;
      bt.num_jobs = (int32_t)J; bt.set_a = sa.data(); bt.set_b = sb.data(); bt.match = match.data(); bt.dist = disti.data(); bt.nmatches = nm.data();
      rc = covgpu_match_batch(OptimizationT<Types>::Context(), &bt, &o);
    }
    if (rc != COVGPU_OK) detail::fatal(covgpu_last_error());
    for (size_t j = 0; j < J; ++j) {
      Matches& r = out[j];
      r.reserve((size_t)nm[j]);
      for (int32_t i = off[j]; i < off[j + 1]; ++i)
        if (match[i] >= 0) r.push_back(Match{(size_t)(i - off[j]), (size_t)match[i], is_float ? (double)distf[i] : (double)disti[i]});
    }
    return out;
  }

  static std::vector<Matches> run(const KeyframePtr& query, const std::vector<KeyframePtr>& candidates, const covgpu_match_opts& o, int which) {
    const bool dense = o.mode == COVGPU_MATCH_DENSE;
    const size_t J = candidates.size();
    std::vector<int32_t> ptr(1, 0), sa(J, 0), sb(J);
    std::vector<uint8_t> desc, skip;
    auto add = [&](Keyframe& kf) {
      int rows = 0; const uint8_t* data = nullptr;
      if (!detail::descriptors<Types>(kf, which, &rows, &data, 0)) rows = 0;
      desc.insert(desc.end(), data, data + 32 * (size_t)rows);
      if (dense)
        for (int k = 0; k < rows; ++k) {
          const auto lm = detail::landmark<Types>(kf, (size_t)k, 0);
          skip.push_back(!lm || lm->IsInvalid() ? 1 : 0);
        }
      ptr.push_back(ptr.back() + rows);
    };
    add(*query);
    for (size_t j = 0; j < J; ++j) { add(*candidates[j]); sb[j] = (int32_t)(j + 1); }
    const size_t nA = (size_t)ptr[1];
    std::vector<int32_t> match(nA * J + 1), dist(nA * J + 1), nm(J + 1);
    covgpu_match_batch_t bt{};
    bt.num_sets = (int32_t)J + 1; bt.row_ptr = ptr.data(); bt.desc = desc.data(); bt.skip = dense ? skip.data() : nullptr;
    bt.num_jobs = (int32_t)J; bt.set_a = sa.data(); bt.set_b = sb.data(); bt.match = match.data(); bt.dist = dist.data(); bt.nmatches = nm.data();
    if (covgpu_match_batch(OptimizationT<Types>::Context(), &bt, &o) != COVGPU_OK) detail::fatal(covgpu_last_error());
    std::vector<Matches> out(J);
    for (size_t j = 0; j < J; ++j) {
      const int32_t* m = &match[j * nA];
      const int32_t* d = &dist[j * nA];
      Matches& r = out[j];
      r.reserve((size_t)nm[j]);
      for (size_t a = 0; a < nA; ++a) if (m[a] >= 0) r.push_back(Match{a, (size_t)m[a], (double)d[a]});
      if (dense) std::sort(r.begin(), r.end(), [](const Match& x, const Match& y) { return x.idxB < y.idxB; });   // matchBody:98 emits by B row
    }
    return out;
  }
};

// ---- RelNonCentralPosSolver's five-point stage (RelNonCentralPosSolver.cpp:82-144, 343-377): the 2D-2D RANSAC between a query and
//      a candidate keyframe, batched (covgpu_fivept_ransac_batch). computePose has the reference's signature and
//      return value; ComputePoseBatch runs many of them in ONE library call per distinct threshold; ComputePoseGrid does what
//      computeNonCentralRelPose does in front of its 17-point stage, for ALL candidates of a query: the two predecessor chains, ONE
//      MatchImagePairsBatch, the mImgMatches test and ALL cells of ALL candidates in ONE covgpu_fivept_ransac_batch.
template <class Types>
class RelPoseSolverT {
 public:
  using Keyframe = typename Types::Keyframe;
  using KeyframePtr = std::shared_ptr<Keyframe>;
  using TransformType = typename Types::TransformType;
  using Matcher = LoopMatcherT<Types>;
  using Matches = typename Matcher::Matches;

  // the reference's defaults (RelNonCentralPosSolver.hpp:47-48); min_img_matches is covins_params::placerec::rel_pose::min_img_matches
  RelPoseSolverT(const size_t minInliers = 50, const double ransacProb = 0.99, const size_t maxIter = 300, const size_t minImgMatches = 0)
      : mMinInliers(minInliers), mRansacProb(ransacProb), mMaxIter(maxIter), mImgMatches(minImgMatches) {}
  void setRansacParams(const int minInliers, const double ransacProb, const int maxIter) {
    mMinInliers = (size_t)minInliers; mRansacProb = ransacProb; mMaxIter = (size_t)maxIter;
  }
  void setMinImgMatches(size_t n) { mImgMatches = n; }
  // what findMatches reads (RelNonCentralPosSolver.cpp:303-340): covins_params::features::type, img_match_thres, ratio_thres
  void setMatchParams(const std::string& feature_type, float img_match_thres, float ratio_thres = 0.8f) {
    mFeatureType = feature_type; mImgMatchThres = img_match_thres; mRatioThres = ratio_thres;
  }

  // one RANSAC: matches between kf1 (idxA) and kf2 (idxB). cell only moves the seed (0 for a call of its own).
  struct PoseJob {
    KeyframePtr kf1, kf2;
    const Matches* matches = nullptr;
    double threshold = 16.0;
    uint64_t cell = 0;
    TransformType* Tc1c2 = nullptr;          // written iff found (:373-374)
    std::vector<int>* inlierInd = nullptr;   // the model's inliers, ascending (opengv's inliers_); empty unless found
    bool found = false;                      // out: computePose's return value
    int status = 0;                          // out: COVGPU_FIVEPT_*
  };

  void ComputePoseBatch(std::vector<PoseJob>& jobs) const {
    std::vector<double> ths;
    for (const PoseJob& j : jobs) if (std::find(ths.begin(), ths.end(), j.threshold) == ths.end()) ths.push_back(j.threshold);
    for (double th : ths) run(jobs, th);
  }

  bool computePose(const KeyframePtr KfPtr1, const KeyframePtr KfPtr2, Matches& ImgMatches, const double threshold, TransformType& Tc1c2,
                   std::vector<int>& inlierInd) const {
    std::vector<PoseJob> jobs(1);
    jobs[0].kf1 = KfPtr1; jobs[0].kf2 = KfPtr2; jobs[0].matches = &ImgMatches; jobs[0].threshold = threshold; jobs[0].Tc1c2 = &Tc1c2;
    jobs[0].inlierInd = &inlierInd;
    ComputePoseBatch(jobs);
    return jobs[0].found;
  }

  // what FrameNoncentralRelativeAdapter is constructed from (:146-147), per candidate; ok = false is the reference's early `return false`
  // (a cell with fewer than mImgMatches matches, a failed cell, or a predecessor chain that ends early) and leaves the rest unspecified.
  struct GridResult {
    bool ok = false;
    std::vector<KeyframePtr> view_A, view_B;
    std::vector<std::vector<Matches>> match_vect;                  // [n_qkfs][n_ckfs]
    std::vector<std::vector<std::vector<int>>> inliers_vect;       // [n_qkfs][n_ckfs], indices ascending
    std::vector<int> inliers_size;                                 // query-major
    TransformType T_init;                                          // cell (0, 0)
    std::vector<std::vector<TransformType>> TF_vect;               // [0]: T_QKF_cw * T_wc of its chain, [1]: the candidate's (:94, 113)
  };

  template <class Binding = Types>
  std::vector<GridResult> ComputePoseGrid(const KeyframePtr& kf_query, const std::vector<KeyframePtr>& candidates, const double threshold,
                                          size_t n_qkfs = 2, size_t n_ckfs = 3) const {
    const std::string& feature_type = mFeatureType;
    const float img_match_thres = mImgMatchThres, ratio_thres = mRatioThres;
    const size_t NC = candidates.size(), cells = n_qkfs * n_ckfs;
    std::vector<GridResult> out(NC);
    std::vector<KeyframePtr> qs;
    for (KeyframePtr k = kf_query; k && qs.size() < n_qkfs; k = k->GetPredecessor()) qs.push_back(k);
    std::vector<std::pair<KeyframePtr, KeyframePtr>> pairs;
    std::vector<size_t> first(NC, (size_t)-1);
    for (size_t c = 0; c < NC; ++c) {
      GridResult& g = out[c];
      for (KeyframePtr k = candidates[c]; k && g.view_B.size() < n_ckfs; k = k->GetPredecessor()) g.view_B.push_back(k);
      if (qs.size() < n_qkfs || g.view_B.size() < n_ckfs) continue;
      g.view_A = qs;
      first[c] = pairs.size();
      for (const KeyframePtr& a : qs) for (const KeyframePtr& b : g.view_B) pairs.emplace_back(a, b);
    }
    std::vector<Matches> lists = Matcher::template MatchImagePairsBatch<Binding>(pairs, feature_type, img_match_thres, ratio_thres);
    std::vector<PoseJob> jobs;
    std::vector<TransformType> T(pairs.size());
    std::vector<std::vector<int>> inl(pairs.size());
    std::vector<size_t> job0(NC, (size_t)-1);
    for (size_t c = 0; c < NC; ++c) {
      if (first[c] == (size_t)-1) continue;
      bool enough = true;
      for (size_t q = 0; q < cells; ++q) enough = enough && lists[first[c] + q].size() >= mImgMatches;    // :119
      if (!enough) continue;
      job0[c] = jobs.size();
      for (size_t q = 0; q < cells; ++q) {
        PoseJob j;
        j.kf1 = pairs[first[c] + q].first; j.kf2 = pairs[first[c] + q].second; j.matches = &lists[first[c] + q]; j.threshold = threshold;
        j.cell = q; j.Tc1c2 = &T[first[c] + q]; j.inlierInd = &inl[first[c] + q];
        jobs.push_back(j);
      }
    }
    ComputePoseBatch(jobs);
    for (size_t c = 0; c < NC; ++c) {
      if (job0[c] == (size_t)-1) continue;
      GridResult& g = out[c];
      bool ok = true;
      for (size_t q = 0; q < cells; ++q) ok = ok && jobs[job0[c] + q].found;                               // :137-139
      if (!ok) continue;
      g.ok = true;
      g.match_vect.assign(n_qkfs, std::vector<Matches>(n_ckfs));
      g.inliers_vect.assign(n_qkfs, std::vector<std::vector<int>>(n_ckfs));
      for (size_t q = 0; q < cells; ++q) {
        g.match_vect[q / n_ckfs][q % n_ckfs] = lists[first[c] + q];
        g.inliers_vect[q / n_ckfs][q % n_ckfs] = inl[first[c] + q];
        g.inliers_size.push_back((int)inl[first[c] + q].size());
      }
      g.T_init = T[first[c]];
      g.TF_vect.assign(2, std::vector<TransformType>());
      for (const KeyframePtr& k : g.view_A) g.TF_vect[0].push_back(mul4(kf_query->GetPoseTcw(), k->GetPoseTwc()));
      for (const KeyframePtr& k : g.view_B) g.TF_vect[1].push_back(mul4(candidates[c]->GetPoseTcw(), k->GetPoseTwc()));
    }
    return out;
  }

  // ---- the 17-point stage and the loop covariance (RelNonCentralPosSolver.cpp:149-301, covgpu_ncrelpose_batch)
  struct NonCentralParams {               // covins_params::placerec::nc_rel_pose (config_backend.yaml:91-97)
    double rp_error = 1.5, rp_error_cov = 10.0;
    int min_inliers = 100, max_iters = 4000;
    double cov_thres = 10.0;
    int cov_iters = 30, cov_max_iters = 300;
  };
  void setNonCentralParams(const NonCentralParams& p) { mNc = p; }

  struct NonCentralResult {
    bool found = false;                   // computeNonCentralRelPose's return value
    int status = -1;                      // COVGPU_NCRELPOSE_*, -1: the five-point grid ended early (GridResult::ok false)
    int inliers = 0;
    TransformType Tc1c2, Ts1s2;           // the polished pose and the loop edge's measurement; written from status 4 on and at 0
    double cov_loop[36];                  // row-major, rotation first: LoopConstraint::cov_mat; the identity unless status is 0 or 6 (:73)
  };

  // computeNonCentralRelPose for ALL candidates of a query: ComputePoseGrid, then every GridResult with ok in ONE library call
  template <class Binding = Types>
  std::vector<NonCentralResult> ComputeNonCentralRelPoseBatch(const KeyframePtr& kf_query, const std::vector<KeyframePtr>& candidates,
                                                              const double threshold, size_t n_qkfs = 2, size_t n_ckfs = 3) const {
    const std::vector<GridResult> grid = ComputePoseGrid<Binding>(kf_query, candidates, threshold, n_qkfs, n_ckfs);
    const size_t NC = candidates.size(), cells = n_qkfs * n_ckfs;
    std::vector<NonCentralResult> out(NC);
    for (NonCentralResult& r : out)
      for (int i = 0; i < 36; ++i) r.cov_loop[i] = i % 7 == 0 ? 1.0 : 0.0;
    std::vector<size_t> sel;
    for (size_t c = 0; c < NC; ++c) if (grid[c].ok) sel.push_back(c);
    const size_t B = sel.size();
    if (B == 0) return out;
    std::vector<int32_t> ptr(1, 0), cell, cam1, cam2, cam_ptr(1, 0);
    std::vector<double> f1, f2, cam, Tq(7 * B), Tc(7 * B);
    std::vector<uint64_t> seed(B);
    for (size_t s = 0; s < B; ++s) {
      const GridResult& g = grid[sel[s]];
      const int32_t o0 = ptr.back();
      for (size_t i = 0; i < n_qkfs; ++i)                              // FrameNoncentralRelativeAdapter.cpp:83-105
        for (size_t j = 0; j < n_ckfs; ++j) {
          cell.push_back((int32_t)(f1.size() / 3) - o0);
          for (int k : g.inliers_vect[i][j]) {
            double a[3], b[3];
            detail::bearing_add<Types>(*g.view_A[i], g.match_vect[i][j][(size_t)k].idxA, a);
            detail::bearing_add<Types>(*g.view_B[j], g.match_vect[i][j][(size_t)k].idxB, b);
            f1.insert(f1.end(), a, a + 3); f2.insert(f2.end(), b, b + 3);
            cam1.push_back((int32_t)i); cam2.push_back((int32_t)(n_qkfs + j));
          }
        }
      cell.push_back((int32_t)(f1.size() / 3) - o0);
      ptr.push_back((int32_t)(f1.size() / 3));
      for (int side = 0; side < 2; ++side)                             // :111-118: first the query side's cameras, then the candidate's
        for (const TransformType& T : g.TF_vect[side]) {
          for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) cam.push_back(T(r, c));
          for (int r = 0; r < 3; ++r) cam.push_back(T(r, 3));
        }
      cam_ptr.push_back((int32_t)(cam.size() / 12));
      detail::transform_to_pose(kf_query->GetStateExtrinsics(), &Tq[7 * s]);
      detail::transform_to_pose(candidates[sel[s]]->GetStateExtrinsics(), &Tc[7 * s]);
      seed[s] = detail::ncrelpose_seed(kf_query.get(), candidates[sel[s]].get());
    }
    std::vector<double> T(7 * B, 0.0), Tr(7 * B, 0.0), Ts(7 * B, 0.0), cov(36 * B, 0.0);
    std::vector<uint8_t> mask(f1.size() / 3 + 1);
    std::vector<int32_t> inl(B), st(B), it(B), bd(B), cr(B), cd(B);
    f1.reserve(1); f2.reserve(1); cam1.reserve(1); cam2.reserve(1); cam.reserve(1);
    covgpu_ncrelpose_batch_t bt{};
    bt.num = (int32_t)B; bt.cells = (int32_t)cells; bt.corr_ptr = ptr.data(); bt.cell_ptr = cell.data(); bt.bearing1 = f1.data(); bt.bearing2 = f2.data();
    bt.cam1 = cam1.data(); bt.cam2 = cam2.data(); bt.cam_ptr = cam_ptr.data(); bt.cam = cam.data(); bt.T_sc_q = Tq.data(); bt.T_sc_c = Tc.data();
    bt.seed = seed.data(); bt.T_c1c2 = T.data(); bt.T_c1c2_ransac = Tr.data(); bt.T_s1s2 = Ts.data(); bt.cov = cov.data(); bt.inlier = mask.data();
    bt.inliers = inl.data(); bt.status = st.data(); bt.iterations = it.data(); bt.best_draw = bd.data(); bt.cov_rows = cr.data(); bt.cov_draws = cd.data();
    covgpu_ncrelpose_opts o;
    covgpu_default_ncrelpose_opts(&o);
    o.rp_error = mNc.rp_error; o.rp_error_cov = mNc.rp_error_cov; o.min_inliers = mNc.min_inliers; o.max_iterations = mNc.max_iters;
    o.cov_thres = mNc.cov_thres; o.cov_iters = mNc.cov_iters; o.cov_max_iters = mNc.cov_max_iters;
    o.probability = OptimizationT<Types>::params().ransac_probability;
    if (covgpu_ncrelpose_batch(OptimizationT<Types>::Context(), &bt, &o) != COVGPU_OK) detail::fatal(covgpu_last_error());
    for (size_t s = 0; s < B; ++s) {
      NonCentralResult& r = out[sel[s]];
      r.status = st[s]; r.found = st[s] == COVGPU_NCRELPOSE_FOUND; r.inliers = inl[s];
      if (st[s] == COVGPU_NCRELPOSE_FOUND || st[s] >= COVGPU_NCRELPOSE_THIN_CELL) {
        detail::pose_to_transform(&T[7 * s], r.Tc1c2);
        detail::pose_to_transform(&Ts[7 * s], r.Ts1s2);
      }
      if (st[s] == COVGPU_NCRELPOSE_FOUND || st[s] == COVGPU_NCRELPOSE_COV_TRACE)
        for (int i = 0; i < 36; ++i) r.cov_loop[i] = cov[36 * s + i];
    }
    return out;
  }

  // the reference's signature and return value; cov_loop is anything indexed (r, c) (an Eigen::Matrix<double, 6, 6>)
  template <class Cov, class Binding = Types>
  bool computeNonCentralRelPose(const KeyframePtr QKF, const KeyframePtr CKF, const double threshold, TransformType& Tc1c2, Cov& cov_loop) const {
    const std::vector<NonCentralResult> r = ComputeNonCentralRelPoseBatch<Binding>(QKF, std::vector<KeyframePtr>(1, CKF), threshold);
    for (int i = 0; i < 6; ++i) for (int j = 0; j < 6; ++j) cov_loop(i, j) = r[0].cov_loop[6 * i + j];
    if (r[0].status == COVGPU_NCRELPOSE_FOUND || r[0].status >= COVGPU_NCRELPOSE_THIN_CELL) Tc1c2 = r[0].Tc1c2;
    return r[0].found;
  }

 private:
  NonCentralParams mNc;
  size_t mMinInliers;
  double mRansacProb;   // stored, not used: see Params::ransac_probability (the reference never passes it to opengv either)
  size_t mMaxIter, mImgMatches;
  std::string mFeatureType = "ORB";
  float mImgMatchThres = 40.0f, mRatioThres = 0.8f;

  static TransformType mul4(TransformType A, TransformType B) {
    TransformType Cm = A;
    for (int r = 0; r < 4; ++r)
      for (int c = 0; c < 4; ++c) {
        double s = 0.0;
        for (int k = 0; k < 4; ++k) s += A(r, k) * B(k, c);
        Cm(r, c) = s;
      }
    return Cm;
  }

  void run(std::vector<PoseJob>& jobs, double th) const {
    std::vector<size_t> sel;
    for (size_t b = 0; b < jobs.size(); ++b) if (jobs[b].threshold == th) sel.push_back(b);
    const size_t B = sel.size();
    if (B == 0) return;
    std::vector<int32_t> ptr(1, 0);
    std::vector<double> f1, f2, T(7 * B, 0.0);
    std::vector<uint64_t> seed(B);
    for (size_t s = 0; s < B; ++s) {
      PoseJob& j = jobs[sel[s]];
      for (const auto& m : *j.matches) {                             // frame-relative-adapter.cpp:27-38
        double a[3], b[3];
        detail::bearing_add<Types>(*j.kf1, m.idxA, a);
        detail::bearing_add<Types>(*j.kf2, m.idxB, b);
        f1.insert(f1.end(), a, a + 3); f2.insert(f2.end(), b, b + 3);
      }
      ptr.push_back((int32_t)(f1.size() / 3));
      seed[s] = detail::fivept_seed(j.kf1.get(), j.kf2.get(), j.cell);
    }
    std::vector<uint8_t> mask(f1.size() / 3 + 1);
    std::vector<int32_t> inl(B), st(B);
    f1.reserve(1); f2.reserve(1);
    covgpu_fivept_batch_t bt{};
    bt.num = (int32_t)B; bt.corr_ptr = ptr.data(); bt.bearing1 = f1.data(); bt.bearing2 = f2.data(); bt.seed = seed.data();
    bt.T_12 = T.data(); bt.inlier = mask.data(); bt.inliers = inl.data(); bt.status = st.data();
    covgpu_fivept_opts o;
    covgpu_default_fivept_opts(&o);
    o.min_inliers = (int32_t)mMinInliers; o.max_iterations = (int32_t)mMaxIter; o.threshold = th;
    o.probability = OptimizationT<Types>::params().ransac_probability;
    if (covgpu_fivept_ransac_batch(OptimizationT<Types>::Context(), &bt, &o) != COVGPU_OK) detail::fatal(covgpu_last_error());
    for (size_t s = 0; s < B; ++s) {
      PoseJob& j = jobs[sel[s]];
      j.status = st[s]; j.found = st[s] == COVGPU_FIVEPT_FOUND;
      if (j.inlierInd) {
        j.inlierInd->clear();
        for (int32_t c = ptr[s]; c < ptr[s + 1]; ++c) if (mask[c]) j.inlierInd->push_back(c - ptr[s]);
      }
      if (j.found && j.Tc1c2) detail::pose_to_transform(&T[7 * s], *j.Tc1c2);
    }
  }
};


// ---- KeyframeDatabase with the reference's method names, the query batched on the GPU (covgpu_detect_candidates_batch, DESIGN.md
// §4.13), plus the bag-of-words transform of arriving keyframes (keyframe_be.cpp:159-183) and the covisibility-consistency groups of
// PlaceRecognition::DetectLoop (placerec_be.cpp:398-460). The database itself is a host-side insertion order; every call uploads what
// it needs. ResidentKeyframeDatabaseT below keeps the database on the device instead.
struct BowVocabulary {                             // the flat form of covgpu_bow_vocab_t, owning its arrays
  int32_t k = 0, L = 0, scoring = COVGPU_BOW_L1_NORM, weighting = COVGPU_BOW_TF_IDF, num_words = 0;
  std::vector<int32_t> parent, child_ptr, child, word_id;
  std::vector<uint8_t> desc;
  std::vector<double> weight;
  covgpu_bow_vocab_t view() const {
    covgpu_bow_vocab_t v{};
    v.num_nodes = (int32_t)parent.size(); v.num_words = num_words; v.k = k; v.L = L; v.scoring = scoring; v.weighting = weighting;
    v.parent = parent.data(); v.child_ptr = child_ptr.data(); v.child = child.data(); v.desc = desc.data(); v.word_id = word_id.data();
    v.weight = weight.data();
    return v;
  }
};

// ---- TemplatedVocabulary::create(training_features, k, L, weighting, scoring) on the device (covgpu_voc_train), with
// DBoW2's argument order and the seed of the counter-based draws behind it. A descriptor is anything with 32 bytes behind data() (a
// std::array<uint8_t, 32>) or behind a data member (a cv::Mat row). The result is the flat vocabulary KeyframeDatabaseT::ComputeBoWBatch
// and ResidentKeyframeDatabaseT take; stats, if given, receives the eight counters of covgpu_voc_train_t::stats.
namespace detail {
template <class D>
inline auto orb_row(const D& d, int) -> decltype(static_cast<const uint8_t*>(d.data())) { return d.data(); }
template <class D>
inline auto orb_row(const D& d, long) -> decltype(static_cast<const uint8_t*>(d.data)) { return d.data; }
}  // namespace detail

template <class Types, class D>
inline BowVocabulary CreateVocabulary(const std::vector<std::vector<D>>& training_features, int k, int L,
                                      int weighting = COVGPU_BOW_TF_IDF, int scoring = COVGPU_BOW_L1_NORM, uint64_t seed = 0,
                                      int64_t* stats = nullptr, int max_iterations = 0) {
  std::vector<int32_t> ptr(1, 0);
  std::vector<uint8_t> desc;
  for (const auto& set : training_features) {
    for (const auto& d : set) { const uint8_t* b = detail::orb_row(d, 0); desc.insert(desc.end(), b, b + 32); }
    ptr.push_back(ptr.back() + (int32_t)set.size());
  }
  desc.reserve(1);
  covgpu_voc_train_opts o;
  covgpu_default_voc_train_opts(&o);
  o.k = k; o.L = L; o.weighting = weighting; o.scoring = scoring; o.seed = seed;
  if (max_iterations > 0) o.max_iterations = max_iterations;
  const size_t R = (size_t)ptr.back();
  size_t full = 1, level = 1;                      // every node of a full tree, as far as the rows can fill it
  for (int l = 0; l < L && full <= 2 * R + 64; ++l) { level *= (size_t)(k > 1 ? k : 2); full += level; }
  size_t cap = std::min(full, 2 * R + 64);
  BowVocabulary voc;
  for (int attempt = 0;; ++attempt) {
    voc.parent.assign(cap, 0); voc.word_id.assign(cap, 0); voc.desc.assign(32 * cap, 0); voc.weight.assign(cap, 0.0);
    int32_t num_nodes = 0, num_words = 0;
    covgpu_voc_train_t t{};
    t.num_sets = (int32_t)training_features.size(); t.row_ptr = ptr.data(); t.desc = desc.data(); t.node_capacity = (int32_t)cap;
    t.num_nodes = &num_nodes; t.num_words = &num_words; t.parent = voc.parent.data(); t.desc_out = voc.desc.data();
    t.word_id = voc.word_id.data(); t.weight = voc.weight.data(); t.stats = stats;
    const int rc = covgpu_voc_train(OptimizationT<Types>::Context(), &t, &o);
    if (rc != COVGPU_OK && attempt == 0 && (size_t)num_nodes > cap) { cap = (size_t)num_nodes; continue; }   // emptied clusters outgrew the guess
    if (rc != COVGPU_OK) detail::fatal(covgpu_last_error());
    const size_t N = (size_t)num_nodes;
    voc.parent.resize(N); voc.word_id.resize(N); voc.desc.resize(32 * N); voc.weight.resize(N);
    voc.k = k; voc.L = L; voc.scoring = scoring; voc.weighting = weighting; voc.num_words = num_words;
    break;
  }
  // the children of a node have consecutive ids, so the child lists follow from parent
  const size_t N = voc.parent.size();
  voc.child_ptr.assign(N + 1, 0); voc.child.assign(N - 1, 0);
  for (size_t n = 1; n < N; ++n) ++voc.child_ptr[(size_t)voc.parent[n] + 1];
  for (size_t n = 0; n < N; ++n) voc.child_ptr[n + 1] += voc.child_ptr[n];
  std::vector<int32_t> at(voc.child_ptr.begin(), voc.child_ptr.end() - 1);
  for (size_t n = 1; n < N; ++n) voc.child[(size_t)at[(size_t)voc.parent[n]]++] = (int32_t)n;
  return voc;
}

template <class Types>
class KeyframeDatabaseT {
 public:
  using Keyframe = typename Types::Keyframe;
  using KeyframePtr = std::shared_ptr<Keyframe>;
  using KeyframeVector = std::vector<KeyframePtr>;

  struct Query {
    KeyframePtr kf;
    size_t db_visible = 0;                         // the query sees the first db_visible keyframes added (DetectCandidatesBatch)
    bool has_min_score = false;                    // false: the reference score of DetectLoop over kf's valid neighbours
    double min_score = 0.0;                        // in when has_min_score, out otherwise
    KeyframeVector candidates;                     // out, in the reference's order
    std::vector<float> acc_score;                  // out
  };

  explicit KeyframeDatabaseT(int mode = COVGPU_DETECT_COVINS) : mode_(mode) { covgpu_default_detect_opts(&opts_, mode); }
  covgpu_detect_opts& options() { return opts_; }
  size_t max_candidates = (size_t)-1;              // candidates kept per query (the output arrays are queries x this, at most the database size)

  void AddKeyframe(KeyframePtr kf) { order_.push_back(std::move(kf)); }
  void EraseKeyframe(const KeyframePtr& kf) { order_.erase(std::remove(order_.begin(), order_.end(), kf), order_.end()); }
  size_t size() const { return order_.size(); }

  KeyframeVector DetectCandidates(KeyframePtr kf, double min_score) {
    std::vector<Query> q(1);
    q[0].kf = std::move(kf); q[0].db_visible = order_.size(); q[0].has_min_score = true; q[0].min_score = min_score;
    DetectCandidatesBatch(q);
    return q[0].candidates;
  }

  // Either every query brings its min_score or none does.
  void DetectCandidatesBatch(std::vector<Query>& queries) {
    const bool g = mode_ == COVGPU_DETECT_COVINS_G;
    std::unordered_map<const Keyframe*, int32_t> index;
    KeyframeVector rows;
    auto row = [&](const KeyframePtr& kf) {
      auto it = index.find(kf.get());
      if (it != index.end()) return it->second;
      index.emplace(kf.get(), (int32_t)rows.size());
      rows.push_back(kf);
      return (int32_t)rows.size() - 1;
    };
    std::vector<int32_t> db, qk, vis;
    std::vector<double> ms;
    for (const auto& kf : order_) db.push_back(row(kf));
    bool given = !queries.empty() && queries[0].has_min_score;
    for (const auto& q : queries) {
      if (q.has_min_score != given) detail::fatal("DetectCandidatesBatch: min_score given for some queries only");
      qk.push_back(row(q.kf)); vis.push_back((int32_t)q.db_visible); ms.push_back(q.min_score);
    }
    // neighbour lists: whole for the queries, the first 10 for the database entries (more are never read)
    std::vector<std::vector<int32_t>> nbs(rows.size());
    std::vector<uint8_t> is_query(rows.size(), 0);
    for (int32_t k : qk) is_query[k] = 1;
    const size_t first = rows.size();
    std::vector<uint8_t> need_bow(first, 1);       // words of the database entries and the queries; other rows stay empty vectors
    for (size_t k = 0; k < first; ++k) {
      const auto con = detail::connected_keyframes<Types>(*rows[k], g, 0);
      const size_t n = is_query[k] ? con.size() : std::min<size_t>(con.size(), 10);
      std::vector<int32_t> l;
      for (size_t i = 0; i < n; ++i) l.push_back(row(con[i]));
      nbs.resize(rows.size());                     // (neighbours outside the database get a row and an empty list)
      if (is_query[k] && !given) { need_bow.resize(rows.size(), 0); for (int32_t i : l) need_bow[i] = 1; }   // the reference score reads them
      nbs[k] = std::move(l);
    }
    const size_t N = rows.size();
    need_bow.resize(N, 0);
    std::vector<int32_t> id(N), client(N), bptr(1, 0), word, nptr(1, 0), nb;
    std::vector<double> value;
    std::vector<uint8_t> invalid(N);
    for (size_t k = 0; k < N; ++k) {
      id[k] = (int32_t)rows[k]->id_.first; client[k] = (int32_t)rows[k]->id_.second; invalid[k] = rows[k]->IsInvalid() ? 1 : 0;
      if (need_bow[k]) detail::visit_bow<Types>(*rows[k], [&](int32_t w, double v) { word.push_back(w); value.push_back(v); }, 0);
      bptr.push_back((int32_t)word.size());
      nb.insert(nb.end(), nbs[k].begin(), nbs[k].end());
      nptr.push_back((int32_t)nb.size());
    }
    const size_t Q = queries.size(), cap = std::min(order_.size(), max_candidates);
    std::vector<int32_t> nc(Q + 1), cand(Q * cap + 1);
    std::vector<float> acc(Q * cap + 1);
    std::vector<double> mso(Q + 1);
    word.reserve(1); value.reserve(1); nb.reserve(1); db.reserve(1);
    covgpu_detect_batch_t bt{};
    bt.num_kf = (int32_t)N; bt.id = id.data(); bt.client = client.data(); bt.bow_ptr = bptr.data(); bt.word = word.data(); bt.value = value.data();
    bt.nb_ptr = nptr.data(); bt.nb = nb.data(); bt.invalid = invalid.data(); bt.num_db = (int32_t)db.size(); bt.db_order = db.data();
    bt.num_queries = (int32_t)Q; bt.query_kf = qk.data(); bt.db_visible = vis.data(); bt.min_score_in = given ? ms.data() : nullptr;
    bt.cap = (int32_t)cap; bt.num_candidates = nc.data(); bt.candidates = cand.data(); bt.acc_score = acc.data(); bt.min_score = mso.data();
    if (covgpu_detect_candidates_batch(OptimizationT<Types>::Context(), &bt, &opts_) != COVGPU_OK) detail::fatal(covgpu_last_error());
    for (size_t q = 0; q < Q; ++q) {
      queries[q].candidates.clear(); queries[q].acc_score.clear();
      queries[q].min_score = mso[q];
      for (size_t i = 0; i < std::min((size_t)nc[q], cap); ++i) {
        queries[q].candidates.push_back(rows[cand[q * cap + i]]);
        queries[q].acc_score.push_back(acc[q * cap + i]);
      }
    }
  }

  // voc->transform(descriptors_, bow_vec_, feat_vec_, levelsup) of every keyframe in one call
  static void ComputeBoWBatch(const BowVocabulary& voc, const KeyframeVector& kfs, int levelsup = 4) {
    std::vector<int32_t> ptr(1, 0);
    std::vector<uint8_t> desc;
    for (const auto& kf : kfs) {
      int rows = 0; const uint8_t* data = nullptr;
      if (!detail::descriptors<Types>(*kf, 0, &rows, &data, 0)) rows = 0;
      desc.insert(desc.end(), data, data + 32 * (size_t)rows);
      ptr.push_back(ptr.back() + rows);
    }
    const size_t R = (size_t)ptr.back(), S = kfs.size();
    std::vector<int32_t> bptr(S + 1), word(R + 1), rw(R + 1), rn(R + 1);
    std::vector<double> value(R + 1);
    desc.reserve(1);
    const covgpu_bow_vocab_t v = voc.view();
    covgpu_bow_transform_batch_t bt{};
    bt.num_sets = (int32_t)S; bt.row_ptr = ptr.data(); bt.desc = desc.data(); bt.levelsup = levelsup; bt.capacity = (int32_t)R;
    bt.bow_ptr = bptr.data(); bt.word = word.data(); bt.value = value.data(); bt.row_word = rw.data(); bt.row_node = rn.data();
    if (covgpu_bow_transform_batch(OptimizationT<Types>::Context(), &v, &bt) != COVGPU_OK) detail::fatal(covgpu_last_error());
    for (size_t s = 0; s < S; ++s) {
      detail::set_bow<Types>(*kfs[s], (size_t)(bptr[s + 1] - bptr[s]), &word[bptr[s]], &value[bptr[s]], 0);
      detail::set_features<Types>(*kfs[s], (size_t)(ptr[s + 1] - ptr[s]), &rw[ptr[s]], &rn[ptr[s]], 0);
    }
  }

  // mvConsistentGroups of DetectLoop: feed one query's candidates, get mvpEnoughConsistentCandidates. Sequential state of one detector.
  class ConsistencyFilter {
   public:
    explicit ConsistencyFilter(int threshold = 3, int mode = COVGPU_DETECT_COVINS) : threshold_(threshold), g_(mode == COVGPU_DETECT_COVINS_G) {}
    KeyframeVector Feed(const KeyframeVector& candidates) {
      KeyframeVector enough;
      if (candidates.empty()) { groups_.clear(); return enough; }
      std::vector<std::pair<std::set<const Keyframe*>, int>> current;
      std::vector<bool> used(groups_.size(), false);
      for (const auto& cand : candidates) {
        std::set<const Keyframe*> group;
        for (const auto& k : detail::connected_keyframes<Types>(*cand, g_, 0)) group.insert(k.get());
        group.insert(cand.get());
        bool is_enough = false, for_some = false;
        for (size_t i = 0; i < groups_.size(); ++i) {
          bool consistent = false;
          for (const Keyframe* k : group) if (groups_[i].first.count(k)) { consistent = true; break; }
          if (!consistent) continue;
          for_some = true;
          const int n = groups_[i].second + 1;
          if (!used[i]) { current.emplace_back(group, n); used[i] = true; }
          if (n >= threshold_ && !is_enough) { enough.push_back(cand); is_enough = true; }
        }
        if (!for_some) current.emplace_back(group, 0);
      }
      groups_ = std::move(current);
      return enough;
    }
    std::vector<int> Counters() const { std::vector<int> c; for (const auto& g : groups_) c.push_back(g.second); return c; }
   private:
    int threshold_;
    bool g_;
    std::vector<std::pair<std::set<const Keyframe*>, int>> groups_;
  };

 private:
  int mode_;
  covgpu_detect_opts opts_;
  KeyframeVector order_;
};

// ---- KeyframeDatabase kept on the device across calls (covgpu_bowdb): the reference's method names on a resident
// vocabulary, vector pool and inverted index. A query uploads the query's own lists; AddKeyframe / EraseKeyframe change the index in
// place. Keyframes are mapped to the handle's slots in the order this class first meets them. One object per context; its calls are
// serialised by the caller, as the reference's mtx_ does. KeyframeDatabaseT above is untouched and remains the stateless form.
//
// track_connections (default true): before each query the first ten connected keyframes and IsInvalid() of every live entry are read
// again and sent (40 B + 1 flag per entry), which is exact whatever happened to the covisibility graph. false: the class relies on
// TouchConnections(kf), which the integrator calls where the reference calls UpdateCovisibilityConnections or SetInvalid on kf.
template <class Types>
class ResidentKeyframeDatabaseT {
 public:
  using Keyframe = typename Types::Keyframe;
  using KeyframePtr = std::shared_ptr<Keyframe>;
  using KeyframeVector = std::vector<KeyframePtr>;

  struct Query {
    KeyframePtr kf;
    bool has_min_score = false;                    // false: the reference score of DetectLoop over kf's valid neighbours
    double min_score = 0.0;                        // in when has_min_score, out otherwise
    KeyframeVector candidates;                     // out, in the reference's order
    std::vector<float> acc_score;                  // out
  };

  // voc may be nullptr: ComputeBoW is then unavailable and vectors come from bow_vec_ (StoreBoW). Its arrays are read here only.
  explicit ResidentKeyframeDatabaseT(const BowVocabulary* voc = nullptr, int mode = COVGPU_DETECT_COVINS) : mode_(mode) {
    covgpu_default_bowdb_opts(&opts_, mode);
    if (voc) { voc_ = *voc; have_voc_ = true; }
  }
  ResidentKeyframeDatabaseT(const ResidentKeyframeDatabaseT&) = delete;
  ResidentKeyframeDatabaseT& operator=(const ResidentKeyframeDatabaseT&) = delete;
  ~ResidentKeyframeDatabaseT() { Close(); }
  void Close() { if (db_) covgpu_bowdb_destroy(db_); db_ = nullptr; }   // before the context goes (covgpu_destroy frees the handle too)
  covgpu_bowdb_opts& options() { return opts_; }   // read when the handle is made, at the first call that needs the device
  bool track_connections = true;
  size_t max_candidates = (size_t)-1;

  int32_t Slot(const KeyframePtr& kf) {
    auto it = slot_.find(kf.get());
    if (it != slot_.end()) return it->second;
    slot_.emplace(kf.get(), (int32_t)kfs_.size());
    kfs_.push_back(kf); stored_.push_back(0); live_.push_back(0);
    return (int32_t)kfs_.size() - 1;
  }
  size_t size() const { return num_live_; }
  KeyframeVector Order() {                         // the live keyframes in insertion order, read back from the device
    std::vector<int32_t> s(num_live_ + 1);
    int32_t n = 0;
    check(covgpu_bowdb_order(handle(), (int32_t)num_live_, s.data(), &n));
    KeyframeVector out;
    for (int32_t i = 0; i < n; ++i) out.push_back(kfs_[s[i]]);
    return out;
  }

  // voc->transform(descriptors_, bow_vec_, feat_vec_, levelsup) of every keyframe in one call; the vectors also stay on the device
  void ComputeBoW(const KeyframeVector& kfs) {
    std::vector<int32_t> ptr(1, 0), slot, id, client;
    std::vector<uint8_t> desc;
    for (const auto& kf : kfs) {
      int rows = 0; const uint8_t* data = nullptr;
      if (!detail::descriptors<Types>(*kf, 0, &rows, &data, 0)) rows = 0;
      desc.insert(desc.end(), data, data + 32 * (size_t)rows);
      ptr.push_back(ptr.back() + rows);
      slot.push_back(Slot(kf)); id.push_back((int32_t)kf->id_.first); client.push_back((int32_t)kf->id_.second);
    }
    const size_t R = (size_t)ptr.back(), S = kfs.size();
    std::vector<int32_t> bptr(S + 1), word(R + 1), rw(R + 1), rn(R + 1);
    std::vector<double> value(R + 1);
    desc.reserve(1);
    covgpu_bow_transform_batch_t bt{};
    bt.num_sets = (int32_t)S; bt.row_ptr = ptr.data(); bt.desc = desc.data(); bt.levelsup = opts_.levelsup; bt.capacity = (int32_t)R;
    bt.bow_ptr = bptr.data(); bt.word = word.data(); bt.value = value.data(); bt.row_word = rw.data(); bt.row_node = rn.data();
    check(covgpu_bowdb_put_descriptors(handle(), slot.data(), id.data(), client.data(), &bt));
    for (size_t s = 0; s < S; ++s) {
      detail::set_bow<Types>(*kfs[s], (size_t)(bptr[s + 1] - bptr[s]), &word[bptr[s]], &value[bptr[s]], 0);
      detail::set_features<Types>(*kfs[s], (size_t)(ptr[s + 1] - ptr[s]), &rw[ptr[s]], &rn[ptr[s]], 0);
      stored_[slot[s]] = 1;
    }
  }
  // the keyframes' bow_vec_ as they are (computed elsewhere), for those not stored yet
  void StoreBoW(const KeyframeVector& kfs) {
    std::vector<int32_t> slot, id, client, bptr(1, 0), word;
    std::vector<double> value;
    for (const auto& kf : kfs) {
      const int32_t s = Slot(kf);
      if (stored_[s] == 1 || stored_[s] == 2) continue;
      stored_[s] = 2;                              // (listed once)
      slot.push_back(s); id.push_back((int32_t)kf->id_.first); client.push_back((int32_t)kf->id_.second);
      detail::visit_bow<Types>(*kf, [&](int32_t w, double v) { word.push_back(w); value.push_back(v); }, 0);
      bptr.push_back((int32_t)word.size());
    }
    if (slot.empty()) return;
    word.reserve(1); value.reserve(1);
    check(covgpu_bowdb_put(handle(), (int32_t)slot.size(), slot.data(), id.data(), client.data(), bptr.data(), word.data(), value.data()));
    for (int32_t s : slot) stored_[s] = 1;
  }

  void AddKeyframe(const KeyframePtr& kf) {
    const int32_t s = Slot(kf);
    StoreBoW({kf});
    if (!track_connections) TouchConnections(kf);
    check(covgpu_bowdb_add(handle(), 1, &s));
    live_[s] = 1; ++num_live_;
  }
  void EraseKeyframe(const KeyframePtr& kf) {
    auto it = slot_.find(kf.get());
    if (it == slot_.end() || !live_[it->second]) return;
    check(covgpu_bowdb_erase(handle(), 1, &it->second));
    live_[it->second] = 0; --num_live_;
  }
  // the first ten connected keyframes and IsInvalid() of kf, as the device keeps them
  void TouchConnections(const KeyframePtr& kf) { send_connections({Slot(kf)}); }

  KeyframeVector DetectCandidates(KeyframePtr kf, double min_score) {
    std::vector<Query> q(1);
    q[0].kf = std::move(kf); q[0].has_min_score = true; q[0].min_score = min_score;
    DetectCandidatesBatch(q);
    return q[0].candidates;
  }

  // Every query sees the database as it is. Either every query brings its min_score or none does.
  void DetectCandidatesBatch(std::vector<Query>& queries) {
    const bool g = mode_ == COVGPU_DETECT_COVINS_G;
    const size_t Q = queries.size();
    if (Q == 0) return;
    const bool given = queries[0].has_min_score;
    std::vector<int32_t> qs, cptr(1, 0), con, flag_slot;
    std::vector<double> ms;
    std::vector<uint8_t> flag;
    KeyframeVector need;
    for (const auto& q : queries) {
      if (q.has_min_score != given) detail::fatal("DetectCandidatesBatch: min_score given for some queries only");
      need.push_back(q.kf);
      for (const auto& n : detail::connected_keyframes<Types>(*q.kf, g, 0)) {
        con.push_back(Slot(n));
        if (!given) {                              // the reference score reads the valid neighbours' vectors
          flag_slot.push_back(con.back()); flag.push_back(n->IsInvalid() ? 1 : 0);
          if (!n->IsInvalid()) need.push_back(n);
        }
      }
      cptr.push_back((int32_t)con.size()); ms.push_back(q.min_score);
    }
    StoreBoW(need);
    for (const auto& q : queries) qs.push_back(Slot(q.kf));
    if (!flag_slot.empty()) check(covgpu_bowdb_set_invalid(handle(), (int32_t)flag_slot.size(), flag_slot.data(), flag.data()));
    if (track_connections) {
      std::vector<int32_t> all;
      for (size_t s = 0; s < live_.size(); ++s) if (live_[s]) all.push_back((int32_t)s);
      send_connections(all);
    }
    const size_t cap = std::min(num_live_, max_candidates);
    std::vector<int32_t> nc(Q + 1), cand(Q * cap + 1);
    std::vector<float> acc(Q * cap + 1);
    std::vector<double> mso(Q + 1);
    con.reserve(1);
    covgpu_bowdb_query_t bq{};
    bq.num_queries = (int32_t)Q; bq.query_slot = qs.data(); bq.con_ptr = cptr.data(); bq.con = con.data();
    bq.min_score_in = given ? ms.data() : nullptr; bq.cap = (int32_t)cap;
    bq.num_candidates = nc.data(); bq.candidates = cand.data(); bq.acc_score = acc.data(); bq.min_score = mso.data();
    check(covgpu_bowdb_query(handle(), &bq));
    for (size_t q = 0; q < Q; ++q) {
      queries[q].candidates.clear(); queries[q].acc_score.clear();
      queries[q].min_score = mso[q];
      for (size_t i = 0; i < std::min((size_t)nc[q], cap); ++i) {
        queries[q].candidates.push_back(kfs_[cand[q * cap + i]]);
        queries[q].acc_score.push_back(acc[q * cap + i]);
      }
    }
  }

  void Stats(int64_t out[16]) { check(covgpu_bowdb_stats(handle(), out)); }

 private:
  static void check(int rc) { if (rc != COVGPU_OK) detail::fatal(covgpu_last_error()); }
  covgpu_bowdb* handle() {
    if (!db_) {
      covgpu_bow_vocab_t v{};
      if (have_voc_) v = voc_.view();
      check(covgpu_bowdb_create(OptimizationT<Types>::Context(), have_voc_ ? &v : nullptr, &opts_, &db_));
    }
    return db_;
  }
  void send_connections(const std::vector<int32_t>& slots) {
    if (slots.empty()) return;
    const bool g = mode_ == COVGPU_DETECT_COVINS_G;
    std::vector<int32_t> ptr(1, 0), nb;
    std::vector<uint8_t> flag;
    for (size_t i = 0; i < slots.size(); ++i) {    // (Slot() may grow kfs_: no reference into it is held)
      const KeyframePtr kf = kfs_[slots[i]];
      const auto con = detail::connected_keyframes<Types>(*kf, g, 0);
      for (size_t j = 0; j < std::min<size_t>(con.size(), 10); ++j) nb.push_back(Slot(con[j]));
      ptr.push_back((int32_t)nb.size());
      flag.push_back(kf->IsInvalid() ? 1 : 0);
    }
    nb.reserve(1);
    check(covgpu_bowdb_set_neighbours(handle(), (int32_t)slots.size(), slots.data(), ptr.data(), nb.data()));
    check(covgpu_bowdb_set_invalid(handle(), (int32_t)slots.size(), slots.data(), flag.data()));
  }

  int mode_;
  covgpu_bowdb_opts opts_;
  BowVocabulary voc_;
  bool have_voc_ = false;
  covgpu_bowdb* db_ = nullptr;
  std::unordered_map<const Keyframe*, int32_t> slot_;
  KeyframeVector kfs_;                             // slot -> keyframe
  std::vector<uint8_t> stored_, live_;
  size_t num_live_ = 0;
};

// ---- Map::RemoveRedundantData (map_be.cpp:745-811) ----
// MapPruneT<Types>::RemoveRedundantData(map, database, th_red, max_kfs) has the reference's semantics and return value (the reference
// takes the map manager and asks it for the database; here the caller passes the database). The map is flattened to one
// covgpu_prune_t (keyframe table = GetKeyframesVec() order, observations landmark-major through detail::visit_observations), the whole
// greedy loop runs in one covgpu_prune_redundant call (the exact integer rule and its three departures from the
// letter of std::sort / NaN / double sums), and the erases are replayed in round order through the map's own
// EraseKeyframeWithDatabase(kf, false, database). The caller holds the map as the reference does (its mtx_map_).
// What Keyframe keeps privately is read through Types: timestamp(kf) [s], is_loop_kf(kf), not_erase(kf).
template <class Types>
class MapPruneT {
 public:
  using Map = typename Types::Map;
  using Keyframe = typename Types::Keyframe;
  using MapPtr = std::shared_ptr<Map>;
  using KeyframePtr = std::shared_ptr<Keyframe>;

  struct Round { KeyframePtr kf; int action; };   // action: 0 erased, 1 time gate, 2 loop keyframe, 3 not_erase (covgpu_prune_t)
  static std::vector<Round>& last_rounds() { static thread_local std::vector<Round> v; return v; }
  static double& max_time_dist() { static double v = 1.0; return v; }   // covins_params::mapping::kf_culling_max_time_dist

  template <class DatabasePtr>
  static auto RemoveRedundantData(MapPtr map, DatabasePtr database, double th_red,
                                  size_t max_kfs = std::numeric_limits<size_t>::max()) -> size_t {
    map->Clean();   // :747
    auto keyframes = map->GetKeyframesVec();
    auto landmarks = map->GetLandmarksVec();
    const size_t K = keyframes.size();
    std::unordered_map<const Keyframe*, int32_t> row;
    row.reserve(2 * K + 16);
    std::vector<uint8_t> kf_invalid(K), kf_first(K), kf_loop(K), kf_not_erase(K), lm_invalid;
    std::vector<int32_t> pred(K, -1), succ(K, -1), obs_ptr{0}, obs_kf;
    std::vector<double> time(K);
    for (size_t k = 0; k < K; ++k) row[keyframes[k].get()] = (int32_t)k;
    auto row_of = [&](const KeyframePtr& kf) { auto it = kf ? row.find(kf.get()) : row.end(); return it == row.end() ? -1 : it->second; };
    for (size_t k = 0; k < K; ++k) {
      Keyframe& kf = *keyframes[k];
      kf_invalid[k] = kf.IsInvalid(); kf_first[k] = kf.id_.first == 0;
      kf_loop[k] = Types::is_loop_kf(kf); kf_not_erase[k] = Types::not_erase(kf);
      time[k] = Types::timestamp(kf);
      pred[k] = row_of(kf.GetPredecessor()); succ[k] = row_of(kf.GetSuccessor());
    }
    for (auto& lm : landmarks) {
      lm_invalid.push_back(lm->IsInvalid());
      detail::visit_observations<Types>(*lm, [&](const KeyframePtr& kf, size_t) { const int32_t r = row_of(kf); if (r >= 0) obs_kf.push_back(r); }, 0);
      obs_ptr.push_back((int32_t)obs_kf.size());
    }
    std::vector<int32_t> round_kf(K ? K : 1), round_action(K ? K : 1);
    int32_t num_rounds = 0, removed = 0, stop = 0;
    covgpu_prune_t p{};
    p.num_kf = (int32_t)K; p.num_lm = (int32_t)landmarks.size();
    p.lm_obs_ptr = obs_ptr.data(); p.obs_kf = obs_kf.data(); p.lm_invalid = lm_invalid.data();
    p.kf_invalid = kf_invalid.data(); p.kf_first = kf_first.data(); p.kf_loop = kf_loop.data(); p.kf_not_erase = kf_not_erase.data();
    p.kf_pred = pred.data(); p.kf_succ = succ.data(); p.kf_time = time.data();
    p.capacity = (int32_t)K; p.round_kf = round_kf.data(); p.round_action = round_action.data();
    p.num_rounds = &num_rounds; p.removed = &removed; p.stop_reason = &stop;
    covgpu_prune_opts o;
    covgpu_default_prune_opts(&o);
    o.th_red = th_red; o.max_time_dist = max_time_dist();
    if (max_kfs != std::numeric_limits<size_t>::max()) o.max_kfs = (int32_t)std::min<size_t>(max_kfs, (size_t)INT32_MAX);
    if (covgpu_prune_redundant(OptimizationT<Types>::Context(), &p, &o) != COVGPU_OK) detail::fatal(covgpu_last_error());
    std::vector<Round>& rounds = last_rounds();
    rounds.clear();
    for (int32_t r = 0; r < num_rounds; ++r) {
      rounds.push_back({keyframes[round_kf[r]], round_action[r]});
      // action 3 too: the reference calls the erase, SetInvalid refuses (keyframe_be.cpp:510), and the call is counted (:776-777)
      if (round_action[r] == 0 || round_action[r] == 3) map->EraseKeyframeWithDatabase(keyframes[round_kf[r]], false, database);
    }
    return (size_t)removed;
  }
};

// ---- Landmark::ComputeDescriptor (landmark_be.cpp:49-92) + Landmark::UpdateNormal (:185-220) for many landmarks ----
// LandmarkRefreshT<Types>::Refresh(map) / Refresh(landmarks) replaces the serial loops that call the two member functions per landmark
// (map_be.cpp:660-661 after a load, communicator_be.cpp:190-198 for a received keyframe's landmarks, placerec_be.cpp:279, 495, 500 after
// a fusion): the landmarks are flattened to one covgpu_landmark_refresh_t — observations in the order detail::visit_observations
// yields them, each with its keyframe's descriptor row (detail::descriptors) and octave (keypoints_aors_[feat](1)), camera centres
// from GetPoseTwc() — one covgpu_landmark_refresh call runs, and the results are written back through
// Types::set_landmark_descriptor / Types::set_landmark_scale. The one departure from the letter of the reference is the order: the
// reference's std::map is keyed by shared_ptr address, so its tie-break and summation order are the allocator's; here they are the
// visit's, one outcome the reference can produce. A landmark without a valid observer keeps its descriptor (ComputeDescriptor
// returns early); UpdateNormal exits on a landmark without reference keyframe or without observations, and so does this, with the
// reference's message, before anything is written. Invalid landmarks are skipped. The caller holds the map as the reference does.
template <class Types>
class LandmarkRefreshT {
 public:
  using Map = typename Types::Map;
  using Keyframe = typename Types::Keyframe;
  using Landmark = typename Types::Landmark;
  using MapPtr = std::shared_ptr<Map>;
  using KeyframePtr = std::shared_ptr<Keyframe>;
  using LandmarkPtr = std::shared_ptr<Landmark>;

  struct Params { double scale_factor = 2.0; int num_octaves = 1; };   // covins_params::features::scale_factor / num_octaves
  static Params& params() { static Params p; return p; }
  // landmarks per kernel form of the calling thread's last call (covgpu_landmark_refresh_t::form_count)
  static std::array<int32_t, COVGPU_LMR_FORMS>& last_forms() { static thread_local std::array<int32_t, COVGPU_LMR_FORMS> f{}; return f; }

  static void Refresh(MapPtr map) { Refresh(map->GetLandmarksVec()); }

  static void Refresh(const std::vector<LandmarkPtr>& landmarks) {
    const size_t L = landmarks.size();
    std::unordered_map<const Keyframe*, int32_t> row;
    std::vector<uint8_t> kf_invalid, lm_invalid(L), obs_desc;
    std::vector<const uint8_t*> kf_desc;
    std::vector<int> kf_rows;
    std::vector<double> center, pos(3 * L);
    std::vector<int32_t> obs_ptr{0}, obs_kf, obs_octave, ref_obs(L, -1);
    auto row_of = [&](Keyframe& kf) -> int32_t {
      auto it = row.find(&kf);
      if (it != row.end()) return it->second;
      const int32_t r = (int32_t)kf_invalid.size();
      row.emplace(&kf, r);
      kf_invalid.push_back(kf.IsInvalid());
      double c[3];
      detail::camera_center<Types>(kf, c, 0);
      center.insert(center.end(), c, c + 3);
      int rows = 0; const uint8_t* data = nullptr;
      if (!detail::descriptors<Types>(kf, 0, &rows, &data, 0)) { rows = 0; data = nullptr; }
      kf_rows.push_back(rows); kf_desc.push_back(data);
      return r;
    };
    for (size_t l = 0; l < L; ++l) {
      Landmark& lm = *landmarks[l];
      lm_invalid[l] = lm.IsInvalid();
      const auto p = lm.GetWorldPos();
      pos[3 * l] = p[0]; pos[3 * l + 1] = p[1]; pos[3 * l + 2] = p[2];
      const KeyframePtr ref = lm.GetReferenceKeyframe();
      const int32_t first = obs_ptr.back();
      detail::visit_observations<Types>(lm, [&](const KeyframePtr& kf, size_t feat) {
        if (!kf) return;
        const int32_t r = row_of(*kf);
        if (ref && kf.get() == ref.get() && ref_obs[l] < 0) ref_obs[l] = (int32_t)obs_kf.size() - first;
        obs_kf.push_back(r);
        obs_octave.push_back(feat < kf->keypoints_aors_.size() ? (int32_t)kf->keypoints_aors_[feat][1] : -1);
        const size_t at = obs_desc.size();
        obs_desc.resize(at + 32, 0);
        if (!kf_invalid[r]) {   // (ComputeDescriptor reads the rows of valid keyframes only)
          if (!kf_desc[r] || feat >= (size_t)kf_rows[r]) detail::fatal("LandmarkRefreshT: an observation without a descriptor row");
          std::memcpy(&obs_desc[at], kf_desc[r] + 32 * feat, 32);
        }
      }, 0);
      obs_ptr.push_back((int32_t)obs_kf.size());
    }
    const size_t K = kf_invalid.size();
    std::vector<int32_t> desc_obs(L ? L : 1), status(L ? L : 1);
    std::vector<uint8_t> desc(32 * (L ? L : 1));
    std::vector<double> normal(3 * (L ? L : 1)), mind(L ? L : 1), maxd(L ? L : 1);
    covgpu_landmark_refresh_t p{};
    p.num_kf = (int32_t)K; p.num_lm = (int32_t)L;
    p.lm_obs_ptr = obs_ptr.data(); p.obs_kf = obs_kf.data(); p.obs_desc = obs_desc.data(); p.obs_octave = obs_octave.data();
    p.lm_ref_obs = ref_obs.data(); p.lm_pos = pos.data(); p.kf_center = center.data();
    p.kf_invalid = kf_invalid.data(); p.lm_invalid = lm_invalid.data();
    p.lm_desc_obs = desc_obs.data(); p.lm_desc = desc.data(); p.lm_normal = normal.data();
    p.lm_min_distance = mind.data(); p.lm_max_distance = maxd.data(); p.lm_status = status.data();
    p.form_count = last_forms().data();
    uint8_t none = 0;
    if (obs_desc.empty()) p.obs_desc = &none;   // (no observation at all: still "descriptors asked for")
    covgpu_landmark_refresh_opts o;
    covgpu_default_landmark_refresh_opts(&o);
    o.scale_factor = params().scale_factor; o.num_octaves = params().num_octaves;
    if (covgpu_landmark_refresh(OptimizationT<Types>::Context(), &p, &o) != COVGPU_OK) detail::fatal(covgpu_last_error());
    for (size_t l = 0; l < L; ++l) {
      if (status[l] & 4) continue;
      if (status[l] & 2) {   // landmark_be.cpp:188-191
        const std::string m = "LM (" + std::to_string(landmarks[l]->id_.first) + "," + std::to_string(landmarks[l]->id_.second) + "): no ref-KF";
        detail::fatal(m.c_str());
      }
      if (status[l] & 1) detail::fatal("no obervations");   // :192-195 (the reference's spelling)
    }
    for (size_t l = 0; l < L; ++l) {
      if (status[l] & 4) continue;
      if (desc_obs[l] >= 0) detail::set_landmark_descriptor<Types>(*landmarks[l], &desc[32 * l], 0);
      detail::set_landmark_scale<Types>(*landmarks[l], &normal[3 * l], mind[l], maxd[l], 0);
    }
  }
};

}  // namespace covins_gpu
