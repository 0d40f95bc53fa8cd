/*
 * covgpu.h — C ABI of the MI355X-native global-bundle-adjustment / pose-graph back-end.
 *
 * This is the drop-in boundary for the ONE hot path of COVINS that this repository
 * replaces:
 *
 *   covins::Optimization::GlobalBundleAdjustment   reference: covins_backend/include/covins/
 *   covins::Optimization::PoseGraphOptimization               covins_backend/optimization_be.hpp:38-51
 *
 * The reference has no FFI or plugin registry for this path — callers link the two static
 * member functions directly (backend.cpp:141-156, placerec_be.cpp:327, placerec_gen_be.cpp:250).
 * The C++ facade in include/covins_gpu/optimization_gpu.hpp keeps those two signatures verbatim,
 * walks Map/Keyframe/Landmark exactly as optimization_be.cpp does, flattens them into the
 * `covgpu_problem` intermediate representation below, and calls the entry points of this header.
 * Nothing here knows about Map/Keyframe, Eigen, torch or any C++ type: plain pointers and sizes.
 *
 * All floating point is FP64 (reference: precision_t = double, typedefs_base.hpp:129).
 * Quaternions are Hamilton, stored [x,y,z,w]; a pose block is [qx,qy,qz,qw,px,py,pz] = T_w_s
 * (keyframe_base.cpp:486-499); a speed-bias block is [v_w(3), b_a(3), b_g(3)] (:513-521).
 */
#ifndef COVGPU_H_
#define COVGPU_H_

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- status codes */
enum {
  COVGPU_OK = 0,
  COVGPU_ERR_INVALID_ARG = 1,   /* malformed problem (index out of range, NULL array, ...)   */
  COVGPU_ERR_NO_DEVICE = 2,     /* no HIP device / HIP runtime failure                        */
  COVGPU_ERR_OUT_OF_MEMORY = 3, /* device allocation failed                                   */
  COVGPU_ERR_NUMERIC = 4,       /* single linear solve not positive definite (covgpu_solve_reduced, covgpu_gn_step) */
  COVGPU_ERR_FATAL_MAP = 5      /* conditions on which the reference calls exit(-1)           */
};
/* The stateless batch calls (covgpu_relpose_batch, covgpu_abspose_ransac_batch, covgpu_p3p_batch, covgpu_match_batch, covgpu_match_float_batch,
 * covgpu_search_se3_batch, covgpu_search_projection_batch, covgpu_pgo_reanchor, covgpu_bow_transform_batch, covgpu_bow_score_pairs,
 * covgpu_detect_candidates_batch, covgpu_prune_redundant, covgpu_landmark_refresh; covins_amd/csrc/batch.hip; covgpu_voc_train;
 * covins_amd/csrc/voctrain.hip) share one convention: a NULL context is COVGPU_ERR_INVALID_ARG with the
 * message "<function>: NULL context", and every argument is checked before any device work. */

/* trust-region strategy (reference uses DOGLEG: optimization_be.cpp:261,564,1028;
 * BASELINE.json north_star asks for Levenberg-Marquardt as well) */
enum { COVGPU_DOGLEG = 0, COVGPU_LM = 1 };

/* lens distortion of a camera (reference dispatch: optimization_be.cpp:483-521; KeyframeBase can
 * only construct RadTan / Equidistant, keyframe_base.cpp:58-82) */
enum { COVGPU_DIST_RADTAN = 0, COVGPU_DIST_EQUIDISTANT = 1 };

/* projection model of a camera; the values are those of the reference's eCamModel (keyframe_base.cpp:58-82).
 * COVGPU_CAM_UNIFIED is aslam::UnifiedProjectionCamera: parameters [xi, fu, fv, cu, cv], with xi in cam_xi and fu fv cu cv in
 * cam_intr; d = |l_C|, m = (X, Y) / (Z + xi d) goes through the camera's distortion. */
enum { COVGPU_CAM_PINHOLE = 0, COVGPU_CAM_UNIFIED = 1 };

/* ---------------------------------------------------------------- options */
typedef struct covgpu_options {
  int32_t strategy;            /* COVGPU_DOGLEG | COVGPU_LM                                         */
  int32_t max_iterations;      /* trust-region iterations incl. rejected (Ceres max_num_iterations) */
  int32_t visual_only;         /* 1: no speed-bias blocks, no IMU factors (opt_be.cpp:332,367)      */
  int32_t device;              /* HIP device ordinal                                                */
  double  reproj_loss_a;       /* Cauchy scale on reprojection blocks, 1.0 (opt_be.cpp:302);  0=off */
  double  initial_radius;      /* 1e4  (Ceres default initial_trust_region_radius)                  */
  double  max_radius;          /* 1e16                                                              */
  double  min_relative_decrease; /* 1e-3                                                            */
  double  function_tolerance;  /* 1e-6                                                              */
  double  parameter_tolerance; /* 1e-8                                                              */
  double  gradient_tolerance;  /* 1e-10                                                             */
  /* IMU noise, already discretised (orb_slam3/src/Tracking.cc:1203-1211) and gravity magnitude */
  double  sigma_a, sigma_g, sigma_aw, sigma_gw, gravity;
  int32_t verbose;
  int32_t shard_policy;        /* sharded solve: 0 replicated top (default) | 1 distributed top (COVGPU_SHARD_POLICY overrides) */
} covgpu_options;

/* Fills `o` with the reference's effective settings (dogleg, 10 iterations, Cauchy(1), Ceres 1.x
 * defaults, EuRoC IMU noise at 200 Hz, g = 9.81). */
void covgpu_default_options(covgpu_options* o);

/* ---------------------------------------------------------------- flat problem IR
 * All pointers are HOST pointers owned by the caller; nothing is retained after a call returns.
 * Index arrays are int32. In/out arrays are overwritten with the optimised estimate.            */
typedef struct covgpu_problem {
  int32_t num_kf;        /* K  valid keyframes                                    */
  int32_t num_cam;       /* A  distinct cameras (one per agent in COVINS)         */
  int32_t num_lm;        /* L  landmarks that passed the >=2-observation gate     */
  int32_t num_obs;       /* O  reprojection residual blocks                       */
  int32_t num_imu;       /* I  IMU preintegration factors                         */
  int32_t num_edge;      /* E  SE3 between factors (loops; PGO odometry edges)    */
  int32_t num_imu_samples; /* S total raw IMU samples over all factors           */
  int32_t reserved;

  /* keyframes */
  double*        kf_pose;        /* [K][7]  in/out  T_w_s                          */
  double*        kf_speed_bias;  /* [K][9]  in/out  (NULL allowed if visual_only)  */
  const uint8_t* kf_fixed;       /* [K]     1 = pose block constant (opt_be.cpp:329-341, 870-881) */
  const int32_t* kf_cam;         /* [K]     camera index                           */

  /* cameras: extrinsics T_s_c, intrinsics fx fy cx cy, 4 distortion coefficients; all constant
   * in every call site (opt_be.cpp:336,349,352) */
  const double*  cam_extr;       /* [A][7] */
  const double*  cam_intr;       /* [A][4] */
  const double*  cam_dist;       /* [A][4] */
  const int32_t* cam_dist_type;  /* [A]    */

  /* landmarks + observations. Observations are grouped by landmark (the reference's iteration
   * order, opt_be.cpp:432-530): those of landmark l are [lm_obs_ptr[l], lm_obs_ptr[l+1]), in any keyframe order.
   * A landmark has at most ONE observation per keyframe (the reference keys a landmark's observations by keyframe): two
   * observations of a landmark by the same keyframe are COVGPU_ERR_INVALID_ARG ("landmark observed twice by one keyframe") —
   * the covisible-pair lists never pair a keyframe with itself, so their cross terms would be missing from the reduced system. */
  double*        lm_pos;         /* [L][3]  in/out  world position                 */
  const int32_t* lm_obs_ptr;     /* [L+1]                                          */
  const int32_t* obs_kf;         /* [O]                                            */
  const double*  obs_uv;         /* [O][2]  keypoint, float32 promoted to double (opt_be.cpp:477) */
  const double*  obs_sigma;      /* [O]     (octave+1)*2 px (opt_be.cpp:478)       */

  /* IMU factors between predecessor kf_i and successor kf_j (opt_be.cpp:369-416). The raw samples
   * are part of the IR because the reference re-propagates the preintegration with the current
   * bias estimate once per solve (opt_be.cpp:396). Sample = [dt, ax,ay,az, wx,wy,wz]. */
  const int32_t* imu_kf_i;       /* [I] */
  const int32_t* imu_kf_j;       /* [I] */
  const int32_t* imu_sample_ptr; /* [I+1] */
  const double*  imu_samples;    /* [S][7] */
  const double*  imu_first;      /* [I][6]  (acc_0, gyr_0): reading at the predecessor (keyframe_be.cpp:187,195) */
  /* Per-factor IMU calibration [sigma_a, sigma_g, sigma_aw, sigma_gw, gravity]: the reference builds every keyframe's
   * preintegrator from THAT keyframe's own calibration (keyframe_be.cpp:187-195: sigma_a_c, sigma_g_c, sigma_aw_c,
   * sigma_gw_c, g), so mixed agents / IMUs keep their own weights. NULL: the five values of covgpu_options apply to
   * every factor. A row with a non-positive sigma or gravity < 9 (keyframe_base.cpp:51-55) is COVGPU_ERR_INVALID_ARG.
   * The values (given or taken from the options) are captured by covgpu_upload / covgpu_gba_solve: the sigma_* / gravity
   * fields of the options passed to a later covgpu_solve_resident are not read again. */
  const double*  imu_noise;      /* [I][5] or NULL */

  /* SE3 between factors (robopt SixDofBetweenError, kImu): measurement T_s1_s2 as [q(4), t(3)],
   * row-major 6x6 sqrt-information (rotation rows first), Cauchy scale per edge (0 = no loss). */
  const int32_t* edge_i;         /* [E] */
  const int32_t* edge_j;         /* [E] */
  const double*  edge_meas;      /* [E][7] */
  const double*  edge_sqrt_info; /* [E][36] */
  const double*  edge_loss_a;    /* [E] */

  /* camera models (appended: the offsets above are unchanged). cam_model NULL = every camera pinhole and cam_xi is not read.
   * An unknown model, a unified row with cam_xi NULL, or a non-finite or negative xi is COVGPU_ERR_INVALID_ARG. */
  const int32_t* cam_model;      /* [A] COVGPU_CAM_* or NULL                        */
  const double*  cam_xi;         /* [A] xi of the unified rows (others not read)   */
} covgpu_problem;

/* per-iteration trace, for parity tests against the oracle */
#define COVGPU_MAX_TRACE 64
typedef struct covgpu_result {
  int32_t iterations;          /* trust-region iterations executed                          */
  int32_t accepted;            /* of which successful                                       */
  int32_t termination;         /* 0 max-iter, 1 function tol, 2 parameter tol, 3 gradient tol, 4 failure: the reduced system stayed
                                * non-positive-definite up to the largest damping. Like ceres::Solve (whose summary the reference
                                * ignores, opt_be.cpp:567) the call still returns COVGPU_OK and the LAST ACCEPTED estimate; callers that
                                * care check this field. COVGPU_ERR_NUMERIC is returned by covgpu_solve_reduced / covgpu_gn_step only. */
  int32_t reserved;            /* IMU factors that carry no weight (their whitening matrix is all zeros): every factor of FEWER THAN TWO samples,
                                * by rule — one midpoint step leaves a covariance whose position rows are dt/2 times its velocity rows, exactly
                                * singular, so no pivot test is asked — and every factor whose preintegrated covariance is not positive definite */
  double  initial_cost;
  double  final_cost;
  double  t_upload_s;          /* H2D incl. layout build                                    */
  double  t_solve_s;           /* device-resident solve (the timed region of bench.py)      */
  double  t_download_s;        /* D2H                                                       */
  double  t_linear_solve_s;    /* part of t_solve_s spent in the reduced-system factor+solve */
  double  cost_trace[COVGPU_MAX_TRACE];    /* cost after each iteration */
  double  radius_trace[COVGPU_MAX_TRACE];
  int32_t accepted_trace[COVGPU_MAX_TRACE];
} covgpu_result;

/* ---------------------------------------------------------------- context */
typedef struct covgpu_context covgpu_context;

/* One context per calling thread / map (the reference may run PGO for different maps on
 * different place-recognition threads, placerec_be.cpp:295). Owns one HIP stream + workspace. */
int  covgpu_create(const covgpu_options* opt, covgpu_context** out);
void covgpu_destroy(covgpu_context* ctx);
const char* covgpu_last_error(void);

/* ---------------------------------------------------------------- solve entry points
 * covgpu_gba_solve   replaces the ceres::Solve of GlobalBundleAdjustment (opt_be.cpp:560-567 and,
 *                    with max_iterations = 5, the outlier round's :257-265).
 * covgpu_pgo_solve   replaces the ceres::Solve of PoseGraphOptimization (opt_be.cpp:1024-1031):
 *                    poses + between factors only (num_lm = num_obs = num_imu = 0).
 * Both upload `p`, run the trust-region loop fully on the device, and write the optimised
 * kf_pose / kf_speed_bias / lm_pos back into the caller's arrays.                               */
int covgpu_gba_solve(covgpu_context* ctx, const covgpu_options* opt, covgpu_problem* p, covgpu_result* out);
int covgpu_pgo_solve(covgpu_context* ctx, const covgpu_options* opt, covgpu_problem* p, covgpu_result* out);

/* Split form used by bench.py so that inputs are HBM-resident before the timed region:
 * upload once, solve (restarts from the uploaded initial estimate every call), download. */
int covgpu_upload(covgpu_context* ctx, const covgpu_options* opt, const covgpu_problem* p);
int covgpu_upload_pgo(covgpu_context* ctx, const covgpu_options* opt, const covgpu_problem* p);
int covgpu_solve_resident(covgpu_context* ctx, const covgpu_options* opt, covgpu_result* out);
int covgpu_download(covgpu_context* ctx, covgpu_problem* p);

/* GBA outlier rule (opt_be.cpp:270-290): evaluates every reprojection block at the current
 * host estimate in `p` and writes the loss-corrected whitened residual norm per observation. */
int covgpu_reprojection_residual_norms(covgpu_context* ctx, const covgpu_options* opt,
                                       const covgpu_problem* p, double* norms /* [O] */);

/* Map maintenance of the outlier round on the device: the erase decisions of opt_be.cpp:276-289
 * and the bookkeeping Map::Clean / RemoveLandmarkOutliers needs (map_be.cpp:448-454, 698-743), evaluated at the estimate
 * RESIDENT on the device after covgpu_gba_solve / covgpu_solve_resident — no second upload, no O doubles over PCIe.
 *   obs_erase[o] = 1 iff the loss-corrected whitened residual norm of observation o exceeds `threshold`
 *                  (kf->EraseLandmark + lm->EraseObservation in the reference)
 *   lm_left[l]   = observations landmark l keeps; < 2 -> RemoveLandmarkOutliers drops it
 *   counts[0..1] = erased observations, landmarks left with fewer than two                                   */
int covgpu_outlier_pass(covgpu_context* ctx, double threshold, uint8_t* obs_erase /* [O] */, int32_t* lm_left /* [L] */,
                        int64_t* counts /* [2] or NULL */);

/* Both rounds of Optimization::GlobalBundleAdjustment (optimization_be.cpp:56-618) behind ONE call: the outlier round (:62-265,
 * max_num_iterations = 5, loop edges without loss), the erase decisions (:270-290), and the main round (:296-567) on the problem the
 * reference REBUILDS from the map after erasing — here derived on the device from the resident first round: the observation stream
 * minus the erased observations, minus the landmarks left with fewer than two (:428-440), the loop edges' loss switched on (:555),
 * optionally more constant poses (:338-341); restarted from the same initial estimate (the outlier round's is discarded, as in the
 * reference). One Map -> IR flatten and one upload per call instead of two.
 *   p            the FIRST round's problem (edge_loss_a as the first round wants it: 0). On return kf_pose / kf_speed_bias hold
 *                the second round's estimate, lm_pos[l] the second round's for every landmark with lm_left[l] >= 2
 *   opt          options of the second round (max_iterations = opt.gba_iteration_limit)
 *   obs_erase, lm_left, counts   as covgpu_outlier_pass, for the caller's map bookkeeping (kf->EraseLandmark, lm->EraseObservation)
 *   round1, round2 (may be NULL)  the two trust-region records; round2->t_upload_s = seconds of the device-side rebuild
 * Afterwards the context holds NO resident problem (what is resident is the second round's compacted problem, which `p` does not
 * describe): covgpu_solve_resident / covgpu_download / covgpu_outlier_pass need a new covgpu_upload first.                        */
typedef struct covgpu_two_round {
  double  outlier_threshold;         /* opt.th_gba_outlier_global (config_backend.yaml:121)                                  */
  int32_t round1_iterations;         /* 5 (optimization_be.cpp:262); <= 0: 5                                                 */
  int32_t use_loops_round2;          /* opt.gba_use_map_loop_constraints (:534)                                              */
  double  loop_loss_round2;          /* Cauchy scale of the loop edges in the second round: 1.0 (:555)                       */
  const uint8_t* kf_fixed_round2;    /* [num_kf] constant poses of the second round (opt.gba_fix_poses_loaded_maps, :338-341) or NULL: as round 1 */
} covgpu_two_round;
int covgpu_gba_two_round(covgpu_context* ctx, const covgpu_options* opt, covgpu_problem* p, const covgpu_two_round* tr,
                         uint8_t* obs_erase /* [O] */, int32_t* lm_left /* [L] */, int64_t* counts /* [2] or NULL */,
                         covgpu_result* round1, covgpu_result* round2);

/* Covisibility recount on the resident problem (Keyframe::UpdateCovisibilityConnections, keyframe_be.cpp:559-608; run over all
 * keyframes after a GBA, backend.cpp:164-167): weight(i, j) = number of landmarks both keyframes observe.
 * Pairs with weight >= threshold (sys.covis_thres) are returned as kf_i > kf_j, sorted by (kf_i, kf_j); constant keyframes
 * take part. *count = pairs found (call again with a larger capacity if it exceeds it). Counted on the device (k_pairs.hip). */
int covgpu_covisibility(covgpu_context* ctx, int32_t threshold, int64_t capacity, int32_t* kf_i, int32_t* kf_j, int32_t* weight,
                        int64_t* count);

/* Batched Optimization::OptimizeRelativePose (optimization_be.cpp:620-831): refines the relative pose
 * T_AB of MANY keyframe pairs (loop candidates, placerec_be.cpp:116-165) in one launch, one wavefront per pair. Per
 * correspondence two reprojection residuals — kNormal: pi_A(R_AB P_B + t_AB) vs kp_A, kInverse: pi_B(R_AB^T (P_A - t_AB))
 * vs kp_B — with sigma = (octave + 1) * 2 and Cauchy(1); DOGLEG 5 iterations, correspondences whose loss-corrected residual
 * norm exceeds th_outlier in either image are dropped, fewer than min_inliers (reference: 12) left -> inliers = 0 and T_ab
 * untouched, else 5 more iterations. NB with Cauchy(1) the corrected norm is < 1, so the reference's configured
 * opt.th_outlier_align = 1.3 never removes anything; that behaviour is reproduced as is.
 * Pairs b = 0..num-1 own correspondences [corr_ptr[b], corr_ptr[b+1]). cam_* rows: fx fy cx cy d0 d1 d2 d3. All HOST pointers.
 * cam_model_a / _b (appended fields, NULL = pinhole) and xi_a / _b select the projection per side as covgpu_problem's cam_model / cam_xi. */
typedef struct covgpu_relpose_batch_t {
  int32_t num_pairs;
  const int32_t* corr_ptr;      /* [num_pairs + 1] */
  const double*  p_b;           /* [C][3] landmark of kf2 in camera-B frame (opt_be.cpp:655-656) */
  const double*  p_a;           /* [C][3] landmark of kf1 in camera-A frame (:653-654)           */
  const double*  kp_a;          /* [C][2] */
  const double*  kp_b;          /* [C][2] */
  const double*  sigma_a;       /* [C]    */
  const double*  sigma_b;       /* [C]    */
  const double*  cam_a;         /* [num_pairs][8] */
  const double*  cam_b;         /* [num_pairs][8] */
  const int32_t* dist_type_a;   /* [num_pairs] COVGPU_DIST_* */
  const int32_t* dist_type_b;   /* [num_pairs] */
  double*        T_ab;          /* [num_pairs][7] in/out */
  uint8_t*       outlier;       /* [C] out: 1 = correspondence removed (matches1[i] = NULL, :807) */
  int32_t*       inliers;       /* [num_pairs] out: the function's return value per pair */
  const int32_t* cam_model_a;   /* [num_pairs] COVGPU_CAM_* or NULL (pinhole) */
  const int32_t* cam_model_b;   /* [num_pairs] or NULL */
  const double*  xi_a;          /* [num_pairs] read for unified rows */
  const double*  xi_b;          /* [num_pairs] */
} covgpu_relpose_batch_t;
int covgpu_relpose_batch(covgpu_context* ctx, const covgpu_relpose_batch_t* batch, double th_outlier, int32_t min_inliers);

/* PGO tail (opt_be.cpp:1046-1047, 1066-1081): rotate velocities and re-anchor every landmark to
 * its reference keyframe: p' = T_ws_new(ref) * T_ws_old(ref)^-1 * p.  ref_kf[l] < 0 skips l. */
int covgpu_pgo_reanchor(covgpu_context* ctx, int32_t num_kf, const double* pose_old /* [K][7] */,
                        const double* pose_new /* [K][7] */, double* velocity /* [K][3] or NULL */,
                        int32_t num_lm, const int32_t* ref_kf /* [L] */, double* lm_pos /* [L][3] */);

/* ---------------------------------------------------------------- per-kernel test entry points
 * (SURVEY.md §8b last row). Each runs exactly one device kernel family on host inputs and returns
 * raw, un-reduced outputs so tests/ can compare them with the oracle.                           */

/* R4+R5+R6: per observation r[2], J_pose[2x6], J_lm[2x3] (whitened, loss-corrected), cost rho/2. */
int covgpu_linearize_reprojection(covgpu_context* ctx, const covgpu_options* opt, const covgpu_problem* p,
                                  double* r /* [O][2] */, double* J_pose /* [O][12] */,
                                  double* J_lm /* [O][6] */, double* cost /* [O] */);

/* R2: per IMU factor delta [dp(3), dq(4), dv(3), dt_sum] (11), bias Jacobian J[15x15],
 * covariance P[15x15], preintegrated at the linearisation bias = speed_bias[kf_j][3:9]. */
int covgpu_preintegrate(covgpu_context* ctx, const covgpu_options* opt, const covgpu_problem* p,
                        double* delta /* [I][11] */, double* J /* [I][225] */, double* P /* [I][225] */);

/* R3: per IMU factor whitened residual r[15] and Jacobians w.r.t. [pose_i(6), sb_i(9), pose_j(6),
 * sb_j(9)] as one row-major 15x30 block. */
int covgpu_linearize_imu(covgpu_context* ctx, const covgpu_options* opt, const covgpu_problem* p,
                         double* r /* [I][15] */, double* J /* [I][450] */);

/* R7: per edge residual r[6] and row-major 6x12 Jacobian w.r.t. [pose_i(6), pose_j(6)]
 * (whitened by sqrt_info, loss-corrected), cost. */
int covgpu_linearize_between(covgpu_context* ctx, const covgpu_options* opt, const covgpu_problem* p,
                             double* r /* [E][6] */, double* J /* [E][72] */, double* cost /* [E] */);

/* R8 building block: damped Schur complement at the current estimate.
 * Outputs the dense reduced system S (n x n, row-major, full symmetric) and b (n),
 * n = dim_per_kf * K with dim_per_kf = 15 (VI) or 6 (visual_only / PGO), plus total cost. */
int covgpu_schur(covgpu_context* ctx, const covgpu_options* opt, const covgpu_problem* p, double mu,
                 double* S, double* b, double* cost);
/* same for the pose-graph problem (edges only, 6 rows per keyframe) */
int covgpu_schur_pgo(covgpu_context* ctx, const covgpu_options* opt, const covgpu_problem* p, double mu,
                     double* S, double* b, double* cost);

/* R8 building block: ONE damped Gauss-Newton step at the estimate in `p`, through the product solve path (speed-bias
 * multifrontal MFMA Cholesky of the reduced camera system over its elimination tree -> landmark back-substitution):
 * dx[n] (IR layout, dim_per_kf per keyframe) and dl[3L]. Tests check S dx = b against the oracle's system at full size. */
int covgpu_gn_step(covgpu_context* ctx, const covgpu_options* opt, const covgpu_problem* p, double mu,
                   double* dx /* [n] */, double* dl /* [L][3] */, double* cost);

/* R8 building block: dense FP64 Cholesky solve of S x = b on the MFMA path (S symmetric positive
 * definite, row-major n x n; only the lower triangle is read). Returns COVGPU_ERR_NUMERIC if a
 * pivot is not positive. */
int covgpu_solve_reduced(covgpu_context* ctx, int32_t n, const double* S, const double* b, double* x);

int32_t covgpu_reduced_dim(const covgpu_options* opt, const covgpu_problem* p);

/* ---- test entry points of the trust-region tail (k_tail.hip and its COVGPU_TAIL=0 predecessor in k_dense.hip) ----
 * covgpu_solve_resident that also copies the trust-region state the host reads at the end of EVERY iteration (COVGPU_TR_COUNT doubles, the
 * TR_* slots of csrc/common.hpp; rounds repeated with a raised damping included) into trace[k][COVGPU_TR_COUNT], k < capacity. *count = rounds
 * the solve ran (it may exceed capacity: the rounds beyond it are not stored). */
#define COVGPU_TR_COUNT 32
#define COVGPU_SC_COUNT 16
int covgpu_solve_resident_traced(covgpu_context* ctx, const covgpu_options* opt, covgpu_result* out, double* trace, int32_t capacity,
                                 int32_t* count);
/* What the last iteration of the last solve left on the device: gradient, diag(J^T J), the Gauss-Newton (LM) step and the scaled gradient
 * c = g / d^2 (fused tail and dogleg only), each [N = dim_per_kf K + 3 L], and the candidate estimate. NULL outputs are skipped. */
int covgpu_fetch_tail_state(covgpu_context* ctx, double* grad, double* hdiag, double* gn, double* vtmp, double* pose_c /* [K][7] */,
                            double* sb_c /* [K][9] */, double* lm_c /* [L][3] */);
/* One launch of the step logic on prescribed inputs; needs no uploaded problem. tr[COVGPU_TR_COUNT] and scal[COVGPU_SC_COUNT] are read and
 * written back; flag0 is the factorisation's failure flag; the options give strategy, max_radius and the tolerances. kernel:
 *   0 k_tail_logic(stage, fresh)
 *   1 k_tail_finish(stage, with_logic, fresh) on part[COVGPU_SC_COUNT][part_n]: fixed-order sums of the stage's slots into scal, and, with_logic
 *     != 0, stage A (stage 1) or B (stage 2) of the step logic in the workgroup that finishes last
 *   2 k_tr_after_solve(fresh)   3 k_tr_after_model   4 k_tr_decide     (the COVGPU_TAIL=0 form) */
int covgpu_tail_logic_probe(covgpu_context* ctx, const covgpu_options* opt, int32_t kernel, int32_t stage, int32_t with_logic, int32_t fresh,
                            int32_t flag0, double* tr, double* scal, const double* part, int32_t part_n);

/* Host-only: lanes per landmark (4 | 8 | 16) of the landmark-major kernels k_lm_lin, k_lm_backsub and k_lm_outliers for a problem of
 * num_obs observations on num_lm landmarks — the rule covgpu_upload applies: mean track length O/L <= 5 -> 4, <= 8 -> 8, else 16
 * (no landmarks: 4). DESIGN.md 4.1. */
int32_t covgpu_lm_group(int64_t num_obs, int32_t num_lm);

/* Host-only: the block partition of round 2's block-arrow pose-graph solve (PoseGraphOptimization's linear solver,
 * optimization_be.cpp:1024-1031; since round 6 the default is the multifrontal solve on the pose graph's own elimination
 * tree — DESIGN.md 4.8 — and this scheme runs with COVGPU_PGO_ND=0). block_of_kf[k] = block index (>= 0) of
 * keyframe k, or -1 if it belongs to the border (loop-closure keyframes and separators). Returns the number of
 * blocks, or 0 if the graph is solved densely (too small, no split, or a border that is a large part of the
 * system; block_of_kf is then all -1). No edge joins two different blocks. Needs no device. */
int32_t covgpu_pgo_partition(int32_t num_kf, int32_t num_edge, const int32_t* edge_i, const int32_t* edge_j, int32_t* block_of_kf);

/* Host-only (no device needed): the nested-dissection plan of the reduced camera system — the elimination tree the
 * multifrontal MFMA Cholesky (covins_amd/csrc/k_front.hip) runs, i.e. what the reference gets from CHOLMOD's fill-reducing
 * ordering inside ceres::Solve(SPARSE_SCHUR) (optimization_be.cpp:560-565). Unknowns are, per keyframe, a 6-dim pose block
 * (variable 2k) and a 9-dim speed-bias block (variable 2k+1, visual-inertial only). Every tree node owns some variables
 * (eliminated there) and carries the ancestor variables its subtree couples to; nodes of equal height form one batch.
 * leaf_dims <= 0: default (COVGPU_ND_LEAF or 600 scalar unknowns per leaf). tests/test_nd_plan.py replays the plan in numpy. */
typedef struct covgpu_nd_plan covgpu_nd_plan;
int  covgpu_nd_plan_create(const covgpu_options* opt, const covgpu_problem* p, int32_t leaf_dims, covgpu_nd_plan** out);
/* the same for a pose-graph problem (edges only): the plan covgpu_pgo_solve runs on since round 6 — 6-dof blocks, an agent's time axis read from the
 * edge graph (connected components of the graph without its bridges, each in breadth-first order: plan_api.hip build_chains_pgo) */
int  covgpu_nd_plan_create_pgo(const covgpu_options* opt, const covgpu_problem* p, int32_t leaf_dims, covgpu_nd_plan** out);
void covgpu_nd_plan_destroy(covgpu_nd_plan* plan);
/* out16 = { nodes, levels, depth, own entries, front-structure entries, front elements over all batches, flops of the partial
 *           factorisations, largest own dims, largest border dims, largest root, candidate tree (top mode, leaf, 100 x group balance),
 *           shard policy of the plan (0 replicated top | 1 distributed top), 0, 0 } */
void covgpu_nd_plan_info(const covgpu_nd_plan* plan, int64_t* out16);
/* parent / level [nodes]; own_ptr / st_ptr [nodes + 1]; own_var / st_var: 2 * keyframe + (0 pose | 1 speed-bias) */
void covgpu_nd_plan_arrays(const covgpu_nd_plan* plan, int32_t* parent, int32_t* level, int32_t* own_ptr, int32_t* own_var,
                           int32_t* st_ptr, int32_t* st_var);

/* ---------------------------------------------------------------- multi-GPU: ONE map sharded by sub-map
 * BASELINE.json north star: "the merged multi-agent map shards by agent/sub-map across the GPUs of one node with RCCL
 * all-reduce over xGMI on the shared-pose Hessian blocks at each LM iteration". One context per GPU (one process per GPU, or
 * several contexts in one process). The unit of the split is a SUBTREE of the elimination tree (an agent, or a stretch of an
 * agent's trajectory); the top of the tree — the separators that join the sub-maps: the "shared" poses — is replicated.
 *   1. every rank calls covgpu_shard_plan on the FULL problem (host-only, deterministic: the same answer everywhere);
 *   2. rank r keeps the landmarks / IMU factors / between factors with *_rank == r (all keyframes stay: K is unchanged),
 *      attaches a collective (covgpu_set_shard_rccl: RCCL, unique id from covgpu_rccl_unique_id on rank 0 passed to the
 *      others by the caller; covgpu_set_shard_group: host threads of one process whose contexts share a device), then
 *      covgpu_upload / covgpu_solve_resident / covgpu_download on that sub-problem;
 *   3. per trust-region iteration the library issues FOUR all-reduces, all enqueued on the context's stream (no host
 *      synchronisation): inside the linear solve ONE over [top fronts | their right-hand sides | gradient and diag(J^T J) of
 *      the top unknowns] after every rank has eliminated its own subtrees, and three of 16 + 2 x world scalars;
 *      shard_policy 1 (distributed top, opt-in): the top is every node whose front order reaches 4 096 plus its ancestors;
 *      its fronts stay SUMS over the ranks' copies — one all-reduce of gradient and diag(J^T J) of the top unknowns, then one
 *      per 256-column panel of the top (the panel's column block and right-hand-side rows), which every rank factorises
 *      redundantly, while each rank applies the trailing update to the tile rows it owns only ((tile row + node) mod world);
 *   4. after the solve an unknown is valid on the rank that owns its tree node (covgpu_nd_plan_owner; top unknowns: on
 *      every rank), a landmark on its lm_rank. */
int32_t covgpu_shard_plan(const covgpu_options* opt, const covgpu_problem* p, int32_t world, covgpu_nd_plan** plan_out,
                          int32_t* lm_rank /* [L] */, int32_t* imu_rank /* [I] */, int32_t* edge_rank /* [E] */);  /* returns the number of subtrees, 0: no split */
void covgpu_nd_plan_owner(const covgpu_nd_plan* plan, int32_t* pose_rank /* [K] */, int32_t* sb_rank /* [K] */);   /* -1: top unknown */
void covgpu_nd_plan_ranks(const covgpu_nd_plan* plan, int32_t* node_rank /* [nodes] */);                          /* -1: top node */
/* host-only accounting of a shard plan under its policy: out[world] = flops of one factorisation on every rank (its subtrees + the top:
 * whole on every rank under policy 0; the redundant panel chain + the trailing-update tiles the rank owns under policy 1). Returns world. */
int32_t covgpu_nd_plan_rank_flops(const covgpu_nd_plan* plan, double* out);
/* out4 = { bytes all-reduced per linear solve and rank, collectives per linear solve, world, shard policy } (host estimate on the real front sizes) */
void covgpu_nd_plan_exchange(const covgpu_nd_plan* plan, int64_t* out4);
typedef struct covgpu_group covgpu_group;   /* in-process group of ranks (host threads), at most 16 */
int  covgpu_group_create(int32_t world, covgpu_group** out);
void covgpu_group_destroy(covgpu_group* g);
void covgpu_group_abort(covgpu_group* g);   /* a failing member releases the others from their barrier */
int  covgpu_set_shard_group(covgpu_context* ctx, const covgpu_nd_plan* plan, int32_t rank, covgpu_group* g);
int  covgpu_rccl_unique_id(uint8_t* out128);   /* ncclGetUniqueId; librccl is loaded on first use */
int  covgpu_set_shard_rccl(covgpu_context* ctx, const covgpu_nd_plan* plan, int32_t rank, int32_t world, const uint8_t* id128);
int  covgpu_set_shard_none(covgpu_context* ctx);   /* back to the single-GPU form */
/* The whole sharded solve behind one call, for a host process that drives several GPUs itself (covins_backend is one
 * process: backend.cpp:141-156): plan on the full problem, one context + one host thread per rank on devices[r], RCCL
 * between them (the in-process group if ranks share a device: virtual ranks), results merged into `p`; `out` = the common
 * trust-region record. obs_erase != NULL: also the outlier decisions of optimization_be.cpp:270-290 at the resident
 * estimate, merged over the ranks (obs_erase [O], lm_left [L], counts[2] as covgpu_outlier_pass). */
int  covgpu_gba_solve_multi(const covgpu_options* opt, covgpu_problem* p, covgpu_result* out, int32_t n_ranks, const int32_t* devices,
                            double outlier_threshold, uint8_t* obs_erase, int32_t* lm_left, int64_t* counts);
/* Both rounds of a GlobalBundleAdjustment call (optimization_be.cpp:56-618) on n_ranks devices behind one call (round 6): the plan on the full problem, ONE
 * upload per rank, the second round derived on every rank's device from its own share exactly as covgpu_gba_two_round derives it on one GPU (a
 * landmark's outlier decisions, the compaction and the pair lists are local to its rank; the elimination tree stays); obs_erase [O], lm_left [L],
 * counts[2] and the second round's estimate merged into `p` as covgpu_gba_solve_multi merges them. */
int  covgpu_gba_two_round_multi(const covgpu_options* opt, covgpu_problem* p, const covgpu_two_round* tr, int32_t n_ranks, const int32_t* devices,
                                uint8_t* obs_erase, int32_t* lm_left, int64_t* counts, covgpu_result* round1, covgpu_result* round2);
int  covgpu_allreduce_host(covgpu_context* ctx, double* host, int64_t n, int32_t op /* 0 sum, 1 max */);  /* through the context's collective */
void covgpu_shard_stats(covgpu_context* ctx, int64_t* out4);  /* collectives issued, bytes all-reduced, rank, world */

/* ---------------------------------------------------------------- measurement hooks (bench.py)
 * With profiling on, covgpu_solve_resident brackets the linearise+Schur pass, the whole factor+solve and
 * every trailing-update (SYRK) launch with HIP events on the context's own stream.
 * out[8] = { build ms, #builds, factor+solve ms, #factorisations, SYRK ms, #SYRK launches, SYRK flops,
 *           #off-diagonal 6x6 pose-pose blocks of the reduced system (covisible + loop-edge keyframe pairs) } */
void covgpu_set_profiling(covgpu_context* ctx, int on);
/* layout of the uploaded problem: out[16] = { ranks of a sharded solve (0: single GPU), this rank, scalar unknowns of the
 * replicated top nodes, top levels, KiB all-reduced per linear solve, how the context orders its streams (1 device flags, 0 HIP events
 * by COVGPU_GATES=0, -1 events and the launch-per-tile backward substitution after a flag gate or a hand-over inside the pipelined
 * backward substitution timed out), dense pose order (padded), covisible keyframe pairs,
 * edge pairs, IMU chains, device MiB allocated for the problem (from the allocator, not by hand), fronts, levels, serial
 * 256-column panels, order of the last level's fronts, MiB of fronts } */
void covgpu_get_layout(covgpu_context* ctx, int64_t* out16);
void covgpu_get_profile(covgpu_context* ctx, double* out8);
/* out16: [0..7] as covgpu_get_profile; [8] k_potrf_panel (the serial panel chain of the front factorisation) milliseconds summed over
 * its launches, [9] its launches, [10] its algorithmic flops (per front n^3/3 + n^2 on the front's real columns in the panel),
 * [11] flops of one multifrontal factorisation of the resident problem (dense count on the fronts' real sizes), [12..15] 0 */
void covgpu_get_profile2(covgpu_context* ctx, double* out16);
/* Census of kernel forms: which of the shape-dependent launch forms of the linear solve (multifrontal GBA solve, pose-graph solve,
 * covgpu_solve_reduced) this context has issued since its last upload. Host-side integers counted where the launches are issued: nothing is
 * added to the device work. out[i], i < min(n, return value), = count of form i; the return value is the number of forms; the name of form i
 * is covgpu_kernel_form_name(i) (NULL outside the range). A count is a number of LAUNCHES unless its line says otherwise. The forms, in order:
 *
 *   FORMS-BEGIN
 *   k_potrf_panel          panel factorisation, sixteen waves per front
 *   k_potrf_panel.fronts   ... fronts (workgroups) over those launches
 *   k_potrf_panel4         panel factorisation, four waves per front (more than 384 fronts of a level with 1..128 real columns in the panel)
 *   k_potrf_panel4.fronts  ... fronts over those launches
 *   potrf_skipped          panels not launched at all: identity padding in every front of the batch
 *   k_trsm_sub4<4>         substitution below a panel of <= 4 real 16-column blocks
 *   k_trsm_sub4<8>         ... 5..8
 *   k_trsm_sub4<12>        ... 9..12
 *   k_trsm_sub4<16>        ... 13..16
 *   k_gemm_abt.tri         trailing update of a tile list as full 128x128 tiles
 *   k_gemm_abt_q.tri       trailing update of a tile list as 64x64 quadrants (lists up to 1024 entries)
 *   k_gemm_abt.tri_grid    trailing update as the implicit triangle grid (batches without live-tile lists: dense solve)
 *   k_gemm_abt.rect        look-ahead update of the next panel's rows as full tiles
 *   k_gemm_abt_q.rect      ... as quadrants (rows h; rest rows up to 512 tiles; the next diagonal block of a one-matrix solve)
 *   k_diag_update          look-ahead update of the next panel's diagonal block of the fronts of a tree: 32x32 sub-blocks, K in one latency
 *   bulk_one_launch        bulk updates (not a front's last) issued as one launch
 *   bulk_two_launches      ... as two: the next-but-one panel's two tile columns first
 *   last_update_whole      a batch's last trailing update issued whole on the chain's stream
 *   last_update_split      ... split for the look-ahead into the next level (split_ta)
 *   panel_one_tile         panels one tile wide (odd tile count)
 *   kd_cut                 panels whose rank update runs a K range cut below the panel's width (the level's largest real interior order)
 *   kd_zero                panels whose rank update is skipped: no real column in the panel
 *   gemm_beta0             first-panel trailing updates given a map of border tiles that start from zero
 *   k_bwd_front            backward substitution of a level, fronts of 1..4 interior tiles, one launch
 *   k_bwd_pipe             backward substitution of a level as a pipeline of tile workgroups
 *   k_bwd_pipe64           ... its form with 64x64 inverses (at most 128 tile workgroups)
 *   k_bwd_tree             bottom levels' backward substitution in one launch
 *   k_bwd_tree64           top levels' backward substitution in one launch
 *   k_bwd_given            backward substitution per tile: the given rows
 *   k_bwd_step_sub         backward substitution per tile: one interior tile
 *   k_nd_extend_rec        extend-add from packed records
 *   k_nd_extend            extend-add from index tables (COVGPU_EXT_RECORDS=0)
 *   nd_extend_split        extend-add launches that carry one half of a level split for the look-ahead
 *   k_nd_top_pack          sharded solve: top fronts packed / unpacked around the all-reduce
 *   k_nd_gh                sharded solve: gradient and diagonal of the top unknowns gathered / scattered
 *   k_nd_top_damp          sharded solve: damping of the top unknowns
 *   k_nd_panel_xfer        sharded solve, distributed top: a panel's exchange packed / unpacked
 *   dist_panel             sharded solve, distributed top: panels factored by dense_cholesky_dist
 *   pgo_arrow              pose-graph solves by the block-arrow elimination
 *   pgo_dense              pose-graph solves by one dense factorisation
 *   k_potrf_leaf           FRONTS of a bottom level of speed-bias leaf fronts factored whole, one launch per solve (also under k_potrf_panel / .fronts)
 *   FORMS-END */
int  covgpu_get_kernel_forms(covgpu_context* ctx, int64_t* out, int32_t n);
const char* covgpu_kernel_form_name(int32_t i);


/* ---------------------------------------------------------------- loop-candidate geometric verification
 * Batched Se3Solver::projectiveAlignment (Se3Solver.cpp:59-110): per candidate b an opengv-style RANSAC (GP3P with one camera at zero
 * offset = central P3P, 4th correspondence picks the solution) over the correspondences [corr_ptr[b], corr_ptr[b+1]):
 * unit bearing f_i in the query camera, world point P_i, sigma_angle_i = sqrt(2) s^2 / fu^2 with s = 0.8 (octave + 1), fu = (fx + fy) / 2.
 * Score ||normalize(R^T (P_i - t)) - f_i||^2 / sigma_angle_i, inlier iff score < threshold. Draw d, slot k uses
 * splitmix64(seed_b + 4 d + k) in a partial Fisher-Yates over [0, n). One workgroup per candidate, one launch per call.
 * max_iterations must lie in 1..100000 (a candidate makes at most 11 max_iterations + 1 draws). */
typedef struct covgpu_abspose_batch_t {
  int32_t num;              const int32_t* corr_ptr;     /* [num+1] */
  const double* bearing;    /* [C][3] */   const double* point_w; /* [C][3] */   const double* sigma_angle; /* [C] */
  const uint64_t* seed;     /* [num] or NULL = opts seed + b */
  double*  T_wc;            /* [num][7] out, qx qy qz qw x y z; untouched when inliers[b] == 0 */
  uint8_t* inlier;          /* [C] out */
  int32_t* inliers;         /* [num] out: inlier count, 0 = no transform found */
  int32_t* iterations;      /* [num] out or NULL */
  int32_t* best_draw;       /* [num] out or NULL: draw index of the model (for parity tests) */
} covgpu_abspose_batch_t;
typedef struct { int32_t min_inliers; int32_t max_iterations; double probability; double threshold; uint64_t seed; } covgpu_ransac_opts;
void covgpu_default_ransac_opts(covgpu_ransac_opts*);   /* 6, 300, 0.99, 25.0, 0 (config_backend.yaml:85-88) */
int  covgpu_abspose_ransac_batch(covgpu_context*, const covgpu_abspose_batch_t*, const covgpu_ransac_opts*);
/* test entry point: the P3P of every quadruple on its first three correspondences, all solutions (ascending v = s3/s1), and the one the
 * 4th correspondence picks (-1: none) */
int  covgpu_p3p_batch(covgpu_context*, int32_t n, const double* f /*[n][4][3]*/, const double* P /*[n][4][3]*/,
                      double* T /*[n][4][7]*/, int32_t* nsol /*[n]*/, int32_t* chosen /*[n]*/);


/* ---------------------------------------------------------------- COVINS-G five-point relative-pose RANSAC
 * Batched RelNonCentralPosSolver::computePose (RelNonCentralPosSolver.cpp:343-377): per job b an opengv-style RANSAC (central
 * relative pose, five-point solver on slots 0..4 of a draw of 8, all 8 pick the pose) over the correspondences
 * [corr_ptr[b], corr_ptr[b+1]): unit bearings f1_i (frame 1, the query side) and f2_i (frame 2). Model T_12 = [R | t], frame 2 in
 * frame 1 (x1 = R x2 + t, ||t|| = 1). Score: the midpoint p of the two rays (triangulate2), r1 = p/||p||, r2 = q/||q|| with
 * q = R^T p - R^T t, score = 0.5 ||r1 - f1||^2 / sigma + 0.5 ||r2 - f2||^2 / sigma, inlier iff score < threshold. Among the up to 40
 * poses of a draw the smallest sum over its 8 correspondences of (1 - f1.r1) + (1 - f2.r2) wins, the first on a tie. Draw d, slot k
 * uses splitmix64(seed_b + 8 d + k) in a partial Fisher-Yates over [0, n). The loop is §4.10's with sample size 8. One workgroup
 * per job, one launch per call; a job's result does not depend on its batch. max_iterations must lie in 1..100000 (a job makes at
 * most 11 max_iterations + 1 draws). All arguments are checked on the host before any device work (covgpu_fivept_check is that check
 * alone); it reads every bearing once, and a non-finite bearing refuses the whole batch. */
typedef struct covgpu_fivept_batch_t {
  int32_t num;              const int32_t* corr_ptr;     /* [num+1] */
  const double* bearing1;   /* [C][3] */   const double* bearing2; /* [C][3] */
  const uint64_t* seed;     /* [num] or NULL = opts seed + b */
  double*  T_12;            /* [num][7] out, qx qy qz qw x y z; untouched unless status[b] == 0 */
  uint8_t* inlier;          /* [C] out: all 0 unless status[b] == 0 */
  int32_t* inliers;         /* [num] out: the best model's inlier count, whatever the status */
  int32_t* status;          /* [num] out: COVGPU_FIVEPT_* */
  int32_t* iterations;      /* [num] out or NULL */
  int32_t* best_draw;       /* [num] out or NULL: draw index of the model (for parity tests) */
} covgpu_fivept_batch_t;
#define COVGPU_FIVEPT_FOUND 0
#define COVGPU_FIVEPT_TOO_FEW 1        /* n < 8 */
#define COVGPU_FIVEPT_NO_MODEL 2       /* every draw failed */
#define COVGPU_FIVEPT_FEW_INLIERS 3    /* fewer than min_inliers */
#define COVGPU_FIVEPT_MAX_ITERATIONS 4 /* iterations >= max_iterations (RelNonCentralPosSolver.cpp:368-369) */
typedef struct { int32_t min_inliers; int32_t max_iterations; double probability; double threshold; double sigma; uint64_t seed; } covgpu_fivept_opts;
void covgpu_default_fivept_opts(covgpu_fivept_opts*);   /* 20, 200, 0.99, 16.0, 4.5e-6, 0 (config_backend.yaml:100-102) */
/* out[0] correspondences staged in LDS (longer jobs read global memory), out[1] hypotheses per pass, out[2] the sample size,
 * out[3] the largest max_iterations */
void covgpu_fivept_limits(int32_t out[4]);
/* the argument check of covgpu_fivept_ransac_batch alone; needs no context and no device */
int  covgpu_fivept_check(const covgpu_fivept_batch_t*, const covgpu_fivept_opts*);
int  covgpu_fivept_ransac_batch(covgpu_context*, const covgpu_fivept_batch_t*, const covgpu_fivept_opts*);
/* test entry point: the five-point problem of every 8-tuple on its slots 0..4: every real E (||E||_F = sqrt 2, the largest-magnitude
 * entry positive, row-major, order unspecified; rows past nsol are zero), the pose that the 8 points pick (untouched if none) and the
 * index of its E (-1: none) */
int  covgpu_fivept_solve_batch(covgpu_context*, int32_t n, const double* f1 /*[n][8][3]*/, const double* f2 /*[n][8][3]*/,
                               double* E /*[n][10][9]*/, int32_t* nsol /*[n]*/, double* T /*[n][7]*/, int32_t* chosen /*[n]*/);


/* ---------------------------------------------------------------- COVINS-G 17-point stage and loop covariance
 * Batched back half of RelNonCentralPosSolver::computeNonCentralRelPose (RelNonCentralPosSolver.cpp:149-301): per job b the
 * non-central 17-point RANSAC over the correspondences [corr_ptr[b], corr_ptr[b+1]) of all cells, the non-linear polish of its
 * model on its inliers, and the sampled 6x6 covariance of the loop edge in the IMU frames. Correspondence i has unit bearings f1_i,
 * f2_i and cameras cam1_i, cam2_i, indices into the job's camera table [cam_ptr[b], cam_ptr[b+1]) of (R_c row-major [9], o_c [3]),
 * the camera in its viewpoint (viewpoint 1 the query keyframe, 2 the candidate): ray direction g = R_c f, origin o_c. The cells of
 * a job are the ranges [cell_ptr[b][j], cell_ptr[b][j+1]) relative to the job, cell_ptr[b][0] = 0, cell_ptr[b][cells] = n_b.
 * Model T_12 = [R | t], x1 = R x2 + t, metric t. Draw d, slot k of the RANSAC uses splitmix64(seed_b + 17 d + k) in a partial
 * Fisher-Yates over [0, n); covariance draw e, cell j, slot k uses splitmix64(seed_b' + (e cells + j) 4 + k) over the cell's
 * ascending inlier list, seed_b' = splitmix64(seed_b ^ 0x17C0F17C0F17C0F1). T_s1s2 = T_sc_q T_c1c2 T_sc_c^-1. One workgroup per
 * job, one launch per call; a job's result does not depend on its batch. Outputs up to the failing stage are written, later ones
 * are untouched. All arguments are checked on the host before any device work (covgpu_ncrelpose_check is that check alone). */
typedef struct covgpu_ncrelpose_batch_t {
  int32_t num;              int32_t cells;               /* cells per job, 1..16 (the reference has 6, query-major) */
  const int32_t* corr_ptr;  /* [num+1] */  const int32_t* cell_ptr; /* [num][cells+1] */
  const double* bearing1;   /* [C][3] */   const double* bearing2; /* [C][3] */
  const int32_t* cam1;      /* [C] */      const int32_t* cam2;    /* [C] */
  const int32_t* cam_ptr;   /* [num+1] */  const double* cam;      /* [M][12] */
  const double* T_sc_q;     /* [num][7] qx qy qz qw x y z */       const double* T_sc_c; /* [num][7] */
  const uint64_t* seed;     /* [num] or NULL = opts seed + b */
  double*  T_c1c2;          /* [num][7] out: the polished pose; written from status 4 on and at 0 */
  double*  T_c1c2_ransac;   /* [num][7] out: the RANSAC model; written unless status is 1 or 2 */
  double*  T_s1s2;          /* [num][7] out: with T_c1c2 */
  double*  cov;             /* [num][36] out, rotation first; written at status 0 and 6 */
  uint8_t* inlier;          /* [C] out: the RANSAC model's inliers (all 0 at status 1 and 2) */
  int32_t* inliers;         /* [num] out */
  int32_t* status;          /* [num] out: COVGPU_NCRELPOSE_* */
  int32_t* iterations;      /* [num] out */
  int32_t* best_draw;       /* [num] out: draw index of the model, -1: none */
  int32_t* cov_rows;        /* [num] out: accepted covariance draws */
  int32_t* cov_draws;       /* [num] out: covariance draws made */
} covgpu_ncrelpose_batch_t;
#define COVGPU_NCRELPOSE_FOUND 0
#define COVGPU_NCRELPOSE_TOO_FEW 1        /* n < 17 */
#define COVGPU_NCRELPOSE_NO_MODEL 2       /* every draw failed */
#define COVGPU_NCRELPOSE_FEW_INLIERS 3    /* fewer than min_inliers (:165) */
#define COVGPU_NCRELPOSE_THIN_CELL 4      /* a cell with fewer than 8 inliers (:222-227) */
#define COVGPU_NCRELPOSE_COV_INCOMPLETE 5 /* the draws ran out before cov_iters rows existed */
#define COVGPU_NCRELPOSE_COV_TRACE 6      /* trace(cov) >= cov_thres (:294) */
typedef struct {
  double rp_error; double rp_error_cov; int32_t min_inliers; int32_t max_iterations; double cov_thres; int32_t cov_iters; int32_t cov_max_iters;
  double probability; uint64_t seed;
  int32_t stage_cap;        /* 0: the library's LDS staging cap; > 0: the smaller of the two (tests force the global-memory path) */
} covgpu_ncrelpose_opts;
void covgpu_default_ncrelpose_opts(covgpu_ncrelpose_opts*);   /* 1.5, 10, 100, 4000, 10, 30, 300, 0.99, 0, 0 (config_backend.yaml:91-97) */
/* out[0] correspondences staged in LDS, out[1] draws per pass, out[2] the sample size, out[3] the largest max_iterations, out[4] the
 * most cells, out[5] the largest cov_iters, out[6] the most rows of a linear solve, out[7] the step cap of the polish */
void covgpu_ncrelpose_limits(int32_t out[8]);
int  covgpu_ncrelpose_check(const covgpu_ncrelpose_batch_t*, const covgpu_ncrelpose_opts*);
int  covgpu_ncrelpose_batch(covgpu_context*, const covgpu_ncrelpose_batch_t*, const covgpu_ncrelpose_opts*);
/* test entry point: the linear solve alone on n tuples of N (17..64) ray pairs, ray = (g [3], o [3]): the pose (untouched where ok is
 * 0), whether the solve succeeded, and sigma_1, sigma_17, sigma_18 of the N x 18 system */
int  covgpu_ncrelpose_solve_batch(covgpu_context*, int32_t n, int32_t N, const double* ray1 /*[n][N][6]*/, const double* ray2 /*[n][N][6]*/,
                                  double* T /*[n][7]*/, int32_t* ok /*[n]*/, double* sv /*[n][3]*/);


/* ---------------------------------------------------------------- loop-candidate descriptor matching
 * Brute-force Hamming matching of 32-byte ORB descriptors (distance = popcount of eight 32-bit XORs, feature_matcher_be.cpp:49-64),
 * job j matching the rows of set set_a[j] (query, "A") against those of set set_b[j] (candidate, "B"). Two modes:
 *  COVGPU_MATCH_DENSE  LandmarkMatchingAlgorithm(dist_threshold) + estd2::DenseMatcher(numBest = 4, no ratio test), placerec_be.cpp:84-90.
 *    Rows with skip[r] != 0 (keypoint without a valid landmark, LandmarkMatchingAlgorithm::doSetup) take no part. Every A row keeps
 *    the 4 best (b, d) with d < dist_threshold, B rows scanned in ascending order, a row inserted iff d < list[3].d, at
 *    std::lower_bound (before equal distances; the last entry drops out). Then DenseMatcher::assignbest is replayed in the
 *    single-thread order (A rows ascending): a free B row is taken, a held one is stolen on a strictly smaller distance and the loser
 *    re-assigned from its entry 1. Every held B row is a match (a, b, d); the reference emits them in ascending b.
 *  COVGPU_MATCH_KNN2   cv::BFMatcher(NORM_HAMMING).knnMatch(k = 2) + distance test + ratio test, placerec_gen_be.cpp:82-114: the two
 *    nearest train rows by (d, index); A row a matches iff B has >= 2 rows, (float)d1 <= dist_threshold and
 *    (float)d1 < ratio * (float)d2 in float32. skip must be NULL. Matches are emitted in ascending a.
 * Outputs of job j start at row offset sum_{j' < j} rows(set_a[j']): match[] = local B row or -1, dist[] = its distance or -1;
 * nmatches[j] = the number of matches (what ComputeSE3 tests against matches_thres). Every set holds at most COVGPU_MATCH_MAX_ROWS
 * rows, and num_jobs * ceil(max rows(set_a[j]) / 256) may not exceed 2^31 - 1. All arguments (the context included) are checked
 * before any device work; zero jobs and empty sets are valid. */
#define COVGPU_MATCH_DENSE 0
#define COVGPU_MATCH_KNN2 1
#define COVGPU_MATCH_MAX_ROWS 4096
typedef struct covgpu_match_batch_t {
  int32_t num_sets;         const int32_t* row_ptr;      /* [num_sets+1], monotone, row_ptr[0] == 0 */
  const uint8_t* desc;      /* [rows][32] */
  const uint8_t* skip;      /* [rows] or NULL = none; DENSE only (must be NULL in KNN2) */
  int32_t num_jobs;         const int32_t* set_a;        /* [num_jobs] query set */   const int32_t* set_b; /* [num_jobs] candidate set */
  int32_t* match;           /* [sum of rows(set_a[j])] out */
  int32_t* dist;            /* [sum of rows(set_a[j])] out or NULL */
  int32_t* nmatches;        /* [num_jobs] out */
} covgpu_match_batch_t;
typedef struct { int32_t mode; float dist_threshold; float ratio; } covgpu_match_opts;
/* DENSE: 50 (placerec_be.cpp:85); KNN2: 40, 0.8 (config_backend.yaml:38-39). ratio is read in KNN2 only but must be finite and positive. */
void covgpu_default_match_opts(covgpu_match_opts*, int32_t mode);
int  covgpu_match_batch(covgpu_context*, const covgpu_match_batch_t*, const covgpu_match_opts*);

/* ---------------------------------------------------------------- loop-candidate float descriptor matching
 * COVINS-G with feat.type SIFT: knnMatch(k = 2) over descriptors_add_ as `dim`-float rows under the L2 norm + distance test + ratio
 * test (placerec_gen_be.cpp:82-114, RelNonCentralPosSolver.cpp:303-340). Sets and jobs as in covgpu_match_batch_t. All in float32:
 *   d2(a, b) = max(0, (|a|^2 + |b|^2) - 2 dot(a, b)),  |x|^2 and dot k-ordered fmaf chains from 0,  d = sqrtf(d2) correctly rounded.
 * Per job the two nearest train rows of every query row by (d2, index), equal distances keeping the lower index first; A row a matches
 * its nearest b1 iff B has >= 2 rows, d1 <= dist_threshold and d1 < ratio * d2 (float32 comparisons). Matches are emitted in ascending
 * a. This is the exact search (cv::BFMatcher(NORM_L2)); the reference's cv::FlannBasedMatcher approximates it and is not reproducible.
 * For integer-valued rows 0..255 (OpenCV's SIFT) at dim <= 128 every intermediate is an exact integer below 2^24, so d2 is the exact
 * sum of squared differences. match[] = local B row or -1, dist[] = d1 of a match or -1, nmatches[j] = the number of matches of job j.
 * mode must be COVGPU_MATCH_KNN2; dim is a positive multiple of 4 up to limits[1]; every set holds at most limits[0] rows;
 * num_jobs * ceil(max rows(set_a[j]) / limits[2]) may not exceed 2^31 - 1; every descriptor value is finite and at most 1e18 in
 * magnitude (a NaN would leave the order undefined). All arguments (the context included) are checked before any device work; zero jobs
 * and empty sets are valid. A set is uploaded once, however many jobs name it. */
typedef struct covgpu_match_float_batch_t {
  int32_t num_sets;         const int32_t* row_ptr;      /* [num_sets+1], monotone, row_ptr[0] == 0 */
  int32_t dim;              const float* desc;           /* [rows][dim] */
  int32_t num_jobs;         const int32_t* set_a;        /* [num_jobs] query set */   const int32_t* set_b; /* [num_jobs] train set */
  int32_t* match;           /* [sum of rows(set_a[j])] out: local B row or -1 */
  float*   dist;            /* same length, out, or NULL: d1 of a match, -1 otherwise */
  int32_t* nmatches;        /* [num_jobs] out */
} covgpu_match_float_batch_t;
/* KNN2, 500, 0.8 (config_backend.yaml:38-39, "use 500 for SIFT") */
void covgpu_default_match_float_opts(covgpu_match_opts*);
/* out = {max rows per set (4096), max dim, query rows per workgroup tile, train rows per staged chunk} */
void covgpu_match_float_limits(int32_t out[4]);
int  covgpu_match_float_batch(covgpu_context*, const covgpu_match_float_batch_t*, const covgpu_match_opts*);
/* The argument checks of covgpu_match_float_batch alone, without a context or a device ("covgpu_match_float_check: <message>"). */
int  covgpu_match_float_check(const covgpu_match_float_batch_t*, const covgpu_match_opts*);

/* ---------------------------------------------------------------- loop-candidate guided matching
 * FeatureMatcher::SearchBySE3 (feature_matcher_be.cpp:293-498) and FeatureMatcher::SearchByProjection (:168-291), many jobs per call.
 * Both project landmarks into a keyframe, collect the keypoints within a radius (KeyframeBase::GetFeaturesInArea, keyframe_base.cpp:
 * 262-318), keep those whose level lies in [predicted - 1, predicted] (LandmarkBase::PredictScale, landmark_base.cpp:120-133) and take
 * the smallest Hamming distance (:49-64) with `<`: the first keypoint visited wins a tie.
 *
 * Keypoint sets (covgpu_keypoint_sets_t, CSR over row_ptr, at most COVGPU_MATCH_MAX_ROWS rows each): kp = keypoints_distorted_ (float,
 * as KeypointType), level = (int)keypoints_aors_[i][1], desc = descriptors_ row, bounds = xmin xmax ymin ymax of IsInImage
 * (keyframe_base.cpp:414-416: x >= xmin && x < xmax && y >= ymin && y < ymax). grid_inv selects the visiting order per set: with
 * grid_inv[2s] > 0 the keyframe's grid order (AssignFeaturesToGrid, :122-143), ascending (cell_x, cell_y, index) with
 * cell = (int)round((double)kp * grid_inv), grid_inv = 64 / image width and 48 / image height; a cell outside the 64 x 48 grid is
 * clamped to it (the reference writes out of bounds there). With grid_inv NULL or grid_inv[2s] <= 0 the brute-force order, ascending
 * index. The two branches of GetFeaturesInArea return the same keypoints, so only the order differs. The area test is the reference's:
 * the target narrowed to float, distance = float32 sqrt(dx*dx + dy*dy) without fused multiply-add, accepted iff (double)distance <= radius.
 * PredictScale: n = ceil(log(max_distance / (double)(float)dist) / log(scale_factor)) clamped to [0, num_octaves - 1].
 *
 * covgpu_search_se3_batch — job j = (query set set_1[j], candidate set set_2[j], T12[j] = [qx qy qz qw x y z], p_1 = R12 p_2 + t12).
 *   Per keypoint row: lm_pos = the row's landmark in that keyframe's own camera frame (Tcw * p_w), lm_max_distance, lm_desc =
 *   Landmark::GetDescriptor() (not the keypoint's row), lm_free = landmark present, valid and not alreadyMatched (:313-339, :412-418);
 *   rows with lm_free == 0 are not searched for, and their other lm_ fields are not read. Reproduced as they are:
 *   (1) the projection is K p / z (:351-352, :431-432), no distortion, against distorted keypoints; (2) radius * 2.0^level, never
 *   scale_factor (:366, :443); (3) the projection into keyframe 1 is tested against keyframe 2's bounds (:433); (4) direction 1->2
 *   accepts bestDist <= th_low (:403), direction 2->1 bestDist < th_low (:479); (5) agreement == 0: row i agrees iff match2[i] == i with
 *   i the QUERY row (:486-495), rows i >= rows(set_2) never (the reference reads past match2); agreement == 1: match2[match1[i]] == i;
 *   (6) z < 0 skips, z == 0 goes on as IEEE has it; (7) no min/max-distance and no viewing-angle test.
 *   match[] (rows of set_1[j], jobs back to back) = the candidate row whose landmark becomes matches12[i], or -1; nfound[j] = the return
 *   value. match1 / match2 (optional) = the two directions' raw matches.
 * covgpu_search_projection_batch — job j = (set set[j], T_cw[j] = [q, t] with p_c = R p_w + t, points point_ptr[j]..point_ptr[j+1]).
 *   Per point: world position, normal, min_distance, max_distance, descriptor, skip (invalid or in spAlreadyFound, :184), existing_idx =
 *   GetFeatureIndex(kf) or -1. Per keypoint row: taken = vpMatched[idx] != NULL on entry. The keyframe's camera (cam = fx fy cx cy
 *   d0..d3, dist_type, cam_model, xi as covgpu_relpose_batch_t) projects; a failed projection skips the point. Filters: z < 0, IsInImage,
 *   0.8 min_distance <= |p_w - O_w| <= 1.2 max_distance (:208-215, landmark_base.cpp:68-76), PO . n >= 0.5 dist (:220). Radius =
 *   radius * scale_factor^level (:227). The points run in order (:240, :284): a point sees the keypoints that are not taken and that no
 *   earlier point has claimed; with bestDist <= th_low it claims its best keypoint when existing_idx == -1, else it claims nothing and
 *   remap_to[p] = bestIdx unless hamming(desc_p, desc[existing_idx]) < bestDist (:260-281; the dist_newplace test of :270-277 compares
 *   bestDist with itself and never fires). claimed[p] / remap_to[p] = keypoint row or -1, best_dist[p] = bestDist when it is <= th_low,
 *   else -1; nmatches[j] = the return value.
 * All HOST pointers. Checked before any device work: NULL pointers, row limits, set and existing_idx ranges, radius > 0 and finite (the
 * reference CHECK_GTs it), scale_factor > 1 when num_octaves > 1, num_octaves >= 1, 0 <= th_low <= 255; a violation is
 * COVGPU_ERR_INVALID_ARG. Zero jobs, empty sets and empty point lists are valid. */
#define COVGPU_GUIDED_SE3 0
#define COVGPU_GUIDED_PROJECTION 1
typedef struct covgpu_guided_opts {
  int32_t th_low;         /* desc_matching_th_low_, 50 */
  double  radius;         /* th: 9.5 (SE3), 10.0 (PROJECTION), config_backend.yaml:45-50 */
  double  scale_factor;   /* features::scale_factor, 2.0 */
  int32_t num_octaves;    /* features::num_octaves, 1 */
  int32_t agreement;      /* SE3: 0 = the reference's literal test, 1 = match2[match1[i]] == i */
} covgpu_guided_opts;
typedef struct covgpu_keypoint_sets_t {
  int32_t num_sets;         const int32_t* row_ptr;      /* [num_sets+1], monotone, row_ptr[0] == 0 */
  const float*   kp;        /* [rows][2] */
  const int32_t* level;     /* [rows] */
  const uint8_t* desc;      /* [rows][32] */
  const double*  bounds;    /* [num_sets][4] xmin xmax ymin ymax */
  const double*  grid_inv;  /* [num_sets][2] or NULL */
} covgpu_keypoint_sets_t;
typedef struct covgpu_search_se3_batch_t {
  covgpu_keypoint_sets_t sets;
  const double*  K;                /* [num_sets][4] fx fy cx cy of calibration_.K */
  const double*  lm_pos;           /* [rows][3] */
  const double*  lm_max_distance;  /* [rows] */
  const uint8_t* lm_desc;          /* [rows][32] */
  const uint8_t* lm_free;          /* [rows] */
  int32_t num_jobs;         const int32_t* set_1;        /* [num_jobs] */   const int32_t* set_2; /* [num_jobs] */
  const double*  T12;              /* [num_jobs][7] */
  int32_t* match;                  /* [sum of rows(set_1[j])] out */
  int32_t* match1;                 /* [sum of rows(set_1[j])] out or NULL */
  int32_t* match2;                 /* [sum of rows(set_2[j])] out or NULL */
  int32_t* nfound;                 /* [num_jobs] out */
} covgpu_search_se3_batch_t;
typedef struct covgpu_search_projection_batch_t {
  covgpu_keypoint_sets_t sets;
  const uint8_t* taken;            /* [rows] or NULL = none */
  const double*  cam;              /* [num_sets][8] fx fy cx cy d0 d1 d2 d3 */
  const int32_t* dist_type;        /* [num_sets] COVGPU_DIST_* */
  const int32_t* cam_model;        /* [num_sets] COVGPU_CAM_* or NULL (pinhole) */
  const double*  xi;               /* [num_sets], read for unified rows */
  int32_t num_jobs;         const int32_t* set;          /* [num_jobs] */
  const double*  T_cw;             /* [num_jobs][7] */
  const int32_t* point_ptr;        /* [num_jobs+1], monotone, point_ptr[0] == 0 */
  const double*  p_w;              /* [P][3] */
  const double*  normal;           /* [P][3] */
  const double*  min_distance;     /* [P] */
  const double*  max_distance;     /* [P] */
  const uint8_t* p_desc;           /* [P][32] */
  const uint8_t* skip;             /* [P] or NULL = none */
  const int32_t* existing_idx;     /* [P] or NULL = all -1 */
  int32_t* claimed;                /* [P] out */
  int32_t* remap_to;               /* [P] out */
  int32_t* best_dist;              /* [P] out or NULL */
  int32_t* nmatches;               /* [num_jobs] out */
} covgpu_search_projection_batch_t;
void covgpu_default_guided_opts(covgpu_guided_opts*, int32_t mode);
int  covgpu_search_se3_batch(covgpu_context*, const covgpu_search_se3_batch_t*, const covgpu_guided_opts*);
int  covgpu_search_projection_batch(covgpu_context*, const covgpu_search_projection_batch_t*, const covgpu_guided_opts*);

/* ---- Bag-of-words retrieval: DBoW2's transform and L1 score, and KeyframeDatabase::DetectCandidates ----
 *
 * The vocabulary is DBoW2's tree in flat form (covins_amd/vocio.py reads and writes the DBoW2 text format). Node 0 is the root, node ids
 * are the line order of the text file, a node's children are in line order and word ids are leaf order. The tree may be irregular:
 * leaves at different depths, nodes with one child, any k >= 1. Only L1_NORM scoring is supported; num_words is at most
 * COVGPU_BOW_MAX_WORDS = 2^20 - 1, so that a (word, row) sort key of 20 + 12 bits never equals the all-ones key of a stopped row. */
#define COVGPU_BOW_L1_NORM 0                     /* DBoW2::ScoringType */
#define COVGPU_BOW_TF_IDF 0                      /* DBoW2::WeightingType */
#define COVGPU_BOW_TF 1
#define COVGPU_BOW_IDF 2
#define COVGPU_BOW_BINARY 3
#define COVGPU_BOW_MAX_WORDS ((1 << 20) - 1)
typedef struct covgpu_bow_vocab_t {
  int32_t num_nodes, num_words;
  int32_t k, L;                                  /* the header's branching factor and depth; L - levelsup is the FeatureVector level */
  int32_t scoring, weighting;
  const int32_t* parent;                         /* [num_nodes] parent[0] = -1, parent[n] < n */
  const int32_t* child_ptr;                      /* [num_nodes+1] */
  const int32_t* child;                          /* [num_nodes-1] children of node n, ascending (line order) */
  const uint8_t* desc;                           /* [num_nodes][32] (the root's row is not read) */
  const int32_t* word_id;                        /* [num_nodes] -1 for an inner node */
  const double*  weight;                         /* [num_nodes] */
} covgpu_bow_vocab_t;

/* transform(features, bow_vec, feat_vec, levelsup) of every descriptor set. Sets arrive in the row_ptr / desc layout of
 * covgpu_match_batch_t, at most COVGPU_MATCH_MAX_ROWS rows each. bow_ptr is always exact; word / value receive the first `capacity`
 * entries and *total the true count. row_word is -1 for a stopped word (weight <= 0); row_node is the node at depth L - levelsup
 * (0 when that is <= 0; the leaf when the leaf lies above that depth, where the reference leaves the value uninitialised). */
typedef struct covgpu_bow_transform_batch_t {
  int32_t num_sets;
  const int32_t* row_ptr;                        /* [num_sets+1] */
  const uint8_t* desc;                           /* [rows][32] */
  int32_t levelsup;                              /* the reference passes 4 */
  int32_t capacity;                              /* entries of word / value */
  int32_t* bow_ptr;                              /* out [num_sets+1] */
  int32_t* word;                                 /* out [capacity] ascending within a set */
  double*  value;                                /* out [capacity] */
  int64_t* total;                                /* out, may be NULL */
  int32_t* row_word;                             /* out [rows], may be NULL */
  int32_t* row_node;                             /* out [rows], may be NULL */
} covgpu_bow_transform_batch_t;
int covgpu_bow_transform_batch(covgpu_context*, const covgpu_bow_vocab_t*, const covgpu_bow_transform_batch_t*);

/* L1Scoring::score of pairs (a[i], b[i]) of the rows of a bow CSR (word ids ascending and duplicate-free within a row). */
int covgpu_bow_score_pairs(covgpu_context*, int32_t num_vec, const int32_t* bow_ptr, const int32_t* word, const double* value,
                           int32_t num_pairs, const int32_t* a, const int32_t* b, double* score);

#define COVGPU_DETECT_COVINS 0
#define COVGPU_DETECT_COVINS_G 1
typedef struct covgpu_detect_opts {
  double  min_score_factor;                      /* 0.8 (COVINS), 0.7 (COVINS-G) */
  int32_t min_loop_dist;                         /* 100 */
  int32_t exclude_kfs_with_id_less_than;         /* 7 */
  int32_t inter_map_matches_only;                /* 0 */
  int32_t scratch_kib;                           /* per-call budget of the per-query device scratch (28 B per database entry and
                                                    query); queries run in chunks that fit it, at least one at a time. 0 = 65 536 */
} covgpu_detect_opts;
void covgpu_default_detect_opts(covgpu_detect_opts*, int32_t mode);

/* One DetectCandidates per query over a keyframe table. Query q is keyframe query_kf[q] and sees the database entries
 * db_order[0 : db_visible[q]] (table indices in insertion order), so one batch replays consecutive queries each followed by
 * AddKeyframe. nb holds, per keyframe, the table indices of GetConnectedKeyframesByWeight(0) (COVINS) or
 * GetConnectedNeighborKeyframes() (COVINS-G) in the reference's order. min_score_in NULL: the reference minimum score over the
 * query's valid neighbours times min_score_factor. Each keyframe is expected to be queried once, as DetectLoop does. */
typedef struct covgpu_detect_batch_t {
  int32_t num_kf;
  const int32_t* id;                             /* [num_kf] >= 0 */
  const int32_t* client;                         /* [num_kf] */
  const int32_t* bow_ptr;                        /* [num_kf+1] */
  const int32_t* word;
  const double*  value;
  const int32_t* nb_ptr;                         /* [num_kf+1] */
  const int32_t* nb;
  const uint8_t* invalid;                        /* [num_kf] or NULL */
  int32_t num_db;
  const int32_t* db_order;                       /* [num_db] each keyframe at most once */
  int32_t num_queries;
  const int32_t* query_kf;                       /* [num_queries] */
  const int32_t* db_visible;                     /* [num_queries] <= num_db */
  const double*  min_score_in;                   /* [num_queries] or NULL */
  int32_t cap;                                   /* candidates kept per query */
  int32_t* num_candidates;                       /* out [num_queries] the true count */
  int32_t* candidates;                           /* out [num_queries][cap] table indices in the reference's order, -1 padded */
  float*   acc_score;                            /* out [num_queries][cap] accScore of the entry that gave the candidate */
  double*  min_score;                            /* out [num_queries] */
  int32_t* num_sharing;                          /* out [num_queries] size of lKFsSharingWords */
  int32_t* max_common_words;                     /* out [num_queries] */
  int32_t* num_scored;                           /* out [num_queries] nscores */
} covgpu_detect_batch_t;
int covgpu_detect_candidates_batch(covgpu_context*, const covgpu_detect_batch_t*, const covgpu_detect_opts*);

/* ---- The resident keyframe database ----
 *
 * A covgpu_bowdb keeps the vocabulary, the bow vectors of the keyframes it was given and the inverted index of the keyframes that are
 * in the database on the device across calls, so that a query uploads the query's own lists only. A query returns exactly what
 * covgpu_detect_candidates_batch returns on the table of the stored slots with db_order = the live slots in insertion order,
 * db_visible = all of them, nb of the query = its con list, nb of an entry = its stored first ten neighbours.
 *
 * Keyframes are named by slots: dense non-negative numbers below COVGPU_BOWDB_MAX_SLOTS chosen by the caller, as a table index is for
 * the stateless call; the per-slot arrays (68 B a slot) reach up to the largest slot ever named, as a put, a neighbour or a connected
 * keyframe. A slot is `stored` once it has a vector and `live` while it is in the index. The handle belongs to its context
 * (covgpu_destroy destroys it) and works on the context's stream; calls on one context are serialised by the caller, as the reference's
 * mtx_ does. An argument error (COVGPU_ERR_INVALID_ARG, with a message) leaves the handle as it was. Every buffer grows by doubling
 * with device-to-device copies. */
#define COVGPU_BOWDB_MAX_SLOTS (1 << 24)
typedef struct covgpu_bowdb covgpu_bowdb;
typedef struct covgpu_bowdb_opts {
  covgpu_detect_opts detect;
  int32_t levelsup;                              /* of put_descriptors; the reference passes 4 */
  int32_t tail_limit;                            /* an add that leaves more positions than this outside the base index rebuilds it */
  int32_t reserve_kf;                            /* initial capacity in slots and positions */
  int32_t reserve_words;                         /* initial capacity of the vector pool, in (word, value) pairs */
  int32_t num_words;                             /* word ids are below this; used without a vocabulary, 0 = COVGPU_BOW_MAX_WORDS */
} covgpu_bowdb_opts;
void covgpu_default_bowdb_opts(covgpu_bowdb_opts*, int32_t mode);   /* detect: covgpu_default_detect_opts(mode); 4, 256, 1024, 2^18, 0 */
/* vocab may be NULL: the handle then takes vectors through covgpu_bowdb_put only. opts NULL: the defaults of COVGPU_DETECT_COVINS. */
int  covgpu_bowdb_create(covgpu_context*, const covgpu_bow_vocab_t* vocab, const covgpu_bowdb_opts* opts, covgpu_bowdb** out);
void covgpu_bowdb_destroy(covgpu_bowdb*);
/* Stores n vectors computed elsewhere (the checks of a bow CSR, word ids below num_words). A slot that is live is refused; a stored
 * slot that is not live gets the new vector. No slot twice in one call. */
int covgpu_bowdb_put(covgpu_bowdb*, int32_t n, const int32_t* slot, const int32_t* id, const int32_t* client, const int32_t* bow_ptr,
                     const int32_t* word, const double* value);
/* The same from descriptor sets, through the transform kernels against the resident vocabulary; the vectors stay on the device.
 * bt->num_sets sets go to slot[0 : num_sets]; bt->levelsup must be the handle's. Every output of bt may be NULL and is downloaded only
 * if it is not (word / value: the first bt->capacity entries). */
int covgpu_bowdb_put_descriptors(covgpu_bowdb*, const int32_t* slot, const int32_t* id, const int32_t* client,
                                 const covgpu_bow_transform_batch_t* bt);
/* The connected keyframes (slots, the reference's order) of n slots; the first ten of each are kept (kf_database.cpp:141-142). */
int covgpu_bowdb_set_neighbours(covgpu_bowdb*, int32_t n, const int32_t* slot, const int32_t* nb_ptr, const int32_t* nb);
/* IsInvalid() of n slots, for the reference minimum score. */
int covgpu_bowdb_set_invalid(covgpu_bowdb*, int32_t n, const int32_t* slot, const uint8_t* flag);
/* AddKeyframe: the slots join the insertion order at its end. A slot without a vector is refused. A slot that is live is refused too:
 * the reference would list it twice and count its words twice, which no caller of it does. */
int covgpu_bowdb_add(covgpu_bowdb*, int32_t n, const int32_t* slot);
/* EraseKeyframe: a slot that is not live is skipped, as in the reference. The vector stays stored (it may be a query's neighbour). */
int covgpu_bowdb_erase(covgpu_bowdb*, int32_t n, const int32_t* slot);
typedef struct covgpu_bowdb_query_t {
  int32_t num_queries;
  const int32_t* query_slot;                     /* [num_queries] stored slots */
  const int32_t* con_ptr;                        /* [num_queries+1] or NULL = no connected keyframes */
  const int32_t* con;                            /* the query's whole connected list: slots, the reference's order */
  const double*  min_score_in;                   /* [num_queries] or NULL: the reference minimum score; every connected slot that is
                                                    not invalid must then be stored */
  int32_t cap;
  int32_t* num_candidates;                       /* out, as covgpu_detect_batch_t; candidates are slots */
  int32_t* candidates;
  float*   acc_score;
  double*  min_score;
  int32_t* num_sharing;
  int32_t* max_common_words;
  int32_t* num_scored;
} covgpu_bowdb_query_t;
/* All queries of one call see the same database state. */
int covgpu_bowdb_query(covgpu_bowdb*, const covgpu_bowdb_query_t*);
/* Rebuilds the base index now: erased positions and dead pool words go, the tail joins the base. */
int covgpu_bowdb_compact(covgpu_bowdb*);
/* The live slots in insertion order: the first `capacity` into slots, the true number into *count. */
int covgpu_bowdb_order(covgpu_bowdb*, int32_t capacity, int32_t* slots, int32_t* count);
/* out[0] stored slots, [1] live entries, [2] positions including erased ones, [3] postings in the base index, [4] positions in the tail,
 * [5] rebuilds so far, [6] host-to-device and [7] device-to-host bytes of the last call on the handle other than this one (after create:
 * the vocabulary upload), [8] device bytes held, [9] pool words in use, [10] pool words dead, [11] slot
 * capacity, [12] position capacity, [13] pool capacity, [14] buffer growths so far, [15] 0. */
int covgpu_bowdb_stats(covgpu_bowdb*, int64_t out[16]);

/* ---------------------------------------------------------------- redundant-keyframe pruning
 * Map::RemoveRedundantData (map_be.cpp:745-811) on the device, as an exact integer rule.
 *
 * Value (Keyframe::ComputeRedundancyValue, keyframe_be.cpp:228-256): a landmark with n live observations is worth v(n) tenths, 0 for
 * n <= 2, then 4, 7, 9 for n = 3, 4, 5 and 10 from 6 on. An observation is live while its keyframe is valid and not erased. Over the live
 * observations of keyframe k on valid landmarks with n >= 2: num[k] = sum of v(n), den[k] = their number; the redundancy value is
 * num / (10 den). A (keyframe, landmark) pair listed twice is counted as given.
 * Candidates (:752-759), fixed before the first round: valid, not kf_first, with a predecessor and a successor.
 * A round picks the candidate of largest value, compared as num_a * den_b > num_b * den_a in int64; den == 0 ranks after every den > 0 and
 * equal values go to the lowest index. Before the pick is handled the call stops, in this order, with stop_reason 2 when max_kfs >= 0 and
 * at most max_kfs valid keyframes are left, 0 when no candidate is left, 1 when max_kfs < 0 and the pick has den == 0 or
 * (double)num / (double)(10 den) < th_red, 3 when max_rounds rounds have run. The pick always leaves the candidate list. It stays in the
 * map with action 1 when time[succ] - time[pred] >= max_time_dist, else 2 when it is a loop keyframe, else 3 when kf_not_erase is set
 * (SetInvalid refuses, keyframe_be.cpp:510, yet the reference's count includes it). Otherwise action 0, SetInvalid (:514-526): its
 * observations stop being live, succ[pred] = succ, pred[succ] = pred, one valid keyframe less.
 *
 * Where this departs from the letter of the reference, each time as one outcome the reference can produce: (1) std::sort leaves the
 * order of equal values to the implementation; (2) a 0/0 value is NaN there, under a comparator that is then no strict weak order;
 * (3) the reference sums the doubles 0.4 / 0.7 / 0.9 / 1.0 in feature order, here the sums are integers.
 * Map::Clean at the top of the reference function changes no value (a landmark with fewer than two observations never counts); the
 * caller runs it, and lm_nobs tells which landmarks a later Clean drops. */
typedef struct covgpu_prune_t {
  int32_t num_kf, num_lm;
  const int32_t* lm_obs_ptr;                     /* [num_lm+1] landmark-major, as covgpu_problem */
  const int32_t* obs_kf;                         /* [lm_obs_ptr[num_lm]] keyframe table index */
  const uint8_t* lm_invalid;                     /* [num_lm] or NULL = none */
  const uint8_t* kf_invalid;                     /* [num_kf] or NULL = none */
  const uint8_t* kf_first;                       /* [num_kf] id_.first == 0, or NULL = none */
  const uint8_t* kf_loop;                        /* [num_kf] is_loop_kf_, or NULL = none */
  const uint8_t* kf_not_erase;                   /* [num_kf] not_erase_, or NULL = none */
  const int32_t* kf_pred;                        /* [num_kf] table index, -1 = none */
  const int32_t* kf_succ;                        /* [num_kf] */
  const double*  kf_time;                        /* [num_kf] seconds */
  int32_t capacity;                              /* entries of round_kf / round_action */
  /* out; each may be NULL */
  int32_t* round_kf;                             /* [capacity] the keyframe of each round */
  int32_t* round_action;                         /* [capacity] 0 erased, 1 time gate, 2 loop keyframe, 3 not_erase */
  int32_t* num_rounds;                           /* the true count, also beyond capacity */
  int32_t* removed;                              /* the reference's return value: actions 0 + 3 */
  int32_t* stop_reason;                          /* 0 no candidates, 1 below threshold, 2 max_kfs reached, 3 max_rounds */
  int32_t* kf_pred_out;                          /* [num_kf] the relinked chain */
  int32_t* kf_succ_out;                          /* [num_kf] */
  int32_t* lm_nobs;                              /* [num_lm] live observations left */
  int32_t* red_num;                              /* [num_kf] for a handled keyframe: at the round it was handled */
  int32_t* red_den;                              /* [num_kf] */
  double*  loop_ms;                              /* device time of the greedy-loop kernel alone (HIP events around it) */
} covgpu_prune_t;
typedef struct covgpu_prune_opts {
  double  th_red;                                /* 0.95 (config_backend.yaml:58) */
  double  max_time_dist;                         /* 1.0 s (config_backend.yaml:59) */
  int32_t max_kfs;                               /* < 0: threshold mode; else count mode: prune down to max_kfs valid keyframes */
  int32_t max_rounds;                            /* <= 0: num_kf */
} covgpu_prune_opts;
void covgpu_default_prune_opts(covgpu_prune_opts*);
/* The argument checks of covgpu_prune_redundant alone (no context, no device): COVGPU_OK or COVGPU_ERR_INVALID_ARG with the message.
 * Rejected: NULL required arrays, lm_obs_ptr not starting at 0 or not monotone, obs_kf out of range, kf_pred / kf_succ out of range or
 * not mutual (succ[pred[k]] == k and pred[succ[k]] == k wherever both exist), non-finite th_red, max_time_dist or kf_time. */
int covgpu_prune_check(const covgpu_prune_t*, const covgpu_prune_opts*);
int covgpu_prune_redundant(covgpu_context*, const covgpu_prune_t*, const covgpu_prune_opts*);

/* ---------------------------------------------------------------- landmark refresh
 * Landmark::ComputeDescriptor (landmark_be.cpp:49-92) and Landmark::UpdateNormal (:185-220) for every landmark of a map in one call: the
 * representative descriptor, the viewing normal and the scale-invariance distances that the guided matching reads.
 *
 * Order: a landmark's observations are taken in the order given. The reference iterates a std::map keyed by shared_ptr address
 * (typedefs_base.hpp:187), so its order — and with it its tie-break and its summation order — is an accident of the allocator; the
 * order given is one outcome the reference can produce. This is the one departure from the letter of the reference.
 * Candidates: the landmark's observations whose keyframe is valid, in list order; n is their number. A keyframe listed twice counts twice.
 * Descriptor: d(i, j) is the Hamming distance over 256 bits, d(i, i) = 0. The median of row i is its element of rank (n - 1) / 2
 * (integer division) in ascending order, the self-distance included (distances[0.5 * (num_desc - 1)]). The choice is the lowest i whose
 * median is strictly smallest (<, :86). lm_desc_obs is the chosen observation's position in the landmark's own list (not among the
 * candidates), -1 when n = 0; lm_desc its 32 bytes, zeros when -1 (the reference leaves descriptor_ as it was).
 * Normal: for each candidate in list order v = lm_pos - kf_center, u = v / sqrt((v.x v.x + v.y v.y) + v.z v.z);
 * normal = (((0 + u_0) + u_1) + ...) / (double)n. Distances: dist = the same norm of lm_pos - kf_center[keyframe of the reference
 * observation] (not asked whether it is valid, as in the reference), max_distance = dist * scale[level], min_distance = max_distance /
 * scale[num_octaves - 1], level = obs_octave of the reference observation, scale[l] = std::pow(scale_factor, l) tabulated on the host.
 * Every operation is an IEEE double operation on its own: no fused multiply-add.
 * lm_status: bit 0 no valid observer (the reference divides 0 by 0; here the normal is 0), bit 1 no reference observation (the
 * reference exits; here the distances are 0), bit 2 the landmark is invalid: skipped, status 4 and every other output 0 / -1. */
#define COVGPU_LMR_GROUP_MAX 64                  /* longest observation list of the lane-group forms; the long form starts one above */
#define COVGPU_LMR_WAVE 64                       /* the long form strides a row over one wavefront ... */
#define COVGPU_LMR_LONG_THREADS 256              /* ... of a workgroup of this size, which also is its chunk of the normal's sum ... */
#define COVGPU_LMR_STAGE 512                     /* ... and keeps this many descriptors of the landmark in LDS */
#define COVGPU_LMR_FORMS 6                       /* form_count: lists of <= 4, 8, 16, 32, 64 (lane groups of that width), longer (long form) */
typedef struct covgpu_landmark_refresh_t {
  int32_t num_kf, num_lm;
  const int32_t* lm_obs_ptr;                     /* [num_lm+1] landmark-major, as covgpu_prune_t */
  const int32_t* obs_kf;                         /* [O = lm_obs_ptr[num_lm]] keyframe table index */
  const uint8_t* obs_desc;                       /* [O][32] the observing keypoint's ORB row, or NULL: no descriptors asked for */
  const int32_t* obs_octave;                     /* [O] (int)keypoints_aors_[feat](1) */
  const int32_t* lm_ref_obs;                     /* [num_lm] position of the reference keyframe's observation in the landmark's list, -1 = none */
  const double*  lm_pos;                         /* [num_lm][3] */
  const double*  kf_center;                      /* [num_kf][3] translation of GetPoseTwc() */
  const uint8_t* kf_invalid;                     /* [num_kf] or NULL = none */
  const uint8_t* lm_invalid;                     /* [num_lm] or NULL = none */
  /* out; each may be NULL */
  int32_t* lm_desc_obs;                          /* [num_lm]; not written when obs_desc is NULL */
  uint8_t* lm_desc;                              /* [num_lm][32]; not written when obs_desc is NULL */
  double*  lm_normal;                            /* [num_lm][3] */
  double*  lm_min_distance;                      /* [num_lm] */
  double*  lm_max_distance;                      /* [num_lm] */
  int32_t* lm_status;                            /* [num_lm] bit mask, see above */
  int32_t* form_count;                           /* [COVGPU_LMR_FORMS] landmarks that took each kernel form; an invalid landmark takes the first */
  double*  kernel_ms;                            /* device time of the kernels alone (HIP events around them) */
} covgpu_landmark_refresh_t;
typedef struct covgpu_landmark_refresh_opts {
  double  scale_factor;                          /* 2.0 (config_backend.yaml:31) */
  int32_t num_octaves;                           /* 1 (config_backend.yaml:32) */
} covgpu_landmark_refresh_opts;
void covgpu_default_landmark_refresh_opts(covgpu_landmark_refresh_opts*);
/* {COVGPU_LMR_GROUP_MAX, COVGPU_LMR_WAVE, COVGPU_LMR_LONG_THREADS, COVGPU_LMR_STAGE} as the library was built */
void covgpu_landmark_refresh_limits(int32_t out[4]);
/* The argument checks of covgpu_landmark_refresh alone (no context, no device): COVGPU_OK or COVGPU_ERR_INVALID_ARG with the message.
 * Rejected: NULL required arrays, lm_obs_ptr not starting at 0 or not monotone, obs_kf out of range, lm_ref_obs outside its landmark's
 * list, a reference observation whose octave is outside [0, 64), num_octaves outside [1, 64], a non-finite or non-positive
 * scale_factor, non-finite positions or centres. */
int covgpu_landmark_refresh_check(const covgpu_landmark_refresh_t*, const covgpu_landmark_refresh_opts*);
int covgpu_landmark_refresh(covgpu_context*, const covgpu_landmark_refresh_t*, const covgpu_landmark_refresh_opts*);

/* ---- Vocabulary training: DBoW2's TemplatedVocabulary::create for ORB descriptors under L1 scoring ----
 *
 * create(training_features, k, L, weighting, scoring): hierarchical k-means (k-means++ seeding, FORB::meanValue centres, FORB::distance
 * association with the first minimum winning), createWords and setNodeWeights. Node ids are the reference's (the children of a node get
 * consecutive ids when the node is processed, nodes are processed depth first), word ids are leaf order. All of it is integer work, so
 * the result is defined bit for bit; tests/voctrain_ref.py restates it. Deliberate departures from the reference:
 *   D1 random numbers are counter based: key(root) = seed, key(child c) = splitmix64(key(node) + 1 + c); draw j of a node is
 *      r = splitmix64(splitmix64(key(node)) + j), u = (r >> 11) * 2^-53; j counts every draw of the node. The first centre is row
 *      min(int(u n), n - 1); a further centre is the first row whose inclusive prefix sum of minimum distances, as a double, is
 *      >= cut_d = u * dist_sum (redrawn while 0.0, at most 64 times), the last row if there is none.
 *   D2 a cluster that loses all its members keeps its previous centre and stays a node (a leaf with an empty group).
 *   D3 the k-means loop of one node runs at most max_iterations associations; stats[2] counts the nodes it cut short.
 *   D4 zero descriptor rows, k < 2, L < 1 and k^L > COVGPU_BOW_MAX_WORDS are COVGPU_ERR_INVALID_ARG; so are k > COVGPU_VOCTRAIN_MAX_K and
 *      a scratch_kib below one set's word bitmap, ceil(k^L / 8192) KiB, and more than 2^31 - 1 - COVGPU_VOCTRAIN_TILE rows.
 * Sets arrive in the row_ptr / desc layout of covgpu_bow_transform_batch_t, without its limit on the rows of a set; empty sets are
 * allowed and count in NDocs. The outputs are the per-node arrays of covgpu_bow_vocab_t; child_ptr / child are left to the caller
 * (vocio.from_nodes, CreateVocabulary of the C++ facade): they follow from parent. If the tree has more than node_capacity nodes the
 * call returns COVGPU_ERR_INVALID_ARG, *num_nodes holds the count needed and no other output is written. */
#define COVGPU_VOCTRAIN_MAX_K 32                 /* largest branching factor: the kernels keep k x 256 bit counters in LDS */
#define COVGPU_VOCTRAIN_WAVE_MAX 256             /* a node of at most this many rows is worked by one wavefront ... */
#define COVGPU_VOCTRAIN_TILE 2048                /* ... a larger one by workgroups of COVGPU_VOCTRAIN_THREADS over tiles of this many rows */
#define COVGPU_VOCTRAIN_THREADS 256
typedef struct covgpu_voc_train_t {
  int32_t num_sets;
  const int32_t* row_ptr;                        /* [num_sets+1] */
  const uint8_t* desc;                           /* [rows][32] */
  int32_t node_capacity;                         /* entries of parent / desc / word_id / weight */
  int32_t* num_nodes;                            /* out: nodes of the tree, the root included */
  int32_t* num_words;                            /* out */
  int32_t* parent;                               /* out [node_capacity] parent[0] = -1 */
  uint8_t* desc_out;                             /* out [node_capacity][32] the root's row is zero */
  int32_t* word_id;                              /* out [node_capacity] -1 for an inner node and the root */
  double*  weight;                               /* out [node_capacity] 0 for an inner node */
  int32_t* row_word;                             /* out [rows] or NULL: the transform leaf (word id) of every training row */
  int64_t* stats;                                /* out [8] or NULL: k-means associations summed; most of one node; nodes cut short by
                                                  * max_iterations; centre updates that met an empty group (D2); nodes seeded with fewer
                                                  * than k centres; levels worked; bytes to the device; bytes from it */
} covgpu_voc_train_t;
typedef struct covgpu_voc_train_opts {
  int32_t k, L;                                  /* 10, 5 */
  int32_t weighting, scoring;                    /* COVGPU_BOW_TF_IDF, COVGPU_BOW_L1_NORM */
  uint64_t seed;                                 /* 0 */
  int32_t max_iterations;                        /* 100 (D3) */
  int32_t scratch_kib;                           /* 65536: device bytes of the per-set word bitmaps behind the weights */
} covgpu_voc_train_opts;
void covgpu_default_voc_train_opts(covgpu_voc_train_opts*);
/* {COVGPU_VOCTRAIN_WAVE_MAX, COVGPU_VOCTRAIN_TILE, COVGPU_VOCTRAIN_MAX_K, COVGPU_VOCTRAIN_THREADS} as the library was built. A node of
 * at most k rows takes no k-means at all: k is the third size at which the path changes. */
void covgpu_voc_train_limits(int32_t out[4]);
/* The argument checks of covgpu_voc_train alone (no context, no device): COVGPU_OK or COVGPU_ERR_INVALID_ARG with the message. */
int covgpu_voc_train_check(const covgpu_voc_train_t*, const covgpu_voc_train_opts*);
int covgpu_voc_train(covgpu_context*, const covgpu_voc_train_t*, const covgpu_voc_train_opts*);

/* ---- Marginal covariances of selected keyframes from the multifrontal factor ----
 *
 * The joint covariance of the chosen keyframes' unknowns after the landmarks (and every other keyframe) are marginalised: the rows and
 * columns `kf` of the inverse of exactly the matrix covgpu_schur / covgpu_schur_pgo return at the same mu (whitened, loss-corrected
 * residuals; A.1's right-perturbation tangent; no further scaling: the fronts hold that matrix entry for entry). With S = L L^T the
 * block is (L^-1 E)^T (L^-1 E) over the unit columns E of the chosen unknowns: forward substitutions along the paths from the fronts
 * that own them to the root, then one Gram product, every sum in a fixed order (k_marginal.hip). `cov` is symmetric bit for bit: a
 * pair is computed once and stored twice.
 * Refused with COVGPU_ERR_INVALID_ARG: num_kf outside [1, COVGPU_MARGINAL_MAX_KF], an index out of range, a duplicate, a keyframe
 * whose pose is constant (kf_fixed: its rows of the system are identity rows, it has no covariance), block outside {0, 1}, mu
 * negative or not finite, a NULL cov; a sharded context; a context whose pose graph is off the elimination tree (COVGPU_PGO_ND=0).
 * A factorisation that meets a non-positive pivot is COVGPU_ERR_NUMERIC, as in covgpu_gn_step.
 * Scratch: per call, freed when it returns: 8 bytes x (columns rounded up to 16) x (own unknowns of the fronts on the chosen paths,
 * each front's rounded up to 16) for the working right-hand sides, 8 m^2 for the result and the index tables. The rows are at most
 * n + 15 per front, so at the limits (32 keyframes, block 1: 480 columns) on the 12-agent map (n = 36 000) a call stays below
 * 8 x 480 x 40 000 = 154 MB. */
#define COVGPU_MARGINAL_MAX_KF 32                /* keyframes of one call */
#define COVGPU_MARGINAL_MAX_COLS 480             /* its columns: 32 x 15 */
#define COVGPU_MARGINAL_MFMA_COLS 16             /* a front with this many active columns or more takes the matrix-core form */
typedef struct covgpu_marginal_t {
  int32_t num_kf;        /* q: 1 .. COVGPU_MARGINAL_MAX_KF */
  const int32_t* kf;     /* [q] keyframe indices of the problem, distinct, any order */
  int32_t block;         /* 0: pose rows only (d = 6); 1: all D rows of the keyframe (15 visual-inertial, 6 visual-only / pose graph) */
  double mu;             /* damping of the factored system, >= 0; 0 = the covariance proper */
  double* cov;           /* out [m][m], m = q*d, row-major, in the order of `kf`, rows of a keyframe in IR order (A.1: dtheta, dp, then dv, db_a, db_g) */
  int64_t* stats;        /* out [8], may be NULL: columns, fronts visited, launches, launches of the matrix-core form, of the vector form,
                          * bytes of scratch, 0, 0 */
} covgpu_marginal_t;
/* {COVGPU_MARGINAL_MAX_KF, COVGPU_MARGINAL_MAX_COLS, COVGPU_MARGINAL_MFMA_COLS, rows of a panel step (128)} as the library was built */
void covgpu_marginal_limits(int32_t out[4]);
/* The argument checks of covgpu_marginal_covariance alone (no context, no device): COVGPU_OK or COVGPU_ERR_INVALID_ARG with the message.
 * The two refusals that depend on the context (sharded; pose graph off the tree) are made by the calls themselves. */
int covgpu_marginal_check(const covgpu_problem*, const covgpu_options*, const covgpu_marginal_t*);
/* Uploads `p` as covgpu_gn_step does (pgo != 0: as covgpu_upload_pgo), linearises at its estimate, builds and factors at mu, sweeps. */
int covgpu_marginal_covariance(covgpu_context*, const covgpu_options*, const covgpu_problem*, int32_t pgo, const covgpu_marginal_t*);
/* The same at the estimate the context holds (what covgpu_download returns) after an upload or a finished solve. A following
 * covgpu_solve_resident returns the bits it would have returned without this call: every solve restarts from the uploaded estimate. */
int covgpu_marginal_resident(covgpu_context*, const covgpu_options*, const covgpu_marginal_t*);

/* ---- Covariance of every keyframe by selected inversion of the multifrontal factor ----
 *
 * Sigma = S^-1 on the structure of L (S = L L^T the matrix covgpu_schur / covgpu_schur_pgo return at the same mu; conventions as the
 * marginal call above): the Takahashi recursion from the root of the elimination tree down. For a front with own unknowns O and border B
 *   Sigma_BO = -Sigma_BB T,  Sigma_OO = W^T W - T^T Sigma_BO   with W = L_OO^-1, T = L_BO W,
 * Sigma_BB gathered from the finished square of the deepest owner among the border rows (k_selinv.hip). The diagonal block of every
 * keyframe is read out of it, and the cross block of every requested pair that lies on the structure of L: with block 0 every pair whose
 * pose blocks are coupled in S (covisible pairs, IMU neighbours, loop edges), with block 1 every pair joined by an IMU factor; any other
 * pair is served when the tree happens to hold it, else pair_ok = 0 and its block is zeroed (take it from covgpu_marginal_covariance).
 * Refused with COVGPU_ERR_INVALID_ARG: block outside {0, 1}, mu negative or not finite, a NULL kf_cov, a negative num_pairs,
 * num_pairs > 0 with a NULL pair array, a pair index out of range, equal indices, a keyframe with a constant pose in a pair; a sharded
 * context; a context whose pose graph is off the elimination tree (COVGPU_PGO_ND=0). A non-positive pivot is COVGPU_ERR_NUMERIC, a
 * scratch allocation that fails COVGPU_ERR_OUT_OF_MEMORY (nothing of the sweep is enqueued, the context stays usable).
 * Scratch (stats[5]): two buffers laid out like the fronts (Sigma, and W / T of the level at work) and the tables. The factor is only read. */
#define COVGPU_SELINV_MFMA_ROWS 128             /* a front with this many rows (own + border) or more takes the matrix-core form */
typedef struct covgpu_selinv_t {
  int32_t block;         /* 0: pose rows (d = 6); 1: all D rows of a keyframe, as covgpu_marginal_t::block */
  double  mu;            /* >= 0, finite */
  double* kf_cov;        /* out [K][d][d] row-major: diagonal block of every keyframe; a constant-pose keyframe: zeros */
  int64_t num_pairs;     /* may be 0 */
  const int32_t *pair_i, *pair_j;   /* [num_pairs] keyframe indices, i != j, both free */
  double* pair_cov;      /* out [num_pairs][d][d]: Sigma[rows of i][columns of j] */
  uint8_t* pair_ok;      /* out [num_pairs]: 1 = every requested sub-block lies on the structure of L; 0 = not stored, block zeroed */
  int64_t* stats;        /* out [8], may be NULL: fronts, levels, launches, launches of the matrix-core form, of the vector form,
                          * bytes of scratch, pairs served, 0 */
} covgpu_selinv_t;
/* {COVGPU_SELINV_MFMA_ROWS, own columns of a panel (128), rows of a block step (16), 0} as the library was built */
void covgpu_selinv_limits(int32_t out[4]);
/* The argument checks of covgpu_selected_inverse alone (no context, no device): COVGPU_OK or COVGPU_ERR_INVALID_ARG with the message. */
int covgpu_selinv_check(const covgpu_problem*, const covgpu_options*, const covgpu_selinv_t*);
/* Uploads `p` as covgpu_gn_step does (pgo != 0: as covgpu_upload_pgo), linearises at its estimate, builds and factors at mu, sweeps. */
int covgpu_selected_inverse(covgpu_context*, const covgpu_options*, const covgpu_problem*, int32_t pgo, const covgpu_selinv_t*);
/* The same at the estimate the context holds, after an upload or a finished solve. A following covgpu_solve_resident returns the bits
 * it would have returned without this call. */
int covgpu_selected_inverse_resident(covgpu_context*, const covgpu_options*, const covgpu_selinv_t*);

/* ---- Covariance of every landmark from the selected inverse ----
 *
 * The 3x3 diagonal block of the inverse of the WHOLE damped system (poses, speed-biases and landmarks) at every landmark, by the Schur
 * identity on what a build at mu leaves resident: with H_ll^-1 = R R^T and Z_a = (J_p^T J_l) R of observation a (k_visual.hip),
 *   Sigma_l = H_ll^-1 + H_ll^-1 H_lp Sigma_pp H_pl H_ll^-1 = R (I + sum over a, b of Z_a^T Sigma_ab Z_b) R^T,
 * a and b the observations of l by keyframes with a free pose, Sigma_ab the 6x6 pose-pose block of the selected inverse above: any two
 * observers of a landmark are covisible, so the block lies on the structure of L. One landmark-major pass (k_lmcov.hip) behind the sweep
 * of covgpu_selected_inverse; every sum in one fixed order, no atomics: two calls return the same bits, and lm_cov is symmetric bit for bit.
 * A landmark no free keyframe observes gets H_ll^-1 = R R^T. A landmark whose damped H_ll the linearisation could not factor (not positive
 * definite: fewer than three independent rows and mu = 0) gets lm_ok = 0 and a zero block, as does a landmark for which a block of
 * Sigma between two of its observers was not found (never a block that is too small). The limit of lm_ok: it is the linearisation's own
 * test (a determinant that is exactly zero, a pivot that is not positive). An H_ll that is rank deficient only up to rounding — two
 * observations on nearly one ray, mu = 0 — can pass it and come back with lm_ok = 1 and a huge, meaningless block: judge such a landmark
 * by the size of its block, or run at a small mu > 0.
 * Refused with COVGPU_ERR_INVALID_ARG: a NULL lm_cov or lm_ok, mu negative or not finite, a problem without landmarks; a context that
 * holds a pose graph; a sharded context; nothing uploaded (resident form). A non-positive pivot of the reduced system is
 * COVGPU_ERR_NUMERIC, a scratch allocation that fails COVGPU_ERR_OUT_OF_MEMORY (nothing is enqueued, the context stays usable).
 * Scratch (stats[5]): the sweep's two buffers and tables, 16 bytes per covisible pair and per keyframe, 4 (K + 1) bytes, the outputs. */
typedef struct covgpu_lmcov_t {
  double   mu;        /* >= 0, finite; 0 = the covariance proper */
  double*  lm_cov;    /* out [L][3][3] row-major, world frame, landmark order of the problem (resident form: of the resident
                         observation set — after covgpu_gba_two_round the second round's landmarks, those with lm_left >= 2, in order) */
  uint8_t* lm_ok;     /* out [L]: 1 = served; 0 = H_ll not positive definite, block zeroed */
  double*  kf_cov;    /* out [K][6][6], may be NULL: the pose diagonal blocks the sweep has anyway (covgpu_selinv_t::kf_cov at block 0) */
  int64_t* stats;     /* out [8], may be NULL: fronts, levels, launches of the sweep, launches of the landmark pass,
                         group width, bytes of scratch, covisible pairs resolved, landmarks with lm_ok = 0 */
} covgpu_lmcov_t;
/* {largest group width (16), threads of a workgroup of the landmark pass (256), doubles of a landmark's block (9), 0} as the library was built */
void covgpu_lmcov_limits(int32_t out[4]);
/* The argument checks of covgpu_landmark_covariance alone (no context, no device): COVGPU_OK or COVGPU_ERR_INVALID_ARG with the message. */
int covgpu_lmcov_check(const covgpu_problem*, const covgpu_options*, const covgpu_lmcov_t*);
/* Uploads `p` as covgpu_gn_step does, linearises at its estimate, builds and factors at mu, sweeps, runs the landmark pass. */
int covgpu_landmark_covariance(covgpu_context*, const covgpu_options*, const covgpu_problem*, const covgpu_lmcov_t*);
/* The same at the estimate and the observation set the context holds, after an upload or a finished solve. A following
 * covgpu_solve_resident returns the bits it would have returned without this call. */
int covgpu_landmark_covariance_resident(covgpu_context*, const covgpu_options*, const covgpu_lmcov_t*);

/* ---- Covariance of every observation and its pose-landmark cross block ----
 *
 * For every observation o = (a, l) of the observation stream, at damping mu (conventions of the three calls above: S whitened and
 * loss-corrected as covgpu_schur returns it, A.1's tangent, world frame):
 *   obs_cov   C_o = J_o Sigma J_o^T, the 2x2 block of the hat matrix: J_o = [J_p J_l] the whitened, loss-corrected 2x9 Jacobian of the
 *             observation, Sigma the inverse of the WHOLE damped system restricted to (pose of a, landmark l). 0 <= C_o <= I in exact
 *             arithmetic at any mu >= 0; the normalised residual of the observation is r^T (I - C_o)^-1 r with r = obs_res.
 *   cross_cov Sigma_al, pose rows of the observer (dtheta, dp) by the landmark's coordinates.
 * With H_ll^-1 = R R^T, Z_b = (J_p^T J_l) R of observation b of l, V_a = sum_b Sigma_ab Z_b, M = sum_a Z_a^T V_a and Y = J_l R:
 *   Sigma_al = -V_a R^T,   C_o = [J_p -Y] [[Sigma_aa, V_a], [V_a^T, (M + M^T) / 2]] [J_p -Y]^T + Y Y^T,
 * one landmark-major pass (k_obscov.hip) behind the sweep of covgpu_selected_inverse: pass 1 is the landmark call's sum, pass 2 evaluates
 * the observation again. Every sum in one fixed order, no atomics: two calls return the same bits; obs_cov is symmetric bit for bit (the
 * off-diagonal entry is computed once and stored twice). lm_cov, lm_ok and kf_cov are covgpu_landmark_covariance's, bit for bit.
 * Edges: an observer with a constant pose has J_p = 0 — its cross_cov is zeros, C_o = J_l Sigma_l J_l^T, obs_ok = 1. An observation that
 * does not project (r = 0, J = 0) has C_o = 0 and obs_ok = 1. An observation of a landmark that is not served (lm_ok = 0 by the landmark
 * call's rule, "a block of Sigma was not found" included) has obs_ok = 0 and zero blocks.
 * Order of the outputs: the landmark-major observation order of the problem (lm_obs_ptr). Resident form: of the resident observation
 * stream — after covgpu_gba_two_round the compacted second-round stream, the kept observations of the landmarks with lm_left >= 2, in order
 * (as lm_cov: the second round's landmarks).
 * With reproj_loss_a > 0 every block is in loss-corrected units (the Jacobians and the residual carry the loss's scale).
 * Refused with COVGPU_ERR_INVALID_ARG: a NULL obs_cov or obs_ok, mu negative or not finite, a problem without observations, lm_cov given
 * without lm_ok; a context that holds a pose graph; a sharded context; nothing uploaded (resident form). A non-positive pivot of the
 * reduced system is COVGPU_ERR_NUMERIC, a scratch allocation that fails COVGPU_ERR_OUT_OF_MEMORY (nothing is enqueued, the context
 * stays usable). Scratch (stats[5]): the landmark call's, and 8 (18 + 4 + 2) + 1 bytes per observation. */
typedef struct covgpu_obscov_t {
  double   mu;         /* >= 0, finite; 0 = the covariance proper */
  double*  obs_cov;    /* out [O][2][2] row-major */
  double*  cross_cov;  /* out [O][6][3] row-major, may be NULL */
  double*  obs_res;    /* out [O][2], may be NULL: the whitened, loss-corrected residual of the same evaluation */
  uint8_t* obs_ok;     /* out [O]: 1 = served; 0 = the landmark is not served, blocks zeroed */
  double*  lm_cov;     /* out [L][3][3], may be NULL: covgpu_lmcov_t::lm_cov */
  uint8_t* lm_ok;      /* out [L], may be NULL unless lm_cov is given */
  double*  kf_cov;     /* out [K][6][6], may be NULL: covgpu_lmcov_t::kf_cov */
  int64_t* stats;      /* out [8], may be NULL: fronts, levels, launches of the sweep, launches of the observation pass, group width,
                          bytes of scratch, observations with obs_ok = 0, observations whose observer has a constant pose */
} covgpu_obscov_t;
/* {largest group width (16), threads of a workgroup of the observation pass (256), doubles of a cross block (18), of an obs block (4)} */
void covgpu_obscov_limits(int32_t out[4]);
/* The argument checks of covgpu_observation_covariance alone (no context, no device): COVGPU_OK or COVGPU_ERR_INVALID_ARG with the message. */
int covgpu_obscov_check(const covgpu_problem*, const covgpu_options*, const covgpu_obscov_t*);
/* Uploads `p` as covgpu_gn_step does, linearises at its estimate, builds and factors at mu, sweeps, runs the observation pass. */
int covgpu_observation_covariance(covgpu_context*, const covgpu_options*, const covgpu_problem*, const covgpu_obscov_t*);
/* The same at the estimate and the observation stream the context holds, after an upload or a finished solve. A following
 * covgpu_solve_resident returns the bits it would have returned without this call. */
int covgpu_observation_covariance_resident(covgpu_context*, const covgpu_options*, const covgpu_obscov_t*);

#ifdef __cplusplus
}
#endif
#endif /* COVGPU_H_ */
