"""ctypes mirror of include/covgpu.h — the C-ABI boundary of the GBA / PGO hot path.

`FlatProblem` is the Python-side owner of the flat problem IR: one numpy array per
`covgpu_problem` field, laid out exactly as the header documents. The C++ facade
(include/covins_gpu/optimization_gpu.hpp) fills the same struct from Map/Keyframe/Landmark as
covins_backend/src/covins_backend/optimization_be.cpp:320-557 does for ceres::Problem.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

COVGPU_OK = 0
COVGPU_DOGLEG, COVGPU_LM = 0, 1
COVGPU_DIST_RADTAN, COVGPU_DIST_EQUIDISTANT = 0, 1
COVGPU_CAM_PINHOLE, COVGPU_CAM_UNIFIED = 0, 1   # camera projection models (values of the reference's eCamModel)
COVGPU_MAX_TRACE = 64
# the trust-region state of the device-side step logic (csrc/common.hpp: TR_*) and its reduced scalars (SC_*), as the test entry points
# covgpu_solve_resident_traced / covgpu_tail_logic_probe hand them over
TR_NAMES = ("RADIUS", "MU", "LMDF", "COST", "ALPHA", "GG", "GN2", "GDOT", "DNORM", "CG", "CN", "MODEL", "SN", "RHO", "COSTNEW", "OK", "VALID", "ACC",
            "TERM", "FNCONV", "RETRY", "FIRST", "INITCOST", "REUSE", "JA", "JB", "JC", "VV", "VG", "NN", "XN2")
SC_NAMES = ("COST", "JV2", "GG", "GN2", "GDOT", "GMAX", "GS", "SN2", "XN2", "VV", "VG", "NN", "JA", "JB", "JC")
TR_COUNT, SC_COUNT = 32, 16
TR = {k: i for i, k in enumerate(TR_NAMES)}
SC = {k: i for i, k in enumerate(SC_NAMES)}
TAIL_LOGIC, TAIL_FINISH, TR_AFTER_SOLVE, TR_AFTER_MODEL, TR_DECIDE = 0, 1, 2, 3, 4   # covgpu_tail_logic_probe: kernel

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_bp = C.POINTER(C.c_uint8)


class Options(C.Structure):
    _fields_ = [
        ("strategy", C.c_int32), ("max_iterations", C.c_int32), ("visual_only", C.c_int32), ("device", C.c_int32),
        ("reproj_loss_a", C.c_double), ("initial_radius", C.c_double), ("max_radius", C.c_double),
        ("min_relative_decrease", C.c_double), ("function_tolerance", C.c_double),
        ("parameter_tolerance", C.c_double), ("gradient_tolerance", C.c_double),
        ("sigma_a", C.c_double), ("sigma_g", C.c_double), ("sigma_aw", C.c_double), ("sigma_gw", C.c_double),
        ("gravity", C.c_double), ("verbose", C.c_int32), ("shard_policy", C.c_int32),
    ]


class ProblemStruct(C.Structure):
    _fields_ = [
        ("num_kf", C.c_int32), ("num_cam", C.c_int32), ("num_lm", C.c_int32), ("num_obs", C.c_int32),
        ("num_imu", C.c_int32), ("num_edge", C.c_int32), ("num_imu_samples", C.c_int32), ("reserved", C.c_int32),
        ("kf_pose", _dp), ("kf_speed_bias", _dp), ("kf_fixed", _bp), ("kf_cam", _ip),
        ("cam_extr", _dp), ("cam_intr", _dp), ("cam_dist", _dp), ("cam_dist_type", _ip),
        ("lm_pos", _dp), ("lm_obs_ptr", _ip), ("obs_kf", _ip), ("obs_uv", _dp), ("obs_sigma", _dp),
        ("imu_kf_i", _ip), ("imu_kf_j", _ip), ("imu_sample_ptr", _ip), ("imu_samples", _dp), ("imu_first", _dp), ("imu_noise", _dp),
        ("edge_i", _ip), ("edge_j", _ip), ("edge_meas", _dp), ("edge_sqrt_info", _dp), ("edge_loss_a", _dp),
    ]


class ProblemStructCam(ProblemStruct):
    """covgpu_problem as include/covgpu.h declares it: the ProblemStruct fields (the layout from before camera models, unchanged) plus the
    two camera-model fields appended at its end. FlatProblem.as_struct always builds this one, so the library never reads past the
    struct it is handed; it passes wherever a POINTER(ProblemStruct) is declared."""
    _fields_ = [("cam_model", _ip), ("cam_xi", _dp)]


class RelposeBatch(C.Structure):
    _fields_ = [("num_pairs", C.c_int32), ("corr_ptr", _ip), ("p_b", _dp), ("p_a", _dp), ("kp_a", _dp), ("kp_b", _dp), ("sigma_a", _dp),
                ("sigma_b", _dp), ("cam_a", _dp), ("cam_b", _dp), ("dist_type_a", _ip), ("dist_type_b", _ip), ("T_ab", _dp), ("outlier", _bp),
                ("inliers", _ip), ("cam_model_a", _ip), ("cam_model_b", _ip), ("xi_a", _dp), ("xi_b", _dp)]


class Result(C.Structure):
    _fields_ = [
        ("iterations", C.c_int32), ("accepted", C.c_int32), ("termination", C.c_int32), ("reserved", C.c_int32),
        ("initial_cost", C.c_double), ("final_cost", C.c_double), ("t_upload_s", C.c_double),
        ("t_solve_s", C.c_double), ("t_download_s", C.c_double), ("t_linear_solve_s", C.c_double),
        ("cost_trace", C.c_double * COVGPU_MAX_TRACE), ("radius_trace", C.c_double * COVGPU_MAX_TRACE),
        ("accepted_trace", C.c_int32 * COVGPU_MAX_TRACE),
    ]


class TwoRound(C.Structure):
    """covgpu_two_round (include/covgpu.h): parameters of the second round of a GlobalBundleAdjustment call."""
    _fields_ = [("outlier_threshold", C.c_double), ("round1_iterations", C.c_int32), ("use_loops_round2", C.c_int32),
                ("loop_loss_round2", C.c_double), ("kf_fixed_round2", C.POINTER(C.c_uint8))]


def _f64(a, shape):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(shape))
    return a


def _i32(a, shape):
    return np.ascontiguousarray(np.asarray(a, dtype=np.int32).reshape(shape))


@dataclass
class FlatProblem:
    """Flat IR of one GBA / PGO call. Arrays are float64 / int32 / uint8, C-contiguous."""
    kf_pose: np.ndarray                 # [K,7]
    kf_speed_bias: np.ndarray           # [K,9]
    kf_fixed: np.ndarray                # [K] uint8
    kf_cam: np.ndarray                  # [K]
    cam_extr: np.ndarray                # [A,7]
    cam_intr: np.ndarray                # [A,4]
    cam_dist: np.ndarray                # [A,4]
    cam_dist_type: np.ndarray           # [A]
    lm_pos: np.ndarray = field(default_factory=lambda: np.zeros((0, 3)))
    lm_obs_ptr: np.ndarray = field(default_factory=lambda: np.zeros(1, np.int32))
    obs_kf: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int32))
    obs_uv: np.ndarray = field(default_factory=lambda: np.zeros((0, 2)))
    obs_sigma: np.ndarray = field(default_factory=lambda: np.zeros(0))
    imu_kf_i: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int32))
    imu_kf_j: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int32))
    imu_sample_ptr: np.ndarray = field(default_factory=lambda: np.zeros(1, np.int32))
    imu_samples: np.ndarray = field(default_factory=lambda: np.zeros((0, 7)))
    imu_first: np.ndarray = field(default_factory=lambda: np.zeros((0, 6)))
    imu_noise: Optional[np.ndarray] = None   # [I,5] sigma_a sigma_g sigma_aw sigma_gw gravity per factor; None -> options
    edge_i: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int32))
    edge_j: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int32))
    edge_meas: np.ndarray = field(default_factory=lambda: np.zeros((0, 7)))
    edge_sqrt_info: np.ndarray = field(default_factory=lambda: np.zeros((0, 36)))
    edge_loss_a: np.ndarray = field(default_factory=lambda: np.zeros(0))
    # camera models: None (the default, and what every pinhole-only map keeps) = every camera pinhole. Otherwise [A] COVGPU_CAM_* and
    # [A] xi of the unified rows. A None field is not an instance attribute at all (__post_init__ drops it; reads see the class default
    # None): walks over __dict__ — the golden input digests, field-by-field comparisons, copy() — see a pinhole problem exactly as before.
    cam_model: Optional[np.ndarray] = None
    cam_xi: Optional[np.ndarray] = None

    def __post_init__(self):
        K = np.asarray(self.kf_pose).reshape(-1, 7).shape[0]
        A = np.asarray(self.cam_extr).reshape(-1, 7).shape[0]
        self.kf_pose = _f64(self.kf_pose, (K, 7))
        self.kf_speed_bias = _f64(self.kf_speed_bias, (K, 9))
        self.kf_fixed = np.ascontiguousarray(np.asarray(self.kf_fixed, dtype=np.uint8).reshape(K))
        self.kf_cam = _i32(self.kf_cam, (K,))
        self.cam_extr = _f64(self.cam_extr, (A, 7))
        self.cam_intr = _f64(self.cam_intr, (A, 4))
        self.cam_dist = _f64(self.cam_dist, (A, 4))
        self.cam_dist_type = _i32(self.cam_dist_type, (A,))
        self.lm_pos = _f64(self.lm_pos, (-1, 3))
        self.lm_obs_ptr = _i32(self.lm_obs_ptr, (-1,))
        self.obs_kf = _i32(self.obs_kf, (-1,))
        self.obs_uv = _f64(self.obs_uv, (-1, 2))
        self.obs_sigma = _f64(self.obs_sigma, (-1,))
        self.imu_kf_i = _i32(self.imu_kf_i, (-1,))
        self.imu_kf_j = _i32(self.imu_kf_j, (-1,))
        self.imu_sample_ptr = _i32(self.imu_sample_ptr, (-1,))
        self.imu_samples = _f64(self.imu_samples, (-1, 7))
        self.imu_first = _f64(self.imu_first, (-1, 6))
        if self.imu_noise is not None:
            self.imu_noise = _f64(self.imu_noise, (-1, 5))
        self.edge_i = _i32(self.edge_i, (-1,))
        self.edge_j = _i32(self.edge_j, (-1,))
        self.edge_meas = _f64(self.edge_meas, (-1, 7))
        self.edge_sqrt_info = _f64(self.edge_sqrt_info, (-1, 36))
        self.edge_loss_a = _f64(self.edge_loss_a, (-1,))
        for name, conv in (("cam_model", _i32), ("cam_xi", _f64)):
            if getattr(self, name) is None:
                self.__dict__.pop(name, None)
            else:
                setattr(self, name, conv(getattr(self, name), (A,)))
        self.validate()

    # sizes
    @property
    def K(self): return self.kf_pose.shape[0]
    @property
    def A(self): return self.cam_extr.shape[0]
    @property
    def L(self): return self.lm_pos.shape[0]
    @property
    def O(self): return self.obs_kf.shape[0]
    @property
    def I(self): return self.imu_kf_i.shape[0]
    @property
    def E(self): return self.edge_i.shape[0]

    def validate(self):
        K, L, O, I, E = self.K, self.L, self.O, self.I, self.E
        assert self.lm_obs_ptr.shape[0] == L + 1 and self.lm_obs_ptr[0] == 0 and self.lm_obs_ptr[-1] == O
        assert np.all(np.diff(self.lm_obs_ptr) >= 0)
        assert self.obs_uv.shape[0] == O and self.obs_sigma.shape[0] == O
        if O:
            assert self.obs_kf.min() >= 0 and self.obs_kf.max() < K
            # one observation per (landmark, keyframe), as the library's validation: the pair lists skip a keyframe paired with itself
            obs_lm = np.repeat(np.arange(L, dtype=np.int64), np.diff(self.lm_obs_ptr))
            assert np.unique(obs_lm * K + self.obs_kf).shape[0] == O, "landmark observed twice by one keyframe"
        assert self.kf_cam.min() >= 0 and self.kf_cam.max() < self.A
        assert self.imu_kf_j.shape[0] == I and self.imu_sample_ptr.shape[0] == I + 1 and self.imu_first.shape[0] == I
        assert self.imu_sample_ptr[-1] == self.imu_samples.shape[0]
        assert self.imu_noise is None or self.imu_noise.shape[0] == I
        if I: assert min(self.imu_kf_i.min(), self.imu_kf_j.min()) >= 0 and max(self.imu_kf_i.max(), self.imu_kf_j.max()) < K
        assert self.edge_j.shape[0] == E and self.edge_meas.shape[0] == E and self.edge_sqrt_info.shape[0] == E
        assert self.edge_loss_a.shape[0] == E
        if E: assert min(self.edge_i.min(), self.edge_j.min()) >= 0 and max(self.edge_i.max(), self.edge_j.max()) < K
        # (cam_model / cam_xi are checked by the library: an invalid model or xi is COVGPU_ERR_INVALID_ARG there, and tests pass such rows on purpose)

    def copy(self) -> "FlatProblem":
        return FlatProblem(**{k: (None if v is None else np.array(v, copy=True)) for k, v in self.__dict__.items()})

    def as_struct(self) -> ProblemStructCam:
        """C view of the arrays (no copies; keep `self` alive while the struct is in use)."""
        s = ProblemStructCam()
        s.num_kf, s.num_cam, s.num_lm, s.num_obs = self.K, self.A, self.L, self.O
        s.num_imu, s.num_edge, s.num_imu_samples = self.I, self.E, self.imu_samples.shape[0]
        for name, ctype in ProblemStruct._fields_ + ProblemStructCam._fields_:
            if name.startswith("num_") or name == "reserved":
                continue
            arr = getattr(self, name)
            setattr(s, name, None if arr is None else arr.ctypes.data_as(ctype))
        return s


class AbsposeBatch(C.Structure):
    _fields_ = [("num", C.c_int32), ("corr_ptr", _ip), ("bearing", _dp), ("point_w", _dp), ("sigma_angle", _dp), ("seed", C.POINTER(C.c_uint64)),
                ("T_wc", _dp), ("inlier", _bp), ("inliers", _ip), ("iterations", _ip), ("best_draw", _ip)]


class RansacOpts(C.Structure):
    _fields_ = [("min_inliers", C.c_int32), ("max_iterations", C.c_int32), ("probability", C.c_double), ("threshold", C.c_double),
                ("seed", C.c_uint64)]


class FiveptBatch(C.Structure):
    _fields_ = [("num", C.c_int32), ("corr_ptr", _ip), ("bearing1", _dp), ("bearing2", _dp), ("seed", C.POINTER(C.c_uint64)),
                ("T_12", _dp), ("inlier", _bp), ("inliers", _ip), ("status", _ip), ("iterations", _ip), ("best_draw", _ip)]


class NcrelposeBatch(C.Structure):
    _fields_ = [("num", C.c_int32), ("cells", C.c_int32), ("corr_ptr", _ip), ("cell_ptr", _ip), ("bearing1", _dp), ("bearing2", _dp),
                ("cam1", _ip), ("cam2", _ip), ("cam_ptr", _ip), ("cam", _dp), ("T_sc_q", _dp), ("T_sc_c", _dp), ("seed", C.POINTER(C.c_uint64)),
                ("T_c1c2", _dp), ("T_c1c2_ransac", _dp), ("T_s1s2", _dp), ("cov", _dp), ("inlier", _bp), ("inliers", _ip), ("status", _ip),
                ("iterations", _ip), ("best_draw", _ip), ("cov_rows", _ip), ("cov_draws", _ip)]


class NcrelposeOpts(C.Structure):
    _fields_ = [("rp_error", C.c_double), ("rp_error_cov", C.c_double), ("min_inliers", C.c_int32), ("max_iterations", C.c_int32),
                ("cov_thres", C.c_double), ("cov_iters", C.c_int32), ("cov_max_iters", C.c_int32), ("probability", C.c_double),
                ("seed", C.c_uint64), ("stage_cap", C.c_int32)]


class FiveptOpts(C.Structure):
    _fields_ = [("min_inliers", C.c_int32), ("max_iterations", C.c_int32), ("probability", C.c_double), ("threshold", C.c_double),
                ("sigma", C.c_double), ("seed", C.c_uint64)]


FIVEPT_FOUND, FIVEPT_TOO_FEW, FIVEPT_NO_MODEL, FIVEPT_FEW_INLIERS, FIVEPT_MAX_ITERATIONS = range(5)   # include/covgpu.h

MATCH_DENSE, MATCH_KNN2, MATCH_MAX_ROWS = 0, 1, 4096   # include/covgpu.h


class MatchBatch(C.Structure):
    _fields_ = [("num_sets", C.c_int32), ("row_ptr", _ip), ("desc", _bp), ("skip", _bp), ("num_jobs", C.c_int32), ("set_a", _ip), ("set_b", _ip),
                ("match", _ip), ("dist", _ip), ("nmatches", _ip)]


class MatchOpts(C.Structure):
    _fields_ = [("mode", C.c_int32), ("dist_threshold", C.c_float), ("ratio", C.c_float)]


GUIDED_SE3, GUIDED_PROJECTION = 0, 1   # include/covgpu.h
_fp = C.POINTER(C.c_float)


class MatchFloatBatch(C.Structure):
    """covgpu_match_float_batch_t (include/covgpu.h): L2 matching of float (SIFT) descriptors, DESIGN.md §4.17."""
    _fields_ = [("num_sets", C.c_int32), ("row_ptr", _ip), ("dim", C.c_int32), ("desc", _fp), ("num_jobs", C.c_int32), ("set_a", _ip),
                ("set_b", _ip), ("match", _ip), ("dist", _fp), ("nmatches", _ip)]


class GuidedOpts(C.Structure):
    _fields_ = [("th_low", C.c_int32), ("radius", C.c_double), ("scale_factor", C.c_double), ("num_octaves", C.c_int32),
                ("agreement", C.c_int32)]


class KeypointSets(C.Structure):
    _fields_ = [("num_sets", C.c_int32), ("row_ptr", _ip), ("kp", _fp), ("level", _ip), ("desc", _bp), ("bounds", _dp), ("grid_inv", _dp)]


class SearchSe3Batch(C.Structure):
    _fields_ = [("sets", KeypointSets), ("K", _dp), ("lm_pos", _dp), ("lm_max_distance", _dp), ("lm_desc", _bp), ("lm_free", _bp),
                ("num_jobs", C.c_int32), ("set_1", _ip), ("set_2", _ip), ("T12", _dp), ("match", _ip), ("match1", _ip), ("match2", _ip),
                ("nfound", _ip)]


class SearchProjectionBatch(C.Structure):
    _fields_ = [("sets", KeypointSets), ("taken", _bp), ("cam", _dp), ("dist_type", _ip), ("cam_model", _ip), ("xi", _dp),
                ("num_jobs", C.c_int32), ("set", _ip), ("T_cw", _dp), ("point_ptr", _ip), ("p_w", _dp), ("normal", _dp),
                ("min_distance", _dp), ("max_distance", _dp), ("p_desc", _bp), ("skip", _bp), ("existing_idx", _ip),
                ("claimed", _ip), ("remap_to", _ip), ("best_dist", _ip), ("nmatches", _ip)]


BOW_L1_NORM = 0                                   # include/covgpu.h (DBoW2::ScoringType / WeightingType)
BOW_TF_IDF, BOW_TF, BOW_IDF, BOW_BINARY = 0, 1, 2, 3
DETECT_COVINS, DETECT_COVINS_G = 0, 1
_lp = C.POINTER(C.c_int64)


class BowVocab(C.Structure):
    _fields_ = [("num_nodes", C.c_int32), ("num_words", C.c_int32), ("k", C.c_int32), ("L", C.c_int32), ("scoring", C.c_int32),
                ("weighting", C.c_int32), ("parent", _ip), ("child_ptr", _ip), ("child", _ip), ("desc", _bp), ("word_id", _ip),
                ("weight", _dp)]


class BowTransformBatch(C.Structure):
    _fields_ = [("num_sets", C.c_int32), ("row_ptr", _ip), ("desc", _bp), ("levelsup", C.c_int32), ("capacity", C.c_int32),
                ("bow_ptr", _ip), ("word", _ip), ("value", _dp), ("total", _lp), ("row_word", _ip), ("row_node", _ip)]


class DetectOpts(C.Structure):
    _fields_ = [("min_score_factor", C.c_double), ("min_loop_dist", C.c_int32), ("exclude_kfs_with_id_less_than", C.c_int32),
                ("inter_map_matches_only", C.c_int32), ("scratch_kib", C.c_int32)]


class DetectBatch(C.Structure):
    _fields_ = [("num_kf", C.c_int32), ("id", _ip), ("client", _ip), ("bow_ptr", _ip), ("word", _ip), ("value", _dp), ("nb_ptr", _ip),
                ("nb", _ip), ("invalid", _bp), ("num_db", C.c_int32), ("db_order", _ip), ("num_queries", C.c_int32), ("query_kf", _ip),
                ("db_visible", _ip), ("min_score_in", _dp), ("cap", C.c_int32), ("num_candidates", _ip), ("candidates", _ip),
                ("acc_score", _fp), ("min_score", _dp), ("num_sharing", _ip), ("max_common_words", _ip), ("num_scored", _ip)]


class BowDbOpts(C.Structure):
    """covgpu_bowdb_opts (include/covgpu.h): the resident keyframe database, DESIGN.md §4.16."""
    _fields_ = [("detect", DetectOpts), ("levelsup", C.c_int32), ("tail_limit", C.c_int32), ("reserve_kf", C.c_int32),
                ("reserve_words", C.c_int32), ("num_words", C.c_int32)]


class BowDbQuery(C.Structure):
    _fields_ = [("num_queries", C.c_int32), ("query_slot", _ip), ("con_ptr", _ip), ("con", _ip), ("min_score_in", _dp), ("cap", C.c_int32),
                ("num_candidates", _ip), ("candidates", _ip), ("acc_score", _fp), ("min_score", _dp), ("num_sharing", _ip),
                ("max_common_words", _ip), ("num_scored", _ip)]


BOWDB_STATS = ("stored", "live", "positions", "base_postings", "tail", "rebuilds", "h2d_bytes", "d2h_bytes", "device_bytes", "pool_used",
               "pool_dead", "slot_capacity", "position_capacity", "pool_capacity", "growths")   # covgpu_bowdb_stats out[0..14]


class PruneBatch(C.Structure):
    """covgpu_prune_t (include/covgpu.h): Map::RemoveRedundantData as one call, DESIGN.md §4.14."""
    _fields_ = [("num_kf", C.c_int32), ("num_lm", C.c_int32), ("lm_obs_ptr", _ip), ("obs_kf", _ip), ("lm_invalid", _bp), ("kf_invalid", _bp),
                ("kf_first", _bp), ("kf_loop", _bp), ("kf_not_erase", _bp), ("kf_pred", _ip), ("kf_succ", _ip), ("kf_time", _dp),
                ("capacity", C.c_int32), ("round_kf", _ip), ("round_action", _ip), ("num_rounds", _ip), ("removed", _ip), ("stop_reason", _ip),
                ("kf_pred_out", _ip), ("kf_succ_out", _ip), ("lm_nobs", _ip), ("red_num", _ip), ("red_den", _ip), ("loop_ms", _dp)]


class PruneOpts(C.Structure):
    _fields_ = [("th_red", C.c_double), ("max_time_dist", C.c_double), ("max_kfs", C.c_int32), ("max_rounds", C.c_int32)]


class LandmarkRefresh(C.Structure):
    """covgpu_landmark_refresh_t (include/covgpu.h): Landmark::ComputeDescriptor + UpdateNormal for every landmark, DESIGN.md §4.15."""
    _fields_ = [("num_kf", C.c_int32), ("num_lm", C.c_int32), ("lm_obs_ptr", _ip), ("obs_kf", _ip), ("obs_desc", _bp), ("obs_octave", _ip),
                ("lm_ref_obs", _ip), ("lm_pos", _dp), ("kf_center", _dp), ("kf_invalid", _bp), ("lm_invalid", _bp),
                ("lm_desc_obs", _ip), ("lm_desc", _bp), ("lm_normal", _dp), ("lm_min_distance", _dp), ("lm_max_distance", _dp),
                ("lm_status", _ip), ("form_count", _ip), ("kernel_ms", _dp)]


class LandmarkRefreshOpts(C.Structure):
    _fields_ = [("scale_factor", C.c_double), ("num_octaves", C.c_int32)]


LMR_NO_OBSERVER, LMR_NO_REFERENCE, LMR_INVALID = 1, 2, 4                                         # lm_status bits
LMR_FORMS = 6                                                                                    # form_count: 4, 8, 16, 32, 64 lanes, long


class VocTrain(C.Structure):
    """covgpu_voc_train_t (include/covgpu.h): TemplatedVocabulary::create, DESIGN.md §4.18."""
    _fields_ = [("num_sets", C.c_int32), ("row_ptr", _ip), ("desc", _bp), ("node_capacity", C.c_int32), ("num_nodes", _ip),
                ("num_words", _ip), ("parent", _ip), ("desc_out", _bp), ("word_id", _ip), ("weight", _dp), ("row_word", _ip),
                ("stats", _lp)]


class VocTrainOpts(C.Structure):
    _fields_ = [("k", C.c_int32), ("L", C.c_int32), ("weighting", C.c_int32), ("scoring", C.c_int32), ("seed", C.c_uint64),
                ("max_iterations", C.c_int32), ("scratch_kib", C.c_int32)]


VOCTRAIN_STATS = ("iterations", "max_node_iterations", "nodes_at_cap", "emptied_clusters", "short_seeded_nodes", "levels", "h2d_bytes",
                  "d2h_bytes")                                                                   # covgpu_voc_train_t::stats[0..7]


class Marginal(C.Structure):
    """covgpu_marginal_t (include/covgpu.h): marginal covariances of selected keyframes, DESIGN.md §4.19."""
    _fields_ = [("num_kf", C.c_int32), ("kf", _ip), ("block", C.c_int32), ("mu", C.c_double), ("cov", _dp), ("stats", _lp)]


MARGINAL_STATS = ("columns", "fronts", "launches", "mfma_launches", "vector_launches", "scratch_bytes", "reserved6", "reserved7")


class Selinv(C.Structure):
    """covgpu_selinv_t (include/covgpu.h): covariance of every keyframe by selected inversion of the factor, DESIGN.md §4.20."""
    _fields_ = [("block", C.c_int32), ("mu", C.c_double), ("kf_cov", _dp), ("num_pairs", C.c_int64), ("pair_i", _ip), ("pair_j", _ip),
                ("pair_cov", _dp), ("pair_ok", _bp), ("stats", _lp)]


SELINV_STATS = ("fronts", "levels", "launches", "mfma_launches", "vector_launches", "scratch_bytes", "pairs_served", "reserved7")


class Lmcov(C.Structure):
    """covgpu_lmcov_t (include/covgpu.h): covariance of every landmark from the selected inverse of the factor, DESIGN.md §4.21."""
    _fields_ = [("mu", C.c_double), ("lm_cov", _dp), ("lm_ok", _bp), ("kf_cov", _dp), ("stats", _lp)]


LMCOV_STATS = ("fronts", "levels", "sweep_launches", "landmark_launches", "group_width", "scratch_bytes", "pairs_resolved", "landmarks_not_ok")


class Obscov(C.Structure):
    """covgpu_obscov_t (include/covgpu.h): covariance of every observation and its pose-landmark cross block, DESIGN.md §4.22."""
    _fields_ = [("mu", C.c_double), ("obs_cov", _dp), ("cross_cov", _dp), ("obs_res", _dp), ("obs_ok", _bp), ("lm_cov", _dp), ("lm_ok", _bp),
                ("kf_cov", _dp), ("stats", _lp)]


OBSCOV_STATS = ("fronts", "levels", "sweep_launches", "observation_launches", "group_width", "scratch_bytes", "observations_not_ok",
                "constant_observers")


PRUNE_ERASED, PRUNE_TIME_GATE, PRUNE_LOOP_KF, PRUNE_NOT_ERASE = 0, 1, 2, 3                       # round_action
PRUNE_STOP_NO_CANDIDATES, PRUNE_STOP_THRESHOLD, PRUNE_STOP_MAX_KFS, PRUNE_STOP_MAX_ROUNDS = 0, 1, 2, 3   # stop_reason


def declare(lib: C.CDLL, prefix: str) -> None:
    """Attach argtypes/restype for the entry points shared by libcovgpu (prefix 'covgpu_', with a context
    argument) and — test side only — the oracle (prefix 'covo_', no context)."""
    ctx = [C.c_void_p] if prefix == "covgpu_" else []
    OP, PP, RP = C.POINTER(Options), C.POINTER(ProblemStruct), C.POINTER(Result)

    def d(name, args, res=C.c_int):
        fn = getattr(lib, prefix + name)
        fn.argtypes, fn.restype = args, res

    d("default_options", [OP], None)
    d("gba_solve", ctx + [OP, PP, RP])
    d("pgo_solve", ctx + [OP, PP, RP])
    d("reprojection_residual_norms", ctx + [OP, PP, _dp])
    d("linearize_reprojection", ctx + [OP, PP, _dp, _dp, _dp, _dp])
    d("preintegrate", ctx + [OP, PP, _dp, _dp, _dp])
    d("linearize_imu", ctx + [OP, PP, _dp, _dp])
    d("linearize_between", ctx + [OP, PP, _dp, _dp, _dp])
    d("pgo_reanchor", ctx + [C.c_int32, _dp, _dp, _dp, C.c_int32, _ip, _dp])
    d("reduced_dim", [OP, PP], C.c_int32)
    if prefix == "covgpu_":
        d("create", [OP, C.POINTER(C.c_void_p)])
        d("destroy", [C.c_void_p], None)
        d("last_error", [], C.c_char_p)
        d("upload", [C.c_void_p, OP, PP])
        d("solve_resident", [C.c_void_p, OP, RP])
        d("download", [C.c_void_p, PP])
        d("schur", [C.c_void_p, OP, PP, C.c_double, _dp, _dp, _dp])
        d("solve_reduced", [C.c_void_p, C.c_int32, _dp, _dp, _dp])
        d("pgo_partition", [C.c_int32, C.c_int32, _ip, _ip, _ip], C.c_int32)
        d("lm_group", [C.c_int64, C.c_int32], C.c_int32)
        d("gn_step", [C.c_void_p, OP, PP, C.c_double, _dp, _dp, _dp])
        d("solve_resident_traced", [C.c_void_p, OP, RP, _dp, C.c_int32, _ip])
        d("fetch_tail_state", [C.c_void_p, _dp, _dp, _dp, _dp, _dp, _dp, _dp])
        d("tail_logic_probe", [C.c_void_p, OP, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _dp, _dp, _dp, C.c_int32])
        d("relpose_batch", [C.c_void_p, C.POINTER(RelposeBatch), C.c_double, C.c_int32])
        d("default_ransac_opts", [C.POINTER(RansacOpts)], None)
        d("abspose_ransac_batch", [C.c_void_p, C.POINTER(AbsposeBatch), C.POINTER(RansacOpts)])
        d("p3p_batch", [C.c_void_p, C.c_int32, _dp, _dp, _dp, _ip, _ip])
        d("default_fivept_opts", [C.POINTER(FiveptOpts)], None)
        d("fivept_limits", [_ip], None)
        d("fivept_check", [C.POINTER(FiveptBatch), C.POINTER(FiveptOpts)])
        d("fivept_ransac_batch", [C.c_void_p, C.POINTER(FiveptBatch), C.POINTER(FiveptOpts)])
        d("fivept_solve_batch", [C.c_void_p, C.c_int32, _dp, _dp, _dp, _ip, _dp, _ip])
        d("default_ncrelpose_opts", [C.POINTER(NcrelposeOpts)], None)
        d("ncrelpose_limits", [_ip], None)
        d("ncrelpose_check", [C.POINTER(NcrelposeBatch), C.POINTER(NcrelposeOpts)])
        d("ncrelpose_batch", [C.c_void_p, C.POINTER(NcrelposeBatch), C.POINTER(NcrelposeOpts)])
        d("ncrelpose_solve_batch", [C.c_void_p, C.c_int32, C.c_int32, _dp, _dp, _dp, _ip, _dp])
        d("default_match_opts", [C.POINTER(MatchOpts), C.c_int32], None)
        d("match_batch", [C.c_void_p, C.POINTER(MatchBatch), C.POINTER(MatchOpts)])
        d("default_match_float_opts", [C.POINTER(MatchOpts)], None)
        d("match_float_limits", [_ip], None)
        d("match_float_batch", [C.c_void_p, C.POINTER(MatchFloatBatch), C.POINTER(MatchOpts)])
        d("match_float_check", [C.POINTER(MatchFloatBatch), C.POINTER(MatchOpts)])
        d("default_guided_opts", [C.POINTER(GuidedOpts), C.c_int32], None)
        d("search_se3_batch", [C.c_void_p, C.POINTER(SearchSe3Batch), C.POINTER(GuidedOpts)])
        d("search_projection_batch", [C.c_void_p, C.POINTER(SearchProjectionBatch), C.POINTER(GuidedOpts)])
        d("bow_transform_batch", [C.c_void_p, C.POINTER(BowVocab), C.POINTER(BowTransformBatch)])
        d("bow_score_pairs", [C.c_void_p, C.c_int32, _ip, _ip, _dp, C.c_int32, _ip, _ip, _dp])
        d("default_detect_opts", [C.POINTER(DetectOpts), C.c_int32], None)
        d("detect_candidates_batch", [C.c_void_p, C.POINTER(DetectBatch), C.POINTER(DetectOpts)])
        d("default_bowdb_opts", [C.POINTER(BowDbOpts), C.c_int32], None)
        d("bowdb_create", [C.c_void_p, C.POINTER(BowVocab), C.POINTER(BowDbOpts), C.POINTER(C.c_void_p)])
        d("bowdb_destroy", [C.c_void_p], None)
        d("bowdb_put", [C.c_void_p, C.c_int32, _ip, _ip, _ip, _ip, _ip, _dp])
        d("bowdb_put_descriptors", [C.c_void_p, _ip, _ip, _ip, C.POINTER(BowTransformBatch)])
        d("bowdb_set_neighbours", [C.c_void_p, C.c_int32, _ip, _ip, _ip])
        d("bowdb_set_invalid", [C.c_void_p, C.c_int32, _ip, _bp])
        d("bowdb_add", [C.c_void_p, C.c_int32, _ip])
        d("bowdb_erase", [C.c_void_p, C.c_int32, _ip])
        d("bowdb_query", [C.c_void_p, C.POINTER(BowDbQuery)])
        d("bowdb_compact", [C.c_void_p])
        d("bowdb_order", [C.c_void_p, C.c_int32, _ip, _ip])
        d("bowdb_stats", [C.c_void_p, C.POINTER(C.c_int64)])
        d("default_prune_opts", [C.POINTER(PruneOpts)], None)
        d("prune_check", [C.POINTER(PruneBatch), C.POINTER(PruneOpts)])
        d("prune_redundant", [C.c_void_p, C.POINTER(PruneBatch), C.POINTER(PruneOpts)])
        d("default_landmark_refresh_opts", [C.POINTER(LandmarkRefreshOpts)], None)
        d("landmark_refresh_limits", [_ip], None)
        d("landmark_refresh_check", [C.POINTER(LandmarkRefresh), C.POINTER(LandmarkRefreshOpts)])
        d("landmark_refresh", [C.c_void_p, C.POINTER(LandmarkRefresh), C.POINTER(LandmarkRefreshOpts)])
        d("default_voc_train_opts", [C.POINTER(VocTrainOpts)], None)
        d("voc_train_limits", [_ip], None)
        d("voc_train_check", [C.POINTER(VocTrain), C.POINTER(VocTrainOpts)])
        d("voc_train", [C.c_void_p, C.POINTER(VocTrain), C.POINTER(VocTrainOpts)])
        d("marginal_limits", [_ip], None)
        d("marginal_check", [PP, OP, C.POINTER(Marginal)])
        d("marginal_covariance", [C.c_void_p, OP, PP, C.c_int32, C.POINTER(Marginal)])
        d("marginal_resident", [C.c_void_p, OP, C.POINTER(Marginal)])
        d("selinv_limits", [_ip], None)
        d("selinv_check", [PP, OP, C.POINTER(Selinv)])
        d("selected_inverse", [C.c_void_p, OP, PP, C.c_int32, C.POINTER(Selinv)])
        d("selected_inverse_resident", [C.c_void_p, OP, C.POINTER(Selinv)])
        d("lmcov_limits", [_ip], None)
        d("lmcov_check", [PP, OP, C.POINTER(Lmcov)])
        d("landmark_covariance", [C.c_void_p, OP, PP, C.POINTER(Lmcov)])
        d("landmark_covariance_resident", [C.c_void_p, OP, C.POINTER(Lmcov)])
        d("obscov_limits", [_ip], None)
        d("obscov_check", [PP, OP, C.POINTER(Obscov)])
        d("observation_covariance", [C.c_void_p, OP, PP, C.POINTER(Obscov)])
        d("observation_covariance_resident", [C.c_void_p, OP, C.POINTER(Obscov)])
        d("outlier_pass", [C.c_void_p, C.c_double, _bp, _ip, C.POINTER(C.c_int64)])
        d("covisibility", [C.c_void_p, C.c_int32, C.c_int64, _ip, _ip, _ip, C.POINTER(C.c_int64)])
        d("gba_solve_multi", [OP, PP, RP, C.c_int32, _ip, C.c_double, _bp, _ip, C.POINTER(C.c_int64)])
        d("gba_two_round_multi", [OP, PP, C.POINTER(TwoRound), C.c_int32, _ip, _bp, _ip, C.POINTER(C.c_int64), RP, RP])
        d("nd_plan_create", [OP, PP, C.c_int32, C.POINTER(C.c_void_p)])
        d("nd_plan_create_pgo", [OP, PP, C.c_int32, C.POINTER(C.c_void_p)])
        d("nd_plan_destroy", [C.c_void_p], None)
        d("nd_plan_info", [C.c_void_p, C.POINTER(C.c_int64)], None)
        d("nd_plan_arrays", [C.c_void_p, _ip, _ip, _ip, _ip, _ip, _ip], None)
        d("shard_plan", [OP, PP, C.c_int32, C.POINTER(C.c_void_p), _ip, _ip, _ip], C.c_int32)
        d("nd_plan_owner", [C.c_void_p, _ip, _ip], None)
        d("nd_plan_ranks", [C.c_void_p, _ip], None)
        d("nd_plan_rank_flops", [C.c_void_p, _dp], C.c_int32)
        d("nd_plan_exchange", [C.c_void_p, C.POINTER(C.c_int64)], None)
        d("group_create", [C.c_int32, C.POINTER(C.c_void_p)])
        d("group_destroy", [C.c_void_p], None)
        d("group_abort", [C.c_void_p], None)
        d("set_shard_group", [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p])
        d("rccl_unique_id", [_bp])
        d("set_shard_rccl", [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, _bp])
        d("set_shard_none", [C.c_void_p])
        d("allreduce_host", [C.c_void_p, _dp, C.c_int64, C.c_int32])
        d("shard_stats", [C.c_void_p, C.POINTER(C.c_int64)], None)


def dptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(_dp)


def iptr(a: np.ndarray):
    return a.ctypes.data_as(_ip)
