"""ctypes binding of the product library covins_amd/libcovgpu.so (C ABI: include/covgpu.h).

There is NO CPU fallback: if the HIP extension is missing or no MI355X is visible, every entry point raises.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import Optional, Tuple

import numpy as np

from . import capi
from .capi import FlatProblem, Options, Result, dptr, iptr

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "libcovgpu.so")
if os.environ.get("COVGPU_LIBRARY"):   # dev aid: another build of the library (compile-time A/B, tools/gpu_ab.sh)
    _SO = os.environ["COVGPU_LIBRARY"]
_LIB: Optional[C.CDLL] = None


class CovGpuError(RuntimeError):
    pass


# ---- what the batch wrappers share: coercion to the C ABI's array types, option structs, output offsets
def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _u8(a):
    return np.ascontiguousarray(a, dtype=np.uint8)


def _opt(coerce, a):
    """coerce(a), or None for an array the caller left out."""
    return None if a is None else coerce(a)


def _bp(a):
    return None if a is None else a.ctypes.data_as(capi._bp)


def _set_opts(o, allowed, opts, what, convert=None):
    """Sets the fields `opts` of the option struct `o` (already at its defaults); a name outside `allowed` is a TypeError."""
    for k, v in opts.items():
        if k not in allowed:
            raise TypeError(f"unknown {what} option {k}")
        setattr(o, k, v if convert is None else convert(k, v))
    return o


def _job_offsets(ptr, sets, ok):
    """[J+1] int64: the first output row of every job, job j writing one row per row of set sets[j] (zeros unless the indices are ok)."""
    off = np.zeros(len(sets) + 1, np.int64)
    if ok and len(sets):
        off[1:] = np.cumsum(np.maximum(ptr[sets + 1] - ptr[sets], 0))
    return off


_MATCH_MODES = {"dense": capi.MATCH_DENSE, "knn2": capi.MATCH_KNN2}
_DETECT_MODES = {"covins": capi.DETECT_COVINS, "covins_g": capi.DETECT_COVINS_G}
_DETECT_OPTS = ("min_score_factor", "min_loop_dist", "exclude_kfs_with_id_less_than", "inter_map_matches_only", "scratch_kib")


def build(force: bool = False) -> str:
    """Compiles the HIP sources for gfx950 (hipcc cross-compiles without a GPU)."""
    args = ["make", "-C", os.path.join(_HERE, "csrc"), "-j8"]
    if force:
        args.append("-B")
    subprocess.check_call(args, stdout=subprocess.DEVNULL)
    return _SO


def lib() -> C.CDLL:
    global _LIB
    if _LIB is None:
        if not os.path.exists(_SO):
            raise CovGpuError(f"{_SO} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(libcovgpu has no CPU fallback)")
        _LIB = C.CDLL(_SO)
        capi.declare(_LIB, "covgpu_")
        OP, PP = C.POINTER(Options), C.POINTER(capi.ProblemStruct)
        _LIB.covgpu_upload_pgo.argtypes = [C.c_void_p, OP, PP]
        _LIB.covgpu_schur_pgo.argtypes = [C.c_void_p, OP, PP, C.c_double, capi._dp, capi._dp, capi._dp]
        _LIB.covgpu_set_profiling.argtypes = [C.c_void_p, C.c_int]
        _LIB.covgpu_set_profiling.restype = None
        _LIB.covgpu_get_profile.argtypes = [C.c_void_p, capi._dp]
        _LIB.covgpu_get_profile.restype = None
        _LIB.covgpu_gba_two_round.argtypes = [C.c_void_p, OP, PP, C.POINTER(capi.TwoRound), capi._bp, C.POINTER(C.c_int32), C.POINTER(C.c_int64),
                                              C.POINTER(capi.Result), C.POINTER(capi.Result)]
        _LIB.covgpu_get_profile2.argtypes = [C.c_void_p, capi._dp]
        _LIB.covgpu_get_profile2.restype = None
        _LIB.covgpu_get_layout.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        _LIB.covgpu_get_layout.restype = None
        _LIB.covgpu_get_kernel_forms.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.c_int32]
        _LIB.covgpu_get_kernel_forms.restype = C.c_int
        _LIB.covgpu_kernel_form_name.argtypes = [C.c_int32]
        _LIB.covgpu_kernel_form_name.restype = C.c_char_p
    return _LIB


def pgo_partition(num_kf: int, edge_i, edge_j):
    """Host-only: block index per keyframe (-1 = border) and the number of blocks (0 = solved densely) of the
    block-arrow pose-graph solve (covgpu_pgo_partition, include/covgpu.h)."""
    import numpy as np
    ei = np.ascontiguousarray(edge_i, np.int32); ej = np.ascontiguousarray(edge_j, np.int32)
    out = np.empty(num_kf, np.int32)
    n = lib().covgpu_pgo_partition(num_kf, len(ei), ei.ctypes.data_as(capi._ip), ej.ctypes.data_as(capi._ip), out.ctypes.data_as(capi._ip))
    return out, int(n)


def lm_group(num_obs: int, num_lm: int) -> int:
    """Host-only: lanes per landmark (4 | 8 | 16) the landmark-major kernels take for O observations on L landmarks (covgpu_lm_group:
    the rule of the upload)."""
    return int(lib().covgpu_lm_group(int(num_obs), int(num_lm)))


def marginal_limits():
    """Host-only: {max_kf, max_cols, mfma_cols, panel_rows} of Context.marginal_covariance as the library was built (covgpu_marginal_limits)."""
    out = (C.c_int32 * 4)()
    lib().covgpu_marginal_limits(out)
    return dict(zip(("max_kf", "max_cols", "mfma_cols", "panel_rows"), (int(v) for v in out)))


def _quat_rot(q):
    x, y, z, w = (float(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def between_jacobian(pose_i, pose_j):
    """Host-only: the 6x12 Jacobian [d/d(dtheta_i, dp_i) | d/d(dtheta_j, dp_j)] of the SE3 between residual (R7: rotation rows first) at zero
    residual — the measurement is the relative pose of the two estimates itself — with unit weight and no loss, in A.1's tangent
    (q <- q * exp(dtheta), p <- p + dp). Poses are [qx, qy, qz, qw, px, py, pz] = T_w_s."""
    pi, pj = np.asarray(pose_i, np.float64), np.asarray(pose_j, np.float64)
    Ri, Rj = _quat_rot(pi[:4]), _quat_rot(pj[:4])
    t = Ri.T @ (pj[4:] - pi[4:])
    sk = np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])
    J = np.zeros((6, 12))
    J[:3, 0:3] = -(Rj.T @ Ri); J[:3, 6:9] = np.eye(3)
    J[3:, 0:3] = sk; J[3:, 3:6] = -Ri.T; J[3:, 9:12] = Ri.T
    return J


def relative_pose_covariance(cov12, pose_i, pose_j):
    """Host-only: covariance J cov12 J^T (6x6, rotation first, translation second: the order of LoopConstraint::cov_mat) of the relative pose
    T_si_sj of two keyframes from their joint pose covariance cov12 (12x12, Context.marginal_covariance(.., [i, j], block="pose")), J =
    between_jacobian(pose_i, pose_j)."""
    S = np.asarray(cov12, np.float64)
    if S.shape != (12, 12):
        raise ValueError("cov12 must be 12x12: the joint pose covariance of two keyframes")
    J = between_jacobian(pose_i, pose_j)
    out = J @ S @ J.T
    return 0.5 * (out + out.T)


def lmcov_limits():
    """Host-only: {max_group, threads, block_doubles} of Context.landmark_covariances as the library was built (covgpu_lmcov_limits)."""
    out = (C.c_int32 * 4)()
    lib().covgpu_lmcov_limits(out)
    return dict(max_group=int(out[0]), threads=int(out[1]), block_doubles=int(out[2]))


def obscov_limits():
    """Host-only: {max_group, threads, cross_doubles, block_doubles} of Context.observation_covariances as the library was built
    (covgpu_obscov_limits)."""
    out = (C.c_int32 * 4)()
    lib().covgpu_obscov_limits(out)
    return dict(max_group=int(out[0]), threads=int(out[1]), cross_doubles=int(out[2]), block_doubles=int(out[3]))


def fivept_limits():
    """Host-only: {stage_cap, hypotheses, sample, max_iterations} of Context.fivept_ransac_batch as the library was built
    (covgpu_fivept_limits): correspondences staged in LDS, hypotheses per pass, correspondences per draw, the largest max_iterations."""
    out = (C.c_int32 * 4)()
    lib().covgpu_fivept_limits(out)
    return dict(zip(("stage_cap", "hypotheses", "sample", "max_iterations"), (int(v) for v in out)))


def _fivept_args(bt: dict, opts: dict):
    """The structures of a five-point call and the arrays they point into (kept alive by the caller)."""
    o = capi.FiveptOpts()
    lib().covgpu_default_fivept_opts(C.byref(o))
    _set_opts(o, [name for name, _ in capi.FiveptOpts._fields_], opts, "five-point")
    ptr = _opt(_i32, bt.get("ptr"))
    B = len(ptr) - 1 if ptr is not None else int(bt.get("num", 0))
    Cn = int(ptr[-1]) if ptr is not None and len(ptr) else 0
    f1 = _opt(lambda a: _f64(a).reshape(-1, 3), bt.get("bearing1"))
    f2 = _opt(lambda a: _f64(a).reshape(-1, 3), bt.get("bearing2"))
    seed = _opt(lambda a: np.ascontiguousarray(a, dtype=np.uint64), bt.get("seed"))
    T = np.array(bt["T0"], dtype=np.float64, order="C").reshape(-1, 7) if bt.get("T0") is not None else np.zeros((max(B, 1), 7))
    mask = np.zeros(max(Cn, 1), np.uint8)
    inl, st, its, bd = (np.zeros(max(B, 1), np.int32) for _ in range(4))
    keep = dict(ptr=ptr, f1=f1, f2=f2, seed=seed, T=T, mask=mask, inl=inl, st=st, its=its, bd=bd, B=B, C=max(Cn, 0))
    s = capi.FiveptBatch(B, _opt(iptr, ptr), _opt(dptr, f1), _opt(dptr, f2), None if seed is None else seed.ctypes.data_as(C.POINTER(C.c_uint64)),
                         dptr(T), _bp(mask), iptr(inl), iptr(st), iptr(its), iptr(bd))
    return s, o, keep


def ncrelpose_limits():
    """Host-only: {stage_cap, hypotheses, sample, max_iterations, max_cells, max_cov_iters, max_rows, polish_steps} of
    Context.ncrelpose_batch as the library was built (covgpu_ncrelpose_limits)."""
    out = (C.c_int32 * 8)()
    lib().covgpu_ncrelpose_limits(out)
    return dict(zip(("stage_cap", "hypotheses", "sample", "max_iterations", "max_cells", "max_cov_iters", "max_rows", "polish_steps"), (int(v) for v in out)))


def _ncrelpose_args(bt: dict, opts: dict):
    """The structures of a 17-point call and the arrays they point into (kept alive by the caller)."""
    o = capi.NcrelposeOpts()
    lib().covgpu_default_ncrelpose_opts(C.byref(o))
    _set_opts(o, [name for name, _ in capi.NcrelposeOpts._fields_], opts, "17-point")
    ptr = _opt(_i32, bt.get("ptr"))
    B = len(ptr) - 1 if ptr is not None else int(bt.get("num", 0))
    Cn = int(ptr[-1]) if ptr is not None and len(ptr) else 0
    cell = _opt(_i32, bt.get("cell_ptr"))
    cells = int(bt["cells"]) if "cells" in bt else (cell.reshape(max(B, 1), -1).shape[1] - 1 if cell is not None and B > 0 else 0)
    f1 = _opt(lambda a: _f64(a).reshape(-1, 3), bt.get("bearing1"))
    f2 = _opt(lambda a: _f64(a).reshape(-1, 3), bt.get("bearing2"))
    c1, c2, cp = (_opt(_i32, bt.get(k)) for k in ("cam1", "cam2", "cam_ptr"))
    cam = _opt(lambda a: _f64(a).reshape(-1, 12), bt.get("cam"))
    Tq = _opt(lambda a: _f64(a).reshape(-1, 7), bt.get("T_sc_q"))
    Tc = _opt(lambda a: _f64(a).reshape(-1, 7), bt.get("T_sc_c"))
    seed = _opt(lambda a: np.ascontiguousarray(a, dtype=np.uint64), bt.get("seed"))
    fill = float(bt.get("fill", 0.0))                        # what untouched outputs hold
    T, Tr, Ts = (np.full((max(B, 1), 7), fill) for _ in range(3))
    cov = np.full((max(B, 1), 36), fill)
    mask = np.zeros(max(Cn, 1), np.uint8)
    inl, st, its, bd, cr, cd = (np.zeros(max(B, 1), np.int32) for _ in range(6))
    keep = dict(ptr=ptr, cell=cell, f1=f1, f2=f2, c1=c1, c2=c2, cp=cp, cam=cam, Tq=Tq, Tc=Tc, seed=seed, T=T, Tr=Tr, Ts=Ts, cov=cov, mask=mask,
                inl=inl, st=st, its=its, bd=bd, cr=cr, cd=cd, B=B, C=max(Cn, 0))
    s = capi.NcrelposeBatch(B, cells, _opt(iptr, ptr), _opt(iptr, cell), _opt(dptr, f1), _opt(dptr, f2), _opt(iptr, c1), _opt(iptr, c2), _opt(iptr, cp),
                            _opt(dptr, cam), _opt(dptr, Tq), _opt(dptr, Tc), None if seed is None else seed.ctypes.data_as(C.POINTER(C.c_uint64)),
                            dptr(T), dptr(Tr), dptr(Ts), dptr(cov), _bp(mask), iptr(inl), iptr(st), iptr(its), iptr(bd), iptr(cr), iptr(cd))
    return s, o, keep


def ncrelpose_check(bt: dict, **opts):
    """Host-only: the argument check of Context.ncrelpose_batch alone (covgpu_ncrelpose_check); raises CovGpuError with the message of
    the first violation. A key of `bt` that is absent is passed as a NULL array."""
    s, o, _keep = _ncrelpose_args(bt, opts)
    rc = lib().covgpu_ncrelpose_check(C.byref(s), C.byref(o))
    if rc != 0:
        raise CovGpuError(f"covgpu error {rc}: {lib().covgpu_last_error().decode()}")


def fivept_check(bt: dict, **opts):
    """Host-only: the argument check of Context.fivept_ransac_batch alone (covgpu_fivept_check); raises CovGpuError with the message
    of the first violation. A key of `bt` that is absent is passed as a NULL array."""
    s, o, _keep = _fivept_args(bt, opts)
    rc = lib().covgpu_fivept_check(C.byref(s), C.byref(o))
    if rc != 0:
        raise CovGpuError(f"covgpu error {rc}: {lib().covgpu_last_error().decode()}")


def selinv_limits():
    """Host-only: {mfma_rows, panel_cols, block_rows} of Context.keyframe_covariances as the library was built (covgpu_selinv_limits)."""
    out = (C.c_int32 * 4)()
    lib().covgpu_selinv_limits(out)
    return dict(zip(("mfma_rows", "panel_cols", "block_rows"), (int(v) for v in out)))


def relative_pose_covariances(kf_cov, pair_cov, pairs, poses, pair_ok=None):
    """Host-only: relative_pose_covariance of every served pair of Context.keyframe_covariances(.., block="pose", pairs=pairs): [P, 6, 6]
    from the diagonal blocks kf_cov [K, 6, 6], the cross blocks pair_cov [P, 6, 6] (rows of i, columns of j) and the poses [K, 7]. A pair
    that was not served (pair_ok[q] == 0) gives a block of NaN."""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    out = np.full((len(pairs), 6, 6), np.nan)
    for q, (i, j) in enumerate(pairs):
        if pair_ok is not None and not pair_ok[q]:
            continue
        c = np.empty((12, 12))
        c[:6, :6] = kf_cov[i][:6, :6]; c[6:, 6:] = kf_cov[j][:6, :6]
        c[:6, 6:] = pair_cov[q][:6, :6]; c[6:, :6] = pair_cov[q][:6, :6].T
        out[q] = relative_pose_covariance(c, poses[i], poses[j])
    return out


def kernel_form_names():
    """Names of the kernel forms Context.kernel_forms() counts, in the library's order."""
    n = lib().covgpu_get_kernel_forms(None, None, 0)
    return [lib().covgpu_kernel_form_name(i).decode() for i in range(n)]


def default_options(**kw) -> Options:
    o = Options()
    lib().covgpu_default_options(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def gba_two_round_multi(prob: FlatProblem, opt: Options, threshold: float, devices, round1_iterations: int = 5, use_loops_round2: bool = True,
                        loop_loss_round2: float = 1.0, kf_fixed_round2=None):
    """Both rounds of GlobalBundleAdjustment on len(devices) ranks behind one call (covgpu_gba_two_round_multi; ranks that share a device are virtual
    ranks on the library's in-process group). Returns what Context.gba_two_round returns."""
    q = prob.copy(); s = q.as_struct(); r1 = Result(); r2 = Result()
    erase = np.zeros(max(prob.O, 1), np.uint8); left = np.zeros(max(prob.L, 1), np.int32); cnt = (C.c_int64 * 2)()
    tr = capi.TwoRound()
    tr.outlier_threshold = float(threshold); tr.round1_iterations = int(round1_iterations); tr.use_loops_round2 = int(bool(use_loops_round2))
    tr.loop_loss_round2 = float(loop_loss_round2)
    fx = None
    if kf_fixed_round2 is not None:
        fx = np.ascontiguousarray(kf_fixed_round2, np.uint8)
        tr.kf_fixed_round2 = fx.ctypes.data_as(C.POINTER(C.c_uint8))
    dev = np.ascontiguousarray(devices, np.int32)
    rc = lib().covgpu_gba_two_round_multi(C.byref(opt), C.byref(s), C.byref(tr), len(dev), iptr(dev), erase.ctypes.data_as(capi._bp), iptr(left), cnt,
                                          C.byref(r1), C.byref(r2))
    if rc != 0:
        raise CovGpuError(f"covgpu error {rc}: {lib().covgpu_last_error().decode()}")
    return q, r1, r2, erase[:prob.O].astype(bool), left[:prob.L], (int(cnt[0]), int(cnt[1]))


class ConsistencyFilter:
    """The covisibility-consistency groups of PlaceRecognition::DetectLoop (placerec_be.cpp:391-460): sequential host state of one
    detector. feed(candidates, group_of) takes one query's loop candidates (Context.detect_candidates_batch) and returns
    mvpEnoughConsistentCandidates; group_of(k) gives candidate k's connected keyframes. `threshold` is cov_consistency_thres."""

    def __init__(self, threshold: int = 3):
        self.threshold = int(threshold)
        self.groups = []                       # mvConsistentGroups: (set of keyframes, consistency counter)

    def feed(self, candidates, group_of):
        if len(candidates) == 0:
            self.groups = []
            return []
        enough, current, taken = [], [], set()
        for cand in candidates:
            group = {int(k) for k in group_of(cand)}
            group.add(int(cand))
            hits = [g for g, (prev, _) in enumerate(self.groups) if not group.isdisjoint(prev)]
            for g in hits:
                if g not in taken:
                    taken.add(g)
                    current.append((group, self.groups[g][1] + 1))
            if any(self.groups[g][1] + 1 >= self.threshold for g in hits):
                enough.append(int(cand))
            if not hits:
                current.append((group, 0))
        self.groups = current
        return enough


class BowDb:
    """The resident keyframe database of one context (covgpu_bowdb): the vocabulary, the bow vectors and the inverted
    index stay on the device across calls. Keyframes are named by slots, dense non-negative numbers chosen by the caller. Made by
    Context.bowdb(); calls on one context are serialised by the caller."""

    def __init__(self, ctx: "Context", voc: Optional[dict] = None, mode="covins", **opts):
        self._ctx, self._h = ctx, C.c_void_p()
        o = capi.BowDbOpts()
        lib().covgpu_default_bowdb_opts(C.byref(o), int(_DETECT_MODES.get(mode, mode)))
        detect = {k: v for k, v in opts.items() if k in _DETECT_OPTS}
        _set_opts(o.detect, _DETECT_OPTS, detect, "bowdb")
        _set_opts(o, ("levelsup", "tail_limit", "reserve_kf", "reserve_words", "num_words"), {k: v for k, v in opts.items() if k not in detect},
                  "bowdb", lambda k, v: int(v))
        self.levelsup = int(o.levelsup)
        keep = []
        v = None if voc is None else C.byref(Context._bow_vocab(voc, keep))
        ctx._check(lib().covgpu_bowdb_create(ctx._h, v, C.byref(o), C.byref(self._h)))

    def _check(self, rc: int):
        self._ctx._check(rc)

    def close(self):
        if self._h and self._ctx._h:               # (a closed context has destroyed its databases)
            lib().covgpu_bowdb_destroy(self._h)
        self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _i32(a):
        return _i32(a).ravel()

    def _meta(self, slot, id, client):
        s, i, c = self._i32(slot), self._i32(id), self._i32(client)
        if len(i) != len(s) or len(c) != len(s):
            raise ValueError("slot, id and client differ in length")
        return s, i, c

    def put(self, slot, id, client, bow_ptr, word, value):
        """Stores vectors computed elsewhere: a bow CSR with one row per slot (covgpu_bowdb_put)."""
        s, i, c = self._meta(slot, id, client)
        ptr, w = self._i32(bow_ptr), self._i32(word)
        v = _f64(value).ravel()
        if len(ptr) != len(s) + 1 or len(v) != len(w) or (len(s) and int(ptr[-1]) > len(w)):
            raise ValueError("bow arrays do not fit the slots")
        self._check(lib().covgpu_bowdb_put(self._h, len(s), iptr(s), iptr(i), iptr(c), iptr(ptr), iptr(w), dptr(v)))

    def put_descriptors(self, slot, id, client, sets: dict, want: bool = False):
        """Transforms descriptor sets (row_ptr [S+1], desc [rows,32]) against the resident vocabulary and stores the vectors without a
        round trip (covgpu_bowdb_put_descriptors). want: also download them; returns what Context.bow_transform_batch returns."""
        s, i, c = self._meta(slot, id, client)
        ptr = self._i32(sets["row_ptr"])
        desc = _u8(sets["desc"]).reshape(-1, 32)
        S, rows = len(ptr) - 1, len(desc)
        if S != len(s) or (S > 0 and int(ptr[-1]) > rows):
            raise ValueError("descriptor sets do not fit the slots")
        bt = capi.BowTransformBatch(S, iptr(ptr), _bp(desc), self.levelsup, 0, None, None, None, None, None, None)
        if want:
            bptr = np.zeros(S + 1, np.int32); word = np.zeros(max(rows, 1), np.int32); value = np.zeros(max(rows, 1))
            rw = np.full(max(rows, 1), -1, np.int32); rn = np.zeros(max(rows, 1), np.int32); tot = C.c_int64(0)
            bt.capacity, bt.bow_ptr, bt.word, bt.value, bt.total = rows, iptr(bptr), iptr(word), dptr(value), C.pointer(tot)
            bt.row_word, bt.row_node = iptr(rw), iptr(rn)
        self._check(lib().covgpu_bowdb_put_descriptors(self._h, iptr(s), iptr(i), iptr(c), C.byref(bt)))
        if want:
            n = int(tot.value)
            return dict(bow_ptr=bptr, word=word[:n], value=value[:n], row_word=rw[:rows], row_node=rn[:rows], total=n)
        return None

    def set_neighbours(self, slot, neighbours):
        """The connected keyframes (slots, the reference's order) of each slot; the first ten are kept."""
        s = self._i32(slot)
        if len(neighbours) != len(s):
            raise ValueError("one neighbour list per slot")
        ptr = np.zeros(len(s) + 1, np.int32); ptr[1:] = np.cumsum([len(x) for x in neighbours])
        nb = self._i32(np.concatenate([self._i32(x) for x in neighbours] + [np.zeros(0, np.int32)]))
        self._check(lib().covgpu_bowdb_set_neighbours(self._h, len(s), iptr(s), iptr(ptr), iptr(nb)))

    def set_invalid(self, slot, flag):
        s = self._i32(slot); f = _u8(flag).ravel()
        if len(f) != len(s):
            raise ValueError("one flag per slot")
        self._check(lib().covgpu_bowdb_set_invalid(self._h, len(s), iptr(s), _bp(f)))

    def add(self, slot):
        """AddKeyframe: the slots join the insertion order at its end."""
        s = self._i32(slot)
        self._check(lib().covgpu_bowdb_add(self._h, len(s), iptr(s)))

    def erase(self, slot):
        """EraseKeyframe: slots that are not in the index are skipped."""
        s = self._i32(slot)
        self._check(lib().covgpu_bowdb_erase(self._h, len(s), iptr(s)))

    def query(self, query_slot, connected, min_score=None, cap: Optional[int] = None):
        """DetectCandidates of the stored slots query_slot against the database as it is; connected[q]: the query's whole connected
        list (slots, the reference's order). Returns what Context.detect_candidates_batch returns, candidates as slots. cap defaults
        to the number of live entries."""
        qs = self._i32(query_slot)
        Q = len(qs)
        if len(connected) != Q:
            raise ValueError("one connected list per query")
        cptr = np.zeros(Q + 1, np.int32); cptr[1:] = np.cumsum([len(x) for x in connected])
        con = self._i32(np.concatenate([self._i32(x) for x in connected] + [np.zeros(0, np.int32)]))
        ms = _opt(lambda a: _f64(a).ravel(), min_score)
        if ms is not None and len(ms) != Q:
            raise ValueError("min_score does not fit the queries")
        cap = self.stats()["live"] if cap is None else int(cap)
        n = max(Q, 1)
        nc = np.zeros(n, np.int32); cand = np.full((n, max(cap, 1)), -1, np.int32); acc = np.zeros((n, max(cap, 1)), np.float32)
        mso = np.zeros(n); nsh = np.zeros(n, np.int32); mcw = np.zeros(n, np.int32); nsc = np.zeros(n, np.int32)
        s = capi.BowDbQuery(Q, iptr(qs), iptr(cptr), iptr(con), dptr(ms), cap, iptr(nc), iptr(cand), acc.ctypes.data_as(capi._fp), dptr(mso),
                            iptr(nsh), iptr(mcw), iptr(nsc))
        self._check(lib().covgpu_bowdb_query(self._h, C.byref(s)))
        kept = np.minimum(nc[:Q], cap)
        return dict(candidates=[cand[q, :kept[q]].copy() for q in range(Q)], acc_score=[acc[q, :kept[q]].copy() for q in range(Q)],
                    num_candidates=nc[:Q], min_score=mso[:Q], num_sharing=nsh[:Q], max_common_words=mcw[:Q], num_scored=nsc[:Q])

    def compact(self):
        """Rebuilds the base index now: erased positions and dead pool words go."""
        self._check(lib().covgpu_bowdb_compact(self._h))

    def order(self):
        """The live slots in insertion order."""
        n = C.c_int32(0)
        out = np.zeros(max(self.stats()["live"], 1), np.int32)
        self._check(lib().covgpu_bowdb_order(self._h, len(out), iptr(out), C.byref(n)))
        return out[:n.value].copy()

    def stats(self) -> dict:
        """covgpu_bowdb_stats by name (capi.BOWDB_STATS); h2d_bytes / d2h_bytes are those of the last call."""
        out = (C.c_int64 * 16)()
        self._check(lib().covgpu_bowdb_stats(self._h, out))
        return {k: int(out[i]) for i, k in enumerate(capi.BOWDB_STATS)}


class Context:
    """One solver context = one HIP stream + HBM workspace (covgpu_create / covgpu_destroy)."""

    def __init__(self, device: int = 0):
        self._h = C.c_void_p()
        o = default_options(device=device)
        self._check(lib().covgpu_create(C.byref(o), C.byref(self._h)))
        self._keep = None
        self._keep_pgo = False

    def _check(self, rc: int):
        if rc != 0:
            raise CovGpuError(f"covgpu error {rc}: {lib().covgpu_last_error().decode()}")

    def close(self):
        if self._h:
            lib().covgpu_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- full solves (upload + solve + download)
    def gba_solve(self, prob: FlatProblem, opt: Options) -> Tuple[FlatProblem, Result]:
        q = prob.copy(); s = q.as_struct(); r = Result()
        self._check(lib().covgpu_gba_solve(self._h, C.byref(opt), C.byref(s), C.byref(r)))
        return q, r

    def gba_two_round(self, prob: FlatProblem, opt: Options, threshold: float, round1_iterations: int = 5, use_loops_round2: bool = True,
                      loop_loss_round2: float = 1.0, kf_fixed_round2=None):
        """Both rounds of GlobalBundleAdjustment behind one call (covgpu_gba_two_round): `prob` is the FIRST round's problem. Returns
        (solution of round 2 in round-1 indexing, round-1 result, round-2 result, erase flags [O] bool, lm_left [L], (erased, short))."""
        q = prob.copy(); s = q.as_struct(); r1 = Result(); r2 = Result()
        erase = np.zeros(max(prob.O, 1), np.uint8); left = np.zeros(max(prob.L, 1), np.int32); cnt = (C.c_int64 * 2)()
        tr = capi.TwoRound()
        tr.outlier_threshold = float(threshold); tr.round1_iterations = int(round1_iterations); tr.use_loops_round2 = int(bool(use_loops_round2))
        tr.loop_loss_round2 = float(loop_loss_round2)
        fx = None
        if kf_fixed_round2 is not None:
            fx = np.ascontiguousarray(kf_fixed_round2, np.uint8)
            tr.kf_fixed_round2 = fx.ctypes.data_as(C.POINTER(C.c_uint8))
        self._keep = prob; self._keep_pgo = False   # (the resident problem: prob's keyframes, the second round's observation set)
        self._check(lib().covgpu_gba_two_round(self._h, C.byref(opt), C.byref(s), C.byref(tr), erase.ctypes.data_as(capi._bp), iptr(left), cnt,
                                               C.byref(r1), C.byref(r2)))
        return q, r1, r2, erase[:prob.O].astype(bool), left[:prob.L], (int(cnt[0]), int(cnt[1]))

    def pgo_solve(self, prob: FlatProblem, opt: Options) -> Tuple[FlatProblem, Result]:
        q = prob.copy(); s = q.as_struct(); r = Result()
        self._check(lib().covgpu_pgo_solve(self._h, C.byref(opt), C.byref(s), C.byref(r)))
        return q, r

    # ---- split form: inputs resident in HBM before the timed region
    def upload(self, prob: FlatProblem, opt: Options, pgo: bool = False):
        self._keep = prob
        self._keep_pgo = bool(pgo)
        s = prob.as_struct()
        fn = lib().covgpu_upload_pgo if pgo else lib().covgpu_upload
        self._check(fn(self._h, C.byref(opt), C.byref(s)))

    def solve_resident(self, opt: Options) -> Result:
        r = Result()
        self._check(lib().covgpu_solve_resident(self._h, C.byref(opt), C.byref(r)))
        return r

    def download(self) -> FlatProblem:
        q = self._keep.copy(); s = q.as_struct()
        self._check(lib().covgpu_download(self._h, C.byref(s)))
        return q

    def set_shard_group(self, plan, rank: int, group):
        """Agent-sharded solve among host threads of THIS process (virtual ranks): `plan` = distrib.ShardPlan, `group` = distrib.Group."""
        self._check(lib().covgpu_set_shard_group(self._h, plan.handle, int(rank), group.handle))
        self._shard_keep = (plan, group)

    def set_shard_rccl(self, plan, rank: int, world: int, unique_id: bytes):
        """Agent-sharded solve, one process per GPU: RCCL communicator from rank 0's covgpu_rccl_unique_id."""
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        self._check(lib().covgpu_set_shard_rccl(self._h, plan.handle, int(rank), int(world), buf))
        self._shard_keep = (plan,)

    def set_shard_none(self):
        self._check(lib().covgpu_set_shard_none(self._h))
        self._shard_keep = None

    def allreduce_host(self, a: np.ndarray, op: int = 0) -> np.ndarray:
        """Sum (0) / max (1) of a small host vector over the ranks of the context's collective (identity without one)."""
        a = np.ascontiguousarray(a, dtype=np.float64).copy()
        self._check(lib().covgpu_allreduce_host(self._h, dptr(a), a.size, int(op)))
        return a

    def shard_stats(self) -> dict:
        out = (C.c_int64 * 4)()
        lib().covgpu_shard_stats(self._h, out)
        return {"collectives": int(out[0]), "bytes": int(out[1]), "rank": int(out[2]), "world": int(out[3])}

    def outlier_pass(self, n_obs: int, n_lm: int, threshold: float):
        """Outlier flags and per-landmark remaining-observation counts at the resident estimate (covgpu_outlier_pass)."""
        erase = np.zeros(max(n_obs, 1), np.uint8); left = np.zeros(max(n_lm, 1), np.int32); cnt = (C.c_int64 * 2)()
        self._check(lib().covgpu_outlier_pass(self._h, float(threshold), erase.ctypes.data_as(capi._bp), iptr(left), cnt))
        return erase[:n_obs].astype(bool), left[:n_lm], (int(cnt[0]), int(cnt[1]))

    def covisibility(self, threshold: int):
        """Covisibility recount on the resident problem (covgpu_covisibility): (kf_i, kf_j, weight) with kf_i > kf_j, weight >= threshold."""
        cap = 1 << 16
        while True:
            ki = np.zeros(cap, np.int32); kj = np.zeros(cap, np.int32); w = np.zeros(cap, np.int32); n = C.c_int64()
            self._check(lib().covgpu_covisibility(self._h, int(threshold), cap, iptr(ki), iptr(kj), iptr(w), C.byref(n)))
            if n.value <= cap:
                return ki[:n.value], kj[:n.value], w[:n.value]
            cap = int(n.value)

    def relpose_batch(self, bt: dict, th_outlier: float = 1.3, min_inliers: int = 12):
        """Batched Optimization::OptimizeRelativePose (covgpu_relpose_batch). `bt`: dict with ptr, pA, pB, kpA, kpB, sigA, sigB,
        camA, camB, distA, distB, T0 (see include/covgpu.h), optionally modelA, modelB, xiA, xiB (COVGPU_CAM_* and xi per pair and side;
        absent = pinhole). Returns (T_ab [B,7], outlier flags [C], inliers [B])."""
        f, i = _f64, _i32
        keep = dict(ptr=i(bt["ptr"]), pB=f(bt["pB"]), pA=f(bt["pA"]), kA=f(bt["kpA"]), kB=f(bt["kpB"]), sA=f(bt["sigA"]), sB=f(bt["sigB"]),
                    cA=f(bt["camA"]), cB=f(bt["camB"]), dA=i(bt["distA"]), dB=i(bt["distB"]), T=np.array(bt["T0"], dtype=np.float64, order="C"))
        for k in ("modelA", "modelB"):
            keep[k] = _opt(i, bt.get(k))
        for k in ("xiA", "xiB"):
            keep[k] = _opt(f, bt.get(k))
        B = len(keep["ptr"]) - 1
        out = np.zeros(max(int(keep["ptr"][-1]), 1), np.uint8); inl = np.zeros(max(B, 1), np.int32)
        ip = lambda a: _opt(iptr, a)
        s = capi.RelposeBatch(B, iptr(keep["ptr"]), dptr(keep["pB"]), dptr(keep["pA"]), dptr(keep["kA"]), dptr(keep["kB"]), dptr(keep["sA"]),
                              dptr(keep["sB"]), dptr(keep["cA"]), dptr(keep["cB"]), iptr(keep["dA"]), iptr(keep["dB"]), dptr(keep["T"]),
                              _bp(out), iptr(inl), ip(keep["modelA"]), ip(keep["modelB"]), dptr(keep["xiA"]), dptr(keep["xiB"]))
        self._check(lib().covgpu_relpose_batch(self._h, C.byref(s), float(th_outlier), int(min_inliers)))
        return keep["T"], out[:int(keep["ptr"][-1])].astype(bool), inl[:B]

    def abspose_ransac_batch(self, bt: dict, **opts):
        """Batched Se3Solver::projectiveAlignment (covgpu_abspose_ransac_batch). `bt`: dict with ptr [num+1], bearing [C,3],
        point_w [C,3], sigma_angle [C], optionally seed [num] (uint64; absent = opts seed + b) and T0 [num,7] (what untouched rows hold).
        `opts`: min_inliers, max_iterations, probability, threshold, seed (defaults: covgpu_default_ransac_opts). Returns dict(T_wc [num,7],
        inlier [C] bool, inliers [num], iterations [num], best_draw [num])."""
        o = capi.RansacOpts()
        lib().covgpu_default_ransac_opts(C.byref(o))
        _set_opts(o, [name for name, _ in capi.RansacOpts._fields_], opts, "RANSAC")
        ptr = _i32(bt["ptr"])
        B = len(ptr) - 1
        Cn = int(ptr[-1]) if B >= 0 and len(ptr) else 0
        f = _f64(bt["bearing"]).reshape(-1, 3)
        P = _f64(bt["point_w"]).reshape(-1, 3)
        sg = _f64(bt["sigma_angle"])
        seed = _opt(lambda a: np.ascontiguousarray(a, dtype=np.uint64), bt.get("seed"))
        T = np.array(bt["T0"], dtype=np.float64, order="C").reshape(-1, 7) if bt.get("T0") is not None else np.zeros((max(B, 1), 7))
        mask = np.zeros(max(Cn, 1), np.uint8)
        inl, its, bd = (np.zeros(max(B, 1), np.int32) for _ in range(3))
        s = capi.AbsposeBatch(B, iptr(ptr), dptr(f), dptr(P), dptr(sg), None if seed is None else seed.ctypes.data_as(C.POINTER(C.c_uint64)),
                              dptr(T), _bp(mask), iptr(inl), iptr(its), iptr(bd))
        self._check(lib().covgpu_abspose_ransac_batch(self._h, C.byref(s), C.byref(o)))
        return dict(T_wc=T[:max(B, 0)], inlier=mask[:Cn].astype(bool), inliers=inl[:max(B, 0)], iterations=its[:max(B, 0)], best_draw=bd[:max(B, 0)])

    def fivept_ransac_batch(self, bt: dict, **opts):
        """Batched five-point relative-pose RANSAC of COVINS-G (covgpu_fivept_ransac_batch). `bt`: dict with ptr [num+1],
        bearing1 [C,3] (frame 1, the query side), bearing2 [C,3], optionally seed [num] (uint64; absent = opts seed + b) and T0 [num,7]
        (what untouched rows hold). `opts`: min_inliers, max_iterations, probability, threshold, sigma, seed (defaults:
        covgpu_default_fivept_opts). Returns dict(T_12 [num,7], inlier [C] bool, inliers [num], status [num], iterations [num],
        best_draw [num])."""
        s, o, k = _fivept_args(bt, opts)
        self._check(lib().covgpu_fivept_ransac_batch(self._h, C.byref(s), C.byref(o)))
        B = max(k["B"], 0)
        return dict(T_12=k["T"][:B], inlier=k["mask"][:k["C"]].astype(bool), inliers=k["inl"][:B], status=k["st"][:B], iterations=k["its"][:B],
                    best_draw=k["bd"][:B])

    def fivept_solve_batch(self, f1, f2):
        """Test entry point (covgpu_fivept_solve_batch): the five-point problem of every 8-tuple f1, f2 [n,8,3] on its slots 0..4. Returns
        dict(E [n,10,3,3] (rows past nsol zero), nsol [n], T [n,7] (zero where no pose), chosen [n] (-1: none))."""
        f1 = _f64(f1).reshape(-1, 8, 3); f2 = _f64(f2).reshape(-1, 8, 3)
        n = len(f1)
        if len(f2) != n:
            raise ValueError("f1 and f2 differ in length")
        E = np.zeros((max(n, 1), 10, 3, 3)); T = np.zeros((max(n, 1), 7))
        ns = np.zeros(max(n, 1), np.int32); ch = np.zeros(max(n, 1), np.int32)
        self._check(lib().covgpu_fivept_solve_batch(self._h, n, dptr(f1), dptr(f2), dptr(E), iptr(ns), dptr(T), iptr(ch)))
        return dict(E=E[:n], nsol=ns[:n], T=T[:n], chosen=ch[:n])

    def ncrelpose_batch(self, bt: dict, **opts):
        """Batched 17-point stage of COVINS-G's loop verification with the polish and the sampled loop covariance
        (covgpu_ncrelpose_batch). `bt`: dict with ptr [num+1], cell_ptr [num,cells+1] (relative to the job), bearing1,
        bearing2 [C,3], cam1, cam2 [C] (into the job's cameras), cam_ptr [num+1], cam [M,12] (R_c row-major | o_c), T_sc_q, T_sc_c [num,7],
        optionally seed [num] (uint64; absent = opts seed + b) and fill (what untouched outputs hold, default 0). `opts`: rp_error,
        rp_error_cov, min_inliers, max_iterations, cov_thres, cov_iters, cov_max_iters, probability, seed, stage_cap (defaults:
        covgpu_default_ncrelpose_opts). Returns dict(T_c1c2, T_c1c2_ransac, T_s1s2 [num,7], cov [num,6,6], inlier [C] bool, inliers,
        status, iterations, best_draw, cov_rows, cov_draws [num])."""
        s, o, k = _ncrelpose_args(bt, opts)
        self._check(lib().covgpu_ncrelpose_batch(self._h, C.byref(s), C.byref(o)))
        B = max(k["B"], 0)
        return dict(T_c1c2=k["T"][:B], T_c1c2_ransac=k["Tr"][:B], T_s1s2=k["Ts"][:B], cov=k["cov"][:B].reshape(-1, 6, 6),
                    inlier=k["mask"][:k["C"]].astype(bool), inliers=k["inl"][:B], status=k["st"][:B], iterations=k["its"][:B],
                    best_draw=k["bd"][:B], cov_rows=k["cr"][:B], cov_draws=k["cd"][:B])

    def ncrelpose_solve_batch(self, ray1, ray2):
        """Test entry point (covgpu_ncrelpose_solve_batch): the 17-point linear solve alone on the tuples ray1, ray2 [n,N,6] (g | o),
        N = 17..64. Returns dict(T [n,7] (zero where not ok), ok [n], sv [n,3] (sigma_1, sigma_17, sigma_18))."""
        ray1 = _f64(ray1); ray2 = _f64(ray2)
        n, N = ray1.shape[0], ray1.shape[1]
        T = np.zeros((max(n, 1), 7)); ok = np.zeros(max(n, 1), np.int32); sv = np.zeros((max(n, 1), 3))
        self._check(lib().covgpu_ncrelpose_solve_batch(self._h, n, N, dptr(ray1), dptr(ray2), dptr(T), iptr(ok), dptr(sv)))
        return dict(T=T[:n], ok=ok[:n], sv=sv[:n])

    def match_batch(self, sets: dict, set_a, set_b, mode: str = "dense", **opts):
        """Batched ORB descriptor matching of loop candidates (covgpu_match_batch). `sets`: dict with row_ptr
        [num_sets+1], desc [rows,32] uint8 and optionally skip [rows] (DENSE only). Job j matches set set_a[j] (query) against set
        set_b[j]. mode "dense" (LandmarkMatchingAlgorithm + DenseMatcher) or "knn2" (BFMatcher knnMatch k=2 + distance and ratio tests).
        `opts`: dist_threshold, ratio (defaults: covgpu_default_match_opts). Returns dict(match [sumA] local B row or -1, dist [sumA],
        nmatches [num_jobs], offset [num_jobs+1] the output rows of job j are offset[j]:offset[j+1])."""
        m = _MATCH_MODES.get(mode, mode)
        o = capi.MatchOpts()
        lib().covgpu_default_match_opts(C.byref(o), int(m) if isinstance(m, int) else -1)
        _set_opts(o, ("dist_threshold", "ratio"), opts, "match")
        ptr = _i32(sets["row_ptr"])
        S = len(ptr) - 1
        desc = _u8(sets["desc"]).reshape(-1, 32)
        skip = _opt(_u8, sets.get("skip"))
        sa, sb = _i32(set_a).ravel(), _i32(set_b).ravel()
        J = len(sa)
        if len(sb) != J:
            raise ValueError("set_a and set_b differ in length")
        off = _job_offsets(ptr, sa, S >= 0 and np.all((sa >= 0) & (sa < S)))
        tot = int(off[-1])
        match = np.full(max(tot, 1), -1, np.int32); dist = np.full(max(tot, 1), -1, np.int32); nm = np.zeros(max(J, 1), np.int32)
        s = capi.MatchBatch(S, iptr(ptr), _bp(desc), _bp(skip), J, iptr(sa), iptr(sb), iptr(match), iptr(dist), iptr(nm))
        self._check(lib().covgpu_match_batch(self._h, C.byref(s), C.byref(o)))
        return dict(match=match[:tot], dist=dist[:tot], nmatches=nm[:J], offset=off)

    def match_float_batch(self, sets: dict, set_a, set_b, **opts):
        """Batched L2 matching of float (SIFT) descriptors of COVINS-G's loop candidates (covgpu_match_float_batch):
        knnMatch(k = 2) + distance and ratio tests, exact search. `sets`: dict with row_ptr [num_sets+1] and desc [rows,dim] float32 (dim
        from desc's last axis, or sets["dim"] where desc has no rows). Job j matches set set_a[j] (query) against set set_b[j] (train).
        `opts`: dist_threshold, ratio, mode (defaults: covgpu_default_match_float_opts). Returns the dict of match_batch, dist in float32."""
        o = capi.MatchOpts()
        lib().covgpu_default_match_float_opts(C.byref(o))
        _set_opts(o, ("dist_threshold", "ratio", "mode"), opts, "match", lambda k, v: _MATCH_MODES.get(v, v) if k == "mode" else v)
        ptr = _i32(sets["row_ptr"])
        S = len(ptr) - 1
        desc = np.ascontiguousarray(sets["desc"], dtype=np.float32)
        dim = int(sets["dim"]) if sets.get("dim") is not None else (int(desc.shape[-1]) if desc.ndim == 2 else 0)
        sa, sb = _i32(set_a).ravel(), _i32(set_b).ravel()
        J = len(sa)
        if len(sb) != J:
            raise ValueError("set_a and set_b differ in length")
        if dim > 0 and S >= 0 and desc.size != int(ptr[-1]) * dim:
            raise ValueError("desc does not hold row_ptr[-1] rows of dim floats")
        off = _job_offsets(ptr, sa, S >= 0 and np.all((sa >= 0) & (sa < S)))
        tot = int(off[-1])
        match = np.full(max(tot, 1), -1, np.int32); dist = np.full(max(tot, 1), -1, np.float32); nm = np.zeros(max(J, 1), np.int32)
        dbuf = desc if desc.size else np.zeros(1, np.float32)
        s = capi.MatchFloatBatch(S, iptr(ptr), dim, dbuf.ctypes.data_as(capi._fp), J, iptr(sa), iptr(sb), iptr(match),
                                 dist.ctypes.data_as(capi._fp), iptr(nm))
        self._check(lib().covgpu_match_float_batch(self._h, C.byref(s), C.byref(o)))
        return dict(match=match[:tot], dist=dist[:tot], nmatches=nm[:J], offset=off)

    @staticmethod
    def _guided_opts(mode, opts):
        o = capi.GuidedOpts()
        lib().covgpu_default_guided_opts(C.byref(o), mode)
        return _set_opts(o, ("th_low", "radius", "scale_factor", "num_octaves", "agreement"), opts, "guided-matching")

    @staticmethod
    def _keypoint_sets(sets: dict, keep: list):
        """covgpu_keypoint_sets_t of `sets` (row_ptr, kp [rows,2], level, desc [rows,32], bounds [S,4], optional grid_inv [S,2]); the
        arrays it points into are appended to `keep`."""
        ptr = _i32(sets["row_ptr"]).ravel()
        S = len(ptr) - 1
        kp = np.ascontiguousarray(sets["kp"], dtype=np.float32).reshape(-1, 2)
        level = _i32(sets["level"]).ravel()
        desc = _u8(sets["desc"]).reshape(-1, 32)
        bounds = _f64(sets["bounds"]).reshape(-1, 4)
        grid = _opt(lambda a: _f64(a).reshape(-1, 2), sets.get("grid_inv"))
        rows = int(ptr[-1]) if S > 0 else 0
        if len(kp) != rows or len(level) != rows or len(desc) != rows or len(bounds) != S or (grid is not None and len(grid) != S):
            raise ValueError("keypoint set arrays do not fit row_ptr")
        keep += [ptr, kp, level, desc, bounds, grid]
        return capi.KeypointSets(S, iptr(ptr), kp.ctypes.data_as(capi._fp), iptr(level), _bp(desc), dptr(bounds),
                                 dptr(grid)), ptr, S, rows

    def search_se3_batch(self, sets: dict, set_1, set_2, T12, **opts):
        """Batched FeatureMatcher::SearchBySE3 (covgpu_search_se3_batch). `sets`: the keypoint sets (row_ptr, kp, level,
        desc, bounds, optional grid_inv) plus K [S,4] and per row lm_pos [rows,3], lm_max_distance, lm_desc [rows,32], lm_free. Job j
        searches set set_1[j] (query) and set set_2[j] (candidate) under T12[j] = [qx qy qz qw x y z]. `opts`: th_low, radius,
        scale_factor, num_octaves, agreement (defaults: covgpu_default_guided_opts). Returns dict(match [sum n1] candidate row or -1,
        match1 [sum n1], match2 [sum n2] the two directions, nfound [num_jobs], offset / offset2 [num_jobs+1] the rows of job j)."""
        o = self._guided_opts(capi.GUIDED_SE3, opts)
        keep = []
        ks, ptr, S, rows = self._keypoint_sets(sets, keep)
        K, pos, maxd = _f64(sets["K"]).reshape(-1, 4), _f64(sets["lm_pos"]).reshape(-1, 3), _f64(sets["lm_max_distance"]).reshape(-1)
        ldesc = _u8(sets["lm_desc"]).reshape(-1, 32)
        free = _u8(sets["lm_free"]).ravel()
        if len(K) != S or len(pos) != rows or len(maxd) != rows or len(ldesc) != rows or len(free) != rows:
            raise ValueError("landmark arrays do not fit row_ptr")
        s1, s2 = _i32(set_1).ravel(), _i32(set_2).ravel()
        T = _f64(T12).reshape(-1, 7)
        J = len(s1)
        if len(s2) != J or len(T) != J:
            raise ValueError("set_1, set_2 and T12 differ in length")
        ok = J > 0 and np.all((s1 >= 0) & (s1 < S) & (s2 >= 0) & (s2 < S))
        off1, off2 = _job_offsets(ptr, s1, ok), _job_offsets(ptr, s2, ok)
        t1, t2 = int(off1[-1]), int(off2[-1])
        match = np.full(max(t1, 1), -1, np.int32); m1 = np.full(max(t1, 1), -1, np.int32); m2 = np.full(max(t2, 1), -1, np.int32)
        nf = np.zeros(max(J, 1), np.int32)
        s = capi.SearchSe3Batch(ks, dptr(K), dptr(pos), dptr(maxd), _bp(ldesc), _bp(free), J, iptr(s1), iptr(s2), dptr(T), iptr(match),
                                iptr(m1), iptr(m2), iptr(nf))
        self._check(lib().covgpu_search_se3_batch(self._h, C.byref(s), C.byref(o)))
        return dict(match=match[:t1], match1=m1[:t1], match2=m2[:t2], nfound=nf[:J], offset=off1, offset2=off2)

    def search_projection_batch(self, sets: dict, jobs: dict, **opts):
        """Batched FeatureMatcher::SearchByProjection (covgpu_search_projection_batch). `sets`: the keypoint sets plus
        cam [S,8] (fx fy cx cy d0..d3), dist_type [S], optional cam_model / xi [S] and taken [rows]. `jobs`: set [J], T_cw [J,7],
        point_ptr [J+1] and per point p_w [P,3], normal [P,3], min_distance, max_distance, desc [P,32], optional skip and existing_idx.
        `opts` as search_se3_batch. Returns dict(claimed [P] keypoint row or -1, remap_to [P], best_dist [P], nmatches [J])."""
        o = self._guided_opts(capi.GUIDED_PROJECTION, opts)
        keep = []
        ks, ptr, S, rows = self._keypoint_sets(sets, keep)
        bp = _bp
        u8 = lambda d, k: _opt(lambda a: _u8(a).ravel(), d.get(k))
        i32 = lambda d, k: _opt(lambda a: _i32(a).ravel(), d.get(k))
        cam = _f64(sets["cam"]).reshape(-1, 8)
        dt, cm, taken = i32(sets, "dist_type"), i32(sets, "cam_model"), u8(sets, "taken")
        xi = _opt(lambda a: _f64(a).ravel(), sets.get("xi"))
        if len(cam) != S or len(dt) != S or (cm is not None and len(cm) != S) or (xi is not None and len(xi) != S) \
                or (taken is not None and len(taken) != rows):
            raise ValueError("camera or taken arrays do not fit row_ptr")
        st = i32(jobs, "set")
        J = len(st)
        T = _f64(jobs["T_cw"]).reshape(-1, 7)
        pp = i32(jobs, "point_ptr")
        f64 = lambda k, w: _f64(jobs[k]).reshape((-1,) + w)
        pw, nrm, mind, maxd = f64("p_w", (3,)), f64("normal", (3,)), f64("min_distance", ()), f64("max_distance", ())
        pdesc = _u8(jobs["desc"]).reshape(-1, 32)
        skip, ex = u8(jobs, "skip"), i32(jobs, "existing_idx")
        P = len(pw)
        if len(T) != J or len(pp) != J + 1 or int(pp[-1]) != P or any(a is not None and len(a) != P for a in (nrm, mind, maxd, pdesc, skip, ex)):
            raise ValueError("job or point arrays differ in length")
        claimed = np.full(max(P, 1), -1, np.int32); remap = np.full(max(P, 1), -1, np.int32); bd = np.full(max(P, 1), -1, np.int32)
        nm = np.zeros(max(J, 1), np.int32)
        s = capi.SearchProjectionBatch(ks, bp(taken), dptr(cam), iptr(dt), _opt(iptr, cm), dptr(xi), J, iptr(st), dptr(T),
                                       iptr(pp), dptr(pw), dptr(nrm), dptr(mind), dptr(maxd), bp(pdesc), bp(skip),
                                       _opt(iptr, ex), iptr(claimed), iptr(remap), iptr(bd), iptr(nm))
        self._check(lib().covgpu_search_projection_batch(self._h, C.byref(s), C.byref(o)))
        return dict(claimed=claimed[:P], remap_to=remap[:P], best_dist=bd[:P], nmatches=nm[:J])

    def bowdb(self, voc: Optional[dict] = None, **opts) -> "BowDb":
        """A resident keyframe database on this context (covgpu_bowdb_create). voc: a vocabulary as covins_amd/vocio.py
        reads it, or None for a handle that only takes ready vectors (put). opts: mode ("covins" | "covins_g"), the detect options of
        detect_candidates_batch, levelsup, tail_limit, reserve_kf, reserve_words, num_words."""
        return BowDb(self, voc, **opts)

    @staticmethod
    def _bow_vocab(voc: dict, keep: list):
        """covgpu_bow_vocab_t over the flat form of covins_amd/vocio.py (`keep` holds the arrays alive)."""
        parent, cptr, child, wid = (_i32(voc[k]).ravel() for k in ("parent", "child_ptr", "child", "word_id"))
        desc = _u8(voc["desc"]).reshape(-1, 32)
        weight = _f64(voc["weight"]).ravel()
        N = len(parent)
        if len(cptr) != N + 1 or len(child) != max(N - 1, 0) or len(desc) != N or len(wid) != N or len(weight) != N:
            raise ValueError("vocabulary arrays differ in length")
        keep += [parent, cptr, child, wid, desc, weight]
        return capi.BowVocab(N, int(voc["num_words"]), int(voc["k"]), int(voc["L"]), int(voc["scoring"]), int(voc["weighting"]),
                             iptr(parent), iptr(cptr), iptr(child), _bp(desc), iptr(wid), dptr(weight))

    def bow_transform_batch(self, voc: dict, sets: dict, levelsup: int = 4, capacity: Optional[int] = None):
        """DBoW2's transform(features, bow_vec, feat_vec, levelsup) of every descriptor set (covgpu_bow_transform_batch, DESIGN.md
        §4.13). `voc`: a vocabulary as covins_amd/vocio.py reads it; `sets`: row_ptr [S+1] and desc [rows,32] as for match_batch.
        Returns dict(bow_ptr [S+1], word, value: the L1-normalised bow vectors as one CSR; row_word [rows] the word of each
        descriptor, -1 if stopped; row_node [rows] its FeatureVector key; total). `capacity` (default: rows, always enough) bounds
        the entries written; bow_ptr and total stay exact."""
        keep = []
        v = self._bow_vocab(voc, keep)
        ptr = _i32(sets["row_ptr"])
        S = len(ptr) - 1
        desc = _u8(sets["desc"]).reshape(-1, 32)
        rows = len(desc)
        cap = rows if capacity is None else int(capacity)
        bptr = np.zeros(S + 1, np.int32); word = np.zeros(max(cap, 1), np.int32); value = np.zeros(max(cap, 1))
        rw = np.full(max(rows, 1), -1, np.int32); rn = np.zeros(max(rows, 1), np.int32); tot = C.c_int64(0)
        s = capi.BowTransformBatch(S, iptr(ptr), _bp(desc), int(levelsup), cap, iptr(bptr), iptr(word), dptr(value),
                                   C.pointer(tot), iptr(rw), iptr(rn))
        self._check(lib().covgpu_bow_transform_batch(self._h, C.byref(v), C.byref(s)))
        n = min(cap, int(tot.value))
        return dict(bow_ptr=bptr, word=word[:n], value=value[:n], row_word=rw[:rows], row_node=rn[:rows], total=int(tot.value))

    def bow_score_pairs(self, bow_ptr, word, value, a, b):
        """L1Scoring::score of the pairs (a[i], b[i]) of the rows of a bow CSR (covgpu_bow_score_pairs). Returns float64 [len(a)]."""
        ptr, w, v = _i32(bow_ptr), _i32(word), _f64(value)
        pa, pb = _i32(a).ravel(), _i32(b).ravel()
        if len(pa) != len(pb):
            raise ValueError("a and b differ in length")
        out = np.zeros(max(len(pa), 1))
        self._check(lib().covgpu_bow_score_pairs(self._h, len(ptr) - 1, iptr(ptr), iptr(w), dptr(v), len(pa), iptr(pa), iptr(pb), dptr(out)))
        return out[:len(pa)]

    def detect_candidates_batch(self, table: dict, db_order, query_kf, db_visible, mode: str = "covins", min_score=None,
                                cap: Optional[int] = None, **opts):
        """KeyframeDatabase::DetectCandidates for many queries (covgpu_detect_candidates_batch). `table`: id, client,
        bow_ptr, word, value, nb_ptr, nb (table indices in the reference's neighbour order) and optionally invalid. Query q is
        keyframe query_kf[q] against db_order[:db_visible[q]]. `min_score` [Q]: given directly instead of the reference score of
        DetectLoop. `opts`: min_score_factor, min_loop_dist, exclude_kfs_with_id_less_than, inter_map_matches_only, scratch_kib (defaults:
        covgpu_default_detect_opts(mode)). `cap` (default: len(db_order)) bounds the candidates kept per query. Returns
        dict(candidates: list of arrays of table indices in the reference's order, acc_score: list of float32 arrays,
        num_candidates, min_score, num_sharing, max_common_words, num_scored [Q])."""
        o = capi.DetectOpts()
        lib().covgpu_default_detect_opts(C.byref(o), int(_DETECT_MODES.get(mode, mode)))
        _set_opts(o, _DETECT_OPTS, opts, "detect")
        i32 = lambda a: _i32(a).ravel()
        kid, client, bptr, word, nptr, nb = (i32(table[k]) for k in ("id", "client", "bow_ptr", "word", "nb_ptr", "nb"))
        value = _f64(table["value"]).ravel()
        inv = _opt(lambda a: _u8(a).ravel(), table.get("invalid"))
        N = len(kid)
        if len(client) != N or len(bptr) != N + 1 or len(nptr) != N + 1 or len(value) != len(word) or (inv is not None and len(inv) != N):
            raise ValueError("table arrays differ in length")
        db, qk, vis = i32(db_order), i32(query_kf), i32(db_visible)
        Q = len(qk)
        if len(vis) != Q:
            raise ValueError("query_kf and db_visible differ in length")
        ms = _opt(lambda a: _f64(a).ravel(), min_score)
        if ms is not None and len(ms) != Q:
            raise ValueError("min_score does not fit the queries")
        cap = len(db) if cap is None else int(cap)
        n = max(Q, 1)
        nc = np.zeros(n, np.int32); cand = np.full((n, max(cap, 1)), -1, np.int32); acc = np.zeros((n, max(cap, 1)), np.float32)
        mso = np.zeros(n); nsh = np.zeros(n, np.int32); mcw = np.zeros(n, np.int32); nsc = np.zeros(n, np.int32)
        s = capi.DetectBatch(N, iptr(kid), iptr(client), iptr(bptr), iptr(word), dptr(value), iptr(nptr), iptr(nb),
                             _bp(inv), len(db), iptr(db), Q, iptr(qk), iptr(vis), dptr(ms), cap,
                             iptr(nc), iptr(cand), acc.ctypes.data_as(capi._fp), dptr(mso), iptr(nsh), iptr(mcw), iptr(nsc))
        self._check(lib().covgpu_detect_candidates_batch(self._h, C.byref(s), C.byref(o)))
        kept = np.minimum(nc[:Q], cap)
        return dict(candidates=[cand[q, :kept[q]].copy() for q in range(Q)], acc_score=[acc[q, :kept[q]].copy() for q in range(Q)],
                    num_candidates=nc[:Q], min_score=mso[:Q], num_sharing=nsh[:Q], max_common_words=mcw[:Q], num_scored=nsc[:Q])

    @staticmethod
    def _prune_batch(lm_obs_ptr, obs_kf, kf_pred, kf_succ, kf_time, lm_invalid, kf_invalid, kf_first, kf_loop, kf_not_erase, capacity,
                     opts, want_loop_ms=False):
        """(PruneBatch, PruneOpts, outputs, keep-alive list) of one covgpu_prune_redundant call."""
        i32 = lambda a: _i32(a).ravel()
        flag = lambda a: _opt(lambda x: _u8(x).ravel(), a)
        ptr, okf, pred, succ = i32(lm_obs_ptr), i32(obs_kf), i32(kf_pred), i32(kf_succ)
        time = _f64(kf_time).ravel()
        K, L = len(pred), len(ptr) - 1
        flags = [flag(a) for a in (lm_invalid, kf_invalid, kf_first, kf_loop, kf_not_erase)]
        if L < 0 or len(succ) != K or len(time) != K or any(f is not None and len(f) != n for f, n in zip(flags, (L, K, K, K, K))):
            raise ValueError("prune arrays differ in length")
        if int(ptr[-1]) > len(okf):
            raise ValueError("lm_obs_ptr runs past obs_kf")
        o = capi.PruneOpts()
        lib().covgpu_default_prune_opts(C.byref(o))
        _set_opts(o, ("th_red", "max_time_dist", "max_kfs", "max_rounds"), opts, "prune", lambda k, v: -1 if k == "max_kfs" and v is None else v)
        cap = K if capacity is None else int(capacity)
        out = dict(round_kf=np.full(max(cap, 1), -1, np.int32), round_action=np.full(max(cap, 1), -1, np.int32),
                   scal=np.zeros(3, np.int32), kf_pred=np.zeros(max(K, 1), np.int32), kf_succ=np.zeros(max(K, 1), np.int32),
                   lm_nobs=np.zeros(max(L, 1), np.int32), red_num=np.zeros(max(K, 1), np.int32), red_den=np.zeros(max(K, 1), np.int32),
                   loop_ms=np.zeros(1))
        sc = out["scal"]
        s = capi.PruneBatch(K, L, iptr(ptr), iptr(okf), *(_bp(f) for f in flags), iptr(pred), iptr(succ), dptr(time), cap,
                            iptr(out["round_kf"]), iptr(out["round_action"]), iptr(sc[0:1]), iptr(sc[1:2]), iptr(sc[2:3]),
                            iptr(out["kf_pred"]), iptr(out["kf_succ"]), iptr(out["lm_nobs"]), iptr(out["red_num"]), iptr(out["red_den"]),
                            dptr(out["loop_ms"]) if want_loop_ms else None)
        return s, o, out, [ptr, okf, pred, succ, time, flags]

    def prune_redundant(self, lm_obs_ptr, obs_kf, kf_pred, kf_succ, kf_time, lm_invalid=None, kf_invalid=None, kf_first=None, kf_loop=None,
                        kf_not_erase=None, capacity: Optional[int] = None, loop_ms: bool = False, **opts):
        """Map::RemoveRedundantData as one device call (covgpu_prune_redundant): the greedy loop over the redundancy
        values, exact in integers. Observations are landmark-major (lm_obs_ptr [L+1], obs_kf [O] keyframe table indices); kf_pred /
        kf_succ are table indices or -1; the flag arrays may be None (none set). `opts`: th_red (0.95), max_time_dist (1.0), max_kfs (None
        or < 0: threshold mode), max_rounds (<= 0: K). `capacity` (default K) bounds the round records kept. Returns dict(round_kf,
        round_action (0 erased, 1 time gate, 2 loop keyframe, 3 not_erase), num_rounds (the true count), removed (actions 0 + 3, the
        reference's return value), stop_reason, kf_pred, kf_succ (the relinked chain), lm_nobs, red_num, red_den; loop_ms if asked for)."""
        s, o, out, keep = self._prune_batch(lm_obs_ptr, obs_kf, kf_pred, kf_succ, kf_time, lm_invalid, kf_invalid, kf_first, kf_loop,
                                            kf_not_erase, capacity, opts, loop_ms)
        self._check(lib().covgpu_prune_redundant(self._h, C.byref(s), C.byref(o)))
        K, L = s.num_kf, s.num_lm
        n, removed, stop = (int(x) for x in out["scal"])
        kept = min(n, s.capacity)
        r = dict(round_kf=out["round_kf"][:kept].copy(), round_action=out["round_action"][:kept].copy(), num_rounds=n, removed=removed,
                 stop_reason=stop, kf_pred=out["kf_pred"][:K], kf_succ=out["kf_succ"][:K], lm_nobs=out["lm_nobs"][:L],
                 red_num=out["red_num"][:K], red_den=out["red_den"][:K])
        if loop_ms:
            r["loop_ms"] = float(out["loop_ms"][0])
        return r

    @staticmethod
    def _refresh_batch(lm_obs_ptr, obs_kf, obs_desc, obs_octave, lm_ref_obs, lm_pos, kf_center, kf_invalid, lm_invalid, opts,
                       want_kernel_ms=False):
        """(LandmarkRefresh, LandmarkRefreshOpts, outputs, keep-alive list) of one covgpu_landmark_refresh call."""
        i32 = lambda a: _i32(a).ravel()
        flag = lambda a: _opt(lambda x: _u8(x).ravel(), a)
        ptr, okf, ooc, ref = i32(lm_obs_ptr), i32(obs_kf), i32(obs_octave), i32(lm_ref_obs)
        pos, cen = _f64(lm_pos).reshape(-1, 3), _f64(kf_center).reshape(-1, 3)
        desc = _opt(lambda a: _u8(a).reshape(-1, 32), obs_desc)
        kinv, linv = flag(kf_invalid), flag(lm_invalid)
        K, L = len(cen), len(ptr) - 1
        if L < 0 or len(ref) != L or len(pos) != L or len(ooc) != len(okf) or (desc is not None and len(desc) != len(okf)) or \
                (kinv is not None and len(kinv) != K) or (linv is not None and len(linv) != L):
            raise ValueError("landmark-refresh arrays differ in length")
        if int(ptr[-1]) > len(okf):
            raise ValueError("lm_obs_ptr runs past obs_kf")
        o = capi.LandmarkRefreshOpts()
        lib().covgpu_default_landmark_refresh_opts(C.byref(o))
        _set_opts(o, ("scale_factor", "num_octaves"), opts, "landmark-refresh")
        n = max(L, 1)
        out = dict(lm_desc_obs=np.full(n, -1, np.int32), lm_desc=np.zeros((n, 32), np.uint8), lm_normal=np.zeros((n, 3)),
                   lm_min_distance=np.zeros(n), lm_max_distance=np.zeros(n), lm_status=np.zeros(n, np.int32),
                   form_count=np.zeros(capi.LMR_FORMS, np.int32), kernel_ms=np.zeros(1))
        bp = _bp
        s = capi.LandmarkRefresh(K, L, iptr(ptr), iptr(okf), bp(desc), iptr(ooc), iptr(ref), dptr(pos), dptr(cen), bp(kinv), bp(linv),
                                 iptr(out["lm_desc_obs"]), bp(out["lm_desc"]), dptr(out["lm_normal"]), dptr(out["lm_min_distance"]),
                                 dptr(out["lm_max_distance"]), iptr(out["lm_status"]), iptr(out["form_count"]),
                                 dptr(out["kernel_ms"]) if want_kernel_ms else None)
        return s, o, out, [ptr, okf, ooc, ref, pos, cen, desc, kinv, linv]

    def refresh_landmarks(self, lm_obs_ptr, obs_kf, obs_desc, obs_octave, lm_ref_obs, lm_pos, kf_center, kf_invalid=None, lm_invalid=None,
                          kernel_ms: bool = False, **opts):
        """Landmark::ComputeDescriptor and Landmark::UpdateNormal for every landmark as one device call (covgpu_landmark_refresh,
        DESIGN.md §4.15). Observations are landmark-major in the order given (lm_obs_ptr [L+1], obs_kf [O] keyframe table indices);
        obs_desc [O,32] the observing keypoints' ORB rows or None (no descriptors asked for), obs_octave [O], lm_ref_obs [L] the position
        of the reference keyframe's observation in the landmark's list or -1, kf_center [K,3] the camera centres. `opts`: scale_factor
        (2.0), num_octaves (1). Returns dict(lm_desc_obs, lm_desc (both None without obs_desc), lm_normal, lm_min_distance,
        lm_max_distance, lm_status (bit 0 no valid observer, 1 no reference, 2 invalid landmark), form_count; kernel_ms if asked for)."""
        s, o, out, keep = self._refresh_batch(lm_obs_ptr, obs_kf, obs_desc, obs_octave, lm_ref_obs, lm_pos, kf_center, kf_invalid,
                                              lm_invalid, opts, kernel_ms)
        self._check(lib().covgpu_landmark_refresh(self._h, C.byref(s), C.byref(o)))
        L = s.num_lm
        r = {k: out[k][:L] for k in ("lm_normal", "lm_min_distance", "lm_max_distance", "lm_status")}
        has = obs_desc is not None
        r.update(lm_desc_obs=out["lm_desc_obs"][:L] if has else None, lm_desc=out["lm_desc"][:L] if has else None,
                 form_count=out["form_count"])
        if kernel_ms:
            r["kernel_ms"] = float(out["kernel_ms"][0])
        return r

    @staticmethod
    def _voc_train_batch(row_ptr, desc, k, L, weighting, seed, opts, node_capacity=None, want_row_word=False):
        """(VocTrain, VocTrainOpts, outputs, keep-alive list) of one covgpu_voc_train call."""
        ptr = _i32(row_ptr).ravel()
        d = _u8(desc).reshape(-1, 32)
        if len(ptr) < 1 or (len(ptr) > 1 and int(ptr[-1]) > len(d)):
            raise ValueError("row_ptr runs past desc")
        o = capi.VocTrainOpts()
        lib().covgpu_default_voc_train_opts(C.byref(o))
        o.k, o.L, o.weighting, o.seed = int(k), int(L), int(weighting), int(seed) & ((1 << 64) - 1)
        _set_opts(o, ("scoring", "max_iterations", "scratch_kib"), opts, "vocabulary-training", lambda k, v: int(v))
        rows = len(d)
        if node_capacity is None:                                  # every node the k-ary tree of depth L can have, or what the rows can fill
            full = sum(int(k) ** i for i in range(int(L) + 1)) if 2 <= int(k) <= 32 and 1 <= int(L) <= 20 else 1
            node_capacity = min(full, 2 * rows + 64)
        n = max(int(node_capacity), 1)
        out = dict(num_nodes=np.zeros(1, np.int32), num_words=np.zeros(1, np.int32), parent=np.full(n, -2, np.int32),
                   desc=np.zeros((n, 32), np.uint8), word_id=np.full(n, -2, np.int32), weight=np.full(n, -1.0),
                   row_word=np.full(max(rows, 1), -2, np.int32) if want_row_word else None, stats=np.zeros(8, np.int64))
        s = capi.VocTrain(len(ptr) - 1, iptr(ptr), _bp(d), int(node_capacity), iptr(out["num_nodes"]),
                          iptr(out["num_words"]), iptr(out["parent"]), _bp(out["desc"]), iptr(out["word_id"]),
                          dptr(out["weight"]), _opt(iptr, out["row_word"]),
                          out["stats"].ctypes.data_as(capi._lp))
        return s, o, out, [ptr, d]

    def train_vocabulary(self, row_ptr, desc, k, L, weighting=capi.BOW_TF_IDF, seed=0, node_capacity=None, row_word=False, **opts):
        """DBoW2's TemplatedVocabulary::create(training_features, k, L, weighting, L1_NORM) on the device (covgpu_voc_train, DESIGN.md
        §4.18). Descriptor sets as for bow_transform_batch: row_ptr [S+1], desc [rows,32]; empty sets count as documents. `opts`:
        scoring, max_iterations (100), scratch_kib. Returns (voc, stats): voc is the flat form of covins_amd/vocio.py, usable by bowdb,
        bow_transform_batch and vocio.write_text; stats maps capi.VOCTRAIN_STATS to ints, plus row_word (the transform leaf of every
        training row) if asked for. Without node_capacity a tree that outgrows the guess (emptied clusters only) is trained again with
        the count the first call reported."""
        from . import vocio
        s, o, out, keep = self._voc_train_batch(row_ptr, desc, k, L, weighting, seed, opts, node_capacity, row_word)
        rc = lib().covgpu_voc_train(self._h, C.byref(s), C.byref(o))
        if rc != 0 and node_capacity is None and int(out["num_nodes"][0]) > s.node_capacity:
            s, o, out, keep = self._voc_train_batch(row_ptr, desc, k, L, weighting, seed, opts, int(out["num_nodes"][0]), row_word)
            rc = lib().covgpu_voc_train(self._h, C.byref(s), C.byref(o))
        self._check(rc)
        N = int(out["num_nodes"][0])
        voc = vocio.from_nodes(o.k, o.L, o.scoring, o.weighting, out["parent"][1:N], out["word_id"][1:N] >= 0, out["desc"][1:N],
                               out["weight"][1:N])
        assert voc["num_words"] == int(out["num_words"][0]) and np.array_equal(voc["word_id"], out["word_id"][:N])
        stats = {name: int(v) for name, v in zip(capi.VOCTRAIN_STATS, out["stats"])}
        if row_word:
            stats["row_word"] = out["row_word"][:len(keep[1])]
        return voc, stats

    def p3p_batch(self, f, P):
        """covgpu_p3p_batch: f, P [n,4,3] -> (T [n,4,7] every solution, qx qy qz qw x y z, ascending v = s3/s1; nsol [n]; chosen [n], -1: none)."""
        f, P = _f64(f).reshape(-1, 4, 3), _f64(P).reshape(-1, 4, 3)
        n = f.shape[0]
        T = np.zeros((max(n, 1), 4, 7)); ns = np.zeros(max(n, 1), np.int32); ch = np.zeros(max(n, 1), np.int32)
        self._check(lib().covgpu_p3p_batch(self._h, n, dptr(f), dptr(P), dptr(T), iptr(ns), iptr(ch)))
        return T[:n], ns[:n], ch[:n]

    def set_profiling(self, on: bool):
        lib().covgpu_set_profiling(self._h, int(on))

    def profile(self) -> dict:
        out = np.zeros(16)
        lib().covgpu_get_profile2(self._h, dptr(out))
        return dict(build_ms=out[0], n_build=int(out[1]), factor_ms=out[2], n_factor=int(out[3]), syrk_ms=out[4],
                    n_syrk=int(out[5]), syrk_flops=out[6], offdiag_blocks=int(out[7]),
                    potrf_ms=out[8], n_potrf=int(out[9]), potrf_flops=out[10], plan_flops=out[11])

    def layout(self) -> dict:
        out = (C.c_int64 * 16)()
        lib().covgpu_get_layout(self._h, out)
        keys = ("shard_world", "shard_rank", "top_unknowns", "top_levels", "allreduce_kib", "stream_ordering", "dense_order", "covisible_pairs",
                "edge_pairs", "chains", "device_mib", "nd_fronts", "nd_levels", "nd_serial_panels", "nd_root_order", "nd_front_mib")
        return {k: int(out[i]) for i, k in enumerate(keys)}

    def kernel_forms(self) -> dict:
        """Launches per kernel form of the linear solves on this context since its last upload (include/covgpu.h lists the forms)."""
        names = kernel_form_names()
        out = (C.c_int64 * len(names))()
        lib().covgpu_get_kernel_forms(self._h, out, len(names))
        return {k: int(out[i]) for i, k in enumerate(names)}

    # ---- per-kernel entry points (tests)
    def residual_norms(self, prob, opt):
        out = np.zeros(prob.O); s = prob.as_struct()
        self._check(lib().covgpu_reprojection_residual_norms(self._h, C.byref(opt), C.byref(s), dptr(out)))
        return out

    def linearize_reprojection(self, prob, opt):
        O = prob.O
        r, Jp, Jl, c = np.zeros((O, 2)), np.zeros((O, 12)), np.zeros((O, 6)), np.zeros(O)
        s = prob.as_struct()
        self._check(lib().covgpu_linearize_reprojection(self._h, C.byref(opt), C.byref(s), dptr(r), dptr(Jp), dptr(Jl), dptr(c)))
        return r, Jp, Jl, c

    def preintegrate(self, prob, opt):
        I = prob.I
        d, J, P = np.zeros((I, 11)), np.zeros((I, 225)), np.zeros((I, 225))
        s = prob.as_struct()
        self._check(lib().covgpu_preintegrate(self._h, C.byref(opt), C.byref(s), dptr(d), dptr(J), dptr(P)))
        return d, J, P

    def linearize_imu(self, prob, opt):
        I = prob.I
        r, J = np.zeros((I, 15)), np.zeros((I, 450))
        s = prob.as_struct()
        self._check(lib().covgpu_linearize_imu(self._h, C.byref(opt), C.byref(s), dptr(r), dptr(J)))
        return r, J

    def linearize_between(self, prob, opt):
        E = prob.E
        r, J, c = np.zeros((E, 6)), np.zeros((E, 72)), np.zeros(E)
        s = prob.as_struct()
        self._check(lib().covgpu_linearize_between(self._h, C.byref(opt), C.byref(s), dptr(r), dptr(J), dptr(c)))
        return r, J, c

    def schur(self, prob, opt, mu, pgo=False):
        n = (6 if (pgo or opt.visual_only) else 15) * prob.K
        S, b, c = np.zeros((n, n)), np.zeros(n), np.zeros(1)
        s = prob.as_struct()
        fn = lib().covgpu_schur_pgo if pgo else lib().covgpu_schur
        self._check(fn(self._h, C.byref(opt), C.byref(s), float(mu), dptr(S), dptr(b), dptr(c)))
        return S, b, float(c[0])

    def gn_step(self, prob, opt, mu):
        """One damped Gauss-Newton step through the product solve path: (dx[n], dl[L,3], cost)."""
        n = (6 if opt.visual_only else 15) * prob.K
        dx, dl, c = np.zeros(n), np.zeros((prob.L, 3)), np.zeros(1)
        s = prob.as_struct()
        self._check(lib().covgpu_gn_step(self._h, C.byref(opt), C.byref(s), float(mu), dptr(dx), dptr(dl), dptr(c)))
        return dx, dl, float(c[0])

    @staticmethod
    def _marginal(kfs, block, mu, D):
        """(Marginal, cov, stats, keep-alive) of one marginal-covariance call; D = unknowns per keyframe of the problem."""
        if block not in ("pose", "full"):
            raise ValueError('block must be "pose" or "full"')
        kf = np.ascontiguousarray(kfs, np.int32).reshape(-1)
        m = len(kf) * (D if block == "full" else 6)
        cov = np.zeros((m, m)); stats = np.zeros(8, np.int64)
        s = capi.Marginal()
        s.num_kf = len(kf); s.kf = iptr(kf); s.block = 1 if block == "full" else 0; s.mu = float(mu)
        s.cov = dptr(cov); s.stats = stats.ctypes.data_as(capi._lp)
        return s, cov, stats, kf

    def marginal_covariance(self, prob, opt, kfs, block="pose", mu=0.0, pgo=False):
        """Joint marginal covariance of the keyframes `kfs` (problem indices, any order) at the estimate in `prob`: the rows and columns of
        the inverse of the reduced camera system at damping mu (covgpu_marginal_covariance). block "pose": 6 rows per
        keyframe (dtheta, dp); "full": all 15 of a visual-inertial problem. Returns (cov [m, m] in the order of kfs, stats dict)."""
        D = 6 if (pgo or opt.visual_only) else 15
        s, cov, stats, keep = self._marginal(kfs, block, mu, D)
        ps = prob.as_struct()
        self._keep = prob; self._keep_pgo = bool(pgo)
        self._check(lib().covgpu_marginal_covariance(self._h, C.byref(opt), C.byref(ps), 1 if pgo else 0, C.byref(s)))
        return cov, dict(zip(capi.MARGINAL_STATS, (int(v) for v in stats)))

    def marginal_covariance_resident(self, opt, kfs, block="pose", mu=0.0):
        """The same at the estimate the context holds (what download() returns), after upload() or a finished solve_resident()."""
        D = 6 if (self._keep_pgo or opt.visual_only) else 15
        s, cov, stats, keep = self._marginal(kfs, block, mu, D)
        self._check(lib().covgpu_marginal_resident(self._h, C.byref(opt), C.byref(s)))
        return cov, dict(zip(capi.MARGINAL_STATS, (int(v) for v in stats)))

    @staticmethod
    def _selinv(K, D, block, mu, pairs):
        """(Selinv, kf_cov, pair_cov, pair_ok, stats, keep-alive) of one selected-inverse call on K keyframes of D unknowns each."""
        if block not in ("pose", "full"):
            raise ValueError('block must be "pose" or "full"')
        d = D if block == "full" else 6
        pr = np.zeros((0, 2), np.int32) if pairs is None else np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        pi, pj = np.ascontiguousarray(pr[:, 0]), np.ascontiguousarray(pr[:, 1])
        kf_cov = np.zeros((K, d, d)); pair_cov = np.zeros((len(pr), d, d)); ok = np.zeros(len(pr), np.uint8); stats = np.zeros(8, np.int64)
        s = capi.Selinv()
        s.block = 1 if block == "full" else 0; s.mu = float(mu); s.kf_cov = dptr(kf_cov); s.num_pairs = len(pr)
        if len(pr):
            s.pair_i = iptr(pi); s.pair_j = iptr(pj); s.pair_cov = dptr(pair_cov); s.pair_ok = ok.ctypes.data_as(capi._bp)
        s.stats = stats.ctypes.data_as(capi._lp)
        return s, kf_cov, pair_cov, ok, stats, (pi, pj)

    def keyframe_covariances(self, prob, opt, block="pose", mu=0.0, pairs=None, pgo=False):
        """Covariance of EVERY keyframe at the estimate in `prob`, and the cross blocks of the keyframe pairs `pairs` ([P, 2] problem indices)
        that lie on the structure of the factor: the diagonal blocks, and the requested off-diagonal ones, of the inverse of the reduced
        camera system at damping mu (covgpu_selected_inverse). block "pose": 6 rows per keyframe; "full": all 15 of a
        visual-inertial problem. Returns (kf_cov [K, d, d] — zeros for a constant pose, pair_cov [P, d, d] = Sigma[rows of i][columns of j],
        pair_ok [P] uint8 — 0: not stored, block zeroed, stats dict)."""
        D = 6 if (pgo or opt.visual_only) else 15
        s, kf_cov, pair_cov, ok, stats, keep = self._selinv(prob.K, D, block, mu, pairs)
        ps = prob.as_struct()
        self._keep = prob; self._keep_pgo = bool(pgo)
        self._check(lib().covgpu_selected_inverse(self._h, C.byref(opt), C.byref(ps), 1 if pgo else 0, C.byref(s)))
        return kf_cov, pair_cov, ok, dict(zip(capi.SELINV_STATS, (int(v) for v in stats)))

    def keyframe_covariances_resident(self, opt, block="pose", mu=0.0, pairs=None):
        """The same at the estimate the context holds (what download() returns), after upload() or a finished solve_resident()."""
        D = 6 if (self._keep_pgo or opt.visual_only) else 15
        K = self._keep.K if self._keep is not None else 1   # (nothing uploaded: the call refuses before it writes)
        s, kf_cov, pair_cov, ok, stats, keep = self._selinv(K, D, block, mu, pairs)
        self._check(lib().covgpu_selected_inverse_resident(self._h, C.byref(opt), C.byref(s)))
        return kf_cov, pair_cov, ok, dict(zip(capi.SELINV_STATS, (int(v) for v in stats)))

    @staticmethod
    def _lmcov(L, K, mu, want_kf):
        """(Lmcov, lm_cov, lm_ok, kf_cov or None, stats) of one landmark-covariance call on L landmarks and K keyframes."""
        lm_cov = np.zeros((max(L, 1), 3, 3)); ok = np.zeros(max(L, 1), np.uint8); stats = np.zeros(8, np.int64)
        kf_cov = np.zeros((K, 6, 6)) if want_kf else None
        s = capi.Lmcov()
        s.mu = float(mu); s.lm_cov = dptr(lm_cov); s.lm_ok = ok.ctypes.data_as(capi._bp)
        if want_kf:
            s.kf_cov = dptr(kf_cov)
        s.stats = stats.ctypes.data_as(capi._lp)
        return s, lm_cov, ok, kf_cov, stats

    def landmark_covariances(self, prob, opt, mu=0.0, want_kf=False):
        """Covariance of EVERY landmark at the estimate in `prob`: the 3x3 diagonal blocks, at the landmarks, of the inverse of the whole
        system (poses, speed-biases, landmarks) at damping mu, from the selected inverse of the reduced camera system
        (covgpu_landmark_covariance). Returns (lm_cov [L, 3, 3] world frame, lm_ok [L] uint8 — 0: H_ll not positive
        definite, block zeroed, kf_cov [K, 6, 6] as keyframe_covariances(block="pose") or None, stats dict)."""
        s, lm_cov, ok, kf_cov, stats = self._lmcov(prob.L, prob.K, mu, want_kf)
        ps = prob.as_struct()
        self._keep = prob; self._keep_pgo = False
        self._check(lib().covgpu_landmark_covariance(self._h, C.byref(opt), C.byref(ps), C.byref(s)))
        return lm_cov[:prob.L], ok[:prob.L], kf_cov, dict(zip(capi.LMCOV_STATS, (int(v) for v in stats)))

    def landmark_covariances_resident(self, opt, mu=0.0, want_kf=False, num_lm=None):
        """The same at the estimate and the observation set the context holds, after upload() or a finished solve. num_lm: the landmarks
        of the resident observation set when it is not the uploaded one — after gba_two_round the landmarks with lm_left >= 2, in order."""
        K = self._keep.K if self._keep is not None else 1   # (nothing uploaded: the call refuses before it writes)
        L0 = self._keep.L if self._keep is not None else 1
        L = int(num_lm) if num_lm is not None else L0
        # (the library writes the resident set's landmarks, whatever num_lm says: never more than the uploaded problem's, so the buffers hold those)
        s, lm_cov, ok, kf_cov, stats = self._lmcov(max(L, L0), K, mu, want_kf)
        self._check(lib().covgpu_landmark_covariance_resident(self._h, C.byref(opt), C.byref(s)))
        return lm_cov[:L], ok[:L], kf_cov, dict(zip(capi.LMCOV_STATS, (int(v) for v in stats)))

    @staticmethod
    def _obscov(O, L, K, mu, want_cross, want_res, want_lm, want_kf):
        """(Obscov, outputs dict, stats) of one observation-covariance call on O observations, L landmarks and K keyframes."""
        O, L = max(O, 1), max(L, 1)
        out = dict(obs_cov=np.zeros((O, 2, 2)), obs_ok=np.zeros(O, np.uint8), cross_cov=np.zeros((O, 6, 3)) if want_cross else None,
                   obs_res=np.zeros((O, 2)) if want_res else None, lm_cov=np.zeros((L, 3, 3)) if want_lm else None,
                   lm_ok=np.zeros(L, np.uint8) if want_lm else None, kf_cov=np.zeros((K, 6, 6)) if want_kf else None)
        stats = np.zeros(8, np.int64)
        s = capi.Obscov()
        s.mu = float(mu)
        for f in ("obs_cov", "cross_cov", "obs_res", "lm_cov", "kf_cov"):
            if out[f] is not None:
                setattr(s, f, dptr(out[f]))
        for f in ("obs_ok", "lm_ok"):
            if out[f] is not None:
                setattr(s, f, out[f].ctypes.data_as(capi._bp))
        s.stats = stats.ctypes.data_as(capi._lp)
        return s, out, stats

    @staticmethod
    def _obscov_result(out, stats, O, L):
        cut = dict(obs_cov=O, obs_ok=O, cross_cov=O, obs_res=O, lm_cov=L, lm_ok=L)
        res = {f: (v if v is None or f not in cut else v[:cut[f]]) for f, v in out.items()}
        res["stats"] = dict(zip(capi.OBSCOV_STATS, (int(v) for v in stats)))
        return res

    def observation_covariances(self, prob, opt, mu=0.0, want_cross=True, want_res=True, want_lm=False, want_kf=False):
        """Covariance of EVERY observation o = (a, l) at the estimate in `prob` (covgpu_observation_covariance), in the
        landmark-major observation order of the problem: obs_cov [O, 2, 2] = J_o Sigma J_o^T (the block of the hat matrix, Sigma the inverse
        of the whole system at damping mu), cross_cov [O, 6, 3] = Sigma_al (pose rows of the observer by the landmark's coordinates), obs_res
        [O, 2] the whitened, loss-corrected residual, obs_ok [O] uint8 (0: the landmark is not served, blocks zeroed); lm_cov, lm_ok and
        kf_cov as landmark_covariances returns them. Returns a dict of these (None where not asked for) and "stats"."""
        s, out, stats = self._obscov(prob.O, prob.L, prob.K, mu, want_cross, want_res, want_lm, want_kf)
        ps = prob.as_struct()
        self._keep = prob; self._keep_pgo = False
        self._check(lib().covgpu_observation_covariance(self._h, C.byref(opt), C.byref(ps), C.byref(s)))
        return self._obscov_result(out, stats, prob.O, prob.L)

    def observation_covariances_resident(self, opt, mu=0.0, want_cross=True, want_res=True, want_lm=False, want_kf=False, num_obs=None,
                                         num_lm=None):
        """The same at the estimate and the observation stream the context holds, after upload() or a finished solve. num_obs / num_lm: the
        observations and landmarks of the resident stream when it is not the uploaded one — after gba_two_round the kept observations of
        the landmarks with lm_left >= 2, in order."""
        K = self._keep.K if self._keep is not None else 1   # (nothing uploaded: the call refuses before it writes)
        L0 = self._keep.L if self._keep is not None else 1
        O0 = self._keep.O if self._keep is not None else 1
        L = int(num_lm) if num_lm is not None else L0
        O = int(num_obs) if num_obs is not None else O0
        # (the library writes the resident stream, whatever the counts say: never more than the uploaded problem's, so the buffers hold those)
        s, out, stats = self._obscov(max(O, O0), max(L, L0), K, mu, want_cross, want_res, want_lm, want_kf)
        self._check(lib().covgpu_observation_covariance_resident(self._h, C.byref(opt), C.byref(s)))
        return self._obscov_result(out, stats, O, L)

    def solve_resident_traced(self, opt: Options, capacity: int = 64):
        """solve_resident that also returns the trust-region state at the end of every iteration, retry rounds included: (Result, trace
        [rounds, capi.TR_COUNT], columns capi.TR)."""
        r = Result(); tr = np.zeros((capacity, capi.TR_COUNT)); n = C.c_int32(0)
        self._check(lib().covgpu_solve_resident_traced(self._h, C.byref(opt), C.byref(r), dptr(tr), capacity, C.byref(n)))
        assert n.value <= capacity, (n.value, capacity)
        return r, tr[:n.value].copy()

    def fetch_tail_state(self, opt: Options) -> dict:
        """What the last iteration of the last solve of the resident problem left on the device: grad, hdiag, gn, vtmp [N], pose_c, sb_c, lm_c."""
        p = self._keep
        vi = not (self._keep_pgo or opt.visual_only)
        N = (15 if vi else 6) * p.K + (0 if self._keep_pgo else 3 * p.L)
        out = dict(grad=np.zeros(N), hdiag=np.zeros(N), gn=np.zeros(N), vtmp=np.zeros(N), pose_c=np.zeros((p.K, 7)), sb_c=np.zeros((p.K, 9)),
                   lm_c=np.zeros((0 if self._keep_pgo else p.L, 3)))
        self._check(lib().covgpu_fetch_tail_state(self._h, *(dptr(out[k]) for k in ("grad", "hdiag", "gn", "vtmp", "pose_c", "sb_c", "lm_c"))))
        return out

    def tail_logic_probe(self, opt: Options, kernel: int, tr, scal, flag0: int = 0, stage: int = 1, with_logic: bool = True, fresh: bool = True,
                         part=None):
        """One launch of the step logic on prescribed inputs (covgpu_tail_logic_probe; kernel = capi.TAIL_LOGIC ...): (tr, scal) afterwards."""
        tr = np.array(tr, dtype=np.float64); scal = np.array(scal, dtype=np.float64)
        assert tr.shape == (capi.TR_COUNT,) and scal.shape == (capi.SC_COUNT,)
        part_n = 0
        if part is not None:
            part = np.ascontiguousarray(part, dtype=np.float64)
            assert part.ndim == 2 and part.shape[0] == capi.SC_COUNT
            part_n = part.shape[1]
        self._check(lib().covgpu_tail_logic_probe(self._h, C.byref(opt), int(kernel), int(stage), int(bool(with_logic)), int(bool(fresh)), int(flag0),
                                                  dptr(tr), dptr(scal), dptr(part), part_n))
        return tr, scal

    def solve_reduced(self, S, b):
        S = np.ascontiguousarray(S, dtype=np.float64); b = np.ascontiguousarray(b, dtype=np.float64)
        x = np.zeros(b.shape[0])
        rc = lib().covgpu_solve_reduced(self._h, b.shape[0], dptr(S), dptr(b), dptr(x))
        return rc, x

    def pgo_reanchor(self, pose_old, pose_new, velocity, ref_kf, lm_pos):
        po = np.ascontiguousarray(pose_old, dtype=np.float64); pn = np.ascontiguousarray(pose_new, dtype=np.float64)
        vel = None if velocity is None else np.array(velocity, dtype=np.float64, order="C")
        lm = np.array(lm_pos, dtype=np.float64, order="C").reshape(-1, 3)
        ref = np.ascontiguousarray(ref_kf, dtype=np.int32)
        self._check(lib().covgpu_pgo_reanchor(self._h, po.shape[0], dptr(po), dptr(pn), dptr(vel), lm.shape[0], iptr(ref), dptr(lm)))
        return vel, lm
