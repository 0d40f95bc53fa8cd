"""Problems for the inertial path — k_preintegrate, imu_unwhitened / imu_stage (inertial_dev.hpp), k_imu_build, k_imu_gather, the IMU segments of
k_tail.hip and the inertial half of k_pose_finish (k_dense.hip) — shared by tests/test_imu_host.py (every point has the property it is named for;
the long double restatement of tests/imu_ref.py against the oracle) and tests/test_gpu_imu.py (the device against the restatement). No GPU code here.

Every point is built from base() = mapdata.flatten_gba(synth.make_map(synth.config_named("tiny")), False, True)[0]: K = 28, two chains of 14 keyframes
(agent A the even, agent B the odd keyframes; factor f joins keyframes f and f + 2, so the agents alternate from factor to factor and every workgroup
of four factors holds two of each), I = 26 factors of 50 samples, E = 1, keyframe 0 constant. The two keyframes of a factor carry the same bias to the
last bit on agent B and biases 2e-5 m/s^2 and 1e-7 rad/s apart on agent A (the map's bias random walk): the bias-correction terms of the factor meet
exact zeros or operands that small there, and no larger.

  id              construction                                                                            what it reaches
  bias-shift      along each chain keyframe k gets the bias b0 + s_k (b0: the chain's first keyframe), s_k     dba, dbg, the corrected dq_c, the block
                  uniform within 0.05 m/s^2 and 0.005 rad/s, drawn per keyframe; velocities moved by up        (3..5, 12..14) of the Jacobian
                  to 0.05 m/s
  bias-shift-one  only keyframe SHIFT_ONE_KF (the middle of chain A) shifted, by SHIFT_ONE                 the two factors at it see the shift in opposite roles
  ragged-cut      factor f keeps its first n_f samples, n_f from CUT_CYCLE = (2, 50, 7, 31, 50, 3, 16, 2):   nmax / on of k_preintegrate, dead waves
                  four different lengths in every workgroup, 2 beside 50, the last workgroup two live
                  and two dead waves
  count-I         I = 1, 3, 4, 5: only the first I factors, cut as ragged-cut; the other keyframes are       a grid of one workgroup, partial and full; the
                  chains of their own                                                                       identity speed-bias rows of keyframes without factor
  ragged-fused    SlamMap.remove_keyframes of FUSED_ERASED (three inner keyframes no two of which are        ragged lengths (100 and 150 among 50) in a problem that
                  neighbours, and two neighbours): consistent factors of 100 and 150 samples                 can be solved
  mixed-calib     imu_noise by agent: A the map's, B (3 sa, 0.3 sg, 0.3 saw, 3 sgw, 9.79)                     per-factor nd[] and gravity inside one workgroup
  fixed-inside    constant besides keyframe 0: one in the middle of chain A, the last of chain B, and both   the fi / fj branches, alone and together
                  keyframes of one factor of chain B
  edge-beside     base plus the loop edges (a, b) and (b, a), a = imu_kf_i[5], b = imu_kf_j[5]                the three-launch branch of enqueue_build (edge_beside_imu):
                                                                                                          a cross block fed by an IMU factor and two edges
  edge-far        base plus the edges EDGE_FAR: none between chain neighbours, keyframe 3 with four,         k_pose_finish with transposed entries and a keyframe of
                  one pair in both orientations                                                              several edges
  edge-none       flatten_gba(..., use_loops=False): E = 0                                                   the P.E > 0 guards of k_pose_finish
  one-sample      ragged-cut with the factors ONE_SAMPLE (first, inside a workgroup, last) cut to one        a factor of one sample carries no weight by rule

ragged-cut, count-I and one-sample cut sample lists: the motion no longer matches the poses there, the residuals are large, which a linearisation
does not mind. The points that run a solve keep consistent data. Edge measurements are the relative pose of the two keyframes composed with a
rotation of about 0.02 rad and a translation of a few centimetres, edge_sqrt_info = GBA_LOOP_SQRT_INFO, edge_loss_a = 1.
"""
import numpy as np
from scipy.spatial.transform import Rotation

from covins_amd import capi, mapdata, synth
from tests import imu_ref
from tests.lm_forms_util import MU_STEP, MUS_SCHUR, rel, scaled_err

CUT_CYCLE = (2, 50, 7, 31, 50, 3, 16, 2)
COUNTS = (1, 3, 4, 5)
SHIFT_ONE_KF = 12
SHIFT_ONE = np.array([0.05, -0.03, 0.02, 0.004, -0.006, 0.002])
FUSED_ERASED = (8, 18, 23, 9, 11)                      # 8, 18 (chain A) and 23 (chain B): no two neighbours; 9, 11: neighbours in chain B
MIXED_B = np.array([3.0, 0.3, 0.3, 3.0])               # agent B's sigmas over agent A's
MIXED_B_GRAVITY = 9.79
FIXED_INSIDE = (0, 12, 27, 9, 11)                      # the gauge, the middle of chain A, the last of chain B, both keyframes of factor 9
BESIDE_FACTOR = 5
EDGE_FAR = ((3, 20), (20, 3), (3, 21), (3, 24), (5, 20))
ONE_SAMPLE = (0, 13, 25)

IDS = (["bias-shift", "bias-shift-one", "ragged-cut"] + [f"count-{n}" for n in COUNTS]
       + ["ragged-fused", "mixed-calib", "fixed-inside", "edge-beside", "edge-far", "edge-none", "one-sample"])
STEP_IDS = ["bias-shift", "ragged-fused", "mixed-calib", "edge-beside", "edge-far", "edge-none"]
SOLVE_IDS = ["bias-shift", "ragged-fused", "edge-beside", "edge-far"]
EDGE_IDS = ["edge-beside", "edge-far"]
DEFAULT_CALIB_IDS = [i for i in IDS if i != "mixed-calib"]

_cache = {}


def base_map():
    if "map" not in _cache:
        _cache["map"] = synth.make_map(synth.config_named("tiny"))
    return _cache["map"]


def base():
    """The flattened `tiny` map; cached, treat as read-only."""
    if "base" not in _cache:
        _cache["base"] = mapdata.flatten_gba(base_map(), False, True)[0]
    return _cache["base"]


def chain_positions(p):
    """perm [K]: the chain-major position of every keyframe, as build_chains (plan_api.hip) lays the IMU chains out: keyframes without a
    predecessor in ascending order, each followed by its successors."""
    succ, has_pred = -np.ones(p.K, np.int64), np.zeros(p.K, bool)
    for i, j in zip(p.imu_kf_i, p.imu_kf_j):
        assert i != j and succ[i] == -1 and not has_pred[j]
        succ[i], has_pred[j] = j, True
    perm, pos = np.zeros(p.K, np.int64), 0
    for k in range(p.K):
        if has_pred[k]:
            continue
        c = k
        while c != -1:
            perm[c], pos, c = pos, pos + 1, succ[c]
    assert pos == p.K
    return perm


def cut_lengths(I):
    return np.resize(np.asarray(CUT_CYCLE, np.int64), I)


def with_factors(p, keep, lengths):
    """`p` with the IMU factors `keep` only, factor keep[q] holding its first lengths[q] samples."""
    q = p.copy()
    keep, lengths = np.asarray(keep, np.int64), np.asarray(lengths, np.int64)
    assert np.all(lengths <= np.diff(p.imu_sample_ptr)[keep]) and np.all(lengths >= 1)
    rows = np.concatenate([p.imu_sample_ptr[f] + np.arange(n) for f, n in zip(keep, lengths)])
    d = dict(q.__dict__)
    d.update(imu_kf_i=p.imu_kf_i[keep], imu_kf_j=p.imu_kf_j[keep], imu_first=p.imu_first[keep], imu_noise=p.imu_noise[keep],
             imu_samples=p.imu_samples[rows], imu_sample_ptr=np.concatenate([[0], np.cumsum(lengths)]))
    return capi.FlatProblem(**d)


def edge_measurement(p, a, b, rng):
    """[q, t] of T_a^-1 T_b at the problem's poses, composed with a rotation of about 0.02 rad and a translation of a few centimetres."""
    Ra, Rb = Rotation.from_quat(p.kf_pose[a, :4]), Rotation.from_quat(p.kf_pose[b, :4])
    w = rng.normal(0, 1, 3)
    Rm = Ra.inv() * Rb * Rotation.from_rotvec(0.02 * w / np.linalg.norm(w))
    q = Rm.as_quat()
    if q[3] < 0:
        q = -q
    t = Ra.inv().apply(p.kf_pose[b, 4:] - p.kf_pose[a, 4:]) + rng.uniform(-0.04, 0.04, 3)
    return np.concatenate([q, t])


def with_edges(p, edges, seed):
    """`p` plus the loop edges `edges`, each with a measurement of its own."""
    rng = np.random.default_rng(seed)
    q = p.copy()
    n = len(edges)
    d = dict(q.__dict__)
    d.update(edge_i=np.concatenate([p.edge_i, [a for a, _ in edges]]), edge_j=np.concatenate([p.edge_j, [b for _, b in edges]]),
             edge_meas=np.concatenate([p.edge_meas, np.array([edge_measurement(p, a, b, rng) for a, b in edges])]),
             edge_sqrt_info=np.concatenate([p.edge_sqrt_info, np.tile(mapdata.GBA_LOOP_SQRT_INFO.reshape(1, 36), (n, 1))]),
             edge_loss_a=np.concatenate([p.edge_loss_a, np.ones(n)]))
    return capi.FlatProblem(**d)


def beside_pair():
    p = base()
    return int(p.imu_kf_i[BESIDE_FACTOR]), int(p.imu_kf_j[BESIDE_FACTOR])


def build(pid):
    """The FlatProblem of point `pid`; cached, treat as read-only."""
    if pid in _cache:
        return _cache[pid]
    b = base()
    if pid == "bias-shift":
        p = b.copy()
        rng = np.random.default_rng(505)
        perm = chain_positions(b)
        first = {}                                                   # chain start of every keyframe
        for k in np.argsort(perm):
            pred = b.imu_kf_i[b.imu_kf_j == k]
            first[int(k)] = first[int(pred[0])] if len(pred) else int(k)
        for k in range(p.K):
            p.kf_speed_bias[k, 3:6] = b.kf_speed_bias[first[k], 3:6] + rng.uniform(-0.05, 0.05, 3)
            p.kf_speed_bias[k, 6:9] = b.kf_speed_bias[first[k], 6:9] + rng.uniform(-0.005, 0.005, 3)
            p.kf_speed_bias[k, 0:3] += rng.uniform(-0.05, 0.05, 3)
    elif pid == "bias-shift-one":
        p = b.copy()
        p.kf_speed_bias[SHIFT_ONE_KF, 3:9] += SHIFT_ONE
    elif pid == "ragged-cut":
        p = with_factors(b, np.arange(b.I), cut_lengths(b.I))
    elif pid.startswith("count-"):
        n = int(pid[6:])
        p = with_factors(b, np.arange(n), cut_lengths(n))
    elif pid == "ragged-fused":
        m = base_map().copy()
        assert m.remove_keyframes([(k, 0) for k in FUSED_ERASED]) == len(FUSED_ERASED)
        p = mapdata.flatten_gba(m, False, True)[0]
    elif pid == "mixed-calib":
        p = b.copy()
        agent_b = base_map().kf_client[p.imu_kf_j] == 1              # (no keyframe of `tiny` is invalid: problem rows are map rows)
        p.imu_noise[agent_b, :4] *= MIXED_B
        p.imu_noise[agent_b, 4] = MIXED_B_GRAVITY
    elif pid == "fixed-inside":
        p = b.copy()
        p.kf_fixed[list(FIXED_INSIDE)] = 1
    elif pid == "edge-beside":
        a, c = beside_pair()
        p = with_edges(b, [(a, c), (c, a)], seed=57)
    elif pid == "edge-far":
        p = with_edges(b, list(EDGE_FAR), seed=320)
    elif pid == "edge-none":
        p = mapdata.flatten_gba(base_map(), False, True, use_loops=False)[0]
    elif pid == "one-sample":
        n = cut_lengths(b.I)
        n[list(ONE_SAMPLE)] = 1
        p = with_factors(b, np.arange(b.I), n)
    else:
        raise KeyError(pid)
    p.validate()
    _cache[pid] = p
    return p


def zero_shift(pid):
    """bias-shift with every keyframe's bias put back to base()'s: the same poses and velocities, no shift."""
    assert pid == "bias-shift"
    p = build(pid).copy()
    p.kf_speed_bias[:, 3:9] = base().kf_speed_bias[:, 3:9]
    return p


# ------------------------------------------------------------------------------------------------ distances from the restatement
PRE_QUANTITIES = ("delta", "J", "P")
WHITE_QUANTITIES = ("r", "Jw", "JtJ", "Jtr")
EPS = 2.0 ** -52


def per_factor(x, ref):
    """[I] max |x_f - ref_f| / max |ref_f| in long double; a reference that is zero throughout asks for exact zeros."""
    I = ref.shape[0]
    x, ref = np.asarray(x, dtype=imu_ref.LD).reshape(I, -1), ref.reshape(I, -1)
    num, den = np.abs(x - ref).max(axis=1), np.abs(ref).max(axis=1)
    out = np.where(den > 0, num / np.where(den > 0, den, 1), np.where(num > 0, np.inf, 0.0))
    return out.astype(np.float64)


def distances(ref, pre=None, lin=None):
    """{quantity: [I] per-factor distance from the restatement `ref` (imu_ref.problem)} of a preintegration (delta, J, P) and / or a whitened
    linearisation (r [I,15], J [I,450]) given in double. J^T J and J^T r are formed in long double from the given r and J."""
    out = {}
    if pre is not None:
        for k, x in zip(PRE_QUANTITIES, pre):
            out[k] = per_factor(x, ref[k])
    if lin is not None:
        r, J = np.asarray(lin[0], dtype=imu_ref.LD), np.asarray(lin[1], dtype=imu_ref.LD).reshape(-1, 15, 30)
        out["r"], out["Jw"] = per_factor(r, ref["r"]), per_factor(J, ref["Jw"])
        out["JtJ"] = per_factor(np.einsum("fka,fkb->fab", J, J), ref["JtJ"])
        out["Jtr"] = per_factor(np.einsum("fka,fk->fa", J, r), ref["Jtr"])
    return out


def floors(ref):
    """{quantity: [I]}: 2^-52 x samples of the factor for the preintegration, 2^-52 x cond(chol P_ref) for the whitened quantities (a factor
    without weight: its zeros are exact, the floor is 0)."""
    fp = EPS * ref["n"].astype(np.float64)
    fw = np.where(np.isfinite(ref["cond"]) & (ref["n"] >= 2), EPS * ref["cond"], 0.0)
    return {**{k: fp for k in PRE_QUANTITIES}, **{k: fw for k in WHITE_QUANTITIES}}


def host_reference(pid):
    """Per point, computed once and shared by the host and the device test (read-only): ref = imu_ref.problem (long double), the oracle's
    preintegration and linearisation, e_orc = {quantity: the oracle's largest per-factor distance from the restatement} and floor = floors(ref)."""
    key = ("ref", pid)
    if key not in _cache:
        from oracle import covo
        p = build(pid)
        o = covo.default_options()
        ref = imu_ref.problem(p)
        pre, lin = covo.preintegrate(p, o), covo.linearize_imu(p, o)
        d = distances(ref, pre, lin)
        _cache[key] = dict(ref=ref, pre=pre, lin=lin, d_orc=d, e_orc={k: float(v.max()) for k, v in d.items()}, floor=floors(ref))
    return _cache[key]


def system_reference(pid):
    """The oracle's reduced systems {mu: (S, b, cost)} at MUS_SCHUR and MU_STEP, and for the points of STEP_IDS its whole-system step (x0, l0) at
    MU_STEP with d = sqrt(diag S) and the spread of its two solvers (tests/structure_util.host_reference); cached."""
    key = ("sys", pid)
    if key not in _cache:
        from oracle import covo
        p = build(pid)
        o = covo.default_options()
        out = dict(schur={mu: covo.schur(p, o, mu) for mu in MUS_SCHUR + ((MU_STEP,) if pid in STEP_IDS else ())})
        if pid in STEP_IDS:
            xs, ls = covo.step(p, o, MU_STEP, dense=False)
            xd, ld = covo.step(p, o, MU_STEP, dense=True)
            d = np.sqrt(np.abs(np.diag(out["schur"][MU_STEP][0])))
            out.update(x0=xd, l0=ld, d=d, h_pose=scaled_err(xs, xd, d), h_lm=rel(ls, ld))
        _cache[key] = out
    return _cache[key]
