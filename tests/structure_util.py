"""Problems with a PRESCRIBED covisibility structure for the code between the landmark-major kernels and the linear solve: the pair lists of
k_pairs.hip (build_pairs_device, build_kf_lists_device, round2_compact_device, k_obs_unpack), the two reductions of k_visual.hip that turn
per-observation records into the pose system (k_kf_reduce, k_pair_blocks), the edge gathers of k_between.hip (k_edge_gather_kf, k_edge_gather_pair)
and the host code that feeds them (build_chains of plan_api.hip; key_of_kf and the edge-pair lists of upload.hip). ONE table of points shared by the host test
(tests/test_structure_host.py: every point has the property it is named for) and the device test (tests/test_gpu_structure.py). No GPU code here.

The synthetic maps list every landmark's observers in ascending keyframe order, every IMU factor from the lower to the higher index, and leave
to chance which pair lands on a lane, trip, group, chunk or round boundary of k_pair_blocks. Here a problem is built from an explicit list of
TRACKS (the observing keyframes of each landmark, in the order given) on a ring of cameras looking at a cube of landmarks (ring_problem), and
relabel() renumbers a built problem at random — keyframes, landmarks, the observations inside every landmark, IMU factors, edges — together
with the maps that take results back to the original numbering.

Points (POINTS; two constant keyframes that share landmarks with free ones unless stated):
  pairs-N    N = 1, 8, 9, 512, 513, 4096, 4097 covisible pairs of free keyframes, each sharing exactly ONE landmark that those two keyframes
             alone observe (every second one listed from the higher to the lower index): the 8-pair groups, 64-workgroup chunks and the
             512-workgroup round of k_pair_blocks, and build_pairs_device's own scan buffer (2 pairs > entries). Every free keyframe also sees
             ANCHORS landmarks together with both constant keyframes, which pin it without adding a pair.
  lanes      pairs sharing exactly 1, 15, 16, 17, 31, 32, 33, 100 landmarks (16 lanes, two terms per trip, the zero-weight odd tail) and free
             keyframes with exactly 0, 1, 63, 64, 65, 129 observations (the 64-lane loop of k_kf_reduce); a keyframe without observations holds
             the highest index (the tail of kf_obs_ptr)
  bits-K     K = 2, 3, 4, 5, 64, 65, 128, 129 keyframes, random tracks of 2 .. 8 observers in random order, the highest index free and observing:
             the radix key width of k_pairs.hip on both sides of a power of two (K = 2: one constant keyframe)
  blocks-L-O L = 255, 256, 257 landmarks and O one below, at, one above a multiple of 256 observations (the 256-thread grids), landmarks with no
             and with one observation (by a constant keyframe) at index 0, at L - 1 and at the 255 / 256 seam
  relabel-ring   relabel() of a 40-keyframe, 600-landmark random point
  relabel-vi     relabel() of the flattened `tiny` map (visual-inertial, with its loop edge): IMU chains that run down the index range
  relabel-vi-reversed   the same renumbering with the loop edge reversed, (i, j, T) -> (j, i, T^-1): ANOTHER valid problem (below), held to the oracle
             only — the transposed edge block in the 15-dimensional layout
  lone-free  single-observation landmarks whose lone observer is a FREE keyframe, at index 0, at L - 1 and inside: that observation runs through
             the landmark pass, k_kf_reduce and the back-substitution. Held at mu = 1e-2 and at the step's 1e-4, not at 1e-8 (_lone_tracks)

relabel() can also reverse half of the edges, (i, j, T) -> (j, i, T^-1). That is another valid problem, not the same one: with e = q_m^-1 q_i^-1 q_j
the rotation rows turn exactly (vec e' = -R_m vec e) but the translation rows become -R(e)^T R_m^T t + R_m^T t_m instead of -R_m^T (t - t_m) — they differ
by (1 - R(e)^T) R_m^T t, first order in the edge's own residual. So relabel-vi keeps its edge's orientation (the oracle is invariant under it to
rounding, which the host test asserts to 1e-12), and reversed edges are held to the oracle directly: in the visual-inertial layout by
relabel-vi-reversed, in the 6-dimensional one on the pose graph of pose_graph_problem().
"""
from collections import namedtuple

import numpy as np
from scipy.spatial.transform import Rotation

from covins_amd import capi, synth
from tests.lm_forms_util import MU_STEP, MUS_SCHUR, rel, scaled_err

RADIUS = 4.0
ANCHORS = 5
EXTR_ROTVEC, EXTR_T = np.array([0.02, -0.03, 1.55]), np.array([-0.02, -0.06, 0.01])      # T_s_c: roughly the EuRoC mounting
Point = namedtuple("Point", "id kind arg")
Built = namedtuple("Built", "p info orig maps")
Relabel = namedtuple("Relabel", "kf lm obs imu edge flipped")      # old index -> new index; flipped [E] bool in the OLD edge numbering


# ------------------------------------------------------------------------------------------------ the builder
def _quat(Rm):
    q = Rotation.from_matrix(Rm).as_quat()
    q[q[:, 3] < 0] *= -1
    return q


def ring_poses(K):
    """True sensor poses T_w_s [K,7] of K keyframes on a circle of radius 4 m whose cameras look at the centre, with a small out-of-plane wobble."""
    th = 2 * np.pi * np.arange(K) / max(K, 1)
    pwc = np.stack([RADIUS * np.cos(th), RADIUS * np.sin(th), 0.25 * np.sin(3 * th + 0.4)], 1)
    z = -pwc / np.linalg.norm(pwc, axis=1, keepdims=True)
    x = np.cross(z, np.array([0.0, 0.0, 1.0])); x /= np.linalg.norm(x, axis=1, keepdims=True)
    Rwc = np.stack([x, np.cross(z, x), z], axis=2)
    wob = Rotation.from_rotvec(0.04 * np.stack([np.sin(2 * th), np.cos(5 * th), np.sin(7 * th + 1.0)], 1)).as_matrix()
    Rwc = Rwc @ wob
    Rsc = Rotation.from_rotvec(EXTR_ROTVEC).as_matrix()
    Rws = Rwc @ Rsc.T
    return np.concatenate([_quat(Rws), pwc - Rws @ EXTR_T], 1)


def project(pose, lw):
    """Pixels [n,2] and camera-frame depth [n] of world points lw [n,3] seen from sensor poses pose [n,7] by THE camera of a ring problem (pinhole +
    RadTan with the EuRoC intrinsics of covins_amd.synth)."""
    Rws = Rotation.from_quat(pose[:, :4]).as_matrix()
    Rsc = Rotation.from_rotvec(EXTR_ROTVEC).as_matrix()
    ls = np.einsum("nji,nj->ni", Rws, lw - pose[:, 4:])
    lc = (ls - EXTR_T) @ Rsc
    x, y = lc[:, 0] / lc[:, 2], lc[:, 1] / lc[:, 2]
    k1, k2, p1, p2 = synth.DIST
    r2 = x * x + y * y
    rad = k1 * r2 + k2 * r2 * r2
    xd = x + x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y + y * rad + 2 * p2 * x * y + p1 * (r2 + 2 * y * y)
    fx, fy, cx, cy = synth.INTR
    return np.stack([fx * xd + cx, fy * yd + cy], 1), lc[:, 2]


def ring_problem(K, tracks, fixed, seed, noise_px=0.5, perturb=True):
    """FlatProblem of K ring keyframes and one landmark per track (its observing keyframes, in the order given; an empty track is a landmark nobody
    observes): landmarks uniform in the cube of +-1 m at the centre (in front of every camera), keypoints = exact projections + N(0, noise_px),
    obs_sigma 1, free poses perturbed by 1 cm / 2 mrad and landmarks by 2 cm, keyframes `fixed` constant, no IMU factors, no edges."""
    rng = np.random.default_rng(seed)
    L = len(tracks)
    n = np.array([len(t) for t in tracks], np.int64)
    obs_kf = np.concatenate([np.asarray(t, np.int64) for t in tracks] + [np.zeros(0, np.int64)])
    obs_lm = np.repeat(np.arange(L), n)
    assert K > 0 and (len(obs_kf) == 0 or (obs_kf.min() >= 0 and obs_kf.max() < K))
    pose = ring_poses(K)
    lm = rng.uniform(-1.0, 1.0, (L, 3))
    uv, depth = project(pose[obs_kf], lm[obs_lm])
    assert len(depth) == 0 or depth.min() > 1.0
    uv = uv + rng.normal(0.0, noise_px, uv.shape)
    kf_fixed = np.zeros(K, np.uint8); kf_fixed[list(fixed)] = 1
    if perturb:
        free = kf_fixed == 0
        dq = Rotation.from_rotvec(rng.normal(0.0, 0.002, (K, 3)))
        q = (Rotation.from_quat(pose[:, :4]) * dq).as_quat(); q[q[:, 3] < 0] *= -1
        pose[free, :4] = q[free]
        pose[free, 4:] += rng.normal(0.0, 0.01, (K, 3))[free]
        lm = lm + rng.normal(0.0, 0.02, (L, 3))
    Rsc = Rotation.from_rotvec(EXTR_ROTVEC)
    qsc = Rsc.as_quat(); qsc = -qsc if qsc[3] < 0 else qsc
    return capi.FlatProblem(kf_pose=pose, kf_speed_bias=np.zeros((K, 9)), kf_fixed=kf_fixed, kf_cam=np.zeros(K, np.int32),
                            cam_extr=np.concatenate([qsc, EXTR_T])[None], cam_intr=synth.INTR[None], cam_dist=synth.DIST[None], cam_dist_type=[0],
                            lm_pos=lm, lm_obs_ptr=np.concatenate([[0], np.cumsum(n)]), obs_kf=obs_kf, obs_uv=uv, obs_sigma=np.ones(len(obs_kf)))


def relabel(p, seed, flip_edges=True):
    """(q, Relabel): `p` under a random renumbering of its keyframes and landmarks, of the observations inside every landmark, of the IMU factors
    (with their sample ranges) and of the edges, half of which are reversed with the inverted measurement when flip_edges is set. The ARRAYS of p are
    permuted: nothing is drawn again, every number of q is a number of p."""
    rng = np.random.default_rng(seed)
    K, L, O, I, E = p.K, p.L, p.O, p.I, p.E
    kf_new = rng.permutation(K)
    lm_new = rng.permutation(L)
    lm_old = np.argsort(lm_new)                                     # old landmark at every new position
    n = np.diff(p.lm_obs_ptr).astype(np.int64)
    rows = np.concatenate([p.lm_obs_ptr[l] + rng.permutation(n[l]) for l in lm_old] + [np.zeros(0, np.int64)]).astype(np.int64)
    obs_new = np.empty(O, np.int64); obs_new[rows] = np.arange(O)
    d = {k: (None if v is None else np.array(v, copy=True)) for k, v in p.__dict__.items()}
    for name in ("kf_pose", "kf_speed_bias", "kf_fixed", "kf_cam"):
        d[name] = np.empty_like(getattr(p, name)); d[name][kf_new] = getattr(p, name)
    d["lm_pos"] = p.lm_pos[lm_old]
    d["lm_obs_ptr"] = np.concatenate([[0], np.cumsum(n[lm_old])])
    d["obs_kf"] = kf_new[p.obs_kf[rows]]; d["obs_uv"] = p.obs_uv[rows]; d["obs_sigma"] = p.obs_sigma[rows]
    f_old = rng.permutation(I)                                      # old factor at every new position
    imu_new = np.empty(I, np.int64); imu_new[f_old] = np.arange(I)
    if I:
        ns = np.diff(p.imu_sample_ptr).astype(np.int64)
        srows = np.concatenate([p.imu_sample_ptr[f] + np.arange(ns[f]) for f in f_old]).astype(np.int64)
        d["imu_kf_i"] = kf_new[p.imu_kf_i[f_old]]; d["imu_kf_j"] = kf_new[p.imu_kf_j[f_old]]
        d["imu_sample_ptr"] = np.concatenate([[0], np.cumsum(ns[f_old])]); d["imu_samples"] = p.imu_samples[srows]
        d["imu_first"] = p.imu_first[f_old]
        if p.imu_noise is not None:
            d["imu_noise"] = p.imu_noise[f_old]
    e_old = rng.permutation(E)
    edge_new = np.empty(E, np.int64); edge_new[e_old] = np.arange(E)
    flipped = np.zeros(E, bool)
    if E:
        if flip_edges:
            flipped[rng.permutation(E)[:(E + 1) // 2]] = True
        ei, ej, meas = p.edge_i.copy(), p.edge_j.copy(), p.edge_meas.copy()
        if flipped.any():
            Rm = Rotation.from_quat(meas[flipped, :4])
            qi = Rm.inv().as_quat().reshape(-1, 4); qi[qi[:, 3] < 0] *= -1
            meas[flipped, :4] = qi; meas[flipped, 4:] = -Rm.inv().apply(meas[flipped, 4:]).reshape(-1, 3)
            ei[flipped], ej[flipped] = p.edge_j[flipped], p.edge_i[flipped]
        d["edge_i"] = kf_new[ei[e_old]]; d["edge_j"] = kf_new[ej[e_old]]; d["edge_meas"] = meas[e_old]
        d["edge_sqrt_info"] = p.edge_sqrt_info[e_old]; d["edge_loss_a"] = p.edge_loss_a[e_old]
    return capi.FlatProblem(**d), Relabel(kf_new, lm_new, obs_new, imu_new, edge_new, flipped)


def rows_of(kf_new, D):
    """Rows of the relabelled reduced system (D per keyframe) in the ORIGINAL keyframe order: S_back = S_new[np.ix_(r, r)], b_back = b_new[r]."""
    return (D * np.asarray(kf_new)[:, None] + np.arange(D)[None, :]).reshape(-1)


# ------------------------------------------------------------------------------------------------ incidence (numpy / scipy.sparse only)
def incidence(p):
    """(W [K,K] int: common landmarks of every keyframe pair = A^T A of the landmark x keyframe incidence matrix, observations per keyframe [K])."""
    import scipy.sparse as sp
    obs_lm = np.repeat(np.arange(p.L), np.diff(p.lm_obs_ptr))
    A = sp.csr_matrix((np.ones(p.O), (obs_lm, p.obs_kf)), shape=(p.L, p.K))
    return (A.T @ A).toarray().astype(np.int64), np.bincount(p.obs_kf, minlength=p.K)


def covisible_triples(W, th):
    i, j = np.nonzero(np.tril(W, -1) >= th)            # row-major: ascending i, then ascending j < i (the order covgpu_covisibility returns)
    return list(zip(i.tolist(), j.tolist(), W[i, j].tolist()))


def free_pairs(p, W=None):
    """Covisible pairs among FREE keyframes: the off-diagonal blocks of the reduced system the landmarks create (Context.layout()['covisible_pairs'])."""
    W = incidence(p)[0] if W is None else W
    free = p.kf_fixed == 0
    return int(((np.tril(W, -1) > 0) & free[:, None] & free[None, :]).sum())


# ------------------------------------------------------------------------------------------------ the points
PAIRS_N = (1, 8, 9, 512, 513, 4096, 4097)
LANES_SHARED = (1, 15, 16, 17, 31, 32, 33, 100)
LANES_NOBS = (0, 1, 63, 64, 65, 129)
BITS_K = (2, 3, 4, 5, 64, 65, 128, 129)
BLOCKS_L = (255, 256, 257)
BLOCKS_O = (1023, 1024, 1025)
# (landmarks without an observation, landmarks with one) per L: index 0, L - 1 and both sides of the 255 / 256 seam each see both kinds
BLOCKS_SPECIAL = {255: ((0, 254), (1, 253)), 256: ((255,), (0, 254)), 257: ((1, 254), (0, 255, 256))}
POINTS = ([Point(f"pairs-{N}", "pairs", N) for N in PAIRS_N] + [Point("lanes", "lanes", None)] + [Point(f"bits-{K}", "bits", K) for K in BITS_K]
          + [Point(f"blocks-L{L}-O{O}", "blocks", (L, O)) for L in BLOCKS_L for O in BLOCKS_O]
          + [Point("relabel-ring", "relabel-ring", None), Point("relabel-vi", "relabel-vi", None), Point("relabel-vi-reversed", "relabel-vi-reversed", None),
             Point("lone-free", "lone", None)])
IDS = [pt.id for pt in POINTS]
RELABELLED = [pt for pt in POINTS if pt.kind in ("relabel-ring", "relabel-vi")]      # the same problem renumbered (relabel-vi-reversed is another one)
BY_ID = {pt.id: pt for pt in POINTS}
_built, _ref = {}, {}


def pairs_free_count(N):
    """Smallest number of free keyframes with N pairs among them."""
    F = 2
    while F * (F - 1) // 2 < N:
        F += 1
    return F


def _pairs_tracks(N):
    F = pairs_free_count(N)
    K = F + 2
    fixed = (1, K // 2)                                              # constant keyframes inside the index range: key_of_kf is no shift of the index
    free = [k for k in range(K) if k not in fixed]
    tracks, q = [], 0
    for i in range(F):
        for j in range(i):
            if q < N:
                tracks.append((free[i], free[j]) if q % 2 else (free[j], free[i]))
                q += 1
    for a, f in enumerate(free):                                     # anchors: constant - free covisibility, which must not create a pair
        for s in range(ANCHORS):
            tracks.append([(fixed[0], f, fixed[1]), (f, fixed[1], fixed[0]), (fixed[1], fixed[0], f)][(a + s) % 3])
    return K, tracks, fixed


def _lanes_tracks():
    fixed = (0, 9)
    pair_kf, nobs_kf, k = [], {}, 1
    def take():
        nonlocal k
        while k in fixed:
            k += 1
        k += 1
        return k - 1
    for _ in LANES_SHARED:
        pair_kf.append((take(), take()))
    for n in LANES_NOBS[2:]:
        nobs_kf[n] = take()
    empty = [take(), take()]                                         # the second one is the highest index
    K = k
    tracks = []
    for m, ((a, b), n) in enumerate(zip(pair_kf, LANES_SHARED)):     # a constant observer pins the shared landmarks and adds no pair
        for s in range(n):
            tracks.append([(b, fixed[0], a), (a, b, fixed[1]), (fixed[1], b, a)][(m + s) % 3])
    for n, e in nobs_kf.items():
        for s in range(n):
            tracks.append((fixed[0], e, fixed[1]) if s % 2 else (e, fixed[1], fixed[0]))
    return K, tracks, fixed, dict(pair_kf=pair_kf, nobs_kf=nobs_kf, empty=empty)


def _random_tracks(rng, K, L, lo=2, hi=8):
    tracks = []
    for _ in range(L):
        n = int(rng.integers(lo, min(hi, K) + 1))
        tracks.append(rng.permutation(K)[:n].tolist())
    return tracks


def _bits_tracks(K):
    rng = np.random.default_rng(700 + K)
    fixed = (0,) if K == 2 else (0, K // 2)
    tracks = _random_tracks(rng, K, max(40, 5 * K))
    assert any(K - 1 in t for t in tracks)
    return K, tracks, fixed


def _blocks_tracks(L, O):
    rng = np.random.default_rng(1000 * L + O)
    K = 20
    zero, one = BLOCKS_SPECIAL[L]
    n = rng.integers(2, 7, L)
    n[list(zero)] = 0; n[list(one)] = 1
    plain = np.array([l for l in range(L) if l not in zero and l not in one])
    while n.sum() != O:                                              # adjust plain tracks inside 2 .. 8 until the total is exactly O
        l = plain[rng.integers(len(plain))]
        step = 1 if n.sum() < O else -1
        if 2 <= n[l] + step <= 8:
            n[l] += step
    # the lone observer of a single-observation landmark is a CONSTANT keyframe: seen by a free one, its damped H_ll (rank 2 + mu diag) has a condition
    # of 1 / mu and the oracle's own S at mu = 1e-8 is off a long-double evaluation of the same blocks by 1.3e-9 .. 1.7e-9 — more than the bound the
    # device is held to (with constant lone observers: 3.6e-15; both figures are asserted by tests/test_structure_host.py on lone-free and on a blocks
    # point, with schur_long_double below). The landmark keeps its place in every list either way; lone-free gives it a free observer.
    tracks = [rng.permutation(K)[:m].tolist() if m != 1 else [(3, 11)[int(rng.integers(2))]] for m in n]
    return K, tracks, (3, 11)


LONE_K, LONE_L, LONE_FIXED = 20, 70, (3, 11)
LONE_AT = {0: 7, 33: 19, 34: 3, LONE_L - 1: 12}                      # landmark -> its lone observer (3 is constant, the others are free; 19 = K - 1)


def _lone_tracks():
    """Single-observation landmarks seen by FREE keyframes. The damped H_ll of such a landmark is rank 2 + mu diag, of condition 1 / mu, and what it
    leaves of its observer's diagonal block is a difference of nearly equal numbers: any double evaluation of S carries a relative error of about
    eps / mu there — 2e-8 at mu = 1e-8, above the 1e-9 the Schur comparison asks for, whoever computes it, the oracle included (that is why the blocks-*
    points give their single observations to a constant keyframe); 2e-14 at mu = 1e-2 and 2e-12 at the step's mu = 1e-4. So this point is held at
    mu = 1e-2 (schur_mus) and by its step, whose bound follows the oracle's own spread."""
    rng = np.random.default_rng(2070)
    tracks = _random_tracks(rng, LONE_K, LONE_L, 2, 6)
    for l, k in LONE_AT.items():
        tracks[l] = [k]
    return LONE_K, tracks, LONE_FIXED


def tiny_vi_problem():
    from covins_amd import mapdata
    return mapdata.flatten_gba(synth.make_map(synth.config_named("tiny")), False, True)[0]


RELABEL_VI_SEED = 4


def build(pt):
    """Built(problem, facts the tests rely on, the original problem and the Relabel maps of a relabelled point); cached, treat as read-only."""
    if pt.id in _built:
        return _built[pt.id]
    info, orig, maps = {}, None, None
    if pt.kind == "pairs":
        K, tracks, fixed = _pairs_tracks(pt.arg)
        p = ring_problem(K, tracks, fixed, seed=pt.arg)
        info = dict(free=pairs_free_count(pt.arg))
    elif pt.kind == "lanes":
        K, tracks, fixed, info = _lanes_tracks()
        p = ring_problem(K, tracks, fixed, seed=77)
    elif pt.kind == "bits":
        K, tracks, fixed = _bits_tracks(pt.arg)
        p = ring_problem(K, tracks, fixed, seed=300 + pt.arg)
    elif pt.kind == "blocks":
        K, tracks, fixed = _blocks_tracks(*pt.arg)
        p = ring_problem(K, tracks, fixed, seed=pt.arg[0] + pt.arg[1])
    elif pt.kind == "lone":
        K, tracks, fixed = _lone_tracks()
        p = ring_problem(K, tracks, fixed, seed=2071)
    elif pt.kind == "relabel-ring":
        rng = np.random.default_rng(40600)
        orig = ring_problem(40, [sorted(t) for t in _random_tracks(rng, 40, 600)], (0, 20), seed=40)
        p, maps = relabel(orig, seed=1)
    else:
        orig = tiny_vi_problem()
        p, maps = relabel(orig, seed=RELABEL_VI_SEED, flip_edges=pt.kind == "relabel-vi-reversed")
    p.validate()
    _built[pt.id] = Built(p, info, orig, maps)
    return _built[pt.id]


def options_kw(pt):
    return dict(visual_only=0 if pt.kind.startswith("relabel-vi") else 1)


def schur_mus(pt):
    """The damping values at which the point's S and b are compared: MUS_SCHUR, without 1e-8 for lone-free (_lone_tracks)."""
    return tuple(mu for mu in MUS_SCHUR if pt.kind != "lone" or mu >= MU_STEP)


# ------------------------------------------------------------------------------------------------ host references
DENSE_MAX_N = 2500


def sparse_full_step(p, o, mu):
    """The damped Gauss-Newton step of the WHOLE system (poses and landmarks, no Schur complement) of a visual-only problem from the oracle's
    per-observation blocks (covo.linearize_reprojection), by SuperLU: what covo.step(dense=True) solves, with the same damping (mu clamp(sqrt(diag
    J^T J), 1e-6, 1e32)^2; an unknown nobody constrains gets a unit diagonal and no step), for systems its dense Cholesky is too slow for."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    from oracle import covo
    assert o.visual_only and p.I == 0 and p.E == 0                  # 6 columns per keyframe, reprojection rows only
    r, Jp, Jl, _ = covo.linearize_reprojection(p, o)
    O, K, L = p.O, p.K, p.L
    obs_lm = np.repeat(np.arange(L), np.diff(p.lm_obs_ptr))
    row = np.repeat(np.arange(2 * O).reshape(O, 2), 6, axis=1).reshape(-1)
    colp = np.tile(6 * p.obs_kf[:, None] + np.arange(6)[None, :], (1, 2)).reshape(-1)
    row3 = np.repeat(np.arange(2 * O).reshape(O, 2), 3, axis=1).reshape(-1)
    coll = 6 * K + np.tile(3 * obs_lm[:, None] + np.arange(3)[None, :], (1, 2)).reshape(-1)
    N = 6 * K + 3 * L
    J = sp.csr_matrix((np.concatenate([Jp.reshape(-1), Jl.reshape(-1)]), (np.concatenate([row, row3]), np.concatenate([colp, coll]))), shape=(2 * O, N))
    H = (J.T @ J).tocsc()
    g = J.T @ r.reshape(-1)
    dg = H.diagonal()
    live = dg != 0.0
    add = np.where(live, mu * np.clip(np.sqrt(np.maximum(dg, 0.0)), 1e-6, 1e32) ** 2, 1.0)
    x = spla.splu((H + sp.diags(add)).tocsc(), permc_spec="MMD_AT_PLUS_A", diag_pivot_thresh=0.0, options=dict(SymmetricMode=True)).solve(-g)
    x[~live] = 0.0
    return x[:6 * K], x[6 * K:].reshape(L, 3)


def host_reference(pt):
    """Per point, computed once and shared (read-only): the oracle's Schur complements {mu: (S, b, cost)} at MUS_SCHUR and MU_STEP, the reference step
    (x0, l0) at MU_STEP with d = sqrt(diag S), and the spread of the oracle's two solvers of that step in the metrics the device is held to
    (tests/lm_forms_util.host_reference): h_pose = scaled_err(Schur step, whole-system step), h_lm = rel(...). The whole-system step is covo.step(dense=True)
    up to DENSE_MAX_N unknowns and sparse_full_step above (visual-only points: it asserts that)."""
    if pt.id in _ref:
        return _ref[pt.id]
    from oracle import covo
    p = build(pt).p
    o = covo.default_options(**options_kw(pt))
    schur = {mu: covo.schur(p, o, mu) for mu in MUS_SCHUR + (MU_STEP,)}
    D = 6 if o.visual_only else 15
    N = D * p.K + 3 * p.L
    xs, ls = covo.step(p, o, MU_STEP, dense=False)
    xd, ld = covo.step(p, o, MU_STEP, dense=True) if N <= DENSE_MAX_N else sparse_full_step(p, o, MU_STEP)
    d = np.sqrt(np.abs(np.diag(schur[MU_STEP][0])))
    _ref[pt.id] = dict(schur=schur, x0=xd, l0=ld, d=d, h_pose=scaled_err(xs, xd, d), h_lm=rel(ls, ld), N=N, whole="dense" if N <= DENSE_MAX_N else "sparse")
    return _ref[pt.id]


def schur_long_double(p, o, mu):
    """S [6K,6K] of a visual-only problem from the oracle's per-observation blocks (covo.linearize_reprojection), accumulated, damped and eliminated in
    long double (the 3 x 3 inverse by the adjugate): what covo.schur computes in double, with the damping of sparse_full_step. It measures the ORACLE's
    rounding error where the text above argues with it (_blocks_tracks, _lone_tracks); tests/test_structure_host.py asserts the figures."""
    LD = np.longdouble
    assert o.visual_only and p.I == 0 and p.E == 0
    from oracle import covo
    _, Jp, Jl, _ = covo.linearize_reprojection(p, o)
    O, K = p.O, p.K
    Jp, Jl = Jp.reshape(O, 2, 6).astype(LD), Jl.reshape(O, 2, 3).astype(LD)
    damp = lambda d: LD(mu) * np.clip(np.sqrt(d), LD(1e-6), LD(1e32)) ** 2
    S = np.zeros((6 * K, 6 * K), LD)
    for i in range(O):
        k = 6 * p.obs_kf[i]
        S[k:k + 6, k:k + 6] += Jp[i].T @ Jp[i]
    d = np.diag(S).copy()
    S[np.arange(6 * K), np.arange(6 * K)] += np.where(d != 0, damp(d), LD(0))
    for l in range(p.L):
        rows = range(p.lm_obs_ptr[l], p.lm_obs_ptr[l + 1])
        if len(rows) == 0:
            continue
        H = sum(Jl[i].T @ Jl[i] for i in rows)
        H = H + np.diag(damp(np.diag(H).copy()))
        c = np.array([[H[(i + 1) % 3, (j + 1) % 3] * H[(i + 2) % 3, (j + 2) % 3] - H[(i + 1) % 3, (j + 2) % 3] * H[(i + 2) % 3, (j + 1) % 3]
                       for i in range(3)] for j in range(3)], LD)
        Hi = c / (H[0] @ c[:, 0])
        W = {i: Jp[i].T @ Jl[i] for i in rows}
        for i in rows:
            for j in rows:
                ki, kj = 6 * p.obs_kf[i], 6 * p.obs_kf[j]
                S[ki:ki + 6, kj:kj + 6] -= W[i] @ Hi @ W[j].T
    return S


# ------------------------------------------------------------------------------------------------ the second round on planted erasures
ERASE_K, ERASE_L, ERASE_FIXED, ERASE_NOISE, ERASE_SHIFT, ERASE_THRESHOLD = 12, 300, (0, 6), 0.05, 40.0, 0.92
ERASE_PATTERNS = ("none", "first-and-last", "left-with-1-and-2", "middle-keyframe", "last-keyframe", "all-but-one")
ERASE_FREE_ALL_BUT_ONE = (3, 9)
_erase = {}


def erase_base(name="none"):
    """The ring problem of the second-round patterns: 12 keyframes, 300 landmarks, random tracks of 2 .. 8 observations (landmark 0: six, see
    displaced()), pixel noise 0.05, keyframes 0 and 6 constant.
    'all-but-one' has a base of its own, for the reason displaced_across() gives: the same sizes, but every keyframe constant except
    ERASE_FREE_ALL_BUT_ONE, and those two observe the surviving landmark and nothing else."""
    if "base" not in _erase:
        rng = np.random.default_rng(12300)
        tracks = _random_tracks(rng, ERASE_K, ERASE_L)
        tracks[0] = rng.permutation(ERASE_K)[:6].tolist()
        _erase["base"] = ring_problem(ERASE_K, tracks, ERASE_FIXED, seed=123, noise_px=ERASE_NOISE)
        others = np.array([k for k in range(ERASE_K) if k not in ERASE_FREE_ALL_BUT_ONE])
        tracks = [others[t].tolist() for t in _random_tracks(rng, len(others), ERASE_L)]
        tracks[ERASE_L // 2] = [ERASE_FREE_ALL_BUT_ONE[1], 0, 7, ERASE_FREE_ALL_BUT_ONE[0], 4]
        _erase["base-all"] = ring_problem(ERASE_K, tracks, others, seed=124, noise_px=ERASE_NOISE)
    return _erase["base-all" if name == "all-but-one" else "base"]


def planted_rows(name):
    """Observation rows of erase_base(name) whose keypoint is displaced, per pattern."""
    p = erase_base(name)
    ptr, n, L = p.lm_obs_ptr, np.diff(p.lm_obs_ptr), p.L
    rows = lambda l, m=None: list(range(ptr[l], ptr[l + 1] if m is None else ptr[l] + m))
    if name == "none":
        out = []
    elif name == "first-and-last":
        out = rows(0) + rows(L - 1)
    elif name == "left-with-1-and-2":                                # all but one observation of every 7th landmark and of L - 1, all but two of every 7th + 3 and of L - 3
        out = []
        for l in sorted(set(range(2, L, 7)) | {L - 1}):
            out += rows(l, n[l] - 1)
        for l in sorted((set(range(5, L, 7)) | {L - 3}) - set(range(2, L, 7)) - {L - 1}):
            if n[l] > 2:
                out += rows(l, n[l] - 2)
    elif name == "middle-keyframe":
        out = np.nonzero(p.obs_kf == 5)[0].tolist()
    elif name == "last-keyframe":
        out = np.nonzero(p.obs_kf == p.K - 1)[0].tolist()
    else:
        keep = L // 2
        out = [o for l in range(L) if l != keep for o in rows(l)[1:]]
    return np.array(sorted(set(out)), np.int64)


def displaced(pb, rows, seed):
    """`pb` with the keypoints of `rows` displaced by at least ERASE_SHIFT px each, in directions no estimate can follow.

    Random +-40 px do not survive the outlier round where nothing clean holds the unknowns they act on (every observation of a landmark, every
    observation of a keyframe): Gauss-Newton moves that landmark or pose to the consistent part of the displacements, the robust weights then favour
    the observations it came closer to, and after five iterations it FITS a subset, which the round no longer erases. So the displacements are
    built to leave the reweighted normal equations alone: with J the oracle's Jacobian at the solution x* of the clean problem and N a basis of the
    directions the clean observations do not determine (they carry 1600 times the weight, so they act as constraints), t is a random vector
    projected onto the complement of range(J_planted N), and observation i gets the residual rho_i = alpha_i t_i at x*, alpha_i such that its
    Cauchy-weighted gradient rho' rho_i = rho_i / (1 + |rho_i|^2) is c t_i: the planted part of the gradient is then c (J_planted N)^T t = 0 for
    every step the clean observations allow. c puts the smallest |rho_i| at ERASE_SHIFT (the others are larger, up to a few thousand px).
    x* is a saddle of the robust cost, not a minimum — a deviation roughly doubles per iteration — but the first iteration takes the perturbed
    start to within a pixel of it, and tests/test_structure_host.py holds every pattern to the separation the second round is tested on."""
    from oracle import covo
    if len(rows) == 0:
        return pb.copy()
    sol, _ = covo.gba_solve(pb, covo.default_options(visual_only=1))
    r, Jp, Jl, _ = covo.linearize_reprojection(sol, covo.default_options(visual_only=1, reproj_loss_a=0.0))
    K, L, O = pb.K, pb.L, pb.O
    obs_lm = np.repeat(np.arange(L), np.diff(pb.lm_obs_ptr))
    J = np.zeros((2 * O, 6 * K + 3 * L))
    for o in range(O):
        J[2 * o:2 * o + 2, 6 * pb.obs_kf[o]:6 * pb.obs_kf[o] + 6] = Jp[o].reshape(2, 6)
        J[2 * o:2 * o + 2, 6 * K + 3 * obs_lm[o]:6 * K + 3 * obs_lm[o] + 3] = Jl[o].reshape(2, 3)
    planted = np.zeros(2 * O, bool); planted[2 * rows] = True; planted[2 * rows + 1] = True
    _, sv, vt = np.linalg.svd(J[~planted], full_matrices=True)
    N = vt[int((sv > 1e-8 * sv[0]).sum()):].T
    A = J[planted] @ N
    rng = np.random.default_rng(seed)
    best = None
    for _ in range(8):                                               # (the draw whose smallest |t_i| is largest: the least spread of |rho_i|)
        z = rng.normal(size=A.shape[0])
        t = (z - A @ np.linalg.lstsq(A, z, rcond=None)[0]).reshape(-1, 2)
        tn = np.linalg.norm(t, axis=1)
        if best is None or tn.min() / tn.max() > best[0]:
            best = (tn.min() / tn.max(), t, tn)
    _, t, tn = best
    x = ERASE_SHIFT / (1.0 + ERASE_SHIFT ** 2) * tn / tn.max()
    rho = t / tn[:, None] * ((1.0 + np.sqrt(1.0 - 4.0 * x * x)) / (2.0 * x))[:, None]
    p = pb.copy()
    p.obs_uv[rows] = pb.obs_uv[rows] + (r[rows] - rho) * pb.obs_sigma[rows, None]      # residual = (projection - keypoint) / sigma
    return p


def displaced_across(pb, rows, seed):
    """`pb` with the keypoints of `rows` displaced by exactly ERASE_SHIFT px ACROSS the epipolar line of the landmark's first observation, for a
    problem whose planted landmarks are seen by constant keyframes only and keep their first observation clean.

    'All landmarks destroyed but one' means at most one clean observation per landmark, and a landmark with one clean observation pins no pose:
    free poses that observe such landmarks are held by nothing but outliers, the trust region rejects steps and the clean observations do not
    converge within the round either. With constant poses every landmark is a problem of its own: the clean observation leaves it the depth along
    its ray, along which a displaced observation moves on its epipolar line — a displacement across that line can only grow (a minimum of the
    robust cost, not a saddle), whatever its sign."""
    from oracle import covo
    sol, _ = covo.gba_solve(pb, covo.default_options(visual_only=1))
    _, _, Jl, _ = covo.linearize_reprojection(sol, covo.default_options(visual_only=1, reproj_loss_a=0.0))
    obs_lm = np.repeat(np.arange(pb.L), np.diff(pb.lm_obs_ptr))
    rng = np.random.default_rng(seed)
    p = pb.copy()
    for o in rows:
        l = obs_lm[o]
        k = pb.obs_kf[pb.lm_obs_ptr[l]]
        assert pb.kf_fixed[k] and pb.kf_fixed[pb.obs_kf[o]] and o != pb.lm_obs_ptr[l]
        centre = sol.kf_pose[k, 4:] + Rotation.from_quat(sol.kf_pose[k, :4]).apply(EXTR_T)
        e = Jl[o].reshape(2, 3) @ (sol.lm_pos[l] - centre)
        p.obs_uv[o] += rng.choice([-1.0, 1.0]) * ERASE_SHIFT * np.array([-e[1], e[0]]) / np.linalg.norm(e)
    return p


def erase_problem(name):
    """(problem with the pattern's keypoints displaced, planted rows, expected lm_left [L])."""
    if name not in _erase:
        rows = planted_rows(name)
        p = (displaced_across if name == "all-but-one" else displaced)(erase_base(name), rows, seed=ERASE_PATTERNS.index(name))
        erase = np.zeros(p.O, bool); erase[rows] = True
        obs_lm = np.repeat(np.arange(p.L), np.diff(p.lm_obs_ptr))
        _erase[name] = (p, rows, np.bincount(obs_lm, weights=~erase, minlength=p.L).astype(np.int32))
    return _erase[name]


def compact(p, erase):
    """(the second round's problem in numpy, kept landmarks [L] bool): `p` minus the erased observations, minus the landmarks left with fewer than two
    and their surviving observation."""
    obs_lm = np.repeat(np.arange(p.L), np.diff(p.lm_obs_ptr))
    left = np.bincount(obs_lm, weights=~erase, minlength=p.L).astype(np.int64)
    keep_l = left >= 2
    keep_o = ~erase & keep_l[obs_lm]
    d = {k: (None if v is None else np.array(v, copy=True)) for k, v in p.__dict__.items()}
    d.update(lm_pos=p.lm_pos[keep_l], lm_obs_ptr=np.concatenate([[0], np.cumsum(left[keep_l])]), obs_kf=p.obs_kf[keep_o], obs_uv=p.obs_uv[keep_o],
             obs_sigma=p.obs_sigma[keep_o])
    return capi.FlatProblem(**d), keep_l


# ------------------------------------------------------------------------------------------------ a pose graph with awkward incidence
PG_K, PG_HUB, PG_FIXED, PG_TRIPLE, PG_ISLAND = 260, 130, (0, 77), (40, 200), 259
_pg = {}


def pose_graph_problem():
    """~260 ring keyframes and, in random order: an odometry chain; one hub keyframe tied to every other (an incidence list longer than 256 in
    k_edge_gather_kf); a triple edge between one pair given as (a, b), (b, a), (a, b) with three different non-diagonal sqrt_info; an edge between
    the two constant keyframes; a free keyframe (the last) whose only edges go to the constant ones; edge_loss_a mixed between 0 and 1."""
    if "pg" in _pg:
        return _pg["pg"]
    rng = np.random.default_rng(260)
    K = PG_K
    true = ring_poses(K)
    Rt, pt_ = Rotation.from_quat(true[:, :4]), true[:, 4:]
    a, b = PG_TRIPLE
    edges = [(k, k + 1) for k in range(K - 2)]                       # the chain ends before the last keyframe
    edges += [(PG_HUB, k) if k % 2 else (k, PG_HUB) for k in range(K - 1) if k != PG_HUB and abs(k - PG_HUB) != 1]
    edges += [(a, b), (b, a), (a, b)]
    edges += [(PG_FIXED[0], PG_FIXED[1])]
    edges += [(PG_ISLAND, PG_FIXED[0]), (PG_FIXED[1], PG_ISLAND)]
    edges = [edges[e] for e in rng.permutation(len(edges))]
    ei, ej = np.array(edges, np.int64).T
    E = len(edges)
    Rm = Rt[ei].inv() * Rt[ej] * Rotation.from_rotvec(rng.normal(0, 0.003, (E, 3)))
    qm = Rm.as_quat(); qm[qm[:, 3] < 0] *= -1
    tm = Rt[ei].inv().apply(pt_[ej] - pt_[ei]) + rng.normal(0, 0.01, (E, 3))
    sq = np.tile(np.diag([200.0] * 3 + [100.0] * 3).reshape(1, 36), (E, 1))
    for e in np.nonzero((np.minimum(ei, ej) == a) & (np.maximum(ei, ej) == b))[0]:
        A = rng.normal(0, 1, (6, 6))
        sq[e] = np.linalg.cholesky(A @ A.T * 300.0 + np.eye(6) * 2000.0).T.reshape(-1)
    loss = (rng.uniform(0, 1, E) < 0.5).astype(np.float64)
    pose = true.copy()
    kf_fixed = np.zeros(K, np.uint8); kf_fixed[list(PG_FIXED)] = 1
    free = kf_fixed == 0
    q = (Rt * Rotation.from_rotvec(rng.normal(0, 0.01, (K, 3)))).as_quat(); q[q[:, 3] < 0] *= -1
    pose[free, :4] = q[free]; pose[free, 4:] += rng.normal(0, 0.05, (K, 3))[free]
    qsc = Rotation.from_rotvec(EXTR_ROTVEC).as_quat()
    _pg["pg"] = capi.FlatProblem(kf_pose=pose, kf_speed_bias=np.zeros((K, 9)), kf_fixed=kf_fixed, kf_cam=np.zeros(K, np.int32),
                                cam_extr=np.concatenate([qsc, EXTR_T])[None], cam_intr=synth.INTR[None], cam_dist=synth.DIST[None], cam_dist_type=[0],
                                edge_i=ei, edge_j=ej, edge_meas=np.concatenate([qm, tm], 1), edge_sqrt_info=sq, edge_loss_a=loss)
    return _pg["pg"]


def pose_graph(name):
    """'pose-graph': pose_graph_problem(); 'pose-graph-reversed': its relabel() with half of the edges reversed (another valid problem)."""
    if name == "pose-graph":
        return pose_graph_problem()
    if "pgr" not in _pg:
        _pg["pgr"] = relabel(pose_graph_problem(), seed=9, flip_edges=True)[0]
    return _pg["pgr"]


PG_NAMES = ("pose-graph", "pose-graph-reversed")
