"""Problems with prescribed track lengths for the three widths of the landmark-major kernels (k_visual.hip: k_lm_lin, k_lm_backsub, k_lm_outliers
as G = 4, 8 or 16 lanes per landmark, pinhole and unified), their host references, and ONE table of points shared by the host test
(tests/test_lm_forms_host.py: every point selects the width it is meant for and holds the track lengths and landmark counts the device test relies
on) and the device test (tests/test_gpu_lm_forms.py). No GPU code here.

The width is chosen by the data alone (backend.lm_group = covgpu_lm_group: O/L <= 5 -> 4, <= 8 -> 8, else 16), so a point is a track-length
PATTERN, repeated up to a landmark count L, cut out of a base map with long tracks: the long-track configuration of
tests/test_gpu_edge_cases.py::test_long_tracks_multi_chunk at 20 keyframes per agent (K = 60, 916 landmarks, tracks of 5 .. 49 observations), seen by
pinhole cameras or by the MIXED cameras of tests/test_gpu_omni.py (pinhole, unified + RadTan, unified + Equidistant: the UNI instantiations).
Slot s of a point takes one base landmark and keeps its first lengths[s] observations; the longest requested tracks go to the longest-tracked base
landmarks, and where the base map has fewer tracks of a length than a point asks for (17 landmarks reach 49 observations, 22 reach 48), the slot
keeps what its landmark has. Two keyframes per camera are constant (gauge and scale of a visual-only problem), between factors are dropped.

The largest point of every width carries three degenerate landmarks (Built.special):
  const   both observers are constant keyframes: no pose Jacobian, no Z record; the landmark still has a step and a cost
  behind  one observation (of a track of G + 1) handed to a keyframe that has the landmark behind it: that block is zero while the track's other
          observations stay valid. No keyframe of the base map has any landmark behind it, so the point gets a 61st keyframe for this — the
          observer's camera turned to look straight away from the landmark, with this one observation (its pose block stays unconstrained)
  two     exactly two observations (H_ll is rank 2 up to the damping)
"""
from collections import namedtuple

import numpy as np

from covins_amd import backend, capi, mapdata, synth

Point = namedtuple("Point", "id G L pattern")
Built = namedtuple("Built", "p lengths base_lm special")

PATTERN = {
    4: (2, 3, 4, 5, 3, 4, 2, 8, 3, 4, 9, 2, 3, 4, 13, 2, 3, 4, 17, 2),             # mean 4.75; 17 = 5 chunks of 4
    8: (2, 7, 8, 9, 5, 6, 7, 3, 16, 17, 2, 3, 4, 25, 6, 4, 5, 4),                   # mean 7.39; 25 = 4 chunks of 8
    16: (2, 15, 16, 17, 31, 32, 33, 48, 49, 5, 6, 10, 12, 20),                      # mean 21.1; 49 = 4 chunks of 16
}
# landmarks per workgroup of 256 threads = 256 / G: that count and its neighbours (a last workgroup with one landmark, a full one, one short of full),
# one point of several workgroups, and for G = 4 a single landmark
COUNTS = {4: (1, 63, 64, 65, 449), 8: (31, 32, 33, 450), 16: (15, 16, 17, 451)}
POINTS = {G: [Point(f"g{G}-L{L}", G, L, PATTERN[G]) for L in COUNTS[G]] for G in (4, 8, 16)}
LARGE = {G: POINTS[G][-1] for G in POINTS}
CAMERAS = ("pinhole", "unified")
ALL = [(pt, cam) for G in (4, 8, 16) for cam in CAMERAS for pt in POINTS[G]]
IDS = [f"{pt.id}-{cam}" for pt, cam in ALL]
MU_STEP = 1e-4
MUS_SCHUR = (1e-8, 1e-2)


def required_lengths(G):
    return (2, G - 1, G, G + 1, 2 * G, 2 * G + 1)


def point_lengths(pt):
    return np.resize(np.asarray(pt.pattern, np.int64), pt.L)


# ------------------------------------------------------------------------------------------------ the builder
_base, _built, _ref = {}, {}, {}


def base_config(unified=False, **kw):
    from tests.test_gpu_omni import MIXED
    cfg = synth.config_named("small"); cfg.p_fuse = 0.5; cfg.max_fused_obs = 70; cfg.track_window = 12
    cfg.max_obs_per_kf = 3000; cfg.new_lm_per_kf = 16; cfg.max_kf_per_agent = 20
    if unified:
        cfg.cameras = MIXED
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def base_problem(unified=False):
    """The flattened base map (with its IMU factors: a visual-only call ignores them), reprojection blocks only, two constant keyframes per camera."""
    from tests.test_gpu_omni import reprojection_only
    if unified not in _base:
        p = reprojection_only(mapdata.flatten_gba(synth.make_map(base_config(unified)), False, True)[0])
        for a in range(p.A):
            p.kf_fixed[np.nonzero(p.kf_cam == a)[0][:2]] = 1
        _base[unified] = p
    return _base[unified]


def assign_tracks(n_base, lengths):
    """(base landmark per slot, length per slot): the longest requested tracks take the longest-tracked base landmarks (both orders stable), a slot
    keeps at most what its landmark has."""
    lengths = np.asarray(lengths, np.int64)
    assert len(lengths) <= len(n_base)
    order = np.argsort(-np.asarray(n_base), kind="stable")
    slots = np.argsort(-lengths, kind="stable")
    lm = np.empty(len(lengths), np.int64)
    lm[slots] = order[:len(lengths)]
    return lm, np.minimum(lengths, np.asarray(n_base)[lm])


def cut_tracks(p, base_lm, lengths):
    """`p` with landmark s = base landmark base_lm[s] cut to its first lengths[s] observations (0: the landmark is dropped); lm_pos, lm_obs_ptr,
    obs_kf, obs_uv and obs_sigma rebuilt, everything else kept."""
    base_lm, lengths = np.asarray(base_lm, np.int64), np.asarray(lengths, np.int64)
    assert np.all(lengths <= np.diff(p.lm_obs_ptr)[base_lm]) and len(set(base_lm.tolist())) == len(base_lm)
    keep = lengths > 0
    base_lm, lengths = base_lm[keep], lengths[keep]
    rows = np.concatenate([p.lm_obs_ptr[l] + np.arange(n) for l, n in zip(base_lm, lengths)]) if len(base_lm) else np.zeros(0, np.int64)
    d = dict(p.__dict__)
    d.update(lm_pos=p.lm_pos[base_lm], lm_obs_ptr=np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32), obs_kf=p.obs_kf[rows],
             obs_uv=p.obs_uv[rows], obs_sigma=p.obs_sigma[rows])
    return capi.FlatProblem(**{k: (None if v is None else np.array(v, copy=True)) for k, v in d.items()})


def camera_frame_valid(p, k, x):
    """Does keyframe k's camera project the world point x (tests/test_omni_host.project_ref: in front of the pinhole camera, inside the unified
    model's validity boundary)?"""
    from tests.test_omni_host import project_ref, quat_R
    c = p.kf_cam[k]
    ls = quat_R(p.kf_pose[k, :4]).T @ (x - p.kf_pose[k, 4:])
    lc = quat_R(p.cam_extr[c, :4]).T @ (ls - p.cam_extr[c, 4:])
    model = p.cam_model[c] if p.cam_model is not None else 0
    xi = p.cam_xi[c] if p.cam_xi is not None else 0.0
    return bool(project_ref(lc, model, xi, p.cam_intr[c], p.cam_dist[c], p.cam_dist_type[c])[0])


def with_keyframe_looking_away(p, k, x):
    """`p` with one more keyframe (free, no IMU factor, no observation yet): keyframe k's camera at the same place, its optical axis pointing
    straight away from the world point x — behind the image plane of a pinhole camera and outside the validity cone of every unified one."""
    from scipy.spatial.transform import Rotation
    from tests.test_omni_host import quat_R
    c = p.kf_cam[k]
    Rws, Rsc, psc = quat_R(p.kf_pose[k, :4]), quat_R(p.cam_extr[c, :4]), p.cam_extr[c, 4:]
    pwc = p.kf_pose[k, 4:] + Rws @ psc
    z = -(x - pwc) / np.linalg.norm(x - pwc)
    a = np.eye(3)[np.argmin(np.abs(z))]
    xa = np.cross(a, z); xa /= np.linalg.norm(xa)
    Rwc = np.stack([xa, np.cross(z, xa), z], axis=1)
    Rn = Rwc @ Rsc.T
    q = Rotation.from_matrix(Rn).as_quat()
    q = -q if q[3] < 0 else q
    d = dict(p.__dict__)
    d.update(kf_pose=np.vstack([p.kf_pose, np.concatenate([q, pwc - Rn @ psc])]), kf_speed_bias=np.vstack([p.kf_speed_bias, p.kf_speed_bias[k]]),
             kf_fixed=np.append(p.kf_fixed, 0), kf_cam=np.append(p.kf_cam, c))
    return capi.FlatProblem(**{n: (None if v is None else np.array(v, copy=True)) for n, v in d.items()})


def build(pt, cam):
    """The point's problem on the pinhole or the unified base (cached; treat as read-only)."""
    key = (pt.id, cam)
    if key in _built:
        return _built[key]
    base = base_problem(cam == "unified")
    n_base = np.diff(base.lm_obs_ptr)
    lm, lengths = assign_tracks(n_base, point_lengths(pt))
    special = {}
    if pt is LARGE[pt.G]:
        two = np.nonzero(lengths == 2)[0]
        first2 = base.kf_fixed[base.obs_kf[base.lm_obs_ptr[:-1]]].astype(bool) & base.kf_fixed[base.obs_kf[base.lm_obs_ptr[:-1] + 1]].astype(bool)
        special["two"] = int(two[~first2[lm[two]]][0])      # (a free keyframe among its two observers)
        # const: a base landmark no slot uses whose first two observers are constant keyframes, into the last slot of length 2
        free = np.setdiff1d(np.nonzero(first2)[0], lm)
        assert len(free) > 0 and two[-1] != special["two"]
        lm[two[-1]] = free[0]
        special["const"] = int(two[-1])
        special["behind"] = int(np.nonzero(lengths == pt.G + 1)[0][0])
    p = cut_tracks(base, lm, lengths)
    if "behind" in special:
        s = special["behind"]
        o0, o1 = p.lm_obs_ptr[s], p.lm_obs_ptr[s + 1]
        assert all(camera_frame_valid(p, k, p.lm_pos[s]) for k in p.obs_kf[o0:o1])
        p = with_keyframe_looking_away(p, int(p.obs_kf[o0 + 1]), p.lm_pos[s])
        assert not camera_frame_valid(p, p.K - 1, p.lm_pos[s])
        p.obs_kf[o0 + 1] = p.K - 1
        srt = o0 + np.argsort(p.obs_kf[o0:o1], kind="stable")      # (tracks stay sorted by keyframe, as the flattening hands them over)
        p.obs_kf[o0:o1], p.obs_uv[o0:o1], p.obs_sigma[o0:o1] = p.obs_kf[srt], p.obs_uv[srt], p.obs_sigma[srt]
        special["behind_obs"] = int(o1 - 1)
        assert p.obs_kf[o1 - 1] == p.K - 1
    p.validate()
    _built[key] = Built(p, lengths, lm, special)
    return _built[key]


def map_with_cut_tracks(pt, **cfg_kw):
    """The pinhole base MAP (not flattened) with the same tracks cut by Map.erase_observations: map landmark base_lm[s] keeps its first lengths[s]
    observations, every other landmark loses all of them (flatten_gba drops it)."""
    m = synth.make_map(base_config(False, **cfg_kw))
    n = np.diff(m.lm_obs_ptr)
    lm, lengths = assign_tracks(n, point_lengths(pt))
    keep_n = np.zeros(m.L, np.int64); keep_n[lm] = lengths
    rank = np.arange(m.O) - np.repeat(m.lm_obs_ptr[:-1], n)
    m.erase_observations(rank >= np.repeat(keep_n, n))
    return m, keep_n


# ------------------------------------------------------------------------------------------------ host references
def scaled_err(x, x0, d):
    """max |(x - x0) d| / max |x0 d| (tests/forms_util.scaled_err); a reference that is zero throughout (no free keyframe observes anything) asks
    for exact zeros."""
    den = float(np.abs(x0 * d).max())
    if den == 0.0:
        return 0.0 if not np.any(x) else np.inf
    return float(np.abs((x - x0) * d).max() / den)


def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _clampd(h):
    return np.clip(np.sqrt(np.maximum(h, 0.0)), 1e-6, 1e32)


class NumpySystem:
    """The normal equations of a visual-only problem from tests/test_omni_host.linearize_ref (the only host statement of the unified model), with
    the damping of the solvers (Ceres: mu clamp(sqrt(diag J^T J), 1e-6, 1e32)^2; a pose dimension nobody constrains gets a unit diagonal and
    no step): the Schur complement, the Schur-then-back-substitute step and the dense step of the whole system."""

    def __init__(self, p):
        from tests.test_omni_host import linearize_ref
        r, Jp, Jl, cost = linearize_ref(p, loss_a=1.0)
        K, L, O = p.K, p.L, p.O
        self.K, self.L = K, L
        lm_of = np.repeat(np.arange(L), np.diff(p.lm_obs_ptr))
        Jp, Jl = Jp.reshape(O, 2, 6), Jl.reshape(O, 2, 3)
        self.cost = float(cost.sum())
        Hpp = np.zeros((6 * K, 6 * K)); gp = np.zeros(6 * K)
        Hpl = np.zeros((6 * K, 3 * L)); Hll = np.zeros((L, 3, 3)); gl = np.zeros((L, 3))
        for o in range(O):
            k, l = p.obs_kf[o], lm_of[o]
            Hpp[6 * k:6 * k + 6, 6 * k:6 * k + 6] += Jp[o].T @ Jp[o]
            Hpl[6 * k:6 * k + 6, 3 * l:3 * l + 3] += Jp[o].T @ Jl[o]
            gp[6 * k:6 * k + 6] += Jp[o].T @ r[o]
            Hll[l] += Jl[o].T @ Jl[o]; gl[l] += Jl[o].T @ r[o]
        self.Hpp, self.Hpl, self.Hll, self.gp, self.gl = Hpp, Hpl, Hll, gp, gl

    def _damped(self, mu):
        dp2 = np.diag(self.Hpp).copy()
        live = dp2 != 0.0
        App = self.Hpp.copy()
        idx = np.arange(6 * self.K)
        App[idx[live], idx[live]] += mu * _clampd(dp2[live]) ** 2
        App[idx[~live], idx[~live]] = 1.0
        All = self.Hll.copy()
        for q in range(3):
            All[:, q, q] += mu * _clampd(self.Hll[:, q, q]) ** 2
        return App, All, live

    def schur(self, mu):
        App, All, _ = self._damped(mu)
        Hi = np.linalg.inv(All)
        Y = np.einsum("ilq,lqr->ilr", self.Hpl.reshape(-1, self.L, 3), Hi).reshape(6 * self.K, 3 * self.L)
        S = App - Y @ self.Hpl.T
        b = -self.gp + Y @ self.gl.reshape(-1)
        return S, b, self.cost

    def schur_step(self, mu):
        _, All, _ = self._damped(mu)
        S, b, _ = self.schur(mu)
        dp = np.linalg.solve(S, b)
        dl = np.linalg.solve(All, (-self.gl - (self.Hpl.T @ dp).reshape(-1, 3))[:, :, None])[:, :, 0]
        return dp, dl

    def dense_step(self, mu):
        App, All, live = self._damped(mu)
        n, m = 6 * self.K, 3 * self.L
        H = np.zeros((n + m, n + m))
        H[:n, :n] = App; H[:n, n:] = self.Hpl; H[n:, :n] = self.Hpl.T
        for l in range(self.L):
            H[n + 3 * l:n + 3 * l + 3, n + 3 * l:n + 3 * l + 3] = All[l]
        g = np.concatenate([self.gp, self.gl.reshape(-1)])
        keep = np.concatenate([live, np.ones(m, bool)])
        x = np.zeros(n + m)
        x[keep] = np.linalg.solve(H[np.ix_(keep, keep)], -g[keep])
        return x[:n], x[n:].reshape(-1, 3)


def host_reference(pt, cam):
    """Per point, computed once and shared by the host and the device test (read-only): the reference Schur complements {mu: (S, b, cost)}, the
    dense reference step (x0, l0) at MU_STEP with d = sqrt(diag S), and the spread of the two host solvers of that step in the metrics the device
    is held to: h_pose = scaled_err(Schur step, dense step), h_lm = rel(...). Pinhole: the oracle (covo.schur, covo.step dense / Schur); unified:
    NumpySystem."""
    key = (pt.id, cam)
    if key in _ref:
        return _ref[key]
    p = build(pt, cam).p
    if cam == "pinhole":
        from oracle import covo
        o = covo.default_options(visual_only=1)
        schur = {mu: covo.schur(p, o, mu) for mu in MUS_SCHUR + (MU_STEP,)}
        steps = {mu: (covo.step(p, o, mu, dense=True), covo.step(p, o, mu, dense=False)) for mu in (MU_STEP, 1e-8)}
    else:
        ns = NumpySystem(p)
        schur = {mu: ns.schur(mu) for mu in MUS_SCHUR + (MU_STEP,)}
        steps = {mu: (ns.dense_step(mu), ns.schur_step(mu)) for mu in (MU_STEP, 1e-8)}
    spread = {}
    for mu, ((xd, ld), (xs, ls)) in steps.items():
        S = schur[mu][0] if mu in schur else (covo.schur(p, o, mu)[0] if cam == "pinhole" else ns.schur(mu)[0])
        d = np.sqrt(np.abs(np.diag(S)))
        spread[mu] = (scaled_err(xs, xd, d), rel(ls, ld), d)
    (x0, l0), _ = steps[MU_STEP]
    _ref[key] = dict(schur=schur, x0=x0, l0=l0, d=spread[MU_STEP][2], h_pose=spread[MU_STEP][0], h_lm=spread[MU_STEP][1],
                     spread={mu: v[:2] for mu, v in spread.items()}, steps=steps)
    return _ref[key]


# ------------------------------------------------------------------------------------------------ the outlier rule
OUTLIER_PX = 20.0
OUTLIER_THRESHOLD = 0.92


def outlier_problem(pt, cam):
    """(problem, {what: observation rows}) — the point's problem with keypoints displaced by OUTLIER_PX in a seeded random direction each:
      all       every observation of one landmark (the shortest track above 2: 3 observations, 5 in the 16-lane pattern; the single landmark at L = 1)
      all_but_1 all but the last observation of a track of G - 1
      last_lane index G - 1 of a track of G: the last lane of a full chunk
      chunk_2   index G of a track of 2 G + 1: the first observation of the second chunk
    on four different landmarks, none of them one of the degenerate ones."""
    b = build(pt, cam)
    p, G = b.p.copy(), pt.G
    taken = {v for k, v in b.special.items() if k != "behind_obs"}

    def slot(n):
        s = [int(i) for i in np.nonzero(b.lengths == n)[0] if int(i) not in taken]
        assert s, (pt.id, n)
        taken.add(s[0])
        return s[0], int(p.lm_obs_ptr[s[0]])

    rows = {}
    if p.L == 1:
        rows["all"] = np.arange(p.O)
    else:
        n_all = int(b.lengths[b.lengths > 2].min())
        s, o0 = slot(n_all); rows["all"] = o0 + np.arange(n_all)
        s, o0 = slot(G - 1); rows["all_but_1"] = o0 + np.arange(G - 2)
        s, o0 = slot(G); rows["last_lane"] = np.array([o0 + G - 1])
        s, o0 = slot(2 * G + 1); rows["chunk_2"] = np.array([o0 + G])
    rng = np.random.default_rng(1000 * G + pt.L)
    for r in rows.values():
        a = rng.uniform(0, 2 * np.pi, len(r))
        p.obs_uv[r] += OUTLIER_PX * np.stack([np.cos(a), np.sin(a)], 1)
    return p, rows
