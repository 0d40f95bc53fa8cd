"""Keyframes, points and jobs for covgpu_search_se3_batch / covgpu_search_projection_batch, and the comparison of a
library result with the restatement (tests/guided_ref.py). Kept apart from covins_amd/synth.py so the golden input digests of the
synthetic maps do not move.

map_keyframes(): one keyframe dict (guided_ref's layout) per keyframe of a synthetic map: its observations as float32 keypoints plus
50-300 distractor keypoints at random pixels, shuffled; every landmark a random 256-bit descriptor, an observation row that descriptor
with bits flipped; max_distance = (distance to the reference keyframe) * scale_factor^(reference level), min_distance =
max_distance / scale_factor^(num_octaves - 1), the normal from the reference camera to the landmark; keypoint levels predicted from the
geometry with a jitter of one level; about 40 % of the landmark rows marked already matched. Keyframes alternate between grid order
and index order. Configuration "ref" is the reference's (scale_factor 2.0, num_octaves 1), "pyr" is (1.2, 8) with levels over 0..7.
adversarial_se3() / adversarial_projection(): hand-built cases on exactly representable coordinates (no fragile point)."""
from __future__ import annotations

import functools

import numpy as np
from scipy.spatial.transform import Rotation as Rot

from covins_amd import synth
from tests import guided_ref as gr
from tests.abspose_util import pose_matrix
from tests.match_util import at_dist, flip

CONFIGS = {"ref": dict(scale_factor=2.0, num_octaves=1), "pyr": dict(scale_factor=1.2, num_octaves=8)}
BOUNDS = (0.0, float(synth.WIDTH), 0.0, float(synth.HEIGHT))
GRID_INV = (64.0 / synth.WIDTH, 48.0 / synth.HEIGHT)


@functools.lru_cache(maxsize=None)
def small_map():
    return synth.make_map(synth.config_named("small"))


def _level(dist, maxd, sf, no):
    return gr.predict_scale(dist, maxd, sf, no)[0]


@functools.lru_cache(maxsize=None)
def map_keyframes(config="ref", seed=0):
    """(keyframes, extras): per keyframe of the small map a guided_ref keyframe dict (with lm [n] the landmark of every row, -1 for a
    distractor, and T_cw 4x4); extras = dict(lm_desc, lm_maxd, lm_mind, lm_normal, kf_lms)."""
    m = small_map()
    sf, no = CONFIGS[config]["scale_factor"], CONFIGS[config]["num_octaves"]
    rng = np.random.default_rng(seed)
    lm_desc = rng.integers(0, 256, (m.L, 32), dtype=np.uint8)
    Twc = [pose_matrix(m.kf_pose[k]) @ pose_matrix(m.cam_extr[int(m.kf_cam[k])]) for k in range(m.K)]
    Tcw = [np.linalg.inv(T) for T in Twc]
    ref = np.clip(m.lm_ref_kf, 0, m.K - 1)
    PO = m.lm_pos - np.array([Twc[k][:3, 3] for k in ref])
    dref = np.linalg.norm(PO, axis=1)
    lm_maxd = dref * sf ** rng.integers(0, no, m.L)
    lm_mind = lm_maxd / sf ** (no - 1)
    lm_normal = PO / dref[:, None]
    kf_lms = [[] for _ in range(m.K)]; kf_obs = [[] for _ in range(m.K)]
    for l in range(m.L):
        for o in range(m.lm_obs_ptr[l], m.lm_obs_ptr[l + 1]):
            kf_lms[m.obs_kf[o]].append(l); kf_obs[m.obs_kf[o]].append(o)
    kfs = []
    for k in range(m.K):
        lms = np.array(kf_lms[k], np.int64); obs = np.array(kf_obs[k], np.int64)
        nd = int(rng.integers(50, 301))
        a = int(m.kf_cam[k])
        kp = np.concatenate([m.obs_uv[obs].reshape(-1, 2), rng.uniform((0, 0), (synth.WIDTH, synth.HEIGHT), (nd, 2))]).astype(np.float32)
        desc = np.concatenate([flip(lm_desc[lms], rng.uniform(0.02, 0.12), rng) if len(lms) else np.zeros((0, 32), np.uint8),
                               rng.integers(0, 256, (nd, 32), dtype=np.uint8)])
        lm = np.concatenate([lms, np.full(nd, -1, np.int64)])
        pc = (Tcw[k][:3, :3] @ m.lm_pos[lms].T).T + Tcw[k][:3, 3] if len(lms) else np.zeros((0, 3))
        dist = np.linalg.norm(pc, axis=1)
        level = np.array([_level(dist[i], lm_maxd[lms[i]], sf, no) for i in range(len(lms))], np.int64)
        level = np.clip(level + rng.integers(-1, 2, len(lms)), 0, no - 1) if no > 1 else level
        level = np.concatenate([level, rng.integers(0, no, nd)]).astype(np.int32)
        perm = rng.permutation(len(kp))
        kp, desc, lm, level = kp[perm], desc[perm], lm[perm], level[perm]
        has = lm >= 0
        lm_pos = np.zeros((len(kp), 3)); lm_pos[has] = (Tcw[k][:3, :3] @ m.lm_pos[lm[has]].T).T + Tcw[k][:3, 3]
        free = has & ~m.lm_invalid[np.maximum(lm, 0)].astype(bool) & (rng.random(len(kp)) >= 0.4)
        kfs.append(dict(kp=kp, level=level, desc=desc, bounds=BOUNDS, grid_inv=GRID_INV if k % 2 == 0 else None,
                        K=m.cam_intr[a].copy(), cam=np.concatenate([m.cam_intr[a], m.cam_dist[a]]), dist_type=int(m.cam_dist_type[a]),
                        cam_model=0, xi=0.0, lm_pos=lm_pos, lm_max_distance=np.where(has, lm_maxd[np.maximum(lm, 0)], 1.0),
                        lm_desc=np.where(has[:, None], lm_desc[np.maximum(lm, 0)], 0).astype(np.uint8), lm_free=free.astype(np.uint8),
                        lm=lm, T_cw=Tcw[k]))
    return kfs, dict(lm_desc=lm_desc, lm_maxd=lm_maxd, lm_mind=lm_mind, lm_normal=lm_normal, kf_lms=[set(s) for s in kf_lms])


def _perturb(T, rng, deg=2.0, trans=0.05):
    """T (4x4) times a random motion of up to `deg` degrees and `trans` metres, as [qx qy qz qw x y z]."""
    ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
    d = np.eye(4)
    d[:3, :3] = Rot.from_rotvec(ax * np.deg2rad(rng.uniform(0, deg))).as_matrix()
    tv = rng.normal(size=3); d[:3, 3] = tv / np.linalg.norm(tv) * rng.uniform(0, trans)
    T = T @ d
    q = Rot.from_matrix(T[:3, :3]).as_quat()
    return np.concatenate([q / np.linalg.norm(q), T[:3, 3]])


@functools.lru_cache(maxsize=None)
def map_se3_case(config="ref", num=64, seed=0):
    """`num` (query, candidate, T12) jobs over the keyframes of the small map: a candidate that shares at least 20 landmarks with the
    query, T12 the true relative camera pose perturbed by up to 2 degrees and 5 cm. A case = dict(kfs, jobs, opts)."""
    kfs, ex = map_keyframes(config, seed)
    rng = np.random.default_rng(seed + 1)
    K = len(kfs)
    jobs = []
    for _ in range(num):
        q = int(rng.integers(K))
        near = [c for c in range(max(0, q - 8), min(K, q + 9)) if c != q and len(ex["kf_lms"][q] & ex["kf_lms"][c]) >= 20]
        c = int(rng.choice(near)) if near else int((q + 1 + rng.integers(K - 1)) % K)
        jobs.append((q, c, _perturb(kfs[q]["T_cw"] @ np.linalg.inv(kfs[c]["T_cw"]), rng)))
    return dict(kfs=kfs, jobs=jobs, opts=dict(CONFIGS[config]))


@functools.lru_cache(maxsize=None)
def map_projection_case(config="ref", num=16, seed=0):
    """`num` SearchByProjection jobs: a keyframe with about half of its observations' landmark associations dropped (those keypoints
    are what the search should find), 30 % of the remaining landmark rows taken; the points are the landmarks of the keyframe and its
    +-3 neighbours. A case = dict(kfs (one per job), jobs [(kf, T_cw [7], points)], opts)."""
    m = small_map()
    kfs, ex = map_keyframes(config, seed)
    rng = np.random.default_rng(seed + 2)
    out_kfs, jobs = [], []
    for j in range(num):
        c = int(rng.integers(3, len(kfs) - 3))
        kf = dict(kfs[c])
        lm = kf["lm"].copy()
        lm[(lm >= 0) & (rng.random(len(lm)) < 0.5)] = -1                       # observed keypoints whose landmark is not associated
        taken = (lm >= 0) & (rng.random(len(lm)) < 0.3)
        kf["taken"] = taken.astype(np.uint8); kf["lm_assoc"] = lm; kf["index"] = c
        row_of = {int(l): r for r, l in enumerate(lm) if l >= 0}
        ids = np.array(sorted(set().union(*[ex["kf_lms"][k] for k in range(c - 3, c + 4)])), np.int64)
        ids = ids[rng.permutation(len(ids))]
        existing = np.array([row_of.get(int(l), -1) for l in ids], np.int32)
        found = np.array([e >= 0 and taken[e] for e in existing])
        skip = m.lm_invalid[ids].astype(bool) | found | (rng.random(len(ids)) < 0.05)
        pts = dict(p_w=m.lm_pos[ids].copy(), normal=ex["lm_normal"][ids], min_distance=ex["lm_mind"][ids], max_distance=ex["lm_maxd"][ids],
                   desc=ex["lm_desc"][ids], skip=skip.astype(np.uint8), existing_idx=existing, lm=ids)
        out_kfs.append(kf)
        jobs.append((j, _perturb(kf["T_cw"], rng, 0.3, 0.01), pts))
    return dict(kfs=out_kfs, jobs=jobs, opts=dict(CONFIGS[config]))


# ---------------------------------------------------------------- hand-built cases

def _kf(kp, level=None, desc=None, bounds=(0.0, 640.0, 0.0, 480.0), grid=False, lm_pos=None, lm_desc=None, lm_free=None, lm_maxd=None,
        taken=None):
    """A keyframe with K = cam = identity pinhole (u = x / z), so that a landmark at (u, v, 1) projects to exactly (u, v)."""
    kp = np.asarray(kp, np.float32).reshape(-1, 2)
    n = len(kp)
    z = lambda a, d: np.asarray(d if a is None else a)
    w = float(bounds[1]), float(bounds[3])
    return dict(kp=kp, level=z(level, np.zeros(n)).astype(np.int32), desc=np.asarray(desc, np.uint8).reshape(n, 32), bounds=tuple(bounds),
                grid_inv=(64.0 / w[0], 48.0 / w[1]) if grid else None, K=np.array([1.0, 1.0, 0.0, 0.0]),
                cam=np.array([1.0, 1.0, 0, 0, 0, 0, 0, 0]), dist_type=0, cam_model=0, xi=0.0,
                lm_pos=z(lm_pos, np.zeros((n, 3))).astype(np.float64).reshape(n, 3), lm_max_distance=z(lm_maxd, np.ones(n)).astype(np.float64),
                lm_desc=z(lm_desc, np.zeros((n, 32))).astype(np.uint8).reshape(n, 32), lm_free=z(lm_free, np.zeros(n)).astype(np.uint8),
                taken=z(taken, np.zeros(n)).astype(np.uint8))


def _at(uv):
    """Camera-frame points (u, v, 1)."""
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    return np.concatenate([uv, np.ones((len(uv), 1))], 1)


IDENT = np.array([0.0, 0, 0, 1, 0, 0, 0])


def adversarial_se3(grid, seed=0):
    """List of cases (dict(name, kfs, jobs, opts)); `grid` selects the visiting order of every keyframe."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, 32, dtype=np.uint8)
    rep = lambda n: np.repeat(x[None], n, 0)
    d_at = lambda d: at_dist(x, d, rng)[0]
    far = lambda n: np.stack([d_at(120) for _ in range(n)])
    cases = []
    # ties: three keypoints at distance 10 from the landmark's descriptor inside one radius; index order takes row 0, grid order row 2
    # (its cell_x is 9, the others' 10). The same layout in the other direction.
    kp = [(103, 104), (97, 96), (94, 100), (300, 300)]
    dk = np.stack([d_at(10), d_at(10), d_at(10), x])
    k1 = _kf(kp, desc=dk, grid=grid, lm_pos=_at([(100, 100), (300, 300), (0, 0), (0, 0)]), lm_desc=rep(4), lm_free=[1, 1, 0, 0])
    k2 = _kf(kp, desc=dk, grid=grid, lm_pos=_at([(100, 100), (300, 300), (0, 0), (0, 0)]), lm_desc=rep(4), lm_free=[1, 1, 0, 0])
    cases.append(dict(name="ties", kfs=[k1, k2], jobs=[(0, 1, IDENT)], opts={}))
    # thresholds: best distance 49, 50, 51 in both directions: 1->2 accepts <= 50, 2->1 accepts < 50
    pos = [(100, 100), (200, 100), (300, 100)]
    k1 = _kf(pos, desc=rep(3), grid=grid, lm_pos=_at(pos), lm_desc=np.stack([d_at(d) for d in (49, 50, 51)]), lm_free=[1, 1, 1])
    k2 = _kf(pos, desc=rep(3), grid=grid, lm_pos=_at(pos), lm_desc=np.stack([d_at(d) for d in (49, 50, 51)]), lm_free=[1, 1, 1])
    cases.append(dict(name="thresholds", kfs=[k1, k2], jobs=[(0, 1, IDENT)], opts={}))
    # agreement: row 0 passes the literal test (match2[0] == 0) but not the intended one (match2[match1[0]] != 0); row 1 the reverse
    p1 = [(50, 50), (150, 50), (250, 50)]; p2 = [(50, 150), (150, 150), (250, 150)]
    k1 = _kf(p1, desc=rep(3), grid=grid, lm_pos=_at([p2[1], p2[2], (0, 0)]), lm_desc=rep(3), lm_free=[1, 1, 0])
    k2 = _kf(p2, desc=rep(3), grid=grid, lm_pos=_at([p1[0], (0, 0), p1[1]]), lm_desc=rep(3), lm_free=[1, 0, 1])
    cases.append(dict(name="agreement", kfs=[k1, k2], jobs=[(0, 1, IDENT)], opts={}))
    # n1 > n2: query rows 3 and 4 find a candidate row, but i >= n2 never agrees literally; row 3 agrees under agreement = 1
    p1 = [(50, 50), (150, 50), (250, 50), (350, 50), (450, 50)]
    k1 = _kf(p1, desc=rep(5), grid=grid, lm_pos=_at([p2[0], (0, 0), (0, 0), p2[0], p2[2]]), lm_desc=rep(5), lm_free=[1, 0, 0, 1, 1])
    k2 = _kf(p2, desc=rep(3), grid=grid, lm_pos=_at([p1[3], p1[1], p1[4]]), lm_desc=rep(3), lm_free=[1, 1, 1])
    cases.append(dict(name="n1>n2", kfs=[k1, k2], jobs=[(0, 1, IDENT), (1, 0, IDENT)], opts={}))
    # depth and image bounds: z < 0 (the pixel would be fine), and projections 0.5 px inside / outside each bound of keyframe 2; the
    # second direction tests keyframe 2's bounds although it projects into keyframe 1 (whose own bounds are smaller)
    edge = [(-0.5, 100), (0.5, 130), (639.5, 160), (640.5, 190), (100, -0.5), (130, 0.5), (160, 479.5), (190, 480.5), (250, 250), (400, 300)]
    n = len(edge)
    lp = _at(edge); lp[8] = (-250.0, -250.0, -1.0)
    k1 = _kf(edge, desc=rep(n), grid=grid, bounds=(0.0, 320.0, 0.0, 240.0), lm_pos=lp, lm_desc=rep(n), lm_free=np.ones(n))
    k2 = _kf(edge, desc=rep(n), grid=grid, lm_pos=lp, lm_desc=rep(n), lm_free=np.ones(n))
    cases.append(dict(name="depth+bounds", kfs=[k1, k2], jobs=[(0, 1, IDENT), (1, 0, IDENT)], opts={}))
    # level window: predicted level 3 (log2(max_distance / dist) = 2.5), keypoints at levels 1..4 and one at 7; radius 9.5 * 2^3 = 76
    pos = [(100, 500), (300, 500), (500, 500), (700, 500), (900, 500)]
    kpos = [(u + 30, v + 40) for u, v in pos]
    lp = _at(pos)
    maxd = np.array([float(np.float32(np.linalg.norm(p))) * 2.0 ** 2.5 for p in lp])
    b = (0.0, 1000.0, 0.0, 1000.0)
    k1 = _kf(kpos, level=[1, 2, 3, 4, 7], desc=rep(5), grid=grid, bounds=b, lm_pos=lp, lm_desc=rep(5), lm_free=np.ones(5), lm_maxd=maxd)
    k2 = _kf(kpos, level=[1, 2, 3, 4, 7], desc=rep(5), grid=grid, bounds=b, lm_pos=lp, lm_desc=rep(5), lm_free=np.ones(5), lm_maxd=maxd)
    cases.append(dict(name="levels", kfs=[k1, k2], jobs=[(0, 1, IDENT)], opts=dict(scale_factor=2.0, num_octaves=8)))
    # a larger random-but-exact set: integer pixels, many keypoints per radius, descriptors in a few clusters (ties abound)
    kp = rng.integers(20, 300, (200, 2)).astype(np.float64)
    cl = np.stack([d_at(int(d)) for d in rng.integers(0, 60, 8)])
    mk = lambda: _kf(kp, desc=cl[rng.integers(0, 8, 200)], grid=grid, lm_pos=_at(kp[rng.permutation(200)] + rng.integers(-3, 4, (200, 2))),
                     lm_desc=cl[rng.integers(0, 8, 200)], lm_free=rng.random(200) < 0.7)
    cases.append(dict(name="dense", kfs=[mk(), mk()], jobs=[(0, 1, IDENT), (1, 0, IDENT), (0, 0, IDENT)], opts={}))
    return cases


def _pts(uv, desc, **kw):
    """Points at (u, v, 1) seen from the origin: inside every distance bound and facing the camera unless overridden."""
    p = _at(uv)
    n = len(p)
    d = dict(p_w=p, normal=p / np.linalg.norm(p, axis=1, keepdims=True), min_distance=np.full(n, 1e-3), max_distance=np.full(n, 1e6),
             desc=np.asarray(desc, np.uint8).reshape(n, 32), skip=np.zeros(n, np.uint8), existing_idx=np.full(n, -1, np.int32))
    for k, v in kw.items():
        d[k] = np.asarray(v, d[k].dtype).reshape(d[k].shape)
    return d


def adversarial_projection(grid, seed=0):
    """List of cases (dict(name, kfs, jobs [(kf, T_cw, points)], opts))."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, 32, dtype=np.uint8)
    rep = lambda n: np.repeat(x[None], n, 0)
    d_at = lambda d, base=x: at_dist(base, d, rng)[0]
    cases = []
    # 40 points onto one cluster of 12 keypoints, all within th_low: long claim chains, used-up lists, and with capacity 8 the rescan
    kp = [(197 + 2 * i, 198 + 2 * j) for i in range(4) for j in range(3)]
    kf = _kf(kp, desc=np.stack([d_at(j) for j in range(12)]), grid=grid)
    uv = [(200 + (p % 2), 200 + (p // 2) % 2) for p in range(40)]
    pts = _pts(uv, np.stack([d_at(int(d)) for d in rng.integers(0, 20, 40)]))
    cases.append(dict(name="cluster", kfs=[kf], jobs=[(0, IDENT, pts)], opts={}))
    # the same with three of the keypoints taken and every third point skipped
    kf2 = _kf(kp, desc=kf["desc"], grid=grid, taken=[1 if j in (0, 5, 7) else 0 for j in range(12)])
    pts2 = dict(pts); pts2["skip"] = (np.arange(40) % 3 == 1).astype(np.uint8)
    cases.append(dict(name="cluster+taken+skip", kfs=[kf2], jobs=[(0, IDENT, pts2)], opts={}))
    # existing_idx on each side of dist_old < bestDist: the best keypoint (row 0 / 2 / 4, distance 10) against the existing one
    # (far away, distance 9, 10, 11); a fourth point whose best is over th_low proposes nothing
    kp = [(100, 100), (500, 100), (100, 200), (500, 200), (100, 300), (500, 300), (100, 400), (500, 400)]
    descs = np.stack([d_at(10), d_at(9), d_at(10), d_at(10), d_at(10), d_at(11), d_at(51), d_at(3)])
    kf = _kf(kp, desc=descs, grid=grid)
    pts = _pts([(103, 104), (103, 204), (103, 304), (103, 404)], rep(4), existing_idx=[1, 3, 5, 7])
    cases.append(dict(name="existing", kfs=[kf], jobs=[(0, IDENT, pts)], opts={}))
    # ties inside one radius (index order row 0, grid order row 2), a taken best, thresholds 50 / 51
    kp = [(103, 104), (97, 96), (94, 100), (300, 100), (303, 104), (400, 300), (500, 300)]
    descs = np.stack([d_at(10), d_at(10), d_at(10), d_at(2), d_at(7), d_at(50), d_at(51)])
    kf = _kf(kp, desc=descs, grid=grid, taken=[0, 0, 0, 1, 0, 0, 0])
    pts = _pts([(100, 100), (100, 100), (300, 100), (400, 300), (500, 300)], rep(5))
    cases.append(dict(name="ties+taken+thresholds", kfs=[kf], jobs=[(0, IDENT, pts)], opts={}))
    # filters: z < 0, 0.5 px inside / outside each bound, distance outside [0.8 min, 1.2 max], a normal facing away
    uv = [(250, 250), (-0.5, 100), (0.5, 130), (639.5, 160), (640.5, 190), (100, -0.5), (130, 0.5), (160, 479.5), (190, 480.5),
          (300, 300), (330, 330), (360, 360), (390, 390)]
    kf = _kf(uv, desc=rep(len(uv)), grid=grid)
    pts = _pts(uv, rep(len(uv)))
    pts["p_w"][0] = (-250.0, -250.0, -1.0); pts["normal"][0] = -pts["normal"][0]
    d = np.linalg.norm(pts["p_w"], axis=1)
    pts["min_distance"][9] = d[9] * 1.5           # 0.8 * min > dist
    pts["max_distance"][10] = d[10] * 0.5         # 1.2 * max < dist
    pts["normal"][11] = -pts["normal"][11]        # PO . n < 0.5 dist
    cases.append(dict(name="filters", kfs=[kf], jobs=[(0, IDENT, pts)], opts={}))
    # level window and radius scaling: predicted level 3 of 8 (log_1.2(max_distance / dist) = 2.5), radius 10 * 1.2^3 = 17.28
    pos = [(100, 500), (300, 500), (500, 500), (700, 500), (900, 500)]
    kp = [(u + 9, v + 12) for u, v in pos[:4]] + [(900 + 12, 500 + 16)]      # 15 px inside, 20 px outside
    kf = _kf(kp, level=[1, 2, 3, 4, 3], desc=rep(5), grid=grid, bounds=(0.0, 1000.0, 0.0, 1000.0))
    pts = _pts(pos, rep(5))
    pts["max_distance"] = np.array([float(np.float32(np.linalg.norm(p))) * 1.2 ** 2.5 for p in pts["p_w"]])
    cases.append(dict(name="levels", kfs=[kf], jobs=[(0, IDENT, pts)], opts=dict(scale_factor=1.2, num_octaves=8)))
    return cases


# ---------------------------------------------------------------- packing, reference, comparison

def pack_sets(kfs, keys):
    """The keyframes as the CSR `sets` dict of Context.search_*_batch; `keys` = the per-row and per-set extras to carry."""
    per_row = {"kp": (2,), "level": (), "desc": (32,), "lm_pos": (3,), "lm_max_distance": (), "lm_desc": (32,), "lm_free": (), "taken": ()}
    ptr = np.zeros(len(kfs) + 1, np.int32)
    ptr[1:] = np.cumsum([len(k["kp"]) for k in kfs])
    s = dict(row_ptr=ptr, bounds=np.array([k["bounds"] for k in kfs], np.float64).reshape(-1, 4),
             grid_inv=np.array([k["grid_inv"] if k.get("grid_inv") else (0.0, 0.0) for k in kfs], np.float64).reshape(-1, 2))
    for key in ["kp", "level", "desc"] + list(keys):
        if key in per_row:
            a0 = [np.asarray(k[key]).reshape((-1,) + per_row[key]) for k in kfs]
            s[key] = np.concatenate(a0) if a0 else np.zeros((0,) + per_row[key])
        else:
            s[key] = np.array([k[key] for k in kfs])
    return s


def run_se3(ctx, case, jobs=None, **opts):
    jobs = case["jobs"] if jobs is None else jobs
    sets = pack_sets(case["kfs"], ["K", "lm_pos", "lm_max_distance", "lm_desc", "lm_free"])
    o = dict(case["opts"]); o.update(opts)
    return ctx.search_se3_batch(sets, [j[0] for j in jobs], [j[1] for j in jobs], np.array([j[2] for j in jobs]).reshape(-1, 7), **o)


def pack_points(jobs):
    ptr = np.zeros(len(jobs) + 1, np.int32)
    ptr[1:] = np.cumsum([len(j[2]["p_w"]) for j in jobs])
    cat = lambda k, w, dt: np.concatenate([np.asarray(j[2][k], dt).reshape((-1,) + w) for j in jobs]) if jobs else np.zeros((0,) + w, dt)
    return dict(set=np.array([j[0] for j in jobs], np.int32), T_cw=np.array([j[1] for j in jobs], np.float64).reshape(-1, 7), point_ptr=ptr,
                p_w=cat("p_w", (3,), np.float64), normal=cat("normal", (3,), np.float64), min_distance=cat("min_distance", (), np.float64),
                max_distance=cat("max_distance", (), np.float64), desc=cat("desc", (32,), np.uint8), skip=cat("skip", (), np.uint8),
                existing_idx=cat("existing_idx", (), np.int32))


def run_projection(ctx, case, jobs=None, **opts):
    jobs = case["jobs"] if jobs is None else jobs
    sets = pack_sets(case["kfs"], ["taken", "cam", "dist_type", "cam_model", "xi"])
    o = dict(case["opts"]); o.update(opts)
    return ctx.search_projection_batch(sets, pack_points(jobs), **o), pack_points(jobs)["point_ptr"]


def ref_se3(case, radius=9.5):
    """The restatement per job (agreement applied later with gr.agree: the two directions do not depend on it)."""
    if "_ref" not in case:
        case["_ref"] = [gr.search_se3(case["kfs"][a], case["kfs"][b], T, radius=radius, **case["opts"]) for a, b, T in case["jobs"]]
    return case["_ref"]


def ref_projection(case, radius=10.0):
    if "_ref" not in case:
        case["_ref"] = [gr.search_projection(case["kfs"][k], T, pts, radius=radius, **case["opts"]) for k, T, pts in case["jobs"]]
    return case["_ref"]


def check_se3(out, refs, agreement, exact=False):
    """Asserts the library result `out` of the jobs whose restatement results are `refs` (in job order): match1, match2 on the
    non-fragile points, match on the rows that hang on none, nfound (exactly when the job has no fragile point, else against the
    library's own match). exact: no fragile point may occur. Returns (nfound per job, fragile points, evaluated points)."""
    nf, frag, ev = [], 0, 0
    for j, r in enumerate(refs):
        a, b = int(out["offset"][j]), int(out["offset"][j + 1]); a2, b2 = int(out["offset2"][j]), int(out["offset2"][j + 1])
        f = int(r["fragile1"].sum() + r["fragile2"].sum())
        frag += f; ev += r["evaluated"]
        assert not (exact and f), f"job {j}: fragile points in an exact case"
        ok1, ok2 = ~r["fragile1"], ~r["fragile2"]
        np.testing.assert_array_equal(out["match1"][a:b][ok1], r["match1"][ok1], err_msg=f"job {j} match1")
        np.testing.assert_array_equal(out["match2"][a2:b2][ok2], r["match2"][ok2], err_msg=f"job {j} match2")
        want = gr.agree(r["match1"], r["match2"], agreement)
        ok = gr.se3_comparable(r, agreement)
        np.testing.assert_array_equal(out["match"][a:b][ok], want[ok], err_msg=f"job {j} match")
        assert int(out["nfound"][j]) == int((out["match"][a:b] >= 0).sum()), f"job {j} nfound against its own match"
        if not f:
            assert int(out["nfound"][j]) == int((want >= 0).sum()), f"job {j} nfound"
        nf.append(int(out["nfound"][j]))
    return nf, frag, ev


def check_projection(out, ptr, refs, exact=False):
    """As check_se3: claimed, remap_to, best_dist on the points before the job's first fragile one, nmatches when it has none."""
    nm, frag, ev = [], 0, 0
    for j, r in enumerate(refs):
        a, b = int(ptr[j]), int(ptr[j + 1])
        f = int(r["fragile"].sum())
        frag += f; ev += r["evaluated"]
        assert not (exact and f), f"job {j}: fragile points in an exact case"
        ok = gr.projection_comparable(r)
        for k in ("claimed", "remap_to", "best_dist"):
            np.testing.assert_array_equal(out[k][a:b][ok], r[k][ok], err_msg=f"job {j} {k}")
        assert int(out["nmatches"][j]) == int((out["claimed"][a:b] >= 0).sum()), f"job {j} nmatches against its own claims"
        if not f:
            assert int(out["nmatches"][j]) == r["nmatches"], f"job {j} nmatches"
        nm.append(int(out["nmatches"][j]))
    return nm, frag, ev


# ---------------------------------------------------------------- the C++ facade on the stand-in map

_SHIM = None


def guided_shim():
    """tests/cpp/facade_guided_shim.cpp: LoopMatcherT::SearchBySE3Batch / SearchByProjection on the stand-in map, extras through the
    optional traits."""
    global _SHIM
    if _SHIM is None:
        import ctypes as C
        import os
        import subprocess
        here = os.path.dirname(os.path.abspath(__file__)); root = os.path.dirname(here)
        so = os.path.join(here, "cpp", "libfacade_guided_shim.so")
        srcs = [os.path.join(here, "cpp", f) for f in ("facade_guided_shim.cpp", "facade_shim.cpp", "standin_map.hpp")] + \
               [os.path.join(root, "include", "covins_gpu", "optimization_gpu.hpp"), os.path.join(root, "include", "covgpu.h")]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", srcs[0], "-o", so, "-L" + os.path.join(root, "covins_amd"),
                                   "-lcovgpu", "-Wl,-rpath," + os.path.join(root, "covins_amd")])
        lib = C.CDLL(so)
        ip, dp, bp, fp = C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_float)
        lib.shim_build.restype = C.c_void_p
        lib.shim_free.argtypes = [C.c_void_p]
        lib.guided_set_params.argtypes = [C.c_int, C.c_double, C.c_int, C.c_int]
        lib.guided_set_landmarks.argtypes = [C.c_void_p, bp, dp, dp, dp]
        lib.guided_set_keyframe.argtypes = [C.c_void_p, C.c_int, C.c_int, fp, ip, bp, ip, dp, dp]
        lib.guided_se3.argtypes = [C.c_void_p, C.c_int, ip, ip, dp, ip, ip, ip, C.c_double]
        lib.guided_projection.argtypes = [C.c_void_p, C.c_int, dp, C.c_int, ip, C.c_int, ip, C.c_double]
        lib.guided_projection.restype = C.c_int
        lib.guided_get_keyframe.argtypes = [C.c_void_p, C.c_int, C.c_int, ip, ip]
        _SHIM = lib
    return _SHIM
