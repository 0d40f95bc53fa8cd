"""Candidate batches for the loop-candidate geometric verification (covgpu_abspose_ransac_batch).

`map_batch` builds them from a synthetic map (covins_amd/synth.py, unchanged): a query keyframe and a candidate keyframe that share
landmarks; per shared landmark the query's bearing (its keypoint undistorted as Keyframe::keypoints_undistorted_, then
keyframe_be.cpp:209-218), the landmark's world position in the map's drifted estimate, an octave 0-3 and the adapter's sigma_angle;
a chosen fraction of the landmarks replaced by wrong ones. The reference pose of a candidate is the query's estimated camera pose
(T_w_s of the map times T_s_c): the landmarks it sees were triangulated from keyframes close to it, so they carry nearly its drift.
`random_batch` draws free-standing candidates of any size."""
from __future__ import annotations

import numpy as np
from scipy.spatial.transform import Rotation as Rot

from tests import abspose_ref as ar


def undistort_radtan(uv, intr, dist, iters=20):
    """Fixed-point inversion of the radial-tangential model (what cv::undistortPoints does for keypoints_undistorted_), pixels."""
    fx, fy, cx, cy = intr
    k1, k2, p1, p2 = dist
    xd = (uv[:, 0] - cx) / fx; yd = (uv[:, 1] - cy) / fy
    x, y = xd.copy(), yd.copy()
    for _ in range(iters):
        r2 = x * x + y * y
        rad = 1 + k1 * r2 + k2 * r2 * r2
        dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x); dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x = (xd - dx) / rad; y = (yd - dy) / rad
    return np.stack([fx * x + cx, fy * y + cy], 1)


def bearings(uv_undist, intr):
    """keyframe_be.cpp:209-218: ((u - cx) / fx, (v - cy) / fy, 1), normalised."""
    fx, fy, cx, cy = intr
    b = np.stack([(uv_undist[:, 0] - cx) * (1.0 / fx), (uv_undist[:, 1] - cy) * (1.0 / fy), np.ones(len(uv_undist))], 1)
    return b / np.linalg.norm(b, axis=1, keepdims=True)


def pose_matrix(p7):
    T = np.eye(4)
    T[:3, :3] = Rot.from_quat(p7[:4]).as_matrix(); T[:3, 3] = p7[4:]
    return T


def _move_near_threshold(cand, seed, opts, rng):
    """A correspondence whose score under the reference's final model lies within 1e-7 relative of the threshold decides on the last
    bits of two different P3P formulations: move its world point a little, until none is left."""
    th = opts.get("threshold", 25.0)
    for _ in range(20):
        r = ar.ransac(cand["bearing"], cand["point_w"], cand["sigma_angle"], seed, **opts)
        if r["R"] is None:
            return r
        sc = ar.score(r["R"], r["t"], cand["bearing"], cand["point_w"], cand["sigma_angle"])
        near = np.abs(sc - th) <= 1e-7 * th
        if not near.any():
            return r
        cand["point_w"][near] += rng.normal(0, 0.01, (int(near.sum()), 3))
    raise RuntimeError("could not move every correspondence off the threshold")


def _pack(cands, seeds, refs, truth):
    ptr = np.zeros(len(cands) + 1, np.int32)
    ptr[1:] = np.cumsum([len(c["bearing"]) for c in cands])
    cat = lambda k, w: np.ascontiguousarray(np.concatenate([c[k] for c in cands]) if cands else np.zeros((0,) + w))
    return dict(ptr=ptr, bearing=cat("bearing", (3,)), point_w=cat("point_w", (3,)), sigma_angle=cat("sigma_angle", ()),
                octave=cat("octave", ()), outlier=cat("outlier", ()), seed=np.array(seeds, np.uint64), ref=refs, truth=truth)


def map_batch(m, num, seed=0, outlier_range=(0.1, 0.6), nmin=20, nmax=400, opts=None, with_ref=True):
    """`num` candidates from map `m` (see the module doc). Returns the batch dict (ptr, bearing, point_w, sigma_angle, seed [num] uint64,
    octave, outlier flags, truth [num] 4x4 T_wc, query / candidate keyframe indices) and, with_ref, the numpy restatement's result per
    candidate (after moving near-threshold correspondences)."""
    opts = opts or {}
    rng = np.random.default_rng(seed)
    K = m.K
    kf_lms = [[] for _ in range(K)]
    kf_obs = [[] for _ in range(K)]
    for l in range(m.L):
        for o in range(m.lm_obs_ptr[l], m.lm_obs_ptr[l + 1]):
            kf_lms[m.obs_kf[o]].append(l); kf_obs[m.obs_kf[o]].append(o)
    lm_sets = [set(s) for s in kf_lms]
    cands, seeds, refs, truth, pairs = [], [], [], [], []
    while len(cands) < num:
        q = int(rng.integers(K))
        if len(kf_lms[q]) < nmin:
            continue
        c = int(rng.integers(K))
        shared = [i for i, l in enumerate(kf_lms[q]) if l in lm_sets[c]] if c != q else []
        if len(shared) < nmin:   # candidate keyframes that share landmarks: take the query's whole view when the pair shares few
            shared = list(range(len(kf_lms[q])))
        n = min(len(shared), int(rng.integers(nmin, nmax + 1)))
        pick = np.sort(rng.choice(len(shared), n, replace=False))
        idx = [shared[i] for i in pick]
        lms = np.array([kf_lms[q][i] for i in idx]); obs = np.array([kf_obs[q][i] for i in idx])
        a = int(m.kf_cam[q])
        intr, dist = m.cam_intr[a], m.cam_dist[a]
        f = bearings(undistort_radtan(m.obs_uv[obs].astype(np.float64), intr, dist), intr)
        P = m.lm_pos[lms].copy()
        frac = rng.uniform(*outlier_range)
        bad = rng.random(n) < frac
        P[bad] = m.lm_pos[rng.integers(m.L, size=int(bad.sum()))]
        octave = rng.integers(0, 4, n)
        cand = dict(bearing=f, point_w=P, sigma_angle=ar.sigma_angle(octave, intr[0], intr[1]), octave=octave, outlier=bad)
        s = int(rng.integers(1 << 63))
        r = _move_near_threshold(cand, s, opts, rng) if with_ref else None
        cands.append(cand); seeds.append(s); refs.append(r)
        truth.append(pose_matrix(m.kf_pose[q]) @ pose_matrix(m.cam_extr[a]))
        pairs.append((q, c))
    bt = _pack(cands, seeds, refs, np.array(truth))
    bt["pairs"] = np.array(pairs, np.int32)
    return bt


def random_batch(sizes, seed=0, outlier_frac=0.3, px=0.5, opts=None, with_ref=True):
    """Free-standing candidates of the given sizes: a random camera T_wc, points 2-12 m in front of it inside a 90 degree cone, pixel
    noise px at fu = 458, a fraction of gross outliers (random world points)."""
    opts = opts or {}
    rng = np.random.default_rng(seed)
    cands, seeds, refs, truth = [], [], [], []
    for n in sizes:
        R = Rot.random(random_state=int(rng.integers(1 << 31))).as_matrix(); t = rng.normal(0, 3, 3)
        z = rng.uniform(2, 12, n)
        Xc = np.stack([rng.uniform(-1, 1, n) * z, rng.uniform(-0.7, 0.7, n) * z, z], 1)
        f = Xc + np.concatenate([rng.normal(0, px / 458.0, (n, 2)) * z[:, None], np.zeros((n, 1))], 1)
        f /= np.linalg.norm(f, axis=1, keepdims=True)
        P = Xc @ R.T + t
        bad = rng.random(n) < outlier_frac
        P[bad] = rng.normal(0, 6, (int(bad.sum()), 3)) + t
        octave = rng.integers(0, 4, n)
        cand = dict(bearing=f, point_w=P, sigma_angle=ar.sigma_angle(octave, 458.654, 457.296), octave=octave, outlier=bad)
        s = int(rng.integers(1 << 63))
        r = _move_near_threshold(cand, s, opts, rng) if with_ref and n >= 4 else (ar.ransac(f, P, cand["sigma_angle"], s, **opts) if with_ref else None)
        cands.append(cand); seeds.append(s); refs.append(r)
        T = np.eye(4); T[:3, :3] = R; T[:3, 3] = t
        truth.append(T)
    return _pack(cands, seeds, refs, np.array(truth))
