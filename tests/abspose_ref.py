"""numpy restatement of the loop-candidate geometric verification: Se3Solver::projectiveAlignment
(Se3Solver.cpp:59-110) = an opengv RANSAC over 2D-3D matches with a minimal P3P, scored by
FrameAbsolutePoseSacProblem::getSelectedDistancesToModel. It is the checker of k_abspose.hip, so it lives with the tests.

The P3P here is Grunert's quartic in v = s3/s1 solved by numpy.roots, the pose by Horn's quaternion alignment; the kernel
solves the same quartic in closed form (Ferrari) and aligns with two orthonormal triads, so the two check each other.
Everything is plain float64 and Python integers (the sampler is bit-exact)."""
from __future__ import annotations

import math

import numpy as np

M64 = (1 << 64) - 1
EPS = np.finfo(np.float64).eps


# ------------------------------------------------------------------------------------------------ sampler
def splitmix64(x: int) -> int:
    z = (x + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw(seed: int, d: int, n: int):
    """The 4 distinct indices of draw d: a partial Fisher-Yates over [0, n), slot k swaps position k with
    k + splitmix64(seed + 4 d + k) mod (n - k)."""
    over = {}
    out = []
    for k in range(4):
        x = splitmix64((seed + 4 * d + k) & M64)
        j = k + x % (n - k)
        vk, vj = over.get(k, k), over.get(j, j)
        over[j] = vk
        out.append(vj)
    return out


# ------------------------------------------------------------------------------------------------ model and score
def score(R, t, f, P, sig):
    """getSelectedDistancesToModel, vectorised: the inverse transform applied to [P; 1], normalised, squared distance to the
    bearing over sigma_angle. R, t: T_wc (query camera in the world)."""
    Ri = R.T
    ti = -(Ri @ t)
    body = P @ Ri.T + ti
    rep = body / np.linalg.norm(body, axis=1, keepdims=True)
    e = rep - f
    return np.sum(e * e, axis=1) / sig


def sigma_angle(octave, fx, fy):
    """FrameNoncentralAbsoluteAdapter: sqrt(2) * s^2 / fu^2 with s = 0.8 (octave + 1), fu = (fx + fy) / 2."""
    fu = (fx + fy) / 2.0
    s = 0.8 * (np.asarray(octave, dtype=np.float64) + 1)
    return math.sqrt(2) * s * s / (fu * fu)


# ------------------------------------------------------------------------------------------------ P3P
def grunert_coeffs(f, P):
    """Grunert's quartic A4 v^4 + ... + A0 in v = s3 / s1 (s_i: depth along bearing i) and what u = s2 / s1 needs."""
    ca = float(f[1] @ f[2]); cb = float(f[0] @ f[2]); cg = float(f[0] @ f[1])
    a2 = float(np.sum((P[1] - P[2]) ** 2)); b2 = float(np.sum((P[0] - P[2]) ** 2)); c2 = float(np.sum((P[0] - P[1]) ** 2))
    if b2 == 0.0:   # coincident world points: the kernel's coefficients are not finite there either
        return np.full(5, np.nan), (ca, cb, cg, math.nan, a2, b2, c2)
    amc = (a2 - c2) / b2; apc = (a2 + c2) / b2
    A4 = (amc - 1) ** 2 - 4 * c2 / b2 * ca * ca
    A3 = 4 * (amc * (1 - amc) * cb - (1 - apc) * ca * cg + 2 * c2 / b2 * ca * ca * cb)
    A2 = 2 * (amc * amc - 1 + 2 * amc * amc * cb * cb + 2 * (b2 - c2) / b2 * ca * ca - 4 * apc * ca * cb * cg + 2 * (b2 - a2) / b2 * cg * cg)
    A1 = 4 * (-amc * (1 + amc) * cb + 2 * a2 / b2 * cg * cg * cb - (1 - apc) * ca * cg)
    A0 = (1 + amc) ** 2 - 4 * a2 / b2 * cg * cg
    return np.array([A4, A3, A2, A1, A0]), (ca, cb, cg, amc, a2, b2, c2)


def refine_depths(s, ca, cb, cg, a2, b2, c2, steps=2):
    """Newton on the three law-of-cosines equations in the depths (u from Grunert's linear relation loses digits where
    cos(gamma) ~ v cos(alpha))."""
    for _ in range(steps):
        s1, s2, s3 = s
        F = np.array([s2 * s2 + s3 * s3 - 2 * s2 * s3 * ca - a2, s1 * s1 + s3 * s3 - 2 * s1 * s3 * cb - b2, s1 * s1 + s2 * s2 - 2 * s1 * s2 * cg - c2])
        J = np.array([[0.0, 2 * (s2 - s3 * ca), 2 * (s3 - s2 * ca)], [2 * (s1 - s3 * cb), 0.0, 2 * (s3 - s1 * cb)], [2 * (s1 - s2 * cg), 2 * (s2 - s1 * cg), 0.0]])
        det = np.linalg.det(J)
        if not (det != 0.0 and math.isfinite(det)):
            break
        s = s - np.linalg.solve(J, F)
    return s


def horn(X, P):
    """R, t with P = R X + t in the least-squares sense (Horn 1987, unit quaternions)."""
    cx, cp = X.mean(0), P.mean(0)
    S = (X - cx).T @ (P - cp)
    Sxx, Sxy, Sxz, Syx, Syy, Syz, Szx, Szy, Szz = S.ravel()
    N = np.array([[Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx],
                  [Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz],
                  [Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy],
                  [Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz]])
    w, V = np.linalg.eigh(N)
    q0, qx, qy, qz = V[:, -1]
    R = np.array([[q0 * q0 + qx * qx - qy * qy - qz * qz, 2 * (qx * qy - q0 * qz), 2 * (qx * qz + q0 * qy)],
                  [2 * (qy * qx + q0 * qz), q0 * q0 - qx * qx + qy * qy - qz * qz, 2 * (qy * qz - q0 * qx)],
                  [2 * (qz * qx - q0 * qy), 2 * (qz * qy + q0 * qx), q0 * q0 - qx * qx - qy * qy + qz * qz]])
    return R, cp - R @ cx


def p3p(f, P, imag_tol=1e-9):
    """Every real solution with positive depths of the central P3P on correspondences 0..2, ordered by v ascending: a list
    of (R, t), T_wc. A coefficient set with A4 == 0 or a non-finite coefficient has no solution."""
    A, (ca, cb, cg, amc, a2, b2, c2) = grunert_coeffs(f, P)
    if not np.all(np.isfinite(A)) or A[0] == 0.0:
        return []
    roots = np.roots(A)
    vs = []
    for r in roots:
        if abs(r.imag) > imag_tol * max(1.0, abs(r.real)):
            continue
        v = float(r.real)
        for _ in range(3):   # Newton on the quartic: numpy.roots (companion eigenvalues) leaves ~1e-10 relative
            fv = (((A[0] * v + A[1]) * v + A[2]) * v + A[3]) * v + A[4]
            dv = ((4 * A[0] * v + 3 * A[1]) * v + 2 * A[2]) * v + A[3]
            if dv == 0.0:
                break
            v -= fv / dv
        vs.append(v)
    vs.sort()
    sols = []
    for v in vs:
        den = 2 * (cg - v * ca)
        u = ((-1 + amc) * v * v - 2 * amc * cb * v + 1 + amc) / den if den != 0.0 else math.nan
        q = 1 + v * v - 2 * v * cb
        if not (v > 0 and u > 0 and q > 0 and math.isfinite(u)):
            continue
        s1 = math.sqrt(b2 / q)
        s = refine_depths(np.array([s1, u * s1, v * s1]), ca, cb, cg, a2, b2, c2)
        if not (np.all(np.isfinite(s)) and np.all(s > 0)):
            continue
        X = s[:, None] * f[:3]
        R, t = horn(X, P[:3])
        if np.all(np.isfinite(R)) and np.all(np.isfinite(t)):
            sols.append((R, t))
    return sols


def pick(sols, f4, P4):
    """opengv's choice among P3P solutions: the smallest 1 - <normalize(R^T (P4 - t)), f4>, first wins a tie; -1: none."""
    best, bi = 1e6, -1
    for i, (R, t) in enumerate(sols):
        Ri = R.T
        b = Ri @ P4 - Ri @ t
        s = 1.0 - float((b / np.linalg.norm(b)) @ f4)
        if s < best:
            best, bi = s, i
    return bi


# ------------------------------------------------------------------------------------------------ RANSAC loop
def ransac(f, P, sig, seed, threshold=25.0, max_iterations=300, probability=0.99, min_inliers=6, hypothesis=None):
    """opengv sac::Ransac::computeModel restated (upstream knowledge: opengv is not part of COVINS), with the sampler above.
    Returns dict(inliers (count, 0 = no transform), mask [n] bool, R, t (None if none), iterations, best_draw (-1: none),
    draws). `hypothesis(d, idx) -> (R, t) | None` replaces the P3P (hand-built loop tests)."""
    n = len(f)
    out = dict(inliers=0, mask=np.zeros(n, bool), R=None, t=None, iterations=0, best_draw=-1, draws=0)
    if n < 4:
        return out
    it, skipped, k, best = 0, 0, 1.0, -(1 << 31)
    bR = bt = None
    d = 0
    while it < k and skipped < 10 * max_iterations:
        idx = draw(seed, d, n)
        if hypothesis is not None:
            h = hypothesis(d, idx)
        else:
            sols = p3p(f[idx], P[idx])
            c = pick(sols, f[idx[3]], P[idx[3]])
            h = sols[c] if c >= 0 else None
        d += 1
        if h is None:
            skipped += 1
            continue
        cnt = int(np.sum(score(h[0], h[1], f, P, sig) < threshold))
        if cnt > best:
            best = cnt
            bR, bt = h
            out["best_draw"] = d - 1
            w = best / n
            pno = 1.0 - w ** 4.0
            pno = min(max(pno, EPS), 1.0 - EPS)
            k = math.log(1.0 - probability) / math.log(pno)
        it += 1
        if it > max_iterations:
            break
    out["iterations"], out["draws"] = it, d
    if bR is None:
        return out
    mask = score(bR, bt, f, P, sig) < threshold
    if int(mask.sum()) < min_inliers or int(mask.sum()) == 0:
        return out
    out.update(inliers=int(mask.sum()), mask=mask, R=bR, t=bt)
    return out


def ransac_batch(bt, seeds, **opts):
    """ransac() per candidate of a batch dict (ptr, bearing, point_w, sigma_angle): list of results."""
    ptr = bt["ptr"]
    res = []
    for b in range(len(ptr) - 1):
        s = slice(int(ptr[b]), int(ptr[b + 1]))
        res.append(ransac(bt["bearing"][s], bt["point_w"][s], bt["sigma_angle"][s], int(seeds[b]), **opts))
    return res


def rot_to_quat(R):
    """Hamilton quaternion x, y, z, w of a rotation matrix (w >= 0)."""
    from scipy.spatial.transform import Rotation
    q = Rotation.from_matrix(R).as_quat()
    return -q if q[3] < 0 else q
