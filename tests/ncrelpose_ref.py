"""Numpy checker of the 17-point batch (covgpu_ncrelpose_batch): the contract restated, draw for draw.

Route A is the reference of the tests: the linear solve by numpy.linalg.svd (null vector, nearest rotation, mean singular value), the
polish by scipy.optimize.least_squares run to convergence. Route B restates the kernel's own formulation: Householder QR of the N x 18
system, one-sided Jacobi on the 18 x 18 factor in a round-robin order, the polar factor by Newton's iteration with Frobenius scaling,
Levenberg-Marquardt with central differences. The spread between the two routes is the yardstick the device is held to (10 x).

Poses are T_12 = [R | t], x1 = R x2 + t; [7] = qx qy qz qw x y z (Hamilton, w >= 0)."""
import math

import numpy as np

SAMPLE = 17
COLS = 18
COV_SAMPLE = 4
SWEEPS = 16
POLAR = 12
LM_ITERS = 40
LM_STEP = 1e-6
LM_TOL = 1e-12
RANK_TOL = 1e-12
COV_SALT = 0x17C0F17C0F17C0F1
DEFAULTS = dict(rp_error=1.5, rp_error_cov=10.0, min_inliers=100, max_iterations=4000, cov_thres=10.0, cov_iters=30, cov_max_iters=300,
                probability=0.99)
M64 = (1 << 64) - 1


def splitmix64(x):
    z = (x + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw(key, cnt, n):
    """cnt distinct indices of [0, n): partial Fisher-Yates, slot k swaps position k with k + splitmix64(key + k) mod (n - k)."""
    a = list(range(n))
    for k in range(cnt):
        j = k + splitmix64((key + k) & M64) % (n - k)
        a[k], a[j] = a[j], a[k]
    return a[:cnt]


def threshold(rp_error):
    return 2.0 * (1.0 - math.cos(math.atan(rp_error * 1 / 800.0)))


# ---- rotations
def skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def exp_so3(w):
    th = float(np.linalg.norm(w))
    if th < 1e-12:
        return np.eye(3) + skew(w)
    K = skew(np.asarray(w) / th)
    return np.eye(3) + math.sin(th) * K + (1.0 - math.cos(th)) * (K @ K)


def quat_rot(q):
    x, y, z, w = (float(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def rot_quat(R):
    """Hamilton x y z w, w >= 0, of a rotation: the eigenvector of the largest eigenvalue of the 4x4 symmetric form."""
    K = np.array([[R[0, 0] - R[1, 1] - R[2, 2], R[1, 0] + R[0, 1], R[2, 0] + R[0, 2], R[2, 1] - R[1, 2]],
                  [R[1, 0] + R[0, 1], R[1, 1] - R[0, 0] - R[2, 2], R[2, 1] + R[1, 2], R[0, 2] - R[2, 0]],
                  [R[2, 0] + R[0, 2], R[2, 1] + R[1, 2], R[2, 2] - R[0, 0] - R[1, 1], R[1, 0] - R[0, 1]],
                  [R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1], R[0, 0] + R[1, 1] + R[2, 2]]]) / 3.0
    w, v = np.linalg.eigh(K)
    q = v[:, -1]
    return q if q[3] >= 0 else -q


def qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz])


def pose7(R, t):
    return np.concatenate([rot_quat(R), np.asarray(t, float)])


def pose_error(R, t, Rt, tt):
    """(rotation angle between the two rotations [rad], norm of the translation difference)"""
    c = (np.trace(R.T @ Rt) - 1.0) / 2.0
    s = np.linalg.norm(R.T @ Rt - (R.T @ Rt).T) / (2.0 * math.sqrt(2.0))
    return math.atan2(s, c), float(np.linalg.norm(np.asarray(t) - np.asarray(tt)))


def sensor_pose(Tq, Tc, R, t):
    """T_s1s2 = T_sc(Q) T_c1c2 T_sc(C)^-1 as (R, t)"""
    Rq, Rc = quat_rot(np.asarray(Tq[:4]) / np.linalg.norm(Tq[:4])), quat_rot(np.asarray(Tc[:4]) / np.linalg.norm(Tc[:4]))
    Ra, ta = Rq @ R, Rq @ t + Tq[4:]
    Rci, tci = Rc.T, -Rc.T @ Tc[4:]
    return Ra @ Rci, Ra @ tci + ta


def minus(q_iter, q_ref):
    """robopt's Minus as restated: 2 vec(q_iter (x) q_ref^-1), the sign with w >= 0"""
    d = qmul(q_iter, np.array([-q_ref[0], -q_ref[1], -q_ref[2], q_ref[3]]))
    return (2.0 if d[3] >= 0 else -2.0) * d[:3]


# ---- rays, rows, the linear solve
def rays(f1, f2, cam1, cam2, cam):
    """g = R_c f, origin o_c: (g1, o1, g2, o2), each [n, 3]"""
    cam = np.asarray(cam, float).reshape(-1, 12)
    R1, R2 = cam[cam1, :9].reshape(-1, 3, 3), cam[cam2, :9].reshape(-1, 3, 3)
    return np.einsum("nij,nj->ni", R1, f1), cam[cam1, 9:], np.einsum("nij,nj->ni", R2, f2), cam[cam2, 9:]


def rows(g1, o1, g2, o2):
    """[g1 (x) g2 , g1 (x) m2 + m1 (x) g2], m = o x g: [..., 18]"""
    m1, m2 = np.cross(o1, g1), np.cross(o2, g2)
    a = np.einsum("...i,...j->...ij", g1, g2)
    b = np.einsum("...i,...j->...ij", g1, m2) + np.einsum("...i,...j->...ij", m1, g2)
    return np.concatenate([a.reshape(a.shape[:-2] + (9,)), b.reshape(b.shape[:-2] + (9,))], axis=-1)


def singular_values(A):
    s = np.linalg.svd(A, compute_uv=False)
    s = np.concatenate([s, np.zeros(COLS - len(s))]) if len(s) < COLS else s
    return s[0], s[COLS - 2], s[COLS - 1]


def solve_a(A):
    """Route A on one N x 18 system: (R, t) or None (a failed draw)."""
    if not np.all(np.isfinite(A)):
        return None
    Ap = np.vstack([A, np.zeros((max(0, COLS - len(A)), COLS))])
    try:
        _, s, Vt = np.linalg.svd(Ap)
    except np.linalg.LinAlgError:
        return None
    if not (s[0] > 0.0) or not (s[COLS - 2] > RANK_TOL * s[0]):
        return None
    x = Vt[-1]
    E, Rt = x[:9].reshape(3, 3), x[9:].reshape(3, 3)
    det = np.linalg.det(Rt)
    if det == 0.0 or not np.isfinite(det):
        return None
    if det < 0:
        E, Rt = -E, -Rt
    U, sr, Wt = np.linalg.svd(Rt)
    R = U @ Wt
    sc = sr.mean()
    M = (E / sc) @ R.T
    t = 0.5 * np.array([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]])
    if not (np.all(np.isfinite(R)) and np.all(np.isfinite(t))):
        return None
    return R, t


def _round_robin():
    out = []
    for r in range(COLS - 1):
        lo, hi = [], []
        for i in range(COLS):
            p = r if i == COLS - 1 else ((2 * r - i) % (COLS - 1))
            if i < COLS - 1 and p == i:
                p = COLS - 1
            if i < p:
                lo.append(i); hi.append(p)
        out.append((np.array(lo), np.array(hi)))
    return out


_ROUNDS = _round_robin()


def solve_b(A):
    """Route B on a batch of systems [T, N, 18], the kernel's formulation. Returns ok [T], R [T,3,3], t [T,3], sv [T,3]."""
    A = np.asarray(A, float)
    T, N = A.shape[0], A.shape[1]
    if N < COLS:
        A = np.concatenate([A, np.zeros((T, COLS - N, COLS))], axis=1)
    Rf = np.linalg.qr(A, mode="r")[:, :COLS, :]
    X = np.concatenate([Rf, np.broadcast_to(np.eye(COLS), (T, COLS, COLS))], axis=1)            # columns of [R; V]
    Xc = np.ascontiguousarray(X.transpose(2, 1, 0))                                              # [column, component, tuple]
    with np.errstate(all="ignore"):
        for _ in range(SWEEPS):
            moved = False                                   # (a sweep in which no pair rotates changes nothing, nor would the ones after it)
            for lo, hi in _ROUNDS:
                p, q = Xc[lo], Xc[hi]
                aa, bb, ab = (p[:, :COLS] ** 2).sum(1), (q[:, :COLS] ** 2).sum(1), (p[:, :COLS] * q[:, :COLS]).sum(1)
                rot = np.abs(ab) > 1.1e-16 * np.sqrt(aa * bb)
                zeta = (bb - aa) / (2.0 * ab)
                t = np.where(zeta < 0, -1.0, 1.0) / (np.abs(zeta) + np.sqrt(1.0 + zeta * zeta))
                c = 1.0 / np.sqrt(1.0 + t * t)
                s = c * t
                rot &= np.isfinite(c) & np.isfinite(s)
                c = np.where(rot, c, 1.0)[:, None, :]; s = np.where(rot, s, 0.0)[:, None, :]
                Xc[lo], Xc[hi] = c * p - s * q, s * p + c * q
                moved = moved or bool(rot.any())
            if not moved:
                break
        X = Xc.transpose(2, 1, 0)
        n2 = (X[:, :COLS] ** 2).sum(1)
        order = np.argsort(n2, axis=1, kind="stable")
        ar = np.arange(T)
        mn, m2, mx = n2[ar, order[:, 0]], n2[ar, order[:, 1]], n2[ar, order[:, -1]]
        ok = np.isfinite(mx) & (mx > 0) & (m2 > RANK_TOL * RANK_TOL * mx)
        x = X[ar, COLS:, order[:, 0]]
        E, Rt = x[:, :9].reshape(T, 3, 3), x[:, 9:].reshape(T, 3, 3)
        det = np.linalg.det(Rt)
        ok &= np.isfinite(det) & (det != 0.0)
        sg = np.where(det < 0, -1.0, 1.0)[:, None, None]
        E, Rt = sg * E, sg * Rt
        Y = Rt.copy()
        for _ in range(POLAR):
            d = np.linalg.det(Y)
            cof = np.stack([np.cross(Y[:, (i + 1) % 3], Y[:, (i + 2) % 3]) for i in range(3)], axis=1) / d[:, None, None]   # Y^-T
            gam = np.sqrt(np.sqrt((cof ** 2).sum((1, 2)) / (Y ** 2).sum((1, 2))))[:, None, None]
            Y = 0.5 * (gam * Y + cof / gam)
        sc = (Y * Rt).sum((1, 2)) / 3.0
        M = np.einsum("tik,tjk->tij", E, Y) / sc[:, None, None]
        t = 0.5 * np.stack([M[:, 2, 1] - M[:, 1, 2], M[:, 0, 2] - M[:, 2, 0], M[:, 1, 0] - M[:, 0, 1]], axis=1)
        ok &= np.isfinite(Y).all((1, 2)) & np.isfinite(t).all(1)
    return ok, Y, t, np.sqrt(np.stack([mx, m2, mn], axis=1))


# ---- the score and the residuals
def reproject(R, t, g1, o1, g2, o2):
    """triangulate2 on general rays: u1, u2 (directions from the two origins to the midpoint P) and the rotated g2"""
    g = g2 @ R.T
    o = o2 @ R.T + t
    b = o - o1
    b0, b1 = (b * g1).sum(-1), (b * g).sum(-1)
    a00, a01, a11 = (g1 * g1).sum(-1), -(g1 * g).sum(-1), -(g * g).sum(-1)
    with np.errstate(all="ignore"):
        det = a00 * a11 + a01 * a01
        l0, l1 = (a11 * b0 - a01 * b1) / det, (a01 * b0 + a00 * b1) / det
        P = 0.5 * (o1 + g1 * l0[..., None] + o + g * l1[..., None])
        d1, d2 = P - o1, P - o
        u1 = d1 / np.linalg.norm(d1, axis=-1, keepdims=True)
        u2 = d2 / np.linalg.norm(d2, axis=-1, keepdims=True)
    return u1, u2, g


def scores(R, t, ry):
    u1, u2, g = reproject(R, t, *ry)
    return (1.0 - (ry[0] * u1).sum(-1)) + (1.0 - (g * u2).sum(-1))


def inlier_mask(R, t, ry, th):
    with np.errstate(all="ignore"):
        return scores(R, t, ry) < th          # a non-finite score compares false


def residuals(R, t, ry):
    u1, u2, g = reproject(R, t, *ry)
    return np.concatenate([u1 - ry[0], u2 - g], axis=-1)       # [n, 6]


def cost(R, t, ry):
    return float((residuals(R, t, ry) ** 2).sum())


def take(ry, idx):
    return tuple(a[idx] for a in ry)


def _margin(sc, th):
    """the smallest relative distance of a finite score from the threshold"""
    f = sc[np.isfinite(sc)]
    return float(np.abs(f - th).min() / th) if len(f) else math.inf


# ---- the RANSAC (§4.10's loop, sample size 17)
def ransac(ry, seed, th, min_inliers=100, max_iterations=4000, probability=0.99, hypothesis=None):
    n = len(ry[0])
    out = dict(status=1, iterations=0, best_draw=-1, inliers=0, mask=np.zeros(n, bool), model=None, draws=0, models={}, margin=math.inf)
    if n < SAMPLE:
        return out
    it = skipped = 0
    bestn, k, d = -(1 << 31), 1.0, 0
    while it < k and skipped < 10 * max_iterations:
        idx = draw((seed + SAMPLE * d) & M64, SAMPLE, n)
        m = hypothesis(d, idx) if hypothesis else solve_a(rows(*take(ry, idx)))
        d += 1
        if m is None:
            skipped += 1
            continue
        with np.errstate(all="ignore"):
            sc = scores(m[0], m[1], ry)
        c = int((sc < th).sum())
        out["margin"] = min(out["margin"], _margin(sc, th))
        out["models"][d - 1] = m
        if c > bestn:
            bestn, out["best_draw"], out["model"] = c, d - 1, m
            w = bestn / n
            pno = min(1.0 - np.finfo(float).eps, max(np.finfo(float).eps, 1.0 - w ** SAMPLE))
            k = math.log(1.0 - probability) / math.log(pno)
        it += 1
        if it > max_iterations:
            break
    out["iterations"], out["draws"] = it, d
    if out["model"] is None:
        out["status"] = 2
        return out
    out["mask"] = inlier_mask(out["model"][0], out["model"][1], ry, th)
    out["inliers"] = int(out["mask"].sum())
    out["status"] = 3 if out["inliers"] < min_inliers else 0
    return out


# ---- the polish
def polish_a(R, t, ry):
    """Route A: scipy's trust-region least squares on (right rotation perturbation, t), re-centred until the step vanishes."""
    from scipy.optimize import least_squares
    R, t = R.copy(), np.asarray(t, float).copy()
    for _ in range(5):
        fun = lambda x: residuals(R @ exp_so3(x[:3]), t + x[3:], ry).ravel()
        r = least_squares(fun, np.zeros(6), method="trf", xtol=1e-15, ftol=1e-15, gtol=1e-15, x_scale=1.0, max_nfev=200)
        R, t = R @ exp_so3(r.x[:3]), t + r.x[3:]
        if np.abs(r.x).max() < 1e-13:
            break
    return R, t


def polish_b(R, t, ry):
    """Route B: the kernel's Levenberg-Marquardt with central differences."""
    R, t, lam = R.copy(), np.asarray(t, float).copy(), 1e-3
    for _ in range(LM_ITERS):
        e = residuals(R, t, ry).ravel()
        J = np.zeros((len(e), 6))
        for p in range(6):
            d = np.zeros(6); d[p] = LM_STEP
            ep = residuals(R @ exp_so3(d[:3]), t + d[3:], ry).ravel()
            em = residuals(R @ exp_so3(-d[:3]), t - d[3:], ry).ravel()
            J[:, p] = (ep - em) * (0.5 / LM_STEP)
        H, g = J.T @ J, J.T @ e
        H = H + lam * np.diag(np.diag(H))
        try:
            step = np.linalg.solve(H, -g)
            pd = bool(np.all(np.isfinite(step))) and bool(np.all(np.linalg.eigvalsh(H) > 0))
        except np.linalg.LinAlgError:
            step, pd = np.zeros(6), False
        done = (pd and np.abs(step).max() < LM_TOL) or lam >= 1e12
        Rc, tc = R @ exp_so3(step[:3]), t + step[3:]
        if pd and cost(Rc, tc, ry) < float(e @ e):
            R, t, lam = Rc, tc, max(lam * 0.1, 1e-15)
        else:
            lam *= 10.0
        if done:
            break
    return R, t


# ---- the covariance
def covariance(ry, mask, cell_ptr, seed, R, t, Tq, Tc, th_cov, cov_iters=30, cov_max_iters=300, cov_thres=10.0, solver=None):
    """RelNonCentralPosSolver.cpp:187-292 as restated: dict(status 0 | 4 | 5 | 6, rows, draws, cov, m)"""
    solver = solver or solve_a
    cells = len(cell_ptr) - 1
    inl = np.flatnonzero(mask)
    per = [inl[(inl >= cell_ptr[j]) & (inl < cell_ptr[j + 1])] for j in range(cells)]
    out = dict(status=4, rows=0, draws=0, cov=None, m=None, margin=math.inf)
    if any(len(p) < 2 * COV_SAMPLE for p in per):
        return out
    cseed = splitmix64(seed ^ COV_SALT)
    Rs, ts = sensor_pose(Tq, Tc, R, t)
    qref = rot_quat(Rs)
    ryi = take(ry, inl)
    m, e = [], 0
    while len(m) < cov_iters and e <= cov_max_iters:
        idx = []
        for j in range(cells):
            idx += [int(per[j][k]) for k in draw((cseed + (e * cells + j) * COV_SAMPLE) & M64, COV_SAMPLE, len(per[j]))]
        e += 1
        mod = solver(rows(*take(ry, idx)))
        if mod is None:
            continue
        with np.errstate(all="ignore"):
            sc = scores(mod[0], mod[1], ryi)
        c = int((sc < th_cov).sum())
        out["margin"] = min(out["margin"], _margin(sc, th_cov))
        if float(np.float32(c) / np.float32(len(inl))) > 0.8:
            Ri, ti = sensor_pose(Tq, Tc, mod[0], mod[1])
            m.append(np.concatenate([minus(rot_quat(Ri), qref), ti]))
    out["rows"], out["draws"] = len(m), e
    if len(m) < cov_iters:
        out["status"] = 5
        return out
    m = np.array(m)
    d = m - np.concatenate([np.zeros(3), ts])
    out["m"], out["cov"] = m, d.T @ d / (len(m) - 1)
    out["status"] = 0 if np.trace(out["cov"]) < cov_thres else 6
    return out


def solve_b_one(A):
    ok, R, t, _ = solve_b(A[None])
    return (R[0], t[0]) if ok[0] else None


def job_rays(j):
    return rays(j["f1"], j["f2"], j["cam1"], j["cam2"], j["cam"])


def run(j, seed, route="a", **opts):
    """The whole job as the library runs it. `j`: dict(f1, f2, cam1, cam2, cam, cell_ptr, T_sc_q, T_sc_c)."""
    o = dict(DEFAULTS); o.update(opts)
    ry = job_rays(j)
    th, thc = threshold(o["rp_error"]), threshold(o["rp_error_cov"])
    r = ransac(ry, seed, th, o["min_inliers"], o["max_iterations"], o["probability"],
               hypothesis=None if route == "a" else (lambda d, idx: solve_b_one(rows(*take(ry, idx)))))
    out = dict(status=r["status"], iterations=r["iterations"], best_draw=r["best_draw"], inliers=r["inliers"], mask=r["mask"], ransac=r["model"],
               models=r["models"], margin=r["margin"], rows=0, draws=0, cov=None, polished=None, T_s1s2=None)
    if r["status"] != 0:
        return out
    ryi = take(ry, np.flatnonzero(r["mask"]))
    R, t = (polish_a if route == "a" else polish_b)(r["model"][0], r["model"][1], ryi)
    out["polished"] = (R, t)
    out["T_s1s2"] = sensor_pose(j["T_sc_q"], j["T_sc_c"], R, t)
    c = covariance(ry, r["mask"], j["cell_ptr"], seed, R, t, j["T_sc_q"], j["T_sc_c"], thc, o["cov_iters"], o["cov_max_iters"], o["cov_thres"],
                   solver=solve_a if route == "a" else solve_b_one)
    out.update(status=c["status"], rows=c["rows"], draws=c["draws"], cov=c["cov"], m=c["m"], margin=min(r["margin"], c["margin"]))
    return out
