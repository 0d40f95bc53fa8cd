"""A plain restatement of the inertial path in numpy.longdouble (80-bit extended on x86-64: eps 1.1e-19), written from SURVEY.md A.4 — not a
translation of k_inertial.hip or of oracle/covo_residuals.hpp — for tests/test_imu_host.py and tests/test_gpu_imu.py:

  preintegrate()   the midpoint preintegration: delta[11] = [dp, dq(xyzw), dv, sum dt], J[15x15], P[15x15]
  unwhitened()     the factor: residual u[15] and Jacobian A[15x30], parameter order [pose_i(6) sb_i(9) pose_j(6) sb_j(9)], pose tangent
                   [dtheta, dp] under q (x) Exp(dtheta), p + dp; the pose columns of constant keyframes zeroed
  whitening()      W = chol(P)^-1 (lower), by hand in long double; zeros for a factor of fewer than two samples (the rule of
                   covgpu_result::reserved) or a covariance that is not positive definite
  normal_pieces()  J^T J (30x30) and J^T r of a whitened factor
  problem()        all of it for every factor of a FlatProblem, preintegrated at the bias of keyframe imu_kf_j[f]

One formula of A.4 is a first-order statement and is restated as such (`exact_bg=False`, what the product and the oracle compute):
d r_theta / d bg_i = -L(e^-1) J[R,BG] treats dq_c = normalise(dq (x) [h, 1]), h = J[R,BG] dbg / 2, as dq_c (x) [dh, 1] under h -> h + dh. Exactly,
[h, 1]^-1 (x) [h + dh, 1] = [(dh - h x dh), 1 + h.(h + dh)] / (1 + |h|^2), so the exact block carries the factor (I - [h]x) / (1 + |h|^2) in front of
J[R,BG] (`exact_bg=True`). That is the version central differences confirm; the two differ by |h|, 6e-4 at a gyroscope bias shift of 0.005 rad/s.
"""
import numpy as np

LD = np.longdouble
EPS_LD = float(np.finfo(LD).eps)


def _v(a):
    return np.asarray(a, dtype=LD)


def skew(v):
    z = LD(0)
    return np.array([[z, -v[2], v[1]], [v[2], z, -v[0]], [-v[1], v[0], z]], dtype=LD)


def qmul(a, b):
    """Hamilton product, [x, y, z, w]."""
    av, aw, bv, bw = a[:3], a[3], b[:3], b[3]
    out = np.empty(4, LD)
    out[:3] = aw * bv + bw * av + np.cross(av, bv)
    out[3] = aw * bw - av @ bv
    return out


def qconj(q):
    return np.array([-q[0], -q[1], -q[2], q[3]], dtype=LD)


def qnormalize(q):
    return q / np.sqrt(q @ q)


def qrot(q):
    """Rotation matrix of a unit quaternion."""
    v, w = q[:3], q[3]
    return (w * w - v @ v) * np.eye(3, dtype=LD) + 2 * np.outer(v, v) + 2 * w * skew(v)


def qexp(phi):
    """Exp(phi) = [sin(|phi|/2) phi/|phi|, cos(|phi|/2)] (A.1)."""
    phi = _v(phi)
    n = np.sqrt(phi @ phi)
    out = np.empty(4, LD)
    if n < LD(1e-30):
        out[:3], out[3] = phi / 2, LD(1)
    else:
        out[:3], out[3] = np.sin(n / 2) * phi / n, np.cos(n / 2)
    return out


def L3(e):
    """L(e) = e_w I + [e_v]x (A.1)."""
    return e[3] * np.eye(3, dtype=LD) + skew(e[:3])


def R3(e):
    """Rr(e) = e_w I - [e_v]x (A.1)."""
    return e[3] * np.eye(3, dtype=LD) - skew(e[:3])


def pose_plus(T, d):
    """The project's retraction: q (x) Exp(dtheta), p + dp; d = [dtheta, dp]."""
    T, d = _v(T), _v(d)
    return np.concatenate([qmul(T[:4], qexp(d[:3])), T[4:] + d[3:]])


# ------------------------------------------------------------------------------------------------ R2: preintegration
def preintegrate(first6, samples, ba, bg, noise5):
    """(delta[11], J[15,15], P[15,15]) of samples [n,7] = (dt, acc, gyr) after the reading first6 = (acc_0, gyr_0), at the biases (ba, bg);
    noise5 = (sigma_a, sigma_g, sigma_aw, sigma_gw, g). State order [P, R, V, BA, BG], noise order [n_a0, n_g0, n_a1, n_g1, n_ba, n_bg]."""
    first6, samples, ba, bg = _v(first6), _v(samples).reshape(-1, 7), _v(ba), _v(bg)
    sa, sg, saw, sgw = (LD(x) for x in noise5[:4])
    N = np.repeat(np.array([sa * sa, sg * sg, sa * sa, sg * sg, saw * saw, sgw * sgw], dtype=LD), 3)
    I3 = np.eye(3, dtype=LD)
    dp, dv, dq, T = np.zeros(3, LD), np.zeros(3, LD), np.array([0, 0, 0, 1], dtype=LD), LD(0)
    J, P = np.eye(15, dtype=LD), np.zeros((15, 15), LD)
    a0, w0 = first6[:3], first6[3:]
    half, quarter, eighth = LD(1) / 2, LD(1) / 4, LD(1) / 8
    for s in samples:
        dt, a1, w1 = s[0], s[1:4], s[4:7]
        w = half * (w0 + w1) - bg
        dq1 = qnormalize(qmul(dq, np.concatenate([w * dt / 2, [LD(1)]])))
        Rq, Rr = qrot(dq), qrot(dq1)
        A0, A1, Om = skew(a0 - ba), skew(a1 - ba), skew(w)
        abar = half * (Rq @ (a0 - ba) + Rr @ (a1 - ba))
        dp1 = dp + dv * dt + half * abar * dt * dt
        dv1 = dv + abar * dt
        ImO = I3 - Om * dt
        F = np.zeros((15, 15), LD)
        F[0:3, 0:3] = I3
        F[0:3, 3:6] = -quarter * Rq @ A0 * dt ** 2 - quarter * Rr @ A1 @ ImO * dt ** 2
        F[0:3, 6:9] = I3 * dt
        F[0:3, 9:12] = -quarter * (Rq + Rr) * dt ** 2
        F[0:3, 12:15] = quarter * Rr @ A1 * dt ** 3
        F[3:6, 3:6] = ImO
        F[3:6, 12:15] = -I3 * dt
        F[6:9, 3:6] = -half * Rq @ A0 * dt - half * Rr @ A1 @ ImO * dt
        F[6:9, 6:9] = I3
        F[6:9, 9:12] = -half * (Rq + Rr) * dt
        F[6:9, 12:15] = half * Rr @ A1 * dt ** 2
        F[9:12, 9:12] = I3
        F[12:15, 12:15] = I3
        V = np.zeros((15, 18), LD)
        V[0:3, 0:3] = quarter * Rq * dt ** 2
        V[0:3, 3:6] = V[0:3, 9:12] = -eighth * Rr @ A1 * dt ** 3
        V[0:3, 6:9] = quarter * Rr * dt ** 2
        V[3:6, 3:6] = V[3:6, 9:12] = half * I3 * dt
        V[6:9, 0:3] = half * Rq * dt
        V[6:9, 3:6] = V[6:9, 9:12] = -quarter * Rr @ A1 * dt ** 2
        V[6:9, 6:9] = half * Rr * dt
        V[9:12, 12:15] = I3 * dt
        V[12:15, 15:18] = I3 * dt
        J = F @ J
        P = F @ P @ F.T + (V * N[None, :]) @ V.T
        dp, dv, dq, T = dp1, dv1, dq1, T + dt
        a0, w0 = a1, w1
    return np.concatenate([dp, dq, dv, [T]]), J, P


# ------------------------------------------------------------------------------------------------ R3: the factor
def residual(delta, J, ba_lin, bg_lin, pose_i, sb_i, pose_j, sb_j, g):
    """Un-whitened residual u[15] = [r_p, r_theta, r_v, r_ba, r_bg] and the intermediate values the Jacobian needs."""
    delta, J, pose_i, sb_i, pose_j, sb_j = _v(delta), _v(J), _v(pose_i), _v(sb_i), _v(pose_j), _v(sb_j)
    dba, dbg = sb_i[3:6] - _v(ba_lin), sb_i[6:9] - _v(bg_lin)
    h = J[3:6, 12:15] @ dbg / 2
    dqc = qnormalize(qmul(delta[3:7], np.concatenate([h, [LD(1)]])))
    dvc = delta[7:10] + J[6:9, 9:12] @ dba + J[6:9, 12:15] @ dbg
    dpc = delta[0:3] + J[0:3, 9:12] @ dba + J[0:3, 12:15] @ dbg
    T = delta[10]
    G = np.array([0, 0, g], dtype=LD)
    qi, qj, pi, pj, vi, vj = pose_i[:4], pose_j[:4], pose_i[4:], pose_j[4:], sb_i[:3], sb_j[:3]
    RiT = qrot(qi).T
    tp = RiT @ (G * T * T / 2 + pj - pi - vi * T)
    tv = RiT @ (G * T + vj - vi)
    e = qmul(qconj(dqc), qmul(qconj(qi), qj))
    u = np.concatenate([tp - dpc, 2 * e[:3], tv - dvc, sb_j[3:6] - sb_i[3:6], sb_j[6:9] - sb_i[6:9]])
    return u, dict(h=h, dqc=dqc, T=T, RiT=RiT, tp=tp, tv=tv, e=e, qi=qi, qj=qj)


def unwhitened(delta, J, ba_lin, bg_lin, pose_i, sb_i, pose_j, sb_j, g, fixed_i=False, fixed_j=False, exact_bg=False):
    """(u[15], A[15,30]); see the module text for exact_bg."""
    u, m = residual(delta, J, ba_lin, bg_lin, pose_i, sb_i, pose_j, sb_j, g)
    J = _v(J)
    I3 = np.eye(3, dtype=LD)
    RiT, T, e, dqc, h = m["RiT"], m["T"], m["e"], m["dqc"], m["h"]
    A = np.zeros((15, 30), LD)
    # pose_i
    A[0:3, 0:3] = skew(m["tp"])
    A[0:3, 3:6] = -RiT
    a = qmul(qconj(m["qj"]), m["qi"])
    A[3:6, 0:3] = -(L3(a) @ R3(dqc) - np.outer(a[:3], dqc[:3]))       # -(Lq(a) Rq4(b))_3x3: vector-vector block of the 4x4 product
    A[6:9, 0:3] = skew(m["tv"])
    # sb_i
    A[0:3, 6:9] = -RiT * T
    A[0:3, 9:12] = -J[0:3, 9:12]
    A[0:3, 12:15] = -J[0:3, 12:15]
    Jq = J[3:6, 12:15]
    if exact_bg:
        Jq = (I3 - skew(h)) @ Jq / (1 + h @ h)
    A[3:6, 12:15] = -L3(qconj(e)) @ Jq
    A[6:9, 6:9] = -RiT
    A[6:9, 9:12] = -J[6:9, 9:12]
    A[6:9, 12:15] = -J[6:9, 12:15]
    A[9:12, 9:12] = -I3
    A[12:15, 12:15] = -I3
    # pose_j
    A[0:3, 18:21] = RiT
    A[3:6, 15:18] = L3(e)
    # sb_j
    A[6:9, 21:24] = RiT
    A[9:12, 24:27] = I3
    A[12:15, 27:30] = I3
    if fixed_i:
        A[:, 0:6] = 0
    if fixed_j:
        A[:, 15:21] = 0
    return u, A


def chol_lower(P):
    """Lower Cholesky factor in long double, or None where a pivot is not positive."""
    P = _v(P)
    n = P.shape[0]
    C = np.zeros((n, n), LD)
    for c in range(n):
        d = P[c, c] - C[c, :c] @ C[c, :c]
        if not d > 0:
            return None
        C[c, c] = np.sqrt(d)
        for r in range(c + 1, n):
            C[r, c] = (P[r, c] - C[r, :c] @ C[c, :c]) / C[c, c]
    return C


def tri_lower_inverse(C):
    n = C.shape[0]
    W = np.zeros((n, n), LD)
    for c in range(n):
        W[c, c] = 1 / C[c, c]
        for r in range(c + 1, n):
            W[r, c] = -(C[r, c:r] @ W[c:r, c]) / C[r, r]
    return W


def whitening(P, num_samples):
    """W = chol(P)^-1 (lower). Zeros for a factor of fewer than two samples — by rule, whatever its pivots — and where P is not positive definite."""
    C = chol_lower(P) if num_samples >= 2 else None
    return np.zeros((15, 15), LD) if C is None else tri_lower_inverse(C)


def cond_chol(P):
    """cond_2 of chol(P) (two digits are all that is asked of it: taken in double from the long double factor)."""
    C = chol_lower(P)
    return float("inf") if C is None else float(np.linalg.cond(C.astype(np.float64)))


def normal_pieces(Jw, r):
    return Jw.T @ Jw, Jw.T @ r


def problem(p, options_noise=None):
    """Every factor of FlatProblem `p`, preintegrated at the bias of keyframe imu_kf_j[f] and evaluated at the problem's state: dict of long double
    arrays delta [I,11], J [I,15,15], P [I,15,15], u [I,15], A [I,15,30], W [I,15,15], r [I,15], Jw [I,15,30], JtJ [I,30,30], Jtr [I,30], and
    n [I] (samples), cond [I] (cond chol P; inf where there is no factor)."""
    I = p.I
    out = dict(delta=np.zeros((I, 11), LD), J=np.zeros((I, 15, 15), LD), P=np.zeros((I, 15, 15), LD), u=np.zeros((I, 15), LD), A=np.zeros((I, 15, 30), LD),
               W=np.zeros((I, 15, 15), LD), r=np.zeros((I, 15), LD), Jw=np.zeros((I, 15, 30), LD), JtJ=np.zeros((I, 30, 30), LD), Jtr=np.zeros((I, 30), LD),
               n=np.diff(p.imu_sample_ptr).astype(np.int64), cond=np.zeros(I))
    for f in range(I):
        i, j = int(p.imu_kf_i[f]), int(p.imu_kf_j[f])
        nz = p.imu_noise[f] if p.imu_noise is not None else options_noise
        s0, s1 = p.imu_sample_ptr[f], p.imu_sample_ptr[f + 1]
        ba, bg = p.kf_speed_bias[j, 3:6], p.kf_speed_bias[j, 6:9]
        d, J, P = preintegrate(p.imu_first[f], p.imu_samples[s0:s1], ba, bg, nz)
        u, A = unwhitened(d, J, ba, bg, p.kf_pose[i], p.kf_speed_bias[i], p.kf_pose[j], p.kf_speed_bias[j], nz[4], bool(p.kf_fixed[i]), bool(p.kf_fixed[j]))
        W = whitening(P, s1 - s0)
        r, Jw = W @ u, W @ A
        JtJ, Jtr = normal_pieces(Jw, r)
        for k, v in (("delta", d), ("J", J), ("P", P), ("u", u), ("A", A), ("W", W), ("r", r), ("Jw", Jw), ("JtJ", JtJ), ("Jtr", Jtr)):
            out[k][f] = v
        out["cond"][f] = cond_chol(P)
    return out
