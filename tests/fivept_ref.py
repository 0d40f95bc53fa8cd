"""numpy restatement of COVINS-G's five-point relative-pose RANSAC: RelNonCentralPosSolver::computePose
(RelNonCentralPosSolver.cpp:343-377) = an opengv RANSAC over 2D-2D matches with the five-point minimal solver, three more
correspondences of the draw picking the pose, scored by the reprojection of the triangulated point in both frames. It is the
checker of k_fivept.hip, so it lives with the tests.

Two host formulations of the minimal solver:
  route A  orthonormal null space (SVD), the ten cubics in graded order, the action matrix of x on the quotient ring
           (Stewenius) and numpy.linalg.eig; poses from an SVD of E. This is the checker.
  route B  what the kernel does, restated: null space by Gauss-Jordan with full pivoting and Gram-Schmidt, Nister's elimination to a degree-10
           polynomial in z, its real roots bracketed by those of its derivatives, x and y from the 3x3 polynomial matrix, three
           Gauss-Newton steps on the ten cubics; poses in closed form. It is used only to
           measure how far two correct FP64 formulations lie apart (the yardsticks s_E, s_T of tests/fivept_util.py).
Everything is plain float64 and Python integers (the sampler is bit-exact)."""
from __future__ import annotations

import math

import numpy as np

M64 = (1 << 64) - 1
EPS = np.finfo(np.float64).eps
SAMPLE = 8
DEFAULTS = dict(min_inliers=20, max_iterations=200, probability=0.99, threshold=16.0, sigma=4.5e-6)


# ------------------------------------------------------------------------------------------------ sampler
def splitmix64(x: int) -> int:
    z = (x + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw(seed: int, d: int, n: int):
    """The 8 distinct indices of draw d: a partial Fisher-Yates over [0, n), slot k swaps position k with
    k + splitmix64(seed + 8 d + k) mod (n - k)."""
    over = {}
    out = []
    for k in range(SAMPLE):
        x = splitmix64((seed + SAMPLE * d + k) & M64)
        j = k + x % (n - k)
        vk, vj = over.get(k, k), over.get(j, j)
        over[j] = vk
        out.append(vj)
    return out


# ------------------------------------------------------------------------------------------------ model and score
def triangulate(R, t, f1, f2):
    """opengv triangulate2 restated, vectorised over the rows of f1, f2: the midpoint of the two rays, in frame 1."""
    g = f2 @ R.T
    b0, b1 = f1 @ t, g @ t
    a00, a01, a11 = np.sum(f1 * f1, 1), -np.sum(f1 * g, 1), -np.sum(g * g, 1)
    det = a00 * a11 + a01 * a01                      # A = [[a00, a01], [-a01, a11]]
    with np.errstate(all="ignore"):
        l0 = (a11 * b0 - a01 * b1) / det
        l1 = (a01 * b0 + a00 * b1) / det
    return (l0[:, None] * f1 + t + l1[:, None] * g) / 2.0


def reproject(R, t, f1, f2):
    p = triangulate(R, t, f1, f2)
    q = (p - t) @ R                                  # R^T p - R^T t
    with np.errstate(all="ignore"):
        r1 = p / np.linalg.norm(p, axis=1, keepdims=True)
        r2 = q / np.linalg.norm(q, axis=1, keepdims=True)
    return r1, r2


def score(R, t, f1, f2, sigma):
    r1, r2 = reproject(R, t, f1, f2)
    e1, e2 = r1 - f1, r2 - f2
    return 0.5 * np.sum(e1 * e1, 1) / sigma + 0.5 * np.sum(e2 * e2, 1) / sigma


def inlier_mask(R, t, f1, f2, sigma, threshold):
    with np.errstate(all="ignore"):
        return score(R, t, f1, f2, sigma) < threshold   # a non-finite score compares false


def selection_sum(R, t, f1, f2):
    r1, r2 = reproject(R, t, f1, f2)
    return float(np.sum((1.0 - np.sum(f1 * r1, 1)) + (1.0 - np.sum(f2 * r2, 1))))


# ------------------------------------------------------------------------------------------------ the ten cubics
def _mono_table(order):
    """[64, 20] 0/1 matrix taking the coefficient of c_a c_b c_c (c = x, y, z, 1) to its monomial in `order`."""
    unit = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]
    S = np.zeros((64, 20))
    for a in range(4):
        for b in range(4):
            for c in range(4):
                e = tuple(unit[a][i] + unit[b][i] + unit[c][i] for i in range(3))
                S[16 * a + 4 * b + c, order.index(e)] = 1.0
    return S


# graded order: the ten cubic monomials, then the basis of the quotient ring x2 xy xz y2 yz z2 x y z 1
ORDER_A = [(3, 0, 0), (2, 1, 0), (2, 0, 1), (1, 2, 0), (1, 1, 1), (1, 0, 2), (0, 3, 0), (0, 2, 1), (0, 1, 2), (0, 0, 3),
           (2, 0, 0), (1, 1, 0), (1, 0, 1), (0, 2, 0), (0, 1, 1), (0, 0, 2), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]
# Nister's order: x3 y3 x2y xy2 x2z x2 y2z y2 xyz xy | xz2 xz x yz2 yz y z3 z2 z 1
ORDER_B = [(3, 0, 0), (0, 3, 0), (2, 1, 0), (1, 2, 0), (2, 0, 1), (2, 0, 0), (0, 2, 1), (0, 2, 0), (1, 1, 1), (1, 1, 0),
           (1, 0, 2), (1, 0, 1), (1, 0, 0), (0, 1, 2), (0, 1, 1), (0, 1, 0), (0, 0, 3), (0, 0, 2), (0, 0, 1), (0, 0, 0)]
_S_A, _S_B = _mono_table(ORDER_A), _mono_table(ORDER_B)
_EPS3 = np.zeros((3, 3, 3))
for _i, _j, _k in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
    _EPS3[_i, _j, _k] = 1.0
    _EPS3[_i, _k, _j] = -1.0


def constraints(N, S):
    """[10, 20] coefficients of 2 E E^T E - tr(E E^T) E (9 rows, row-major) and det E (row 9) for E = x N0 + y N1 + z N2 + N3."""
    G = np.einsum("aik,blk,clj->abcij", N, N, N)
    T = np.einsum("akl,bkl,cij->abcij", N, N, N)
    K = (2.0 * G - T).reshape(64, 9)
    D = np.einsum("ijk,ai,bj,ck->abc", _EPS3, N[:, 0, :], N[:, 1, :], N[:, 2, :]).reshape(64, 1)
    return np.concatenate([K, D], axis=1).T @ S


def cubic_residual(E):
    """Largest absolute value of the ten cubics at E (scaled to ||E||_F = sqrt 2 by the caller)."""
    EEt = E @ E.T
    return max(float(np.max(np.abs(2.0 * EEt @ E - np.trace(EEt) * E))), abs(float(np.linalg.det(E))))


def epipolar_residual(E, f1, f2):
    return float(np.max(np.abs(np.einsum("ki,ij,kj->k", f1[:5], E, f2[:5]))))


def epipolar_rows(f1, f2):
    """[5, 9]: row k is f1_k (x) f2_k, so that row . vec(E) = f1^T E f2 (E row-major)."""
    return (f1[:5, :, None] * f2[:5, None, :]).reshape(5, 9)


def normalise_E(E):
    """||E||_F = sqrt 2, the largest-magnitude entry positive."""
    E = E * (math.sqrt(2.0) / np.linalg.norm(E))
    k = int(np.argmax(np.abs(E)))
    return -E if E.ravel()[k] < 0 else E


# ------------------------------------------------------------------------------------------------ route A
REAL_TOL = 1e-8     # a solution counts as real when no coordinate of (x, y, z) has |imag| above this (relative to max(1, |.|))


def solve_A(f1, f2, detail=False):
    """Every real essential matrix of correspondences 0..4 (list of 3x3, ||E||_F = sqrt 2). With detail: also the real (x, y, z)
    and all ten complex (x, y, z) in the SVD basis. A rank-deficient sample has no solution."""
    none = ([], np.zeros((0, 3)), np.zeros((0, 3), complex)) if detail else []
    Q = epipolar_rows(f1, f2)
    if not np.all(np.isfinite(Q)):
        return none
    _, s, Vt = np.linalg.svd(Q)
    if not (s[4] > 1e-12 * s[0]):
        return none
    N = Vt[5:].reshape(4, 3, 3)
    M = constraints(N, _S_A)
    try:
        Bm = np.linalg.solve(M[:, :10], M[:, 10:])
    except np.linalg.LinAlgError:
        return none
    if not np.all(np.isfinite(Bm)):
        return none
    Ax = np.zeros((10, 10))
    Ax[:6] = -Bm[:6]
    Ax[6, 0] = Ax[7, 1] = Ax[8, 2] = Ax[9, 6] = 1.0
    _, V = np.linalg.eig(Ax)
    with np.errstate(all="ignore"):
        xyz = (V[6:9] / V[9]).T                      # [10, 3] complex
    Es, real = [], []
    for v in xyz:
        if not np.all(np.isfinite(v)):
            continue
        if np.max(np.abs(v.imag)) > REAL_TOL * max(1.0, float(np.max(np.abs(v.real)))):
            continue
        x, y, z = v.real
        E = x * N[0] + y * N[1] + z * N[2] + N[3]
        if np.all(np.isfinite(E)) and np.linalg.norm(E) > 0:
            Es.append(normalise_E(E))
            real.append(v.real)
    if detail:
        return Es, np.array(real).reshape(-1, 3), xyz
    return Es


def separated(real, xyz):
    """The issue's rule: route A's real solutions pairwise >= 1e-2 apart in (x, y, z), no complex root with |imag| < 1e-2."""
    if len(real) == 0 or not np.all(np.isfinite(xyz)):
        return False
    for i in range(len(real)):
        for j in range(i + 1, len(real)):
            if np.linalg.norm(real[i] - real[j]) < 1e-2:
                return False
    for v in xyz:
        im = float(np.max(np.abs(v.imag)))
        if REAL_TOL * max(1.0, float(np.max(np.abs(v.real)))) < im < 1e-2:
            return False
    return True


def decompose_svd(E):
    """The four poses of E from its SVD: {U W V^T, U W^T V^T} x {u3, -u3}, rotations with det +1."""
    U, _, Vt = np.linalg.svd(E)
    if np.linalg.det(U) < 0:
        U = -U
    if np.linalg.det(Vt) < 0:
        Vt = -Vt
    W = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    t = U[:, 2]
    return [(U @ W @ Vt, t), (U @ W @ Vt, -t), (U @ W.T @ Vt, t), (U @ W.T @ Vt, -t)]


def _skew(t):
    return np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])


def decompose_closed(E):
    """The four poses in closed form: t the left null direction of E (the largest cross product of two columns), E scaled to
    ||t|| = 1 (||E||_F = sqrt 2), R = cof(E) -+ [t]x E with cof(E) the matrix of cofactors."""
    c = [np.cross(E[:, 0], E[:, 1]), np.cross(E[:, 0], E[:, 2]), np.cross(E[:, 1], E[:, 2])]
    k = int(np.argmax([v @ v for v in c]))
    t = c[k] / np.linalg.norm(c[k])
    E = E * (math.sqrt(2.0) / np.linalg.norm(E))
    cof = np.array([np.cross(E[1], E[2]), np.cross(E[2], E[0]), np.cross(E[0], E[1])])
    tE = _skew(t) @ E
    Ra, Rb = cof - tE, cof + tE
    return [(Ra, t), (Ra, -t), (Rb, t), (Rb, -t)]


def choose(Es, f1, f2, decompose=decompose_svd, sums=None):
    """The pose of the draw: the smallest selection sum over its 8 correspondences among the four poses of every E; a
    non-finite sum is skipped, the first wins a tie. Returns (index of E or -1, R, t). `sums` (a list) receives every finite sum."""
    best, bi, bR, bt = math.inf, -1, None, None
    for i, E in enumerate(Es):
        for R, t in decompose(E):
            s = selection_sum(R, t, f1, f2)
            if not math.isfinite(s):
                continue
            if sums is not None:
                sums.append(s)
            if s < best:
                best, bi, bR, bt = s, i, R, t
    return bi, bR, bt


# ------------------------------------------------------------------------------------------------ route B
def _nullspace_gj(Q):
    """An orthonormal basis of the null space of the 5x9 Q: Gauss-Jordan with full pivoting, then Gram-Schmidt; None where a
    pivot vanishes."""
    A = Q.copy()
    cols = list(range(9))
    scale = float(np.max(np.abs(A)))
    for c in range(5):
        sub = np.abs(A[c:, c:])
        r, k = np.unravel_index(int(np.argmax(sub)), sub.shape)
        if not (sub[r, k] > 1e-12 * scale):
            return None
        A[[c, c + r]] = A[[c + r, c]]
        A[:, [c, c + k]] = A[:, [c + k, c]]
        cols[c], cols[c + k] = cols[c + k], cols[c]
        A[c] /= A[c, c]
        for i in range(5):
            if i != c:
                A[i] -= A[i, c] * A[c]
    N = np.zeros((4, 9))
    for m in range(4):
        N[m, cols[5 + m]] = 1.0
        for c in range(5):
            N[m, cols[c]] = -A[c, 5 + m]
    for m in range(4):                               # modified Gram-Schmidt, twice: E's coordinates then do not depend on scale
        for _ in range(2):
            for k in range(m):
                N[m] -= (N[m] @ N[k]) * N[k]
        N[m] /= np.linalg.norm(N[m])
    return N


def nister_poly(Bm):
    """The 3x3 polynomial matrix C(z) [x, y, 1]^T = 0 from rows 4..9 of the reduced system (right-hand 10 columns Bm[6, 10]:
    xz2 xz x yz2 yz y z3 z2 z 1) and its determinant, degree 10, highest power first."""
    rows = []
    for e, f in ((0, 1), (2, 3), (4, 5)):            # <e> - z <f>: rows of x2z & x2, y2z & y2, xyz & xy
        cx = np.array([-Bm[f, 0], Bm[e, 0] - Bm[f, 1], Bm[e, 1] - Bm[f, 2], Bm[e, 2]])
        cy = np.array([-Bm[f, 3], Bm[e, 3] - Bm[f, 4], Bm[e, 4] - Bm[f, 5], Bm[e, 5]])
        c1 = np.array([-Bm[f, 6], Bm[e, 6] - Bm[f, 7], Bm[e, 7] - Bm[f, 8], Bm[e, 8] - Bm[f, 9], Bm[e, 9]])
        rows.append((cx, cy, c1))
    pm = np.polymul
    m01 = np.polysub(pm(rows[1][0], rows[2][1]), pm(rows[1][1], rows[2][0]))
    m02 = np.polysub(pm(rows[0][0], rows[2][1]), pm(rows[0][1], rows[2][0]))
    m03 = np.polysub(pm(rows[0][0], rows[1][1]), pm(rows[0][1], rows[1][0]))
    det = np.polyadd(np.polysub(pm(m01, rows[0][2]), pm(m02, rows[1][2])), pm(m03, rows[2][2]))
    det = np.concatenate([np.zeros(11 - len(det)), det])
    return rows, det


def polish(N, v, steps=3):
    """Gauss-Newton in (x, y, z) on the ten cubics evaluated at E = x N0 + y N1 + z N2 + N3 itself, so that what the elimination
    lost does not stay in the solution."""
    for _ in range(steps):
        E = v[0] * N[0] + v[1] * N[1] + v[2] * N[2] + N[3]
        G = E @ E.T
        tr = np.trace(G)
        cof = np.array([np.cross(E[1], E[2]), np.cross(E[2], E[0]), np.cross(E[0], E[1])])
        r = np.concatenate([(2.0 * G @ E - tr * E).ravel(), [E[0] @ cof[0]]])
        J = np.zeros((10, 3))
        for a in range(3):
            dE = N[a]
            K = dE @ E.T
            J[:9, a] = (2.0 * ((K + K.T) @ E + G @ dE) - 2.0 * np.trace(K) * E - tr * dE).ravel()
            J[9, a] = np.sum(cof * dE)
        H, g = J.T @ J, J.T @ r
        det = np.linalg.det(H)
        if not (det != 0.0 and math.isfinite(det)):
            break
        step = np.linalg.solve(H, g)
        if not np.all(np.isfinite(step)):
            break
        v = v - step
    return v


_SIGN = np.uint64(1 << 63)


def _key(x):
    """Doubles to unsigned integers in the same order (the bit pattern, negative values reflected): halving a bracket in this
    key reaches neighbouring doubles in 64 steps whatever the magnitudes, where the arithmetic mean would need a thousand."""
    b = np.asarray(x, dtype=np.float64).view(np.uint64)
    return np.where(b & _SIGN, ~b, b | _SIGN)


def _unkey(k):
    k = np.asarray(k, dtype=np.uint64)
    return np.where(k & _SIGN, k & ~_SIGN, ~k).view(np.float64)


def bracket_roots(a, steps=64):
    """Real roots of the polynomial a (highest power first), ascending: the roots of each derivative bracket those of the one
    below it (Rolle), every bracket with a sign change is halved `steps` times in the ordered bit patterns of its ends. Roots of even multiplicity are not found.
    (numpy.roots on the same coefficients turns real roots 1e-2 apart into complex pairs on one tuple in a hundred.)"""
    a = np.asarray(a, dtype=np.float64)
    n = len(a) - 1
    if not np.all(np.isfinite(a)) or a[0] == 0.0:
        return []
    bound = 1.0 + float(np.max(np.abs(a[1:] / a[0])))   # Cauchy; the derivatives' roots lie in the hull of the roots (Gauss-Lucas)
    if not math.isfinite(bound):
        return []
    c = a[::-1]
    roots = np.zeros(0)
    for d in range(1, n + 1):
        m = n - d
        D = np.array([c[j + m] * math.comb(j + m, m) for j in range(d, -1, -1)])   # p^(m) / m!
        ends = np.concatenate([[-bound], roots, [bound]])
        lo, hi = ends[:-1].copy(), ends[1:].copy()
        neg = np.polyval(D, lo) < 0
        keep = neg != (np.polyval(D, hi) < 0)
        lo, hi, neg = lo[keep], hi[keep], neg[keep]
        lo, hi = _key(lo), _key(hi)
        for _ in range(steps):
            mid = lo + ((hi - lo) >> np.uint64(1))
            same = (np.polyval(D, _unkey(mid)) < 0) == neg
            lo = np.where(same, mid, lo)
            hi = np.where(same, hi, mid)
        roots = _unkey(lo)
    return list(roots)


DEDUP = 1e-6    # two candidates whose E (||E||_F = sqrt 2, up to sign) agree to this in every entry are one solution


def _nister_round(N):
    """The candidates of one elimination with N[2]'s coordinate as the hidden variable: list of E (||E||_F = sqrt 2)."""
    M = constraints(N, _S_B)
    with np.errstate(all="ignore"):
        try:
            Bm = np.linalg.solve(M[:, :10], M[:, 10:])
        except np.linalg.LinAlgError:
            return []
    if not np.all(np.isfinite(Bm)):
        return []
    rows, det = nister_poly(Bm[4:])
    Es = []
    for z in bracket_roots(det):
        Cz = np.array([[np.polyval(c, z) for c in row] for row in rows])
        cr = [np.cross(Cz[0], Cz[1]), np.cross(Cz[0], Cz[2]), np.cross(Cz[1], Cz[2])]
        v = cr[int(np.argmax([abs(c[2]) for c in cr]))]
        if v[2] == 0.0:
            continue
        x, y, z = polish(N, np.array([v[0] / v[2], v[1] / v[2], z]))
        E = x * N[0] + y * N[1] + z * N[2] + N[3]
        if np.all(np.isfinite(E)) and np.linalg.norm(E) > 0:
            E = normalise_E(E)
            if cubic_residual(E) <= CUBIC_GATE:
                Es.append(E)
    return Es


CUBIC_GATE = 1e-9   # an E (||E||_F = sqrt 2) whose cubics exceed this after the polish is not a solution


def solve_B(f1, f2):
    """Route B: every real essential matrix of correspondences 0..4 by Nister's elimination and bracketed real roots. Solutions
    that lie close in the hidden variable merge in the polynomial, so the elimination runs three times, with z, x and y hidden
    (the basis vectors rotated), and a candidate joins the solutions unless it repeats one."""
    Q = epipolar_rows(f1, f2)
    if not np.all(np.isfinite(Q)):
        return []
    Nv = _nullspace_gj(Q)
    if Nv is None:
        return []
    N = Nv.reshape(4, 3, 3)
    Es = []
    for _ in range(3):
        for E in _nister_round(N):
            if all(np.max(np.abs(E - F)) > DEDUP for F in Es):
                Es.append(E)
        N = N[[1, 2, 0, 3]]
    return Es[:10]


# ------------------------------------------------------------------------------------------------ comparing solutions
def match_sets(Ea, Eb):
    """Largest entry-wise difference between two solution sets matched by the nearest E (inf where the counts differ)."""
    if len(Ea) != len(Eb):
        return math.inf
    worst, left = 0.0, list(range(len(Eb)))
    for E in Ea:
        d = [float(np.max(np.abs(E - Eb[j]))) for j in left]
        k = int(np.argmin(d))
        worst = max(worst, d[k])
        left.pop(k)
    return worst


def pose_error(Ra, ta, Rb, tb):
    """(rotation angle between Ra and Rb, angle between the translation directions), radians."""
    c = 0.5 * (np.trace(Ra.T @ Rb) - 1.0)
    ct = float(ta @ tb) / (np.linalg.norm(ta) * np.linalg.norm(tb))
    # small angles from the sine side: acos loses half the digits near 1
    sr = np.linalg.norm(Ra.T @ Rb - Rb.T @ Ra) / (2.0 * math.sqrt(2.0))
    st = np.linalg.norm(np.cross(ta, tb)) / (np.linalg.norm(ta) * np.linalg.norm(tb))
    return (math.atan2(sr, c), math.atan2(st, ct))


def rot_to_quat(R):
    """Hamilton quaternion x, y, z, w of a rotation matrix (w >= 0)."""
    from scipy.spatial.transform import Rotation
    q = Rotation.from_matrix(R).as_quat()
    return -q if q[3] < 0 else q


def quat_to_rot(q):
    from scipy.spatial.transform import Rotation
    return Rotation.from_quat(q).as_matrix()


# ------------------------------------------------------------------------------------------------ RANSAC loop
def hypothesis_A(f1, f2, sums=None):
    """The model of one draw (its 8 correspondences in slot order) by route A, or None for a failed draw."""
    Es = solve_A(f1, f2)
    i, R, t = choose(Es, f1, f2, sums=sums)
    return None if i < 0 else (R, t)


def ransac(f1, f2, seed, threshold=16.0, max_iterations=200, probability=0.99, min_inliers=20, sigma=4.5e-6, hypothesis=None,
           trace=None):
    """opengv sac::Ransac::computeModel restated with sample size 8 and the sampler above. Returns dict(status, inliers (the best
    model's count), mask [n] bool (all False unless status 0), R, t (the best model, None if none), iterations, best_draw (-1:
    none), draws). `hypothesis(d, idx) -> (R, t) | None` replaces the solver (hand-built loop tests); `trace` (a list)
    receives per draw the finite selection sums of route A."""
    n = len(f1)
    out = dict(status=1, inliers=0, mask=np.zeros(n, bool), R=None, t=None, iterations=0, best_draw=-1, draws=0)
    if n < SAMPLE:
        return out
    it, skipped, k, best = 0, 0, 1.0, -(1 << 31)
    bR = bt = None
    d = 0
    while it < k and skipped < 10 * max_iterations:
        idx = draw(seed, d, n)
        if hypothesis is not None:
            h = hypothesis(d, idx)
        else:
            sums = [] if trace is not None else None
            h = hypothesis_A(f1[idx], f2[idx], sums)
            if trace is not None:
                trace.append(sums)
        d += 1
        if h is None:
            skipped += 1
            continue
        cnt = int(np.sum(inlier_mask(h[0], h[1], f1, f2, sigma, threshold)))
        if cnt > best:
            best = cnt
            bR, bt = h
            out["best_draw"] = d - 1
            w = best / n
            pno = 1.0 - w ** 8.0
            pno = min(max(pno, EPS), 1.0 - EPS)
            k = math.log(1.0 - probability) / math.log(pno)
        it += 1
        if it > max_iterations:
            break
    out["iterations"], out["draws"] = it, d
    if bR is None:
        out["status"] = 2
        return out
    mask = inlier_mask(bR, bt, f1, f2, sigma, threshold)
    out.update(inliers=int(mask.sum()), R=bR, t=bt)
    if out["inliers"] < min_inliers:
        out["status"] = 3
    elif it >= max_iterations:
        out["status"] = 4
    else:
        out["status"] = 0
        out["mask"] = mask
    return out


def ransac_batch(bt, seeds, **opts):
    """ransac() per job of a batch dict (ptr, bearing1, bearing2): list of results."""
    ptr = bt["ptr"]
    res = []
    for b in range(len(ptr) - 1):
        s = slice(int(ptr[b]), int(ptr[b + 1]))
        res.append(ransac(bt["bearing1"][s], bt["bearing2"][s], int(seeds[b]), **opts))
    return res
