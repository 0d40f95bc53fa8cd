"""The observation covariance restated in numpy (Context.observation_covariances): three host routes to the 2x2 block
C_o = J_o Sigma J_o^T and to the pose-landmark cross block Sigma_al of every observation o = (a, l), all from the oracle's linearisation and its
reduced camera system (tests/lmcov_ref.Linearisation, with the per-observation Jacobians kept here). Nothing of the device code.

  route A  the block formulas on the dense Sigma_pp = S^-1:  Sigma_al = -sum_b Sigma_ab W_b H_ll^-1 over the free observers b of l, Sigma_l as
           lmcov_ref.route_a, Sigma_aa read out; C_o = J_p Sigma_aa J_p^T + J_p Sigma_al J_l^T + (its transpose) + J_l Sigma_l J_l^T
  route B  no Schur identity: the dense inverse of the full system built as lmcov_ref.route_b builds it ((n + 3 m)^2 with the m landmarks of
           `sample` put back as unknowns, or all of them), Sigma_aa, Sigma_al and Sigma_l read straight out of it
  route C  the kernel's formula: with R = chol(H_ll^-1), Z = W R, V_a = sum_b Sigma_ab Z_b, M = sum_a Z_a^T V_a, Y = J_l R
           Sigma_al = -V_a R^T,  C_o = [J_p -Y] [[Sigma_aa, V_a], [V_a^T, (M + M^T) / 2]] [J_p -Y]^T + Y Y^T

An observer with a constant pose has J_p = 0 and no rows in Sigma: its cross block is zeros. Every route returns, per observation, the block
C [O, 2, 2], the cross block X [O, 6, 3] and the diagonals of Sigma_aa [O, 6] and Sigma_l [O, 3] (for the correlation scaling of X, whose rows mix
radians and metres); route C also the blocks Sigma_aa and Sigma_l themselves. Rows of observations a route does not cover stay zero.
"""
import numpy as np
import scipy.linalg as sl

from oracle import covo
from tests import lmcov_ref as lr


class ObsLinearisation(lr.Linearisation):
    """lmcov_ref.Linearisation with Jp [O, 2, 6], Jl [O, 2, 3] and r [O, 2] kept per observation (Jp of a constant observer zeroed)."""

    def __init__(self, prob, visual_only, mu, unified=False):
        super().__init__(prob, visual_only, mu, unified=unified)
        if unified:
            from tests.test_omni_host import linearize_ref
            r, Jp, Jl, c = linearize_ref(prob, loss_a=1.0)
        else:
            r, Jp, Jl, c = covo.linearize_reprojection(prob, covo.default_options(visual_only=1 if visual_only else 0))
        O = prob.O
        self.r = np.asarray(r, np.float64).reshape(O, 2)
        self.Jp = np.array(Jp, np.float64).reshape(O, 2, 6)
        self.Jl = np.asarray(Jl, np.float64).reshape(O, 2, 3)
        self.Jp[~self.free_obs] = 0.0
        self.kf_of = np.asarray(prob.obs_kf, np.int64)

    def obs_of(self, landmarks=None):
        ls = range(self.prob.L) if landmarks is None else landmarks
        return np.concatenate([np.arange(self.ptr[l], self.ptr[l + 1]) for l in ls if self.ok[l]] + [np.zeros(0, np.int64)]).astype(np.int64)


def _blank(lin):
    O = lin.prob.O
    return dict(C=np.zeros((O, 2, 2)), X=np.zeros((O, 6, 3)), daa=np.zeros((O, 6)), dl=np.zeros((O, 3)), Saa=np.zeros((O, 6, 6)), Sl=np.zeros((O, 3, 3)))


def _assemble(lin, o, Saa, X, Sl):
    Jp, Jl = lin.Jp[o], lin.Jl[o]
    cx = Jp @ X @ Jl.T
    return Jp @ Saa @ Jp.T + cx + cx.T + Jl @ Sl @ Jl.T


def route_a(lin, landmarks=None):
    out = _blank(lin)
    for l in (range(lin.prob.L) if landmarks is None else landmarks):
        if not lin.ok[l]:
            continue
        of, rows = lin.observers(l)
        Hi = lin.Hinv[l]
        Sl, G, Sll = Hi, None, None
        if len(of):
            idx = rows.reshape(-1)
            Wl = lin.W[of].reshape(-1, 3)
            Sll = lin.Sig[np.ix_(idx, idx)]
            G = Sll @ Wl @ Hi                                  # [6 m, 3]: -Sigma_al stacked over the free observers
            Sl = Hi + Hi @ (Wl.T @ Sll @ Wl) @ Hi
        where = {int(o): t for t, o in enumerate(of)}
        for o in range(lin.ptr[l], lin.ptr[l + 1]):
            t = where.get(int(o))
            Saa = Sll[6 * t:6 * t + 6, 6 * t:6 * t + 6] if t is not None else np.zeros((6, 6))
            X = -G[6 * t:6 * t + 6] if t is not None else np.zeros((6, 3))
            out["C"][o] = _assemble(lin, o, Saa, X, Sl); out["X"][o] = X; out["daa"][o] = np.diag(Saa); out["dl"][o] = np.diag(Sl)
    return out


def route_c(lin, landmarks=None):
    out = _blank(lin)
    for l in (range(lin.prob.L) if landmarks is None else landmarks):
        if not lin.ok[l]:
            continue
        of, rows = lin.observers(l)
        R = lin.R[l]
        Z = lin.W[of] @ R
        V = np.zeros((len(of), 6, 3)); M = np.zeros((3, 3))
        for a in range(len(of)):
            for b in range(len(of)):
                V[a] += lin.Sig[np.ix_(rows[a], rows[b])] @ Z[b]
            M += Z[a].T @ V[a]
        Ms = 0.5 * (M + M.T)
        where = {int(o): t for t, o in enumerate(of)}
        for o in range(lin.ptr[l], lin.ptr[l + 1]):
            t = where.get(int(o))
            Saa = lin.Sig[np.ix_(rows[t], rows[t])] if t is not None else np.zeros((6, 6))
            Va = V[t] if t is not None else np.zeros((6, 3))
            Y = lin.Jl[o] @ R
            u = np.hstack([lin.Jp[o], -Y])
            Q = np.block([[Saa, Va], [Va.T, Ms]])
            out["C"][o] = u @ Q @ u.T + Y @ Y.T
            out["X"][o] = -Va @ R.T
            out["Saa"][o] = Saa; out["Sl"][o] = R @ (np.eye(3) + Ms) @ R.T
            out["daa"][o] = np.diag(Saa); out["dl"][o] = np.diag(out["Sl"][o])
    return out


def route_b(lin, sample=None):
    """sample None: every landmark is an unknown of the matrix; else only those (the others stay eliminated inside S, and their observations'
    rows stay zero here)."""
    L = lin.prob.L
    good = np.flatnonzero(lin.ok) if sample is None else np.array([l for l in sample if lin.ok[l]], np.int64)
    n, Hpp = lr._full_blocks(lin, None if sample is None else good)
    col = -np.ones(L, np.int64); col[good] = n + 3 * np.arange(len(good))
    N = n + 3 * len(good)
    F = np.zeros((N, N), order="F")
    F[:n, :n] = Hpp
    for l in good:
        c = col[l]
        F[c:c + 3, c:c + 3] = lin.H[l]
        of, rows = lin.observers(l)
        for t in range(len(of)):
            F[rows[t], c:c + 3] = lin.W[of[t]]; F[c:c + 3, rows[t]] = lin.W[of[t]].T
    c_, info = sl.lapack.dpotrf(F, lower=1, overwrite_a=1)
    assert info == 0, f"the full system is not positive definite (potrf info {info})"
    inv, info = sl.lapack.dpotri(c_, lower=1, overwrite_c=1)
    assert info == 0

    def sym(i):     # a diagonal block through its lower triangle
        b = np.tril(inv[np.ix_(i, i)])
        return b + np.tril(b, -1).T

    out = _blank(lin)
    for l in good:
        cl = np.arange(col[l], col[l] + 3)
        Sl = sym(cl)
        of, rows = lin.observers(l)
        where = {int(o): t for t, o in enumerate(of)}
        for o in range(lin.ptr[l], lin.ptr[l + 1]):
            t = where.get(int(o))
            Saa = sym(rows[t]) if t is not None else np.zeros((6, 6))
            X = inv[np.ix_(cl, rows[t])].T if t is not None else np.zeros((6, 3))   # (landmark rows lie below the pose rows: the lower triangle)
            out["C"][o] = _assemble(lin, o, Saa, X, Sl); out["X"][o] = X; out["daa"][o] = np.diag(Saa); out["dl"][o] = np.diag(Sl)
    return out


def err_block(A, B, A_ref):
    """max |A - B| / max |A_routeA| per observation, for stacks [m, 2, 2] (an all-zero reference block: the absolute difference)."""
    den = np.abs(A_ref).reshape(len(A_ref), -1).max(axis=1)
    num = np.abs(A - B).reshape(len(A), -1).max(axis=1)
    return num / np.where(den > 0, den, 1.0)


def err_cross(XA, XB, refA, rows):
    """max |corr(XA) - corr(XB)| per observation of `rows`: entries scaled by 1 / sqrt of route A's diagonals of Sigma_aa and Sigma_l (a zero
    diagonal — a constant observer, whose block is zeros — scales by 1)."""
    da, dl = refA["daa"][rows], refA["dl"][rows]
    sc = np.sqrt(np.where(da > 0, da, 1.0))[:, :, None] * np.sqrt(np.where(dl > 0, dl, 1.0))[:, None, :]
    return (np.abs(XA[rows] - XB[rows]) / sc).reshape(len(rows), -1).max(axis=1)
