"""The landmark covariance restated in numpy (Context.landmark_covariances): three host routes to the 3x3 diagonal block, at
every landmark, of the inverse of the whole damped system, all from the oracle's linearisation and its reduced camera system. Nothing of the
device code.

With J_p (2x6), J_l (2x3) the loss-corrected Jacobians of an observation (covo.linearize_reprojection), W_o = J_p^T J_l, H_ll = sum J_l^T J_l
plus the damping of covo_dense_step (mu clampd(H_ll,rr)^2 on the diagonal) and S = covo.schur(prob, opt, mu):

  route A  the block formula   Sigma_l = H_ll^-1 + H_ll^-1 (sum over a, b of W_a^T Sigma_ab W_b) H_ll^-1, Sigma_ab the pose rows of the dense
           inverse of S, a and b over the observers with a free pose (a constant pose has identity rows in S and no covariance)
  route B  no Schur identity   the full (n + 3 L)^2 matrix [[H_pp, H_pl], [H_lp, H_ll]] with H_pp = S + sum_l W H_ll^-1 W^T, inverted by dense
           Cholesky (LAPACK potrf + potri), landmark diagonal blocks read out. Where the full matrix is too large to hold (`sample`), only
           the sampled landmarks are put back as unknowns: (n + 3 m)^2, H_pp = S + the sum over the sample; the others stay inside S
  route C  the kernel's formula   R (I + sum Z_a^T Sigma_ab Z_b) R^T with R = chol(H_ll^-1) and Z_a = W_a R, Sigma_ab as in route A

Metric per landmark: max |A - B| / max |A_routeA|. A landmark whose damped H_ll has no Cholesky factor is degenerate: no route serves it.
"""
import numpy as np
import scipy.linalg as sl

from oracle import covo


def clampd(h):
    return np.clip(np.sqrt(np.maximum(h, 0.0)), 1e-6, 1e32)


def spd_inverse(A):
    """Inverse of the symmetric positive definite A by dense Cholesky, both triangles filled. Overwrites a copy."""
    c, info = sl.lapack.dpotrf(np.array(A, order="F"), lower=1, overwrite_a=1)
    assert info == 0, f"not positive definite (potrf info {info})"
    inv, info = sl.lapack.dpotri(c, lower=1, overwrite_c=1)
    assert info == 0
    inv = np.tril(inv)
    return inv + np.tril(inv, -1).T


class Linearisation:
    """What all routes share: W [O, 6, 3], the damped H_ll [L, 3, 3] and its inverse, which landmarks are degenerate, S and Sigma = S^-1."""

    def __init__(self, prob, visual_only, mu, unified=False):
        """unified: a visual-only problem with unified cameras, which the oracle does not model — the linearisation and S come from the
        numpy restatement (tests/test_omni_host.linearize_ref, tests/lm_forms_util.NumpySystem) instead."""
        self.prob, self.vo, self.mu = prob, bool(visual_only), float(mu)
        self.D = 6 if visual_only else 15
        opt = covo.default_options(visual_only=1 if visual_only else 0)
        if unified:
            assert visual_only
            from tests.test_omni_host import linearize_ref
            r, Jp, Jl, c = linearize_ref(prob, loss_a=1.0)
        else:
            r, Jp, Jl, c = covo.linearize_reprojection(prob, opt)
        O, L = prob.O, prob.L
        Jp, Jl = Jp.reshape(O, 2, 6), Jl.reshape(O, 2, 3)
        self.W = np.einsum("oki,okj->oij", Jp, Jl)
        self.ptr = np.asarray(prob.lm_obs_ptr, np.int64)
        self.lm_of = np.repeat(np.arange(L), np.diff(self.ptr))
        H = np.zeros((L, 3, 3))
        np.add.at(H, self.lm_of, np.einsum("oki,okj->oij", Jl, Jl))
        self.H0 = H.copy()
        for q in range(3):
            H[:, q, q] += mu * clampd(H[:, q, q]) ** 2
        self.H = H
        self.ok = np.zeros(L, bool)
        self.Hinv = np.zeros((L, 3, 3)); self.R = np.zeros((L, 3, 3))
        for l in range(L):
            try:
                np.linalg.cholesky(H[l])
                self.Hinv[l] = np.linalg.inv(H[l]); self.Hinv[l] = 0.5 * (self.Hinv[l] + self.Hinv[l].T)
                self.R[l] = np.linalg.cholesky(self.Hinv[l])
                self.ok[l] = True
            except np.linalg.LinAlgError:
                pass
        self.free_obs = np.asarray(prob.kf_fixed)[prob.obs_kf] == 0
        if unified:
            from tests.lm_forms_util import NumpySystem
            self.S = NumpySystem(prob).schur(mu)[0]
        else:
            self.S = covo.schur(prob, opt, mu)[0]
        self._Sig = None

    @property
    def Sig(self):
        if self._Sig is None:
            self._Sig = spd_inverse(self.S)
        return self._Sig

    def observers(self, l):
        """(observation rows, solution indices of their pose rows [m, 6]) of the free observers of landmark l, in landmark order."""
        o = np.arange(self.ptr[l], self.ptr[l + 1])
        o = o[self.free_obs[o]]
        return o, self.D * np.asarray(self.prob.obs_kf)[o][:, None] + np.arange(6)[None, :]


def route_a(lin, landmarks=None):
    out = np.zeros((lin.prob.L, 3, 3))
    for l in (range(lin.prob.L) if landmarks is None else landmarks):
        if not lin.ok[l]:
            continue
        o, rows = lin.observers(l)
        Hi = lin.Hinv[l]
        if len(o):
            idx = rows.reshape(-1)
            Wl = lin.W[o].reshape(-1, 3)                      # H_pl of this landmark on its observers' pose rows
            out[l] = Hi + Hi @ (Wl.T @ lin.Sig[np.ix_(idx, idx)] @ Wl) @ Hi
        else:
            out[l] = Hi
    return out


def route_c(lin, landmarks=None):
    out = np.zeros((lin.prob.L, 3, 3))
    for l in (range(lin.prob.L) if landmarks is None else landmarks):
        if not lin.ok[l]:
            continue
        o, rows = lin.observers(l)
        R = lin.R[l]
        M = np.zeros((3, 3))
        Z = lin.W[o] @ R
        for a in range(len(o)):
            V = np.zeros((6, 3))
            for b in range(len(o)):
                V += lin.Sig[np.ix_(rows[a], rows[b])] @ Z[b]
            M += Z[a].T @ V
        out[l] = R @ (np.eye(3) + M) @ R.T
    return out


def _full_blocks(lin, landmarks=None):
    """H_pp = S + sum over `landmarks` (None: all) of W H_ll^-1 W^T: the pose block of the system in which those landmarks are unknowns."""
    n = lin.S.shape[0]
    Hpp = lin.S.copy()
    for l in (range(lin.prob.L) if landmarks is None else landmarks):
        o, rows = lin.observers(l)
        if len(o) == 0 or not lin.ok[l]:
            continue
        idx = rows.reshape(-1)
        Wl = lin.W[o].reshape(-1, 3)
        Hpp[np.ix_(idx, idx)] += Wl @ lin.Hinv[l] @ Wl.T
    return n, Hpp


def route_b(lin, sample=None):
    """sample None: every landmark is an unknown of the matrix. sample = landmark indices: only those are (the others stay eliminated inside
    S, and their blocks stay zero here): the matrix has n + 3 len(sample) rows."""
    L = lin.prob.L
    good = np.flatnonzero(lin.ok) if sample is None else np.array([l for l in sample if lin.ok[l]], np.int64)
    n, Hpp = _full_blocks(lin, None if sample is None else good)
    out = np.zeros((L, 3, 3))
    col = -np.ones(L, np.int64); col[good] = n + 3 * np.arange(len(good))   # (a degenerate landmark has no block: it is left out of the matrix)
    N = n + 3 * len(good)
    F = np.zeros((N, N), order="F")
    F[:n, :n] = Hpp
    for l in good:
        c = col[l]
        F[c:c + 3, c:c + 3] = lin.H[l]
        o, rows = lin.observers(l)
        for t in range(len(o)):
            F[rows[t], c:c + 3] = lin.W[o[t]]; F[c:c + 3, rows[t]] = lin.W[o[t]].T
    c_, info = sl.lapack.dpotrf(F, lower=1, overwrite_a=1)
    assert info == 0, f"the full system is not positive definite (potrf info {info})"
    inv, info = sl.lapack.dpotri(c_, lower=1, overwrite_c=1)
    assert info == 0
    for l in good:
        c = col[l]
        blk = np.tril(inv[c:c + 3, c:c + 3])
        out[l] = blk + np.tril(blk, -1).T
    return out


def err(A, B, A_ref):
    """max |A - B| / max |A_routeA| per landmark, for stacks [m, 3, 3]."""
    den = np.abs(A_ref).reshape(len(A_ref), -1).max(axis=1)
    num = np.abs(A - B).reshape(len(A), -1).max(axis=1)
    return num / np.where(den > 0, den, 1.0)
