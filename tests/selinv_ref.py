"""The selected inverse restated in numpy: the Takahashi recursion over the fronts of a host plan (forms_util.host_plan), on
the oracle's reduced camera system. Nothing of the device code: own and border sets and the order alone.

A front f has own unknowns O and border B. With S = L L^T and Sigma = S^-1:
    Sigma_BO = -Sigma_BB L_BO L_OO^-1,     Sigma_OO = L_OO^-T (L_OO^-1 - L_BO^T Sigma_BO)
and Sigma_BB is a gather out of the finished square of the deepest owner p among f's border rows (B is a subset of own(p) + border(p): the
fill property). Fronts are visited root first: by decreasing level.
"""
import numpy as np

from tests.test_nd_plan import _scalars


def factor_fronts(S, parent, level, own, st, D):
    """Multifrontal Cholesky of the dense symmetric S over the plan: per front (rows: own then border, m = own count, L_OO, L_BO)."""
    nn = len(parent)
    rows_own = [_scalars(own[k], D) for k in range(nn)]
    rows_st = [_scalars(st[k], D) for k in range(nn)]
    upd = [np.zeros((len(rows_own[k]) + len(rows_st[k]),) * 2) for k in range(nn)]
    where = -np.ones(S.shape[0], int)
    out = [None] * nn
    for k in np.argsort(level, kind="stable"):
        idx = np.r_[rows_own[k], rows_st[k]]
        m = len(rows_own[k])
        F = upd[k]
        F[:, :m] += S[np.ix_(idx, rows_own[k])]
        F[:m, m:] = F[m:, :m].T
        L11 = np.linalg.cholesky(F[:m, :m])
        L21 = np.linalg.solve(L11, F[:m, m:]).T
        out[k] = (idx, m, L11, L21)
        p = parent[k]
        if p >= 0 and len(idx) > m:
            pidx = np.r_[rows_own[p], rows_st[p]]
            where[pidx] = np.arange(len(pidx))
            loc = where[idx[m:]]
            assert (loc >= 0).all(), "fill outside the parent's front"
            upd[p][np.ix_(loc, loc)] += F[m:, m:] - L21 @ L21.T
            where[pidx] = -1
    return out


def selected_inverse(S, parent, level, own, st, D):
    """Per front (rows [own + border], Sigma on them [own + border, own + border]) by the recursion, root first."""
    nn = len(parent)
    fac = factor_fronts(S, parent, level, own, st, D)
    n = S.shape[0]
    owner = -np.ones(n, int)
    for k in range(nn):
        owner[fac[k][0][:fac[k][1]]] = k
    depth = np.zeros(nn, int)
    for k in range(nn):
        if parent[k] >= 0:
            assert parent[k] < k
            depth[k] = depth[parent[k]] + 1
    where = -np.ones(n, int)
    out = [None] * nn
    for k in np.argsort(-np.asarray(level), kind="stable"):
        idx, m, L11, L21 = fac[k]
        nb = len(idx) - m
        Sig = np.zeros((len(idx), len(idx)))
        W = np.linalg.solve(L11, np.eye(m))             # L_OO^-1
        if nb:
            own_of_border = owner[idx[m:]]
            p = own_of_border[np.argmax(depth[own_of_border])]   # the deepest owner among the border rows
            assert level[p] > level[k]
            pidx, pSig = out[p]
            where[pidx] = np.arange(len(pidx))
            loc = where[idx[m:]]
            where[pidx] = -1
            assert (loc >= 0).all(), "a border row outside the ancestor's square: the fill property does not hold"
            G = pSig[np.ix_(loc, loc)]
            Sbo = -G @ (L21 @ W)
            Sig[m:, m:] = G
            Sig[m:, :m] = Sbo
            Sig[:m, m:] = Sbo.T
            Sig[:m, :m] = W.T @ (W - L21.T @ Sbo)
        else:
            Sig[:m, :m] = W.T @ W
        out[k] = (idx, Sig)
    return out
