"""Numpy restatement of the float (SIFT) descriptor matching contract (covgpu_match_float_batch): squared L2
distances in float64 from the float32 rows, the two nearest train rows by (d2, index) through a stable argsort, the distance and ratio
tests on np.float32(np.sqrt(d2)) as float32 comparisons. It also returns, per query row, whether every decision survives the rounding
bound of the float32 formula (the row is "decisive"), and that bound."""
import numpy as np


def gamma(dim):
    """(dim + 2) 2^-24: the bound of a length-dim float32 fma chain, with room for the two roundings of (|a|^2 + |b|^2) - 2 ab."""
    return (dim + 2) * 2.0 ** -24


def d2_matrix(A, B):
    """(|a|^2 + |b|^2) - 2 a.b, clamped at 0, in float64 from float32 rows: [nA, nB]."""
    A = np.asarray(A, np.float32).astype(np.float64)
    B = np.asarray(B, np.float32).astype(np.float64)
    na = (A * A).sum(1)
    nb = (B * B).sum(1)
    return np.maximum(0.0, (na[:, None] + nb[None, :]) - 2.0 * (A @ B.T))


def d2_matrix_f32(A, B):
    """The contract's own arithmetic: every product, sum and difference rounded to float32 (the sums in k order)."""
    A = np.asarray(A, np.float32)
    B = np.asarray(B, np.float32)
    na = np.zeros(len(A), np.float32)
    nb = np.zeros(len(B), np.float32)
    ab = np.zeros((len(A), len(B)), np.float32)
    for k in range(A.shape[1]):
        # a float64 product of two float32 values is exact, so rounding (p + s) once is the fmaf
        na = (A[:, k].astype(np.float64) ** 2 + na).astype(np.float32)
        nb = (B[:, k].astype(np.float64) ** 2 + nb).astype(np.float32)
        ab = (np.outer(A[:, k].astype(np.float64), B[:, k].astype(np.float64)) + ab).astype(np.float32)
    s = (na[:, None] + nb[None, :]).astype(np.float32)
    return np.maximum(np.float32(0), (s - np.float32(2) * ab).astype(np.float32))


def knn2(A, B, thr=500.0, ratio=0.8):
    """One job. Returns dict(match [nA] int32 (local B row or -1), dist [nA] float32 (d1 of a match, -1 otherwise), n, decisive [nA]
    bool, eps1 [nA] (the bound on the best's squared distance), d1 [nA] float64 (the best's distance, nan without two train rows))."""
    A = np.asarray(A, np.float32)
    B = np.asarray(B, np.float32)
    nA, nB = len(A), len(B)
    match = np.full(nA, -1, np.int32)
    dist = np.full(nA, -1.0, np.float32)
    out = dict(match=match, dist=dist, n=0, decisive=np.ones(nA, bool), eps1=np.zeros(nA), d1=np.full(nA, np.nan))
    if nA == 0 or nB < 2:                                    # fewer than two train rows: no match, and nothing to decide
        return out
    dim = A.shape[1]
    D2 = d2_matrix(A, B)
    order = np.argsort(D2, axis=1, kind="stable")            # equal distances keep the lower index first
    rows = np.arange(nA)
    i1, i2 = order[:, 0], order[:, 1]
    q1, q2 = D2[rows, i1], D2[rows, i2]
    f32 = lambda x: np.sqrt(x).astype(np.float32)
    t, r = np.float32(thr), np.float32(ratio)
    d1, d2 = f32(q1), f32(q2)
    ok = (d1 <= t) & (d1 < r * d2)
    match[ok] = i1[ok]
    dist[ok] = d1[ok]
    out["n"] = int(ok.sum())
    out["d1"] = np.sqrt(q1)
    # decisive: every decision survives +-eps(a, b) = 2 gamma (|a|^2 + |b|^2) on each squared distance
    A64, B64 = A.astype(np.float64), B.astype(np.float64)
    E = 2.0 * gamma(dim) * ((A64 * A64).sum(1)[:, None] + (B64 * B64).sum(1)[None, :])
    lo, hi = np.maximum(0.0, D2 - E), D2 + E
    e1, e2 = E[rows, i1], E[rows, i2]
    out["eps1"] = e1
    lo_rest = lo.copy(); lo_rest[rows, i1] = np.inf
    best = hi[rows, i1] < lo_rest.min(1)                      # the identity of the best
    lo_rest[rows, i2] = np.inf
    second = hi[rows, i2] < lo_rest.min(1)                    # the identity of the second best: d3 - d2 (true with two train rows)
    lo1, hi1, lo2, hi2 = f32(lo[rows, i1]), f32(hi[rows, i1]), f32(lo[rows, i2]), f32(hi[rows, i2])
    thr_ok = (lo1 <= t) == (hi1 <= t)
    ratio_ok = (hi1 < r * lo2) == (lo1 < r * hi2)
    out["decisive"] = best & second & thr_ok & ratio_ok
    return out


def batch(sets, set_a, set_b, thr=500.0, ratio=0.8):
    """The jobs of one call: dict(match, dist, nmatches, offset, decisive, eps1, d1) in the layout of Context.match_float_batch."""
    ptr = np.asarray(sets["row_ptr"])
    desc = np.asarray(sets["desc"], np.float32)
    res = [knn2(desc[ptr[a]:ptr[a + 1]], desc[ptr[b]:ptr[b + 1]], thr, ratio) for a, b in zip(set_a, set_b)]
    off = np.zeros(len(res) + 1, np.int64)
    off[1:] = np.cumsum([len(r["match"]) for r in res])
    cat = lambda k, dt: np.concatenate([r[k] for r in res]).astype(dt) if res else np.zeros(0, dt)
    return dict(match=cat("match", np.int32), dist=cat("dist", np.float32), nmatches=np.array([r["n"] for r in res], np.int32), offset=off,
                decisive=cat("decisive", bool), eps1=cat("eps1", np.float64), d1=cat("d1", np.float64))


# ---- generators of the tests (OpenCV's SIFT rows are integers 0..255 stored as float)

def sift_rows(rng, n, dim):
    """gamma(0.6) bins, normalised, clamped at 0.2, renormalised, x512, rounded and saturated to 255."""
    x = rng.gamma(0.6, size=(n, dim))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    x = np.minimum(x, 0.2)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return np.minimum(np.rint(x * 512.0), 255.0).astype(np.float32)


def train_rows(rng, Q, n, sigma=12.0):
    """n train rows for the query rows Q: one third noisy copies of query rows (sigma, re-rounded) among fresh rows, shuffled."""
    dim = Q.shape[1]
    k = min(n // 3, n) if len(Q) else 0
    src = Q[rng.integers(0, len(Q), k)] if k else np.zeros((0, dim), np.float32)
    noisy = np.clip(np.rint(src + rng.normal(0.0, sigma, src.shape)), 0.0, 255.0).astype(np.float32)
    rows = np.concatenate([noisy, sift_rows(rng, n - k, dim)])
    return rows[rng.permutation(n)]


def rootsift(X):
    """RootSIFT: L1-normalise, square root; unit L2 norm."""
    X = np.asarray(X, np.float64)
    return np.sqrt(X / np.maximum(X.sum(1, keepdims=True), 1e-300)).astype(np.float32)


def rootsift_job(rng, nA, nB, dim, sigma=0.02):
    """A non-integer job: RootSIFT query rows; one third of the train rows are query rows + N(0, sigma), clipped at 0 and renormalised."""
    Q = rootsift(sift_rows(rng, nA, dim))
    k = nB // 3 if nA else 0
    src = Q[rng.integers(0, nA, k)].astype(np.float64) if k else np.zeros((0, dim))
    noisy = np.maximum(src + rng.normal(0.0, sigma, src.shape), 0.0)
    noisy /= np.maximum(np.linalg.norm(noisy, axis=1, keepdims=True), 1e-300)
    T = np.concatenate([noisy.astype(np.float32), rootsift(sift_rows(rng, nB - k, dim))])
    return Q, T[rng.permutation(nB)]


def make_sets(parts):
    """dict(row_ptr, desc) of a list of [rows, dim] arrays."""
    ptr = np.zeros(len(parts) + 1, np.int32)
    ptr[1:] = np.cumsum([len(p) for p in parts])
    dim = parts[0].shape[1]
    return dict(row_ptr=ptr, desc=np.concatenate(parts).astype(np.float32).reshape(-1, dim), dim=dim)
