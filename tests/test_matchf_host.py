"""Host side of the float (SIFT) descriptor matching (covgpu_match_float_batch): the numpy restatement
(tests/matchf_ref.py) on hand cases, the exactness claim for integer-valued rows, the share of indecisive rows of the non-integer
generator, the header's declarations against capi and the library's limits, the default options and the argument checks, which run
before any device work (covgpu_match_float_check runs them without a context)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from covins_amd import backend, capi
from tests import matchf_ref as fr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def rows(*r):
    return np.array(r, np.float32)


def test_threshold_boundary():
    """Four coordinates differing by 250 give d2 = 250 000: d = 500 matches at 500; one more unit of d2 does not."""
    q = np.zeros((1, 8), np.float32)
    near = np.zeros(8, np.float32); near[:4] = 250
    far = np.full(8, 255, np.float32)
    r = fr.knn2(q, np.stack([near, far]), 500.0, 0.8)
    assert r["match"].tolist() == [0] and r["dist"][0] == np.float32(500.0) and r["n"] == 1
    near[4] = 1                                              # d2 = 250 001
    r = fr.knn2(q, np.stack([near, far]), 500.0, 0.8)
    assert r["match"].tolist() == [-1] and r["dist"][0] == np.float32(-1) and r["n"] == 0


def test_ratio_boundary_in_float32():
    """d1 = 4, d2 = 5, ratio 0.8: 4 < 0.8f * 5 is false in float32 (0.8f * 5 rounds to 4)."""
    q = np.zeros((1, 4), np.float32)
    assert np.float32(0.8) * np.float32(5) == np.float32(4)
    assert fr.knn2(q, rows([4, 0, 0, 0], [3, 4, 0, 0]), 500.0, 0.8)["match"].tolist() == [-1]
    assert fr.knn2(q, rows([4, 0, 0, 0], [3, 4, 1, 0]), 500.0, 0.8)["match"].tolist() == [0]


def test_duplicates_and_short_train_sets():
    q = rows([10, 20, 30, 40])
    b = rows([200, 0, 0, 0], [10, 20, 30, 41], [10, 20, 30, 41], [0, 0, 0, 200])
    r = fr.knn2(q, b, 500.0, 1.5)                             # duplicated train rows: the lower index wins (1 < 1.5 * 1)
    assert r["match"].tolist() == [1] and r["dist"][0] == np.float32(1)
    assert fr.knn2(q, b, 500.0, 0.8)["match"].tolist() == [-1]
    s = np.concatenate([q, q, rows([1, 2, 3, 4])])           # identical sets with a duplicated row: 0 < 0.8 * 0 is false
    r = fr.knn2(s, s, 500.0, 0.8)                             # (the row that is there once matches itself at d = 0)
    assert r["match"].tolist() == [-1, -1, 2] and r["dist"].tolist() == [-1.0, -1.0, 0.0]
    assert fr.knn2(q, q, 500.0, 0.8)["match"].tolist() == [-1]   # one-row train set: no match
    assert fr.knn2(q, np.zeros((0, 4), np.float32))["n"] == 0
    assert fr.knn2(np.zeros((0, 4), np.float32), b)["match"].shape == (0,)


def test_integer_rows_make_the_float32_formula_exact():
    """For rows of integers 0..255 at dim 128 every intermediate is an integer below 2^24: float32 == float64 in every entry."""
    rng = np.random.default_rng(0)
    for _ in range(3):
        A = fr.sift_rows(rng, 300, 128)
        B = fr.train_rows(rng, A, 300)
        assert A.max() <= 255 and A.min() >= 0 and np.array_equal(A, np.rint(A))
        D64 = fr.d2_matrix(A, B)
        assert D64.max() < 2 ** 24 and np.array_equal(fr.d2_matrix_f32(A, B).astype(np.float64), D64)
        assert np.array_equal(D64, ((A[:, None, :].astype(np.float64) - B[None].astype(np.float64)) ** 2).sum(2))
    full = np.full((1, 128), 255, np.float32)                # the largest rows: |a|^2 + |b|^2 = 2 * 128 * 255^2 < 2^24
    assert fr.d2_matrix_f32(full, np.zeros((1, 128), np.float32))[0, 0] == 128 * 255 ** 2 and 2 * 128 * 255 ** 2 < 2 ** 24
    assert fr.d2_matrix_f32(full, full)[0, 0] == 0


def test_indecisive_share_of_the_rootsift_generator():
    """The GPU test lets indecisive rows differ and asserts that they are at most 3 % of a case: the generator must stay well below."""
    rng = np.random.default_rng(0)
    tot = bad = 0
    for _ in range(20):
        Q, T = fr.rootsift_job(rng, 300, 300, 128)
        assert np.allclose(np.linalg.norm(Q.astype(np.float64), axis=1), 1.0, atol=1e-6)
        r = fr.knn2(Q, T, 0.6, 0.8)
        assert r["n"] > 30                                   # the noisy copies match
        tot += 300; bad += int((~r["decisive"]).sum())
    print(f"indecisive rows: {bad} of {tot} = {100.0 * bad / tot:.2f} %")
    assert bad <= 0.03 * tot


def test_header_capi_and_limits_agree():
    h = open(os.path.join(ROOT, "include", "covgpu.h")).read()
    for name in ("covgpu_match_float_batch_t", "covgpu_default_match_float_opts", "covgpu_match_float_limits", "covgpu_match_float_batch",
                 "covgpu_match_float_check"):
        assert name in h
    body = re.search(r"typedef struct covgpu_match_float_batch_t \{(.*?)\} covgpu_match_float_batch_t;", h, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.search(r"(\w+)\s*$", d.strip()).group(1) for d in body.split(";") if d.strip()]
    assert fields == [f[0] for f in capi.MatchFloatBatch._fields_]
    assert fields == ["num_sets", "row_ptr", "dim", "desc", "num_jobs", "set_a", "set_b", "match", "dist", "nmatches"]
    assert re.search(r"covgpu_match_batch, covgpu_match_float_batch,", h)          # the list of the stateless batch calls
    lim = (C.c_int32 * 4)()
    backend.lib().covgpu_match_float_limits(lim)
    max_rows, max_dim, tile, chunk = list(lim)
    assert max_rows == capi.MATCH_MAX_ROWS == 4096 and max_dim >= 256 and max_dim % 4 == 0
    assert tile > 0 and tile % 32 == 0 and chunk > 0 and chunk % 32 == 0
    src = open(os.path.join(ROOT, "covins_amd", "csrc", "batch_limits.hpp")).read()
    assert int(re.search(r"kMatchFloatTileRows = (\d+);", src).group(1)) == tile
    assert int(re.search(r"kMatchFloatChunkRows = (\d+);", src).group(1)) == chunk
    assert int(re.search(r"kMatchFloatMaxDim = (\d+);", src).group(1)) == max_dim


def test_default_match_float_opts():
    o = capi.MatchOpts()
    backend.lib().covgpu_default_match_float_opts(C.byref(o))
    assert (o.mode, o.dist_threshold, o.ratio) == (capi.MATCH_KNN2, 500.0, np.float32(0.8))
    backend.lib().covgpu_default_match_float_opts(None)      # tolerated


def _check(parts, set_a, set_b, drop=(), dim=None, **opts):
    """covgpu_match_float_check of a batch; `drop`: struct fields passed as NULL. Returns (rc, message)."""
    o = capi.MatchOpts()
    backend.lib().covgpu_default_match_float_opts(C.byref(o))
    for k, v in opts.items():
        setattr(o, k, v)
    s = fr.make_sets(parts)
    ptr = np.ascontiguousarray(s["row_ptr"], np.int32)
    desc = np.ascontiguousarray(s["desc"], np.float32)
    sa, sb = np.array(set_a, np.int32), np.array(set_b, np.int32)
    tot = max(int(sum(len(parts[a]) for a in set_a if 0 <= a < len(parts))), 1)
    match, dist, nm = np.zeros(tot, np.int32), np.zeros(tot, np.float32), np.zeros(max(len(sa), 1), np.int32)
    keep = dict(row_ptr=capi.iptr(ptr), desc=desc.ctypes.data_as(capi._fp), set_a=capi.iptr(sa), set_b=capi.iptr(sb), match=capi.iptr(match),
                dist=dist.ctypes.data_as(capi._fp), nmatches=capi.iptr(nm))
    for k in drop:
        keep[k] = None
    b = capi.MatchFloatBatch(len(parts), keep["row_ptr"], s["dim"] if dim is None else dim, keep["desc"], len(sa), keep["set_a"], keep["set_b"],
                             keep["match"], keep["dist"], keep["nmatches"])
    rc = backend.lib().covgpu_match_float_check(C.byref(b), C.byref(o))
    return rc, backend.lib().covgpu_last_error().decode() if rc else ""


def test_argument_checks_need_no_device():
    lib = backend.lib()
    b, o = capi.MatchFloatBatch(), capi.MatchOpts()
    lib.covgpu_default_match_float_opts(C.byref(o))
    assert lib.covgpu_match_float_batch(None, C.byref(b), C.byref(o)) == 1
    assert lib.covgpu_last_error() == b"covgpu_match_float_batch: NULL context"
    assert lib.covgpu_match_float_check(None, None) == 1
    rng = np.random.default_rng(1)
    P = [fr.sift_rows(rng, 5, 8), fr.sift_rows(rng, 7, 8), np.zeros((0, 8), np.float32)]
    assert _check(P, [0, 1, 2, 0], [1, 0, 0, 2])[0] == 0                           # empty sets are valid
    assert _check(P, [], [])[0] == 0                                               # zero jobs are valid
    assert _check(P, [0], [1], drop=("dist",))[0] == 0                             # dist is optional
    nan = [P[0].copy(), P[1].copy()]; nan[1][3, 2] = np.nan
    inf = [P[0].copy(), P[1].copy()]; inf[0][0, 0] = np.inf
    big = [P[0].copy(), P[1].copy()]; big[0][0, 0] = 1e19
    dec = fr.make_sets(P)["row_ptr"]
    for kw, msg in ((dict(parts=P, set_a=[0], set_b=[1], mode=capi.MATCH_DENSE), "mode must be COVGPU_MATCH_KNN2"),
                    (dict(parts=P, set_a=[0], set_b=[1], dist_threshold=0.0), "dist_threshold"),
                    (dict(parts=P, set_a=[0], set_b=[1], dist_threshold=float("nan")), "dist_threshold"),
                    (dict(parts=P, set_a=[0], set_b=[1], ratio=float("inf")), "ratio"),
                    (dict(parts=P, set_a=[0], set_b=[1], dim=6), "dim must be a positive multiple of 4"),
                    (dict(parts=P, set_a=[0], set_b=[1], dim=0), "dim must be a positive multiple of 4"),
                    (dict(parts=P, set_a=[0], set_b=[1], dim=260), "dim must be a positive multiple of 4"),
                    (dict(parts=P, set_a=[0], set_b=[3]), "set index out of range"),
                    (dict(parts=P, set_a=[-1], set_b=[0]), "set index out of range"),
                    (dict(parts=nan, set_a=[0], set_b=[1]), "descriptor value not finite"),
                    (dict(parts=inf, set_a=[0], set_b=[1]), "descriptor value not finite"),
                    (dict(parts=big, set_a=[0], set_b=[1]), "above 1e18"),
                    (dict(parts=P, set_a=[0], set_b=[1], drop=("desc",)), "NULL desc"),
                    (dict(parts=P, set_a=[0], set_b=[1], drop=("row_ptr",)), "NULL row_ptr"),
                    (dict(parts=P, set_a=[0], set_b=[1], drop=("match",)), "NULL match"),
                    (dict(parts=P, set_a=[0], set_b=[1], drop=("nmatches",)), "NULL job array"),
                    (dict(parts=[np.zeros((4097, 4), np.float32)], set_a=[0], set_b=[0]), "more than COVGPU_MATCH_MAX_ROWS rows")):
        rc, err = _check(**kw)
        assert rc == 1 and err.startswith("covgpu_match_float_check: ") and msg in err, (msg, rc, err)
    # row_ptr itself: not starting at 0, not monotone
    o2 = capi.MatchOpts(); lib.covgpu_default_match_float_opts(C.byref(o2))
    desc = np.zeros((12, 8), np.float32)
    for ptr, msg in ((np.array([1, 5, 12], np.int32), "row_ptr[0] != 0"), (np.array([0, 7, 5], np.int32), "row_ptr not monotone")):
        bb = capi.MatchFloatBatch(2, capi.iptr(ptr), 8, desc.ctypes.data_as(capi._fp), 0, None, None, None, None, None)
        assert lib.covgpu_match_float_check(C.byref(bb), C.byref(o2)) == 1 and msg in lib.covgpu_last_error().decode()
    assert dec[0] == 0


def test_python_wrapper_rejects_before_the_library():
    class NoCtx(backend.Context):
        def __init__(self):
            self._h = None
    c = NoCtx()
    with pytest.raises(TypeError):
        backend.Context.match_float_batch(c, dict(row_ptr=[0, 1], desc=np.zeros((1, 4), np.float32)), [0], [0], radius=1.0)
    with pytest.raises(ValueError):
        backend.Context.match_float_batch(c, dict(row_ptr=[0, 1], desc=np.zeros((1, 4), np.float32)), [0, 0], [0])


def test_facade_matchf_shim_compiles():
    """LoopMatcherT's float and pair-list entry points instantiate on COVINS-shaped classes without traits
    (tests/cpp/facade_matchf_shim.cpp; tests/test_gpu_matchf.py drives it)."""
    from tests import matchf_util as fu
    lib = fu.matchf_shim()
    assert lib.mf_match_float is not None and lib.mf_match_grid is not None
