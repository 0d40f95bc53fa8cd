"""covgpu_match_float_batch (k_matchf.hip) on the GPU against the numpy restatement (tests/matchf_ref.py): integer-valued
(SIFT) rows bit for bit over every size at which the kernel takes another path (sizes read from covgpu_match_float_limits), hand cases,
batch independence, shared sets, other thresholds; non-integer (RootSIFT) rows on their decisive rows, with the share of indecisive rows
asserted; the argument checks on the device path; the chain into covgpu_relpose_batch; and the C++ facade."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
from scipy.spatial.transform import Rotation as Rot

from covins_amd import backend, capi, synth
from tests import matchf_ref as fr
from tests import matchf_util as fu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = backend.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def lim():
    out = (C.c_int32 * 4)()
    backend.lib().covgpu_match_float_limits(out)
    return dict(rows=out[0], dim=out[1], tile=out[2], chunk=out[3])


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def check_exact(ctx, parts, set_a, set_b, **opts):
    """One call against the restatement, bit for bit: match, dist as float32 bits, nmatches."""
    sets = fr.make_sets(parts)
    res = ctx.match_float_batch(sets, set_a, set_b, **opts)
    ref = fr.batch(sets, set_a, set_b, opts.get("dist_threshold", 500.0), opts.get("ratio", 0.8))
    assert np.array_equal(res["offset"], ref["offset"])
    bad = np.flatnonzero(res["match"] != ref["match"])
    assert bad.size == 0, (bad[:8], res["match"][bad[:8]], ref["match"][bad[:8]])
    assert np.array_equal(bits(res["dist"]), bits(ref["dist"]))
    assert np.array_equal(res["nmatches"], ref["nmatches"])
    return res, ref


def int_jobs(rng, sizes, dim):
    """A job of its own two sets per (query rows, train rows)."""
    parts, sa, sb = [], [], []
    for nA, nB in sizes:
        Q = fr.sift_rows(rng, nA, dim)
        parts += [Q, fr.train_rows(rng, Q, nB)]
        sa.append(len(parts) - 2); sb.append(len(parts) - 1)
    return parts, sa, sb


# ------------------------------------------------------------------------------------------------ integer-valued rows: bit for bit
@pytest.mark.parametrize("dim", [4, 128, 132, "max"])
def test_integer_rows_every_size_bit_for_bit(ctx, lim, dim):
    dim = lim["dim"] if dim == "max" else dim
    t, c = lim["tile"], lim["chunk"]
    sizes = [(nA, nB) for nA in (1, t - 1, t, t + 1, 2 * t + 1) for nB in (0, 1, 2, c - 1, c, c + 1, 2 * c + 1)]
    parts, sa, sb = int_jobs(np.random.default_rng(100 + dim), sizes, dim)
    res, ref = check_exact(ctx, parts, sa, sb)
    if dim >= 128:
        assert ref["nmatches"].sum() > 100                   # the noisy copies are found


def test_a_set_of_the_largest_size_bit_for_bit(ctx, lim):
    rng = np.random.default_rng(7)
    big = fr.sift_rows(rng, lim["rows"], 128)
    small = fr.train_rows(rng, big, 300)
    res, ref = check_exact(ctx, [big, small], [0, 1], [1, 0])
    assert ref["nmatches"][1] > 50


def test_hand_cases_bit_for_bit(ctx, lim):
    z = lambda n, d, v=0.0: np.full((n, d), v, np.float32)
    q = np.array([[10, 20, 30, 40]], np.float32)
    dup = np.array([[200, 0, 0, 0], [10, 20, 30, 41], [10, 20, 30, 41], [0, 0, 0, 200]], np.float32)
    res, _ = check_exact(ctx, [q, dup], [0], [1], ratio=1.5)                      # duplicated train rows: the lower index wins
    assert res["match"].tolist() == [1] and res["dist"].tolist() == [1.0]
    check_exact(ctx, [q, dup], [0], [1])
    near = z(1, 8); near[0, :4] = 250
    far = z(1, 8, 255.0)
    res, _ = check_exact(ctx, [z(1, 8), np.concatenate([near, far])], [0], [1])   # d2 = 250 000: d = 500 matches at 500
    assert res["match"].tolist() == [0] and res["dist"].tolist() == [500.0]
    near[0, 4] = 1
    res, _ = check_exact(ctx, [z(1, 8), np.concatenate([near, far])], [0], [1])   # d2 = 250 001 does not
    assert res["match"].tolist() == [-1]
    r45 = np.array([[4, 0, 0, 0], [3, 4, 0, 0]], np.float32)
    res, _ = check_exact(ctx, [z(1, 4), r45], [0], [1])                           # 4 < 0.8f * 5 is false in float32
    assert res["match"].tolist() == [-1]
    r45[1, 2] = 1
    res, _ = check_exact(ctx, [z(1, 4), r45], [0], [1])
    assert res["match"].tolist() == [0]
    # all-equal rows over more than one tile and chunk: every distance 0, every list (0, 1), 0 < 0.8 * 0 false
    same = z(lim["tile"] + 3, 128, 17.0)
    res, _ = check_exact(ctx, [same, same[:lim["chunk"] + 5]], [0], [1])
    assert res["nmatches"].tolist() == [0]
    res, _ = check_exact(ctx, [same, same[:lim["chunk"] + 5]], [0], [1], ratio=1.0)
    assert res["nmatches"].tolist() == [0]
    # a train row equal to the query: d2 = 0 exactly, never negative (sqrtf of a negative number would be NaN)
    rng = np.random.default_rng(3)
    Q = fr.sift_rows(rng, 70, 128)
    T = np.concatenate([fr.sift_rows(rng, 90, 128), Q])[rng.permutation(160)]
    res, _ = check_exact(ctx, [Q, T], [0], [1])
    assert res["nmatches"][0] == 70 and np.all(res["dist"] == 0.0)
    # the largest rows against zero rows: the padding of the last chunk is zero too, and may win only if its distance is not +inf
    for dim in (128, lim["dim"]):
        res, _ = check_exact(ctx, [z(2, dim, 255.0), z(2, dim)], [0], [1], dist_threshold=5000.0, ratio=1.5)
        assert res["match"].tolist() == [0, 0] and np.all(res["dist"] == np.float32(np.sqrt(dim * 255.0 ** 2)))
        res, _ = check_exact(ctx, [z(2, dim, 255.0), z(3, dim, 255.0), z(1, dim)], [0, 0], [1, 2], dist_threshold=5000.0, ratio=1.5)
        assert res["nmatches"].tolist() == [0, 0]                                  # 0 < 1.5 * 0 false; one train row


def test_a_job_alone_equals_the_same_job_in_a_shuffled_batch(ctx):
    rng = np.random.default_rng(11)
    sizes = [(int(a), int(b)) for a, b in zip(rng.integers(60, 301, 40), rng.integers(60, 301, 40))]
    parts, sa, sb = int_jobs(rng, sizes, 128)
    order = rng.permutation(40)
    res, _ = check_exact(ctx, parts, [sa[j] for j in order], [sb[j] for j in order])
    for pos in (0, 17, 39):
        j = order[pos]
        one = ctx.match_float_batch(fr.make_sets([parts[sa[j]], parts[sb[j]]]), [0], [1])
        lo, hi = res["offset"][pos], res["offset"][pos + 1]
        assert np.array_equal(one["match"], res["match"][lo:hi]) and np.array_equal(bits(one["dist"]), bits(res["dist"][lo:hi]))
        assert one["nmatches"][0] == res["nmatches"][pos]


def test_a_set_named_by_several_jobs(ctx):
    rng = np.random.default_rng(12)
    Q = fr.sift_rows(rng, 200, 128)
    parts = [Q, fr.train_rows(rng, Q, 150), fr.train_rows(rng, Q, 70), np.zeros((0, 128), np.float32)]
    res, ref = check_exact(ctx, parts, [0, 0, 1, 0, 2, 3, 0, 1], [1, 2, 0, 0, 1, 0, 3, 1])
    assert ref["nmatches"][0] > 20 and ref["nmatches"][5] == 0 and ref["nmatches"][6] == 0
    # zero jobs are valid
    none = ctx.match_float_batch(fr.make_sets(parts), [], [])
    assert none["match"].shape == (0,) and none["nmatches"].shape == (0,)


@pytest.mark.parametrize("opts", [dict(dist_threshold=400.0, ratio=0.7), dict(dist_threshold=600.0, ratio=1.0)])
def test_other_thresholds(ctx, opts):
    rng = np.random.default_rng(13)
    parts, sa, sb = int_jobs(rng, [(300, 300), (129, 200), (50, 65)], 128)
    _, ref = check_exact(ctx, parts, sa, sb, **opts)
    assert ref["nmatches"][0] > 20


# ------------------------------------------------------------------------------------------------ non-integer rows
@pytest.mark.parametrize("dim,sizes", [(128, [(300, 300)] * 8), (132, [(257, 129), (129, 257)]), ("max", [(257, 129), (300, 300)])])
def test_rootsift_rows_agree_on_the_decisive_rows(ctx, lim, dim, sizes):
    """RootSIFT rows (unit norm, noise 0.02, thresholds 0.6 / 0.8): a row whose identity of best and second best, threshold test, ratio
    test and d3 - d2 all survive +-eps = 2 (dim + 2) 2^-24 (|a|^2 + |b|^2) on each squared distance must agree exactly in match, and in
    dist to 2 ulp plus eps / (2 d). The other rows may differ, and may be at most 3 % of the case."""
    dim = lim["dim"] if dim == "max" else dim
    rng = np.random.default_rng(0)
    parts, sa, sb = [], [], []
    for nA, nB in sizes:
        parts += list(fr.rootsift_job(rng, nA, nB, dim))
        sa.append(len(parts) - 2); sb.append(len(parts) - 1)
    sets = fr.make_sets(parts)
    res = ctx.match_float_batch(sets, sa, sb, dist_threshold=0.6, ratio=0.8)
    ref = fr.batch(sets, sa, sb, 0.6, 0.8)
    dec = ref["decisive"]
    share = 1.0 - dec.mean()
    differ = int((res["match"] != ref["match"]).sum())
    print(f"dim {dim}: indecisive {100 * share:.2f} % of {dec.size} rows; rows that differ in match: {differ}; matches {int(ref['nmatches'].sum())}")
    assert share <= 0.03
    assert ref["nmatches"].sum() > 0.1 * dec.size            # (the noisy copies match: the case exercises the tests, not only rejections)
    assert np.array_equal(res["match"][dec], ref["match"][dec])
    hit = dec & (ref["match"] >= 0)
    g, r = res["dist"][hit].astype(np.float64), ref["dist"][hit].astype(np.float64)
    with np.errstate(divide="ignore"):
        tol = 2.0 * np.spacing(ref["dist"][hit]).astype(np.float64) + ref["eps1"][hit] / (2.0 * ref["d1"][hit])
    err = np.abs(g - r)
    print(f"  dist: max error {err.max():.3e}, max error / tolerance {np.max(err / tol):.3f}")
    assert np.all(err <= tol)
    assert np.all(res["dist"][dec & (ref["match"] < 0)] == -1.0)
    if not differ:                                            # then the counts agree as well
        assert np.array_equal(res["nmatches"], ref["nmatches"])


# ------------------------------------------------------------------------------------------------ validation on the device path
def test_invalid_arguments_are_rejected_on_the_device_path(ctx, lim):
    rng = np.random.default_rng(5)
    P = [fr.sift_rows(rng, 5, 8), fr.sift_rows(rng, 7, 8)]
    with pytest.raises(backend.CovGpuError, match="mode must be COVGPU_MATCH_KNN2"):
        ctx.match_float_batch(fr.make_sets(P), [0], [1], mode="dense")
    with pytest.raises(backend.CovGpuError, match="more than COVGPU_MATCH_MAX_ROWS rows"):
        ctx.match_float_batch(fr.make_sets([np.zeros((lim["rows"] + 1, 4), np.float32), P[0][:, :4]]), [1], [0])
    with pytest.raises(backend.CovGpuError, match="dim must be a positive multiple of 4"):
        ctx.match_float_batch(fr.make_sets([P[0][:, :6], P[1][:, :6]]), [0], [1])
    with pytest.raises(backend.CovGpuError, match="covgpu_match_float_batch: descriptor value not finite"):
        bad = P[1].copy(); bad[2, 3] = np.nan
        ctx.match_float_batch(fr.make_sets([P[0], bad]), [0], [1])
    check_exact(ctx, P, [0], [1])                             # the context still works


# ------------------------------------------------------------------------------------------------ chain into the relative pose
def _pose(p7):
    T = np.eye(4); T[:3, :3] = Rot.from_quat(p7[:4]).as_matrix(); T[:3, 3] = p7[4:]
    return T


def test_chain_float_matches_into_relpose(ctx):
    """Plumbing: the matches of an integer-row job between two map keyframes (one SIFT row per landmark, noisy per observation, plus
    distractor rows) become the correspondences of covgpu_relpose_batch, which runs to a finite result."""
    m = synth.make_map(synth.config_named("small"))
    rng = np.random.default_rng(21)
    seen = [dict() for _ in range(m.K)]                      # per keyframe: landmark -> observation
    for l in range(m.L):
        for o in range(m.lm_obs_ptr[l], m.lm_obs_ptr[l + 1]):
            seen[int(m.obs_kf[o])][l] = o
    q, c = max(((a, b) for a in range(m.K) for b in range(a + 1, min(a + 4, m.K))), key=lambda p: len(set(seen[p[0]]) & set(seen[p[1]])))
    assert len(set(seen[q]) & set(seen[c])) >= 30
    base = fr.sift_rows(rng, m.L, 128)
    def rows_of(k):
        lms = np.array(sorted(seen[k]))
        own = np.clip(np.rint(base[lms] + rng.normal(0.0, 8.0, (len(lms), 128))), 0, 255).astype(np.float32)
        d = np.concatenate([own, fr.sift_rows(rng, 40, 128)])
        lm = np.concatenate([lms, np.full(40, -1)])
        p = rng.permutation(len(d))
        return d[p], lm[p]
    dq, lq = rows_of(q)
    dc, lc = rows_of(c)
    res, _ = check_exact(ctx, [dq, dc], [0], [1])
    a = np.flatnonzero(res["match"] >= 0)
    lA, lB = lq[a], lc[res["match"][a]]
    assert len(a) >= 25 and np.all(lA >= 0) and np.mean(lA == lB) > 0.95
    Twc = lambda k: _pose(m.kf_pose[k]) @ _pose(m.cam_extr[int(m.kf_cam[k])])
    to_cam = lambda k, l: (np.linalg.inv(Twc(k)) @ np.c_[m.lm_pos[l], np.ones(len(l))].T).T[:, :3]
    T12 = np.linalg.inv(Twc(q)) @ Twc(c)
    qt = Rot.from_matrix(T12[:3, :3]).as_quat()
    camv = np.concatenate([m.cam_intr[0], m.cam_dist[0]])
    n = len(a)
    rb = dict(ptr=np.array([0, n], np.int32), pA=to_cam(q, lA), pB=to_cam(c, lB),
              kpA=np.array([m.obs_uv[seen[q][int(l)]] for l in lA], np.float64), kpB=np.array([m.obs_uv[seen[c][int(l)]] for l in lB], np.float64),
              sigA=np.ones(n), sigB=np.ones(n), camA=camv[None], camB=camv[None], distA=np.array([int(m.cam_dist_type[0])], np.int32),
              distB=np.array([int(m.cam_dist_type[0])], np.int32), T0=np.concatenate([qt if qt[3] >= 0 else -qt, T12[:3, 3]])[None])
    T, outl, inl = ctx.relpose_batch(rb, th_outlier=1.3, min_inliers=12)
    assert np.all(np.isfinite(T)) and T.shape == (1, 7) and abs(np.linalg.norm(T[0, :4]) - 1.0) < 1e-9
    assert inl[0] > 0 and outl.shape == (n,)


# ------------------------------------------------------------------------------------------------ C++ facade
def _ref_lists(parts, q, cands, thr, ratio):
    out = []
    for c in cands:
        r = fr.knn2(parts[q], parts[c], thr, ratio)
        out.append([(int(a), int(r["match"][a]), float(r["dist"][a])) for a in np.flatnonzero(r["match"] >= 0)])
    return out


@pytest.fixture(scope="module")
def shim():
    lib = fu.matchf_shim()
    yield lib
    lib.mf_shutdown()


def test_facade_float_matcher_equals_the_restatement(shim):
    """LoopMatcherT::MatchImagesFloatBatch, descriptors_add_ read as a CV_32F cv::Mat: one query against five candidates (one empty)."""
    rng = np.random.default_rng(31)
    Q = fr.sift_rows(rng, 300, 128)
    parts = [Q] + [fr.train_rows(rng, Q, n) for n in (300, 257, 64, 1)] + [np.zeros((0, 128), np.float32)]
    h = fu.build(shim, parts, fu.CV_32F, [-1] * len(parts))
    try:
        got = fu.match(shim, h, 0, [1, 2, 3, 4, 5], 500.0, 0.8)
        want = _ref_lists(parts, 0, [1, 2, 3, 4, 5], 500.0, 0.8)
        assert got == want and len(want[0]) > 50 and want[3] == [] and want[4] == []
        assert fu.match(shim, h, 0, [2, 1], 400.0, 0.7) == _ref_lists(parts, 0, [2, 1], 400.0, 0.7)
        assert fu.match(shim, h, 0, [], 500.0, 0.8) == []
    finally:
        shim.mf_free(h)


@pytest.mark.parametrize("feature_type", ["SIFT", "ORB"])
def test_facade_pair_grid_equals_six_single_calls(shim, feature_type):
    """LoopMatcherT::MatchImagePairsBatch on findMatches' 2 x 3 grid (the query and its predecessor against the candidate and its two
    predecessors) in one call equals the six single-candidate calls, for float rows and for ORB rows."""
    rng = np.random.default_rng(32)
    orb = feature_type == "ORB"
    if orb:
        base = rng.integers(0, 256, (400, 32), dtype=np.uint8)
        def kf_rows(n):
            d = base[rng.choice(400, n, replace=False)].copy()
            flip = rng.integers(0, 256, d.shape, dtype=np.uint8) & rng.integers(0, 256, d.shape, dtype=np.uint8) & \
                rng.integers(0, 256, d.shape, dtype=np.uint8) & rng.integers(0, 256, d.shape, dtype=np.uint8)
            return d ^ flip                                   # about 16 of 256 bits flipped
        parts = [kf_rows(n) for n in (250, 300, 200, 257, 300)]
        thr, ratio = 40.0, 0.8
    else:
        Q = fr.sift_rows(rng, 300, 128)
        parts = [fr.train_rows(rng, Q, 250), Q, fr.train_rows(rng, Q, 200), fr.train_rows(rng, Q, 257), fr.train_rows(rng, Q, 300)]
        thr, ratio = 500.0, 0.8
    # keyframes 0 <- 1 (the query) and 2 <- 3 <- 4 (the candidate)
    h = fu.build(shim, parts, fu.CV_8U if orb else fu.CV_32F, [-1, 0, -1, 2, 3])
    try:
        pairs, lists = fu.match_grid(shim, h, 1, 4, 2, 3, feature_type, thr, ratio)
        assert pairs == [(1, 4), (1, 3), (1, 2), (0, 4), (0, 3), (0, 2)]
        assert sum(len(l) for l in lists) > 100
        for (a, b), got in zip(pairs, lists):
            assert got == fu.match(shim, h, a, [b], thr, ratio, orb=orb)[0], (a, b)
        if not orb:
            assert lists == [_ref_lists(parts, a, [b], thr, ratio)[0] for a, b in pairs]
        # a grid cut short by a missing predecessor
        pairs, lists = fu.match_grid(shim, h, 0, 3, 2, 3, feature_type, thr, ratio)
        assert pairs == [(0, 3), (0, 2)] and lists[0] == fu.match(shim, h, 0, [3], thr, ratio, orb=orb)[0]
    finally:
        shim.mf_free(h)


def test_facade_float_call_on_a_cv8u_matrix_is_fatal():
    """A CV_8U descriptors_add_ handed to the float call takes the reference's fatal path (exit(-1)), before any device work; in a child
    process, since the path ends the process."""
    fu.matchf_shim()
    code = ("import numpy as np\n"
            "from tests import matchf_util as fu\n"
            "lib = fu.matchf_shim()\n"
            "h = fu.build(lib, [np.zeros((3, 32), np.uint8), np.ones((4, 32), np.uint8)], fu.CV_8U, [-1, -1])\n"
            "fu.match(lib, h, 0, [1], 500.0, 0.8)\n"
            "print('survived')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=fu.ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 255 and "survived" not in r.stdout
    assert "FATAL: descriptors_add_ is not a continuous CV_32F matrix" in r.stderr
