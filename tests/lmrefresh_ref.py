"""The rule of covgpu_landmark_refresh (include/covgpu.h) restated in numpy: Landmark::ComputeDescriptor
(landmark_be.cpp:49-92) and Landmark::UpdateNormal (:185-220) for every landmark, observations in the order given. Written from the
rule, not from the kernel: integer Hamming distances, a sorted row per candidate, the element of rank (n - 1) // 2, the first strict
minimum; float64 operations one at a time in the stated order (numpy rounds every elementwise operation on its own, so there is no
fused multiply-add). It is the yardstick of tests/test_gpu_lmrefresh.py, bit for bit, and is itself held to a serial C++ restatement of
the reference's literal arithmetic in tests/test_lmrefresh_host.py."""
import math

import numpy as np

DEFAULT_OPTS = dict(scale_factor=2.0, num_octaves=1)   # config_backend.yaml:31-32
FORM_LANES = (4, 8, 16, 32, 64)                        # the lane-group forms; a longer list takes the long form
OUTPUTS = ("lm_desc_obs", "lm_desc", "lm_normal", "lm_min_distance", "lm_max_distance", "lm_status")


def make_inputs(lm_obs_ptr, obs_kf, obs_desc, obs_octave, lm_ref_obs, lm_pos, kf_center, kf_invalid=None, lm_invalid=None):
    ptr = np.ascontiguousarray(lm_obs_ptr, np.int32); okf = np.ascontiguousarray(obs_kf, np.int32)
    cen = np.ascontiguousarray(kf_center, np.float64).reshape(-1, 3)
    K, L = len(cen), len(ptr) - 1
    flag = lambda a, n: np.zeros(n, bool) if a is None else np.asarray(a, bool)
    return dict(K=K, L=L, lm_obs_ptr=ptr, obs_kf=okf,
                obs_desc=None if obs_desc is None else np.ascontiguousarray(obs_desc, np.uint8).reshape(-1, 32),
                obs_octave=np.ascontiguousarray(obs_octave, np.int32), lm_ref_obs=np.ascontiguousarray(lm_ref_obs, np.int32),
                lm_pos=np.ascontiguousarray(lm_pos, np.float64).reshape(-1, 3), kf_center=cen, kf_invalid=flag(kf_invalid, K),
                lm_invalid=flag(lm_invalid, L))


def hamming_matrix(desc):
    """[n,n] int64 pairwise Hamming distances of [n,32] uint8 rows."""
    bits = np.unpackbits(np.asarray(desc, np.uint8).reshape(-1, 32), axis=1).astype(np.int64)
    return bits @ (1 - bits).T + (1 - bits) @ bits.T


def choose_descriptor(desc):
    """Position among the candidate rows `desc` [n,32] of the row with the strictly smallest median distance, and the medians."""
    n = len(desc)
    med = np.sort(hamming_matrix(desc), axis=1)[:, (n - 1) // 2]      # self-distance 0 included
    return int(np.argmin(med)), med                                   # argmin: the first of equal minima, as `<` keeps it


def form_counts(inp):
    m = np.where(inp["lm_invalid"], 0, np.diff(inp["lm_obs_ptr"]))    # an invalid landmark is skipped by the narrowest form
    return np.bincount(np.searchsorted(FORM_LANES, m), minlength=len(FORM_LANES) + 1).astype(np.int32)


def refresh_exact(inp, scale_factor=2.0, num_octaves=1):
    L, ptr, okf = inp["L"], inp["lm_obs_ptr"], inp["obs_kf"]
    O = int(ptr[-1])
    has_desc = inp["obs_desc"] is not None
    scale = np.array([math.pow(float(scale_factor), float(l)) for l in range(64)])   # std::pow(scale_factor, l): libm's pow
    obs_lm = np.repeat(np.arange(L), np.diff(ptr))
    cand = ~inp["kf_invalid"][okf[:O]] & ~inp["lm_invalid"][obs_lm]
    out = dict(lm_desc_obs=np.full(L, -1, np.int32) if has_desc else None, lm_desc=np.zeros((L, 32), np.uint8) if has_desc else None,
               lm_normal=np.zeros((L, 3)), lm_min_distance=np.zeros(L), lm_max_distance=np.zeros(L), lm_status=np.zeros(L, np.int32),
               form_count=form_counts(inp))
    # unit vectors of every observation: v = pos - centre, u = v / sqrt((vx vx + vy vy) + vz vz)
    v = inp["lm_pos"][obs_lm] - inp["kf_center"][okf[:O]]
    with np.errstate(invalid="ignore", divide="ignore"):
        nrm = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
        u = v / nrm[:, None]
    # the sum in list order: position 0 of every list, then position 1, ... (one addition per landmark and step)
    s = np.zeros((L, 3))
    n = np.zeros(L, np.int64)
    where = np.arange(O) - ptr[:-1][obs_lm]
    for j in range(int(np.diff(ptr).max()) if L else 0):
        sel = np.flatnonzero((where == j) & cand)
        s[obs_lm[sel]] = s[obs_lm[sel]] + u[sel]
        n[obs_lm[sel]] += 1
    some = n > 0
    out["lm_normal"][some] = s[some] / n[some].astype(np.float64)[:, None]
    out["lm_status"][~some] |= 1
    ref = inp["lm_ref_obs"]
    hasref = ref >= 0
    out["lm_status"][~hasref] |= 2
    ro = (ptr[:-1] + ref)[hasref]
    pc = inp["lm_pos"][hasref] - inp["kf_center"][okf[ro]]
    dist = np.sqrt((pc[:, 0] * pc[:, 0] + pc[:, 1] * pc[:, 1]) + pc[:, 2] * pc[:, 2])
    maxd = dist * scale[inp["obs_octave"][ro]]
    out["lm_max_distance"][hasref] = maxd
    out["lm_min_distance"][hasref] = maxd / scale[num_octaves - 1]
    inv = inp["lm_invalid"]
    for k in ("lm_normal", "lm_min_distance", "lm_max_distance"):
        out[k][inv] = 0.0
    out["lm_status"][inv] = 4
    if has_desc:
        for l in np.flatnonzero(~inv):
            pos = np.flatnonzero(cand[ptr[l]:ptr[l + 1]])              # list positions of the candidates
            if len(pos) == 0:
                continue
            best, _ = choose_descriptor(inp["obs_desc"][ptr[l] + pos])
            out["lm_desc_obs"][l] = pos[best]
            out["lm_desc"][l] = inp["obs_desc"][ptr[l] + pos[best]]
    return out


def assert_same(got, ref, what=""):
    """Bit for bit: the doubles are compared as their 64-bit patterns (-0.0 is not 0.0)."""
    for k in OUTPUTS:
        if ref[k] is None:
            assert got[k] is None, (what, k)
            continue
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(ref[k])
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k, a.shape, b.shape, a.dtype, b.dtype)
        same = a.view(np.uint64) == b.view(np.uint64) if a.dtype == np.float64 else a == b
        bad = np.argwhere(~same)
        assert len(bad) == 0, (what, k, len(bad), bad[:4].tolist(), a[tuple(bad[0])], b[tuple(bad[0])])
    assert np.array_equal(got["form_count"], ref["form_count"]), (what, got["form_count"], ref["form_count"])
