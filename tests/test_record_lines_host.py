"""Host half of tests/test_gpu_record_lines.py: every point of tests/record_lines_util.py has the property it is named for, so that the device
test cannot quietly stop exercising a tail, an end of the record array or a kernel width when a generator or the width rule changes."""
import numpy as np
import pytest

from covins_amd import backend
from tests import record_lines_util as ru
from tests import structure_util as su


def _near(v, m):
    return {(-1, 0, 1)[k] for k in range(3) if any((x + (1, 0, -1)[k]) % m == 0 for x in v)}


def test_common_pairs_share_exactly_1_to_72_landmarks():
    b = ru.build(ru.BY_ID["common-1..72"])
    p = b.p
    W, _ = su.incidence(p)
    print(f"common-1..72: K={p.K} L={p.L} O={p.O}")
    assert (p.K, p.L, p.O) == (146, 2628, 7884)
    assert [int(W[a, c]) for a, c in b.info["pair_kf"]] == list(ru.COMMON_N)
    free = np.nonzero(p.kf_fixed == 0)[0]
    assert sorted(k for pr in b.info["pair_kf"] for k in pr) == free.tolist() and list(np.nonzero(p.kf_fixed)[0]) == list(ru.COMMON_FIXED)
    assert su.free_pairs(p, W) == len(ru.COMMON_N)                   # no pair of free keyframes besides the 72
    # every tail of a sixteen-term trip, up to five trips; the segment counts of one half (9 n) and of both (18 n) around the multiples of 16 and 64
    assert {n % 16 for n in ru.COMMON_N} == set(range(16)) and {-(-n // 16) for n in ru.COMMON_N} == {1, 2, 3, 4, 5}
    for m in (16, 64):
        assert _near([9 * n for n in ru.COMMON_N], m) == {-1, 0, 1}, m
        assert _near([18 * n for n in ru.COMMON_N], m) == {0}, m      # (18 n is even: never next to a multiple)


def test_slot_ends_owns_the_first_and_the_last_record():
    b = ru.build(ru.BY_ID["slot-ends"])
    p, lo, mid, hi = b.p, b.info["lo"], b.info["mid"], b.info["hi"]
    z = ru.slots_of(p)
    assert (lo, hi) == (0, p.K - 1) and not p.kf_fixed[[lo, mid, hi]].any() and hi == np.nonzero(p.kf_fixed == 0)[0].max()
    assert p.obs_kf[0] == lo and z[0] == 0                           # landmark 0 seen by keyframe 0: the first record
    assert p.obs_kf[p.O - 1] == hi and z[p.O - 1] == p.O - 1         # landmark L - 1 seen by the highest keyframe, which observes last: the last record
    ptr = p.lm_obs_ptr
    first, last = set(p.obs_kf[ptr[0]:ptr[1]].tolist()), set(p.obs_kf[ptr[p.L - 1]:ptr[p.L]].tolist())
    assert {lo, mid, hi} <= first and {lo, mid, hi} <= last
    W, _ = su.incidence(p)
    assert W[hi, lo] == ru.SLOT_MIDDLE + 2 and W[mid, lo] == 2 and W[hi, mid] == 2
    assert su.free_pairs(p, W) == 3
    print(f"slot-ends: K={p.K} L={p.L} O={p.O}; slots of landmark 0: {z[ptr[0]:ptr[1]].tolist()}, of landmark L-1: {z[ptr[p.L - 1]:ptr[p.L]].tolist()}")


def test_common_scattered_runs_against_the_index_order():
    b = ru.build(ru.BY_ID["common-scattered"])
    p, orig, maps = b.p, b.orig, b.maps
    W, _ = su.incidence(p)
    pairs = [(int(maps.kf[a]), int(maps.kf[c])) for a, c in b.info["pair_kf"]]
    assert [int(W[a, c]) for a, c in pairs] == list(ru.COMMON_N) and su.free_pairs(p, W) == len(ru.COMMON_N)
    up = sum(a < c for a, c in pairs)
    assert 10 < up < 62                                              # the first keyframe of a pair is the lower index in some, the higher in others
    ptr = p.lm_obs_ptr
    unsorted = sum(bool(np.any(np.diff(p.obs_kf[ptr[l]:ptr[l + 1]]) < 0)) for l in range(p.L))
    assert unsorted > p.L // 2                                       # tracks no longer sorted by keyframe
    obs_lm = np.repeat(np.arange(p.L), np.diff(ptr))
    a, c = pairs[-1]
    lms = np.intersect1d(obs_lm[p.obs_kf == a], obs_lm[p.obs_kf == c])
    assert len(lms) == 72 and lms.max() - lms.min() > p.L // 2       # the common landmarks of a pair are scattered over the landmark range
    assert (p.K, p.L, p.O) == (orig.K, orig.L, orig.O)
    print(f"common-scattered: {up} of 72 pairs listed lower keyframe first, {unsorted} of {p.L} tracks not sorted by keyframe")


@pytest.mark.parametrize("G", [4, 8, 16])
def test_stores_point_selects_its_width_and_mixes_its_tiles(G):
    p = ru.build(ru.BY_ID[f"stores-G{G}"]).p
    n = np.diff(p.lm_obs_ptr)
    groups = 256 // G
    print(f"stores-G{G}: K={p.K} L={p.L} O={p.O} O/L={p.O / p.L:.3f} -> {backend.lm_group(p.O, p.L)} lanes; workgroups {-(-p.L // groups)}")
    assert backend.lm_group(p.O, p.L) == G
    assert set(range(2, 4 * G + 2)) <= set(n.tolist()) and n.max() == 4 * G + 1 and np.array_equal(n, ru.stores_lengths(G))
    assert p.L % groups == 1 and p.L > groups                        # more than one workgroup, the last with one landmark and empty groups
    # a wave holds 64 / G landmarks: some wave's first chunk mixes full, partial and (behind the last landmark) empty records
    per_wave = 64 // G
    kinds = set()
    for w0 in range(0, p.L, per_wave):
        m = n[w0:w0 + per_wave]
        kinds.add((bool((m >= G).any()), bool((m < G).any()), len(m) < per_wave))
    assert any(f and part for f, part, _ in kinds) and any(e for _, _, e in kinds)
    assert not p.kf_fixed[p.K - 1] and p.kf_fixed.sum() == 2


@pytest.mark.parametrize("pt", ru.POINTS, ids=ru.IDS)
def test_golden_file_covers_the_point(pt):
    """tests/golden/record_lines_parent.npz (tools/make_record_lines_golden.py, run at the commit it names) holds every array the device test compares."""
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", ru.GOLDEN)
    assert os.path.getsize(path) < 1000000
    with np.load(path) as z:
        names = set(z.files)
        assert len(str(z["parent_commit"])) == 40
        p = ru.build(pt).p
        for mu in ru.MUS_SCHUR:
            k = f"{pt.id}/mu={mu:g}/"
            assert {k + "S_sha256", k + "b", k + "cost"} <= names and z[k + "b"].shape == (6 * p.K,)
            assert ((k + "S_blocks") in names) == (mu in ru.GOLDEN_FULL_S[pt.id])
        assert z[f"{pt.id}/step/dx"].shape == (6 * p.K,) and z[f"{pt.id}/step/dl"].shape == (p.L, 3)
