"""CPU side of the sample-count points (tests/imu_lengths_util.py; the device side is tests/test_gpu_imu_lengths.py). On the oracle and the long double
restatement alone:
  - the points are what their names say: the counts, four different lengths in every workgroup of the shuffled point, a partly dead last workgroup;
  - every factor of two samples or more has a positive-definite covariance and carries weight; the one-sample factor is weightless by rule and its
    W is exactly zero;
  - the oracle's own distance from the restatement stays under the bounds of tests/test_imu_host.py (PROJECT_BOUNDS, ORACLE_MARGIN floors): what the
    device test reads as e_orc is sound at 1 .. 150 samples too.
"""
import numpy as np
import pytest

from tests import imu_lengths_util as lu
from tests import imu_util as iu
from tests.test_imu_host import ORACLE_MARGIN, PROJECT_BOUNDS


def test_points_are_what_they_are_named_for():
    s, m = lu.build("lengths-sorted"), lu.build("lengths-shuffled")
    assert tuple(np.diff(s.imu_sample_ptr)) == lu.COUNTS and s.I == 16 and s.I % 4 == 0
    for c in (16, 32, 64, 128):                                          # a count under, at and over every power of two from 16 to 128
        assert {c - 1, c, c + 1} <= set(lu.COUNTS)
    assert {1, 2, 100, 150} <= set(lu.COUNTS)
    n = np.diff(m.imu_sample_ptr)
    assert sorted(n) == sorted(lu.COUNTS + lu.EXTRA) and m.I == 18 and m.I % 4 == 2     # the last workgroup: two live and two dead waves
    assert list(n) != sorted(n)
    for g in range(0, m.I, 4):
        assert len(set(n[g:g + 4])) == len(n[g:g + 4]), g                # different lengths in every workgroup
    assert any(n[g:g + 4].max() >= 100 and n[g:g + 4].min() <= 2 for g in range(0, m.I, 4))   # a long factor beside a very short one
    f = lu.long_factor(iu.build("ragged-fused"))
    src = iu.build("ragged-fused")
    rows = src.imu_samples[src.imu_sample_ptr[f]:src.imu_sample_ptr[f + 1]]
    for p in (s, m):
        assert np.all(p.imu_kf_j != p.imu_kf_i) and len(set(p.imu_kf_i)) == p.I
        for q in range(p.I):                                             # factor q: the first n_q samples of the 150-sample factor
            assert np.array_equal(p.imu_samples[p.imu_sample_ptr[q]:p.imu_sample_ptr[q + 1]], rows[:p.imu_sample_ptr[q + 1] - p.imu_sample_ptr[q]])
            assert np.array_equal(p.imu_first[q], src.imu_first[f])


@pytest.mark.parametrize("pid", lu.IDS)
def test_conditions_on_the_oracle(pid):
    p = lu.build(pid)
    h = iu.host_reference(pid)
    ref, fl = h["ref"], h["floor"]
    n = ref["n"]
    assert np.array_equal(n, np.diff(p.imu_sample_ptr)) and (n == 1).sum() == 1
    print(f"{pid}: oracle against restatement " + "  ".join(f"{k} {h['e_orc'][k]:.2e} ({(h['d_orc'][k] / np.maximum(fl[k], 1e-300)).max():.2f} floors)"
                                                             for k in iu.PRE_QUANTITIES + iu.WHITE_QUANTITIES))
    w = n < 2
    # two samples or more: positive definite (the long double factorisation exists, the double covariance of the oracle has positive eigenvalues), with weight
    assert np.isfinite(ref["cond"][~w]).all()
    P_orc = np.asarray(h["pre"][2]).reshape(p.I, 15, 15)
    for f in np.nonzero(~w)[0]:
        assert np.linalg.eigvalsh(0.5 * (P_orc[f] + P_orc[f].T)).min() > 0, f
        assert np.abs(ref["W"][f]).max() > 0
    assert np.all(np.abs(h["lin"][1][~w]).max(axis=1) > 0) and np.all(np.abs(h["lin"][0][~w]).max(axis=1) > 0)
    # one sample: weightless by rule, W exactly zero, on both sides
    assert not ref["W"][w].any() and not h["lin"][0][w].any() and not h["lin"][1][w].any()
    # the oracle's own distance: the suite's bounds
    for k, bound in PROJECT_BOUNDS.items():
        assert h["e_orc"][k] < bound, k
    for k in iu.PRE_QUANTITIES + iu.WHITE_QUANTITIES:
        assert np.all(h["d_orc"][k] <= ORACLE_MARGIN * fl[k]), (k, h["d_orc"][k], fl[k])
