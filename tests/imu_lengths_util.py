"""Two more points for the inertial path, shared by tests/test_imu_lengths_host.py and tests/test_gpu_imu_lengths.py: sample counts from 1 to 150 in one
problem. k_preintegrate runs one wave per factor and every wave its own sample count (no workgroup barrier); whatever it does in groups of samples
(a prefetch of the next sample, a chunk of lanes) meets a count just under, at and just over every power of two up to 128 here. No GPU code.

Built from imu_util's `ragged-fused` point (K = 23, I = 21): every factor is given the sample list and first sample of that point's one 150-sample factor,
then imu_util.with_factors keeps the first len(counts) factors and cuts factor q to counts[q] samples. The other keyframes are chains of their own, as at
imu_util's count-I points; the motion no longer matches the poses, which a linearisation does not mind.

  lengths-sorted     one factor per count of COUNTS, ascending: four full workgroups
  lengths-shuffled   COUNTS and EXTRA shuffled (seed 11): the four waves of every workgroup hold four different lengths, and the last workgroup of
                     the 18 factors has two live and two dead waves

The points are entered into imu_util's cache under these ids, so imu_util.build / host_reference and test_gpu_imu._hold serve them like the others.
"""
import numpy as np

from covins_amd import capi
from tests import imu_util as iu

COUNTS = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 150)   # (the kernel has no lane-per-sample chunk of its own to add)
EXTRA = (7, 50)
IDS = ("lengths-sorted", "lengths-shuffled")


def long_factor(p):
    n = np.diff(p.imu_sample_ptr)
    f = int(np.argmax(n))
    assert n[f] == 150 and (n == 150).sum() == 1
    return f


def all_factors_long(p):
    """`p` with the 150 samples (and the first sample) of its one 150-sample factor in every factor."""
    f = long_factor(p)
    rows = p.imu_samples[p.imu_sample_ptr[f]:p.imu_sample_ptr[f + 1]]
    d = dict(p.copy().__dict__)
    d.update(imu_samples=np.tile(rows, (p.I, 1)), imu_sample_ptr=150 * np.arange(p.I + 1, dtype=p.imu_sample_ptr.dtype),
             imu_first=np.tile(p.imu_first[f], (p.I, 1)))
    return capi.FlatProblem(**d)


def counts_of(pid):
    if pid == "lengths-sorted":
        return np.asarray(COUNTS, np.int64)
    assert pid == "lengths-shuffled"
    return np.random.default_rng(11).permutation(np.asarray(COUNTS + EXTRA, np.int64))


def build(pid):
    """The FlatProblem of `pid`; cached in imu_util's cache, treat as read-only."""
    if pid not in iu._cache:
        n = counts_of(pid)
        p = iu.with_factors(all_factors_long(iu.build("ragged-fused")), np.arange(len(n)), n)
        p.validate()
        iu._cache[pid] = p
    return iu._cache[pid]
