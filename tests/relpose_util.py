"""Inputs that take covgpu_relpose_batch (covins_amd/csrc/k_relpose.hip) off the plain Gauss-Newton path and to the edges of its sizes.

tests/util.py::make_relpose_batch starts every pair 0.03 rad / 0.05 m from the truth: all its trust-region steps are accepted Gauss-Newton
steps. The regimes below replace that start (`perturbed`), the sizes, or the quaternion's scale, and `reference` runs the CPU oracle
(oracle/covo_relpose.cpp) on them pair by pair WITH its trace, so that a test can (a) prove which branches of the loop an input reaches
(tests/test_relpose_host.py) and (b) leave out of a device comparison the few pairs on which two correct implementations may decide
differently (`selected`).

Regimes (each for both distortion types; `regime(name, dist_type)`):
  near          0.03 rad / 0.05 m, n in 16..180: the control, what the suite tested before
  mid           0.6 rad / 1.0 m, n in 16..180: rejected steps, linearisation reuse, rho < 0.25
  far           1.0 rad / 2.0 m, n in 16..180: the above plus radius-limited steps and solves in which nothing projects
  wide          n = 300, all sigmas 2.0, 1.5..3 rad about a random axis, 0.5 m
  stride        n in {63, 64, 65, 127, 128, 129, 192, 193} (the kernel strides its 64 lanes over the correspondences), mid start
  few           n in {0, 1, 2, 3, 4}, min_inliers = 0, near start, empty pairs between non-empty ones
  unnormalised  T0 quaternions scaled by 0.5, 3, -1 and -3 (w < 0), near start, some pairs that fail the min_inliers gate
`gate_cases(dist_type)` gives pairs with the two thresholds that leave exactly min_inliers and min_inliers - 1 survivors.

Tolerance on T_AB. The kernel sums over 64 lanes and a butterfly, the oracle serially, and a trust-region loop that starts far away
amplifies that: the bound cannot be derived, so it is measured on the REFERENCE, never on the kernel. `python -m tests.relpose_util`
builds the oracle a second time with -O0 -ffp-contract=off (no FMA contraction, no vectorised sums; into oracle/_ref/), runs every regime
through both builds and prints, per regime, the largest |dT| over the selected pairs and whether any decision (inlier count, flag, trace
kind, accepted) differed. TOL = max(1e-9, 10 x spread): 10 for the kernel's different summation order, 1e-9 what
test_gpu_parity.py::test_batched_relative_pose_matches_oracle holds; a regime that needed more than 1e-6 would have to be shortened."""
from __future__ import annotations

import functools

import numpy as np

from tests.util import make_relpose_batch

TH = (0.9, 1.3)            # 0.9 removes correspondences, 1.3 is the reference's configured value
MIN_INLIERS = 12           # optimization_be.cpp:813
MAX_LEFT_OUT = 0.10        # of a regime's pairs
MARGIN = 1e-6
RAN_AWAY = 1e3

# Measured with `python -m tests.relpose_util` (both distortion types, both thresholds, selected pairs; x86-64, g++ -O3 -mavx2 -mfma against
# g++ -O0 -ffp-contract=off): largest |dT| between the two builds of the oracle. The two builds took the same decisions on every pair.
SPREAD = {"near": 1.3e-15, "mid": 2.2e-9, "far": 1.3e-8, "wide": 3.3e-9, "stride": 5.1e-12, "few": 2.1e-14, "unnormalised": 2.6e-15, "gate": 1.3e-15}
TOL = {k: max(1e-9, 10.0 * v) for k, v in SPREAD.items()}
assert max(TOL.values()) <= 1e-6
# `few`, n < 3 (rank-deficient up to the 1e-8 damping: T is not comparable): largest |d cost| between the two builds at the returned poses
FEW_COST_SPREAD = 4.4e-8
FEW_COST_TOL = max(1e-12, 10.0 * FEW_COST_SPREAD)

_SIZES = {"near": 60, "mid": 50, "far": 60, "wide": 40, "stride": 48, "few": 26, "unnormalised": 24}
STRIDE_N = (63, 64, 65, 127, 128, 129, 192, 193)
FEW_N = (3, 0, 1, 0, 0, 2, 4, 0, 1, 2, 3, 4, 0)      # empty pairs first-but-one, doubled, and last
UNNORMALISED_SCALE = (0.5, 3.0, -1.0, -3.0)


def perturbed(bt, rot_sigma, trans_sigma, seed, angle_range=None):
    """`bt` with T0 = truth (+) a perturbation of its own fixed seed: rotation vector N(0, rot_sigma) per axis (or, with `angle_range`, an
    angle uniform in that range about a uniformly random axis), translation N(0, trans_sigma) per axis. Quaternions with w >= 0."""
    from scipy.spatial.transform import Rotation as R
    rng = np.random.default_rng(seed)
    T0 = np.empty_like(bt["Ttrue"])
    for b, Tt in enumerate(bt["Ttrue"]):
        if angle_range is None:
            rv = rng.normal(0, rot_sigma, 3)
        else:
            ax = rng.normal(0, 1, 3)
            rv = ax / np.linalg.norm(ax) * rng.uniform(*angle_range)
        q = (R.from_quat(Tt[:4]) * R.from_rotvec(rv)).as_quat()
        T0[b, :4] = -q if q[3] < 0 else q
        T0[b, 4:] = Tt[4:] + rng.normal(0, trans_sigma, 3)
    return dict(bt, T0=T0)


def concat(batches):
    """One batch out of several (same cameras per pair as in the parts)."""
    out = {}
    for k in batches[0]:
        if k == "ptr":
            n = np.concatenate([np.diff(b["ptr"]) for b in batches])
            out[k] = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
        else:
            out[k] = np.ascontiguousarray(np.concatenate([b[k] for b in batches]))
    return out


def subbatch(bt, idx):
    """The pairs `idx` of `bt` as a batch of their own."""
    parts = []
    for b in idx:
        s = slice(bt["ptr"][b], bt["ptr"][b + 1])
        parts.append({k: np.array([0, s.stop - s.start], np.int32) if k == "ptr" else v[b:b + 1] if k in _PER_PAIR else v[s] for k, v in bt.items()})
    return concat(parts)


_PER_PAIR = ("camA", "camB", "distA", "distB", "T0", "Ttrue", "modelA", "modelB", "xiA", "xiB")


def _sized(ns, seed, dist_type, outlier_frac=0.1):
    return concat([make_relpose_batch(1, seed=seed + 1000 * i, nmin=n, nmax=n, outlier_frac=outlier_frac, dist_type=dist_type) for i, n in enumerate(ns)])


# (data seed, start seed) per regime and distortion type, chosen on the CPU so that every reach condition of tests/test_relpose_host.py and
# the selection cap hold
SEEDS = {("near", 0): (101, 201), ("near", 1): (102, 202), ("mid", 0): (111, 261), ("mid", 1): (150, 250), ("far", 0): (121, 261),
         ("far", 1): (122, 322), ("wide", 0): (131, 271), ("wide", 1): (134, 234), ("stride", 0): (141, 241), ("stride", 1): (142, 242),
         ("few", 0): (151, 251), ("few", 1): (152, 252), ("unnormalised", 0): (161, 261), ("unnormalised", 1): (162, 262)}


def build_regime(name, d, seed, start_seed):
    num = _SIZES[name]
    if name == "near":
        return perturbed(make_relpose_batch(num, seed=seed, dist_type=d), 0.03, 0.05, start_seed)
    if name == "mid":
        return perturbed(make_relpose_batch(num, seed=seed, dist_type=d), 0.6, 1.0, start_seed)
    if name == "far":
        return perturbed(make_relpose_batch(num, seed=seed, dist_type=d), 1.0, 2.0, start_seed)
    if name == "wide":
        bt = make_relpose_batch(num, seed=seed, nmin=300, nmax=300, dist_type=d)
        bt = dict(bt, sigA=np.full_like(bt["sigA"], 2.0), sigB=np.full_like(bt["sigB"], 2.0))
        return perturbed(bt, None, 0.5, start_seed, angle_range=(1.5, 3.0))
    if name == "stride":
        return perturbed(_sized(STRIDE_N * (num // len(STRIDE_N)), seed, d), 0.6, 1.0, start_seed)
    if name == "few":
        return perturbed(_sized(FEW_N * (num // len(FEW_N)), seed, d, outlier_frac=0.0), 0.03, 0.05, start_seed)
    if name == "unnormalised":
        bt = concat([make_relpose_batch(16, seed=seed, nmax=80, dist_type=d),
                     make_relpose_batch(8, seed=seed + 50, nmin=13, nmax=13, outlier_frac=0.6, dist_type=d)])   # (these miss the min_inliers gate at 0.9)
        bt = perturbed(bt, 0.03, 0.05, start_seed)
        T0 = bt["T0"].copy()
        T0[:, :4] *= np.array([UNNORMALISED_SCALE[b % 4] for b in range(num)])[:, None]
        return dict(bt, T0=T0)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def regime(name, dist_type):
    """The named regime's batch (dict as make_relpose_batch's; never modified: copy before changing)."""
    return build_regime(name, dist_type, *SEEDS[name, dist_type])


def min_inliers_of(name):
    return 0 if name == "few" else MIN_INLIERS


def pair_args(bt, b):
    """Positional arguments of covo.relpose / covo.relpose_cost (after T) for pair b."""
    s = slice(bt["ptr"][b], bt["ptr"][b + 1])
    return (bt["pB"][s], bt["pA"][s], bt["kpA"][s], bt["kpB"][s], bt["sigA"][s], bt["sigB"][s], bt["camA"][b], int(bt["distA"][b]),
            bt["camB"][b], int(bt["distB"][b]))


def run_oracle(bt, th, min_inliers):
    """covo.relpose with its trace on every pair: list of dict(n, T, out, rows, norms)."""
    from oracle import covo
    res = []
    for b in range(len(bt["ptr"]) - 1):
        n, T, out, tr = covo.relpose(*pair_args(bt, b), bt["T0"][b], th_outlier=th, min_inliers=min_inliers, trace=True)
        res.append(dict(n=n, T=T, out=out, **tr))
    return res


@functools.lru_cache(maxsize=None)
def reference(name, dist_type, th):
    """The oracle's results and traces for a regime, computed once per session. Not to be modified."""
    return run_oracle(regime(name, dist_type), th, min_inliers_of(name))


def col(rows, name):
    from oracle import covo
    return rows[:, covo.RELPOSE_TRACE_COLS.index(name)]


def kind_is(rows, column, name):
    from oracle import covo
    return col(rows, column) == covo.RELPOSE_KINDS.index(name)


def too_close_to_call(r, th):
    """True if the oracle's trace of one pair shows a decision that two correct implementations may take differently: a rho within 1e-6 of
    1e-3, 0.25 or 0.75; gn_norm within 1e-6 relative of the radius; the convergence test |cost - cost_new| <= 1e-6 cost within 1e-6 relative
    of equality; an outlier-pass norm within 1e-6 of the threshold. Also a solve that ran away (a coordinate of the returned pose beyond
    RAN_AWAY metres, seen in `far`): T is compared absolutely, and at 5e5 m two builds of the oracle itself are 6e-7 apart."""
    rows = r["rows"]
    if np.abs(r["T"]).max() > RAN_AWAY:
        return True
    rho = col(rows, "rho"); rho = rho[np.isfinite(rho)]
    if any((np.abs(rho - c) <= MARGIN).any() for c in (1e-3, 0.25, 0.75)):
        return True
    gn, rad = col(rows, "gn_norm"), col(rows, "radius")
    ok = np.isfinite(gn)
    if (np.abs(gn[ok] - rad[ok]) <= MARGIN * rad[ok]).any():
        return True
    acc = col(rows, "accepted") == 1
    dc, lim = np.abs(col(rows, "cost")[acc] - col(rows, "cost_new")[acc]), 1e-6 * col(rows, "cost")[acc]
    if (np.abs(dc - lim) <= MARGIN * lim).any():
        return True
    return bool((np.abs(r["norms"] - th) <= MARGIN).any())


def selection(results, th):
    """Mask of the pairs that enter a device comparison; asserts that at most 10 % are left out."""
    sel = np.array([not too_close_to_call(r, th) for r in results], bool)
    assert (~sel).sum() <= MAX_LEFT_OUT * len(sel), (int((~sel).sum()), len(sel))
    return sel


def selected(name, dist_type, th):
    return selection(reference(name, dist_type, th), th)


@functools.lru_cache(maxsize=None)
def gate_cases(dist_type, num=12):
    """(batch, [(b, th_in, th_out)]): for pair b of the batch exactly MIN_INLIERS correspondences survive the outlier pass at th_in and
    exactly MIN_INLIERS - 1 at th_out (its twin: the same pair one gap lower). Both thresholds lie in the middle of a gap between consecutive
    sorted residual norms of the oracle's trace (the larger of a correspondence's two norms decides); pairs with a gap below 1e-4 are not used."""
    bt = make_relpose_batch(num, seed=181 + dist_type, nmin=16, nmax=48, outlier_frac=0.3, dist_type=dist_type)
    cases = []
    for b, r in enumerate(run_oracle(bt, 1.0, MIN_INLIERS)):       # (the norms of the first solve do not depend on the threshold)
        m = np.sort(r["norms"].max(axis=1))
        M = MIN_INLIERS
        if m[M] - m[M - 1] >= 1e-4 and m[M - 1] - m[M - 2] >= 1e-4:
            cases.append((b, 0.5 * (m[M - 1] + m[M]), 0.5 * (m[M - 2] + m[M - 1])))
    return bt, cases


# ------------------------------------------------------------------------------------------------ the measurement behind SPREAD
def _second_build():
    """The oracle's relative-pose entry point compiled without optimisation and without contraction, as a callable like covo.relpose."""
    import ctypes as C
    import os
    import subprocess
    from oracle import covo
    here = os.path.dirname(os.path.abspath(covo.__file__))
    os.makedirs(os.path.join(here, "_ref"), exist_ok=True)
    so = os.path.join(here, "_ref", "libcovo_O0.so")
    subprocess.check_call(["g++", "-O0", "-ffp-contract=off", "-fopenmp", "-std=c++17", "-fPIC", "-shared", os.path.join(here, "covo_solver.cpp"),
                           os.path.join(here, "covo_relpose.cpp"), "-o", so])
    L = C.CDLL(so)
    L.covo_relpose_traced.argtypes = covo.lib().covo_relpose_traced.argtypes
    L.covo_relpose_cost.argtypes = covo.lib().covo_relpose_cost.argtypes
    L.covo_relpose_cost.restype = C.c_double
    return L


def _measure():
    from oracle import covo
    L = _second_build()
    first = covo.lib()
    few_cost = 0.0
    for name in list(_SIZES) + ["gate"]:
        spread, same, left_out, total = 0.0, True, 0, 0
        for d in (0, 1):
            if name == "gate":
                bt, cases = gate_cases(d)
                runs = [(bt, th, MIN_INLIERS, [b]) for b, th_in, th_out in cases for th in (th_in, th_out)]
            else:
                runs = [(regime(name, d), th, min_inliers_of(name), None) for th in TH]
            for bt, th, mi, only in runs:
                a = run_oracle(bt, th, mi)
                try:
                    covo._LIB = L
                    o = run_oracle(bt, th, mi)
                finally:
                    covo._LIB = first
                sel = np.array([not too_close_to_call(r, th) for r in a])
                left_out += int((~sel).sum()); total += len(sel)
                for b in (range(len(a)) if only is None else only):
                    if not sel[b]:
                        continue
                    ra, ro = a[b], o[b]
                    same &= ra["n"] == ro["n"] and np.array_equal(ra["out"], ro["out"]) and len(ra["rows"]) == len(ro["rows"]) and all(
                        np.array_equal(col(ra["rows"], c), col(ro["rows"], c)) for c in ("solve", "kind", "step", "accepted"))
                    if name == "few" and len(ra["out"]) < 3:
                        ca, co = (covo.relpose_cost(r["T"], *pair_args(bt, b), outlier=r["out"]) for r in (ra, ro))
                        few_cost = max(few_cost, abs(ca - co))
                    else:
                        spread = max(spread, float(np.abs(ra["T"] - ro["T"]).max()))
        print(f"{name:13s} spread {spread:.3e}  same decisions {bool(same)}  left out {left_out}/{total}")
    print(f"few, n < 3: cost spread {few_cost:.3e}")


if __name__ == "__main__":
    _measure()
