"""CPU side of the inertial suite (tests/imu_util.py, tests/imu_ref.py; the device side is tests/test_gpu_imu.py):
  - every point of imu_util has the property it is named for;
  - the long double restatement of SURVEY.md A.4 against the oracle, factor by factor: covo.preintegrate and covo.linearize_imu on every point,
    covo_imu_residual on single factors linearised at biases that are not keyframe i's. The distances are what the device test reads as e_orc;
  - the restatement's own Jacobian against central differences of its own long double residual on bias-shift, so that a wrong bias-correction block
    cannot hide behind the agreement of two FP64 codes;
  - the rank argument of the one-sample rule on the restatement's covariance.

Observed (x86-64, 80-bit long double). Oracle against restatement, largest per-factor distance over all points: delta 5.6e-16, J 7.6e-16, P 3.0e-15,
whitened r 2.6e-13, J 1.4e-15, J^T J 2.8e-15, J^T r 3.5e-13; in units of the floors of imu_util.floors at most 0.29 (delta), 0.22 (J), 1.61 (P, a
one-sample factor: floor 2.2e-16), 0.07 (r), 0.11 (J^T r), below 0.005 (J, J^T J). cond(chol P) is 1.46e4 .. 1.65e4 at every point, agent B of
mixed-calib included (1.47e4). Central differences at a step of 1e-7: the exact Jacobian agrees to 1.5e-12 of the largest entry of its column block;
the first-order block d r_theta / d bg_i that the scheme states (and the product and the oracle compute) is off by 1.15e-3 of its own largest entry,
where h = J[R,BG] dbg / 2 reaches 1.15e-3 (dbg up to 0.01 rad/s across a factor of 0.25 s).
"""
import ctypes as C

import numpy as np
import pytest

from covins_amd import capi
from oracle import covo
from tests import imu_ref
from tests import imu_util as iu

LD = imu_ref.LD
ORACLE_MARGIN = 10          # the oracle evaluates the same recurrences in FP64: within 10 floors of the restatement, as the device is asked to be


def _lengths(pid):
    return np.diff(iu.build(pid).imu_sample_ptr)


# ------------------------------------------------------------------------------------------------ every point has its property
def test_base_is_the_map_the_points_assume():
    p = iu.base()
    assert (p.K, p.I, p.E) == (28, 26, 1) and list(np.nonzero(p.kf_fixed)[0]) == [0]
    assert np.all(np.diff(p.imu_sample_ptr) == 50)
    assert np.array_equal(p.imu_kf_i, np.arange(26)) and np.array_equal(p.imu_kf_j, np.arange(2, 28))
    perm = iu.chain_positions(p)
    assert np.array_equal(perm[0::2], np.arange(14)) and np.array_equal(perm[1::2], 14 + np.arange(14))        # two chains of 14, agents alternating
    db = np.abs(p.kf_speed_bias[p.imu_kf_i, 3:] - p.kf_speed_bias[p.imu_kf_j, 3:])
    assert db[:, :3].max() < 1e-4 and db[:, 3:].max() < 1e-6           # what the bias-correction terms meet without the shifted points:
    assert not db[1::2].any() and db[0::2].any()                       # exact zeros on agent B's factors, a random walk of 2e-5 / 1e-7 on agent A's
    assert p.edge_i[0] == 0 and abs(perm[p.edge_i[0]] - perm[p.edge_j[0]]) > 1


@pytest.mark.parametrize("pid", ["bias-shift", "bias-shift-one"])
def test_bias_shift_points(pid):
    p, b = iu.build(pid), iu.base()
    db = p.kf_speed_bias[p.imu_kf_i, 3:] - p.kf_speed_bias[p.imu_kf_j, 3:]
    if pid == "bias-shift":
        assert np.abs(db[:, :3]).max(axis=1).min() > 1e-3 and np.abs(db[:, 3:]).max(axis=1).min() > 1e-4       # across EVERY factor
        assert np.abs(db[:, :3]).max() <= 0.1 and np.abs(db[:, 3:]).max() <= 0.01
        assert len(np.unique(p.kf_speed_bias[:, 3])) == p.K                                                      # different for every keyframe
        dv = np.abs(p.kf_speed_bias[:, :3] - b.kf_speed_bias[:, :3])
        assert 0.01 < dv.max() <= 0.05
    else:
        k = iu.SHIFT_ONE_KF
        as_j, as_i = np.nonzero(p.imu_kf_j == k)[0], np.nonzero(p.imu_kf_i == k)[0]
        assert len(as_j) == 1 and len(as_i) == 1                                                                # the middle of a chain: both roles
        big = np.abs(db).max(axis=1) > 1e-3
        assert sorted(np.nonzero(big)[0]) == sorted([as_j[0], as_i[0]])
        assert np.allclose(db[as_i[0]], iu.SHIFT_ONE, atol=1e-4) and np.allclose(db[as_j[0]], -iu.SHIFT_ONE, atol=1e-4)
    # a shift of bias(i) leaves the factor's preintegration, linearised at bias(j), alone where bias(j) is not shifted
    assert np.array_equal(p.imu_samples, b.imu_samples) and np.array_equal(p.kf_pose, b.kf_pose)


def test_ragged_cut_lengths_per_workgroup():
    n = _lengths("ragged-cut")
    assert len(n) == 26 and len(n) % 4 == 2                             # the last workgroup: two live and two dead waves
    for g in range(0, 24, 4):
        assert len(set(n[g:g + 4])) == 4, g                             # four different lengths in every full workgroup
    assert n[24] != n[25]
    assert n.min() == 2 and n.max() == 50 and any({2, 50} <= set(n[g:g + 4]) for g in range(0, 24, 4))
    p, b = iu.build("ragged-cut"), iu.base()
    for f in (0, 3, 25):
        assert np.array_equal(p.imu_samples[p.imu_sample_ptr[f]:p.imu_sample_ptr[f + 1]], b.imu_samples[b.imu_sample_ptr[f]:b.imu_sample_ptr[f] + n[f]])


@pytest.mark.parametrize("n", iu.COUNTS)
def test_count_points(n):
    p = iu.build(f"count-{n}")
    assert p.I == n and [n % 4 for n in iu.COUNTS] == [1, 3, 0, 1]
    assert np.array_equal(np.diff(p.imu_sample_ptr), iu.cut_lengths(n))
    perm = iu.chain_positions(p)
    in_factor = np.zeros(p.K, bool); in_factor[p.imu_kf_i] = True; in_factor[p.imu_kf_j] = True
    assert (~in_factor).sum() == p.K - len(set(p.imu_kf_i) | set(p.imu_kf_j)) > 0      # keyframes no factor touches: chains of their own
    assert sorted(perm) == list(range(p.K))
    assert np.all(perm[p.imu_kf_j] == perm[p.imu_kf_i] + 1)


def test_ragged_fused_lengths():
    p = iu.build("ragged-fused")
    n = np.diff(p.imu_sample_ptr)
    assert p.K == 28 - len(iu.FUSED_ERASED) and p.I == p.K - 2 and p.E == 1
    assert sorted(n) == [50] * 17 + [100] * 3 + [150]
    assert any(len(set(n[g:g + 4])) > 1 for g in range(0, p.I, 4))
    # consistent data: the fused factors' whitened residuals stay those of the undisturbed map (173 at the perturbed estimate), where a cut sample
    # list leaves 2.9e5
    big = lambda pid: np.abs(iu.host_reference(pid)["lin"][0]).max()
    assert big("ragged-fused") <= big("edge-none") < 1e-2 * big("ragged-cut")


def test_mixed_calib_rows_differ_inside_every_workgroup():
    p, b = iu.build("mixed-calib"), iu.base()
    for g in range(0, p.I, 4):
        assert len({tuple(row) for row in p.imu_noise[g:g + 4]}) == 2, g
    odd = np.arange(p.I) % 2 == 1
    assert np.allclose(p.imu_noise[odd, :4], b.imu_noise[odd, :4] * iu.MIXED_B) and np.all(p.imu_noise[odd, 4] == iu.MIXED_B_GRAVITY)
    assert np.array_equal(p.imu_noise[~odd], b.imu_noise[~odd])
    c = iu.host_reference("mixed-calib")["ref"]["cond"]
    print(f"mixed-calib: cond(chol P_ref) agent A {c[~odd].min():.3e} .. {c[~odd].max():.3e}, agent B {c[odd].min():.3e} .. {c[odd].max():.3e}")


def test_fixed_inside_reaches_every_branch():
    p = iu.build("fixed-inside")
    fi, fj = p.kf_fixed[p.imu_kf_i] == 1, p.kf_fixed[p.imu_kf_j] == 1
    assert (fi & ~fj).sum() >= 2 and (~fi & fj).sum() >= 2 and (fi & fj).sum() == 1 and (~fi & ~fj).sum() > 10
    perm = iu.chain_positions(p)
    assert perm[12] == 6 and perm[27] == 27                              # the middle of chain A, the last keyframe of chain B
    both = np.nonzero(fi & fj)[0][0]
    assert (p.imu_kf_i[both], p.imu_kf_j[both]) == (9, 11)


def test_edge_points():
    b = iu.base()
    a, c = iu.beside_pair()
    p = iu.build("edge-beside")
    perm = iu.chain_positions(p)
    assert perm[c] == perm[a] + 1                                        # neighbouring chain positions: edge_beside_imu is set
    assert p.E == 3 and list(zip(p.edge_i[1:], p.edge_j[1:])) == [(a, c), (c, a)]
    assert not np.array_equal(p.edge_meas[1], p.edge_meas[2])
    p = iu.build("edge-far")
    perm = iu.chain_positions(p)
    assert p.E == 6 and np.abs(perm[p.edge_i] - perm[p.edge_j]).min() > 1          # no edge at distance 1: the one-launch branch
    deg = np.bincount(np.concatenate([p.edge_i, p.edge_j]), minlength=p.K)
    assert deg[3] == 4 and deg[20] == 3
    pairs = list(zip(p.edge_i, p.edge_j))
    assert (3, 20) in pairs and (20, 3) in pairs
    assert any(perm[i] > perm[j] for i, j in pairs) and any(perm[i] < perm[j] for i, j in pairs)       # both orientations against the position order
    for pid in iu.EDGE_IDS:
        p = iu.build(pid)
        assert np.all(p.edge_loss_a == 1.0) and np.all(p.edge_sqrt_info == p.edge_sqrt_info[0])
        r, _, _ = covo.linearize_between(p, covo.default_options(reproj_loss_a=1.0))
        assert 0.5 < np.abs(r[b.E:]).max(axis=1).min()                   # every added edge pulls (0.02 rad x 100, centimetres x 1e4, under the loss)
    q = iu.build("edge-none")
    assert q.E == 0 and q.I == b.I and np.array_equal(q.kf_pose, b.kf_pose)


def test_one_sample_point():
    n, r = _lengths("one-sample"), _lengths("ragged-cut")
    assert list(np.nonzero(n == 1)[0]) == list(iu.ONE_SAMPLE) == [0, 13, 25]           # the first, one inside a workgroup (13 = 4 * 3 + 1), the last
    keep = n != 1
    assert np.array_equal(n[keep], r[keep])


# ------------------------------------------------------------------------------------------------ the oracle against the restatement
PROJECT_BOUNDS = dict(delta=1e-12, J=1e-11, P=1e-11, r=1e-7, Jw=1e-7)     # per factor (tests/test_gpu_parity.py)


@pytest.mark.parametrize("pid", iu.IDS)
def test_oracle_against_restatement(pid):
    h = iu.host_reference(pid)
    fl = h["floor"]
    print(f"{pid}: oracle against restatement " + "  ".join(f"{k} {h['e_orc'][k]:.2e} ({(h['d_orc'][k] / np.maximum(fl[k], 1e-300)).max():.2f} floors)"
                                                             for k in iu.PRE_QUANTITIES + iu.WHITE_QUANTITIES))
    for k, bound in PROJECT_BOUNDS.items():
        assert h["e_orc"][k] < bound, k
    for k in iu.PRE_QUANTITIES + iu.WHITE_QUANTITIES:
        assert np.all(h["d_orc"][k] <= ORACLE_MARGIN * fl[k]), (k, h["d_orc"][k], fl[k])
    ref = h["ref"]
    assert np.abs(ref["delta"][:, 3:7] @ np.ones(4)).max() > 0 and np.allclose((ref["delta"][:, 3:7].astype(float) ** 2).sum(1), 1.0, atol=1e-15)
    assert np.isfinite(ref["cond"][ref["n"] >= 2]).all()                 # every factor of two samples or more has its whitening
    w = ref["n"] < 2
    assert not ref["W"][w].any() and not h["lin"][0][w].any() and not h["lin"][1][w].any()          # no weight by rule, exactly, on both sides
    assert np.all(np.abs(h["lin"][1][~w]).max(axis=1) > 0)


def _imu_residual(p, f, ba_lin, bg_lin, whiten):
    i, j = p.imu_kf_i[f], p.imu_kf_j[f]
    s = np.ascontiguousarray(p.imu_samples[p.imu_sample_ptr[f]:p.imu_sample_ptr[f + 1]])
    r, J, d = np.zeros(15), np.zeros(450), np.zeros(11)
    a = lambda x: capi.dptr(np.ascontiguousarray(x, dtype=np.float64))
    keep = [np.ascontiguousarray(x, dtype=np.float64) for x in (p.imu_first[f], ba_lin, bg_lin, p.imu_noise[f], p.kf_pose[i], p.kf_speed_bias[i], p.kf_pose[j],
                                                                p.kf_speed_bias[j])]
    covo.lib().covo_imu_residual(capi.dptr(keep[0]), capi.dptr(s), s.shape[0], *(capi.dptr(x) for x in keep[1:]), int(whiten), capi.dptr(r), capi.dptr(J),
                                 capi.dptr(d))
    return r, J.reshape(15, 30), d


@pytest.mark.parametrize("pid", ["bias-shift", "ragged-cut"])
def test_single_factors_linearised_away_from_bias_i(pid):
    """covo_imu_residual with (ba_lin, bg_lin) = keyframe j's bias reproduces covo.linearize_imu exactly (the factor is preintegrated there), and at a
    third bias (neither keyframe's) it is held to the restatement: the un-whitened u, A and the whitened r, J."""
    p, h = iu.build(pid), iu.host_reference(pid)
    rng = np.random.default_rng(9)
    worst = dict(u=0.0, A=0.0, r=0.0, J=0.0)
    for f in (0, 1, 6, 13, 25):
        i, j = p.imu_kf_i[f], p.imu_kf_j[f]
        r, J, _ = _imu_residual(p, f, p.kf_speed_bias[j, 3:6], p.kf_speed_bias[j, 6:9], 1)
        if not (p.kf_fixed[i] or p.kf_fixed[j]):
            assert np.array_equal(r, h["lin"][0][f]) and np.array_equal(J.reshape(-1), h["lin"][1][f])
        ba, bg = p.kf_speed_bias[i, 3:6] + rng.uniform(-0.05, 0.05, 3), p.kf_speed_bias[i, 6:9] + rng.uniform(-0.005, 0.005, 3)
        d, Jp, P = imu_ref.preintegrate(p.imu_first[f], p.imu_samples[p.imu_sample_ptr[f]:p.imu_sample_ptr[f + 1]], ba, bg, p.imu_noise[f])
        u0, A0 = imu_ref.unwhitened(d, Jp, ba, bg, p.kf_pose[i], p.kf_speed_bias[i], p.kf_pose[j], p.kf_speed_bias[j], p.imu_noise[f, 4])
        W = imu_ref.whitening(P, p.imu_sample_ptr[f + 1] - p.imu_sample_ptr[f])
        u, A, dd = _imu_residual(p, f, ba, bg, 0)
        r, J, _ = _imu_residual(p, f, ba, bg, 1)
        e = dict(u=iu.per_factor(u[None], u0[None])[0], A=iu.per_factor(A[None], A0[None])[0], r=iu.per_factor(r[None], (W @ u0)[None])[0],
                 J=iu.per_factor(J[None], (W @ A0)[None])[0])
        assert iu.per_factor(dd[None], d[None])[0] < 1e-12
        assert e["u"] < 1e-11 and e["A"] < 1e-12 and e["r"] < 1e-7 and e["J"] < 1e-7, (f, e)
        worst = {k: max(worst[k], e[k]) for k in e}
    print(f"{pid}: covo_imu_residual at a third bias against the restatement: " + "  ".join(f"{k} {v:.2e}" for k, v in worst.items()))


# ------------------------------------------------------------------------------------------------ the restatement against central differences
FD_STEP = LD(1e-7)


def _fd_jacobian(p, f, d, Jp, ba, bg):
    i, j = p.imu_kf_i[f], p.imu_kf_j[f]
    g = p.imu_noise[f, 4]
    x = [np.asarray(a, dtype=LD) for a in (p.kf_pose[i], p.kf_speed_bias[i], p.kf_pose[j], p.kf_speed_bias[j])]

    def u_at(which, delta):
        y = list(x)
        y[which] = imu_ref.pose_plus(x[which], delta) if which in (0, 2) else x[which] + delta
        return imu_ref.residual(d, Jp, ba, bg, *y, g)[0]

    A = np.zeros((15, 30), LD)
    for which, (c0, n) in enumerate(((0, 6), (6, 9), (15, 6), (21, 9))):
        for c in range(n):
            e = np.zeros(n, LD); e[c] = FD_STEP
            A[:, c0 + c] = (u_at(which, e) - u_at(which, -e)) / (2 * FD_STEP)
    return A


def test_restatement_jacobian_against_central_differences():
    """On bias-shift (dba up to 0.1 m/s^2, dbg up to 0.01 rad/s across a factor). A long double step of 1e-7 leaves truncation ~1e-14 and rounding
    ~1e-12: the exact Jacobian is held to 1e-10 of the largest entry of each column block. The block d r_theta / d bg_i as the scheme states it is the
    exact one without the factor (I - [h]x) / (1 + |h|^2): held to |h| (and shown to differ, so the comparison is not blind there)."""
    p, ref = iu.build("bias-shift"), iu.host_reference("bias-shift")["ref"]
    worst, worst_first, worst_h = 0.0, 0.0, 0.0
    for f in (2, 5, 12, 13, 24):
        i, j = p.imu_kf_i[f], p.imu_kf_j[f]
        ba, bg = p.kf_speed_bias[j, 3:6], p.kf_speed_bias[j, 6:9]
        d, Jp = ref["delta"][f], ref["J"][f]
        args = (d, Jp, ba, bg, p.kf_pose[i], p.kf_speed_bias[i], p.kf_pose[j], p.kf_speed_bias[j], p.imu_noise[f, 4])
        _, A_exact = imu_ref.unwhitened(*args, exact_bg=True)
        u, A_first = imu_ref.unwhitened(*args)
        assert np.array_equal(A_first, ref["A"][f]) and np.array_equal(u, ref["u"][f])
        fd = _fd_jacobian(p, f, d, Jp, ba, bg)
        for c0, c1 in ((0, 6), (6, 15), (15, 21), (21, 30)):
            worst = max(worst, float(np.abs(A_exact[:, c0:c1] - fd[:, c0:c1]).max() / np.abs(fd[:, c0:c1]).max()))
        blk = np.abs(fd[3:6, 12:15]).max()
        assert blk > 0.1                                                   # J[R,BG] ~ -dt: nothing small
        worst = max(worst, float(np.abs(A_exact[3:6, 12:15] - fd[3:6, 12:15]).max() / blk))         # the bias-correction block on its own scale
        diff = A_first - A_exact
        rest = diff.copy(); rest[3:6, 12:15] = 0
        assert not rest.any()                                              # the two statements differ in that block alone
        h = float(np.abs(Jp[3:6, 12:15] @ (np.asarray(p.kf_speed_bias[i, 6:9], dtype=LD) - bg) / 2).max())
        first = float(np.abs(A_first[3:6, 12:15] - fd[3:6, 12:15]).max() / blk)
        assert 0.05 * h < first < 3 * h, (first, h)
        worst_first, worst_h = max(worst_first, first), max(worst_h, h)
    print(f"central differences, step {float(FD_STEP):g}: exact Jacobian {worst:.2e} of the block's largest entry; first-order d r_theta / d bg block {worst_first:.2e} "
          f"(|h| up to {worst_h:.2e})")
    assert worst < 1e-10


# ------------------------------------------------------------------------------------------------ the one-sample rule
def test_one_sample_covariance_is_singular_by_construction():
    """After one midpoint step P = V N V^T, and the position rows of V are dt/2 times its velocity rows block for block: so are the rows of P, to the
    rounding of long double. The smallest pivot is then rounding, of either sign."""
    p, h = iu.build("one-sample"), iu.host_reference("one-sample")
    ref = h["ref"]
    for f in iu.ONE_SAMPLE:
        assert ref["n"][f] == 1
        P, dt = ref["P"][f], LD(p.imu_samples[p.imu_sample_ptr[f], 0])
        assert np.abs(P[0:3] - dt / 2 * P[6:9]).max() <= 8 * imu_ref.EPS_LD * np.abs(P[0:3]).max()
        ev = np.linalg.eigvalsh(P.astype(np.float64))
        assert abs(ev[0]) < 1e-15 * ev[-1]
        # delta, J, P of such a factor are ordinary numbers, and the oracle returns them
        for k, x in zip(iu.PRE_QUANTITIES, h["pre"]):
            assert iu.per_factor(x[f:f + 1], ref[k][f:f + 1])[0] < 1e-14
    # the oracle's solve leaves such factors out: the cost is that of the other factors
    o = covo.default_options()
    c = covo.cost(p, o)
    q = iu.with_factors(p, [f for f in range(p.I) if f not in iu.ONE_SAMPLE], np.delete(np.diff(p.imu_sample_ptr), list(iu.ONE_SAMPLE)))
    assert abs(c - covo.cost(q, o)) <= 1e-14 * c
