"""Marginal covariances, host side: the C struct and the limits against the header, every refusal of covgpu_marginal_check
with its message (the check runs without a context or a device, like covgpu_prune_check and covgpu_match_float_check), the relative-pose
covariance helper against central differences of a numpy restatement of the between residual and against the oracle's between Jacobian, and
the three reference builders of tests/marginal_util.py against each other. No GPU.

The two refusals that depend on a context (a sharded context; a pose graph off the elimination tree) are made by the device calls and are
tested in tests/test_gpu_marginal.py.

Reference spread h (largest pairwise err among SuperLU, dense LU and dense Cholesky + Gram; must stay below 1e-6), measured on the CPU
for the three keyframes this file selects (the first, the middle and the last free one):
tiny visual-inertial mu 0: 5.0e-7; small visual-inertial mu 0: 1.6e-8; small visual-only mu 0: 1.5e-11.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from covins_amd import backend, capi
from oracle import covo
from tests import forms_util as fu
from tests import marginal_util as mu_

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_struct_and_limits_match_the_header(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "covgpu.h"\nint main(void) { printf("%zu %zu %zu %zu %d %d %d\\n", '
                   "sizeof(covgpu_marginal_t), offsetof(covgpu_marginal_t, block), offsetof(covgpu_marginal_t, cov), "
                   "offsetof(covgpu_marginal_t, stats), COVGPU_MARGINAL_MAX_KF, COVGPU_MARGINAL_MAX_COLS, COVGPU_MARGINAL_MFMA_COLS); return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    lim = backend.marginal_limits()
    assert got == [C.sizeof(capi.Marginal), capi.Marginal.block.offset, capi.Marginal.cov.offset, capi.Marginal.stats.offset,
                   lim["max_kf"], lim["max_cols"], lim["mfma_cols"]]
    assert lim["max_cols"] == 15 * lim["max_kf"] and lim["mfma_cols"] == 16 and lim["panel_rows"] == 128
    assert len(capi.MARGINAL_STATS) == 8


def test_the_check_header_needs_no_hip(tmp_path):
    """marginal_check.hpp is plain C++17: a host program includes it as it is (no HIP header, no device) and gets the library's messages."""
    src = tmp_path / "chk.cpp"
    src.write_text('#include <cstdio>\n#include "marginal_check.hpp"\nint main() { covgpu_problem p{}; covgpu_options o{}; covgpu_marginal_t m{}; '
                   'p.num_kf = 3; double c[36]; int32_t k[1] = {3}; m.num_kf = 1; m.kf = k; m.cov = c; '
                   'std::printf("%s|", covgpu::marginal_check(&p, &o, &m)); k[0] = 2; '
                   'std::printf("%d\\n", covgpu::marginal_check(&p, &o, &m) == nullptr); return 0; }\n')
    exe = tmp_path / "chk"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "covins_amd", "csrc"), str(src), "-o", str(exe)])
    assert subprocess.check_output([str(exe)]).decode().strip() == "keyframe index out of range|1"


def test_null_context_is_refused():
    s = capi.Marginal()
    o = backend.default_options()
    assert backend.lib().covgpu_marginal_resident(None, C.byref(o), C.byref(s)) == 1
    assert backend.lib().covgpu_last_error() == b"covgpu_marginal_resident: NULL context"
    assert backend.lib().covgpu_marginal_covariance(None, C.byref(o), None, 0, C.byref(s)) == 1
    assert backend.lib().covgpu_last_error() == b"covgpu_marginal_covariance: NULL context"


def _check(prob, kfs, block=0, mu=0.0, drop=(), opt=True):
    kf = np.ascontiguousarray(kfs, np.int32)
    cov = np.zeros((max(1, 15 * len(kf)),) * 2)
    s = capi.Marginal()
    s.num_kf = len(kf); s.kf = capi.iptr(kf); s.block = block; s.mu = mu; s.cov = capi.dptr(cov); s.stats = None
    for f in drop:
        setattr(s, f, None)
    o = backend.default_options()
    ps = prob.as_struct() if prob is not None else None
    rc = backend.lib().covgpu_marginal_check(C.byref(ps) if ps is not None else None, C.byref(o) if opt else None, C.byref(s))
    return rc, backend.lib().covgpu_last_error().decode()


def test_every_refusal_of_the_check_and_the_accepted_boundaries():
    prob = fu.point_problem(fu._pt("small", None, False, 0))
    free = [int(k) for k in np.flatnonzero(prob.kf_fixed == 0)]
    fixed = [int(k) for k in np.flatnonzero(prob.kf_fixed != 0)]
    lim = backend.marginal_limits()
    assert len(free) >= lim["max_kf"] + 1 and fixed, (len(free), fixed)
    # accepted: one keyframe, the limit's number, the first and the last index, both blocks, mu = 0 and a large one, no stats
    assert _check(prob, free[:1])[0] == 0
    assert _check(prob, free[:lim["max_kf"]], block=1)[0] == 0
    assert _check(prob, [free[-1], free[0]], block=1, mu=1e300)[0] == 0
    assert _check(prob, [k for k in (0, prob.K - 1) if k in free] or free[:1])[0] == 0

    def bad(msg, *a, **kw):
        rc, err = _check(*a, **kw)
        assert rc == 1 and err == "covgpu_marginal_check: " + msg, (msg, rc, err)

    bad("num_kf outside [1, COVGPU_MARGINAL_MAX_KF]", prob, [])
    bad("num_kf outside [1, COVGPU_MARGINAL_MAX_KF]", prob, free[:lim["max_kf"] + 1])
    bad("keyframe index out of range", prob, [free[0], prob.K])
    bad("keyframe index out of range", prob, [-1])
    bad("duplicate keyframe", prob, [free[0], free[1], free[0]])
    bad("a keyframe with a constant pose has no covariance", prob, [free[0], fixed[0]])
    bad("block outside {0, 1}", prob, free[:2], block=2)
    bad("block outside {0, 1}", prob, free[:2], block=-1)
    bad("mu negative or not finite", prob, free[:2], mu=-1e-300)
    bad("mu negative or not finite", prob, free[:2], mu=float("nan"))
    bad("mu negative or not finite", prob, free[:2], mu=float("inf"))
    bad("NULL cov", prob, free[:2], drop=("cov",))
    bad("NULL kf", prob, free[:2], drop=("kf",))
    bad("NULL problem or options", None, free[:2])
    bad("NULL problem or options", prob, free[:2], opt=False)
    assert backend.lib().covgpu_marginal_check(None, None, None) == 1


# ---- the between residual restated in numpy (R7: rotation rows first; q = [x, y, z, w] Hamilton; A.1: q <- q * exp(dtheta), p <- p + dp)
def _qmul(a, b):
    ax, ay, az, aw = a; bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz])


def _qconj(q):
    return np.array([-q[0], -q[1], -q[2], q[3]])


def _qexp(th):
    a = np.linalg.norm(th)
    return np.array([0.0, 0.0, 0.0, 1.0]) if a == 0.0 else np.concatenate([np.sin(a / 2) * th / a, [np.cos(a / 2)]])


def _rot(q):
    return backend._quat_rot(q)


def _residual(pi, pj, meas):
    er = _qmul(_qconj(meas[:4]), _qmul(_qconj(pi[:4]), pj[:4]))
    return np.concatenate([2.0 * er[:3], _rot(pi[:4]).T @ (pj[4:] - pi[4:]) - meas[4:]])


def _perturb(p, dx):
    return np.concatenate([_qmul(p[:4], _qexp(dx[:3])), p[4:] + dx[3:]])


def _relative(pi, pj):
    return np.concatenate([_qmul(_qconj(pi[:4]), pj[:4]), _rot(pi[:4]).T @ (pj[4:] - pi[4:])])


def _random_pose(rng):
    q = rng.normal(size=4); q /= np.linalg.norm(q)
    return np.concatenate([q, rng.normal(size=3) * 3.0])


def test_between_jacobian_against_central_differences():
    rng = np.random.default_rng(7)
    for _ in range(5):
        pi, pj = _random_pose(rng), _random_pose(rng)
        meas = _relative(pi, pj)
        assert np.abs(_residual(pi, pj, meas)).max() < 1e-14
        J = backend.between_jacobian(pi, pj)
        Jn = np.zeros((6, 12)); eps = 1e-6
        for c in range(12):
            dx = np.zeros(12); dx[c] = eps
            rp = _residual(_perturb(pi, dx[:6]), _perturb(pj, dx[6:]), meas)
            rm = _residual(_perturb(pi, -dx[:6]), _perturb(pj, -dx[6:]), meas)
            Jn[:, c] = (rp - rm) / (2 * eps)
        assert np.abs(J - Jn).max() < 1e-8, np.abs(J - Jn).max()   # central differences at 1e-6: O(eps^2) truncation + 1e-16 / eps rounding


def test_between_jacobian_against_the_oracle_and_the_covariance_product():
    p = mu_.pgo_problem("tiny").copy()
    assert p.E >= 2
    p.kf_fixed[:] = 0
    for e in range(p.E):
        p.edge_meas[e] = _relative(p.kf_pose[p.edge_i[e]], p.kf_pose[p.edge_j[e]])
        p.edge_sqrt_info[e] = np.eye(6).reshape(-1)
        p.edge_loss_a[e] = 0.0
    r, J, _ = covo.linearize_between(p, covo.default_options())
    assert np.abs(r).max() < 1e-12
    for e in range(min(p.E, 8)):
        Jb = backend.between_jacobian(p.kf_pose[p.edge_i[e]], p.kf_pose[p.edge_j[e]])
        assert np.abs(J[e].reshape(6, 12) - Jb).max() < 1e-12, e
    rng = np.random.default_rng(3)
    A = rng.normal(size=(12, 12)); S = A @ A.T
    pi, pj = p.kf_pose[p.edge_i[0]], p.kf_pose[p.edge_j[0]]
    Jb = backend.between_jacobian(pi, pj)
    R = backend.relative_pose_covariance(S, pi, pj)
    assert R.shape == (6, 6) and np.array_equal(R, R.T) and np.allclose(R, Jb @ S @ Jb.T, rtol=1e-13, atol=0)
    assert np.linalg.eigvalsh(R).min() > 0
    with pytest.raises(ValueError):
        backend.relative_pose_covariance(np.eye(6), pi, pj)


@pytest.mark.parametrize("name,vo", [("tiny", False), ("small", False), ("small", True)])
def test_reference_builders_agree(name, vo):
    pt = fu._pt(name, None, vo, 0)
    prob = fu.point_problem(pt)
    free = np.flatnonzero(prob.kf_fixed == 0)
    kfs = [int(free[0]), int(free[len(free) // 2]), int(free[-1])]
    ref = mu_.point_reference(pt, 0.0, kfs)
    assert set(ref) >= {"lu", "dense", "chol"}
    print(f"{pt.id}: n={ref['n']} h={ref['h']:.2e}")
    assert ref["h"] < 1e-6, ref["h"]
    for k in ("lu", "dense", "chol"):
        assert (np.diag(ref[k]) > 0).all()
    # a sub-selection in another order is the same numbers
    sub = mu_.take(ref["chol"], kfs, ref["D"], [kfs[2], kfs[0]], block_full=False)
    D = ref["D"]
    assert sub.shape == (12, 12) and sub[0, 0] == ref["chol"][2 * D, 2 * D] and sub[6, 0] == ref["chol"][0, 2 * D]
