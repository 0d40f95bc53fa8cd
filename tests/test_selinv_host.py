"""Covariance of every keyframe by selected inversion, host side: the C struct and the limits against the header, every
refusal of covgpu_selinv_check with its message (the check runs without a context or a device), the check header as plain C++17 and as a
stand-alone program under the address and undefined-behaviour sanitizers, and the recursion itself restated in numpy over the fronts of the
host plan (tests/selinv_ref.py) against the dense inverse of the oracle's system. No GPU.

The refusals that depend on a context (a sharded context; a pose graph off the elimination tree; nothing uploaded) are made by the device
calls and are tested in tests/test_gpu_selinv.py.

The numpy recursion against numpy.linalg.inv on every entry of every front's square, in the metric max |(A - B) o d d^T| / max |A o d d^T| with
d = sqrt(diag S) over the square: bound 100 max(h, 1e-13) with h the same metric between numpy.linalg.inv and the inverse from the dense Cholesky
factor over the whole matrix (two host routes to the same matrix). The factor 100 is the largest of the 10 / 30 / 100 of
tests/test_gpu_marginal.py, taken before measuring: a front's square is normalised by its own largest entry, h by the largest entry of the whole
inverse, so a square of small entries carries the same absolute error at a larger ratio. Measured on the CPU: small leaf 15 (184 fronts)
h 1.4e-8, worst square 2.04 h; small default plan (19 fronts) worst square 1.09 h.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from covins_amd import backend, capi
from tests import forms_util as fu
from tests import selinv_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "covins_amd", "csrc")


def test_struct_and_limits_match_the_header(tmp_path):
    fields = ("block", "mu", "kf_cov", "num_pairs", "pair_i", "pair_j", "pair_cov", "pair_ok", "stats")
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "covgpu.h"\nint main(void) { printf("%zu", sizeof(covgpu_selinv_t));\n' +
                   "".join(f'printf(" %zu", offsetof(covgpu_selinv_t, {f}));\n' for f in fields) +
                   'printf(" %d\\n", COVGPU_SELINV_MFMA_ROWS); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    lim = backend.selinv_limits()
    assert got == [C.sizeof(capi.Selinv)] + [getattr(capi.Selinv, f).offset for f in fields] + [lim["mfma_rows"]]
    assert [f for f, _ in capi.Selinv._fields_] == list(fields)
    assert lim["panel_cols"] == 128 and lim["block_rows"] == 16 and lim["mfma_rows"] >= 16
    assert len(capi.SELINV_STATS) == 8


def test_the_check_header_needs_no_hip(tmp_path):
    """selinv_check.hpp is plain C++17: a host program includes it as it is (no HIP header, no device) and gets the library's messages."""
    src = tmp_path / "chk.cpp"
    src.write_text('#include <cstdio>\n#include "selinv_check.hpp"\nint main() { covgpu_problem p{}; covgpu_options o{}; covgpu_selinv_t s{}; '
                   'p.num_kf = 3; double c[108]; s.kf_cov = c; s.block = 2; '
                   'std::printf("%s|", covgpu::selinv_check(&p, &o, &s)); s.block = 0; '
                   'std::printf("%d\\n", covgpu::selinv_check(&p, &o, &s) == nullptr); return 0; }\n')
    exe = tmp_path / "chk"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, str(src), "-o", str(exe)])
    assert subprocess.check_output([str(exe)]).decode().strip() == "block outside {0, 1}|1"


def test_null_context_is_refused():
    s = capi.Selinv()
    o = backend.default_options()
    assert backend.lib().covgpu_selected_inverse_resident(None, C.byref(o), C.byref(s)) == 1
    assert backend.lib().covgpu_last_error() == b"covgpu_selected_inverse_resident: NULL context"
    assert backend.lib().covgpu_selected_inverse(None, C.byref(o), None, 0, C.byref(s)) == 1
    assert backend.lib().covgpu_last_error() == b"covgpu_selected_inverse: NULL context"


def _check(prob, pairs=(), block=0, mu=0.0, drop=(), opt=True, num_pairs=None):
    pr = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    pi, pj = np.ascontiguousarray(pr[:, 0]), np.ascontiguousarray(pr[:, 1])
    K = prob.K if prob is not None else 1
    kf_cov = np.zeros((K, 15, 15)); pc = np.zeros((max(1, len(pr)), 15, 15)); ok = np.zeros(max(1, len(pr)), np.uint8)
    s = capi.Selinv()
    s.block = block; s.mu = mu; s.kf_cov = capi.dptr(kf_cov); s.num_pairs = len(pr) if num_pairs is None else num_pairs
    s.pair_i = capi.iptr(pi); s.pair_j = capi.iptr(pj); s.pair_cov = capi.dptr(pc); s.pair_ok = ok.ctypes.data_as(capi._bp); s.stats = None
    for f in drop:
        setattr(s, f, None)
    o = backend.default_options()
    ps = prob.as_struct() if prob is not None else None
    rc = backend.lib().covgpu_selinv_check(C.byref(ps) if ps is not None else None, C.byref(o) if opt else None, C.byref(s))
    return rc, backend.lib().covgpu_last_error().decode()


def test_every_refusal_of_the_check_and_the_accepted_boundaries():
    prob = fu.point_problem(fu._pt("small", None, False, 0))
    free = [int(k) for k in np.flatnonzero(prob.kf_fixed == 0)]
    fixed = [int(k) for k in np.flatnonzero(prob.kf_fixed != 0)]
    assert len(free) >= 3 and fixed
    # accepted: no pairs (with and without pair arrays), one pair, both orders of a pair and a repeated pair, both blocks, a large mu
    assert _check(prob)[0] == 0
    assert _check(prob, drop=("pair_i", "pair_j", "pair_cov", "pair_ok"))[0] == 0
    assert _check(prob, [(free[0], free[1])])[0] == 0
    assert _check(prob, [(free[0], free[-1]), (free[-1], free[0]), (free[0], free[-1])], block=1, mu=1e300)[0] == 0

    def bad(msg, *a, **kw):
        rc, err = _check(*a, **kw)
        assert rc == 1 and err == "covgpu_selinv_check: " + msg, (msg, rc, err)

    one = [(free[0], free[1])]
    bad("block outside {0, 1}", prob, one, block=2)
    bad("block outside {0, 1}", prob, one, block=-1)
    bad("mu negative or not finite", prob, one, mu=-1e-300)
    bad("mu negative or not finite", prob, one, mu=float("nan"))
    bad("mu negative or not finite", prob, one, mu=float("inf"))
    bad("NULL kf_cov", prob, one, drop=("kf_cov",))
    bad("negative num_pairs", prob, one, num_pairs=-1)
    for f in ("pair_i", "pair_j", "pair_cov", "pair_ok"):
        bad("num_pairs > 0 with a NULL pair array", prob, one, drop=(f,))
    bad("pair index out of range", prob, one + [(free[0], prob.K)])
    bad("pair index out of range", prob, [(-1, free[0])])
    bad("a pair of equal indices", prob, one + [(free[2], free[2])])
    bad("a keyframe with a constant pose in a pair", prob, [(free[0], fixed[0])])
    bad("a keyframe with a constant pose in a pair", prob, [(fixed[0], free[0])])
    bad("NULL problem or options", None, one)
    bad("NULL problem or options", prob, one, opt=False)
    assert backend.lib().covgpu_selinv_check(None, None, None) == 1


def test_check_program_under_the_sanitizers(tmp_path):
    """tests/cpp/selinv_check_main.cpp: the check on valid and malformed requests as a program of its own, built with the address and the
    undefined-behaviour sanitizer."""
    exe = tmp_path / "selinv_check_main"
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "selinv_check_main.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    want = {"no pairs": "ok", "three pairs": "ok", "large mu": "ok", "negative mu": "mu negative or not finite", "nan mu": "mu negative or not finite",
            "block 2": "block outside {0, 1}", "null kf_cov": "NULL kf_cov", "null pair_j": "num_pairs > 0 with a NULL pair array",
            "null pair_ok": "num_pairs > 0 with a NULL pair array", "index K": "pair index out of range", "index -1": "pair index out of range",
            "equal": "a pair of equal indices", "fixed": "a keyframe with a constant pose in a pair", "fixed unknown": "ok",
            "negative count": "negative num_pairs", "null problem": "NULL problem or options", "null request": "NULL request", "restored": "ok"}
    got = dict(l.split(": ", 1) for l in r.stdout.strip().splitlines())
    assert got == want


def test_relative_pose_covariances_apply_the_pair_helper():
    rng = np.random.default_rng(5)
    K = 4
    A = rng.normal(size=(6 * K, 6 * K)); Sig = A @ A.T
    poses = np.zeros((K, 7)); poses[:, :4] = rng.normal(size=(K, 4)); poses[:, :4] /= np.linalg.norm(poses[:, :4], axis=1)[:, None]
    poses[:, 4:] = rng.normal(size=(K, 3))
    kf_cov = np.stack([Sig[6 * k:6 * k + 6, 6 * k:6 * k + 6] for k in range(K)])
    pairs = [(0, 2), (3, 1), (1, 0)]
    pair_cov = np.stack([Sig[6 * i:6 * i + 6, 6 * j:6 * j + 6] for i, j in pairs])
    out = backend.relative_pose_covariances(kf_cov, pair_cov, pairs, poses, pair_ok=[1, 0, 1])
    assert out.shape == (3, 6, 6) and np.isnan(out[1]).all()
    for q in (0, 2):
        i, j = pairs[q]
        idx = np.r_[6 * i:6 * i + 6, 6 * j:6 * j + 6]
        assert np.array_equal(out[q], backend.relative_pose_covariance(Sig[np.ix_(idx, idx)], poses[i], poses[j]))


@pytest.mark.parametrize("leaf", [15, 0], ids=["leaf15", "default"])
def test_numpy_recursion_reproduces_the_dense_inverse(leaf):
    import scipy.linalg as sl
    pt = fu._pt("small", None, False, leaf)
    sysm = fu.host_system(pt, 0.0)
    S = sysm["S"].toarray()
    info, parent, level, own, st = fu.host_plan(pt)
    inv = np.linalg.inv(S)
    Lc = np.linalg.cholesky(S)
    Y = sl.solve_triangular(Lc, np.eye(len(S)), lower=True, check_finite=False)
    inv_c = Y.T @ Y
    d = sysm["d"]
    w = np.outer(d, d)
    h = float(np.abs((inv - inv_c) * w).max() / np.abs(inv * w).max())
    squares = selinv_ref.selected_inverse(S, parent, level, own, st, sysm["D"])
    covered = np.zeros(len(S), bool)
    worst = 0.0
    for idx, Sig in squares:
        ww = np.outer(d[idx], d[idx])
        want = inv[np.ix_(idx, idx)]
        worst = max(worst, float(np.abs((Sig - want) * ww).max() / np.abs(want * ww).max()))
        assert np.allclose(Sig, Sig.T, rtol=0, atol=1e-9 * np.abs(Sig).max())
        covered[idx] = True
    print(f"{pt.id}: n={len(S)} fronts={len(squares)} h={h:.2e} worst square {worst:.2e} ({worst / max(h, 1e-13):.2f} h)")
    assert covered.all()
    assert worst <= 100 * max(h, 1e-13), (worst, h)
