"""Covariance of every landmark, host side: the three host routes to a landmark's block agree (the formula and the damping
rule, pinned without a device), the C struct and the limits against the header, every refusal of covgpu_lmcov_check with its message (the
check runs without a context or a device), the check header as plain C++17 and as a stand-alone program under the address and
undefined-behaviour sanitizers, and the host plan's resolution of the covisible pairs restated on the plan arrays. No GPU.

The refusals that depend on a context (a pose graph, a sharded context, nothing uploaded) are made by the device calls and are tested in
tests/test_gpu_lmcov.py.

Measured on the CPU (small, every landmark): route A against route B (the dense inverse of the full 16 191 / 17 811-row matrix) and the kernel's
formula (route C, every 25th landmark) against route A; the figures are printed. Routes A and C share Sigma_pp and differ only in the 3x3
algebra, so they are held to 1e-9 of the block's largest entry (3x3 factors of condition up to ~1e6 at 1e-16); routes A and B are two
factorisations of matrices of condition ~1e9: held to 1e-6 — a wrong damping rule or a dropped term shows at 1e-3 and above.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from covins_amd import backend, capi
from tests import forms_util as fu
from tests import lmcov_ref as lr
from tests import lmcov_util as lu
from tests import selinv_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "covins_amd", "csrc")


@pytest.mark.parametrize("visual_only", [True, False], ids=["vo", "vi"])
@pytest.mark.parametrize("mu", [0.0, 1e-8])
def test_the_three_routes_agree_on_small(visual_only, mu):
    pt = fu._pt("small", None, visual_only, 0)
    prob = fu.point_problem(pt)
    ref = lu.reference(prob, visual_only, mu, key="small")
    lin = ref["lin"]
    assert lin.ok.all() and len(ref["checked"]) == prob.L
    every = np.arange(0, prob.L, 25)
    Cc = lr.route_c(lin, every)
    eC = lr.err(Cc[every], ref["A"][every], ref["A"][every]).max()
    print(f"small {'vo' if visual_only else 'vi'} mu={mu:g}: L={prob.L} spread A-B h={ref['h']:.2e}  A-C on {len(every)} landmarks {eC:.2e}")
    assert ref["h"] <= 1e-6 and eC <= 1e-9
    assert (np.diagonal(ref["A"], axis1=1, axis2=2) >= np.diagonal(lin.Hinv, axis1=1, axis2=2) * (1 - 1e-9)).all()
    from oracle import covo
    H_or = covo.landmark_hessians(prob, covo.default_options(visual_only=1 if visual_only else 0))
    assert np.abs(H_or - lin.H0).max() <= 1e-12 * np.abs(H_or).max()
    if mu > 0:
        # the damping rule against the oracle's: H_pp = S + sum W H_ll^-1 W^T, with the oracle's S(mu) and THIS file's H_ll(mu), may differ from
        # H_pp at mu = 0 on the diagonal only (the poses' own damping). A landmark damping other than the oracle's shows off the diagonal at
        # mu = 1e-8 of the entries; rounding (S is a difference of sums of ~1e3 terms) at 1e-13
        n, Hmu = lr._full_blocks(lin)
        n, H0 = lr._full_blocks(lu.reference(prob, visual_only, 0.0, key="small")["lin"])
        off = (Hmu - H0) - np.diag(np.diag(Hmu - H0))
        print(f"  damping rule: off-diagonal change of H_pp {np.abs(off).max() / np.abs(H0).max():.2e} of its largest entry")
        assert np.abs(off).max() <= 1e-11 * np.abs(H0).max()


def test_struct_and_limits_match_the_header(tmp_path):
    fields = ("mu", "lm_cov", "lm_ok", "kf_cov", "stats")
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "covgpu.h"\nint main(void) { printf("%zu", sizeof(covgpu_lmcov_t));\n' +
                   "".join(f'printf(" %zu", offsetof(covgpu_lmcov_t, {f}));\n' for f in fields) + 'printf("\\n"); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(capi.Lmcov)] + [getattr(capi.Lmcov, f).offset for f in fields]
    assert [f for f, _ in capi.Lmcov._fields_] == list(fields)
    lim = backend.lmcov_limits()
    assert lim == dict(max_group=16, threads=256, block_doubles=9)
    assert lim["threads"] % lim["max_group"] == 0 and len(capi.LMCOV_STATS) == 8
    for g in (4, 8, 16):
        assert g <= lim["max_group"]
    assert {backend.lm_group(o, 100) for o in (200, 500, 501, 800, 801, 5000)} == {4, 8, 16}


def test_null_context_is_refused():
    s = capi.Lmcov()
    o = backend.default_options()
    assert backend.lib().covgpu_landmark_covariance_resident(None, C.byref(o), C.byref(s)) == 1
    assert backend.lib().covgpu_last_error() == b"covgpu_landmark_covariance_resident: NULL context"
    assert backend.lib().covgpu_landmark_covariance(None, C.byref(o), None, C.byref(s)) == 1
    assert backend.lib().covgpu_last_error() == b"covgpu_landmark_covariance: NULL context"


def _check(prob, mu=0.0, drop=(), opt=True, request=True):
    L = prob.L if prob is not None else 1
    lm_cov = np.zeros((max(L, 1), 3, 3)); ok = np.zeros(max(L, 1), np.uint8); kf = np.zeros((prob.K if prob is not None else 1, 6, 6))
    st = np.zeros(8, np.int64)
    s = capi.Lmcov()
    s.mu = mu; s.lm_cov = capi.dptr(lm_cov); s.lm_ok = ok.ctypes.data_as(capi._bp); s.kf_cov = capi.dptr(kf); s.stats = st.ctypes.data_as(capi._lp)
    for f in drop:
        setattr(s, f, None)
    o = backend.default_options()
    ps = prob.as_struct() if prob is not None else None
    rc = backend.lib().covgpu_lmcov_check(C.byref(ps) if ps is not None else None, C.byref(o) if opt else None, C.byref(s) if request else None)
    return rc, backend.lib().covgpu_last_error().decode()


def test_every_refusal_of_the_check_and_the_accepted_boundaries():
    prob = fu.point_problem(fu._pt("small", None, False, 0))
    assert _check(prob)[0] == 0
    assert _check(prob, drop=("kf_cov", "stats"))[0] == 0
    assert _check(prob, mu=1e300)[0] == 0

    def bad(msg, *a, **kw):
        rc, err = _check(*a, **kw)
        assert rc == 1 and err == "covgpu_lmcov_check: " + msg, (msg, rc, err)

    bad("NULL lm_cov", prob, drop=("lm_cov",))
    bad("NULL lm_ok", prob, drop=("lm_ok",))
    bad("mu negative or not finite", prob, mu=-1e-300)
    bad("mu negative or not finite", prob, mu=float("nan"))
    bad("mu negative or not finite", prob, mu=float("inf"))
    from tests import marginal_util as mu_
    bad("a problem without landmarks", mu_.pgo_problem("small"))
    bad("NULL problem or options", None)
    bad("NULL problem or options", prob, opt=False)
    bad("NULL request", prob, request=False)
    assert backend.lib().covgpu_lmcov_check(None, None, None) == 1


def test_the_check_header_needs_no_hip(tmp_path):
    """lmcov_check.hpp is plain C++17: a host program includes it as it is (no HIP header, no device) and gets the library's messages."""
    src = tmp_path / "chk.cpp"
    src.write_text('#include <cstdio>\n#include "lmcov_check.hpp"\nint main() { covgpu_problem p{}; covgpu_options o{}; covgpu_lmcov_t s{}; '
                   'p.num_lm = 2; p.num_obs = 4; double c[18]; unsigned char k[2]; s.lm_cov = c; '
                   'std::printf("%s|", covgpu::lmcov_check(&p, &o, &s)); s.lm_ok = k; '
                   'std::printf("%d\\n", covgpu::lmcov_check(&p, &o, &s) == nullptr); return 0; }\n')
    exe = tmp_path / "chk"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, str(src), "-o", str(exe)])
    assert subprocess.check_output([str(exe)]).decode().strip() == "NULL lm_ok|1"


def test_check_program_under_the_sanitizers(tmp_path):
    """tests/cpp/lmcov_check_main.cpp: the check on valid and malformed requests as a program of its own, built with the address and the
    undefined-behaviour sanitizer."""
    exe = tmp_path / "lmcov_check_main"
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "lmcov_check_main.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    nf = "mu negative or not finite"
    want = {"plain": "ok", "with kf_cov and stats": "ok", "large mu": "ok", "negative mu": nf, "nan mu": nf, "inf mu": nf,
            "null lm_cov": "NULL lm_cov", "null lm_ok": "NULL lm_ok", "no landmarks": "a problem without landmarks",
            "no observations": "a problem without landmarks", "request alone": "ok", "null problem": "NULL problem or options",
            "null options": "NULL problem or options", "null request": "NULL request", "restored": "ok"}
    got = dict(l.split(": ", 1) for l in r.stdout.strip().splitlines())
    assert got == want


@pytest.mark.parametrize("leaf", [15, 0], ids=["leaf15", "default"])
def test_pair_resolution_restated_on_the_host_tables(leaf):
    """Every covisible pair of free keyframes and every free keyframe resolves by the rule of sel_want / sel_locate, and the 6x6 block read
    through the table out of the numpy Sigma of that front (tests/selinv_ref.py) is the dense inverse's block, to the bound of
    tests/test_selinv_host.py (100 max(h, 1e-13) in its metric, taken over the block)."""
    import scipy.linalg as sl
    pt = fu._pt("small", None, False, leaf)
    prob = fu.point_problem(pt)
    sysm = fu.host_system(pt, 0.0)
    S = sysm["S"].toarray(); D = sysm["D"]
    info, parent, level, own, st = fu.host_plan(pt)
    free = [int(k) for k in np.flatnonzero(prob.kf_fixed == 0)]
    pairs = lu.covisible_pairs(prob)
    assert len(pairs) > len(free)
    got_p, got_k = lu.resolve(level, own, st, D, pairs, free)
    assert all(g is not None for g in got_p), [pairs[i] for i, g in enumerate(got_p) if g is None][:5]
    assert all(g is not None for g in got_k)
    # both orientations occur: the row keyframe's pose before and behind the column keyframe's in the square, own x own and border x own
    assert any(r0 > q0 for f, r0, q0 in got_p) and any(r0 < q0 for f, r0, q0 in got_p)
    assert len({f for f, _, _ in got_p}) > 1
    inv = np.linalg.inv(S)
    Lc = np.linalg.cholesky(S)
    Y = sl.solve_triangular(Lc, np.eye(len(S)), lower=True, check_finite=False)
    d = sysm["d"]; w = np.outer(d, d)
    h = float(np.abs((inv - Y.T @ Y) * w).max() / np.abs(inv * w).max())
    squares = selinv_ref.selected_inverse(S, parent, level, own, st, D)
    worst, den = 0.0, float(np.abs(inv * w).max())
    for (i, j), (f, r0, q0) in list(zip(pairs, got_p)) + [((k, k), g) for k, g in zip(free, got_k)]:
        idx, Sig = squares[f]
        assert np.array_equal(idx[r0:r0 + 6], D * i + np.arange(6)) and np.array_equal(idx[q0:q0 + 6], D * j + np.arange(6))
        blk = Sig[r0:r0 + 6, q0:q0 + 6]
        want = inv[D * i:D * i + 6, D * j:D * j + 6]
        ww = np.outer(d[D * i:D * i + 6], d[D * j:D * j + 6])
        worst = max(worst, float(np.abs((blk - want) * ww).max()) / den)
    print(f"{pt.id}: {len(pairs)} pairs + {len(free)} keyframes over {len(squares)} fronts  h={h:.2e}  worst block {worst / max(h, 1e-13):.2f} h")
    assert worst <= 100 * max(h, 1e-13), (worst, h)
