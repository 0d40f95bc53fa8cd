"""Covariance of every observation, host side: the three host routes to an observation's 2x2 block and to its
pose-landmark cross block agree (the formula pinned without a device), 0 <= C_o <= I on every observation, the C struct and the limits
against the header, every refusal of covgpu_obscov_check with its message (the check runs without a context or a device), the check header
as plain C++17 and as a stand-alone program under the address and undefined-behaviour sanitizers; and why the GPU file holds the call's
own outputs, reassembled, relative to the absolute products (test_reassembly_is_good_to_the_absolute_products_only). No GPU.

The refusals that depend on a context (a pose graph, a sharded context, nothing uploaded) are made by the device calls and are tested in
tests/test_gpu_obscov.py.

Measured on the CPU (block / cross-block correlations, worst over the observations compared):
  cut problems at mu 1e-4   A-B (every observation): g4-L1 2.6e-13 / 0 (both observers constant), g8-L31 8.6e-12 / 1.8e-13,
                            g16-L15 3.2e-12 / 4.2e-13        A-C: 1.7e-13 / 0, 6.3e-12 / 6.4e-14, 1.5e-12 / 1.9e-14
  small (route B on the 1 131 observations of lmcov_util.sample_landmarks, route C on every 25th landmark: 2 614 observations)
                            A-B: vo mu 0 1.3e-11 / 8.4e-12, vo 1e-8 2.9e-11 / 3.8e-12, vi mu 0 5.5e-11 / 1.8e-9, vi 1e-8 1.1e-11 / 4.5e-10
                            A-C: 1.7e-11 / 7.3e-14, 1.3e-11 / 7.6e-14, 1.2e-12 / 8.4e-15, 1.2e-12 / 5.6e-15
Routes A and C share Sigma_pp and differ only in the 3x3 / 2x9 algebra: held to 1e-9 (the bound tests/test_lmcov_host.py gives that algebra:
3x3 factors of condition up to ~1e6 at 1e-16; route A also subtracts the cross terms from the large J_l Sigma_l J_l^T, which route C does
not). Routes A and B are two factorisations of matrices of condition ~1e9: held to 1e-6 — a dropped term or a wrong sign of the cross block
shows at 1e-3 and above. 0 <= C_o <= I is exact in theory at any mu >= 0 (H_mu >= J_o^T J_o); the slack is for rounding: measured, the
eigenvalues of route A's blocks lie in [8.2e-3, 1 - 2.5e-5] on every point (0.49 .. 0.76 on g4-L1), so the rounding never reached either
end; held to 1e-9, the bound of the algebra.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from covins_amd import backend, capi
from tests import forms_util as fu
from tests import lm_forms_util as lf
from tests import obscov_ref as orf
from tests import obscov_util as ou

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "covins_amd", "csrc")
TOL_ALGEBRA, TOL_FACTOR, TOL_PSD = 1e-9, 1e-6, 1e-9


def _layout(route):
    """The references' blocks have the shapes the library was built with (covgpu_obscov_limits): 2x2 and 6x3 doubles per observation."""
    lim = backend.obscov_limits()
    assert route["C"][0].size == lim["block_doubles"] and route["X"][0].size == lim["cross_doubles"]


def _agree(tag, ref, landmarks_c):
    lin, A = ref["lin"], ref["A"]
    _layout(A)
    rows_c = lin.obs_of(landmarks_c)
    Cc = orf.route_c(lin, landmarks_c)
    eC = orf.err_block(Cc["C"][rows_c], A["C"][rows_c], A["C"][rows_c]).max()
    xC = orf.err_cross(Cc["X"], A["X"], A, rows_c).max()
    lo, hi = ou.psd_slack(A["C"][ref["rows"]])
    print(f"{tag}: O={lin.prob.O} A-B on {len(ref['rows_b'])} observations block {ref['h']:.2e} cross {ref['hx']:.2e}   A-C on {len(rows_c)} "
          f"block {eC:.2e} cross {xC:.2e}   eigenvalues of C_o in [{lo:.2e}, 1 + {hi - 1:.2e}]")
    assert ref["h"] <= TOL_FACTOR and ref["hx"] <= TOL_FACTOR, (tag, ref["h"], ref["hx"])
    assert eC <= TOL_ALGEBRA and xC <= TOL_ALGEBRA, (tag, eC, xC)
    assert lo >= -TOL_PSD and hi <= 1.0 + TOL_PSD, (tag, lo, hi)
    return lin


@pytest.mark.parametrize("pt", [lf.POINTS[4][0], lf.POINTS[8][0], lf.POINTS[16][0]], ids=lambda p: p.id)
def test_the_three_routes_agree_on_the_cut_problems(pt):
    assert pt.id in ("g4-L1", "g8-L31", "g16-L15")
    prob = lf.build(pt, "pinhole").p
    ref = ou.reference(prob, True, lf.MU_STEP, key=("cut", pt.id))
    lin = _agree(pt.id, ref, None)
    assert lin.ok.all() and len(ref["rows"]) == len(ref["rows_b"]) == prob.O
    # constant observers occur (two constant keyframes per camera): their cross block is zeros, their block J_l Sigma_l J_l^T
    fx = np.flatnonzero(~lin.free_obs)
    if len(fx):
        assert not ref["A"]["X"][fx].any() and not ref["B"]["X"][fx].any()


@pytest.mark.parametrize("visual_only", [True, False], ids=["vo", "vi"])
@pytest.mark.parametrize("mu", [0.0, 1e-8])
def test_the_three_routes_agree_on_small(visual_only, mu):
    prob = fu.point_problem(fu._pt("small", None, visual_only, 0))
    ref = ou.reference(prob, visual_only, mu, key="small", sample=ou.lu.sample_landmarks(prob))
    lin = _agree(f"small {'vo' if visual_only else 'vi'} mu={mu:g}", ref, np.arange(0, prob.L, 25))
    assert lin.ok.all() and len(ref["rows"]) == prob.O and len(ref["rows_b"]) >= 64


def test_reassembly_is_good_to_the_absolute_products_only():
    """Why tests/test_gpu_obscov.py holds the call's own outputs, reassembled, relative to the largest |J| |Sigma| |J|^T: on the host alone,
    route C's blocks (Sigma_aa, Sigma_al, Sigma_l in doubles, no device) put back together as J Sigma J^T miss route C's own C_o by far more
    than rounding of the RESULT's terms allows where J_l Sigma_l J_l^T cancels (mu = 0, a landmark with little parallax), and stay within
    the bound relative to the absolute products. Points: the largest 8-wide cut problem with a landmark behind its observers at mu = 0 (h =
    1.7e-4: nearly singular), and at mu = 1e-4. Measured: plain 7.4e-7 and 1.2e-12, absolute 1.6e-16 and 1.8e-16 of the largest term."""
    from tests import lmcov_util as lu
    pt = lf.LARGE[8]
    b = lf.build(pt, "pinhole")
    taken = {v for k, v in b.special.items() if k != "behind_obs"}
    l = next(int(s) for s in np.nonzero(b.lengths == 9)[0] if int(s) not in taken)
    prob = lu.landmark_behind_its_observers(b.p, l)
    for mu in (0.0, lf.MU_STEP):
        lin = orf.ObsLinearisation(prob, True, mu)
        Cc = orf.route_c(lin)
        _layout(Cc)
        good = lin.obs_of()
        plain, ab = ou.reassembly(lin, good, Cc["Saa"][good], Cc["X"][good], Cc["Sl"][good], Cc["C"][good])
        print(f"{pt.id}-behind mu={mu:g}: route C reassembled from its own blocks: {plain:.2e} of the largest term as it comes out, {ab:.2e} of the "
              f"largest absolute product")
        assert ab <= ou.C_SELF * ou.H_FLOOR
        if mu == 0.0:
            assert plain > 100 * ou.C_SELF * ou.H_FLOOR      # the plain denominator cannot be met by exact blocks rounded to doubles


def test_struct_and_limits_match_the_header(tmp_path):
    fields = ("mu", "obs_cov", "cross_cov", "obs_res", "obs_ok", "lm_cov", "lm_ok", "kf_cov", "stats")
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "covgpu.h"\nint main(void) { printf("%zu", sizeof(covgpu_obscov_t));\n' +
                   "".join(f'printf(" %zu", offsetof(covgpu_obscov_t, {f}));\n' for f in fields) + 'printf("\\n"); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(capi.Obscov)] + [getattr(capi.Obscov, f).offset for f in fields]
    assert [f for f, _ in capi.Obscov._fields_] == list(fields)
    lim = backend.obscov_limits()
    assert lim == dict(max_group=16, threads=256, cross_doubles=18, block_doubles=4)
    assert lim["threads"] % lim["max_group"] == 0 and len(capi.OBSCOV_STATS) == 8
    assert lim["max_group"] == backend.lmcov_limits()["max_group"] and lim["threads"] == backend.lmcov_limits()["threads"]


def test_null_context_is_refused():
    s = capi.Obscov()
    o = backend.default_options()
    assert backend.lib().covgpu_observation_covariance_resident(None, C.byref(o), C.byref(s)) == 1
    assert backend.lib().covgpu_last_error() == b"covgpu_observation_covariance_resident: NULL context"
    assert backend.lib().covgpu_observation_covariance(None, C.byref(o), None, C.byref(s)) == 1
    assert backend.lib().covgpu_last_error() == b"covgpu_observation_covariance: NULL context"


def _check(prob, mu=0.0, drop=(), opt=True, request=True):
    O = prob.O if prob is not None else 1
    L = prob.L if prob is not None else 1
    K = prob.K if prob is not None else 1
    s, out, st = backend.Context._obscov(O, L, K, mu, True, True, True, True)
    for f in drop:
        setattr(s, f, None)
    o = backend.default_options()
    ps = prob.as_struct() if prob is not None else None
    rc = backend.lib().covgpu_obscov_check(C.byref(ps) if ps is not None else None, C.byref(o) if opt else None, C.byref(s) if request else None)
    return rc, backend.lib().covgpu_last_error().decode()


def test_every_refusal_of_the_check_and_the_accepted_boundaries():
    prob = fu.point_problem(fu._pt("small", None, False, 0))
    assert _check(prob)[0] == 0
    assert _check(prob, drop=("cross_cov", "obs_res", "lm_cov", "lm_ok", "kf_cov", "stats"))[0] == 0
    assert _check(prob, drop=("lm_cov",))[0] == 0          # lm_ok alone is accepted
    assert _check(prob, mu=1e300)[0] == 0

    def bad(msg, *a, **kw):
        rc, err = _check(*a, **kw)
        assert rc == 1 and err == "covgpu_obscov_check: " + msg, (msg, rc, err)

    bad("NULL obs_cov", prob, drop=("obs_cov",))
    bad("NULL obs_ok", prob, drop=("obs_ok",))
    bad("lm_cov without lm_ok", prob, drop=("lm_ok",))
    bad("mu negative or not finite", prob, mu=-1e-300)
    bad("mu negative or not finite", prob, mu=float("nan"))
    bad("mu negative or not finite", prob, mu=float("inf"))
    from tests import marginal_util as mu_
    bad("a problem without observations", mu_.pgo_problem("small"))
    bad("NULL problem or options", None)
    bad("NULL problem or options", prob, opt=False)
    bad("NULL request", prob, request=False)
    assert backend.lib().covgpu_obscov_check(None, None, None) == 1


def test_the_check_header_needs_no_hip(tmp_path):
    """obscov_check.hpp is plain C++17: a host program includes it as it is (no HIP header, no device) and gets the library's messages."""
    src = tmp_path / "chk.cpp"
    src.write_text('#include <cstdio>\n#include "obscov_check.hpp"\nint main() { covgpu_problem p{}; covgpu_options o{}; covgpu_obscov_t s{}; '
                   'p.num_lm = 2; p.num_obs = 4; double c[16]; unsigned char k[4]; s.obs_cov = c; '
                   'std::printf("%s|", covgpu::obscov_check(&p, &o, &s)); s.obs_ok = k; '
                   'std::printf("%d\\n", covgpu::obscov_check(&p, &o, &s) == nullptr); return 0; }\n')
    exe = tmp_path / "chk"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, str(src), "-o", str(exe)])
    assert subprocess.check_output([str(exe)]).decode().strip() == "NULL obs_ok|1"


def test_check_program_under_the_sanitizers(tmp_path):
    """tests/cpp/obscov_check_main.cpp: the check on valid and malformed requests as a program of its own, built with the address and the
    undefined-behaviour sanitizer and run directly."""
    exe = tmp_path / "obscov_check_main"
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "obscov_check_main.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    nf, np_ = "mu negative or not finite", "a problem without observations"
    want = {"plain": "ok", "with every output": "ok", "lm_ok alone": "ok", "lm_cov without lm_ok": "lm_cov without lm_ok", "large mu": "ok",
            "negative mu": nf, "nan mu": nf, "inf mu": nf, "null obs_cov": "NULL obs_cov", "null obs_ok": "NULL obs_ok", "no landmarks": np_,
            "no observations": np_, "request alone": "ok", "null problem": "NULL problem or options", "null options": "NULL problem or options",
            "null request": "NULL request", "restored": "ok"}
    got = dict(l.split(": ", 1) for l in r.stdout.strip().splitlines())
    assert got == want
