"""COVINS-G's 17-point stage, host side: the numpy checker tests/ncrelpose_ref.py against the truth of synthetic
two-rig scenes and against itself (two routes), the sampler against a C restatement, the loop and the covariance statuses with the
solver replaced, the C structures against the header, and every refusal of covgpu_ncrelpose_check through Python and through the
stand-alone program tests/cpp/ncrelpose_check_main.cpp under the address and undefined-behaviour sanitizers. No GPU.

The parity tolerance of the device tests is measured, not chosen: s_R [rad] and s_t are the largest differences between routes A (SVD)
and B (Householder QR, one-sided Jacobi, Newton polar factor: the kernel's formulation) on the separated tuples of
ncrelpose_util.standard(N); the device gets 10 s_R and 10 s_t. Measured on the CPU, 2000 tuples each: N = 17: 1941 separated (97.1 %),
s_R 2.3e-12, s_t 3.2e-12, route A against the truth 1.7e-12 / 2.1e-12; N = 24: 1999 separated, s_R 3.7e-14, s_t 1.1e-13."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from covins_amd import backend, capi
from tests import ncrelpose_ref as nr
from tests import ncrelpose_util as nu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "covins_amd", "csrc")


def test_struct_and_limits_match_the_header(tmp_path):
    bf = [f for f, _ in capi.NcrelposeBatch._fields_]
    of = [f for f, _ in capi.NcrelposeOpts._fields_]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "covgpu.h"\nint main(void) { printf("%zu %zu", sizeof(covgpu_ncrelpose_batch_t), '
                   'sizeof(covgpu_ncrelpose_opts));\n' + "".join(f'printf(" %zu", offsetof(covgpu_ncrelpose_batch_t, {f}));\n' for f in bf) +
                   "".join(f'printf(" %zu", offsetof(covgpu_ncrelpose_opts, {f}));\n' for f in of) +
                   'printf(" %d %d %d %d %d %d %d\\n", COVGPU_NCRELPOSE_FOUND, COVGPU_NCRELPOSE_TOO_FEW, COVGPU_NCRELPOSE_NO_MODEL, '
                   'COVGPU_NCRELPOSE_FEW_INLIERS, COVGPU_NCRELPOSE_THIN_CELL, COVGPU_NCRELPOSE_COV_INCOMPLETE, COVGPU_NCRELPOSE_COV_TRACE); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = [C.sizeof(capi.NcrelposeBatch), C.sizeof(capi.NcrelposeOpts)] + [getattr(capi.NcrelposeBatch, f).offset for f in bf] + \
           [getattr(capi.NcrelposeOpts, f).offset for f in of] + [0, 1, 2, 3, 4, 5, 6]
    assert got == want
    lim = backend.ncrelpose_limits()
    assert lim["sample"] == nr.SAMPLE == 17 and lim["hypotheses"] == 8 and lim["max_iterations"] == 100000 and lim["stage_cap"] >= 256
    assert lim["max_cells"] == 16 and lim["max_cov_iters"] == 256 and lim["max_rows"] == 64 and lim["polish_steps"] == nr.LM_ITERS
    o = capi.NcrelposeOpts()
    backend.lib().covgpu_default_ncrelpose_opts(C.byref(o))
    assert {k: getattr(o, k) for k in nr.DEFAULTS} == nr.DEFAULTS
    assert o.seed == 0 and o.stage_cap == 0


def test_sampler_matches_a_c_restatement(tmp_path):
    src = tmp_path / "draw.c"
    src.write_text(r'''#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
static uint64_t mix(uint64_t x) { uint64_t z = x + 0x9E3779B97F4A7C15ull; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
int main(int argc, char** argv) { uint64_t key = strtoull(argv[1], 0, 10); int n = atoi(argv[2]), cnt = atoi(argv[3]);
  int* a = malloc(sizeof(int) * n);
  for (int i = 0; i < n; ++i) a[i] = i;
  for (int k = 0; k < cnt; ++k) { int j = k + (int)(mix(key + k) % (uint64_t)(n - k)); int t = a[k]; a[k] = a[j]; a[j] = t; printf("%d ", a[k]); }
  printf("\n%llu\n", (unsigned long long)mix(key ^ 0x17C0F17C0F17C0F1ull)); free(a); return 0; }
''')
    exe = tmp_path / "draw"
    subprocess.check_call(["gcc", "-std=c99", "-O1", str(src), "-o", str(exe)])
    for key, n, cnt in ((0, 17, 17), (1, 18, 17), (12345678901234567890, 300, 17), ((1 << 64) - 3, 8, 4), (42, 513, 17), (7, 9, 4)):
        lines = subprocess.check_output([str(exe), str(key), str(n), str(cnt)]).decode().strip().split("\n")
        idx = nr.draw(key, cnt, n)
        assert idx == [int(x) for x in lines[0].split()]
        assert len(set(idx)) == cnt and all(0 <= i < n for i in idx)
        assert int(lines[1]) == nr.splitmix64(key ^ nr.COV_SALT)


@pytest.mark.parametrize("N,share", [(17, 0.90), (24, 0.99)])
def test_route_a_finds_the_truth_and_the_routes_agree(N, share):
    """The shares of separated tuples are conditions of the scene (measured 97.1 % and 100 %); on every separated tuple route A returns
    the true pose to 1e-10, and the A-B yardsticks stay where the docstring quotes them (within a factor of 10: they are maxima)."""
    tp, y = nu.standard(N)
    print(f"N {N}: separated {int(y['sep'].sum())} of {len(y['sep'])}  s_R {y['s_R']:.3e}  s_t {y['s_t']:.3e}  truth {y['truth_R']:.3e} {y['truth_t']:.3e}")
    assert y["sep"].mean() >= share
    assert y["truth_R"] < 1e-10 and y["truth_t"] < 1e-10
    q = {17: (2.3e-12, 3.2e-12), 24: (3.7e-14, 1.1e-13)}[N]
    assert q[0] / 10 < y["s_R"] < q[0] * 10 and q[1] / 10 < y["s_t"] < q[1] * 10
    sv_err = np.abs(y["svb"][y["sep"]] - y["sv"][y["sep"]]).max(0) / y["sv"][y["sep"], 0].max()
    assert sv_err[0] < 1e-13 and sv_err[1] < 1e-13


def test_score_and_threshold():
    assert abs(nr.threshold(1.5) - 2.0 * (1.0 - 1.0 / math.sqrt(1.0 + (1.5 / 800.0) ** 2))) < 1e-18
    j = nu.job(nu.split(60), 0.0, 0.0, 3)
    ry = nr.job_rays(j)
    assert nr.scores(j["R"], j["t"], ry).max() < 1e-14 and nr.cost(j["R"], j["t"], ry) < 1e-26
    assert not nr.inlier_mask(j["R"], j["t"], tuple(np.full_like(a, np.nan) for a in ry), 1.0).any()      # a non-finite score is no inlier


def test_loop_statuses_with_hand_built_hypotheses():
    """The loop itself, the solver replaced: n < 17; every draw failing stops after 10 max_iterations skipped draws; a model below
    min_inliers; no max_iterations status (RelNonCentralPosSolver.cpp:165)."""
    j = nu.job(nu.split(60), 0.25, 2e-4, 77)
    ry = nr.job_rays(j)
    th = nr.threshold(1.5)
    assert nr.ransac(nr.take(ry, np.arange(16)), 1, th)["status"] == 1
    r = nr.ransac(ry, 1, th, max_iterations=20, hypothesis=lambda d, idx: None)
    assert (r["status"], r["draws"], r["iterations"], r["best_draw"]) == (2, 200, 0, -1)
    good = (j["R"], j["t"])
    nin = int(nr.inlier_mask(j["R"], j["t"], ry, th).sum())
    assert 35 <= nin <= 52
    r = nr.ransac(ry, 1, th, min_inliers=nin + 1, hypothesis=lambda d, idx: good)
    assert r["status"] == 3 and r["inliers"] == nin and r["mask"].sum() == nin
    r = nr.ransac(ry, 1, th, min_inliers=nin, max_iterations=5, hypothesis=lambda d, idx: good)       # k > 5: the loop ends at 6, found all the same
    assert r["status"] == 0 and r["iterations"] == 6


def test_covariance_statuses_and_the_mean_it_uses():
    j = nu.job(nu.split(240), 0.15, 2e-4, 9)
    r = nr.run(j, 5, "a", min_inliers=40, max_iterations=300)
    assert r["status"] == 0 and r["rows"] == 30 and r["draws"] >= 30
    d = r["m"] - np.concatenate([np.zeros(3), r["T_s1s2"][1]])
    assert np.allclose(r["cov"], d.T @ d / 29.0, rtol=0, atol=1e-18) and not np.allclose(r["cov"], np.cov(r["m"].T))    # about (0, t_ref), not the sample mean
    assert nr.run(j, 5, "a", min_inliers=40, max_iterations=300, cov_iters=20, cov_max_iters=18)["status"] == 5
    assert nr.run(j, 5, "a", min_inliers=40, max_iterations=300, cov_thres=1e-12)["status"] == 6
    j4 = nu.job([7, 40, 40, 40, 40, 40], 0.1, 2e-4, 10)
    assert nr.run(j4, 5, "a", min_inliers=40, max_iterations=300)["status"] == 4
    assert max(nr.pose_error(*r["polished"], j["R"], j["t"])) < max(nr.pose_error(*r["ransac"], j["R"], j["t"]))


def _valid():
    j = nu.job(nu.split(24), 0.0, 0.0, 1)
    return nu.batch([j])


@pytest.mark.parametrize("change,opts,message", [
    (dict(ptr=[0, 23]), {}, "cell_ptr does not span the job"),
    (dict(ptr=[1, 24]), {}, "corr_ptr[0] != 0"),
    (dict(ptr=None, num=1), {}, "NULL array"),
    (dict(cell_ptr=None, cells=6), {}, "NULL array"),
    (dict(cell_ptr=[[0, 4, 3, 12, 16, 20, 24]]), {}, "cell_ptr not monotone"),
    (dict(cell_ptr=[[0] * 18], ptr=[0, 0]), {}, "cells outside 1..16"),
    (dict(bearing1=None), {}, "NULL correspondence array"),
    (dict(cam1=None), {}, "NULL correspondence array"),
    (dict(cam=None), {}, "NULL camera table"),
    (dict(cam2=np.full(24, 5, np.int32)), {}, "camera index out of range"),
    (dict(cam1=np.full(24, -1, np.int32)), {}, "camera index out of range"),
    (dict(bearing2=np.full((24, 3), np.nan)), {}, "non-finite bearing"),
    (dict(cam=np.full((5, 12), np.inf)), {}, "non-finite camera table"),
    (dict(T_sc_q=np.full((1, 7), np.nan)), {}, "non-finite extrinsics"),
    (dict(T_sc_c=np.zeros((1, 7))), {}, "zero quaternion in the extrinsics"),
    ({}, dict(max_iterations=0), "max_iterations outside 1..100000"),
    ({}, dict(max_iterations=100001), "max_iterations outside 1..100000"),
    ({}, dict(cov_iters=1), "cov_iters outside 2..256"),
    ({}, dict(cov_iters=257), "cov_iters outside 2..256"),
    ({}, dict(cov_max_iters=-1), "cov_max_iters < 0"),
    ({}, dict(probability=1.0), "probability outside (0, 1)"),
    ({}, dict(rp_error=0.0), "rp_error not finite or not positive"),
    ({}, dict(rp_error_cov=math.inf), "rp_error_cov not finite or not positive"),
    ({}, dict(cov_thres=math.nan), "cov_thres is NaN"),
    ({}, dict(stage_cap=-1), "stage_cap < 0"),
])
def test_check_refuses(change, opts, message):
    bt = _valid()
    bt.update(change)
    esc = message.replace("(", r"\(").replace(")", r"\)").replace("[", r"\[").replace("]", r"\]")
    with pytest.raises(backend.CovGpuError, match="covgpu_ncrelpose_check: " + esc):
        backend.ncrelpose_check(bt, **opts)


def test_check_accepts_and_null_arguments():
    backend.ncrelpose_check(_valid())
    backend.ncrelpose_check(_valid(), max_iterations=100000, cov_iters=256, seed=3, stage_cap=16)
    backend.ncrelpose_check(dict(ptr=[0]))                      # no jobs: nothing is read
    lib = backend.lib()
    o = capi.NcrelposeOpts()
    lib.covgpu_default_ncrelpose_opts(C.byref(o))
    assert lib.covgpu_ncrelpose_check(None, C.byref(o)) != 0 and b"NULL batch or options" in lib.covgpu_last_error()
    assert lib.covgpu_ncrelpose_check(C.byref(capi.NcrelposeBatch()), None) != 0
    assert lib.covgpu_ncrelpose_batch(None, C.byref(capi.NcrelposeBatch()), C.byref(o)) != 0
    assert lib.covgpu_last_error() == b"covgpu_ncrelpose_batch: NULL context"
    assert lib.covgpu_ncrelpose_solve_batch(None, 0, 17, None, None, None, None, None) != 0
    assert lib.covgpu_last_error() == b"covgpu_ncrelpose_solve_batch: NULL context"
    with pytest.raises(TypeError):
        backend.ncrelpose_check(_valid(), iterations=3)


def test_check_program_under_the_sanitizers(tmp_path):
    """tests/cpp/ncrelpose_check_main.cpp: the check on valid and malformed batches as a program of its own, built with the address and
    the undefined-behaviour sanitizer."""
    exe = tmp_path / "ncrelpose_check_main"
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "ncrelpose_check_main.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [ln.split(": ", 1) for ln in r.stdout.strip().split("\n")]
    plans = [v for k, v in got if k == "plan"]
    assert plans == ["20 5 20 5 6 %.17g %.17g" % (nr.threshold(1.5), nr.threshold(10.0)), "7 9"]
    lines = {k: v for k, v in got if k != "plan"}
    na, nc = "NULL array", "NULL correspondence array"
    want = {"valid": "ok", "seeds": "ok", "null batch": "NULL batch or options", "null options": "NULL batch or options", "negative num": "num < 0",
            "no jobs": "ok", "max_iterations 0": "max_iterations outside 1..100000", "max_iterations 100001": "max_iterations outside 1..100000",
            "max_iterations 100000": "ok", "cov_iters 1": "cov_iters outside 2..256", "cov_iters 257": "cov_iters outside 2..256", "cov_iters 256": "ok",
            "cov_iters 2": "ok", "cov_max_iters -1": "cov_max_iters < 0", "min_inliers -1": "min_inliers < 0", "stage_cap -1": "stage_cap < 0",
            "probability 0": "probability outside (0, 1)", "probability 1": "probability outside (0, 1)", "probability nan": "probability outside (0, 1)",
            "rp_error 0": "rp_error not finite or not positive", "rp_error nan": "rp_error not finite or not positive",
            "rp_error_cov negative": "rp_error_cov not finite or not positive", "rp_error_cov inf": "rp_error_cov not finite or not positive",
            "cov_thres nan": "cov_thres is NaN", "cells 0": "cells outside 1..16", "cells 17": "cells outside 1..16",
            "null corr_ptr": na, "null cell_ptr": na, "null cam_ptr": na, "null T_sc_q": na, "null cov": na, "null cov_draws": na,
            "null cam": "NULL camera table", "null bearing1": nc, "null cam2": nc, "null inlier": nc,
            "first not 0": "corr_ptr[0] != 0", "not monotone": "corr_ptr not monotone", "cam first not 0": "cam_ptr[0] != 0",
            "cam not monotone": "cam_ptr not monotone", "cell first not 0": "cell_ptr does not span the job", "cell short": "cell_ptr does not span the job",
            "cell not monotone": "cell_ptr not monotone", "cam1 too large": "camera index out of range", "cam2 negative": "camera index out of range",
            "nan camera": "non-finite camera table", "inf extrinsics": "non-finite extrinsics", "zero quaternion": "zero quaternion in the extrinsics",
            "nan bearing": "non-finite bearing", "inf bearing": "non-finite bearing", "restored": "ok", "solve n 0": "ok", "solve n -1": "n < 0",
            "solve N 16": "N outside 17..64", "solve N 65": "N outside 17..64", "solve null": "NULL array", "solve ok": "ok", "solve nan": "non-finite ray"}
    assert lines == want


def test_facade_ncrelpose_shim_compiles_and_seeds_differ_by_pair():
    """RelPoseSolverT's 17-point stage instantiates on a COVINS-G-shaped stand-in without traits (tests/cpp/facade_ncrelpose_shim.cpp;
    tests/test_gpu_ncrelpose_chain.py runs it); a job's seed comes from the two keyframes' ids and is none of the five-point cells' seeds."""
    lib = nu.facade_shim()
    sc = dict(row_ptr=np.arange(4, dtype=np.int32), desc=np.zeros((3, 32), np.uint8), bearing=np.ones((3, 3)), client=np.array([0, 1, 0], np.int32),
              pred=np.array([-1, 0, 1], np.int32), T_wc=np.tile(np.eye(4), (3, 1, 1)), T_cw=np.tile(np.eye(4), (3, 1, 1)))
    h = nu.shim_scene(lib, sc, np.tile(np.eye(4), (3, 1, 1)))
    s = {(a, b): lib.n17_seed(h, a, b) for a in range(3) for b in range(3) if a != b}
    assert len(set(s.values())) == 6 and s[(0, 1)] == lib.n17_seed(h, 0, 1)
    from tests import fivept_util as fu
    f5 = fu.facade_shim()
    h5 = f5.f5_build(3, sc["row_ptr"].ctypes.data_as(C.POINTER(C.c_int)), sc["desc"].ctypes.data_as(C.POINTER(C.c_ubyte)),
                     sc["bearing"].ctypes.data_as(C.POINTER(C.c_double)), sc["client"].ctypes.data_as(C.POINTER(C.c_int)),
                     sc["pred"].ctypes.data_as(C.POINTER(C.c_int)), sc["T_wc"].ctypes.data_as(C.POINTER(C.c_double)),
                     sc["T_cw"].ctypes.data_as(C.POINTER(C.c_double)))
    assert s[(0, 1)] not in {f5.f5_seed(h5, 0, 1, cell) for cell in range(6)}
    f5.f5_free(h5)
    lib.n17_free(h)
