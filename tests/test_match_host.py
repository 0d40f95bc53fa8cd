"""Host side of the loop candidates' descriptor matching (covgpu_match_batch): the numpy restatement
(tests/match_ref.py) against match lists computed by the reference's own DenseMatcher (tests/golden/densematcher_ref.npz, made by
tools/make_ref_densematcher_fixture.py), the regenerated fixture inputs, the header's declarations, and the facade shim's compile."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import match_ref as mr
from tests import match_util as mu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIXTURE = os.path.join(HERE, "golden", "densematcher_ref.npz")


def fixture_cases():
    """Per fixture case: (A, B, skipA, skipB, digest, the reference's single-thread match list [(a, b, d)])."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("mk_dm", os.path.join(ROOT, "tools", "make_ref_densematcher_fixture.py"))
    mk = importlib.util.module_from_spec(spec); spec.loader.exec_module(mk)
    from covins_amd import synth
    z = np.load(FIXTURE)
    small = synth.make_map(synth.config_named("small"))
    out = []
    for i, (kind, seed, job) in enumerate(zip(z["kind"], z["seed"], z["job"])):
        A, B, sA, sB, dg = mk.case_inputs(str(kind), int(seed), int(job), small)
        m = z["matches"][int(z["ptr"][i]):int(z["ptr"][i + 1])]
        out.append((A, B, sA, sB, dg, str(z["digest"][i]), [(int(a), int(b), int(d)) for a, b, d in m]))
    return out, float(z["thr"])


@pytest.fixture(scope="module")
def cases():
    return fixture_cases()


def test_regenerated_inputs_hash_to_the_fixture_digest(cases):
    cs, _ = cases
    assert len(cs) >= 8
    for c in cs:
        assert c[4] == c[5]


def test_restatement_equals_the_reference_densematcher(cases):
    cs, thr = cases
    for A, B, sA, sB, _, _, ref in cs:
        assert mr.dense(A, B, sA, sB, thr) == ref


def test_restatement_eviction_and_ratio_examples():
    rng = np.random.default_rng(0)
    x = rng.integers(0, 256, 32, dtype=np.uint8)
    rows = [mu.at_dist(x, 10, rng)[0] for _ in range(5)] + [mu.at_dist(x, 5, rng)[0]]
    D = mr.hamming(x[None], np.stack(rows))
    lists = mr.dense_lists(D, np.zeros(1, bool), np.zeros(6, bool))
    assert [b for b, _ in lists[0]] == [5, 3, 2, 1]          # row 4 rejected (not < 10), row 0 evicted by row 5
    r1, used = mu.at_dist(x, 32, rng); r2, _ = mu.at_dist(x, 40, rng, avoid=used)
    assert mr.knn2(x[None], np.stack([r1, r2])) == []        # 32 < 0.8f * 40 is false in float32
    r1, used = mu.at_dist(x, 31, rng); r2, _ = mu.at_dist(x, 40, rng, avoid=used)
    assert mr.knn2(x[None], np.stack([r1, r2])) == [(0, 0, 31)]
    assert mr.knn2(x[None], x[None]) == []                   # one train row: no match
    assert mr.knn2(np.stack([x, x]), np.stack([x, x])) == []  # 0 < 0.8 * 0 is false


def test_header_declares_the_match_batch():
    h = open(os.path.join(ROOT, "include", "covgpu.h")).read()
    for name in ("covgpu_match_batch_t", "covgpu_match_opts", "covgpu_default_match_opts", "covgpu_match_batch"):
        assert name in h
    assert re.search(r"#define COVGPU_MATCH_DENSE 0\b", h) and re.search(r"#define COVGPU_MATCH_KNN2 1\b", h)
    assert re.search(r"#define COVGPU_MATCH_MAX_ROWS 4096\b", h)
    from covins_amd import capi
    assert (capi.MATCH_DENSE, capi.MATCH_KNN2, capi.MATCH_MAX_ROWS) == (0, 1, 4096)
    assert [f[0] for f in capi.MatchBatch._fields_] == ["num_sets", "row_ptr", "desc", "skip", "num_jobs", "set_a", "set_b", "match", "dist",
                                                        "nmatches"]


def test_default_match_opts():
    from covins_amd import backend, capi
    o = capi.MatchOpts()
    backend.lib().covgpu_default_match_opts(C.byref(o), capi.MATCH_DENSE)
    assert (o.mode, o.dist_threshold) == (0, 50.0)
    backend.lib().covgpu_default_match_opts(C.byref(o), capi.MATCH_KNN2)
    assert (o.mode, o.dist_threshold, o.ratio) == (1, 40.0, np.float32(0.8))


_SHIM = None


def match_shim():
    """tests/cpp/facade_match_shim.cpp: the facade's batched matcher on the stand-in map, descriptors through the optional trait."""
    global _SHIM
    if _SHIM is None:
        import subprocess
        so = os.path.join(HERE, "cpp", "libfacade_match_shim.so")
        srcs = [os.path.join(HERE, "cpp", f) for f in ("facade_match_shim.cpp", "facade_shim.cpp", "standin_map.hpp")] + \
               [os.path.join(ROOT, "include", "covins_gpu", "optimization_gpu.hpp"), os.path.join(ROOT, "include", "covgpu.h")]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", srcs[0], "-o", so, "-L" + os.path.join(ROOT, "covins_amd"),
                                   "-lcovgpu", "-Wl,-rpath," + os.path.join(ROOT, "covins_amd")])
        lib = C.CDLL(so)
        lib.shim_build.restype = C.c_void_p
        lib.shim_free.argtypes = [C.c_void_p]
        lib.match_set_descriptors.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint8), C.c_int, C.POINTER(C.c_int)]
        lib.match_candidates.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                         C.POINTER(C.c_int)]
        lib.match_candidates.restype = C.c_int
        _SHIM = lib
    return _SHIM


def test_facade_matcher_compiles():
    """The facade's LoopMatcherT instantiates on the stand-in map (tests/test_gpu_match.py drives it)."""
    assert match_shim().match_candidates is not None


_COVLIKE = None


def covins_like_lib():
    """tests/cpp/facade_match_covins_like.cpp: LoopMatcherT on COVINS-shaped classes (non-const GetLandmark / IsInvalid, cv::Mat-like
    descriptors_ / descriptors_add_ members) with no traits."""
    global _COVLIKE
    if _COVLIKE is None:
        import subprocess
        so = os.path.join(HERE, "cpp", "libfacade_match_covins_like.so")
        srcs = [os.path.join(HERE, "cpp", "facade_match_covins_like.cpp"), os.path.join(ROOT, "include", "covins_gpu", "optimization_gpu.hpp"),
                os.path.join(ROOT, "include", "covgpu.h")]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", srcs[0], "-o", so, "-L" + os.path.join(ROOT, "covins_amd"),
                                   "-lcovgpu", "-Wl,-rpath," + os.path.join(ROOT, "covins_amd")])
        lib = C.CDLL(so)
        lib.match_covins_like.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.c_int, C.POINTER(C.c_int),
                                          C.POINTER(C.c_int), C.POINTER(C.c_int)]
        lib.match_covins_like.restype = C.c_int
        _COVLIKE = lib
    return _COVLIKE


def test_facade_matcher_compiles_on_covins_shaped_classes_without_traits():
    """The default path (GetLandmark / IsInvalid non-const, descriptors read from the cv::Mat members) instantiates."""
    assert covins_like_lib().match_covins_like is not None
