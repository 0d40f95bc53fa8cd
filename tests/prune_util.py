"""Inputs shared by tests/test_prune_host.py and tests/test_gpu_prune.py: the hand-built cases, the shapes that stress the kernel and
the synthetic maps, each with the options it is run with. Everything is seeded; prune_ref.prune_exact is computed once per case."""
import functools

import numpy as np

from covins_amd import synth
from tests import prune_ref as pr


def chain(K, tracks, dt=0.125, **flags):
    """K keyframes in one chain (0 is the agent's first, id_.first == 0), `tracks`: per landmark the list of observing keyframes."""
    ptr = np.concatenate([[0], np.cumsum([len(t) for t in tracks])]).astype(np.int32)
    obs = np.array([k for t in tracks for k in t], np.int32)
    first = np.zeros(K, bool); first[:1] = True
    first = flags.pop("kf_first", first)
    pred = np.arange(K) - 1
    succ = np.arange(K) + 1; succ[-1:] = -1
    return pr.make_inputs(ptr, obs, pred, succ, np.arange(K) * dt, kf_first=first, **flags)


def _flags(K, *on):
    f = np.zeros(K, bool); f[list(on)] = True
    return f


def hand_cases():
    """name -> (inputs, options). K <= 12. What each is for is asserted in tests/test_prune_host.py::test_hand_cases_do_what_they_are_for."""
    c = {}
    every = lambda ks, n: [list(ks)] * n
    # five landmarks seen by all six keyframes: candidates 1..4 all have value 1.0; erasing one brings n to 5, value 0.9 < 0.95
    c["ties"] = (chain(6, every(range(6), 5)), dict(th_red=0.95))
    # keyframe 2 sees nothing: den == 0, picked after 1 and 3 although its index lies between theirs
    c["den0"] = (chain(5, every((0, 1, 3, 4), 4)), dict(max_kfs=2))
    # a landmark of keyframes 1 and 2 only: erasing 1 takes it off den[2]
    c["two_to_one"] = (chain(5, every(range(5), 3) + [[1, 2]] + every((3, 4), 2)), dict(max_kfs=4))
    # one landmark per bucket edge, all seen by keyframes 1 and 2, the only candidates: n = 7, 6, 5, 4, 3, 2 each go down by one, twice
    c["buckets"] = (chain(9, [list(range(1, 1 + n)) for n in (7, 6, 5, 4, 3, 2)], kf_first=~_flags(9, 1, 2)), dict(max_kfs=7))
    # keyframes 0.5 s apart and a limit of 1.0: every span equals the limit, and the test is >=
    c["time_equal"] = (chain(6, every(range(6), 5), dt=0.5), dict(max_kfs=2, max_time_dist=1.0))
    c["time_below"] = (chain(6, every(range(6), 5), dt=0.5), dict(max_kfs=2, max_time_dist=1.0 + 2.0 ** -40))
    c["loop_kf"] = (chain(6, every(range(6), 5), kf_loop=_flags(6, 1, 3)), dict(th_red=0.85))
    c["not_erase"] = (chain(6, every(range(6), 5), kf_not_erase=_flags(6, 1)), dict(max_kfs=4))
    c["gates_together"] = (chain(6, every(range(6), 5), dt=0.5, kf_loop=_flags(6, 1, 2), kf_not_erase=_flags(6, 1, 3)), dict(max_kfs=0))
    # keyframe 2 is invalid but still listed as an observer; landmarks 0 and 1 are invalid
    c["invalid"] = (chain(8, every(range(8), 4) + every((1, 2, 3), 3) + [[2, 5]],
                          kf_invalid=_flags(8, 2), lm_invalid=[True, True] + [False] * 6), dict(max_kfs=4))
    c["count_stop"] = (chain(10, every(range(10), 3) + every((2, 3, 4), 2)), dict(max_kfs=7))
    c["threshold_round0"] = (chain(6, every(range(1, 4), 5)), dict(th_red=0.95))           # n = 3: every value is 0.4
    c["no_candidates"] = (chain(4, every(range(4), 3), kf_first=np.ones(4, bool)), dict(th_red=0.0))
    c["no_candidates_count"] = (chain(2, every(range(2), 3)), dict(max_kfs=0))
    c["max_rounds_1"] = (chain(8, every(range(8), 4)), dict(max_kfs=2, max_rounds=1))
    c["listed_twice"] = (chain(6, every(range(6), 2) + [[1, 1, 2], [1, 3, 3, 4], [2, 2]]), dict(max_kfs=3))
    c["no_landmarks"] = (chain(5, []), dict(max_kfs=3))
    c["threshold_no_landmarks"] = (chain(5, []), dict(th_red=0.0))
    return c


def empty_case():
    return pr.make_inputs(np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0))


def sparse_map(K=1100, L=6000, seed=3):
    """A random sparse map with tracks of 2..7 inside a window of 12 keyframes: more than one keyframe per thread in the argmax, K no
    multiple of 64, every bucket edge crossed many times."""
    rng = np.random.default_rng(seed)
    tracks = []
    for _ in range(L):
        s = int(rng.integers(0, K - 12))
        tracks.append(sorted(s + rng.choice(12, size=int(rng.integers(2, 8)), replace=False)))
    return chain(K, tracks, dt=0.0625)


def wide_keyframe():
    """Keyframe 3 sees 1500 landmarks, more than the workgroup has threads; each is shared with two to four of the others.
    Keyframes 3 and 5 are the candidates."""
    rng = np.random.default_rng(5)
    others = [1, 2, 4, 5, 6]
    tracks = [sorted([3] + list(rng.choice(others, size=int(rng.integers(2, 5)), replace=False))) for _ in range(1500)]
    return chain(8, tracks + [[1, 2, 4, 5, 6, 7]] * 40, kf_first=~_flags(8, 3, 5))


def dense_block():
    """64 keyframes that all see the same 300 landmarks: tracks longer than a wave, every counter hit by every landmark, every round
    changes every value."""
    return chain(66, [list(range(1, 65))] * 300, dt=2.0 ** -10)


@functools.lru_cache(maxsize=None)
def stress_cases():
    sp = sparse_map()
    return {"sparse_count": (sp, dict(max_kfs=550)), "sparse_threshold": (sp, dict(th_red=0.6)),
            "wide_keyframe": (wide_keyframe(), dict(max_kfs=6)), "dense_block": (dense_block(), dict(max_kfs=3))}


@functools.lru_cache(maxsize=None)
def stress_exact(name):
    inp, opts = stress_cases()[name]
    return pr.prune_exact(inp, **opts)


MAP_MODES = {"th095": dict(th_red=0.95), "th060": dict(th_red=0.6), "half": None}   # half: count mode at K/2


@functools.lru_cache(maxsize=None)
def map_inputs(name, thin):
    m = synth.make_map(synth.config_named(name))
    inp = pr.inputs_of_map(m)
    return pr.thinned(inp) if thin else inp


def map_case(name, thin, mode):
    inp = map_inputs(name, thin)
    return inp, (MAP_MODES[mode] or dict(max_kfs=inp["K"] // 2))


@functools.lru_cache(maxsize=None)
def map_exact(name, thin, mode):
    inp, opts = map_case(name, thin, mode)
    return pr.prune_exact(inp, **opts)


OUTPUTS = ("round_kf", "round_action", "num_rounds", "removed", "stop_reason", "kf_pred", "kf_succ", "lm_nobs", "red_num", "red_den")


def assert_same(got, ref, what=""):
    for k in OUTPUTS:
        assert np.array_equal(np.asarray(got[k]), np.asarray(ref[k])), (what, k, got[k], ref[k])


_SHIM = None


def prune_shim():
    """tests/cpp/facade_prune_shim.cpp: MapPruneT on the stand-in classes of tests/cpp/standin_prune.hpp, and the serial restatement."""
    global _SHIM
    if _SHIM is None:
        import ctypes as C
        import os
        import subprocess
        here = os.path.dirname(os.path.abspath(__file__)); root = os.path.dirname(here)
        so = os.path.join(here, "cpp", "libfacade_prune_shim.so")
        srcs = [os.path.join(here, "cpp", f) for f in ("facade_prune_shim.cpp", "standin_prune.hpp", "standin_map.hpp")] + \
               [os.path.join(root, "include", "covins_gpu", "optimization_gpu.hpp"), os.path.join(root, "include", "covgpu.h")]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", srcs[0], "-o", so, "-L" + os.path.join(root, "covins_amd"),
                                   "-lcovgpu", "-Wl,-rpath," + os.path.join(root, "covins_amd")])
        lib = C.CDLL(so)
        ip, dp, bp, vp = C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.c_void_p
        lib.prune_build.restype = vp
        lib.prune_build.argtypes = [C.c_int, ip, ip, bp, dp, bp, bp, ip, ip, C.POINTER(C.c_long), dp, dp, C.c_int, bp, ip, ip]
        lib.prune_free.argtypes = [vp]
        lib.prune_shutdown.argtypes = []
        lib.prune_facade.argtypes = [vp, C.c_double, C.c_int, C.c_double, ip, ip, ip]
        lib.prune_serial.argtypes = [vp, C.c_double, C.c_int, C.c_double, ip, ip, ip, dp]
        lib.prune_state.argtypes = [vp, bp, ip, ip, ip, dp, dp, ip, ip]
        _SHIM = lib
    return _SHIM


class StandinPruneMap:
    """A SlamMap as stand-in Map / Keyframe / Landmark objects; the keyframes of the map's loop constraints are its loop keyframes."""

    def __init__(self, m, kf_not_erase=None):
        import ctypes as C
        self.K = m.K
        inp = pr.inputs_of_map(m, kf_not_erase)
        u8 = lambda a: np.ascontiguousarray(a, dtype=np.uint8)
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
        f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
        k = [i32(m.kf_id), i32(m.kf_client), u8(m.kf_invalid), f64(m.kf_time), u8(inp["kf_loop"]), u8(inp["kf_not_erase"]), i32(m.kf_pred),
             i32(m.kf_succ), np.ascontiguousarray(m.imu_ptr, dtype=np.int64), f64(m.imu_samples), f64(m.imu_first), u8(m.lm_invalid),
             i32(m.lm_obs_ptr), i32(m.obs_kf)]
        t = [C.c_int, C.c_int, C.c_uint8, C.c_double, C.c_uint8, C.c_uint8, C.c_int, C.c_int, C.c_long, C.c_double, C.c_double, C.c_uint8,
             C.c_int, C.c_int]
        a = [p(x, y) for x, y in zip(k, t)]
        self.h = C.c_void_p(prune_shim().prune_build(m.K, *a[:11], m.L, *a[11:]))

    def close(self):
        if self.h:
            prune_shim().prune_free(self.h)
            self.h = None

    def _run(self, fn, th_red, max_kfs, max_time_dist, timed):
        import ctypes as C
        rk, ra = np.zeros(max(self.K, 1), np.int32), np.zeros(max(self.K, 1), np.int32)
        n, ms = C.c_int(0), C.c_double(0.0)
        ip = C.POINTER(C.c_int)
        args = [self.h, th_red, -1 if max_kfs is None else int(max_kfs), max_time_dist, rk.ctypes.data_as(ip), ra.ctypes.data_as(ip), C.byref(n)]
        removed = fn(*args, C.byref(ms)) if timed else fn(*args)
        return dict(round_kf=rk[:n.value].copy(), round_action=ra[:n.value].copy(), num_rounds=n.value, removed=int(removed), ms=ms.value)

    def facade(self, th_red=0.95, max_kfs=None, max_time_dist=1.0):
        """MapPruneT::RemoveRedundantData (one covgpu_prune_redundant call, then the erases replayed on the map)."""
        return self._run(prune_shim().prune_facade, th_red, max_kfs, max_time_dist, False)

    def serial(self, th_red=0.95, max_kfs=None, max_time_dist=1.0):
        """The serial restatement of the reference loop on the same map; `ms` is its wall time."""
        return self._run(prune_shim().prune_serial, th_red, max_kfs, max_time_dist, True)

    def state(self):
        import ctypes as C
        K = max(self.K, 1)
        out = dict(invalid=np.zeros(K, np.uint8), pred=np.zeros(K, np.int32), succ=np.zeros(K, np.int32), imu_count=np.zeros(K, np.int32),
                   imu_dt_sum=np.zeros(K), imu_first=np.zeros((K, 6)), num_landmarks=np.zeros(K, np.int32))
        n = C.c_int(0)
        ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
        prune_shim().prune_state(self.h, out["invalid"].ctypes.data_as(C.POINTER(C.c_uint8)), out["pred"].ctypes.data_as(ip),
                                 out["succ"].ctypes.data_as(ip), out["imu_count"].ctypes.data_as(ip), out["imu_dt_sum"].ctypes.data_as(dp),
                                 out["imu_first"].ctypes.data_as(dp), out["num_landmarks"].ctypes.data_as(ip), C.byref(n))
        out = {k: v[:self.K] for k, v in out.items()}
        out["db_erased"] = n.value
        return out
