"""Inputs shared by tests/test_lmrefresh_host.py and tests/test_gpu_lmrefresh.py: hand-built landmarks, one batch with
every track length at which the kernel takes another path, a shuffled batch of mixed lengths, the synthetic maps with descriptors made
as tests/guided_util.map_keyframes makes them (noisy copies of a per-landmark pattern: tied medians abound), a writer of saved maps
with descriptors, and the C++ shim. Everything is seeded; lmrefresh_ref.refresh_exact is computed once per case."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

from covins_amd import backend, mapio, optimization, synth
from tests import lmrefresh_ref as lr
from tests.match_util import at_dist, flip


@functools.lru_cache(maxsize=None)
def limits():
    """(longest list of the lane-group forms, wave size, workgroup size of the long form, descriptors it stages in LDS) as built."""
    out = np.zeros(4, np.int32)
    backend.lib().covgpu_landmark_refresh_limits(out.ctypes.data_as(C.POINTER(C.c_int32)))
    return tuple(int(x) for x in out)


class Builder:
    """Landmarks one at a time over K keyframes with random centres (|c| of a few metres, landmarks some 20 m away)."""

    def __init__(self, K, seed=0):
        self.rng = np.random.default_rng(seed)
        self.K = K
        self.center = self.rng.normal(size=(K, 3)) * 3.0
        self.kfs, self.desc, self.oct, self.ref, self.pos, self.inv, self.names = [], [], [], [], [], [], {}

    def add(self, kfs, desc=None, ref=0, octave=None, invalid=False, name=None, p=None):
        """kfs: the observing keyframes in list order. desc [n,32] (default: noisy copies of a fresh pattern, bit flip probability p)."""
        n = len(kfs)
        if desc is None:
            pat = self.rng.integers(0, 256, (1, 32), dtype=np.uint8)
            desc = flip(np.repeat(pat, n, 0), self.rng.uniform(0.02, 0.12) if p is None else p, self.rng) if n else np.zeros((0, 32), np.uint8)
        self.kfs.append(np.asarray(kfs, np.int32)); self.desc.append(np.asarray(desc, np.uint8).reshape(n, 32))
        self.oct.append(np.zeros(n, np.int32) if octave is None else np.asarray(octave, np.int32))
        self.ref.append(ref if n else -1); self.inv.append(invalid)
        self.pos.append(self.rng.normal(size=3) * 4.0 + np.array([0.0, 0.0, 20.0]))
        if name:
            self.names[name] = len(self.kfs) - 1
        return len(self.kfs) - 1

    def track(self, n, **kw):
        """A landmark seen by n distinct keyframes in random order, a random one of them its reference."""
        kfs = self.rng.choice(self.K, n, replace=False)
        return self.add(kfs, ref=int(self.rng.integers(n)) if n else -1, **kw)

    def inputs(self, kf_invalid=(), with_desc=True, order=None):
        L = len(self.kfs)
        order = np.arange(L) if order is None else np.asarray(order)
        pick = lambda a: [a[i] for i in order]
        kfs, desc, octs = pick(self.kfs), pick(self.desc), pick(self.oct)
        ptr = np.concatenate([[0], np.cumsum([len(k) for k in kfs])]).astype(np.int32)
        inv = np.zeros(self.K, bool); inv[list(kf_invalid)] = True
        cat = lambda a, w, dt: np.concatenate(a).astype(dt) if len(a) else np.zeros((0,) + w, dt)
        return lr.make_inputs(ptr, cat(kfs, (), np.int32), cat(desc, (32,), np.uint8) if with_desc else None, cat(octs, (), np.int32),
                              np.array(pick(self.ref), np.int32), np.array(pick(self.pos)).reshape(L, 3), self.center, inv,
                              np.array(pick(self.inv), bool))


@functools.lru_cache(maxsize=None)
def hand_case():
    """(inputs, names): K = 12, keyframes 9 and 10 invalid. What each landmark is for is asserted in
    tests/test_lmrefresh_host.py::test_hand_cases_do_what_they_are_for."""
    b = Builder(12, seed=1)
    rng = np.random.default_rng(2)
    x = rng.integers(0, 256, 32, dtype=np.uint8)
    d_at = lambda d, base=x: at_dist(base, d, rng)[0]
    b.add([9, 10], name="n0", ref=0)                                              # every observer invalid
    b.add([3], name="n1")
    b.add([3, 5], desc=[d_at(40), x], name="n2")                                  # every median is the self-distance 0: index 0
    b.add([1, 2, 3], desc=[x, d_at(10), d_at(30)], name="n3")                     # rank 1: the nearest neighbour's distance
    b.add([1, 2, 3, 4], name="n4")
    b.add([1, 2, 3, 4, 5], name="n5")
    b.add([0, 1, 2, 3, 4, 5], desc=np.repeat(x[None], 6, 0), name="identical")    # all medians 0: the first
    b.add([9, 1, 10, 2, 3, 10], desc=[x, d_at(60), x, d_at(3), x, x], ref=3, name="invalid_between")   # candidates at 1, 3, 4
    b.add([1, 2, 3], desc=[x, ~x, ~x], name="complementary")                      # row 0 is (0, 256, 256): 256 must not wrap to 0
    b.add([4, 4, 5], desc=[d_at(5), d_at(5), d_at(90)], name="listed_twice")
    b.add([1, 2, 3], invalid=True, name="invalid_lm")
    b.add([1, 2, 3], ref=-1, name="no_reference")
    b.add([9, 1, 2], ref=0, name="reference_invalid")                             # the distance is taken from keyframe 9 all the same
    b.add([], name="no_observations")
    t = b.rng.integers(0, 256, 32, dtype=np.uint8)
    b.add([1, 2, 3, 4], desc=[at_dist(t, 20, rng)[0], at_dist(t, 4, rng)[0], at_dist(t, 4, rng)[0], at_dist(t, 20, rng)[0]], name="tie_1_2")
    return b.inputs(kf_invalid=(9, 10)), dict(b.names)


def octave_case():
    """Reference observations on levels 0 and 7 (and between), for num_octaves 8."""
    b = Builder(10, seed=3)
    for lvl in (0, 7, 3, 7, 0):
        b.add([1, 2, 3, 4], ref=2, octave=[1, 5, lvl, 2])
    return b.inputs()


@functools.lru_cache(maxsize=None)
def edge_lengths():
    g, wave, wg, stage = limits()
    s = {0, 1, 2, 3, 4, 5, 1500}
    for w in (4, 8, 16, 32, g):
        s |= {w - 1, w, w + 1}
    for lim in (g, wave, wg, stage):          # g + 1 is the first long-form length
        s |= {lim - 1, lim, lim + 1}
    return sorted(s)


@functools.lru_cache(maxsize=None)
def lengths_case(kf_invalid=False):
    """One landmark per length of edge_lengths(), all observers valid (so the candidate count is the length) unless kf_invalid: then a
    tenth of the keyframes is invalid and candidates and list positions part."""
    b = Builder(1600, seed=4)
    for n in edge_lengths():
        b.track(n, p=0.03)
    bad = b.rng.choice(1600, 160, replace=False) if kf_invalid else ()
    return b.inputs(kf_invalid=bad)


@functools.lru_cache(maxsize=None)
def mixed_case(with_desc=True):
    """3000 landmarks of lengths 1..40 in random order over 60 keyframes (3 invalid), some invalid or without reference."""
    b = Builder(60, seed=5)
    for i in range(3000):
        j = b.track(int(b.rng.integers(1, 41)), invalid=bool(b.rng.random() < 0.02))
        if b.rng.random() < 0.02:
            b.ref[j] = -1
    return b.inputs(kf_invalid=(7, 30, 31), with_desc=with_desc)


def map_descriptors(m, seed=0):
    """obs_desc [O,32] for a map: a random pattern per landmark, an observation that pattern with bits flipped, the flip probability
    drawn per keyframe in 0.02..0.12 (tests/guided_util.map_keyframes)."""
    rng = np.random.default_rng(seed)
    lm_desc = rng.integers(0, 256, (m.L, 32), dtype=np.uint8)
    obs_lm = np.repeat(np.arange(m.L), np.diff(m.lm_obs_ptr))
    desc = np.zeros((m.O, 32), np.uint8)
    for k in range(m.K):
        idx = np.flatnonzero(m.obs_kf == k)
        if len(idx):
            desc[idx] = flip(lm_desc[obs_lm[idx]], rng.uniform(0.02, 0.12), rng)
    return desc


def inputs_of_map(m, obs_desc):
    return lr.make_inputs(m.lm_obs_ptr, m.obs_kf, obs_desc, m.obs_octave, optimization.reference_observations(m), m.lm_pos,
                          optimization.kf_centers(m), m.kf_invalid, m.lm_invalid)


@functools.lru_cache(maxsize=None)
def map_case(name):
    m = synth.make_map(synth.config_named(name))
    m.kf_invalid = m.kf_invalid.copy(); m.kf_invalid[[3, m.K // 2]] = True          # observers that stay listed
    return inputs_of_map(m, map_descriptors(m))


@functools.lru_cache(maxsize=None)
def exact(which, *args, **opts_items):
    case = {"hand": lambda: hand_case()[0], "lengths": lengths_case, "mixed": mixed_case, "map": map_case}[which](*args)
    return lr.refresh_exact(case, **opts_items)


def save_map_with_descriptors(path, m, obs_desc):
    """mapio.save_map with every keyframe's descriptor matrix filled in: row f of keyframe k is the descriptor of its f-th observation
    in observation order (save_map's feature index). save_map itself writes zero rows."""
    per_kf = iter([obs_desc[np.flatnonzero(m.obs_kf == k)] for k in range(m.K)])

    class W(mapio.Writer):
        def __init__(self):
            super().__init__(); self.calls = 0

        def cvmat(self, mat):   # a keyframe archive's first matrix is descriptors_ (msg_keyframe.hpp:129-146)
            self.calls += 1
            super().cvmat(next(per_kf) if self.calls == 1 else mat)

    plain, mapio.Writer = mapio.Writer, W
    try:
        mapio.save_map(path, m)
    finally:
        mapio.Writer = plain


_SHIM = None


def refresh_shim():
    """tests/cpp/facade_refresh_shim.cpp: LandmarkRefreshT on the stand-in classes of tests/cpp/standin_refresh.hpp, and the serial
    restatement of the reference's two functions."""
    global _SHIM
    if _SHIM is None:
        here = os.path.dirname(os.path.abspath(__file__)); root = os.path.dirname(here)
        so = os.path.join(here, "cpp", "libfacade_refresh_shim.so")
        srcs = [os.path.join(here, "cpp", f) for f in ("facade_refresh_shim.cpp", "standin_refresh.hpp", "standin_map.hpp")] + \
               [os.path.join(root, "include", "covins_gpu", "optimization_gpu.hpp"), os.path.join(root, "include", "covgpu.h")]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", srcs[0], "-o", so,
                                   "-L" + os.path.join(root, "covins_amd"), "-lcovgpu", "-Wl,-rpath," + os.path.join(root, "covins_amd")])
        lib = C.CDLL(so)
        ip, dp, bp, vp = C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.c_void_p
        lib.refresh_build.restype = vp
        lib.refresh_build.argtypes = [C.c_int, bp, dp, C.c_int, bp, dp, ip, ip, ip, bp, ip]
        lib.refresh_free.argtypes = [vp]
        lib.refresh_shutdown.argtypes = []
        lib.refresh_facade.argtypes = [vp, C.c_double, C.c_int, ip]
        lib.refresh_state.argtypes = [vp, bp, bp, dp, dp, dp]
        lib.refresh_serial.argtypes = [vp, C.c_double, C.c_int, ip, bp, dp, dp, dp, ip, dp]
        _SHIM = lib
    return _SHIM


class StandinRefreshMap:
    """The inputs of one refresh call as stand-in Keyframe / Landmark objects (needs obs_desc)."""

    def __init__(self, inp):
        self.L = inp["L"]
        u8 = lambda a: np.ascontiguousarray(a, dtype=np.uint8)
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
        f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
        a = [u8(inp["kf_invalid"]), f64(inp["kf_center"]), u8(inp["lm_invalid"]), f64(inp["lm_pos"]), i32(inp["lm_ref_obs"]),
             i32(inp["lm_obs_ptr"]), i32(inp["obs_kf"]), u8(inp["obs_desc"]), i32(inp["obs_octave"])]
        t = [C.c_uint8, C.c_double, C.c_uint8, C.c_double, C.c_int, C.c_int, C.c_int, C.c_uint8, C.c_int]
        q = [p(x, y) for x, y in zip(a, t)]
        self.h = C.c_void_p(refresh_shim().refresh_build(inp["K"], q[0], q[1], inp["L"], *q[2:]))

    def close(self):
        if self.h:
            refresh_shim().refresh_free(self.h)
            self.h = None

    def _buffers(self):
        n = max(self.L, 1)
        return dict(lm_desc_obs=np.full(n, -1, np.int32), lm_desc=np.zeros((n, 32), np.uint8), lm_normal=np.zeros((n, 3)),
                    lm_min_distance=np.zeros(n), lm_max_distance=np.zeros(n), lm_status=np.zeros(n, np.int32))

    def serial(self, scale_factor=2.0, num_octaves=1):
        """The serial restatement of the reference's functions; outputs as refresh_exact's, plus `ms`, its wall time."""
        o = self._buffers()
        ms = C.c_double(0.0)
        ip, dp, bp = C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_uint8)
        refresh_shim().refresh_serial(self.h, scale_factor, num_octaves, o["lm_desc_obs"].ctypes.data_as(ip), o["lm_desc"].ctypes.data_as(bp),
                                      o["lm_normal"].ctypes.data_as(dp), o["lm_min_distance"].ctypes.data_as(dp),
                                      o["lm_max_distance"].ctypes.data_as(dp), o["lm_status"].ctypes.data_as(ip), C.byref(ms))
        o = {k: v[:self.L] for k, v in o.items()}
        o["ms"] = ms.value
        return o

    def facade(self, scale_factor=2.0, num_octaves=1):
        """LandmarkRefreshT::Refresh(map), then the landmarks' members: dict(has_desc, lm_desc, lm_normal, lm_min_distance,
        lm_max_distance, form_count)."""
        forms = np.zeros(6, np.int32)
        refresh_shim().refresh_facade(self.h, scale_factor, num_octaves, forms.ctypes.data_as(C.POINTER(C.c_int)))
        o = self._buffers()
        has = np.zeros(max(self.L, 1), np.uint8)
        dp, bp = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
        refresh_shim().refresh_state(self.h, has.ctypes.data_as(bp), o["lm_desc"].ctypes.data_as(bp), o["lm_normal"].ctypes.data_as(dp),
                                     o["lm_min_distance"].ctypes.data_as(dp), o["lm_max_distance"].ctypes.data_as(dp))
        r = {k: o[k][:self.L] for k in ("lm_desc", "lm_normal", "lm_min_distance", "lm_max_distance")}
        r.update(has_desc=has[:self.L].astype(bool), form_count=forms)
        return r
