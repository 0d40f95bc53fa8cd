"""Host references and checks for the covariance of every landmark (Context.landmark_covariances), shared by
tests/test_lmcov_host.py and tests/test_gpu_lmcov.py. The routes themselves are in tests/lmcov_ref.py; nothing here runs device code.

Metric per landmark: err = max |A - B| / max |A_routeA|. h = the worst err(route A, route B) over the landmarks checked. The device is held to
err(device, route A) <= C_BOUND max(h, H_FLOOR) and err(device, route B) <= the same, per landmark; a degenerate landmark (the damped H_ll has
no Cholesky factor on the host) must come back with lm_ok = 0 and a zero block, every other one with lm_ok = 1.

Route A covers every landmark at every point, so EVERY landmark but the degenerate ones is held to the bound against A (the count is
asserted). Where route B covers every landmark too (the dense inverse of the full (n + 3 L)^2 matrix: `small` and the cut problems, up to about
18 000 rows, 13 - 25 s each on eight cores, built once per (problem, mu) and shared), every landmark is also held to it against B. On mh123@200
(n + 3 L = 79 833) that matrix cannot be held: route B puts a sample back into the system as unknowns (64 landmarks spread over the list, the
ones with the fewest and the most observations, and 16 spread over the landmarks that more than one agent observes) and inverts that; h is the
spread of A and B on the sample, the sample is held to the bound against both routes and every other landmark against A.

C_BOUND = 100: the smallest of 10 / 30 / 100 that leaves a factor 3 over the worst ratio err / max(h, H_FLOOR) measured on one MI355X (12.27) —
the rule of tests/test_gpu_selinv.py. Every point but mh123@200 stays below 2.5; there all 23 611 landmarks are held against route A while h
is the spread of A and B on 81 of them, so the worst of 23 611 is set against the worst of 81 (on those 81 the ratios are 2.81 and 2.12).
Measured ratios, worst over the landmarks of the point, against route A / route B:
  small visual-inertial (5 037 landmarks, h 5.3e-10 at mu 0, 5.8e-10 at 1e-8)   leaf 15: 0.64 / 1.10 and 0.85 / 0.15   leaf 128: 1.43 / 1.81 and
        0.45 / 0.67   default plan: 0.94 / 1.32 and 0.83 / 0.25
  small visual-only (h 2.9e-11 / 2.3e-11)   leaf 15: 1.16 / 1.07 and 1.70 / 1.15   leaf 128: 1.17 / 1.35 and 1.26 / 0.71   default: 1.17 / 1.12 and 1.58 / 1.04
  cut problems at mu 1e-4 (h 5.4e-13 .. 3.0e-12)   G = 4: 0.65 .. 1.29 / 0.23 .. 1.75   G = 8: 0.64 .. 2.43 / 0.87 .. 2.47 (g8-L33)   G = 16: 0.94 .. 1.36 / 1.20 .. 1.97
  the largest cut problems with a landmark behind its observers, mu 0 (h 5.5e-6 / 1.6e-6 / 1.6e-6; one landmark skipped each)   1.08 / 1.03, 0.51 / 0.79, 0.33 / 0.76
  small with planted constant poses (h 4.6e-12)   1.03 / 1.07        unified cameras, g8-L450 (h 2.7e-12)   1.12 / 1.65
  mh123@200 (h 4.9e-10 on the 81 landmarks of route B, 27 of them seen by more than one agent; against A all 23 611, 3 362 of them seen by more
        than one agent)   COVGPU_ND_TOP=0: 12.27 / 2.81   COVGPU_ND_TOP=1: 9.38 / 2.12
  small visual-only after a two-round solve (5 observations erased, 1 landmark left out, 5 036 checked, h 1.6e-11)   1.32 / 0.53
The mh123 ratios are the system's, as the visual-only ratios of tests/test_gpu_selinv.py: the device assembles S in another summation order than
the oracle, whose S both host routes share.
"""
import os
import subprocess

import numpy as np

from tests import lmcov_ref as lr

H_FLOOR = 1e-13
C_BOUND = 100

_refs = {}
_pairs = {}


def agents_of(prob, l):
    """The agents (cameras) whose keyframes observe landmark l."""
    return {int(prob.kf_cam[k]) for k in prob.obs_kf[prob.lm_obs_ptr[l]:prob.lm_obs_ptr[l + 1]]}


def sample_landmarks(prob, n=64, cross=16):
    """Landmarks route B covers where the full matrix cannot be held: n spread over the list, the ones with the fewest and the most observations,
    and `cross` spread over the landmarks that keyframes of more than one agent observe (all of them if there are fewer)."""
    nobs = np.diff(prob.lm_obs_ptr)
    s = set(int(v) for v in np.linspace(0, prob.L - 1, n).astype(int))
    s.add(int(np.argmin(nobs))); s.add(int(np.argmax(nobs)))
    multi = [l for l in range(prob.L) if len(agents_of(prob, l)) > 1]
    if multi:
        s |= {multi[int(i)] for i in np.linspace(0, len(multi) - 1, min(cross, len(multi))).astype(int)}
    return np.array(sorted(s))


def reference(prob, visual_only, mu, key, sample=None, unified=False):
    """{lin, A, B, checked, checked_b, h}: routes A and B of (prob, mu), cached under `key` (the caller's name for prob). Route A covers every
    landmark the host can factor (`checked`). sample None: route B is dense and covers them all too; else the landmark indices route B
    covers (`checked_b`). h: the worst err(A, B) over checked_b. Read-only."""
    key = (key, bool(visual_only), float(mu), None if sample is None else tuple(int(v) for v in sample))
    if key not in _refs:
        lin = lr.Linearisation(prob, visual_only, mu, unified=unified)
        checked = np.flatnonzero(lin.ok)
        checked_b = checked if sample is None else np.array([l for l in sample if lin.ok[l]])
        A = lr.route_a(lin)
        B = lr.route_b(lin, sample)
        e = lr.err(A[checked_b], B[checked_b], A[checked_b])
        _refs[key] = dict(lin=lin, A=A, B=B, checked=checked, checked_b=checked_b, h=float(e.max()) if len(e) else 0.0)
    return _refs[key]


def hold(tag, ref, lm_cov, lm_ok, expect_bad):
    """Every check of one device result against a reference. expect_bad: the degenerate landmarks the point was built with (asserted against the
    host's count, so nothing else can be left out). Returns the worst ratio err / max(h, H_FLOOR)."""
    lin = ref["lin"]
    L = lin.prob.L
    assert lm_cov.shape == (L, 3, 3) and lm_ok.shape == (L,)
    bad = np.flatnonzero(~lin.ok)
    assert len(bad) == expect_bad, (tag, "degenerate on the host", len(bad), expect_bad)
    assert np.array_equal(np.flatnonzero(lm_ok == 0), bad), (tag, np.flatnonzero(lm_ok == 0)[:8], bad[:8])
    assert not lm_cov[bad].any(), tag
    ck, cb = ref["checked"], ref["checked_b"]
    assert len(ck) == L - expect_bad and len(cb) > 0, (tag, len(ck), len(cb), L, expect_bad)     # EVERY other landmark is held to the bound
    h = max(ref["h"], H_FLOOR)
    eA = lr.err(lm_cov[ck], ref["A"][ck], ref["A"][ck]); eB = lr.err(lm_cov[cb], ref["B"][cb], ref["A"][cb])
    worst = float(max(eA.max(), eB.max())) / h
    print(f"{tag}: L={L} against A {len(ck)}, against B {len(cb)}, skipped {len(bad)}  h={ref['h']:.2e}  vs A {eA.max() / h:.2f} h  vs B {eB.max() / h:.2f} h")
    assert eA.max() <= C_BOUND * h and eB.max() <= C_BOUND * h, (tag, eA.max(), eB.max(), ref["h"])
    properties(tag, lin, lm_cov, lm_ok, h)
    return worst


def properties(tag, lin, lm_cov, lm_ok, h):
    """Bit symmetry, positive eigenvalues, and diag(Sigma_l) >= diag(H_ll^-1) (1 - C max(h, 1e-13)) on every served landmark."""
    good = np.flatnonzero(lm_ok != 0)
    assert np.array_equal(lm_cov, lm_cov.transpose(0, 2, 1)), tag
    assert (np.linalg.eigvalsh(lm_cov[good]) > 0).all(), tag
    dg = np.diagonal(lm_cov[good], axis1=1, axis2=2); d0 = np.diagonal(lin.Hinv[good], axis1=1, axis2=2)
    assert (dg >= d0 * (1.0 - C_BOUND * max(h, H_FLOOR))).all(), (tag, float((dg / d0).min()))


# ------------------------------------------------------------------------------------------------ the host plan's pair resolution, restated
def covisible_pairs(prob):
    """Every pair (i > j) of free keyframes that observe a common landmark, in keyframe indices of the problem. (The library keeps the same list
    in chain-major positions perm[keyframe]; the resolution itself works in solution indices D * keyframe + component, as this restatement.)"""
    if id(prob) in _pairs and _pairs[id(prob)][0] is prob:
        return _pairs[id(prob)][1]
    fixed = np.asarray(prob.kf_fixed)
    out = set()
    for l in range(prob.L):
        ks = sorted({int(k) for k in prob.obs_kf[prob.lm_obs_ptr[l]:prob.lm_obs_ptr[l + 1]] if not fixed[k]})
        for a in range(len(ks)):
            for b in range(a):
                out.add((ks[a], ks[b]))
    _pairs[id(prob)] = (prob, sorted(out))
    return _pairs[id(prob)][1]


def resolve(level, own, st, D, pairs, free):
    """The rule of sel_want / sel_locate on the plan arrays: per pair and per free keyframe (front, first row of i's pose in the front's
    [own | border] list, first row of j's) — or None where the block is not in that square."""
    from tests.test_nd_plan import _scalars
    nn = len(level)
    rows = [np.r_[_scalars(own[k], D), _scalars(st[k], D)] for k in range(nn)]
    owner = {}
    for k in range(nn):
        for v in own[k]:
            owner[int(v)] = k
    where = [{int(g): t for t, g in enumerate(rows[k])} for k in range(nn)]

    def one(ki, kj):
        fa, fb = owner[2 * ki], owner[2 * kj]
        if fa != fb and level[fa] == level[fb]:
            return None
        f = fa if level[fa] <= level[fb] else fb
        r0, q0 = where[f].get(D * ki), where[f].get(D * kj)
        if r0 is None or q0 is None:
            return None
        assert all(where[f].get(D * ki + t) == r0 + t and where[f].get(D * kj + t) == q0 + t for t in range(6)), "rows of a variable not contiguous"
        return f, r0, q0

    return [one(i, j) for i, j in pairs], [one(k, k) for k in free]


# ------------------------------------------------------------------------------------------------ problems with special landmarks
def landmark_behind_its_observers(p, l):
    """`p` with landmark l moved behind every camera that observes it: all its Jacobians are zero, H_ll = 0 — not positive definite at mu = 0."""
    from tests.lm_forms_util import camera_frame_valid
    from tests.test_omni_host import quat_R
    q = p.copy()
    ks = [int(k) for k in q.obs_kf[q.lm_obs_ptr[l]:q.lm_obs_ptr[l + 1]]]
    cen, axis = [], []
    for k in ks:
        c = q.kf_cam[k]
        Rws, Rsc = quat_R(q.kf_pose[k, :4]), quat_R(q.cam_extr[c, :4])
        cen.append(q.kf_pose[k, 4:] + Rws @ q.cam_extr[c, 4:]); axis.append((Rws @ Rsc)[:, 2])
    a = np.mean(axis, 0); a /= np.linalg.norm(a)
    for dist in (5.0, 20.0, 100.0):
        x = np.mean(cen, 0) - dist * a
        if not any(camera_frame_valid(q, k, x) for k in ks):
            q.lm_pos[l] = x
            return q
    raise AssertionError("no point behind all observers")


_shim = None


def shim():
    """tests/cpp/libfacade_lmcov_shim.so: LandmarkCovariances of the C++ facade on the stand-in map (built as selinv_util.shim builds its)."""
    global _shim
    if _shim is None:
        import ctypes as C
        from tests import facade_util
        here = os.path.dirname(os.path.abspath(__file__)); root = os.path.dirname(here)
        so = os.path.join(here, "cpp", "libfacade_lmcov_shim.so")
        srcs = [os.path.join(here, "cpp", f) for f in ("facade_lmcov_shim.cpp", "facade_shim.cpp", "standin_map.hpp")] + \
               [os.path.join(root, "include", "covins_gpu", "optimization_gpu.hpp"), os.path.join(root, "include", "covgpu.h")]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", srcs[0], "-o", so, "-L" + os.path.join(root, "covins_amd"),
                                   "-lcovgpu", "-Wl,-rpath," + os.path.join(root, "covins_amd")])
        facade_util.lib()
        lib = C.CDLL(so)
        lib.shim_landmark_covariances.argtypes = [C.c_void_p, C.c_int, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_ubyte),
                                                  C.POINTER(C.c_longlong), C.c_char_p]
        _shim = lib
    return _shim
