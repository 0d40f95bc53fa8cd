"""Host references and checks for the covariance of every observation (Context.observation_covariances), shared by
tests/test_obscov_host.py and tests/test_gpu_obscov.py. The routes themselves are in tests/obscov_ref.py; nothing here runs device code.

Metrics per observation: on the 2x2 block err = max |A - B| / max |A_routeA|; on the 6x3 cross block the largest difference of the
correlations (entries scaled by 1 / sqrt of route A's diagonals of Sigma_aa and Sigma_l: its rows mix radians and metres). h (one per
metric) = the worst spread of routes A and B over the observations route B covers. The device is held per observation to
err <= C_BOUND max(h, H_FLOOR) against route A everywhere and against route B where B covers; every observation of every landmark the host
can factor is checked (the count is asserted), and obs_ok == 0 is asserted on exactly the observations of the host's degenerate landmarks,
with zero blocks there.

Route B covers every observation on the cut problems (the dense inverse of the full matrix, a few thousand rows); on `small` it covers
lmcov_util.sample_landmarks (the full matrix takes tens of seconds there).

Consistency of the call's own outputs: C_o reassembled on the host from the returned kf_cov, cross_cov, lm_cov and the oracle's Jacobians
equals obs_cov within C_SELF * H_FLOOR of the largest entry of the four terms J_p Sigma_aa J_p^T, J_p Sigma_al J_l^T, its transpose and
J_l Sigma_l J_l^T, each term taken with absolute values (|J| |Sigma| |J|^T): the returned blocks are rounded to an ulp of their own entries,
and a sum of products of rounded numbers is good to that many ulp of the sum of the ABSOLUTE products, not of the result. The two differ by
the anisotropy of a landmark's block: Sigma_l is large along the viewing rays where J_l is small, so J_l Sigma_l J_l^T cancels — by a factor
of 1e3 .. 1e7 at mu = 0 on a landmark seen with little parallax. That cancellation is the reassembly's (it is why the kernel does not take
this route); tests/test_obscov_host.py shows it on the host alone, where route C's own blocks, reassembled, miss the plain denominator by the
same factor. H_FLOOR = 1e-13 is about 450 ulp: a few dozen operations per term.

C_BOUND and C_SELF: the smallest of 10 / 30 / 100 that leaves a factor 3 over the worst ratio measured on one MI355X — the rule of
tests/test_gpu_selinv.py and tests/lmcov_util.py. Measured ratios (worst over the observations of the point; block vs A / vs B, cross vs A /
vs B, self-consistency): see MEASURED below.
"""
import os
import subprocess

import numpy as np

from tests import lmcov_util as lu
from tests import obscov_ref as orf

H_FLOOR = 1e-13
C_BOUND = 100
C_SELF = 10

MEASURED = """One MI355X; per point: block vs A / vs B (in h), cross vs A / vs B (in hx), self-consistency (in H_FLOOR of the largest absolute product).
  cut problems at mu 1e-4 (h 2.6e-13 .. 1.6e-11, hx 0 .. 3.1e-13)
    g4-L1 1.77 / 1.82, 0 / 0 (both observers constant), 0.00     g4-L64 0.50 / 1.11, 0.64 / 0.72, 0.00     g4-L65 0.96 / 1.50, 1.26 / 1.87, 0.00
    g4-L449 1.00 / 0.19, 1.82 / 2.20, 0.10     g8-L32 2.02 / 1.20, 0.62 / 1.19, 0.00     g8-L33 0.90 / 0.82, 0.55 / 1.06, 0.00
    g8-L450 1.33 / 1.33, 0.81 / 1.31, 0.09     g16-L16 1.00 / 0.86, 1.08 / 1.46, 0.01     g16-L17 2.09 / 2.26, 0.78 / 1.75, 0.01
    g16-L451 0.54 / 1.06, 1.93 / 2.47, 0.25
  g8-L450 with a landmark behind its observers, mu 0 (h 1.7e-4, hx 9.2e-8; 9 observations not served)   1.00 / 0.01, 0.77 / 1.54, 0.09
  small visual-inertial, 66 484 observations against A, 1 131 against B (h 5.5e-11 / 1.1e-11, hx 1.8e-9 / 4.5e-10 at mu 0 / 1e-8)
    leaf 15: 2.20 / 0.86, 0.46 / 1.04, 0.62 and 3.69 / 1.93, 2.42 / 1.15, 0.62     default plan: 8.06 / 1.55, 2.33 / 3.04, 0.62 and 2.52 / 1.56, 2.00 / 0.84, 0.63
  small visual-only with planted constant poses (h 2.7e-12, hx 2.0e-13; 1 142 observations against B)   14.33 / 0.59, 27.56 / 27.01, 0.43
  unified cameras, g8-L450 (h 2.7e-12, hx 1.5e-13)   1.17 / 1.40, 0.97 / 1.80, 0.08
  small visual-only after a two-round solve (66 478 of 66 484 observations, 1 061 against B; h 4.3e-12, hx 3.0e-12)   15.65 / 0.63, 7.15 / 6.11, 0.47
Worst: 27.56 (C_BOUND = 100), self-consistency 0.63 (C_SELF = 10). The visual-only ratios above 10 are the system's, as in tests/lmcov_util.py:
the device assembles S in another summation order than the oracle, whose S both host routes share, while h is the spread of the two host
routes on that one S. Relative to the largest term AS IT COMES OUT the self-consistency figures are 1.7 .. 17 on every point at mu > 0 or
on `small`, and 3.9e6 on the point at mu = 0 with h = 1.7e-4 (see above why)."""

_refs = {}


def reference(prob, visual_only, mu, key, sample=None, unified=False):
    """{lin, A, B, rows, rows_b, h, hx}: routes A and B of (prob, mu), cached under `key`. `rows`: every observation of every landmark the host
    can factor (route A covers them); `rows_b`: those route B covers (sample None: all of them). h / hx: the worst spread of A and B over
    rows_b on the 2x2 block / on the cross block's correlations. Read-only."""
    key = (key, bool(visual_only), float(mu), None if sample is None else tuple(int(v) for v in sample))
    if key not in _refs:
        lin = orf.ObsLinearisation(prob, visual_only, mu, unified=unified)
        rows = lin.obs_of()
        rows_b = rows if sample is None else lin.obs_of(sample)
        A = orf.route_a(lin)
        B = orf.route_b(lin, sample)
        e = orf.err_block(A["C"][rows_b], B["C"][rows_b], A["C"][rows_b])
        ex = orf.err_cross(A["X"], B["X"], A, rows_b)
        _refs[key] = dict(lin=lin, A=A, B=B, rows=rows, rows_b=rows_b, h=float(e.max()) if len(e) else 0.0, hx=float(ex.max()) if len(ex) else 0.0)
    return _refs[key]


def psd_slack(C):
    """(smallest eigenvalue, largest eigenvalue) over a stack of symmetric 2x2 blocks."""
    w = np.linalg.eigvalsh(0.5 * (C + C.transpose(0, 2, 1)))
    return float(w.min()), float(w.max())


def hold(tag, ref, res, expect_bad_lm):
    """Every check of one device result (the dict of Context.observation_covariances with cross_cov) against a reference. expect_bad_lm: the
    degenerate landmarks the point was built with (asserted against the host's count). Returns the worst ratios
    (block vs A, block vs B, cross vs A, cross vs B)."""
    lin = ref["lin"]
    O = lin.prob.O
    C, X, ok = res["obs_cov"], res["cross_cov"], res["obs_ok"]
    assert C.shape == (O, 2, 2) and X.shape == (O, 6, 3) and ok.shape == (O,), (tag, C.shape, X.shape, ok.shape)
    bad_lm = np.flatnonzero(~lin.ok)
    assert len(bad_lm) == expect_bad_lm, (tag, "degenerate on the host", len(bad_lm), expect_bad_lm)
    bad = np.concatenate([np.arange(lin.ptr[l], lin.ptr[l + 1]) for l in bad_lm] + [np.zeros(0, np.int64)]).astype(np.int64)
    assert np.array_equal(np.flatnonzero(ok == 0), bad), (tag, np.flatnonzero(ok == 0)[:8], bad[:8])
    assert not C[bad].any() and not X[bad].any(), tag
    rows, rb = ref["rows"], ref["rows_b"]
    assert len(rows) == O - len(bad) and len(rb) > 0, (tag, len(rows), len(rb), O, len(bad))     # EVERY other observation is held to the bound
    h, hx = max(ref["h"], H_FLOOR), max(ref["hx"], H_FLOOR)
    A, B = ref["A"], ref["B"]
    eA = orf.err_block(C[rows], A["C"][rows], A["C"][rows]).max() / h
    eB = orf.err_block(C[rb], B["C"][rb], A["C"][rb]).max() / h
    xA = orf.err_cross(X, A["X"], A, rows).max() / hx
    xB = orf.err_cross(X, B["X"], A, rb).max() / hx
    print(f"{tag}: O={O} against A {len(rows)}, against B {len(rb)}, not served {len(bad)}  h={ref['h']:.2e} hx={ref['hx']:.2e}  "
          f"block vs A {eA:.2f} h  vs B {eB:.2f} h  cross vs A {xA:.2f} hx  vs B {xB:.2f} hx")
    assert max(eA, eB, xA, xB) <= C_BOUND, (tag, eA, eB, xA, xB, ref["h"], ref["hx"])
    # properties: symmetric bit for bit, eigenvalues in [-t, 1 + t]
    assert np.array_equal(C[:, 0, 1], C[:, 1, 0]), tag
    t = C_BOUND * h
    lo, hi = psd_slack(C[rows])
    assert lo >= -t and hi <= 1.0 + t, (tag, lo, hi, t)
    # a constant observer: zero cross block; an observation that does not project: a zero block
    fx = rows[~lin.free_obs[rows]]
    assert not X[fx].any(), tag
    dead = rows[~lin.Jl[rows].any(axis=(1, 2))]
    assert not C[dead].any() and ok[dead].all(), tag
    return float(eA), float(eB), float(xA), float(xB)


def reassembly(lin, good, Saa, X, Sl, C):
    """C_o of the observations `good` reassembled from the blocks Sigma_aa [m, 6, 6], Sigma_al [m, 6, 3], Sigma_l [m, 3, 3] and the oracle's
    Jacobians against C [m, 2, 2]: the worst |difference| relative to (the largest entry of the four terms as they come out, the largest
    entry of the four terms taken with absolute values, |J| |Sigma| |J|^T)."""
    Jp, Jl = lin.Jp[good], lin.Jl[good]
    T = lambda a: a.transpose(0, 2, 1)
    t1, t2, t4 = Jp @ Saa @ T(Jp), Jp @ X @ T(Jl), Jl @ Sl @ T(Jl)
    a1, a2, a4 = np.abs(Jp) @ np.abs(Saa) @ T(np.abs(Jp)), np.abs(Jp) @ np.abs(X) @ T(np.abs(Jl)), np.abs(Jl) @ np.abs(Sl) @ T(np.abs(Jl))
    big = lambda *t: np.where(np.max([np.abs(x).max(axis=(1, 2)) for x in t], axis=0) > 0, np.max([np.abs(x).max(axis=(1, 2)) for x in t], axis=0), 1.0)
    diff = np.abs(t1 + t2 + T(t2) + t4 - C).max(axis=(1, 2))
    return float((diff / big(t1, t2, t4)).max()), float((diff / big(a1, a2, a4)).max())


def self_consistency(tag, lin, res):
    """obs_cov against C_o reassembled from the call's own kf_cov, cross_cov and lm_cov and the oracle's Jacobians, relative to the largest
    entry of the four terms taken with absolute values; returns the worst ratio to H_FLOOR over the served observations."""
    good = np.flatnonzero(res["obs_ok"] != 0)
    plain, ab = reassembly(lin, good, res["kf_cov"][lin.kf_of[good]], res["cross_cov"][good], res["lm_cov"][lin.lm_of[good]], res["obs_cov"][good])
    ratio = ab / H_FLOOR
    print(f"{tag}: self-consistency on {len(good)} observations {ratio:.2f} x {H_FLOOR:g} of the largest term (absolute products); "
          f"{plain / H_FLOOR:.2f} x of the largest term as it comes out")
    assert ratio <= C_SELF, (tag, ratio)
    return ratio


_shim = None


def shim():
    """tests/cpp/libfacade_obscov_shim.so: ObservationCovariances of the C++ facade on the stand-in map (built as lmcov_util.shim builds its)."""
    global _shim
    if _shim is None:
        import ctypes as C
        from tests import facade_util
        here = os.path.dirname(os.path.abspath(__file__)); root = os.path.dirname(here)
        so = os.path.join(here, "cpp", "libfacade_obscov_shim.so")
        srcs = [os.path.join(here, "cpp", f) for f in ("facade_obscov_shim.cpp", "facade_shim.cpp", "standin_map.hpp")] + \
               [os.path.join(root, "include", "covins_gpu", "optimization_gpu.hpp"), os.path.join(root, "include", "covgpu.h")]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", srcs[0], "-o", so, "-L" + os.path.join(root, "covins_amd"),
                                   "-lcovgpu", "-Wl,-rpath," + os.path.join(root, "covins_amd")])
        facade_util.lib()
        lib = C.CDLL(so)
        dp, ll = C.POINTER(C.c_double), C.POINTER(C.c_longlong)
        lib.shim_observation_covariances.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_longlong, dp, dp, C.POINTER(C.c_ubyte), ll, ll, ll, ll,
                                                     C.c_char_p]
        _shim = lib
    return _shim


__all__ = ["reference", "hold", "self_consistency", "shim", "lu"]
