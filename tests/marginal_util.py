"""Host references for the marginal covariances (Context.marginal_covariance): from the oracle's reduced camera system alone
(covo.schur_sparse, as forms_util.host_system), never from device code.

For the unit columns E of the chosen unknowns three independent routes to Sigma = E^T S^-1 E:
  (a) lu     SuperLU solves of the unit columns (the solver of forms_util.host_system)
  (b) dense  dense LAPACK (LU): the chosen columns of the inverse, n <= 9 000
  (c) chol   dense Cholesky S = L L^T, forward solves Y = L^-1 E and the Gram product Y^T Y — the device's route, in LAPACK's elimination order
Metric: err(A, B) = max |(A - B) o d d^T| / max |A_lu o d d^T| with d = sqrt(diag S) on the chosen rows; h = the largest pairwise err of the
three. A reference is built once per (problem, mu, keyframes) for ALL D rows of the keyframes and shared; a selection takes its rows from it.
"""
import numpy as np

from covins_amd import mapdata, synth
from oracle import covo
from tests import forms_util as fu

DENSE_MAX_N = 9000
H_FLOOR = 1e-13            # tests/test_gpu_forms.py's H_FLOOR

_refs, _pgo = {}, {}


_shim = None


def shim():
    """tests/cpp/libfacade_marginal_shim.so: MarginalCovariance / RelativePoseCovariance of the C++ facade on the stand-in map."""
    global _shim
    if _shim is None:
        import ctypes as C
        import os
        import subprocess
        from tests import facade_util
        here = os.path.dirname(os.path.abspath(__file__)); root = os.path.dirname(here)
        so = os.path.join(here, "cpp", "libfacade_marginal_shim.so")
        srcs = [os.path.join(here, "cpp", f) for f in ("facade_marginal_shim.cpp", "facade_shim.cpp", "standin_map.hpp")] + \
               [os.path.join(root, "include", "covins_gpu", "optimization_gpu.hpp"), os.path.join(root, "include", "covgpu.h")]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", srcs[0], "-o", so, "-L" + os.path.join(root, "covins_amd"),
                                   "-lcovgpu", "-Wl,-rpath," + os.path.join(root, "covins_amd")])
        facade_util.lib()
        lib = C.CDLL(so)
        ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
        lib.shim_marginal.argtypes = [C.c_void_p, C.c_int, ip, C.c_int, C.c_int, C.c_double, dp, C.POINTER(C.c_longlong), C.c_char_p]
        lib.shim_relative_pose_covariance.argtypes = [C.c_void_p, C.c_int, C.c_int, dp, dp]
        lib.shim_relative_pose_covariance.restype = None
        lib.shim_marginal_ir.argtypes = [C.c_void_p, C.c_int, C.c_char_p, dp]
        lib.shim_marginal_ir.restype = C.c_int
        _shim = lib
    return _shim


# detail::Flat's double arrays -> the fields of capi.FlatProblem
FACADE_FIELDS = dict(pose="kf_pose", sb="kf_speed_bias", cam_extr="cam_extr", cam_intr="cam_intr", cam_dist="cam_dist", lm="lm_pos", uv="obs_uv",
                     sigma="obs_sigma", samples="imu_samples", first="imu_first", noise="imu_noise", meas="edge_meas", info="edge_sqrt_info",
                     loss="edge_loss_a")


def facade_problem(sm, prob, visual_only):
    """`prob` (mapdata.flatten_gba of the map behind the stand-in `sm`, second-round form) with every double array replaced by the one the C++
    facade's own walk of the map produces, and the observations of every landmark in the facade's order: the same problem (each array within
    1e-7 of Python's, the observation arrays the same entries; tests/test_facade.py has the other integer arrays equal) in the facade's bits. Returns (problem, names of the arrays whose bits differed)."""
    import ctypes as C
    lib = shim()
    q = prob.copy()
    moved = []
    for name, field in FACADE_FIELDS.items():
        mine = getattr(q, field)
        n = lib.shim_marginal_ir(sm.h, int(visual_only), name.encode(), None)
        if mine is None or (visual_only and name in ("samples", "first", "noise")):
            continue
        mine = np.ascontiguousarray(mine, np.float64)
        assert n == mine.size, (name, n, mine.size)
        got = np.zeros(mine.shape)
        lib.shim_marginal_ir(sm.h, int(visual_only), name.encode(), got.ctypes.data_as(C.POINTER(C.c_double)))
        if name in ("uv", "sigma"):   # a landmark's observations come in the order of the facade's walk (below): the same entries
            assert np.array_equal(np.sort(got.reshape(-1)), np.sort(mine.reshape(-1))), name
        else:
            assert np.abs(got - mine).max(initial=0.0) < 1e-7, name
        if not np.array_equal(got, mine):
            moved.append(name)
        setattr(q, field, got)
    # The facade lists a landmark's observations as the map's observation container yields them — for the stand-in, as for COVINS, a std::map keyed
    # by the keyframe's address, so the order inside a landmark is the allocator's. Same observations, another summation order: last bits.
    okf = np.ascontiguousarray(sm.flatten_gba(visual_only, True)["obs_kf"], np.int32)
    for l in range(q.L):
        a, b = q.lm_obs_ptr[l], q.lm_obs_ptr[l + 1]
        assert sorted(okf[a:b]) == sorted(q.obs_kf[a:b]), l
    if not np.array_equal(okf, q.obs_kf):
        moved.append("obs_kf")
    q.obs_kf = okf
    return q, moved


def pgo_problem(name, kf=None):
    """The pose graph of a synthetic map, as tests/test_gpu_forms.py builds it."""
    key = (name, kf)
    if key not in _pgo:
        cfg = synth.config_named(name)
        if kf:
            cfg.max_kf_per_agent = kf
        cfg.drift_trans = 0.05; cfg.drift_yaw_deg = 0.5
        _pgo[key] = mapdata.flatten_pgo(synth.make_map(cfg), {}, mapdata.PgoParams())[0]
    return _pgo[key]


def rows_of(kfs, D, block_full=True):
    """Solution indices of the chosen keyframes' rows in the request's order: D per keyframe, or the 6 pose rows."""
    d = D if block_full else 6
    return np.array([D * int(k) + r for k in kfs for r in range(d)], np.int64)


def err(A, B, A_lu, d):
    w = np.outer(d, d)
    return float(np.abs((A - B) * w).max() / np.abs(A_lu * w).max())


def reference(prob, visual_only, mu, kfs, pgo=False, key=None):
    """dict(lu, dense, chol: [m, m] with m = D len(kfs), all rows of the keyframes in the order of kfs; d: sqrt(diag S) there; h; n; D; rows)."""
    import scipy.linalg as sl
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    kfs = tuple(int(k) for k in kfs)
    ck = (key, visual_only, mu, kfs, pgo)
    if key is not None and ck in _refs:
        return _refs[ck]
    D = 6 if (pgo or visual_only) else 15
    ptr, col, blocks, b, cost = covo.schur_sparse(prob, covo.default_options(visual_only=1 if visual_only else 0), mu, pgo=pgo)
    n = D * prob.K
    S = sp.bsr_matrix((blocks, col, ptr), shape=(n, n)).tocsr()
    rows = rows_of(kfs, D)
    m = len(rows)
    E = np.zeros((n, m)); E[rows, np.arange(m)] = 1.0
    lu = spla.splu(S.tocsc(), permc_spec="MMD_AT_PLUS_A", diag_pivot_thresh=0.0, options=dict(SymmetricMode=True))
    out = dict(lu=lu.solve(E)[rows], n=n, D=D, rows=rows, d=np.sqrt(np.abs(S.diagonal()))[rows], cost=cost)
    if n <= DENSE_MAX_N:
        Sd = S.toarray()
        out["dense"] = np.linalg.solve(Sd, E)[rows]
        L = np.linalg.cholesky(Sd)
        Y = sl.solve_triangular(L, E, lower=True, check_finite=False)
        out["chol"] = Y.T @ Y
    names = [k for k in ("lu", "dense", "chol") if k in out]
    out["h"] = max([err(out[a], out[b_], out["lu"], out["d"]) for a in names for b_ in names if a < b_], default=0.0)
    if key is not None:
        _refs[ck] = out
    return out


def point_reference(pt, mu, kfs):
    return reference(fu.point_problem(pt), pt.visual_only, mu, kfs, key=(pt.map, pt.kf))


def take(ref_cov, ref_kfs, D, kfs, block_full):
    """The selection `kfs` (a sub-list of ref_kfs, any order) out of a reference over ref_kfs with D rows per keyframe."""
    pos = {int(k): i for i, k in enumerate(ref_kfs)}
    d = D if block_full else 6
    idx = np.array([D * pos[int(k)] + r for k in kfs for r in range(d)], np.int64)
    return ref_cov[np.ix_(idx, idx)]
