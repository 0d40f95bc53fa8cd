"""Unified-projection (omni) cameras on the GPU: every entry point that evaluates a reprojection residual against the numpy restatement
of tests/test_omni_host.py (the oracle knows no unified model), xi = 0 against the pinhole kernels, known answers on a mixed map
(pinhole + RadTan, unified + RadTan, unified + Equidistant), the device-side second round, the sharded solves, relative pose, argument
validation and the C++ facade."""
import ctypes as C

import numpy as np
import pytest

from covins_amd import backend, capi, distrib, mapdata, synth
from tests.test_omni_host import build_omni_standin, linearize_ref, omni_shim, project_ref
from tests.util import rot_angle

pytestmark = pytest.mark.gpu

MIXED = (synth.SynthCamera(0, 0), synth.SynthCamera(1, 0, 0.9), synth.SynthCamera(1, 1, 1.3))


@pytest.fixture(scope="module")
def ctx():
    c = backend.Context(0)
    yield c
    c.close()


def small_mixed(seed=0, **kw):
    cfg = synth.SynthConfig(agents=(1, 2, 3), max_kf_per_agent=10, new_lm_per_kf=15, track_window=4, seed=seed, cameras=MIXED, **kw)
    return synth.make_map(cfg)


def rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def reprojection_only(p):
    """`p` without its between factors (the loop edges of a synthetic map carry noisy measurements): reprojection blocks only."""
    d = dict(p.__dict__)
    d.update(edge_i=np.zeros(0, np.int32), edge_j=np.zeros(0, np.int32), edge_meas=np.zeros((0, 7)), edge_sqrt_info=np.zeros((0, 36)),
             edge_loss_a=np.zeros(0))
    return capi.FlatProblem(**d)


def with_models(p, model, xi):
    q = p.copy()
    q.cam_model = np.asarray(model, np.int32); q.cam_xi = np.asarray(xi, np.float64)
    return capi.FlatProblem(**q.__dict__)


# ------------------------------------------------------------------------------------------------ linearisation
def test_linearize_unified_matches_the_restatement(ctx):
    m = small_mixed()
    p, _ = mapdata.flatten_gba(m, True, True)
    # some landmarks behind the unified cameras' validity boundary: their blocks must come back as zeros
    lm_of = np.repeat(np.arange(p.L), np.diff(p.lm_obs_ptr))
    pick = np.unique(lm_of[np.isin(p.kf_cam[p.obs_kf], [1, 2])])[::7]
    for l in pick:
        k = p.obs_kf[p.lm_obs_ptr[l]]
        c = p.kf_pose[k, 4:]
        p.lm_pos[l] = c - 3.0 * (p.lm_pos[l] - c)
    o = backend.default_options(visual_only=1)
    r, Jp, Jl, cost = ctx.linearize_reprojection(p, o)
    r0, Jp0, Jl0, c0 = linearize_ref(p, loss_a=1.0)
    invalid = (np.abs(Jl0).sum(1) == 0)
    assert invalid.sum() >= 3 and (~invalid).sum() > 100
    assert np.all(r[invalid] == 0) and np.all(Jp[invalid] == 0) and np.all(Jl[invalid] == 0) and np.all(cost[invalid] == 0)
    for a, b in ((r, r0), (Jp, Jp0), (Jl, Jl0), (cost, c0)):
        assert rel(a, b) <= 1e-12, rel(a, b)
    # the residual norms of the outlier rule (covgpu_reprojection_residual_norms) are the same blocks
    n = ctx.residual_norms(p, o)
    assert rel(n, np.linalg.norm(r0, axis=1)) <= 1e-12


def test_xi_zero_is_the_pinhole_linearisation(ctx):
    m = synth.make_map(synth.config_named("tiny"))
    p, _ = mapdata.flatten_gba(m, True, True)
    o = backend.default_options(visual_only=1)
    a = ctx.linearize_reprojection(p, o)
    b = ctx.linearize_reprojection(with_models(p, np.ones(p.A), np.zeros(p.A)), o)
    # the residual is a difference of pixel coordinates (~ 500 px): its rounding is relative to the image, not to the residual
    assert np.abs(b[0] - a[0]).max() * p.obs_sigma.min() <= 1e-14 * synth.WIDTH
    # Jacobians: the same value through another (equivalent) order of operations — rounding, amplified by the cross product of the
    # rotation columns (observed 2e-14 relative to the largest entry)
    for x, y in zip(a[1:3], b[1:3]):
        assert rel(y, x) <= 1e-13
    assert np.abs(b[3] - a[3]).max() <= 1e-14 * synth.WIDTH * max(np.abs(a[0]).max(), 1.0)


def test_xi_zero_gba_follows_the_pinhole_gba():
    """mh01-sized map: the unified path with xi = 0 takes the pinhole path's accept sequence and lands within 1e-9 m of it."""
    m = synth.make_map(synth.config_named("mh01"))
    p, _ = mapdata.flatten_gba(m, False, True)
    o = backend.default_options(max_iterations=10)
    c = backend.Context(0)
    try:
        s0, r0 = c.gba_solve(p, o)
        s1, r1 = c.gba_solve(with_models(p, np.ones(p.A), np.zeros(p.A)), o)
    finally:
        c.close()
    assert r0.iterations == r1.iterations
    assert list(r0.accepted_trace[:r0.iterations]) == list(r1.accepted_trace[:r1.iterations])
    assert np.abs(s0.kf_pose[:, 4:] - s1.kf_pose[:, 4:]).max() <= 1e-9
    assert abs(r0.final_cost - r1.final_cost) <= 1e-9 * r0.final_cost


# ------------------------------------------------------------------------------------------------ known answers
def exact_problem(m, visual_only=True):
    """`m` flattened at its TRUE state with exact (float64, noise-free) keypoints from the restatement, two constant keyframes per agent
    (the gauge and the scale of a visual-only problem)."""
    t = m.copy()
    t.kf_pose = m.truth["kf_pose"].copy(); t.lm_pos = m.truth["lm_pos"].copy()
    t.kf_velocity = m.truth["kf_velocity"].copy(); t.kf_bias_a = m.truth["kf_bias_a"].copy(); t.kf_bias_g = m.truth["kf_bias_g"].copy()
    p, idx = mapdata.flatten_gba(t, visual_only, True)
    p = reprojection_only(p)
    p.obs_uv[:] = 0.0
    r, _, _, _ = linearize_ref(p, loss_a=0.0)
    p.obs_uv[:] = r * p.obs_sigma[:, None]
    assert np.abs(linearize_ref(p, loss_a=0.0)[0]).max() < 1e-9
    for a in range(p.A):
        ks = np.nonzero(p.kf_cam == a)[0]
        p.kf_fixed[ks[:2]] = 1
    return p


def perturbed(p, seed=0, dpos=0.01, drot=0.002, dlm=0.02):
    from scipy.spatial.transform import Rotation as R
    rng = np.random.default_rng(seed)
    q = p.copy()
    free = q.kf_fixed == 0
    q.kf_pose[free, 4:] += rng.normal(0, dpos, (free.sum(), 3))
    rot = R.from_quat(q.kf_pose[free, :4]) * R.from_rotvec(rng.normal(0, drot, (free.sum(), 3)))
    qq = rot.as_quat(); qq[qq[:, 3] < 0] *= -1
    q.kf_pose[free, :4] = qq
    q.lm_pos += rng.normal(0, dlm, q.lm_pos.shape)
    return capi.FlatProblem(**q.__dict__)


def tight_options(**kw):
    return backend.default_options(visual_only=1, max_iterations=25, function_tolerance=0.0, parameter_tolerance=0.0, gradient_tolerance=0.0, **kw)


def test_mixed_map_returns_to_the_known_answer(ctx):
    m = synth.make_map(synth.config_named("mixed"))
    p = exact_problem(m)
    assert list(p.cam_model) == [0, 1, 1] and list(p.cam_dist_type) == [0, 0, 1]
    sol, res = ctx.gba_solve(perturbed(p), tight_options())
    print(f"mixed map K={p.K} L={p.L} O={p.O}: cost {res.initial_cost:.3e} -> {res.final_cost:.3e} in {res.iterations} iterations")
    assert res.initial_cost > 1e3 and res.final_cost < 1e-12
    assert np.abs(sol.kf_pose[:, 4:] - p.kf_pose[:, 4:]).max() <= 1e-9
    assert np.abs(sol.lm_pos - p.lm_pos).max() <= 1e-8


def test_gn_step_equals_a_dense_numpy_gauss_newton_step(ctx):
    """covgpu_gn_step on a small noisy unified problem == (J^T J + mu D^T D)^-1 (-J^T r) with J from the restatement (Ceres' damping:
    D^2 = clamp(sqrt(diag J^T J), 1e-6, 1e32)^2; constant poses carry no unknowns)."""
    m = small_mixed(seed=2)
    p = reprojection_only(mapdata.flatten_gba(m, True, True)[0])
    for a in range(p.A):
        p.kf_fixed[np.nonzero(p.kf_cam == a)[0][:2]] = 1
    mu = 1e-4
    r, Jp, Jl, _ = linearize_ref(p, loss_a=1.0)
    K, L, O = p.K, p.L, p.O
    J = np.zeros((2 * O, 6 * K + 3 * L))
    lm_of = np.repeat(np.arange(L), np.diff(p.lm_obs_ptr))
    for o_ in range(O):
        k, l = p.obs_kf[o_], lm_of[o_]
        J[2 * o_:2 * o_ + 2, 6 * k:6 * k + 6] = Jp[o_].reshape(2, 6)
        J[2 * o_:2 * o_ + 2, 6 * K + 3 * l:6 * K + 3 * l + 3] = Jl[o_].reshape(2, 3)
    keep = np.ones(6 * K + 3 * L, bool)
    for k in np.nonzero(p.kf_fixed)[0]:
        keep[6 * k:6 * k + 6] = False
    Jk = J[:, keep]
    H = Jk.T @ Jk; g = Jk.T @ r.reshape(-1)
    d = np.clip(np.sqrt(np.maximum(np.diag(H), 0)), 1e-6, 1e32)
    x = np.zeros(6 * K + 3 * L)
    x[keep] = np.linalg.solve(H + mu * np.diag(d * d), -g)
    dx, dl, cost = ctx.gn_step(p, backend.default_options(visual_only=1), mu)
    assert rel(np.asarray(dx).reshape(-1)[:6 * K], x[:6 * K]) <= 1e-8
    assert rel(np.asarray(dl).reshape(-1), x[6 * K:]) <= 1e-8


def test_two_round_call_equals_the_literal_two_flatten_sequence():
    from covins_amd.optimization import Optimization
    cfg = synth.config_named("mixed"); cfg.outlier_frac = 0.03
    m = synth.make_map(cfg)
    a, b = m.copy(), m.copy()
    ia = Optimization.GlobalBundleAdjustment(a, 10, -1.0, False, True, False, device_second_round=True)
    ib = Optimization.GlobalBundleAdjustment(b, 10, -1.0, False, True, False, device_second_round=False)
    assert ia["outliers_removed"] == ib["outliers_removed"] > 0
    assert ia["problem"] == ib["problem"]
    assert list(ia["round2"].accepted_trace[:10]) == list(ib["round2"].accepted_trace[:10])
    assert np.array_equal(a.lm_invalid, b.lm_invalid)
    assert np.abs(a.kf_pose - b.kf_pose).max() < 1e-10 and np.abs(a.lm_pos - b.lm_pos).max() < 1e-9


def test_outlier_pass_matches_the_restatement(ctx):
    cfg = synth.config_named("mixed"); cfg.outlier_frac = 0.03
    m = synth.make_map(cfg)
    p, _ = mapdata.flatten_gba(m, False, True)
    o = backend.default_options(max_iterations=5)
    ctx.upload(p, o)
    ctx.solve_resident(o)
    sol = ctx.download()
    th = 0.5
    erase, left, counts = ctx.outlier_pass(p.O, p.L, th)
    r, _, _, _ = linearize_ref(sol, loss_a=1.0)
    ref = np.linalg.norm(r, axis=1) > th
    assert ref.sum() > 0 and np.array_equal(erase, ref)
    assert np.array_equal(left, np.add.reduceat((~ref).astype(int), p.lm_obs_ptr[:-1]))
    assert counts[0] == ref.sum()


# ------------------------------------------------------------------------------------------------ sharded solves
@pytest.mark.parametrize("world,policy", [(2, 0), (4, 0), (2, 1), (4, 1)])
def test_sharded_mixed_map_equals_unsharded(world, policy):
    from tests.test_gpu_shard import run_virtual_ranks
    m = synth.make_map(synth.SynthConfig(agents=(1, 2, 3), max_kf_per_agent=60, new_lm_per_kf=30, track_window=8, cameras=MIXED))
    p, _ = mapdata.flatten_gba(m, False, True)
    o = backend.default_options(max_iterations=10, shard_policy=policy)
    plan = distrib.shard_plan(p, o, world)
    assert plan is not None and plan.subtrees >= 2
    c = backend.Context(0)
    try:
        s0, r0 = c.gba_solve(p, o)
    finally:
        c.close()

    def job(cx, sub, r):
        assert sub.cam_model is not None and list(sub.cam_model) == [0, 1, 1]
        return cx.gba_solve(sub, o)
    parts, _ = run_virtual_ranks(p, plan, job)
    for _, rr in parts:
        assert list(rr.accepted_trace[:rr.iterations]) == list(r0.accepted_trace[:r0.iterations])
    merged = distrib.merge_solution(p, plan, [s for s, _ in parts])
    assert np.abs(merged.kf_pose[:, 4:] - s0.kf_pose[:, 4:]).max() <= 1e-8
    assert np.abs(merged.lm_pos - s0.lm_pos).max() <= 1e-6


# ------------------------------------------------------------------------------------------------ relative pose
def unified_relpose_batch(num, xi_a, xi_b, dist_type=0, seed=0):
    from scipy.spatial.transform import Rotation as R
    rng = np.random.default_rng(seed)
    dist = synth.DIST if dist_type == 0 else synth.EQUI_DIST
    cam = np.concatenate([synth.INTR, dist])
    ptr, pA, pB, kA, kB, T0, Tt = [0], [], [], [], [], [], []
    for b in range(num):
        n = int(rng.integers(40, 120))
        Rab = R.from_rotvec(rng.normal(0, 0.15, 3)); tab = rng.normal(0, 0.4, 3)
        XB = np.stack([rng.uniform(-4, 4, n), rng.uniform(-3, 3, n), rng.uniform(1.0, 8.0, n)], 1)
        XA = Rab.apply(XB) + tab
        pa = lambda X, xi: np.array([project_ref(x, 1, xi, synth.INTR, dist, dist_type)[1] for x in X])
        okA = np.array([project_ref(x, 1, xi_a, synth.INTR, dist, dist_type)[0] for x in XA])
        XA, XB = XA[okA], XB[okA]
        pA.append(XA); pB.append(XB); kA.append(pa(XA, xi_a)); kB.append(pa(XB, xi_b))
        q = (Rab * R.from_rotvec(rng.normal(0, 0.03, 3))).as_quat(); q = -q if q[3] < 0 else q
        T0.append(np.concatenate([q, tab + rng.normal(0, 0.05, 3)]))
        qt = Rab.as_quat(); Tt.append(np.concatenate([qt if qt[3] >= 0 else -qt, tab]))
        ptr.append(ptr[-1] + len(XA))
    cat = lambda a: np.ascontiguousarray(np.concatenate(a))
    C_ = ptr[-1]
    return dict(ptr=np.array(ptr, np.int32), pA=cat(pA), pB=cat(pB), kpA=cat(kA), kpB=cat(kB), sigA=np.full(C_, 2.0), sigB=np.full(C_, 2.0),
                camA=np.tile(cam, (num, 1)), camB=np.tile(cam, (num, 1)), distA=np.full(num, dist_type, np.int32),
                distB=np.full(num, dist_type, np.int32), T0=np.array(T0), Ttrue=np.array(Tt),
                modelA=np.ones(num, np.int32), modelB=np.ones(num, np.int32), xiA=np.full(num, xi_a), xiB=np.full(num, xi_b))


@pytest.mark.parametrize("dist_type", [0, 1])
def test_relpose_recovers_T_ab_with_unified_cameras(ctx, dist_type):
    bt = unified_relpose_batch(24, 0.9, 1.3, dist_type=dist_type, seed=3 + dist_type)
    T, out, inl = ctx.relpose_batch(bt, th_outlier=1.3, min_inliers=12)
    assert not out.any() and np.array_equal(inl, np.diff(bt["ptr"]))
    assert np.abs(T[:, 4:] - bt["Ttrue"][:, 4:]).max() <= 1e-8
    assert np.abs(np.abs(np.sum(T[:, :4] * bt["Ttrue"][:, :4], axis=1)) - 1).max() <= 1e-12
    # the pinhole kernel on the same unified keypoints does NOT recover it: the batch really went through the unified projection
    pin = {k: v for k, v in bt.items() if k not in ("modelA", "modelB", "xiA", "xiB")}
    T2, _, _ = ctx.relpose_batch(pin, th_outlier=1e9, min_inliers=0)
    assert np.abs(T2[:, 4:] - bt["Ttrue"][:, 4:]).max() > 1e-4


def test_relpose_xi_zero_equals_the_pinhole_pairs(ctx):
    from tests.util import make_relpose_batch
    bt = make_relpose_batch(40, seed=21)
    T0, o0, n0 = ctx.relpose_batch(bt, th_outlier=0.9, min_inliers=12)
    bu = dict(bt, modelA=np.ones(40, np.int32), modelB=np.ones(40, np.int32), xiA=np.zeros(40), xiB=np.zeros(40))
    T1, o1, n1 = ctx.relpose_batch(bu, th_outlier=0.9, min_inliers=12)
    assert np.array_equal(o0, o1) and np.array_equal(n0, n1)
    assert np.abs(T0 - T1).max() <= 1e-9


# ------------------------------------------------------------------------------------------------ C ABI and facade
def test_c_abi_rejects_invalid_camera_models(ctx):
    m = small_mixed()
    p, _ = mapdata.flatten_gba(m, True, True)
    o = backend.default_options(visual_only=1)
    for model, xi, msg in (([0, 2, 1], [0, 0.9, 1.3], "unknown camera model"), ([0, 1, 1], [0, -0.1, 1.3], "negative or not finite"),
                           ([0, 1, 1], [0, np.nan, 1.3], "negative or not finite"), ([0, 1, 1], [0, np.inf, 1.3], "negative or not finite")):
        with pytest.raises(backend.CovGpuError, match=msg):
            ctx.linearize_reprojection(with_models(p, model, xi), o)
    q = capi.FlatProblem(**{**p.__dict__, "cam_model": np.array([0, 1, 1], np.int32), "cam_xi": None})
    assert q.cam_xi is None
    with pytest.raises(backend.CovGpuError, match="without cam_xi"):
        ctx.linearize_reprojection(q, o)
    with pytest.raises(backend.CovGpuError, match="unknown camera model"):
        ctx.relpose_batch(dict(unified_relpose_batch(2, 0.9, 0.9), modelA=np.array([1, 3], np.int32)))
    with pytest.raises(backend.CovGpuError, match="negative or not finite"):
        ctx.relpose_batch(dict(unified_relpose_batch(2, 0.9, 0.9), xiB=np.array([0.9, -1.0])))


def test_facade_gba_on_omni_standin_map_equals_the_python_mirror():
    """The pattern and tolerances of tests/test_facade.py::test_cpp_gba_matches_python_facade, on the `tiny` map seen by two unified
    cameras: both rounds, outlier removal included."""
    from covins_amd.optimization import Optimization
    from tests import facade_util
    cfg = synth.config_named("tiny"); cfg.outlier_frac = 0.03
    cfg.cameras = (synth.SynthCamera(1, 0, 0.9), synth.SynthCamera(1, 1, 1.3))
    m = synth.make_map(cfg)
    lib = omni_shim()
    sm = build_omni_standin(m)
    saved = facade_util._LIB
    try:
        lib.omni_gba(sm.h, 10, 0, 1)
        facade_util._LIB = lib    # (the state is read through this library's own copy of shim_get_state)
        st = sm.state()
    finally:
        facade_util._LIB = saved
        lib.shim_free(sm.h); sm.h = None
    mp = m.copy()
    info = Optimization.GlobalBundleAdjustment(mp, 10, -1.0, False, True, False)
    assert info["outliers_removed"] > 0
    assert np.abs(st["pose"][:, 4:] - mp.kf_pose[:, 4:]).max() < 1e-6
    assert rot_angle(st["pose"][:, :4], mp.kf_pose[:, :4]).max() < 1e-6
    d = np.abs(st["lm"] - mp.lm_pos).max(axis=1)
    assert np.median(d) < 1e-7 and d.max() < 1e-2
    assert np.array_equal(st["lm_nobs"], np.diff(mp.lm_obs_ptr)) and np.array_equal(st["lm_invalid"].astype(bool), mp.lm_invalid)
    # ... and away from the pinhole answer on the same keypoints: the unified cameras were used
    m0 = m.copy(); m0.cam_model = None; m0.cam_xi = None
    Optimization.GlobalBundleAdjustment(m0, 10, -1.0, False, True, False)
    assert np.abs(m0.kf_pose[:, 4:] - mp.kf_pose[:, 4:]).max() > 1e-4
