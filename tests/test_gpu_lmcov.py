"""Covariance of every landmark from the selected inverse of the factor (Context.landmark_covariances) against host references.

Every landmark's 3x3 block is held to the spread of two HOST routes to the same block (tests/lmcov_util.py over tests/lmcov_ref.py: route A, the
block formula on the dense inverse of the oracle's reduced system; route B, the inverse of the full (n + 3 L)^2 matrix with no Schur identity):
err(device, A) and err(device, B) <= C max(h, 1e-13) in the metric max |X - Y| / max |A|, h the worst err(A, B) over the landmarks checked.
Never compared with another run of the device code, except where the assertion IS that two runs return the same bits.

Points, the smallest shapes at which the pass can go wrong: `small` under three plans (leaf 15: the observer pairs of a landmark lie in
different fronts' squares, own x own and border x own, in both orientations; leaf 128; the default plan), visual-inertial and visual-only, mu 0
and 1e-8; the cut problems of tests/lm_forms_util.py at every group width (tracks of G - 1, G, G + 1, 2 G + 1 and four to five chunks, 256 / G
- 1, 256 / G and 256 / G + 1 landmarks, landmarks observed by constant keyframes only, one observation behind its camera, two observations),
the largest of each width also with one landmark moved behind all its observers (H_ll = 0: lm_ok = 0, a zero block); constant-pose observers
planted in `small`; unified cameras; mh123@200 under both cuts of the top; the second round of a two-round solve. The cut problems run at
mu = 1e-4, the damping every solve starts at: with a handful of landmarks many keyframes see fewer than three and the reduced system is
singular at mu = 0. C and the measured ratios: tests/lmcov_util.py.
"""
import ctypes as C

import numpy as np
import pytest

from covins_amd import backend
from tests import forms_util as fu
from tests import lm_forms_util as lf
from tests import lmcov_util as lu
from tests import marginal_util as mu_

pytestmark = pytest.mark.gpu

SMALL_POINTS = [fu._pt("small", None, vo, leaf) for vo in (False, True) for leaf in (15, 128, 0)]
MUS = (0.0, 1e-8)
WIDTH_POINTS = [pt for G in (4, 8, 16) for pt in lf.POINTS[G]]
MU_CUT = lf.MU_STEP


@pytest.fixture(scope="module")
def shared():
    c = backend.Context(0)
    state = dict(ctx=c, ratios={}, first=None)
    yield state
    c.close()


def _stats_ok(tag, st, prob, G=None):
    assert st["fronts"] >= st["levels"] >= 1 and st["sweep_launches"] >= 1 and st["landmark_launches"] == 1 and st["scratch_bytes"] > 0, (tag, st)
    assert st["group_width"] == (G if G is not None else backend.lm_group(prob.O, prob.L)), (tag, st)
    assert st["pairs_resolved"] == len(lu.covisible_pairs(prob)), (tag, st)


@pytest.mark.parametrize("pt", SMALL_POINTS, ids=[p.id for p in SMALL_POINTS])
def test_small_under_three_plans(shared, pt):
    ctx = shared["ctx"]
    prob, opt = fu.point_problem(pt), fu.point_options(pt)
    with fu.forced_env(pt, leaf_too=True):
        ctx.upload(prob, opt)
        for mu in MUS:
            ref = lu.reference(prob, pt.visual_only, mu, key="small")
            cov, ok, kf, st = ctx.landmark_covariances_resident(opt, mu=mu, want_kf=True)
            tag = f"{pt.id} mu={mu:g}"
            _stats_ok(tag, st, prob)
            assert st["landmarks_not_ok"] == 0
            shared["ratios"][tag] = lu.hold(tag, ref, cov, ok, expect_bad=0)
            # the pose diagonal blocks the sweep has anyway == keyframe_covariances' pose blocks, bit for bit
            kp = ctx.keyframe_covariances_resident(opt, block="pose", mu=mu)[0]
            assert np.array_equal(kf, kp), tag
            # a second call, and the one-call form (upload + factor + sweep + pass), return the same bits
            again = ctx.landmark_covariances_resident(opt, mu=mu)
            assert np.array_equal(again[0], cov) and np.array_equal(again[1], ok) and again[2] is None
            one = ctx.landmark_covariances(prob, opt, mu=mu, want_kf=True)
            assert np.array_equal(one[0], cov) and np.array_equal(one[1], ok) and np.array_equal(one[2], kf)
            if shared["first"] is None:
                shared["first"] = (pt, mu, cov, ok, kf)


def test_repeat_on_a_fresh_context_is_bit_identical(shared):
    if shared["first"] is None:
        test_small_under_three_plans(shared, SMALL_POINTS[0])
    pt, mu, cov, ok, kf = shared["first"]
    prob, opt = fu.point_problem(pt), fu.point_options(pt)
    c = backend.Context(0)
    try:
        with fu.forced_env(pt, leaf_too=True):
            for _ in range(2):   # (the second with history)
                one = c.landmark_covariances(prob, opt, mu=mu, want_kf=True)
                assert np.array_equal(one[0], cov) and np.array_equal(one[1], ok) and np.array_equal(one[2], kf)
    finally:
        c.close()


@pytest.mark.parametrize("pt", WIDTH_POINTS, ids=[p.id for p in WIDTH_POINTS])
def test_group_widths(shared, pt):
    b = lf.build(pt, "pinhole")
    prob = b.p
    opt = backend.default_options(visual_only=1)
    assert backend.lm_group(prob.O, prob.L) == pt.G
    ref = lu.reference(prob, True, MU_CUT, key=("cut", pt.id))
    cov, ok, _, st = shared["ctx"].landmark_covariances(prob, opt, mu=MU_CUT)
    _stats_ok(pt.id, st, prob, G=pt.G)
    shared["ratios"][pt.id] = lu.hold(pt.id, ref, cov, ok, expect_bad=0)
    if "const" in b.special:
        # observed by constant keyframes only: Sigma_l = H_ll^-1 = R R^T
        l = b.special["const"]
        lin = ref["lin"]
        assert len(lin.observers(l)[0]) == 0 and ok[l] == 1
        assert np.abs(cov[l] - lin.Hinv[l]).max() <= lu.C_BOUND * max(ref["h"], lu.H_FLOOR) * np.abs(lin.Hinv[l]).max()


@pytest.mark.parametrize("G", [4, 8, 16])
def test_degenerate_landmark_gets_a_zero_block(shared, G):
    """The largest point of a width with one more degenerate landmark: a track of G + 1 moved behind all its observers, H_ll = 0 exactly. At
    mu = 0 neither the host nor k_lm_lin can factor it; at MU_CUT the damping of a zero diagonal (mu 1e-6^2) makes it a valid, huge block."""
    from oracle import covo
    pt = lf.LARGE[G]
    b = lf.build(pt, "pinhole")
    taken = {v for k, v in b.special.items() if k != "behind_obs"}
    l = next(int(s) for s in np.nonzero(b.lengths == G + 1)[0] if int(s) not in taken)
    prob = lu.landmark_behind_its_observers(b.p, l)
    opt = backend.default_options(visual_only=1)
    H = covo.landmark_hessians(prob, covo.default_options(visual_only=1))
    assert not H[l].any() and all(np.linalg.eigvalsh(H[k]).min() > 0 for k in range(prob.L) if k != l)
    ref = lu.reference(prob, True, 0.0, key=("cut-behind", pt.id))
    cov, ok, _, st = shared["ctx"].landmark_covariances(prob, opt, mu=0.0)
    assert st["group_width"] == G and st["landmarks_not_ok"] == 1
    shared["ratios"][pt.id + "-behind"] = lu.hold(pt.id + "-behind mu=0", ref, cov, ok, expect_bad=1)
    assert ok[l] == 0 and not cov[l].any()


def test_constant_pose_observers(shared):
    """`small`, visual-only, with keyframes marked constant: one landmark with one constant observer among free ones, one with all observers
    constant (Sigma_l = R R^T = the host's H_ll^-1, lm_ok = 1)."""
    pt = fu._pt("small", None, True, 0)
    prob = fu.point_problem(pt).copy()
    nobs = np.diff(prob.lm_obs_ptr)
    l_all = int(np.flatnonzero(nobs == nobs.min())[0])
    kall = set(int(k) for k in prob.obs_kf[prob.lm_obs_ptr[l_all]:prob.lm_obs_ptr[l_all + 1]])
    l_one = next(l for l in range(prob.L) if nobs[l] >= 4 and not kall & set(int(k) for k in prob.obs_kf[prob.lm_obs_ptr[l]:prob.lm_obs_ptr[l + 1]]))
    k_one = int(prob.obs_kf[prob.lm_obs_ptr[l_one] + 1])
    prob.kf_fixed[list(kall) + [k_one]] = 1
    opt = fu.point_options(pt)
    ref = lu.reference(prob, True, 0.0, key="small-fixed")
    lin = ref["lin"]
    assert len(lin.observers(l_all)[0]) == 0 and len(lin.observers(l_one)[0]) == nobs[l_one] - 1 >= 3
    cov, ok, kf, st = shared["ctx"].landmark_covariances(prob, opt, mu=0.0, want_kf=True)
    _stats_ok("small-fixed", st, prob)
    shared["ratios"]["small-fixed"] = lu.hold("small-fixed", ref, cov, ok, expect_bad=0)
    assert ok[l_all] == 1
    assert np.abs(cov[l_all] - lin.Hinv[l_all]).max() <= lu.C_BOUND * max(ref["h"], lu.H_FLOOR) * np.abs(lin.Hinv[l_all]).max()
    assert not kf[prob.kf_fixed != 0].any() and kf[prob.kf_fixed == 0].any(axis=(1, 2)).all()


def test_unified_cameras(shared):
    """One point on the mixed cameras of tests/test_gpu_omni.py (pinhole, unified + RadTan, unified + Equidistant) at the default plan: the
    references come from the numpy restatement of the unified model."""
    pt = lf.LARGE[8]
    prob = lf.build(pt, "unified").p
    assert prob.cam_model is not None and (np.asarray(prob.cam_model) == 1).any()
    opt = backend.default_options(visual_only=1)
    ref = lu.reference(prob, True, MU_CUT, key=("cut-unified", pt.id), unified=True)
    cov, ok, _, st = shared["ctx"].landmark_covariances(prob, opt, mu=MU_CUT)
    _stats_ok("unified", st, prob, G=8)
    shared["ratios"]["unified " + pt.id] = lu.hold("unified " + pt.id, ref, cov, ok, expect_bad=0)


@pytest.mark.parametrize("top", ["0", "1"])
def test_three_agents_under_both_cuts_of_the_top(shared, top):
    pt = fu._pt("mh123", 200, False, 0, env={"COVGPU_ND_TOP": top})
    prob, opt = fu.point_problem(pt), fu.point_options(pt)
    ref = lu.reference(prob, False, 0.0, key="mh123@200", sample=lu.sample_landmarks(prob))
    with fu.forced_env(pt, leaf_too=True):
        cov, ok, _, st = shared["ctx"].landmark_covariances(prob, opt, mu=0.0)
    assert st["group_width"] == backend.lm_group(prob.O, prob.L) and st["landmarks_not_ok"] == 0 and st["pairs_resolved"] > 0
    # multi-agent: landmarks observed from several agents are in route B's sample, and every landmark (they too) is held against route A
    multi_b = sum(len(lu.agents_of(prob, l)) > 1 for l in ref["checked_b"])
    multi_a = sum(len(lu.agents_of(prob, l)) > 1 for l in ref["checked"])
    print(f"{pt.id}: seen by more than one agent: {multi_b} of {len(ref['checked_b'])} sampled landmarks, {multi_a} of {len(ref['checked'])}")
    assert multi_b >= 8 and multi_a >= multi_b and len(ref["checked"]) == prob.L
    shared["ratios"][pt.id] = lu.hold(pt.id, ref, cov, ok, expect_bad=0)


def test_resident_call_between_two_solves_leaves_the_second_its_bits():
    pt = fu._pt("small", None, False, 0)
    prob = fu.point_problem(pt)
    opt = fu.point_options(pt, max_iterations=3)
    a, b, c = backend.Context(0), backend.Context(0), backend.Context(0)
    try:
        a.upload(prob, opt); ra1 = a.solve_resident(opt); qa1 = a.download()
        got = a.landmark_covariances_resident(opt, mu=0.0, want_kf=True)
        ra2 = a.solve_resident(opt); qa2 = a.download()
        b.upload(prob, opt); b.solve_resident(opt); rb2 = b.solve_resident(opt); qb2 = b.download()
        for f in ("kf_pose", "kf_speed_bias", "lm_pos"):
            assert np.array_equal(getattr(qa2, f), getattr(qb2, f)), f
            assert np.array_equal(getattr(qa2, f), getattr(qa1, f)), f
        assert ra2.final_cost == rb2.final_cost == ra1.final_cost and ra2.iterations == rb2.iterations
        # the resident call at the solve's estimate == the one-call form at the downloaded estimate, bit for bit
        one = c.landmark_covariances(qa1, opt, mu=0.0, want_kf=True)
        for x, y in zip(got[:3], one[:3]):
            assert np.array_equal(x, y)
        assert got[1].all() and got[3] == one[3]
    finally:
        a.close(); b.close(); c.close()


def test_after_a_two_round_solve(shared):
    """The resident call after covgpu_gba_two_round works on the second round's compacted observation set and rebuilt pair lists: it must match
    routes A and B on the downloaded estimate with the erased observations (the result's flags) removed."""
    from oracle import covo
    from tests import structure_util as su
    pt = fu._pt("small", None, True, 0)
    prob = fu.point_problem(pt).copy()
    nobs = np.diff(prob.lm_obs_ptr)
    # planted: all but one observation of a track of three (the landmark drops out), one observation of a long track
    l3 = int(np.flatnonzero(nobs == 3)[0]); l9 = int(np.flatnonzero(nobs >= 9)[0])
    rows = np.array([prob.lm_obs_ptr[l3], prob.lm_obs_ptr[l3] + 1, prob.lm_obs_ptr[l9] + 4])
    prob.obs_uv[rows] += np.float32(lf.OUTLIER_PX)
    th = lf.OUTLIER_THRESHOLD    # (the loss-corrected norm of a whitened residual stays below 1)
    norms = covo.residual_norms(prob, covo.default_options(visual_only=1))
    assert (norms[rows] > th + 0.5 * (1.0 - th)).all(), norms[rows]   # on the CPU: the threshold erases at least the planted observations
    opt = backend.default_options(max_iterations=4, visual_only=1)
    ctx = shared["ctx"]
    sol, r1, r2, erase, left, (nb, ns) = ctx.gba_two_round(prob, opt, th)
    assert erase[rows].all() and nb == int(erase.sum()) >= 3 and ns == int((left < 2).sum()) >= 1 and left[l3] < 2
    q, keep = su.compact(sol, erase)
    assert q.L == prob.L - ns and keep.sum() == q.L and not keep[l3]
    cov, ok, _, st = ctx.landmark_covariances_resident(opt, mu=0.0, num_lm=q.L)
    assert st["pairs_resolved"] == len(lu.covisible_pairs(q))
    ref = lu.reference(q, True, 0.0, key="small-round2")
    print(f"two-round: erased {nb}, landmarks left out {ns} of {prob.L}")
    shared["ratios"]["small-round2"] = lu.hold("small-round2", ref, cov, ok, expect_bad=0)


def test_facade_shim_returns_the_python_calls_bits(shared):
    from covins_amd import capi, mapdata, synth
    from tests.facade_util import StandinMap
    m = synth.make_map(synth.config_named("tiny"))
    lib = lu.shim()
    sm = StandinMap(m)
    try:
        # (tiny visual-only is not positive definite without damping: that case runs at the damping of a solve's first iteration)
        for visual_only, mu in ((False, 0.0), (True, 1e-4)):
            prob, idx = mapdata.flatten_gba(m, visual_only, loop_loss=True)
            prob, moved = mu_.facade_problem(sm, prob, visual_only)   # the same problem in the facade's bits (tests/marginal_util.py)
            opt = backend.default_options(visual_only=1 if visual_only else 0)
            cov, ok, _, st = shared["ctx"].landmark_covariances(prob, opt, mu=mu)
            rows = np.asarray(idx.lm_rows)
            cov2 = np.zeros((m.L, 3, 3)); present = np.zeros(m.L, np.uint8)
            stats = (C.c_longlong * 8)(); msg = C.create_string_buffer(256)
            rc = lib.shim_landmark_covariances(sm.h, int(visual_only), mu, cov2.ctypes.data_as(C.POINTER(C.c_double)),
                                               present.ctypes.data_as(C.POINTER(C.c_ubyte)), stats, msg)
            assert rc == 0, msg.value
            assert np.array_equal(cov2[rows], cov) and np.array_equal(present[rows], ok) and ok.any()
            assert present.sum() == ok.sum()          # landmarks outside the problem, or with lm_ok = 0, are absent
            assert [int(v) for v in stats] == [st[k] for k in capi.LMCOV_STATS]
        rc = lib.shim_landmark_covariances(sm.h, 1, -1.0, cov2.ctypes.data_as(C.POINTER(C.c_double)), present.ctypes.data_as(C.POINTER(C.c_ubyte)),
                                           None, msg)
        assert rc == 1 and b"mu negative or not finite" in msg.value, msg.value
    finally:
        sm.close()


def test_refusals_that_depend_on_the_context(shared):
    ctx = shared["ctx"]
    prob = mu_.pgo_problem("small")
    opt = backend.default_options()
    ctx.upload(prob, opt, pgo=True)
    with pytest.raises(backend.CovGpuError, match="pose graph"):
        ctx.landmark_covariances_resident(opt)
    fresh = backend.Context(0)
    try:
        with pytest.raises(backend.CovGpuError, match="no problem uploaded"):
            fresh.landmark_covariances_resident(opt)
    finally:
        fresh.close()
    # a sharded context holds one rank's share of the factor: refused before anything is uploaded or exchanged
    from covins_amd import distrib
    pt = fu._pt("small", None, False, 0)
    gprob, gopt = fu.point_problem(pt), fu.point_options(pt)
    plan = distrib.shard_plan(gprob, gopt, 2)
    assert plan is not None
    grp = distrib.Group(2)
    sc = backend.Context(0)
    try:
        sc.set_shard_group(plan, 0, grp)
        with pytest.raises(backend.CovGpuError, match="sharded context"):
            sc.landmark_covariances(gprob, gopt)
        with pytest.raises(backend.CovGpuError, match="sharded context"):
            sc.landmark_covariances_resident(gopt)
        sc.set_shard_none()
    finally:
        sc.close(); grp.close()


def test_worst_ratios_of_the_file(shared):
    for tag, w in shared["ratios"].items():
        print(f"worst ratio {tag}: {w:.2f}")
