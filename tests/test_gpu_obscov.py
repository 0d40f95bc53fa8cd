"""Covariance of every observation and its pose-landmark cross block (Context.observation_covariances) against host references.

Every observation's 2x2 block C_o = J_o Sigma J_o^T and 6x3 cross block Sigma_al are held to the spread of two HOST routes to the same blocks
(tests/obscov_util.py over tests/obscov_ref.py: route A, the block formulas on the dense inverse of the oracle's reduced system; route B, the
inverse of the full matrix with no Schur identity): err <= C max(h, 1e-13) per observation, against A everywhere and against B where B covers.
Never compared with another run of the device code, except where the assertion IS that two runs return the same bits.

Points, the smallest at which the pass can go wrong: the cut problems of tests/lm_forms_util.py at mu = 1e-4 (g4-L1: one landmark, one
workgroup; g4-L64 / L65, g8-L32 / L33, g16-L16 / L17: a full and a spilled workgroup; the largest of each width: tracks of G - 1, G, G + 1, 2 G,
2 G + 1, so a lane takes 1, 2 and 3 observations and pass 2 reads back several stored V_a; a landmark with constant observers only, one
observation behind its camera inside a live track, a track of two); the largest of one width at mu = 0 with a landmark behind all its
observers (obs_ok = 0 on its observations and nothing else); `small` visual-inertial at leaf 15 and at the default plan, mu 0 and 1e-8 (D = 15:
the pose rows sit inside 15-row keyframe blocks); `small` with planted constant poses; g8-L450 with unified cameras; the compacted stream after
a two-round solve. On every point the call's own outputs are checked against each other (obscov_util.self_consistency), and lm_cov, lm_ok and
kf_cov against landmark_covariances, bit for bit. C and the measured ratios: tests/obscov_util.py.
"""
import ctypes as C

import numpy as np
import pytest

from covins_amd import backend, capi
from tests import forms_util as fu
from tests import lm_forms_util as lf
from tests import lmcov_util as lu
from tests import marginal_util as mu_
from tests import obscov_util as ou

pytestmark = pytest.mark.gpu

MU_CUT = lf.MU_STEP
CUT_IDS = ("g4-L1", "g4-L64", "g4-L65", "g8-L32", "g8-L33", "g16-L16", "g16-L17", lf.LARGE[4].id, lf.LARGE[8].id, lf.LARGE[16].id)
CUT_POINTS = [pt for G in (4, 8, 16) for pt in lf.POINTS[G] if pt.id in CUT_IDS]
SMALL_VI = [fu._pt("small", None, False, leaf) for leaf in (15, 0)]
MUS = (0.0, 1e-8)
ALL = dict(want_cross=True, want_res=True, want_lm=True, want_kf=True)
FIELDS = ("obs_cov", "cross_cov", "obs_res", "obs_ok", "lm_cov", "lm_ok", "kf_cov")


@pytest.fixture(scope="module")
def shared():
    c = backend.Context(0)
    state = dict(ctx=c, ratios={}, first=None)
    yield state
    c.close()


def _same(a, b, fields=FIELDS):
    return all(np.array_equal(a[f], b[f]) for f in fields)


def _stats_ok(tag, st, prob, lin, G=None, bad=0):
    assert st["fronts"] >= st["levels"] >= 1 and st["sweep_launches"] >= 1 and st["observation_launches"] == 1 and st["scratch_bytes"] > 0, (tag, st)
    assert st["group_width"] == (G if G is not None else backend.lm_group(prob.O, prob.L)), (tag, st)
    assert st["observations_not_ok"] == bad and st["constant_observers"] == int((~lin.free_obs).sum()), (tag, st)


def _point(shared, tag, res, ref, prob, opt, mu, G=None, expect_bad_lm=0, landmark_call=True):
    """The checks every point gets: the bound against both routes, the counts, the properties, the residual, the call's own outputs against
    each other, and the landmark call's bits."""
    lin = ref["lin"]
    nbad = int(sum(lin.ptr[l + 1] - lin.ptr[l] for l in np.flatnonzero(~lin.ok)))
    _stats_ok(tag, res["stats"], prob, lin, G=G, bad=nbad)
    r = ou.hold(tag, ref, res, expect_bad_lm)
    # the residual of the same evaluation: the oracle's whitened, loss-corrected residual (an absolute 1e-9 of a whitened pixel: float inputs,
    # a few dozen operations on coordinates of size ~10)
    assert np.abs(res["obs_res"] - lin.r).max() <= 1e-9, (tag, np.abs(res["obs_res"] - lin.r).max())
    s = ou.self_consistency(tag, lin, res)
    shared["ratios"][tag] = r + (s,)
    if landmark_call:
        lm = shared["ctx"].landmark_covariances(prob, opt, mu=mu, want_kf=True)
        assert np.array_equal(lm[0], res["lm_cov"]) and np.array_equal(lm[1], res["lm_ok"]) and np.array_equal(lm[2], res["kf_cov"]), tag


@pytest.mark.parametrize("pt", CUT_POINTS, ids=[p.id for p in CUT_POINTS])
def test_cut_problems(shared, pt):
    b = lf.build(pt, "pinhole")
    prob = b.p
    opt = backend.default_options(visual_only=1)
    assert backend.lm_group(prob.O, prob.L) == pt.G
    ref = ou.reference(prob, True, MU_CUT, key=("cut", pt.id))
    res = shared["ctx"].observation_covariances(prob, opt, mu=MU_CUT, **ALL)
    _point(shared, pt.id, res, ref, prob, opt, MU_CUT, G=pt.G)
    lin = ref["lin"]
    if pt is lf.LARGE[pt.G]:
        assert set(lf.required_lengths(pt.G)) <= set(int(v) for v in b.lengths)
        # const: constant observers only — zero cross blocks, C_o = J_l H_ll^-1 J_l^T
        l = b.special["const"]
        o = np.arange(lin.ptr[l], lin.ptr[l + 1])
        assert len(lin.observers(l)[0]) == 0 and res["obs_ok"][o].all() and not res["cross_cov"][o].any()
        want = lin.Jl[o] @ lin.Hinv[l] @ lin.Jl[o].transpose(0, 2, 1)
        assert np.abs(res["obs_cov"][o] - want).max() <= ou.C_BOUND * max(ref["h"], ou.H_FLOOR) * np.abs(want).max()
        # behind: one zero block inside a live track, served; its cross block is the (keyframe, landmark) block all the same
        ob = b.special["behind_obs"]
        assert not lin.Jl[ob].any() and res["obs_ok"][ob] == 1 and not res["obs_cov"][ob].any() and not res["obs_res"][ob].any()
        assert res["obs_cov"][lin.ptr[b.special["behind"]]].any()
        l2 = b.special["two"]
        assert lin.ptr[l2 + 1] - lin.ptr[l2] == 2 and res["obs_ok"][lin.ptr[l2]:lin.ptr[l2 + 1]].all()


def test_degenerate_landmark_is_not_served(shared):
    """The largest point of a width with one more degenerate landmark: a track of G + 1 moved behind all its observers, H_ll = 0 exactly at
    mu = 0: obs_ok = 0 and zero blocks on all its observations and nothing else."""
    G = 8
    pt = lf.LARGE[G]
    b = lf.build(pt, "pinhole")
    taken = {v for k, v in b.special.items() if k != "behind_obs"}
    l = next(int(s) for s in np.nonzero(b.lengths == G + 1)[0] if int(s) not in taken)
    prob = lu.landmark_behind_its_observers(b.p, l)
    opt = backend.default_options(visual_only=1)
    ref = ou.reference(prob, True, 0.0, key=("cut-behind", pt.id))
    res = shared["ctx"].observation_covariances(prob, opt, mu=0.0, **ALL)
    _point(shared, pt.id + "-behind mu=0", res, ref, prob, opt, 0.0, G=G, expect_bad_lm=1)
    o = np.arange(prob.lm_obs_ptr[l], prob.lm_obs_ptr[l + 1])
    assert len(o) == G + 1 and not res["obs_ok"][o].any() and res["lm_ok"][l] == 0 and res["stats"]["observations_not_ok"] == G + 1
    assert not res["obs_cov"][o].any() and not res["cross_cov"][o].any()


@pytest.mark.parametrize("pt", SMALL_VI, ids=[p.id for p in SMALL_VI])
def test_small_visual_inertial(shared, pt):
    ctx = shared["ctx"]
    prob, opt = fu.point_problem(pt), fu.point_options(pt)
    sample = lu.sample_landmarks(prob)
    with fu.forced_env(pt, leaf_too=True):
        ctx.upload(prob, opt)
        for mu in MUS:
            ref = ou.reference(prob, False, mu, key="small", sample=sample)
            res = ctx.observation_covariances_resident(opt, mu=mu, **ALL)
            tag = f"{pt.id} mu={mu:g}"
            _point(shared, tag, res, ref, prob, opt, mu, landmark_call=False)
            lm = ctx.landmark_covariances_resident(opt, mu=mu, want_kf=True)
            assert np.array_equal(lm[0], res["lm_cov"]) and np.array_equal(lm[1], res["lm_ok"]) and np.array_equal(lm[2], res["kf_cov"]), tag
            # a second call returns the same bits; so does every subset of the optional outputs, and the one-call form
            assert _same(ctx.observation_covariances_resident(opt, mu=mu, **ALL), res), tag
            for drop in ("want_cross", "want_res", "want_lm", "want_kf"):
                part = ctx.observation_covariances_resident(opt, mu=mu, **{**ALL, drop: False})
                gone = {"want_cross": ("cross_cov",), "want_res": ("obs_res",), "want_lm": ("lm_cov", "lm_ok"), "want_kf": ("kf_cov",)}[drop]
                assert all(part[f] is None for f in gone) and _same(part, res, [f for f in FIELDS if f not in gone]), (tag, drop)
            bare = ctx.observation_covariances_resident(opt, mu=mu, want_cross=False, want_res=False)
            assert _same(bare, res, ("obs_cov", "obs_ok")) and bare["cross_cov"] is None and bare["lm_cov"] is None, tag
            assert _same(ctx.observation_covariances(prob, opt, mu=mu, **ALL), res), tag
            if shared["first"] is None:
                shared["first"] = (pt, mu, res)


def test_repeat_on_a_fresh_context_is_bit_identical(shared):
    if shared["first"] is None:
        test_small_visual_inertial(shared, SMALL_VI[0])
    pt, mu, res = shared["first"]
    prob, opt = fu.point_problem(pt), fu.point_options(pt)
    c = backend.Context(0)
    try:
        with fu.forced_env(pt, leaf_too=True):
            for _ in range(2):   # (the second with history)
                assert _same(c.observation_covariances(prob, opt, mu=mu, **ALL), res)
    finally:
        c.close()


def test_constant_pose_observers(shared):
    """`small`, visual-only, with keyframes marked constant: one landmark with one constant observer among free ones, one with all observers
    constant (zero cross blocks, C_o = J_l H_ll^-1 J_l^T, obs_ok = 1)."""
    pt = fu._pt("small", None, True, 0)
    prob = fu.point_problem(pt).copy()
    nobs = np.diff(prob.lm_obs_ptr)
    l_all = int(np.flatnonzero(nobs == nobs.min())[0])
    kall = set(int(k) for k in prob.obs_kf[prob.lm_obs_ptr[l_all]:prob.lm_obs_ptr[l_all + 1]])
    l_one = next(l for l in range(prob.L) if nobs[l] >= 4 and not kall & set(int(k) for k in prob.obs_kf[prob.lm_obs_ptr[l]:prob.lm_obs_ptr[l + 1]]))
    k_one = int(prob.obs_kf[prob.lm_obs_ptr[l_one] + 1])
    prob.kf_fixed[list(kall) + [k_one]] = 1
    opt = fu.point_options(pt)
    ref = ou.reference(prob, True, 0.0, key="small-fixed", sample=sorted(set(lu.sample_landmarks(prob).tolist() + [l_all, l_one])))
    lin = ref["lin"]
    assert len(lin.observers(l_all)[0]) == 0 and len(lin.observers(l_one)[0]) == nobs[l_one] - 1 >= 3
    res = shared["ctx"].observation_covariances(prob, opt, mu=0.0, **ALL)
    _point(shared, "small-fixed", res, ref, prob, opt, 0.0)
    o = np.arange(lin.ptr[l_all], lin.ptr[l_all + 1])
    assert res["obs_ok"][o].all() and not res["cross_cov"][o].any()
    o1 = lin.ptr[l_one] + 1
    assert not res["cross_cov"][o1].any() and res["cross_cov"][o1 - 1].any() and res["obs_cov"][o1].any()
    assert res["stats"]["constant_observers"] >= len(o) + 1


def test_unified_cameras(shared):
    """g8-L450 on the mixed cameras of tests/test_gpu_omni.py through the UNI instantiation: the references come from the numpy restatement of
    the unified model."""
    pt = lf.LARGE[8]
    prob = lf.build(pt, "unified").p
    assert pt.id == "g8-L450" and prob.cam_model is not None and (np.asarray(prob.cam_model) == 1).any()
    opt = backend.default_options(visual_only=1)
    ref = ou.reference(prob, True, MU_CUT, key=("cut-unified", pt.id), unified=True)
    res = shared["ctx"].observation_covariances(prob, opt, mu=MU_CUT, **ALL)
    _point(shared, "unified " + pt.id, res, ref, prob, opt, MU_CUT, G=8)


def test_resident_call_between_two_solves_leaves_the_second_its_bits():
    pt = fu._pt("small", None, False, 0)
    prob = fu.point_problem(pt)
    opt = fu.point_options(pt, max_iterations=3)
    a, b, c = backend.Context(0), backend.Context(0), backend.Context(0)
    try:
        a.upload(prob, opt); ra1 = a.solve_resident(opt); qa1 = a.download()
        got = a.observation_covariances_resident(opt, mu=0.0, **ALL)
        ra2 = a.solve_resident(opt); qa2 = a.download()
        b.upload(prob, opt); b.solve_resident(opt); rb2 = b.solve_resident(opt); qb2 = b.download()
        for f in ("kf_pose", "kf_speed_bias", "lm_pos"):
            assert np.array_equal(getattr(qa2, f), getattr(qb2, f)), f
            assert np.array_equal(getattr(qa2, f), getattr(qa1, f)), f
        assert ra2.final_cost == rb2.final_cost == ra1.final_cost and ra2.iterations == rb2.iterations
        # the resident call at the solve's estimate == the one-call form at the downloaded estimate, bit for bit
        one = c.observation_covariances(qa1, opt, mu=0.0, **ALL)
        assert _same(got, one) and got["obs_ok"].all() and got["stats"] == one["stats"]
    finally:
        a.close(); b.close(); c.close()


def test_after_a_two_round_solve(shared):
    """The resident call after covgpu_gba_two_round works on the second round's compacted observation stream: it must match routes A and B on
    the downloaded estimate with the erased observations (the result's flags) removed, in that order."""
    from oracle import covo
    from tests import structure_util as su
    pt = fu._pt("small", None, True, 0)
    prob = fu.point_problem(pt).copy()
    nobs = np.diff(prob.lm_obs_ptr)
    l3 = int(np.flatnonzero(nobs == 3)[0]); l9 = int(np.flatnonzero(nobs >= 9)[0])
    rows = np.array([prob.lm_obs_ptr[l3], prob.lm_obs_ptr[l3] + 1, prob.lm_obs_ptr[l9] + 4])
    prob.obs_uv[rows] += np.float32(lf.OUTLIER_PX)
    th = lf.OUTLIER_THRESHOLD
    norms = covo.residual_norms(prob, covo.default_options(visual_only=1))
    assert (norms[rows] > th + 0.5 * (1.0 - th)).all(), norms[rows]
    opt = backend.default_options(max_iterations=4, visual_only=1)
    ctx = shared["ctx"]
    sol, r1, r2, erase, left, (nb, ns) = ctx.gba_two_round(prob, opt, th)
    assert erase[rows].all() and nb == int(erase.sum()) >= 3 and ns == int((left < 2).sum()) >= 1 and left[l3] < 2
    q, keep = su.compact(sol, erase)
    assert q.L == prob.L - ns and keep.sum() == q.L and not keep[l3] and q.O <= prob.O - nb
    res = ctx.observation_covariances_resident(opt, mu=0.0, num_obs=q.O, num_lm=q.L, **ALL)
    ref = ou.reference(q, True, 0.0, key="small-round2", sample=lu.sample_landmarks(q))
    print(f"two-round: erased {nb}, landmarks left out {ns} of {prob.L}, observations {q.O} of {prob.O}")
    _point(shared, "small-round2", res, ref, q, opt, 0.0, G=res["stats"]["group_width"], landmark_call=False)
    lm = ctx.landmark_covariances_resident(opt, mu=0.0, want_kf=True, num_lm=q.L)
    assert np.array_equal(lm[0], res["lm_cov"]) and np.array_equal(lm[1], res["lm_ok"]) and np.array_equal(lm[2], res["kf_cov"])


def test_facade_shim_returns_the_python_calls_bits(shared):
    from covins_amd import mapdata, synth
    from tests.facade_util import StandinMap
    m = synth.make_map(synth.config_named("tiny"))
    lib = ou.shim()
    sm = StandinMap(m)
    dp, ll = C.POINTER(C.c_double), C.POINTER(C.c_longlong)
    try:
        # (tiny visual-only is not positive definite without damping: that case runs at the damping of a solve's first iteration)
        for visual_only, mu in ((False, 0.0), (True, 1e-4)):
            prob, idx = mapdata.flatten_gba(m, visual_only, loop_loss=True)
            prob, moved = mu_.facade_problem(sm, prob, visual_only)   # the same problem in the facade's bits (tests/marginal_util.py)
            opt = backend.default_options(visual_only=1 if visual_only else 0)
            res = shared["ctx"].observation_covariances(prob, opt, mu=mu)
            cap = prob.O
            oc = np.zeros((cap, 2, 2)); cc = np.zeros((cap, 6, 3)); ok = np.zeros(cap, np.uint8)
            lm_id = np.zeros((cap, 2), np.int64); kf_id = np.zeros((cap, 2), np.int64)
            n = C.c_longlong(0); stats = (C.c_longlong * 8)(); msg = C.create_string_buffer(256)
            rc = lib.shim_observation_covariances(sm.h, int(visual_only), mu, cap, oc.ctypes.data_as(dp), cc.ctypes.data_as(dp),
                                                  ok.ctypes.data_as(C.POINTER(C.c_ubyte)), lm_id.ctypes.data_as(ll), kf_id.ctypes.data_as(ll),
                                                  C.byref(n), stats, msg)
            assert rc == 0, msg.value
            assert n.value == prob.O and ok.any()
            assert np.array_equal(oc, res["obs_cov"]) and np.array_equal(cc, res["cross_cov"]) and np.array_equal(ok, res["obs_ok"])
            assert [int(v) for v in stats] == [res["stats"][k] for k in capi.OBSCOV_STATS]
            # one record per observation, landmark-major: the landmark id is constant along a track and changes between tracks
            ptr = np.asarray(prob.lm_obs_ptr)
            first = lm_id[ptr[:-1]]
            assert np.array_equal(lm_id, np.repeat(first, np.diff(ptr), axis=0)) and len({tuple(v) for v in first}) == prob.L
            kf_first = {}
            for o, k in enumerate(np.asarray(prob.obs_kf)):
                assert kf_first.setdefault(int(k), tuple(kf_id[o])) == tuple(kf_id[o])
            assert len(set(kf_first.values())) == len(kf_first)
        rc = lib.shim_observation_covariances(sm.h, 1, -1.0, cap, oc.ctypes.data_as(dp), cc.ctypes.data_as(dp), ok.ctypes.data_as(C.POINTER(C.c_ubyte)),
                                              lm_id.ctypes.data_as(ll), kf_id.ctypes.data_as(ll), C.byref(n), None, msg)
        assert rc == 1 and b"mu negative or not finite" in msg.value, msg.value
    finally:
        sm.close()


def test_refusals_that_depend_on_the_context(shared):
    ctx = shared["ctx"]
    prob = mu_.pgo_problem("small")
    opt = backend.default_options()
    ctx.upload(prob, opt, pgo=True)
    with pytest.raises(backend.CovGpuError, match="pose graph"):
        ctx.observation_covariances_resident(opt)
    fresh = backend.Context(0)
    try:
        with pytest.raises(backend.CovGpuError, match="no problem uploaded"):
            fresh.observation_covariances_resident(opt)
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
            sc.observation_covariances(gprob, gopt)
        with pytest.raises(backend.CovGpuError, match="sharded context"):
            sc.observation_covariances_resident(gopt)
        sc.set_shard_none()
    finally:
        sc.close(); grp.close()


def test_worst_ratios_of_the_file(shared):
    assert backend.obscov_limits()["block_doubles"] == 4    # (the figures below are this library's)
    for tag, w in shared["ratios"].items():
        assert max(w[:4]) <= ou.C_BOUND and w[4] <= ou.C_SELF, (tag, w)
        print(f"worst ratios {tag}: block vs A {w[0]:.2f}  vs B {w[1]:.2f}  cross vs A {w[2]:.2f}  vs B {w[3]:.2f}  self {w[4]:.2f}")
