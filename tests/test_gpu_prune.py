"""covgpu_prune_redundant on the GPU against tests/prune_ref.prune_exact, bit for bit: the rounds, the actions, the
reference's count, the stop reason, the relinked chain, the observation counts and every keyframe's num / den. Integer arithmetic on
both sides, so there is no tolerance."""
import ctypes as C

import numpy as np
import pytest

from covins_amd import backend, capi, mapdata, optimization, synth
from oracle import covo
from tests import prune_ref as pr
from tests import prune_util as pu
from tests.util import rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = backend.Context(0)
    yield c
    c.close()


def run(ctx, inp, **opts):
    return ctx.prune_redundant(inp["lm_obs_ptr"], inp["obs_kf"], inp["kf_pred"], inp["kf_succ"], inp["kf_time"], inp["lm_invalid"],
                               inp["kf_invalid"], inp["kf_first"], inp["kf_loop"], inp["kf_not_erase"], **opts)


@pytest.mark.parametrize("name", list(pu.hand_cases()))
def test_hand_built_cases(ctx, name):
    inp, opts = pu.hand_cases()[name]
    pu.assert_same(run(ctx, inp, **opts), pr.prune_exact(inp, **opts), name)


def test_flag_arrays_may_be_null(ctx):
    inp, opts = pu.hand_cases()["count_stop"]
    got = ctx.prune_redundant(inp["lm_obs_ptr"], inp["obs_kf"], inp["kf_pred"], inp["kf_succ"], inp["kf_time"], kf_first=inp["kf_first"], **opts)
    pu.assert_same(got, pr.prune_exact(inp, **opts))
    got = ctx.prune_redundant(inp["lm_obs_ptr"], inp["obs_kf"], inp["kf_pred"], inp["kf_succ"], inp["kf_time"], **opts)   # keyframe 0 a candidate? no: no predecessor
    pu.assert_same(got, pr.prune_exact(dict(inp, kf_first=np.zeros(inp["K"], bool)), **opts))


def test_empty_map(ctx):
    e = pu.empty_case()
    pu.assert_same(run(ctx, e), pr.prune_exact(e))
    pu.assert_same(run(ctx, e, max_kfs=0), pr.prune_exact(e, max_kfs=0))
    only_lm = dict(e, L=3, lm_obs_ptr=np.zeros(4, np.int32), lm_invalid=np.zeros(3, bool))     # landmarks nobody sees, no keyframe
    pu.assert_same(run(ctx, only_lm), pr.prune_exact(only_lm))


def test_capacity_smaller_than_the_round_count(ctx):
    """The true num_rounds is reported, the first `capacity` records are written and nothing past them."""
    inp, opts = pu.hand_cases()["count_stop"]
    ref = pr.prune_exact(inp, **opts)
    assert ref["num_rounds"] >= 3
    for cap in (0, 2):
        s, o, out, keep = ctx._prune_batch(inp["lm_obs_ptr"], inp["obs_kf"], inp["kf_pred"], inp["kf_succ"], inp["kf_time"], inp["lm_invalid"],
                                           inp["kf_invalid"], inp["kf_first"], inp["kf_loop"], inp["kf_not_erase"], cap, opts)
        rk, ra = np.full(16, -7, np.int32), np.full(16, -7, np.int32)
        s.round_kf, s.round_action = capi.iptr(rk), capi.iptr(ra)
        assert backend.lib().covgpu_prune_redundant(ctx._h, C.byref(s), C.byref(o)) == 0
        assert out["scal"].tolist() == [ref["num_rounds"], ref["removed"], ref["stop_reason"]]
        assert rk[:cap].tolist() == ref["round_kf"][:cap].tolist() and ra[:cap].tolist() == ref["round_action"][:cap].tolist()
        assert (rk[cap:] == -7).all() and (ra[cap:] == -7).all()
        assert np.array_equal(out["kf_pred"][:inp["K"]], ref["kf_pred"]) and np.array_equal(out["lm_nobs"][:inp["L"]], ref["lm_nobs"])
    got = run(ctx, inp, capacity=2, **opts)
    assert got["num_rounds"] == ref["num_rounds"] and got["round_kf"].tolist() == ref["round_kf"][:2].tolist()


def test_invalid_arguments_reach_no_kernel(ctx):
    inp, opts = pu.hand_cases()["count_stop"]
    obs = inp["obs_kf"].copy(); obs[0] = inp["K"]
    with pytest.raises(backend.CovGpuError, match="covgpu_prune_redundant: obs_kf out of range"):
        run(ctx, dict(inp, obs_kf=obs), **opts)
    pu.assert_same(run(ctx, inp, **opts), pr.prune_exact(inp, **opts))       # the context still works


@pytest.mark.parametrize("name", list(pu.stress_cases()))
def test_shapes_where_the_kernel_can_go_wrong(ctx, name):
    inp, opts = pu.stress_cases()[name]
    pu.assert_same(run(ctx, inp, **opts), pu.stress_exact(name), name)


def test_max_rounds_cuts_a_long_run_and_the_rest_continues(ctx):
    """Two calls of 40 rounds are not one call of 80 (the second starts from the unchanged map), but each equals the rule."""
    inp, opts = pu.stress_cases()["sparse_count"]
    for mr in (1, 40):
        pu.assert_same(run(ctx, inp, max_rounds=mr, **opts), pr.prune_exact(inp, max_rounds=mr, **opts), mr)


@pytest.mark.parametrize("name", ["tiny", "small"])
@pytest.mark.parametrize("thin", [False, True])
@pytest.mark.parametrize("mode", list(pu.MAP_MODES))
def test_synthetic_maps(ctx, name, thin, mode):
    inp, opts = pu.map_case(name, thin, mode)
    pu.assert_same(run(ctx, inp, **opts), pu.map_exact(name, thin, mode), (name, thin, mode))


def test_loop_time_is_reported_when_asked_for(ctx):
    inp, opts = pu.map_case("tiny", False, "half")
    r = ctx.prune_redundant(inp["lm_obs_ptr"], inp["obs_kf"], inp["kf_pred"], inp["kf_succ"], inp["kf_time"], kf_first=inp["kf_first"],
                            kf_loop=inp["kf_loop"], loop_ms=True, **opts)
    pu.assert_same(r, pu.map_exact("tiny", False, "half"))
    assert 0.0 < r["loop_ms"] < 1000.0


def test_prune_apply_flatten_preintegrate_solve():
    """The chain a caller runs: prune `small` to K/2 through optimization.remove_redundant_data, flatten the pruned map, preintegrate the
    fused IMU buffers on the device against the oracle on the same samples (tolerances of tests/test_gpu_parity.py::test_preintegration),
    and solve the pruned problem."""
    m = synth.make_map(synth.config_named("small"))
    ctx = backend.Context(0)
    try:
        info = {}
        removed = optimization.remove_redundant_data(m, ctx, max_kfs=m.K // 2, info=info)
        ref = pu.map_exact("small", False, "half")
        pu.assert_same(info, ref)
        assert removed == ref["removed"] and (~m.kf_invalid).sum() == m.K // 2
        prob, idx = mapdata.flatten_gba(m, False, True)
        assert prob.K == m.K // 2 and prob.I == prob.K - 3 and np.diff(prob.imu_sample_ptr).max() >= 100   # fused buffers: two steps and more
        g, o = backend.default_options(), covo.default_options()
        d, J, P = ctx.preintegrate(prob, g)
        d0, J0, P0 = covo.preintegrate(prob, o)
        assert rel_err(d, d0) < 1e-12 and rel_err(J, J0) < 1e-11
        assert np.max(np.abs(P - P0) / np.abs(P0).max(axis=1, keepdims=True)) < 1e-11
        sol, res = ctx.gba_solve(prob, backend.default_options(max_iterations=5))
        assert res.termination != 4 and res.final_cost <= res.initial_cost
    finally:
        ctx.close()


@pytest.mark.parametrize("mode", ["th095", "half"])
def test_facade_equals_the_python_mirror(mode):
    """MapPruneT::RemoveRedundantData on a stand-in map built from `small`: the same rounds and the same count as the Python mirror, and
    the map its own EraseKeyframeWithDatabase leaves equals SlamMap.remove_keyframes: chain, fused IMU buffers, database."""
    m = synth.make_map(synth.config_named("small"))
    _, opts = pu.map_case("small", False, mode)
    sm = pu.StandinPruneMap(m)
    try:
        r = sm.facade(th_red=opts.get("th_red", 0.95), max_kfs=opts.get("max_kfs"))
        st = sm.state()
    finally:
        sm.close()
        pu.prune_shim().prune_shutdown()
    ref = pu.map_exact("small", False, mode)
    assert r["round_kf"].tolist() == ref["round_kf"].tolist() and r["round_action"].tolist() == ref["round_action"].tolist()
    assert r["removed"] == ref["removed"]
    m.remove_keyframes(ref)
    assert np.array_equal(st["invalid"].astype(bool), m.kf_invalid) and st["db_erased"] == m.kf_invalid.sum()
    v = ~m.kf_invalid
    assert np.array_equal(st["pred"][v], m.kf_pred[v]) and np.array_equal(st["succ"][v], m.kf_succ[v])
    assert np.array_equal(st["imu_count"], np.diff(m.imu_ptr)) and np.array_equal(st["imu_first"][v], m.imu_first[v])
    assert np.array_equal(st["num_landmarks"], np.bincount(m.obs_kf, minlength=m.K))


def test_facade_counts_a_refused_erase():
    """not_erase_: SetInvalid refuses, the keyframe stays, the returned count includes it (keyframe_be.cpp:510, map_be.cpp:776-777)."""
    m = synth.make_map(synth.config_named("tiny"))
    ne = np.zeros(m.K, bool); ne[pu.map_exact("tiny", False, "half")["round_kf"][:2]] = True
    inp = pr.inputs_of_map(m, ne)
    ref = pr.prune_exact(inp, max_kfs=m.K // 2)
    assert (ref["round_action"] == 3).sum() == 2
    sm = pu.StandinPruneMap(m, ne)
    try:
        r = sm.facade(max_kfs=m.K // 2)
        st = sm.state()
    finally:
        sm.close()
        pu.prune_shim().prune_shutdown()
    assert r["round_kf"].tolist() == ref["round_kf"].tolist() and r["round_action"].tolist() == ref["round_action"].tolist()
    assert r["removed"] == ref["removed"] == (ref["round_action"] == 0).sum() + 2
    assert st["invalid"].sum() == (ref["round_action"] == 0).sum() and st["db_erased"] == ref["removed"]
