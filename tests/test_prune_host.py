"""Redundant-keyframe pruning, host side: the C structs against the header, the argument checks of
covgpu_prune_redundant (they run before any device work: covgpu_prune_check runs them without a context), the integer rule of
tests/prune_ref.py against the reference's literal arithmetic, and SlamMap.remove_keyframes. No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from covins_amd import backend, capi, mapdata, synth
from tests import prune_ref as pr
from tests import prune_util as pu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_struct_sizes_match_the_header(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "covgpu.h"\nint main(void) { printf("%zu %zu %zu %zu %zu\\n", '
                   "sizeof(covgpu_prune_t), sizeof(covgpu_prune_opts), offsetof(covgpu_prune_t, capacity), offsetof(covgpu_prune_t, loop_ms), "
                   "offsetof(covgpu_prune_opts, max_rounds)); return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(capi.PruneBatch), C.sizeof(capi.PruneOpts), capi.PruneBatch.capacity.offset, capi.PruneBatch.loop_ms.offset,
                   capi.PruneOpts.max_rounds.offset]


def test_defaults_and_null_context():
    o = capi.PruneOpts()
    backend.lib().covgpu_default_prune_opts(C.byref(o))
    assert (o.th_red, o.max_time_dist, o.max_kfs, o.max_rounds) == (0.95, 1.0, -1, 0)        # config_backend.yaml:58-59
    assert (pr.DEFAULT_OPTS["th_red"], pr.DEFAULT_OPTS["max_time_dist"]) == (0.95, 1.0)
    assert backend.lib().covgpu_prune_redundant(None, C.byref(capi.PruneBatch()), C.byref(o)) == 1
    assert backend.lib().covgpu_last_error() == b"covgpu_prune_redundant: NULL context"


def _check(inp, drop=(), capacity=None, **opts):
    """covgpu_prune_check of the inputs; `drop`: struct fields passed as NULL."""
    s, o, out, keep = backend.Context._prune_batch(inp["lm_obs_ptr"], inp["obs_kf"], inp["kf_pred"], inp["kf_succ"], inp["kf_time"],
                                                   inp["lm_invalid"], inp["kf_invalid"], inp["kf_first"], inp["kf_loop"], inp["kf_not_erase"],
                                                   capacity, opts)
    for f in drop:
        setattr(s, f, None)
    rc = backend.lib().covgpu_prune_check(C.byref(s), C.byref(o))
    return rc, backend.lib().covgpu_last_error().decode()


def test_invalid_arguments_are_rejected_before_any_device_work():
    good = pu.hand_cases()["buckets"][0]
    assert _check(good)[0] == 0
    assert _check(pu.empty_case())[0] == 0                                    # K = 0, L = 0
    assert _check(pu.hand_cases()["no_landmarks"][0])[0] == 0 and _check(pu.hand_cases()["no_candidates"][0])[0] == 0
    # every optional array may be NULL
    assert _check(good, drop=("lm_invalid", "kf_invalid", "kf_first", "kf_loop", "kf_not_erase", "num_rounds", "removed", "stop_reason",
                              "kf_pred_out", "kf_succ_out", "lm_nobs", "red_num", "red_den"))[0] == 0
    assert _check(good, drop=("round_kf", "round_action"), capacity=0)[0] == 0

    def bad(msg, inp=good, **kw):
        rc, err = _check(inp, **kw)
        assert rc == 1 and err.startswith("covgpu_prune_check: ") and msg in err, (msg, rc, err)

    for f in ("lm_obs_ptr", "obs_kf", "kf_pred", "kf_succ", "kf_time", "round_kf", "round_action"):
        bad("NULL", drop=(f,))
    assert backend.lib().covgpu_prune_check(None, None) == 1
    ptr = good["lm_obs_ptr"].copy(); ptr[2], ptr[3] = ptr[3], ptr[2] - 1
    bad("not monotone", dict(good, lm_obs_ptr=ptr))
    ptr = good["lm_obs_ptr"].copy(); ptr[0] = 1
    bad("lm_obs_ptr[0]", dict(good, lm_obs_ptr=ptr))
    for v in (-1, good["K"]):
        obs = good["obs_kf"].copy(); obs[5] = v
        bad("obs_kf out of range", dict(good, obs_kf=obs))
    for name in ("kf_pred", "kf_succ"):
        for v in (-2, good["K"]):
            a = good[name].copy(); a[3] = v
            bad("out of range", dict(good, **{name: a}))
    a = good["kf_pred"].copy(); a[4] = 2                                      # succ[2] is 3, not 4
    bad("not mutual", dict(good, kf_pred=a))
    a = good["kf_succ"].copy(); a[4] = 6                                      # pred[6] is 5, not 4
    bad("not mutual", dict(good, kf_succ=a))
    for v in (np.nan, np.inf):
        bad("non-finite", th_red=v)
        bad("non-finite", max_time_dist=v)
        t = good["kf_time"].copy(); t[1] = v
        bad("non-finite kf_time", dict(good, kf_time=t))
    bad("negative", capacity=-1)


def test_hand_cases_do_what_they_are_for():
    c = pu.hand_cases()
    run = lambda n: pr.prune_exact(c[n][0], **c[n][1])
    r = run("ties");             assert r["round_kf"].tolist() == [1] and r["stop_reason"] == 1 and r["red_num"][1] == 50 and r["red_den"][1] == 5
    r = run("den0");             assert r["round_kf"].tolist() == [1, 3, 2] and r["red_den"][2] == 0 and r["stop_reason"] == 2
    r = run("two_to_one");       assert r["round_kf"].tolist() == [1] and r["lm_nobs"][3] == 1 and (r["red_num"][2], r["red_den"][2]) == (21, 3)
    r = run("buckets");          assert r["round_kf"].tolist() == [1, 2] and r["lm_nobs"].tolist() == [5, 4, 3, 2, 1, 0]
    r = run("time_equal");       assert r["round_action"].tolist() == [1, 1, 1, 1] and r["removed"] == 0 and r["stop_reason"] == 0
    r = run("time_below");       assert r["round_action"][0] == 0 and r["removed"] >= 1
    r = run("loop_kf");          assert r["round_action"].tolist()[:2] == [2, 0] and r["round_kf"].tolist()[:2] == [1, 2]
    r = run("not_erase");        assert (r["round_kf"][0], r["round_action"][0]) == (1, 3) and r["removed"] == 3 and r["stop_reason"] == 2
    r = run("gates_together");   assert dict(zip(r["round_kf"].tolist(), r["round_action"].tolist())) == {1: 1, 2: 1, 3: 1, 4: 1}
    r = run("invalid");          assert 2 not in r["round_kf"].tolist() and r["red_den"][2] == 0 and r["stop_reason"] == 2
    r = run("count_stop");       assert r["stop_reason"] == 2 and r["removed"] == 3
    r = run("threshold_round0"); assert r["num_rounds"] == 0 and r["stop_reason"] == 1
    r = run("no_candidates");    assert r["num_rounds"] == 0 and r["stop_reason"] == 0
    r = run("max_rounds_1");     assert r["num_rounds"] == 1 and r["stop_reason"] == 3
    r = run("listed_twice");     assert r["stop_reason"] == 2
    r = run("no_landmarks");     assert r["round_kf"].tolist() == [1, 2] and r["stop_reason"] == 2
    r = run("threshold_no_landmarks"); assert r["num_rounds"] == 0 and r["stop_reason"] == 1
    r = pr.prune_exact(pu.empty_case()); assert r["num_rounds"] == 0 and r["stop_reason"] == 0
    stress = {n: v for n, v in pu.stress_cases().items() if not n.startswith("sparse")}   # (the sparse map: 550 rounds x 1100 literal values)
    for name, (inp, opts) in list(c.items()) + list(stress.items()):
        r = pu.stress_exact(name) if name in stress else pr.prune_exact(inp, **opts)
        pr.validate_literal(inp, list(zip(r["round_kf"], r["round_action"])), r["stop_reason"], r, **opts)


def test_stress_shapes_are_what_they_claim():
    s = pu.stress_cases()
    sp = s["sparse_count"][0]
    n = np.diff(sp["lm_obs_ptr"])
    assert sp["K"] == 1100 and sp["K"] % 64 != 0 and n.min() == 2 and n.max() == 7
    r = pu.stress_exact("sparse_count")
    assert r["num_rounds"] >= 550 and r["stop_reason"] == 2
    assert pu.stress_exact("sparse_threshold")["num_rounds"] > 50
    w = s["wide_keyframe"][0]
    assert np.bincount(w["obs_kf"])[3] == 1500
    assert 3 in pu.stress_exact("wide_keyframe")["round_kf"].tolist()
    d = s["dense_block"][0]
    r = pu.stress_exact("dense_block")
    assert np.diff(d["lm_obs_ptr"]).min() == 64 and r["removed"] == 63 and r["lm_nobs"].max() == 1


@pytest.mark.parametrize("name", ["tiny", "small"])
@pytest.mark.parametrize("thin", [False, True])
@pytest.mark.parametrize("mode", list(pu.MAP_MODES))
def test_integer_rule_is_a_literal_outcome(name, thin, mode):
    inp, opts = pu.map_case(name, thin, mode)
    r = pu.map_exact(name, thin, mode)
    pr.validate_literal(inp, list(zip(r["round_kf"], r["round_action"])), r["stop_reason"], r, **opts)
    if thin:
        n = np.diff(inp["lm_obs_ptr"])
        assert 0.40 < len(inp["obs_kf"]) / len(pu.map_inputs(name, False)["obs_kf"]) < 0.50 and np.isin(np.arange(2, 8), n).all()
    if name == "small" and (mode != "th095" or not thin):
        assert r["num_rounds"] >= 100
        assert (r["round_action"] == 1).sum() >= 10            # the time gate fires: neighbours 0.25 s apart, the third in a row is blocked
    if mode == "half":
        assert r["stop_reason"] == 2 and (r["round_action"] == 0).sum() == inp["K"] - inp["K"] // 2


def test_validate_literal_rejects_a_wrong_replay():
    inp, opts = pu.map_case("tiny", False, "th060")
    r = pu.map_exact("tiny", False, "th060")
    rounds = list(zip(r["round_kf"].tolist(), r["round_action"].tolist()))
    worst = int(np.nanargmin(np.where(pr.candidates(inp), pr.literal_values(inp, ~inp["kf_invalid"]), np.nan)))
    with pytest.raises(AssertionError):
        pr.validate_literal(inp, [(worst, 0)] + rounds, **opts)
    with pytest.raises(AssertionError):
        pr.validate_literal(inp, [(rounds[0][0], 1 - min(rounds[0][1], 1))] + rounds[1:], **opts)
    with pytest.raises(AssertionError):
        pr.validate_literal(inp, rounds[:3], r["stop_reason"], **opts)     # stops although the top value is above the threshold


@pytest.mark.parametrize("name,mode", [("tiny", "th060"), ("small", "half"), ("small", "th095")])
def test_remove_keyframes_invariants(name, mode):
    m = synth.make_map(synth.config_named(name))
    inp, opts = pu.map_case(name, False, mode)
    r = pu.map_exact(name, False, mode)
    before = m.copy()
    n = m.remove_keyframes(r)
    erased = r["round_kf"][r["round_action"] == 0]
    assert n == len(erased) > 0 and m.kf_invalid[erased].all() and m.kf_invalid.sum() == n
    assert np.array_equal(m.kf_pred, r["kf_pred"]) and np.array_equal(m.kf_succ, r["kf_succ"])
    v = np.flatnonzero(~m.kf_invalid)
    for k in v:                                                            # mutual, and inside the valid set
        if m.kf_pred[k] >= 0:
            assert m.kf_succ[m.kf_pred[k]] == k and not m.kf_invalid[m.kf_pred[k]]
        if m.kf_succ[k] >= 0:
            assert m.kf_pred[m.kf_succ[k]] == k and not m.kf_invalid[m.kf_succ[k]]
    assert not np.isin(m.obs_kf, erased).any() and np.array_equal(np.diff(m.lm_obs_ptr), r["lm_nobs"])
    assert m.imu_ptr[-1] == before.imu_ptr[-1] == len(m.imu_samples)           # every IMU sample is still there
    assert (np.diff(m.imu_ptr)[erased] == 0).all()
    # Each buffer's sum of dt equals time[kf] - time[new pred] to 1e-9. The synthetic maps stamp their keyframes with the recorded camera
    # times, which differ from the 50 x 5 ms of IMU between two keyframes by 1.28e-7 s per step before anything is pruned; so the
    # statement is checked on stamps rebuilt from the unpruned buffers (time[k] = time[pred] + sum of dt), and on the map's own stamps
    # with what the unpruned buffers of the same span already missed taken out.
    sum_dt = lambda mm, k: mm.imu_samples[mm.imu_ptr[k]:mm.imu_ptr[k + 1], 0].sum()
    stamp = before.kf_time.copy()
    miss = np.zeros(m.K)                                                   # (sum of dt) - (time step), accumulated along each chain
    for k in np.flatnonzero(before.kf_pred < 0):
        while before.kf_succ[k] >= 0:
            s = before.kf_succ[k]
            stamp[s] = stamp[k] + sum_dt(before, s)
            miss[s] = miss[k] + sum_dt(before, s) - (before.kf_time[s] - before.kf_time[k])
            k = s
    assert np.abs(stamp - before.kf_time).max() < 1e-4
    checked = 0
    for k in v:
        p = m.kf_pred[k]
        if p >= 0:
            assert abs(sum_dt(m, k) - (stamp[k] - stamp[p])) < 1e-9, k
            assert abs(sum_dt(m, k) - (m.kf_time[k] - m.kf_time[p]) - (miss[k] - miss[p])) < 1e-9, k
            checked += 1
    assert checked == len(v) - len(np.unique(m.kf_client))
    fused = [k for k in v if before.kf_pred[k] != m.kf_pred[k]]
    assert len(fused) > 0
    for k in fused:                                                        # the reading at the new predecessor
        q = before.kf_pred[k]
        while before.kf_pred[q] != m.kf_pred[k]:
            q = before.kf_pred[q]
        assert np.array_equal(m.imu_first[k], before.imu_first[q])
        assert np.array_equal(m.kf_bias_a[k], before.kf_bias_a[k])
    has = np.diff(m.lm_obs_ptr) > 0
    assert not m.kf_invalid[m.lm_ref_kf[has & (m.lm_ref_kf >= 0)]].any()
    prob, idx = mapdata.flatten_gba(m, False, True)
    assert prob.K == m.K - n and prob.I == prob.K - len(np.unique(m.kf_client))
    assert m.remove_keyframes([(int(erased[0]), 1)]) == 0                   # only action 0 erases
    with pytest.raises(ValueError):
        m.remove_keyframes([(int(erased[0]), 0)])                           # invalid already


@pytest.mark.parametrize("thin", [False, True])
@pytest.mark.parametrize("mode", ["th060", "half"])
def test_serial_restatement_is_a_literal_outcome(thin, mode):
    """tests/cpp/facade_prune_shim.cpp compiles (MapPruneT instantiates on the stand-in classes), and its serial restatement of the
    reference loop, double sums and std::stable_sort, makes choices the literal check accepts and leaves the map SetInvalid leaves. Its
    sequence is not compared with the integer rule's for equality: where two literal values lie within an ulp, the two may differ."""
    m = synth.make_map(synth.config_named("small"))
    inp, opts = pu.map_case("small", thin, mode)
    if thin:
        m.obs_kf, m.lm_obs_ptr = inp["obs_kf"], inp["lm_obs_ptr"]       # (remove_keyframes is not used on this map)
    sm = pu.StandinPruneMap(m)
    try:
        r = sm.serial(th_red=opts.get("th_red", 0.95), max_kfs=opts.get("max_kfs"))
        st = sm.state()
    finally:
        sm.close()
    assert r["num_rounds"] >= 100
    stop = 2 if mode == "half" else None
    pr.validate_literal(inp, list(zip(r["round_kf"].tolist(), r["round_action"].tolist())), stop, **opts)
    if mode == "half":
        assert r["removed"] == inp["K"] - inp["K"] // 2
    erased = r["round_kf"][r["round_action"] == 0]
    assert st["invalid"].sum() == len(erased) == st["db_erased"] and st["invalid"][erased].all()
    assert st["imu_count"].sum() == m.imu_ptr[-1] and (st["imu_count"][erased] == 0).all()
