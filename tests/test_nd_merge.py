"""Amalgamation of thin levels of the elimination tree (nd_plan.hip: nd_amalgamate, switch COVGPU_ND_MERGE) — host only.

Where the caller leaves the tree to the planner (leaf 0), whole levels are merged into the level above if the refitted cost model says it pays.
Checked here on the small map and on the 3-agent map cut to 200 keyframes per agent, with the switch on (default) and off: the merged plan is
shorter, owns every variable exactly once, keeps levels = node heights and parents in front of their children, is deterministic, and its numpy
replay (tests/test_nd_plan) on the ORACLE's system equals the dense solve; a forced leaf size keeps its tree; shard plans and pose-graph plans are
never merged and ignore the switch."""
import os

import numpy as np
import pytest

from covins_amd import backend, distrib
from tests import forms_util as fu
from tests.test_nd_plan import _plan, _replay_sparse

MAPS = {"small": fu._pt("small", None, False, 0), "mh123@200": fu._pt("mh123", 200, False, 0)}
MU = 1e-4


class merge_switch:
    """COVGPU_ND_MERGE for the length of a `with` (read by nd_plan_build on every call); None: unset = the default, on."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get("COVGPU_ND_MERGE")
        os.environ.pop("COVGPU_ND_MERGE", None)
        if self.value is not None:
            os.environ["COVGPU_ND_MERGE"] = self.value

    def __exit__(self, *a):
        os.environ.pop("COVGPU_ND_MERGE", None)
        if self.old is not None:
            os.environ["COVGPU_ND_MERGE"] = self.old


_plans = {}


def plan(name, switch, leaf=0):
    key = (name, switch, leaf)
    if key not in _plans:
        pt = MAPS[name]
        with fu.forced_env(pt), merge_switch(switch):
            _plans[key] = _plan(fu.point_problem(pt), fu.point_options(pt), leaf)
    return _plans[key]


def dims(vs):
    return sum(9 if int(v) & 1 else 6 for v in vs)


def serial_panels(p):
    info, parent, level, own, st = p
    od = np.array([dims(o) for o in own])
    return sum(-(-int(od[level == l].max()) // 256) for l in range(info[1]))


@pytest.mark.parametrize("name", list(MAPS))
def test_merged_plan_is_shorter(name):
    off, on, on1 = plan(name, "0"), plan(name, None), plan(name, "1")
    print(f"{name}: fronts {off[0][0]} -> {on[0][0]}, levels {off[0][1]} -> {on[0][1]}, serial panels {serial_panels(off)} -> {serial_panels(on)}, "
          f"flops {off[0][6]:.3e} -> {on[0][6]:.3e}")
    assert on[0][1] < off[0][1] or serial_panels(on) < serial_panels(off)
    assert on[0][1] <= off[0][1] and serial_panels(on) <= serial_panels(off)
    # unset and "1" are the same plan
    assert on[0] == on1[0] and np.array_equal(on[1], on1[1]) and all(np.array_equal(a, b) for a, b in zip(on[3], on1[3]))


@pytest.mark.parametrize("name", list(MAPS))
@pytest.mark.parametrize("switch", ["0", None])
def test_tree_is_well_formed_and_deterministic(name, switch):
    info, parent, level, own, st = plan(name, switch)
    K = fu.point_problem(MAPS[name]).K
    owned = np.concatenate(own)
    assert len(owned) == 2 * K and np.array_equal(np.sort(owned), np.arange(2 * K))     # every variable exactly once
    h = np.zeros(len(parent), int)
    for k in range(len(parent) - 1, -1, -1):
        if parent[k] >= 0:
            assert parent[k] < k                                                       # a parent's index is below its children's
            h[parent[k]] = max(h[parent[k]], h[k] + 1)
    assert np.array_equal(h, level)                                                    # levels are node heights
    assert info[1] == level.max() + 1
    pt = MAPS[name]
    with fu.forced_env(pt), merge_switch(switch):
        again = _plan(fu.point_problem(pt), fu.point_options(pt), 0)
    assert again[0] == info and np.array_equal(again[1], parent) and np.array_equal(again[2], level)
    assert all(np.array_equal(a, b) for a, b in zip(again[3], own)) and all(np.array_equal(a, b) for a, b in zip(again[4], st))


@pytest.mark.parametrize("name", list(MAPS))
@pytest.mark.parametrize("switch", ["0", None])
def test_replay_equals_dense_solve(name, switch):
    sysm = fu.host_system(MAPS[name], MU)        # the oracle's S, b and the dense LAPACK solution (n <= 9 000)
    info, parent, level, own, st = plan(name, switch)
    x = _replay_sparse(sysm["S"], sysm["b"], parent, level, own, st, sysm["D"])
    xd = sysm["x_d"]
    assert xd is not None
    assert np.abs(x - xd).max() <= 1e-9 * np.abs(xd).max()


def test_forced_leaf_keeps_its_tree():
    for name, leaf in (("small", 90), ("mh123@200", 256)):
        a, b = plan(name, "0", leaf), plan(name, None, leaf)
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
        assert all(np.array_equal(x, y) for x, y in zip(a[3], b[3])) and all(np.array_equal(x, y) for x, y in zip(a[4], b[4]))


def _same_plan(a, b):
    return (a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and all(np.array_equal(x, y) for x, y in zip(a[3], b[3]))
            and all(np.array_equal(x, y) for x, y in zip(a[4], b[4])))


def _shard_plan_arrays(p, world, switch):
    import ctypes as C
    with merge_switch(switch):
        pl = distrib.shard_plan(p, backend.default_options(), world)
    assert pl is not None and pl.subtrees >= 2
    try:
        lib = backend.lib()
        info = (C.c_int64 * 16)()
        lib.covgpu_nd_plan_info(pl.handle, info)
        nn = int(info[0])
        parent = np.zeros(nn, np.int32); level = np.zeros(nn, np.int32); optr = np.zeros(nn + 1, np.int32); sptr = np.zeros(nn + 1, np.int32)
        ov = np.zeros(max(int(info[3]), 1), np.int32); sv = np.zeros(max(int(info[4]), 1), np.int32)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        lib.covgpu_nd_plan_arrays(pl.handle, ip(parent), ip(level), ip(optr), ip(ov), ip(sptr), ip(sv))
        return list(info), parent, level, ov.copy(), sv.copy(), np.asarray(pl.node_rank).copy(), distrib.plan_digest(pl)
    finally:
        pl.close()


@pytest.mark.parametrize("world", [2, 4])
def test_shard_plans_ignore_the_switch(world):
    """Shard plans are NOT merged (covgpu_shard_plan prescribes the cut of the agents, and its tree must stay the one that COVGPU_ND_TOP / COVGPU_ND_LEAF
    rebuild on one GPU): this guards exactly that — the plans with the switch on and off are one plan, array for array — and that the plan is
    well-formed as tests/test_shard_dist_plan.py asks of today's plans (every node has a rank or is top, the top is ancestor-closed). It is no
    coverage of merged shard plans: there are none."""
    p = fu.point_problem(MAPS["mh123@200"])
    on, off = _shard_plan_arrays(p, world, None), _shard_plan_arrays(p, world, "0")
    assert on[0] == off[0] and on[6] == off[6] and all(np.array_equal(a, b) for a, b in zip(on[1:6], off[1:6]))
    info, parent, level, ov, sv, rank, _ = on
    assert len(rank) == info[0] and ((rank >= -1) & (rank < world)).all()              # every node has a rank or is top
    top = rank < 0
    assert top[parent < 0].all()
    assert all(top[parent[n]] for n in np.nonzero(top)[0] if parent[n] >= 0)           # the top is ancestor-closed
    assert all(rank[parent[n]] in (-1, rank[n]) for n in np.nonzero(~top)[0])          # a subtree belongs to one rank
    # and the default one-GPU plan of the same map IS merged: the shard plan's tree is not it
    assert plan("mh123@200", None)[0][1] < plan("mh123@200", "0")[0][1]


def test_pose_graph_plan_ignores_the_switch():
    """The pose graph's tree (6-dof fronts, covgpu_nd_plan_create_pgo and the pose-graph upload) is never merged: the model was fitted on
    visual-inertial fronts only."""
    from covins_amd import mapdata, synth
    cfg = synth.config_named("mh123")
    cfg.max_kf_per_agent = 120
    cfg.drift_trans = 0.05; cfg.drift_yaw_deg = 0.5
    p = mapdata.flatten_pgo(synth.make_map(cfg), {}, mapdata.PgoParams())[0]
    with merge_switch(None):
        on = _plan(p, backend.default_options(), 0, pgo=True)
    with merge_switch("0"):
        off = _plan(p, backend.default_options(), 0, pgo=True)
    assert on[0][0] > 3 and _same_plan(on, off)
