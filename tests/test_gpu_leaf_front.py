"""The one-launch leaf form of the panel factorisation (k_panel.hip: k_potrf_leaf) and its place in the schedule.

A bottom level of the elimination tree whose fronts own speed-bias blocks only, with own <= 128, border <= 128 and at most 384 fronts (leaf_front.hpp:
leaf_level_eligible; decided at upload, NdLevel::leaf_one) is factored whole by ONE launch — factor, L21, Schur complement and the right-hand side
that rides along — on the head stream beside the landmark pass; the serial chain of the solve starts at level 1. Everything else keeps the panel route.

Shapes, found on the CPU with tests/forms_util.plan_shape (level 0 of each point: fronts | own | border | largest own + border):

  small-leaf15        60 | 9 .. 9     | 21 .. 36  |  45    the smallest own order there is: ONE 16-block, ending inside it; the smallest border
  small-leaf60        36 | 18 .. 54   | 39 .. 66  | 120    two to four own blocks
  small-leaf128       18 | 54 .. 126  | 51 .. 114 | 240    own = 126 (eight blocks, the last two columns padding), the largest border and the largest own + border the maps give
  small-leafdefault   15 | 99 .. 108  | 81 .. 96  | 195    the default plan (3 levels: level 1 is the last level below the root)
  mh01-leaf128 (VI)   70 | 27 .. 81   | 48 .. 84  | 165    another map
  not taken:  mh01-vo-leaf128 (visual-only: pose blocks), mh123-leaf15 (494 fronts: the four-wave form), mh123@200-leaf1920 (own up to 171, own + border up
  to 315). No point of the maps has a bottom level of one front (the smallest has 15).

Every own order is a multiple of 9, so every one but 144 ends inside a 16-block. Every step is held by the rule of test_gpu_forms.test_sweep_point (the
host solvers' spread, its constants imported). The census: k_potrf_leaf counts the FRONTS the form took (= the plan's level-0 fronts, or 0), and every level
on the panel route below the root issues exactly one split last update (last_update_split) with its substitution — levels - 2 of them when level 0 is
the leaf form's, levels - 1 otherwise.

Observed on one MI355X: against COVGPU_LEAF_ONE=0 the steps differ by 1e-14 .. 1e-13 relative at mu 1e-4 (the Schur complements are summed in 16-column
steps instead of by k_trsm_sub4 + k_gemm_abt_q: not bit-identical, and not promised to be); beside the pass | on the chain (COVGPU_LEAF_ONE=2) | device
flags | HIP events are bit-identical among themselves.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from covins_amd import backend, mapdata
from tests import forms_util as fu
from tests.test_gpu_forms import C_BOUND, H_FLOOR, R_FLOOR

pytestmark = pytest.mark.gpu

HELPER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "leaf_solve.py")


def _sweep(map_, kf, vo, leaf):
    """The SWEEP point of this shape (its host references are shared with tests/test_gpu_forms.py), or a new point."""
    for p in fu.SWEEP:
        if (p.map, p.kf, p.visual_only, p.leaf) == (map_, kf, vo, leaf) and not p.env:
            return p
    return fu._pt(map_, kf, vo, leaf)


TAKEN = [_sweep("small", None, False, 15), _sweep("small", None, False, 60), _sweep("small", None, False, 128), _sweep("small", None, False, 0),
         _sweep("mh01", None, False, 128)]
NOT_TAKEN = [_sweep("mh01", None, True, 128), fu.FOUR_WAVE, _sweep("mh123", 200, False, 1920)]


@pytest.fixture(scope="module")
def ctx():
    c = backend.Context(0)
    yield c
    c.close()


def _eligible(pt, shape, own_vars):
    l0 = shape["level"] == 0
    od, bd = shape["own"][l0], shape["border"][l0]
    sb_only = not pt.visual_only and all(all(int(v) & 1 for v in own_vars[i]) for i in np.nonzero(l0)[0])
    return bool(sb_only and shape["levels"] >= 2 and len(od) <= fu.K_SMALL_MIN and od.max() <= 128 and bd.max() <= 128 and (od + bd).max() <= 256), od, bd


def _held_step(ctx, pt, mu):
    with fu.forced_env(pt, leaf_too=True):
        dx, dl, cost = ctx.gn_step(fu.point_problem(pt), fu.point_options(pt), mu)
        forms = ctx.kernel_forms()
    sysm = fu.host_system(pt, mu)
    h, r_h, xs = fu.host_spread(pt, mu)
    err = fu.scaled_err(dx, sysm["x_ref"], sysm["d"])
    res = float(np.linalg.norm(sysm["S"] @ dx - sysm["b"]) / np.linalg.norm(sysm["b"]))
    print(f"{pt.id} mu={mu:g}: n={sysm['n']} host {'/'.join(sorted(xs))} h={h:.2e} r_h={r_h:.2e} | device err={err:.2e} ({err / max(h, H_FLOOR):.2f} h) "
          f"residual={res:.2e} ({res / max(r_h, R_FLOOR):.2f} r_h) | k_potrf_leaf={forms['k_potrf_leaf']} last_update_split={forms['last_update_split']}")
    assert abs(cost - sysm["cost"]) <= 1e-10 * sysm["cost"]
    assert err <= C_BOUND * max(h, H_FLOOR), (err, h)
    assert res <= C_BOUND * max(r_h, R_FLOOR), (res, r_h)
    return forms


@pytest.mark.parametrize("pt", TAKEN, ids=[p.id for p in TAKEN])
def test_leaf_level_against_host_solvers(ctx, pt):
    plan = fu.host_plan(pt)
    shape = fu.plan_shape(pt, plan)
    ok, od, bd = _eligible(pt, shape, plan[3])
    print(f"{pt.id}: level 0 has {len(od)} fronts, own {od.min()} .. {od.max()}, border {bd.min()} .. {bd.max()}, own + border <= {(od + bd).max()}")
    assert ok, "the point was chosen for a bottom level the leaf form takes"
    panels = int(((shape["own"] + 255) // 256).sum())
    for mu in ((1e-4, 1e-8) if pt.map == "small" else (1e-4,)):   # (the small map's references take a second each, the other's ten)
        forms = _held_step(ctx, pt, mu)
        assert forms["k_potrf_leaf"] == len(od), "every front of level 0, in the one launch"
        assert forms["k_potrf_panel.fronts"] + forms["k_potrf_panel4.fronts"] == panels
        assert forms["last_update_split"] == shape["levels"] - 2, "no substitution / update launch of the panel route for level 0"


def test_the_edges_of_the_form_are_among_the_points():
    """own = 9 (one block) and 126, the smallest and the largest border, the largest own + border: the shapes the cases above are there for."""
    own, border, total = [], [], []
    for pt in TAKEN:
        plan = fu.host_plan(pt)
        ok, od, bd = _eligible(pt, fu.plan_shape(pt, plan), plan[3])
        assert ok
        own += list(od); border += list(bd); total += list(od + bd)
    assert min(own) == 9 and max(own) == 126 and any(o % 16 for o in own)
    assert min(border) == 21 and max(border) == 114 and max(total) == 240


@pytest.mark.parametrize("pt", NOT_TAKEN, ids=[p.id for p in NOT_TAKEN])
def test_ineligible_levels_keep_the_panel_route(ctx, pt):
    plan = fu.host_plan(pt)
    shape = fu.plan_shape(pt, plan)
    ok, od, bd = _eligible(pt, shape, plan[3])
    print(f"{pt.id}: level 0 has {len(od)} fronts, own {od.min()} .. {od.max()}, border {bd.min()} .. {bd.max()}, own + border <= {(od + bd).max()}, visual-only {pt.visual_only}")
    assert not ok
    forms = _held_step(ctx, pt, 1e-4)
    assert forms["k_potrf_leaf"] == 0
    assert forms["last_update_split"] == shape["levels"] - 1


def test_no_stale_border():
    """The border x border accumulators start from zero in the kernel and the tiles are never cleared in memory: a second step on the same context, at
    another damping and another state, must leave exactly what a fresh context leaves."""
    pt = _sweep("small", None, False, 128)
    m = fu.point_map(pt).copy()
    rng = np.random.default_rng(7)
    m.kf_velocity = m.kf_velocity + 0.05 * rng.standard_normal(m.kf_velocity.shape)
    m.kf_pose = m.kf_pose.copy(); m.kf_pose[:, :3] += 0.01 * rng.standard_normal((m.kf_pose.shape[0], 3))
    p2 = mapdata.flatten_gba(m, visual_only=False, loop_loss=True)[0]
    a, b = backend.Context(0), backend.Context(0)
    try:
        with fu.forced_env(pt, leaf_too=True):
            first = a.gn_step(fu.point_problem(pt), fu.point_options(pt), 1e-4)
            second = a.gn_step(p2, fu.point_options(pt), 1e-6)
            assert a.kernel_forms()["k_potrf_leaf"] > 0
            fresh = b.gn_step(p2, fu.point_options(pt), 1e-6)
        assert not np.array_equal(first[0], second[0])
        assert second[2] == fresh[2] and np.array_equal(second[0], fresh[0]) and np.array_equal(second[1], fresh[1]), np.abs(second[0] - fresh[0]).max()
    finally:
        a.close(); b.close()


_solves = {}


def _solve(tmp_path_factory, name, **env):
    key = (name,) + tuple(sorted(env.items()))
    if key not in _solves:
        out = str(tmp_path_factory.mktemp("leaf") / "solve.npz")
        r = subprocess.run([sys.executable, HELPER, name, "10", out], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        _solves[key] = np.load(out)
    return _solves[key]


@pytest.mark.parametrize("name", ["small", "mh01"])
def test_device_flags_and_events_give_the_same_bits(tmp_path_factory, name):
    a = _solve(tmp_path_factory, name)
    b = _solve(tmp_path_factory, name, COVGPU_GATES="0")
    assert int(a["leaf_fronts"]) > 0 and int(b["leaf_fronts"]) > 0, "the leaf form ran in both"
    assert int(a["ordering"]) == 1, "device flags, and neither a time-out nor the fall-back to events"
    assert int(b["ordering"]) == 0
    for k in ("pose", "sb", "lm", "cost", "acc"):
        assert np.array_equal(a[k], b[k]), f"device-flag ordering and event ordering differ in {k}"


def test_whole_solve_against_the_panel_route(tmp_path_factory):
    """mh01, 10 iterations: the default against COVGPU_LEAF_ONE=0 (level 0 on the panel route) — the same accept sequence and the cost trace to 1e-8, the
    bound tests/test_gpu_schedule.py holds between kernel forms of one solve — and against COVGPU_LEAF_ONE=2 (the same launch at level 0's old place on
    the chain: the same arithmetic, so the same bits)."""
    a = _solve(tmp_path_factory, "mh01")
    b = _solve(tmp_path_factory, "mh01", COVGPU_LEAF_ONE="0")
    c = _solve(tmp_path_factory, "mh01", COVGPU_LEAF_ONE="2")
    assert int(a["leaf_fronts"]) > 0 and int(b["leaf_fronts"]) == 0 and int(c["leaf_fronts"]) == int(a["leaf_fronts"])
    assert int(b["split_updates"]) > int(a["split_updates"])
    assert np.array_equal(a["acc"], b["acc"]), (a["acc"], b["acc"])
    rel = np.abs(a["cost"] - b["cost"]) / np.abs(b["cost"])
    print("cost trace, default against COVGPU_LEAF_ONE=0: largest relative difference", rel.max())
    assert rel.max() <= 1e-8, rel
    for k in ("pose", "sb", "lm", "cost", "acc"):
        assert np.array_equal(a[k], c[k]), f"beside the pass and on the chain differ in {k}: a dependency between the streams is missing"
