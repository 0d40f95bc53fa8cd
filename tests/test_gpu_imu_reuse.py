"""What the inertial path keeps from one launch to the next. k_imu_build stores the whitened Jacobian of every factor (DevProblem::imu_Jw) and the J*v passes
of the same iteration read it back; the preintegration of a solve runs on the side stream beside the first linearisation. Three ways in which something kept
could be the wrong thing:

  (i)   rejected step   bias-shift under OPTS_REJECT (Levenberg-Marquardt, no reprojection loss, initial radius 1e6, min_relative_decrease 0.999): the
                        ORACLE's accept trace is [1, 0, 0, 1, 0] — asserted here — so the device re-linearises at an unchanged state twice, moves, and
                        linearises at the new state. A Jacobian left over from an earlier linearisation moves |J step|^2, the model decrease and rho, and
                        with them the accept sequence, the cost and the radius traces: held to the oracle's by tests/test_gpu_edge_cases.check (what
                        tests/test_gpu_imu.py::test_solve asks) and, per iteration, by the same bound as its final cost.
                        Found on the CPU: with the default Cauchy loss the solve points of imu_util accept every step at min_relative_decrease 1.0 and
                        none at 1.001, at initial radii from 1e2 to 1e12 no step is rejected, and a rejected step is followed by rejected ones (a smaller
                        step moves rho closer to 1 from above); without the loss the large LM steps of this point fall short of their model by up to 1e-3.
                        The oracle's trace is the same at min_relative_decrease 0.998 (at 0.9995 the fourth step is rejected too), and its costs move by
                        3e-12, its state by 7e-12 when its inputs are perturbed by 1e-14 .. 1e-12: the point is no knife's edge.
  (ii)  history         a context that has solved bias-shift (26 factors), then uploads and solves count-3, returns the cost trace and the state arrays of a
                        fresh context on count-3, bit for bit: rows of imu_Jw or pre_* beyond the live factors do not leak. (count-3's chains differ from
                        bias-shift's, so the upload builds its own elimination tree: the plan cache of up_choose_plan does not apply.)
  (iii) two solves      solve_resident twice on one context gives identical bits: the side-stream preintegration of the second solve does not race the
                        tail of the first.
"""
import time

import numpy as np
import pytest

from covins_amd import backend, capi
from oracle import covo
from tests import imu_util as iu
from tests.test_gpu_edge_cases import check

pytestmark = pytest.mark.gpu

OPTS_REJECT = dict(strategy=capi.COVGPU_LM, reproj_loss_a=0.0, initial_radius=1e6, min_relative_decrease=0.999, max_iterations=5)


@pytest.fixture(scope="module")
def ctx():
    t0 = time.perf_counter()
    c = backend.Context(0)
    yield c
    c.close()
    print(f"\ntests/test_gpu_imu_reuse.py: {time.perf_counter() - t0:.1f} s")


def test_rejected_step_then_accepted(ctx):
    p = iu.build("bias-shift")
    g, o = backend.default_options(**OPTS_REJECT), covo.default_options(**OPTS_REJECT)
    _, rres = covo.gba_solve(p, o)
    n = rres.iterations
    acc = list(rres.accepted_trace[:n])
    assert acc == [1, 0, 0, 1, 0], acc                                   # the oracle: two rejected steps, an accepted one behind them
    sol, ref = check(ctx, p, g, o)                                       # iterations, termination, accept sequence, final cost, poses
    _, res = ctx.gba_solve(p, g)
    cost, cost0 = np.array(res.cost_trace[:n]), np.array(rres.cost_trace[:n])
    rad, rad0 = np.array(res.radius_trace[:n]), np.array(rres.radius_trace[:n])
    print(f"bias-shift, rejected steps: cost trace {np.abs(cost / cost0 - 1).max():.2e}  radius trace {np.abs(rad / rad0 - 1).max():.2e}  "
          f"speed-bias {np.abs(sol.kf_speed_bias - ref.kf_speed_bias).max():.2e}")
    assert list(res.accepted_trace[:n]) == acc
    assert np.all(np.abs(cost - cost0) <= 1e-7 * cost0 + 1e-12 * rres.initial_cost)     # (check's bound on the final cost, at every iteration)
    # LM radius: halved, quartered on a rejection, times 1 / max(1/3, 1 - (2 rho - 1)^3) = 3 on these acceptances (rho > 0.99): exact factors on both sides
    assert np.all(np.abs(rad - rad0) <= 1e-7 * rad0)
    assert np.abs(sol.kf_speed_bias - ref.kf_speed_bias).max() < 1e-6
    moved = np.abs(sol.kf_speed_bias[:, 3:] - p.kf_speed_bias[:, 3:]).max()
    assert moved > 0


def _solve_fresh(p, g):
    c = backend.Context(0)
    try:
        c.upload(p, g)
        res = c.solve_resident(g)
        return c.download(), res
    finally:
        c.close()


def _same(a, b):
    (sa, ra), (sb, rb) = a, b
    n = ra.iterations
    assert n == rb.iterations and n > 0 and ra.termination == rb.termination and ra.reserved == rb.reserved
    assert list(ra.cost_trace[:n]) == list(rb.cost_trace[:n]) and list(ra.radius_trace[:n]) == list(rb.radius_trace[:n])
    assert list(ra.accepted_trace[:n]) == list(rb.accepted_trace[:n]) and ra.final_cost == rb.final_cost and ra.initial_cost == rb.initial_cost
    assert np.array_equal(sa.kf_pose, sb.kf_pose) and np.array_equal(sa.kf_speed_bias, sb.kf_speed_bias) and np.array_equal(sa.lm_pos, sb.lm_pos)


def test_history_does_not_leak(ctx):
    big, small = iu.build("bias-shift"), iu.build("count-3")
    assert big.I == 26 and small.I == 3
    g = backend.default_options(max_iterations=5)
    ctx.upload(big, g)
    r0 = ctx.solve_resident(g)
    assert r0.iterations == 5 and r0.accepted > 0
    ctx.upload(small, g)
    after = (None, ctx.solve_resident(g))
    after = (ctx.download(), after[1])
    fresh = _solve_fresh(small, g)
    assert np.abs(after[0].kf_speed_bias - small.kf_speed_bias).max() > 0     # the solve moved the state
    _same(after, fresh)


def test_two_solves_on_one_context(ctx):
    p = iu.build("ragged-fused")
    g = backend.default_options(max_iterations=5)
    ctx.upload(p, g)
    out = []
    for _ in range(2):
        res = ctx.solve_resident(g)                                      # every solve restarts from the uploaded state
        out.append((ctx.download(), res))
    assert out[0][1].accepted > 0
    _same(out[0], out[1])
