"""The amalgamated elimination tree (nd_plan.hip: nd_amalgamate, COVGPU_ND_MERGE) on the device: the same solve in another elimination order.

One damped Gauss-Newton step of the small map and of the 3-agent map at 200 keyframes per agent on the default plan, with the switch on and
off, each held to the spread of the host solvers of the oracle's system by the criterion and bound of tests/test_gpu_forms.py; the device must
have run the tree the host plan shows (tests/test_nd_merge.py says where the two differ). Then one whole 10-iteration solve of the small map on
both trees: the same accept / reject sequence, poses within 1e-9 m, cost traces within 1e-8 relative."""
import numpy as np
import pytest

from covins_amd import backend
from tests import forms_util as fu
from tests.test_gpu_forms import C_BOUND, H_FLOOR, R_FLOOR
from tests.test_nd_merge import MAPS, MU, merge_switch, plan
from tests.test_nd_plan import _replay_sparse

pytestmark = pytest.mark.gpu

def _linear_solve(name, switch):
    pt = MAPS[name]
    ctx = backend.Context(0)
    try:
        with fu.forced_env(pt, leaf_too=True), merge_switch(switch):
            dx, dl, cost = ctx.gn_step(fu.point_problem(pt), fu.point_options(pt), MU)
            lay = ctx.layout()
    finally:
        ctx.close()
    sysm = fu.host_system(pt, MU)
    # host solvers of the oracle's system: SuperLU, dense LAPACK, and the numpy replay of THIS tree
    info, parent, level, own, st = plan(name, switch)
    xs = {"lu": sysm["x_lu"], "dense": sysm["x_d"], "replay": _replay_sparse(sysm["S"], sysm["b"], parent, level, own, st, sysm["D"])}
    names = sorted(xs)
    h = max(fu.scaled_err(xs[a], xs[b], sysm["d"]) for a in names for b in names if a != b)
    nb = np.linalg.norm(sysm["b"])
    r_h = max(float(np.linalg.norm(sysm["S"] @ x - sysm["b"]) / nb) for x in xs.values())
    err = fu.scaled_err(dx, sysm["x_ref"], sysm["d"])
    res = float(np.linalg.norm(sysm["S"] @ dx - sysm["b"]) / nb)
    print(f"{name} merge {switch or 'on'}: fronts={lay['nd_fronts']} levels={lay['nd_levels']} panels={lay['nd_serial_panels']} h={h:.2e} r_h={r_h:.2e} | "
          f"device err={err:.2e} ({err / max(h, H_FLOOR):.2f} h) residual={res:.2e} ({res / max(r_h, R_FLOOR):.2f} r_h)")
    assert abs(cost - sysm["cost"]) <= 1e-10 * sysm["cost"]
    assert err <= C_BOUND * max(h, H_FLOOR), (err, h)
    assert res <= C_BOUND * max(r_h, R_FLOOR), (res, r_h)
    assert (lay["nd_fronts"], lay["nd_levels"]) == (info[0], info[1]), lay     # the device ran the tree of the host plan
    return lay["nd_fronts"], lay["nd_levels"], lay["nd_serial_panels"]


@pytest.mark.parametrize("name", list(MAPS))
def test_linear_solve_against_host_solvers(name):
    """Switch on, then off, in one body: each step against the host solvers, then the two layouts against each other."""
    on, off = _linear_solve(name, None), _linear_solve(name, "0")
    host_on, host_off = plan(name, None)[0], plan(name, "0")[0]
    assert (on[1] != off[1]) == (host_on[1] != host_off[1]), (on, off)        # levels differ where the host plans' do
    assert on != off, (on, off)                                                 # and the two trees are two trees


def test_whole_solve_on_both_trees():
    pt = MAPS["small"]
    out = {}
    for switch in (None, "0"):
        ctx = backend.Context(0)
        try:
            with fu.forced_env(pt, leaf_too=True), merge_switch(switch):
                sol, res = ctx.gba_solve(fu.point_problem(pt), fu.point_options(pt, max_iterations=10))
                lay = ctx.layout()
        finally:
            ctx.close()
        n = res.iterations
        out[switch] = (sol.kf_pose.copy(), np.array(res.cost_trace[:n]), list(res.accepted_trace[:n]), lay)
    (pa, ca, aa, la), (pb, cb, ab, lb) = out[None], out["0"]
    print(f"small: levels {lb['nd_levels']} -> {la['nd_levels']}, panels {lb['nd_serial_panels']} -> {la['nd_serial_panels']}; poses {np.abs(pa[:, 4:] - pb[:, 4:]).max():.2e} m, "
          f"cost {np.abs(ca / cb - 1).max():.2e} relative, accepted {aa}")
    assert (la["nd_fronts"], la["nd_levels"], la["nd_serial_panels"]) != (lb["nd_fronts"], lb["nd_levels"], lb["nd_serial_panels"])
    assert aa == ab
    assert np.abs(pa[:, 4:] - pb[:, 4:]).max() <= 1e-9
    assert np.allclose(ca, cb, rtol=1e-8, atol=0.0)
