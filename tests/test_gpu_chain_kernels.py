"""The two small kernels between two panel factorisations of the serial chain (k_panel.hip: k_trsm_sub4, k_chol.hip: k_diag_update), at the
shapes where they can go wrong, against host solvers only — never against another run of the device.

  1. widths: TWO points of tests/forms_util.SWEEP chosen on the CPU (forms_util.plan_shape) so that the real interior orders of their levels select
     all four widths of k_trsm_sub4 in panels that HAVE rows below them (the last panel of a root has none) and one root front has three panels
     (two look-ahead updates of a next diagonal block: k_diag_update, the second with 64 real columns in the block it updates). The device steps
     are held to the spread of the host solvers by the rule of test_gpu_forms.test_sweep_point, and the census must show, over the two points,
     every width and k_diag_update.
  2. dense solves (Context.solve_reduced) at n = 257, 300, 513, 770 — rows h only | rows h and rest rows | an odd tile count with an eight-block
     last panel | three panels — on two constructions in which the rows below a panel carry weight:
       ill-scaled     the construction of test_gpu_parity.test_mfma_cholesky_ill_scaled (dense off the diagonal, scales 1e2 / 3e3 / 3e6 with
                      period 15, i.e. the whole span inside every 64-column block);
       6x6 blocks     of condition 1e10 as in test_mfma_cholesky_ill_conditioned_blocks, with the coupling term U U^T raised from U ~ 1e-5 to
                      U ~ COUPLING = 0.1: off-diagonal entries of ~0.06 beside block entries of ~1 (there 6e-10: the rows below a panel were
                      negligible). U U^T is positive semi-definite, so the sum stays positive definite at any scale; np.linalg.cholesky checks it.
     Bounds, both with the margin of 10x that test_mfma_cholesky_ill_conditioned_blocks grants and a floor of 1e-16: the device's backward error
     against the oracle's own (covo.solve_reduced on the same matrix), and the device's scaled error (forms_util.scaled_err against a solution
     refined in extended precision) against the oracle's own scaled error. Observed on one MI355X (device | oracle): ill-scaled 1.0e-15 .. 3.3e-15 |
     1.6e-15 .. 3.6e-15 scaled, 1e-20 | 2e-20 backward; 6x6 blocks 1.4e-6 .. 3.9e-6 | 1.3e-6 .. 3.6e-6 scaled (condition 5e10 .. 1e11), 0.9e-16 .. 1.1e-16 |
     1.0e-16 .. 1.1e-16 backward.
     The oracle alone must stay inside the absolute bounds of those two tests (1e-13 backward, 1e-8 scaled) before an input is relied on.
  3. a level of two panels with fronts whose real columns end INSIDE a 32-column chunk of the first panel (own = 156, 168, 216 beside fronts of
     264 .. 342): k_diag_update with a K range cut by GemmArgs::own whose last chunk holds identity padding. Held as in 1.
"""
import numpy as np
import pytest

from covins_amd import backend
from oracle import covo
from tests import forms_util as fu
from tests.test_gpu_forms import C_BOUND, H_FLOOR, R_FLOOR

pytestmark = pytest.mark.gpu

WIDTHS_POINTS = ["mh01-vo-leaf128",   # levels of 108, 108, 234, 180, 120 real columns (8, 8, 16, 12, 8) under a root of 576 = 256 + 256 + 64
                 "small-leaf128"]     # levels of 126, 48, 51, 93, 105 (8, 4, 4, 8, 8) under a root of 624
CUT_POINT = "mh01-vo-leaf384"        # bottom level: two panels, fronts of 156 .. 342 real columns
COUPLING = 0.1
SIZES = [257, 300, 513, 770]


def _point(name):
    return [p for p in fu.SWEEP if p.id == name][0]


def _launch_widths(shape):
    """Widths of k_trsm_sub4 the plan selects: per level and panel with rows below it (a later panel of the level, or a border), the 16-column
    blocks that hold real columns of the level's widest front."""
    out = set()
    for om, tiles in zip(shape["lev_own_max"], shape["lev_tiles"]):
        npan = (om + 255) // 256
        for P in range(npan):
            if P + 1 < npan or tiles > 2 * npan:
                nb = min(16, (om - 256 * P + 15) // 16)
                out.add(4 * ((nb + 3) // 4))
    return out


@pytest.fixture(scope="module")
def ctx():
    c = backend.Context(0)
    yield c
    c.close()


def _held_to_host_spread(ctx, pt):
    """One damped Gauss-Newton step per damping of the point, by the rule of test_gpu_forms.test_sweep_point; returns the census of the last."""
    forms = None
    for mu in pt.mus:
        with fu.forced_env(pt, leaf_too=True):
            dx, dl, cost = ctx.gn_step(fu.point_problem(pt), fu.point_options(pt), mu)
            forms = ctx.kernel_forms()
        sysm = fu.host_system(pt, mu)
        h, r_h, xs = fu.host_spread(pt, mu)
        err = fu.scaled_err(dx, sysm["x_ref"], sysm["d"])
        res = float(np.linalg.norm(sysm["S"] @ dx - sysm["b"]) / np.linalg.norm(sysm["b"]))
        print(f"{pt.id} mu={mu:g}: n={sysm['n']} h={h:.2e} r_h={r_h:.2e} | device err={err:.2e} ({err / max(h, H_FLOOR):.2f} h) residual={res:.2e} "
              f"({res / max(r_h, R_FLOOR):.2f} r_h) | " + ", ".join(f"{k}={v}" for k, v in forms.items() if v))
        assert abs(cost - sysm["cost"]) <= 1e-10 * sysm["cost"]
        assert err <= C_BOUND * max(h, H_FLOOR), (err, h)
        assert res <= C_BOUND * max(r_h, R_FLOOR), (res, r_h)
    return forms


def test_every_width_and_the_diagonal_update(ctx):
    pts = [_point(name) for name in WIDTHS_POINTS]
    shapes = [fu.plan_shape(pt) for pt in pts]
    assert set().union(*[_launch_widths(s) for s in shapes]) == {4, 8, 12, 16}, [s["lev_own_max"] for s in shapes]
    assert max(int(((s["own"] + 255) // 256).max()) for s in shapes) >= 3
    assert all(fu.host_system(pt, pt.mus[0])["n"] <= 3288 for pt in pts)
    ran = {}
    for pt in pts:
        for k, v in _held_to_host_spread(ctx, pt).items():
            ran[k] = ran.get(k, 0) + v
    for w in (4, 8, 12, 16):
        assert ran[f"k_trsm_sub4<{w}>"] > 0, (w, ran)
    assert ran["k_diag_update"] > 0, ran


def test_front_ending_inside_a_chunk_of_a_non_last_panel(ctx):
    pt = _point(CUT_POINT)
    shape = fu.plan_shape(pt)
    cut = []
    for l in range(shape["levels"]):
        npan = (shape["lev_own_max"][l] + 255) // 256
        cut += [int(v) for v in shape["own"][shape["level"] == l] if npan >= 2 and v < 256 * (npan - 1) and v % 32]
    assert cut, "no front of this plan ends inside a 32-column chunk of a non-last panel"
    forms = _held_to_host_spread(ctx, pt)
    assert forms["k_diag_update"] > 0, forms


# ---- dense solves
def ill_scaled(n):
    rng = np.random.default_rng(5)
    A = rng.normal(0, 1, (n, 2 * n)); S = A @ A.T / n + np.eye(n)
    d = np.resize(np.array([1e2] * 6 + [3e3] * 3 + [3e6] * 6), n)
    return S * d[:, None] * d[None, :], rng.normal(0, 1, n) * d


def coupled_blocks(n):
    rng = np.random.default_rng(17)
    m = -(-n // 6) * 6
    S = np.zeros((m, m))
    for i in range(0, m, 6):
        R, _ = np.linalg.qr(rng.normal(0, 1, (6, 6)))
        S[i:i + 6, i:i + 6] = R @ np.diag([1.0, 0.7, 0.4, 1e-10, 3e-10, 6e-10]) @ R.T
    U = rng.normal(0, 1, (m, 40)) * COUPLING
    S += U @ U.T
    S = 0.5 * (S + S.T)[:n, :n]      # (a leading principal block of a positive definite matrix)
    return S, rng.normal(0, 1, n)


def refined(S, b):
    """The solution to working precision of the extended type: LAPACK solve, three steps of refinement with residuals in np.longdouble."""
    Sl, bl = S.astype(np.longdouble), b.astype(np.longdouble)
    x = np.linalg.solve(S, b).astype(np.longdouble)
    for _ in range(3):
        x = x + np.linalg.solve(S, (bl - Sl @ x).astype(np.float64)).astype(np.longdouble)
    return x.astype(np.float64)


def backward_error(S, x, b):
    return float(np.linalg.norm(S @ x - b) / (np.linalg.norm(S, 2) * np.linalg.norm(x) + np.linalg.norm(b)))


_dense = {}


def dense_case(kind, n):
    """(S, b, d, x_ref, the oracle's backward error, the oracle's scaled error), built once."""
    if (kind, n) not in _dense:
        S, b = (ill_scaled if kind == "ill_scaled" else coupled_blocks)(n)
        np.linalg.cholesky(S)            # positive definite
        rc0, xo = covo.solve_reduced(S, b)
        assert rc0 == 0
        d = np.sqrt(np.diag(S))
        x_ref = refined(S, b)
        _dense[(kind, n)] = (S, b, d, x_ref, backward_error(S, xo, b), fu.scaled_err(xo, x_ref, d))
    return _dense[(kind, n)]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["ill_scaled", "coupled_blocks"])
def test_dense_solve_where_the_substitution_carries_weight(ctx, kind, n):
    S, b, d, x_ref, back0, err0 = dense_case(kind, n)
    assert back0 < 1e-13 and (kind != "ill_scaled" or err0 < 1e-8), (back0, err0)     # the oracle alone is inside the bounds of the two parity tests
    rc, x = ctx.solve_reduced(S, b)
    assert rc == 0
    back, err = backward_error(S, x, b), fu.scaled_err(x, x_ref, d)
    print(f"{kind} n={n}: backward error device {back:.2e} oracle {back0:.2e} | scaled error device {err:.2e} oracle {err0:.2e}")
    assert back < 10 * max(back0, 1e-16), (back, back0)
    assert err < 10 * max(err0, 1e-16), (err, err0)
