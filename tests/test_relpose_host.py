"""The relative-pose oracle (oracle/covo_relpose.cpp) alone, on the inputs of tests/relpose_util.py: proof that every regime reaches the
branches of the trust-region loop it is named for, so that tests/test_gpu_relpose.py, which compares the kernel with the oracle on the same
inputs, cannot pass without the kernel having taken them. No GPU.

Reached, and asserted below: accepted and rejected Gauss-Newton steps, the linearisation reuse after one and after two rejections in a row
(`radius *= 0.5` each time), accepted steps with rho < 0.25 (the halving on acceptance), radius-limited steps of the interpolation branch
with c > 0, the empty-system exit (gmax <= 1e-10, nothing projects: H is zero, so is every H[k][k] the diagonal substitution looks at), the
convergence exit, the min_inliers gate from both sides.

NOT reached by the reference on any of these inputs (so no test here or on the GPU claims them):
  - the Cauchy step (g_norm * alpha >= radius);
  - the interpolation with c <= 0;
  - a failed 6x6 factorisation, and with it the damping retry (mu *= 10 inside the solve) and the `mu >= 1` exit;
  - a non-positive model.
On the equidistant pairs (dist_type 1) of `wide` no radius-limited step occurred under any of 100 seeds tried (a rejected equidistant solve
mostly rejects all five of its steps); that condition is asserted on the radial-tangential pairs of `wide` and on both types of `far`."""
import numpy as np
import pytest

from oracle import covo
from tests import relpose_util as ru

REGIMES = ("near", "mid", "far", "wide", "stride", "few", "unnormalised")


def _rejected(rows):
    return np.isfinite(ru.col(rows, "rho")) & (ru.col(rows, "accepted") == 0)


def _twice_in_a_row(rows):
    """Two consecutive rejections inside one solve: the second one runs on the reused alpha, gh and gn."""
    for s in (0, 1):
        r = _rejected(rows)[ru.col(rows, "solve") == s]
        if (r[1:] & r[:-1]).any():
            return True
    return False


def _radius_limited(rows):
    return ru.col(rows, "step") >= 1


def _nothing_projects(r):
    rows = r["rows"]
    return len(r["out"]) > 0 and len(rows) > 0 and ru.kind_is(rows[:1], "kind", "stopped_gmax")[0]


def _normalised(T):
    return np.concatenate([T[:4] / np.sqrt(T[0] * T[0] + T[1] * T[1] + T[2] * T[2] + T[3] * T[3]), T[4:]])


@pytest.mark.parametrize("dist_type", [0, 1])
@pytest.mark.parametrize("name", REGIMES)
def test_the_traced_entry_point_returns_the_bits_of_the_plain_one(name, dist_type):
    bt = ru.regime(name, dist_type)
    for th in ru.TH:
        for b, r in enumerate(ru.reference(name, dist_type, th)):
            n, T, out = covo.relpose(*ru.pair_args(bt, b), bt["T0"][b], th_outlier=th, min_inliers=ru.min_inliers_of(name))
            assert n == r["n"] and T.tobytes() == r["T"].tobytes() and np.array_equal(out, r["out"]), (th, b)
            rows = r["rows"]
            assert len(rows) <= 10 and (np.diff(ru.col(rows, "solve")) >= 0).all()
            assert r["norms"].shape == (len(out), 2)
            assert np.array_equal(out, (r["norms"] > th).any(axis=1))


@pytest.mark.parametrize("dist_type", [0, 1])
@pytest.mark.parametrize("name", REGIMES)
def test_at_most_a_tenth_of_a_regime_is_too_close_to_call(name, dist_type):
    for th in ru.TH:
        assert len(ru.selected(name, dist_type, th)) == ru._SIZES[name]       # (the cap is asserted inside)


@pytest.mark.parametrize("dist_type", [0, 1])
def test_the_cost_entry_point_is_the_objective_of_the_solve(dist_type):
    bt = ru.regime("mid", dist_type)
    for b, r in enumerate(ru.reference("mid", dist_type, 0.9)):
        rows = r["rows"]
        # (the loop's own cost comes out of the linearisation, which sums the same terms beside the Jacobians: equal up to rounding)
        assert covo.relpose_cost(bt["T0"][b], *ru.pair_args(bt, b)) == pytest.approx(ru.col(rows, "cost")[0], rel=1e-12)
        if r["n"]:       # the last linearisation of the second solve is not traced, but an accepted last step leaves cost_new as the final cost
            last = rows[-1]
            if ru.col(last[None], "accepted")[0] == 1:
                assert covo.relpose_cost(r["T"], *ru.pair_args(bt, b), outlier=r["out"]) == pytest.approx(ru.col(last[None], "cost_new")[0], rel=1e-12)


@pytest.mark.parametrize("dist_type", [0, 1])
def test_near_takes_accepted_gauss_newton_steps_only(dist_type):
    """What the suite covered before: the start of tests/util.py::make_relpose_batch."""
    for th in ru.TH:
        for r in ru.reference("near", dist_type, th):
            rows = r["rows"]
            assert not _rejected(rows).any() and ru.kind_is(rows, "step", "gauss_newton").all() and (ru.col(rows, "accepted") == 1).all()


@pytest.mark.parametrize("dist_type", [0, 1])
def test_mid_rejects_steps_and_reuses_the_linearisation(dist_type):
    for th in ru.TH:
        assert any(_twice_in_a_row(r["rows"]) for r in ru.reference("mid", dist_type, th))
    ref = ru.reference("mid", dist_type, 1.3)        # (at 0.9 the pairs that miss the min_inliers gate have no second solve)
    assert sum(int(_rejected(r["rows"]).sum()) for r in ref) >= 20
    assert any(((ru.col(r["rows"], "accepted") == 1) & (ru.col(r["rows"], "rho") < 0.25)).any() for r in ref)


@pytest.mark.parametrize("name, dist_type", [("far", 0), ("far", 1), ("wide", 0)])
def test_far_and_wide_take_radius_limited_steps(name, dist_type):
    for th in ru.TH:
        ref = ru.reference(name, dist_type, th)
        assert any(_radius_limited(r["rows"]).any() for r in ref)
        # a radius-limited step is taken on a radius that rejections halved, and some are accepted
    assert any((_radius_limited(r["rows"]) & (ru.col(r["rows"], "accepted") == 1)).any() for r in ru.reference(name, dist_type, 1.3))


@pytest.mark.parametrize("name", ["mid", "far", "wide", "stride"])
def test_radius_limited_steps_count_in_the_device_comparison(name):
    """A rejected Gauss-Newton step on the initial radius of 1e4 changes no result by itself: the halvings show in T_AB only once the radius
    falls below gn_norm. So the device comparison has teeth where a SELECTED pair that returns a pose took a radius-limited step: the
    radial-tangential pairs of these four regimes at 1.3. (Equidistant: the only such pair found under 80 seeds ran away and is left out.)"""
    ref, sel = ru.reference(name, 0, 1.3), ru.selected(name, 0, 1.3)
    assert any(sel[b] and r["n"] > 0 and _radius_limited(r["rows"]).any() for b, r in enumerate(ref))


@pytest.mark.parametrize("dist_type", [0, 1])
@pytest.mark.parametrize("name", ["far", "wide"])
def test_a_solve_in_which_nothing_projects_returns_its_start(name, dist_type):
    bt = ru.regime(name, dist_type)
    for th in ru.TH:
        ref = ru.reference(name, dist_type, th)
        hit = [b for b, r in enumerate(ref) if _nothing_projects(r)]
        assert hit
        for b in hit:
            r = ref[b]
            # zero residuals everywhere: nothing is flagged, every correspondence counts, the second solve stops the same way
            assert not r["out"].any() and r["n"] == len(r["out"]) and not r["norms"].any()
            assert ru.kind_is(r["rows"], "kind", "stopped_gmax").all() and len(r["rows"]) == 2
            assert np.abs(r["T"] - _normalised(bt["T0"][b])).max() <= 4.5e-16


@pytest.mark.parametrize("dist_type", [0, 1])
def test_stride_sizes_leave_the_gauss_newton_path_too(dist_type):
    bt = ru.regime("stride", dist_type)
    assert sorted(set(np.diff(bt["ptr"]))) == sorted(ru.STRIDE_N)
    ref = ru.reference("stride", dist_type, 1.3)
    # rejected steps both where the lanes pass over the correspondences once and where they pass more often
    assert sum(int(_rejected(r["rows"]).sum()) for r in ref) >= 20
    assert any(_rejected(r["rows"]).any() for r in ref if len(r["out"]) <= 64) and any(_rejected(r["rows"]).any() for r in ref if len(r["out"]) > 64)


@pytest.mark.parametrize("dist_type", [0, 1])
def test_few_correspondences(dist_type):
    bt = ru.regime("few", dist_type)
    assert sorted(set(np.diff(bt["ptr"]))) == [0, 1, 2, 3, 4]
    kinds = set()
    for th in ru.TH:
        for b, r in enumerate(ru.reference("few", dist_type, th)):
            n = len(r["out"])
            assert np.isfinite(r["T"]).all() and np.isfinite(r["norms"]).all() and 0 <= r["n"] <= n
            assert r["n"] == n - r["out"].sum()          # min_inliers = 0: the gate never closes
            kinds |= {covo.RELPOSE_KINDS[int(k)] for k in ru.col(r["rows"], "kind")}
            if n == 0:
                assert r["n"] == 0 and ru.kind_is(r["rows"], "kind", "stopped_gmax").all() and len(r["rows"]) == 2
                assert np.abs(r["T"] - _normalised(bt["T0"][b])).max() <= 4.5e-16
    # the kinds that occur on these sizes
    assert kinds == {"gauss_newton", "stopped_gmax", "stopped_converged"}


@pytest.mark.parametrize("dist_type", [0, 1])
def test_gate_both_sides_of_min_inliers(dist_type):
    bt, cases = ru.gate_cases(dist_type)
    assert len(cases) >= 6
    for b, th_in, th_out in cases:
        args = ru.pair_args(bt, b)
        n, T, out, tr = covo.relpose(*args, bt["T0"][b], th_outlier=th_in, min_inliers=ru.MIN_INLIERS, trace=True)
        assert (~out).sum() == ru.MIN_INLIERS and n == ru.MIN_INLIERS
        assert (ru.col(tr["rows"], "solve") == 1).any() and T.tobytes() != bt["T0"][b].tobytes()
        n, T, out, tr = covo.relpose(*args, bt["T0"][b], th_outlier=th_out, min_inliers=ru.MIN_INLIERS, trace=True)
        assert (~out).sum() == ru.MIN_INLIERS - 1 and n == 0
        assert T.tobytes() == bt["T0"][b].tobytes()                                  # the pose bytes are the input's
        assert np.array_equal(out, (tr["norms"] > th_out).any(axis=1)) and out.any()  # the flags of the first pass are written
        assert not (ru.col(tr["rows"], "solve") == 1).any()
        assert np.abs(tr["norms"] - th_in).min() >= 4e-5 and np.abs(tr["norms"] - th_out).min() >= 4e-5


@pytest.mark.parametrize("dist_type", [0, 1])
def test_unnormalised_quaternions(dist_type):
    bt = ru.regime("unnormalised", dist_type)
    scale = np.linalg.norm(bt["T0"][:, :4], axis=1)
    assert {0.5, 3.0, 1.0} == set(np.round(scale, 12)) and (bt["T0"][:, 3] < 0).sum() >= 8
    unit = dict(bt, T0=np.array([_normalised(T) for T in bt["T0"]]))
    ref1 = ru.run_oracle(unit, 0.9, ru.MIN_INLIERS)
    zero = set()
    for b, (r, r1) in enumerate(zip(ru.reference("unnormalised", dist_type, 0.9), ref1)):
        assert r["n"] == r1["n"] and np.array_equal(r["out"], r1["out"])
        if r["n"] == 0:
            assert r["T"].tobytes() == bt["T0"][b].tobytes()      # untouched means unnormalised
            zero.add(ru.UNNORMALISED_SCALE[b % 4])
        else:
            assert abs(np.linalg.norm(r["T"][:4]) - 1) <= 1e-15 and np.abs(r["T"] - r1["T"]).max() <= 1e-9
    assert zero == set(ru.UNNORMALISED_SCALE)
