"""covgpu_ncrelpose_batch / covgpu_ncrelpose_solve_batch (k_ncrelpose.hip) against the numpy restatement
tests/ncrelpose_ref.py: the linear solve on noise-free and rank-deficient tuples, the RANSAC loop draw for draw at every size where the
kernel takes another path, the polish against scipy's least squares, the sampled covariance row for row, each status, and batch
invariance.

Tolerances are 10 x the spread between the two host routes of the checker (A: SVD and scipy; B: the kernel's formulation in numpy),
computed here on the very tuples and jobs the device is held on, once per session, and printed. Measured on the CPU: s_R 1.3e-12 rad
and s_t 2.4e-12 on the separated 17-tuples, 3e-14 / 5e-14 on the 24-tuples; polish 3e-12 rad / 3e-11; covariance 1e-9 of its largest
entry."""
import functools
import math

import numpy as np
import pytest

from covins_amd import backend
from tests import ncrelpose_ref as nr
from tests import ncrelpose_util as nu

pytestmark = pytest.mark.gpu

OPTS = dict(min_inliers=40, max_iterations=300)
FILL = -7.0


@pytest.fixture(scope="module")
def ctx():
    c = backend.Context(0)
    yield c
    c.close()


def _err(T, R, t):
    return nr.pose_error(nr.quat_rot(T[:4]), T[4:], R, t)


@pytest.mark.parametrize("N", [17, 18, 24, 32])
def test_solve_matches_route_a_on_separated_tuples(ctx, N):
    tp, y = nu.standard(N)
    out = ctx.ncrelpose_solve_batch(tp["ray1"], tp["ray2"])
    assert np.all(np.isfinite(out["T"])) and np.all(np.isfinite(out["sv"]))
    share = y["sep"].mean()
    worst_R = worst_t = worst_sv = 0.0
    for i in np.flatnonzero(y["sep"]):
        assert out["ok"][i] == 1
        dr, dt = _err(out["T"][i], *y["A"][i])
        worst_R, worst_t = max(worst_R, dr), max(worst_t, dt)
        worst_sv = max(worst_sv, abs(out["sv"][i, 0] - y["sv"][i, 0]) / y["sv"][i, 0], abs(out["sv"][i, 1] - y["sv"][i, 1]) / y["sv"][i, 0])
    print(f"N {N}: separated {share:.3f}  device against route A: R {worst_R:.3e} (s_R {y['s_R']:.3e})  t {worst_t:.3e} (s_t {y['s_t']:.3e})  sv {worst_sv:.3e}")
    assert share >= (0.9 if N == 17 else 0.99)
    assert worst_R <= 10 * y["s_R"] and worst_t <= 10 * y["s_t"] and worst_sv <= 1e-12


def test_solve_on_rank_deficient_tuples(ctx):
    """All from one camera pair with no offsets (a central system), all bearings equal, two repeated correspondences, all camera offsets
    zero: the call ends, and a tuple comes back failed or with a finite pose."""
    for N in (17, 24):
        tp = nu.tuples(4, N, seed=99)
        r1, r2 = tp["ray1"].copy(), tp["ray2"].copy()
        r1[0, :, 3:] = 0.0; r2[0, :, 3:] = 0.0                     # every camera offset zero
        r1[1, :, :] = r1[1, 0, :]; r2[1, :, :] = r2[1, 0, :]        # all bearings (and origins) equal
        r1[2, 1] = r1[2, 0]; r2[2, 1] = r2[2, 0]; r1[2, 3] = r1[2, 2]; r2[2, 3] = r2[2, 2]   # two repeated correspondences
        r1[3, :, 3:] = r1[3, 0, 3:]; r2[3, :, 3:] = r2[3, 0, 3:]    # one camera pair: one origin on each side
        out = ctx.ncrelpose_solve_batch(r1, r2)
        assert np.all(np.isfinite(out["T"])) and set(out["ok"].tolist()) <= {0, 1}
        assert np.all(out["T"][out["ok"] == 0] == 0.0)
        if N == 17:
            assert out["ok"][2] == 0                                  # 15 distinct rows: rank 15 at the most
        print(N, "rank-deficient tuples: ok", out["ok"].tolist(), "sigma_17 / sigma_1", (out["sv"][:, 1] / out["sv"][:, 0]).tolist())


@functools.lru_cache(maxsize=None)
def _reference():
    """The 64 jobs of the RANSAC test and their replay by route A, built once."""
    cap = backend.ncrelpose_limits()["stage_cap"]
    rng = np.random.default_rng(2024)
    sizes = [0, 16, 17, 18, 63, 64, 65, 255, 256, 257, cap - 1, cap, cap + 1]
    sizes += [int(v) for v in rng.integers(120, 201, 64 - len(sizes))]
    jobs, refs, seeds = [], [], []
    for b, n in enumerate(sizes):
        seed = 1000 + 17 * b
        j, r = nu.margin_job(nu.split(n), float(rng.uniform(0.10, 0.25)), float(rng.uniform(1e-4, 3e-4)), 50 + b, seed, **OPTS)
        jobs.append(j); refs.append(r); seeds.append(seed)
    return jobs, refs, seeds


@pytest.fixture(scope="module")
def device(ctx):
    jobs, refs, seeds = _reference()
    bt = nu.batch(jobs, seeds)
    bt["fill"] = FILL
    return ctx.ncrelpose_batch(bt, **OPTS), bt


def test_ransac_equals_the_replay(device):
    jobs, refs, _ = _reference()
    out, bt = device
    hist = {}
    for b, (j, r) in enumerate(zip(jobs, refs)):
        lo, hi = bt["ptr"][b], bt["ptr"][b + 1]
        got = (int(out["status"][b]), int(out["iterations"][b]), int(out["best_draw"][b]), int(out["inliers"][b]))
        assert got == (r["status"], r["iterations"], r["best_draw"], r["inliers"]), (b, hi - lo, got)
        assert np.array_equal(out["inlier"][lo:hi], r["mask"]), b
        hist[r["status"]] = hist.get(r["status"], 0) + 1
        if r["ransac"] is None:
            assert np.all(out["T_c1c2_ransac"][b] == FILL)
    print("statuses of the 64 jobs:", hist)
    assert hist.get(0, 0) >= 16 and hist.get(1, 0) == 2


def _found(refs, most=16):
    return [b for b, r in enumerate(refs) if r["status"] == 0][:most]


@functools.lru_cache(maxsize=None)
def _route_b():
    """Route B's polish and covariance from route A's model and inliers on the first 16 found jobs, and the spreads"""
    jobs, refs, seeds = _reference()
    out = {}
    s_R = s_t = s_cov = 0.0
    for b in _found(refs):
        j, r = jobs[b], refs[b]
        ry = nr.job_rays(j)
        Rb, tb = nr.polish_b(r["ransac"][0], r["ransac"][1], nr.take(ry, np.flatnonzero(r["mask"])))
        cb = nr.covariance(ry, r["mask"], j["cell_ptr"], seeds[b], Rb, tb, j["T_sc_q"], j["T_sc_c"], nr.threshold(nr.DEFAULTS["rp_error_cov"]),
                           solver=nr.solve_b_one)
        dr, dt = nr.pose_error(Rb, tb, *r["polished"])
        s_R, s_t = max(s_R, dr), max(s_t, dt)
        assert cb["rows"] == r["rows"] and cb["draws"] == r["draws"]
        s_cov = max(s_cov, float(np.abs(cb["cov"] - r["cov"]).max() / np.abs(r["cov"]).max()))
        out[b] = (Rb, tb, cb)
    return out, s_R, s_t, s_cov


def test_polish_reaches_the_minimiser(device):
    jobs, refs, _ = _reference()
    out, bt = device
    _, s_R, s_t, _ = _route_b()
    worst_R = worst_t = 0.0
    for b in _found(refs):
        j, r = jobs[b], refs[b]
        ryi = nr.take(nr.job_rays(j), np.flatnonzero(r["mask"]))
        dr, dt = _err(out["T_c1c2"][b], *r["polished"])
        worst_R, worst_t = max(worst_R, dr), max(worst_t, dt)
        Tr, Tp = out["T_c1c2_ransac"][b], out["T_c1c2"][b]
        assert nr.cost(nr.quat_rot(Tp[:4]), Tp[4:], ryi) <= nr.cost(nr.quat_rot(Tr[:4]), Tr[4:], ryi)
        Rs, ts = nr.sensor_pose(j["T_sc_q"], j["T_sc_c"], nr.quat_rot(Tp[:4]), Tp[4:])
        assert max(_err(out["T_s1s2"][b], Rs, ts)) < 1e-12
    print(f"polish, device against route A: R {worst_R:.3e} (A-B {s_R:.3e})  t {worst_t:.3e} (A-B {s_t:.3e})")
    assert worst_R <= 10 * s_R and worst_t <= 10 * s_t


def test_covariance_equals_the_replay(device):
    jobs, refs, _ = _reference()
    out, bt = device
    _, _, _, s_cov = _route_b()
    worst = 0.0
    for b, r in enumerate(refs):
        assert (int(out["cov_rows"][b]), int(out["cov_draws"][b])) == (r["rows"], r["draws"]), b
        if r["status"] in (0, 6):
            Cd = out["cov"][b]
            assert np.array_equal(Cd, Cd.T) and np.linalg.eigvalsh(Cd).min() >= -1e-12 * np.abs(Cd).max()
        else:
            assert np.all(out["cov"][b] == FILL)
    for b in _found(refs):
        worst = max(worst, float(np.abs(out["cov"][b] - refs[b]["cov"]).max() / np.abs(refs[b]["cov"]).max()))
    print(f"covariance, device against route A, relative to the largest entry: {worst:.3e} (A-B {s_cov:.3e})")
    assert worst <= 10 * s_cov


def test_each_status_and_what_it_leaves(ctx):
    """Statuses 3, 4, 5 and 6 by hand-built jobs; the outputs of the earlier stages are written, the later ones untouched."""
    cases = [(nu.split(150), 0.40, dict(min_inliers=100, max_iterations=300), 3),
             ([7, 40, 40, 40, 40, 40], 0.10, dict(OPTS), 4),
             (nu.split(240), 0.15, dict(OPTS, cov_iters=20, cov_max_iters=18), 5),
             (nu.split(240), 0.15, dict(OPTS, cov_thres=1e-12), 6)]
    for k, (sizes, wrong, opts, want) in enumerate(cases):
        j, r = nu.margin_job(sizes, wrong, 2e-4, 900 + k, 77 + k, **opts)
        assert r["status"] == want, (k, r["status"])
        bt = nu.batch([j], [77 + k]); bt["fill"] = FILL
        out = ctx.ncrelpose_batch(bt, **opts)
        assert (int(out["status"][0]), int(out["iterations"][0]), int(out["best_draw"][0]), int(out["inliers"][0]), int(out["cov_rows"][0]),
                int(out["cov_draws"][0])) == (want, r["iterations"], r["best_draw"], r["inliers"], r["rows"], r["draws"])
        assert np.array_equal(out["inlier"], r["mask"])
        assert max(_err(out["T_c1c2_ransac"][0], *r["ransac"])) < 1e-9
        if want == 3:
            assert np.all(out["T_c1c2"][0] == FILL) and np.all(out["T_s1s2"][0] == FILL) and np.all(out["cov"][0] == FILL)
        else:
            assert np.all(out["T_c1c2"][0] != FILL) and np.all(out["T_s1s2"][0] != FILL)
            assert np.all(out["cov"][0] == FILL) if want in (4, 5) else np.all(np.isfinite(out["cov"][0])) and np.trace(out["cov"][0]) >= 1e-12
        if want == 5:
            assert out["cov_draws"][0] == 19 and out["cov_rows"][0] < 20


def _same(a, b, ia, ib, sa, sb):
    for k in ("T_c1c2", "T_c1c2_ransac", "T_s1s2", "cov", "inliers", "status", "iterations", "best_draw", "cov_rows", "cov_draws"):
        assert np.array_equal(a[k][ia], b[k][ib]), k
    assert np.array_equal(a["inlier"][sa], b["inlier"][sb])


def test_a_job_does_not_depend_on_its_batch(ctx, device):
    jobs, refs, seeds = _reference()
    out, bt = device
    b = _found(refs)[0]
    order = [(b + 1 + k) % 64 for k in range(40)] + [b] + [(b + 41 + k) % 64 for k in range(24)]          # 65 jobs, the job in the middle
    big = ctx.ncrelpose_batch(dict(nu.batch([jobs[i] for i in order], [seeds[i] for i in order]), fill=FILL), **OPTS)
    alone = ctx.ncrelpose_batch(dict(nu.batch([jobs[b]], [seeds[b]]), fill=FILL), **OPTS)
    n = len(jobs[b]["f1"])
    lo = sum(len(jobs[i]["f1"]) for i in order[:40])
    _same(alone, big, 0, 40, slice(0, n), slice(lo, lo + n))
    _same(alone, out, 0, b, slice(0, n), slice(bt["ptr"][b], bt["ptr"][b + 1]))
    forced = ctx.ncrelpose_batch(dict(nu.batch([jobs[b]], [seeds[b]]), fill=FILL), stage_cap=16, **OPTS)   # n > 16: the global-memory path
    _same(alone, forced, 0, 0, slice(0, n), slice(0, n))
    assert alone["status"][0] == 0
