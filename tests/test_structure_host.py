"""Host half of tests/test_gpu_structure.py: every point of tests/structure_util.py HAS the structure it is named for, asserted from its arrays alone
(numpy / scipy.sparse incidence, as test_covisibility_recount does), so that the device test cannot quietly run another structure when a builder changes;
relabel() permutes and does not redraw, and the oracle is invariant under it to rounding; the planted outliers of the second-round patterns are separated
from everything else by the oracle's own outlier round; the pose graph has the incidence it is meant to have; and FlatProblem.validate refuses a landmark
observed twice by one keyframe (the library's validation: tests/test_gpu_structure.py).

Seen here. Spread of the oracle's two solvers at mu = 1e-4 over the 29 points: poses 3e-14 .. 1.6e-11, landmarks 2e-15 .. 8.1e-12; the smallest eigenvalue of
the Jacobi-scaled S: 1.0e-4 (relabel-vi, lanes) .. 8.9e-3. Relabelling: scaled S 1.6e-15 (ring), 5e-15 (tiny, visual-inertial). Planted outliers after the
5-iteration round of the oracle: planted norms >= 0.9997, every other norm <= 0.2 in every pattern."""
import numpy as np
import pytest

from covins_amd import capi
from tests import structure_util as su

EPS = np.finfo(np.float64).eps


def _tracks(p):
    return [p.obs_kf[p.lm_obs_ptr[l]:p.lm_obs_ptr[l + 1]] for l in range(p.L)]


@pytest.mark.parametrize("pt", su.POINTS, ids=su.IDS)
def test_point_has_the_structure_it_is_named_for(pt):
    b = su.build(pt)
    p = b.p
    W, nobs = su.incidence(p)
    n = np.diff(p.lm_obs_ptr)
    free = p.kf_fixed == 0
    Wl = np.tril(W, -1)
    ff = free[:, None] & free[None, :]
    cf = (free[:, None] ^ free[None, :])
    print(f"{pt.id}: K={p.K} ({int(free.sum())} free) L={p.L} O={p.O} free pairs {su.free_pairs(p, W)}, constant-free pairs {int(((Wl > 0) & cf).sum())}, "
          f"weights {Wl[Wl > 0].min() if (Wl > 0).any() else 0} .. {Wl.max()}")
    assert p.I == 0 or pt.kind.startswith("relabel-vi")
    assert np.unique(np.repeat(np.arange(p.L), n) * p.K + p.obs_kf).size == p.O           # no keyframe twice in a track
    if not pt.kind.startswith("relabel-vi"):
        assert (~free).sum() == (1 if pt.id == "bits-2" else 2)
        assert ((Wl > 0) & cf).any()                                                       # constant - free covisibility exists (and must create no pair)
    if pt.kind == "pairs":
        N, F = pt.arg, b.info["free"]
        assert free.sum() == F and F * (F - 1) // 2 >= N > (F - 1) * (F - 2) // 2 and (N != 4097 or F == 92)
        assert su.free_pairs(p, W) == N and set(Wl[(Wl > 0) & ff].tolist()) == {1}
        fk = np.nonzero(free)[0]
        want = [(fk[i], fk[j]) for i in range(F) for j in range(i)][:N]                     # the first N pairs of the (i, j < i) enumeration
        two = [t for t in _tracks(p) if len(t) == 2]
        assert len(two) == N and sorted((max(t), min(t)) for t in two) == sorted(want)
        assert all(free[t].all() for t in two) and all(len(t) == 3 and (~free[t]).sum() == 2 for t in _tracks(p) if len(t) != 2)
        if N > 1:
            assert any(t[0] > t[1] for t in two) and any(t[0] < t[1] for t in two)         # both orientations of pair_oa / pair_ob
        entries = int(Wl[ff].sum())                                                        # what k_pair_emit writes: one entry per pair and common landmark
        assert entries == N and 2 * N > entries                                            # -> build_pairs_device allocates its own scan buffer
    elif pt.kind == "lanes":
        for (a, c), m in zip(b.info["pair_kf"], su.LANES_SHARED):
            assert W[a, c] == m and free[a] and free[c]
        assert su.free_pairs(p, W) == len(su.LANES_SHARED)
        for m, k in b.info["nobs_kf"].items():
            assert nobs[k] == m and free[k]
        for m in su.LANES_NOBS:
            assert (nobs[free] == m).any(), m
        assert nobs[p.K - 1] == 0 and free[p.K - 1] and p.K - 1 in b.info["empty"]
    elif pt.kind == "bits":
        K = pt.arg
        assert p.K == K and free[K - 1] and nobs[K - 1] > 0 and n.min() >= 2 and n.max() <= 8
        assert K <= 8 or set(n.tolist()) == set(range(2, 9))
        assert any(np.any(np.diff(t) < 0) for t in _tracks(p))                             # observers not in ascending order
    elif pt.kind == "blocks":
        L, O = pt.arg
        zero, one = su.BLOCKS_SPECIAL[L]
        assert (p.L, p.O) == (L, O) and O % 256 in (255, 0, 1) and L in (255, 256, 257)
        assert sorted(np.nonzero(n == 0)[0].tolist()) == sorted(zero) and sorted(np.nonzero(n == 1)[0].tolist()) == sorted(one)
        assert all(not free[p.obs_kf[p.lm_obs_ptr[l]]] for l in one)                      # (why a constant keyframe: structure_util._blocks_tracks)
        assert n[0] < 2 and n[L - 1] < 2 and n[254] < 2 and (L < 256 or n[255] < 2) and (L < 257 or n[256] < 2)
    elif pt.kind == "relabel-ring":
        assert (p.K, p.L) == (40, 600)
    elif pt.kind == "lone":
        one = np.nonzero(n == 1)[0]
        assert one.tolist() == sorted(su.LONE_AT) and one[0] == 0 and one[-1] == p.L - 1 and n.min() == 1
        seen_by = p.obs_kf[p.lm_obs_ptr[one]]
        assert seen_by.tolist() == [su.LONE_AT[l] for l in one] and free[seen_by].sum() == 3 and (~free[seen_by]).sum() == 1 and p.K - 1 in seen_by
        assert su.schur_mus(pt) == (1e-2,)
    else:
        assert p.I > 0 and p.E > 0
        if pt.kind == "relabel-vi-reversed":                                               # the edge of relabel-vi the other way round, all else equal
            q, m = su.build(su.BY_ID["relabel-vi"]).p, b.maps
            assert m.flipped.any() and np.array_equal(p.edge_i[m.edge[m.flipped]], q.edge_j[m.edge[m.flipped]])
            assert np.array_equal(p.edge_j[m.edge[m.flipped]], q.edge_i[m.edge[m.flipped]]) and not np.array_equal(p.edge_meas, q.edge_meas)
            assert np.array_equal(p.obs_kf, q.obs_kf) and np.array_equal(p.imu_kf_i, q.imu_kf_i) and np.array_equal(p.kf_pose, q.kf_pose)
    assert su.schur_mus(pt) == su.MUS_SCHUR or pt.kind == "lone"


def test_the_block_points_cover_both_kinds_at_every_edge():
    at = {"first": set(), "last": set(), "254": set(), "255": set()}
    for L, (zero, one) in su.BLOCKS_SPECIAL.items():
        for kind, idx in (("zero", zero), ("one", one)):
            for l in idx:
                for name, where in (("first", 0), ("last", L - 1), ("254", 254), ("255", 255)):
                    if l == where:
                        at[name].add(kind)
    assert all(v == {"zero", "one"} for v in at.values()), at
    assert {O % 256 for O in su.BLOCKS_O} == {255, 0, 1}


def _multiset(a):
    a = np.asarray(a, np.float64).reshape(len(a), -1)
    return a[np.lexsort(a.T[::-1])]


@pytest.mark.parametrize("pt", su.RELABELLED, ids=[pt.id for pt in su.RELABELLED])
def test_relabel_permutes_the_arrays_and_the_oracle_does_not_notice(pt):
    from oracle import covo
    b = su.build(pt)
    p, q, m = b.orig, b.p, b.maps
    # every number of q is a number of p, found through the maps
    assert np.array_equal(q.kf_pose[m.kf], p.kf_pose) and np.array_equal(q.kf_fixed[m.kf], p.kf_fixed) and np.array_equal(q.kf_speed_bias[m.kf], p.kf_speed_bias)
    assert np.array_equal(q.lm_pos[m.lm], p.lm_pos)
    assert np.array_equal(q.obs_uv[m.obs], p.obs_uv) and np.array_equal(q.obs_kf[m.obs], m.kf[p.obs_kf])
    q_lm = np.repeat(np.arange(q.L), np.diff(q.lm_obs_ptr)); p_lm = np.repeat(np.arange(p.L), np.diff(p.lm_obs_ptr))
    assert np.array_equal(q_lm[m.obs], m.lm[p_lm])
    assert sorted(m.kf.tolist()) == list(range(p.K)) and sorted(m.lm.tolist()) == list(range(p.L)) and sorted(m.obs.tolist()) == list(range(p.O))
    assert not np.array_equal(m.kf, np.arange(p.K)) and not np.array_equal(m.lm, np.arange(p.L))
    # the original lists every track in ascending keyframe order; the relabelled one does not
    assert all(np.all(np.diff(t) > 0) for t in _tracks(p))
    desc = sum(bool(np.any(np.diff(t) < 0)) for t in _tracks(q))
    assert desc > q.L // 2, desc
    if p.I:
        assert np.all(p.imu_kf_i < p.imu_kf_j)
        down = int((q.imu_kf_j < q.imu_kf_i).sum())
        starts = np.setdiff1d(np.arange(q.K), q.imu_kf_j)                                   # keyframes without a predecessor
        print(f"{pt.id}: {down} of {q.I} IMU factors run down the index range; chains start at {starts.tolist()} (K = {q.K})")
        assert 3 * down > q.I and (starts > q.K / 2).any()
        assert np.array_equal(q.imu_kf_i[m.imu], m.kf[p.imu_kf_i]) and np.array_equal(q.imu_first[m.imu], p.imu_first)
        for f in (0, p.I // 2, p.I - 1):
            g = m.imu[f]
            assert np.array_equal(q.imu_samples[q.imu_sample_ptr[g]:q.imu_sample_ptr[g + 1]], p.imu_samples[p.imu_sample_ptr[f]:p.imu_sample_ptr[f + 1]])
        assert not m.flipped.any() and np.array_equal(q.edge_meas[m.edge], p.edge_meas) and np.array_equal(q.edge_i[m.edge], m.kf[p.edge_i])
    o = covo.default_options(**su.options_kw(pt))
    D = 6 if o.visual_only else 15
    r = su.rows_of(m.kf, D)
    for mu in su.MUS_SCHUR:
        S0, b0, c0 = covo.schur(p, o, mu)
        S1, b1, c1 = covo.schur(q, o, mu)
        sc = np.sqrt(np.abs(np.diag(S0)))
        eS = np.abs((S1[np.ix_(r, r)] - S0) / sc[:, None] / sc[None, :]).max()
        eb = np.abs((b1[r] - b0) / sc).max() / np.abs(b0 / sc).max()
        print(f"{pt.id} mu={mu:g}: oracle under relabelling: scaled S {eS:.2e}  b {eb:.2e}  cost {abs(c1 - c0) / c0:.2e}")
        assert eS < 1e-12 and eb < 1e-12 and abs(c1 - c0) < 1e-12 * c0


def test_relabel_reverses_edges_with_the_inverse_measurement():
    from scipy.spatial.transform import Rotation
    p = su.pose_graph("pose-graph")
    q, m = su.relabel(p, seed=9, flip_edges=True)
    assert abs(int(m.flipped.sum()) - p.E / 2) <= 1
    for e in range(p.E):
        g = m.edge[e]
        i, j = (p.edge_j[e], p.edge_i[e]) if m.flipped[e] else (p.edge_i[e], p.edge_j[e])
        assert (q.edge_i[g], q.edge_j[g]) == (m.kf[i], m.kf[j])
        assert np.array_equal(q.edge_sqrt_info[g], p.edge_sqrt_info[e]) and q.edge_loss_a[g] == p.edge_loss_a[e]
    f = np.nonzero(m.flipped)[0]
    Ra, Rb = Rotation.from_quat(p.edge_meas[f, :4]), Rotation.from_quat(q.edge_meas[m.edge[f], :4])
    assert (Ra * Rb).magnitude().max() < 1e-14                                               # T T^-1 = 1
    assert np.abs(Ra.apply(q.edge_meas[m.edge[f], 4:]) + p.edge_meas[f, 4:]).max() < 1e-14
    k = ~m.flipped
    assert np.array_equal(q.edge_meas[m.edge[k]], p.edge_meas[k])
    assert np.array_equal(su.pose_graph("pose-graph-reversed").edge_meas, q.edge_meas)


@pytest.mark.parametrize("pt", su.POINTS, ids=su.IDS)
def test_host_solvers_agree(pt):
    """The spread the device step is held to (tests/test_lm_forms_host.py): both solvers are backward stable on a system whose Jacobi-scaled form has
    eigenvalues in [mu, O(1)], so their forward errors differ by at most about N eps / mu."""
    ref = su.host_reference(pt)
    N, mu = ref["N"], su.MU_STEP
    print(f"{pt.id}: N={N} whole-system solver {ref['whole']}: h_pose={ref['h_pose']:.2e} h_lm={ref['h_lm']:.2e} (bound {N * EPS / mu:.1e})")
    assert ref["h_pose"] <= N * EPS / mu and ref["h_lm"] <= N * EPS / mu
    assert np.abs(ref["l0"]).max() > 0 and (np.abs(ref["x0"]).max() > 0)
    for S, b, c in ref["schur"].values():
        assert np.allclose(S, S.T) and c > 0


def test_oracle_rounding_with_a_free_lone_observer():
    """Why lone-free is not compared at mu = 1e-8 and why the blocks-* points give their single observations to a constant keyframe
    (structure_util._lone_tracks): the oracle's own S against a long-double evaluation of the same blocks, in the metric of the Schur comparison. With a
    free lone observer it is off by about eps / mu — more than the 1e-9 bound at mu = 1e-8, far inside it at 1e-2; with constant ones it is at rounding."""
    from oracle import covo
    o = covo.default_options(visual_only=1)
    seen = {}
    for pid in ("lone-free", "blocks-L255-O1023"):
        pt = su.BY_ID[pid]
        p, ref = su.build(pt).p, su.host_reference(pt)
        free = np.repeat(p.kf_fixed == 0, 6)
        for mu in su.MUS_SCHUR:
            S0 = ref["schur"][mu][0]
            sc = np.sqrt(np.abs(np.diag(S0)))
            e = np.abs((su.schur_long_double(p, o, mu) - S0) / sc[:, None] / sc[None, :])[np.ix_(free, free)]
            seen[pid, mu] = float(e.max())
            print(f"{pid} mu={mu:g}: oracle against long double: scaled S {seen[pid, mu]:.2e}  (eps / mu = {EPS / mu:.1e})")
    assert seen["lone-free", 1e-8] > 1e-9 and seen["lone-free", 1e-8] < 10 * EPS / 1e-8
    assert seen["lone-free", 1e-2] < 1e-12 and seen["blocks-L255-O1023", 1e-8] < 1e-12 and seen["blocks-L255-O1023", 1e-2] < 1e-12


def test_sparse_whole_system_step_is_the_dense_step():
    """structure_util.sparse_full_step (the whole-system solver above DENSE_MAX_N unknowns) against covo.step(dense=True) where both run."""
    from oracle import covo
    for pid in ("pairs-513", "blocks-L257-O1025", "lanes"):
        pt = su.BY_ID[pid]
        p, ref = su.build(pt).p, su.host_reference(pt)
        assert ref["whole"] == "dense"
        x, l = su.sparse_full_step(p, covo.default_options(visual_only=1), su.MU_STEP)
        e_pose, e_lm = su.scaled_err(x, ref["x0"], ref["d"]), su.rel(l, ref["l0"])
        print(f"{pid}: sparse against dense: poses {e_pose:.2e} landmarks {e_lm:.2e}")
        assert e_pose <= ref["N"] * EPS / su.MU_STEP and e_lm <= ref["N"] * EPS / su.MU_STEP
    assert su.host_reference(su.BY_ID["pairs-4097"])["whole"] == "sparse"


# ------------------------------------------------------------------------------------------------ planted erasures
@pytest.mark.parametrize("name", su.ERASE_PATTERNS)
def test_planted_outliers_are_separated_by_the_oracle(name):
    from oracle import covo
    p, rows, left = su.erase_problem(name)
    base = su.erase_base(name)
    n = np.diff(p.lm_obs_ptr)
    assert (p.K, p.L) == (su.ERASE_K, su.ERASE_L) and n.min() >= 2 and n.max() <= 8 and set(n.tolist()) == set(range(2, 9))
    planted = np.zeros(p.O, bool); planted[rows] = True
    shift = np.linalg.norm(p.obs_uv - base.obs_uv, axis=1)
    assert np.array_equal(p.obs_uv[~planted], base.obs_uv[~planted]) and (len(rows) == 0 or shift[planted].min() > su.ERASE_SHIFT - 1.0)
    assert np.array_equal(p.kf_fixed, base.kf_fixed) and p.kf_fixed.sum() == (2 if name != "all-but-one" else p.K - 2)
    sol, res = covo.gba_solve(p, covo.default_options(visual_only=1, max_iterations=5))
    norms = covo.residual_norms(sol, covo.default_options(visual_only=1))
    lo = norms[planted].min() if planted.any() else 1.0
    hi = norms[~planted].max()
    print(f"{name}: {planted.sum()} planted of {p.O}, displaced by {shift[planted].min() if planted.any() else 0:.0f} .. {shift.max():.0f} px, smallest planted norm {lo:.4f}, largest other norm {hi:.4f}; landmarks left with 0 / 1 / 2: "
          f"{(left == 0).sum()} / {(left == 1).sum()} / {((left == 2) & (n > 2)).sum()}")
    assert lo > 0.97 and hi < 0.46
    free_mid, last = 5, p.K - 1
    assert name == "all-but-one" or (not p.kf_fixed[free_mid] and not p.kf_fixed[last])
    if name == "none":
        assert len(rows) == 0
    elif name == "first-and-last":
        assert left[0] == 0 and left[-1] == 0 and (left[1:-1] == n[1:-1]).all()
    elif name == "left-with-1-and-2":
        assert (left == 1).sum() > 10 and ((left == 2) & (n > 2)).sum() > 10 and (left >= 1).all()
        assert (left[-3:] == 1).any() and ((left[-3:] == 2) & (n[-3:] > 2)).any()
    elif name == "middle-keyframe":
        assert planted[p.obs_kf == free_mid].all() and planted.sum() == (p.obs_kf == free_mid).sum() > 0
    elif name == "last-keyframe":
        assert planted[p.obs_kf == last].all() and planted.sum() == (p.obs_kf == last).sum() > 0
    else:
        assert (left >= 2).sum() == 1 and (left[left < 2] == 1).all()
    if name in ("middle-keyframe", "last-keyframe"):                                       # some landmark of that keyframe had two observations
        assert (left == 1).any()


def test_compaction_in_numpy():
    p, rows, left = su.erase_problem("left-with-1-and-2")
    erase = np.zeros(p.O, bool); erase[rows] = True
    q, keep = su.compact(p, erase)
    assert np.array_equal(keep, left >= 2) and q.L == keep.sum() and q.O == left[keep].sum() < p.O - len(rows)
    assert np.array_equal(np.diff(q.lm_obs_ptr), left[keep]) and np.array_equal(q.lm_pos, p.lm_pos[keep])
    obs_lm = np.repeat(np.arange(p.L), np.diff(p.lm_obs_ptr))
    kept_rows = np.nonzero(~erase & keep[obs_lm])[0]
    assert np.array_equal(q.obs_uv, p.obs_uv[kept_rows]) and np.array_equal(q.obs_kf, p.obs_kf[kept_rows])


# ------------------------------------------------------------------------------------------------ the pose graph
@pytest.mark.parametrize("name", su.PG_NAMES)
def test_pose_graph_has_its_incidence(name):
    p = su.pose_graph(name)
    base = su.pose_graph("pose-graph")
    assert p.K == su.PG_K and p.L == 0 and p.O == 0 and p.E == base.E and p.kf_fixed.sum() == 2
    deg = np.bincount(p.edge_i, minlength=p.K) + np.bincount(p.edge_j, minlength=p.K)
    assert deg.max() > 256 and (deg > 256).sum() == 1                                       # the hub's incidence list
    hub = int(np.argmax(deg))
    assert (p.edge_i == hub).sum() > 100 and (p.edge_j == hub).sum() > 100                  # on both sides of its edges
    key = np.minimum(p.edge_i, p.edge_j).astype(np.int64) * p.K + np.maximum(p.edge_i, p.edge_j)
    u, c = np.unique(key, return_counts=True)
    assert sorted(c.tolist())[-2:] == [2, 3] or sorted(c.tolist())[-1] == 3                 # the triple edge (and the hub's edge doubling a chain edge, if any)
    tri = np.nonzero(key == u[np.argmax(c)])[0]
    assert len(tri) == 3 and len({(p.edge_i[e], p.edge_j[e]) for e in tri}) == 2             # given in both orientations
    for e in tri:
        S = p.edge_sqrt_info[e].reshape(6, 6)
        assert np.abs(S - np.diag(np.diag(S))).max() > 1.0
    assert len({p.edge_sqrt_info[e].tobytes() for e in tri}) == 3
    fx = np.nonzero(p.kf_fixed)[0]
    assert ((np.isin(p.edge_i, fx)) & (np.isin(p.edge_j, fx))).sum() == 1                    # an edge between the two constant keyframes
    only_fixed = [k for k in range(p.K) if not p.kf_fixed[k] and deg[k] > 0
                  and all(p.kf_fixed[p.edge_j[e] if p.edge_i[e] == k else p.edge_i[e]] for e in np.nonzero((p.edge_i == k) | (p.edge_j == k))[0])]
    assert len(only_fixed) == 1 and deg[only_fixed[0]] == 2
    assert set(p.edge_loss_a.tolist()) == {0.0, 1.0} and 0.3 < p.edge_loss_a.mean() < 0.7
    assert np.any(np.diff(np.minimum(p.edge_i, p.edge_j)) < 0)                               # listed in no order
    assert not np.any(p.edge_i == p.edge_j)


# ------------------------------------------------------------------------------------------------ one observation per landmark and keyframe
def test_validate_refuses_a_landmark_observed_twice_by_one_keyframe():
    p = su.build(su.BY_ID["bits-5"]).p.copy()
    p.validate()
    o0 = p.lm_obs_ptr[3]
    p.obs_kf[o0 + 1] = p.obs_kf[o0]
    with pytest.raises(AssertionError, match="observed twice"):
        p.validate()
    with pytest.raises(AssertionError, match="observed twice"):
        p.copy()
    # the same keyframe in two DIFFERENT landmarks is what every problem has
    q = su.build(su.BY_ID["bits-5"]).p.copy()
    assert q.obs_kf[q.lm_obs_ptr[0]] in q.obs_kf[q.lm_obs_ptr[1]:]
    q.validate()
    # (a problem without observations stays valid)
    capi.FlatProblem(kf_pose=q.kf_pose, kf_speed_bias=q.kf_speed_bias, kf_fixed=q.kf_fixed, kf_cam=q.kf_cam, cam_extr=q.cam_extr, cam_intr=q.cam_intr,
                     cam_dist=q.cam_dist, cam_dist_type=q.cam_dist_type).validate()
