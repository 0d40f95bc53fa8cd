"""Host half of tests/test_gpu_lm_forms.py: the points of tests/lm_forms_util.py, built on the pinhole and on the unified base,

  - select the width they are meant for (backend.lm_group, the rule of the upload) and hold the track lengths, landmark counts and degenerate
    landmarks the device test relies on, so that the device test cannot quietly run another form when the generator or the rule changes;
  - have host references that agree among themselves: the oracle's dense step against its Schur step (pinhole), the numpy dense Gauss-Newton step
    against the numpy Schur-then-back-substitute step from the same linearize_ref blocks (unified). Their spread h (pose part in the metric of the
    system, landmark part max-relative) is what the device step is held to.

Spread seen over the 26 points: mu = 1e-4: poses 2e-13 .. 1.3e-11, landmarks 1.7e-13 .. 8.1e-12; mu = 1e-8: poses up to 1.8e-7, landmarks up to 8.6e-8
(L = 1: no free keyframe observes the landmark, the pose step is zero on both sides). The bound is not fitted to these: both solvers are backward stable
on a system whose Jacobi-scaled form has eigenvalues in [mu, O(1)], so their forward errors differ by at most about N eps / mu for N unknowns.

The degenerate landmarks (constant observers only, one observation behind its keyframe, two observations) are solved by both host solvers like the
rest: their difference stays inside the spread of the other landmarks at every width and on both bases, so all three stay in the points."""
import numpy as np
import pytest

from covins_amd import backend
from tests import lm_forms_util as lu

EPS = np.finfo(np.float64).eps


@pytest.mark.parametrize("pt,cam", lu.ALL, ids=lu.IDS)
def test_point_selects_its_form_and_holds_the_required_tracks(pt, cam):
    b = lu.build(pt, cam)
    p, G = b.p, pt.G
    n = np.diff(p.lm_obs_ptr)
    print(f"{pt.id}-{cam}: K={p.K} L={p.L} O={p.O} O/L={p.O / p.L:.3f} -> {backend.lm_group(p.O, p.L)} lanes; tracks {sorted(set(n.tolist()))}; "
          f"chunks up to {-(-n.max() // G)}; workgroups {-(-p.L // (256 // G))}, the last with {(p.L - 1) % (256 // G) + 1} of {256 // G} groups; {b.special}")
    assert backend.lm_group(p.O, p.L) == G
    assert p.L == pt.L and np.array_equal(n, b.lengths) and n.min() >= 2
    assert (G == 4 and p.O / p.L <= 5) or (G == 8 and 5 < p.O / p.L <= 8) or (G == 16 and p.O / p.L > 8)
    assert p.kf_fixed.sum() == 2 * p.A and all(p.kf_fixed[np.nonzero(p.kf_cam == a)[0][:2]].all() for a in range(p.A))
    assert (p.cam_model is not None and list(p.cam_model) == [0, 1, 1]) == (cam == "unified")
    if p.L >= len(pt.pattern):
        for want in lu.required_lengths(G):
            assert (n == want).any(), want
        assert n.max() >= 2 * G + 1 and -(-n.max() // G) >= 3
    else:
        assert pt.L == 1 and G == 4
    for l in range(p.L):                      # tracks stay as the flattening hands them over: sorted by keyframe, no keyframe twice
        assert np.all(np.diff(p.obs_kf[p.lm_obs_ptr[l]:p.lm_obs_ptr[l + 1]]) > 0)


@pytest.mark.parametrize("G", [4, 8, 16])
def test_form_has_the_required_landmark_counts(G):
    counts = [pt.L for pt in lu.POINTS[G]]
    groups = 256 // G
    assert {groups - 1, groups, groups + 1} <= set(counts)
    assert sum(400 <= c <= 500 for c in counts) == 1 and lu.LARGE[G].L == max(counts)
    assert (1 in counts) == (G == 4)
    assert all(pt.G == G for pt in lu.POINTS[G])


@pytest.mark.parametrize("cam", lu.CAMERAS)
@pytest.mark.parametrize("G", [4, 8, 16])
def test_large_point_has_the_degenerate_landmarks(G, cam):
    from tests.test_omni_host import linearize_ref
    b = lu.build(lu.LARGE[G], cam)
    p, sp = b.p, b.special
    assert len({sp["const"], sp["behind"], sp["two"]}) == 3
    ptr = p.lm_obs_ptr
    assert p.kf_fixed[p.obs_kf[ptr[sp["const"]]:ptr[sp["const"] + 1]]].all()
    assert ptr[sp["two"] + 1] - ptr[sp["two"]] == 2 and not p.kf_fixed[p.obs_kf[ptr[sp["two"]]:ptr[sp["two"] + 1]]].all()
    s = sp["behind"]
    rows = np.arange(ptr[s], ptr[s + 1])
    assert len(rows) == G + 1 and sp["behind_obs"] in rows
    ok = np.array([lu.camera_frame_valid(p, p.obs_kf[o], p.lm_pos[s]) for o in rows])
    assert list(rows[~ok]) == [sp["behind_obs"]]
    assert (p.obs_kf == p.obs_kf[sp["behind_obs"]]).sum() == 1 and not p.kf_fixed[p.obs_kf[sp["behind_obs"]]]
    # ... and the linearisation sees them so: the oracle on the pinhole base, the restatement on the unified one
    if cam == "pinhole":
        from oracle import covo
        r, Jp, Jl, c = covo.linearize_reprojection(p, covo.default_options(visual_only=1))
    else:
        q = lu.cut_tracks(p, [sp["const"], sp["behind"], sp["two"]], np.diff(ptr)[[sp["const"], sp["behind"], sp["two"]]])
        r, Jp, Jl, c = linearize_ref(q, loss_a=1.0)
        ptr = q.lm_obs_ptr
        rows = np.arange(ptr[1], ptr[2]); sp = dict(const=0, behind=1, two=2, behind_obs=int(ptr[1] + (sp["behind_obs"] - p.lm_obs_ptr[s])))
    bo = sp["behind_obs"]
    assert not r[bo].any() and not Jp[bo].any() and not Jl[bo].any() and c[bo] == 0
    others = rows[rows != bo]
    assert np.abs(Jl[others]).sum(1).min() > 0 and np.abs(Jp[others]).sum(1).max() > 0
    cr = np.arange(ptr[sp["const"]], ptr[sp["const"] + 1])
    assert not Jp[cr].any() and np.abs(Jl[cr]).sum(1).min() > 0 and np.abs(r[cr]).sum() > 0


@pytest.mark.parametrize("pt,cam", lu.ALL, ids=lu.IDS)
def test_host_solvers_agree(pt, cam):
    p = lu.build(pt, cam).p
    ref = lu.host_reference(pt, cam)
    N = 6 * int((p.kf_fixed == 0).sum()) + 3 * p.L
    print(f"{pt.id}-{cam}: N={N} " + "  ".join(f"mu={mu:g}: h_pose={hp:.2e} h_lm={hl:.2e} (bound {N * EPS / mu:.1e})" for mu, (hp, hl) in ref["spread"].items()))
    for mu, (hp, hl) in ref["spread"].items():
        assert hp <= N * EPS / mu and hl <= N * EPS / mu, (mu, hp, hl)
    assert ref["h_pose"] == ref["spread"][lu.MU_STEP][0] and ref["h_lm"] == ref["spread"][lu.MU_STEP][1]
    # the Schur complements the device is compared with: symmetric, unit diagonal on the blocks without unknowns
    for mu, (S, b, c) in ref["schur"].items():
        assert np.allclose(S, S.T) and c > 0
        for k in np.nonzero(p.kf_fixed)[0]:
            assert np.array_equal(S[6 * k:6 * k + 6, 6 * k:6 * k + 6], np.eye(6)) and not b[6 * k:6 * k + 6].any()
    if p.L > 1:
        assert np.abs(ref["x0"]).max() > 0
    assert np.abs(ref["l0"]).max() > 0


@pytest.mark.parametrize("cam", lu.CAMERAS)
@pytest.mark.parametrize("G", [4, 8, 16])
def test_degenerate_landmarks_lie_inside_the_host_spread(G, cam):
    """Per landmark, |dense step - Schur step| relative to the largest landmark step: the three degenerate landmarks against the rest."""
    pt = lu.LARGE[G]
    b = lu.build(pt, cam)
    ref = lu.host_reference(pt, cam)
    for mu, ((xd, ld), (xs, ls)) in ref["steps"].items():
        e = np.abs(ls - ld).max(axis=1) / np.abs(ld).max()
        special = [b.special[k] for k in ("const", "behind", "two")]
        rest = np.delete(e, special).max()
        print(f"{pt.id}-{cam} mu={mu:g}: const {e[special[0]]:.2e} behind {e[special[1]]:.2e} two {e[special[2]]:.2e} | the rest up to {rest:.2e}")
        assert e[special].max() <= rest, (mu, e[special], rest)
        assert np.abs(ld[special]).max(axis=1).min() > 0      # every one of them has a step to compare
