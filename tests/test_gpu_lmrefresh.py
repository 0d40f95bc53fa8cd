"""covgpu_landmark_refresh on the GPU against tests/lmrefresh_ref.refresh_exact, bit for bit: the chosen observation,
its 32 bytes, the status, the landmarks per kernel form, and the doubles as their 64-bit patterns — f64 sqrt, /, * and + are correctly
rounded on gfx950 and the kernel contracts nothing, so there is no tolerance."""
import ctypes as C

import numpy as np
import pytest

from covins_amd import backend, capi, mapio, optimization, synth
from tests import guided_ref as gr
from tests import guided_util as gu
from tests import lmrefresh_ref as lr
from tests import lmrefresh_util as lu
from tests import prune_util as pu
from tests.abspose_util import pose_matrix

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = backend.Context(0)
    yield c
    c.close()


def run(ctx, inp, **opts):
    return ctx.refresh_landmarks(inp["lm_obs_ptr"], inp["obs_kf"], inp["obs_desc"], inp["obs_octave"], inp["lm_ref_obs"], inp["lm_pos"],
                                 inp["kf_center"], inp["kf_invalid"], inp["lm_invalid"], **opts)


def test_hand_built_landmarks(ctx):
    """n = 0 .. 5, identical descriptors, invalid keyframes between valid ones, a complementary pair, a keyframe listed twice, an
    invalid landmark, no reference, an invalid reference keyframe, an empty list, a tie (tests/lmrefresh_util.hand_case)."""
    inp, at = lu.hand_case()
    got = run(ctx, inp)
    lr.assert_same(got, lu.exact("hand"), "hand")
    assert got["lm_desc_obs"][at["complementary"]] == 1 and got["lm_desc_obs"][at["invalid_between"]] == 3


@pytest.mark.parametrize("kf_invalid", [False, True])
def test_every_length_at_which_the_kernel_takes_another_path(ctx, kf_invalid):
    """Lists of 0..5, every lane-group width g at g - 1, g, g + 1, the first long-form length, one on either side of the wave size, the
    workgroup size and the LDS staging capacity, and 1500 — read from the library, not guessed."""
    g, wave, wg, stage = lu.limits()
    assert {0, 1, 2, 3, 4, 5, g - 1, g, g + 1, wave + 1, wg - 1, wg, wg + 1, stage - 1, stage, stage + 1, 1500} <= set(lu.edge_lengths())
    inp = lu.lengths_case(kf_invalid)
    assert np.diff(inp["lm_obs_ptr"]).tolist() == lu.edge_lengths()
    got = run(ctx, inp)
    lr.assert_same(got, lu.exact("lengths", kf_invalid), ("lengths", kf_invalid))
    assert (got["form_count"] > 0).all()


def test_mixed_lengths_in_random_order(ctx):
    inp = lu.mixed_case()
    got = run(ctx, inp)
    lr.assert_same(got, lu.exact("mixed"), "mixed")
    assert (got["form_count"][:4] > 100).all() and got["form_count"].sum() == inp["L"]


def test_without_descriptors_only_the_geometry_is_computed(ctx):
    inp = lu.mixed_case()
    got = run(ctx, dict(inp, obs_desc=None))
    ref = dict(lu.exact("mixed"), lm_desc_obs=None, lm_desc=None)
    lr.assert_same(got, ref, "no descriptors")
    # through the C struct: the descriptor outputs are not touched
    s, o, out, keep = ctx._refresh_batch(inp["lm_obs_ptr"], inp["obs_kf"], None, inp["obs_octave"], inp["lm_ref_obs"], inp["lm_pos"],
                                         inp["kf_center"], inp["kf_invalid"], inp["lm_invalid"], {})
    out["lm_desc_obs"][:] = -7; out["lm_desc"][:] = 7
    assert backend.lib().covgpu_landmark_refresh(ctx._h, C.byref(s), C.byref(o)) == 0
    assert (out["lm_desc_obs"] == -7).all() and (out["lm_desc"] == 7).all()
    assert np.array_equal(out["lm_status"][:inp["L"]], ref["lm_status"])


@pytest.mark.parametrize("opts", [dict(scale_factor=2.0, num_octaves=1), dict(scale_factor=1.2, num_octaves=8),
                                  dict(scale_factor=1.2, num_octaves=1)])
def test_octaves_and_scale_factor(ctx, opts):
    """Reference observations on levels 0 and 7 under num_octaves 1 and 8."""
    inp = lu.octave_case()
    lr.assert_same(run(ctx, inp, **opts), lr.refresh_exact(inp, **opts), opts)


def test_no_landmarks(ctx):
    e = lu.Builder(0).inputs()
    got = run(ctx, e)
    assert got["lm_status"].shape == (0,) and got["lm_normal"].shape == (0, 3) and not got["form_count"].any()
    only_kf = lu.Builder(5).inputs()
    assert run(ctx, only_kf)["lm_desc"].shape == (0, 32)


def test_invalid_arguments_reach_no_kernel(ctx):
    inp = lu.hand_case()[0]
    obs = inp["obs_kf"].copy(); obs[0] = inp["K"]
    with pytest.raises(backend.CovGpuError, match="covgpu_landmark_refresh: obs_kf out of range"):
        run(ctx, dict(inp, obs_kf=obs))
    lr.assert_same(run(ctx, inp), lu.exact("hand"))                                 # the context still works


def test_kernel_time_is_reported_when_asked_for(ctx):
    got = run(ctx, lu.map_case("tiny"), kernel_ms=True)
    lr.assert_same(got, lu.exact("map", "tiny"))
    assert 0.0 < got["kernel_ms"] < 1000.0


@pytest.mark.parametrize("name", ["tiny", "small"])
def test_synthetic_maps(ctx, name):
    lr.assert_same(run(ctx, lu.map_case(name)), lu.exact("map", name), name)


def _guided_case(m, obs_desc, attr, num=24, seed=0):
    """SearchBySE3 jobs over the keyframes of `m`, every landmark attribute taken from `attr` (lm_desc, lm_maxd, lm_status): a keyframe's
    rows are its observations — the keypoint, its level and its descriptor row — and the landmark each row is associated with. A
    landmark is offered to the search when its status is 0 (the synthetic maps name reference keyframes that are no observers: those
    landmarks have no reference observation, status 2 and no distance range)."""
    obs_lm = np.repeat(np.arange(m.L), np.diff(m.lm_obs_ptr))
    Tcw = [np.linalg.inv(pose_matrix(m.kf_pose[k]) @ pose_matrix(m.cam_extr[int(m.kf_cam[k])])) for k in range(m.K)]
    kfs, lms_of = [], []
    for k in range(m.K):
        obs = np.flatnonzero(m.obs_kf == k)
        lm = obs_lm[obs]
        a = int(m.kf_cam[k])
        pc = (Tcw[k][:3, :3] @ m.lm_pos[lm].T).T + Tcw[k][:3, 3] if len(lm) else np.zeros((0, 3))
        kfs.append(dict(kp=m.obs_uv[obs].astype(np.float32).reshape(-1, 2), level=m.obs_octave[obs].astype(np.int32), desc=obs_desc[obs],
                        bounds=gu.BOUNDS, grid_inv=gu.GRID_INV if k % 2 == 0 else None, K=m.cam_intr[a].copy(), lm_pos=pc,
                        lm_max_distance=attr["lm_maxd"][lm], lm_desc=attr["lm_desc"][lm],
                        lm_free=(attr["lm_status"][lm] == 0).astype(np.uint8), T_cw=Tcw[k]))
        lms_of.append(set(lm.tolist()))
    rng = np.random.default_rng(seed)
    jobs = []
    while len(jobs) < num:
        q = int(rng.integers(m.K))
        near = [c for c in range(max(0, q - 6), min(m.K, q + 7)) if c != q and len(lms_of[q] & lms_of[c]) >= 10]
        if near:
            c = int(rng.choice(near))
            jobs.append((q, c, gu._perturb(kfs[q]["T_cw"] @ np.linalg.inv(kfs[c]["T_cw"]), rng)))
    return dict(kfs=kfs, jobs=jobs, opts=dict(lr.DEFAULT_OPTS, agreement=1))   # (the intended agreement test: the literal one keeps next to nothing)


def test_load_refresh_guided_matching(ctx, tmp_path):
    """The chain a loaded map runs: save `small` with descriptors, load_map + load_observation_features, refresh every landmark on the
    device, and feed covgpu_search_se3_batch jobs built from the refreshed attributes; against tests/guided_ref.py fed the
    restatement's attributes. Nothing here is drawn from a random generator but the descriptors' noise and the jobs."""
    m0 = synth.make_map(synth.config_named("small"))
    path = str(tmp_path / "map")
    lu.save_map_with_descriptors(path, m0, lu.map_descriptors(m0, seed=3))
    m = mapio.load_map(path)
    obs_desc, _ = mapio.load_observation_features(path)
    info = {}
    attr = optimization.refresh_landmarks(m, obs_desc, ctx, info=info)
    ref = lr.refresh_exact(lu.inputs_of_map(m, obs_desc))
    lr.assert_same(info, ref, "loaded map")
    assert np.isin(attr["lm_status"], (0, 2)).all() and (attr["lm_status"] == 0).sum() > m.L // 2
    assert (attr["lm_desc_obs"] >= 0).all() and info["form_count"][1:3].sum() > 0
    norms = np.linalg.norm(attr["lm_normal"], axis=1)                               # a mean of unit vectors
    assert (norms <= 1.0 + 1e-12).all() and norms.min() > 0.5 and (attr["lm_maxd"][attr["lm_status"] == 0] > 0).all()
    ref_attr = dict(lm_desc=ref["lm_desc"], lm_maxd=ref["lm_max_distance"], lm_status=ref["lm_status"])
    case, case_ref = _guided_case(m, obs_desc, attr), _guided_case(m, obs_desc, ref_attr)
    out = gu.run_se3(ctx, case)
    nf, frag, ev = gu.check_se3(out, gu.ref_se3(case_ref), 1)
    assert sum(nf) >= len(case["jobs"]) and ev > 0


def test_prune_remove_refresh(ctx):
    """Tracks shrink: prune `small` to half its keyframes, replay the erases (SlamMap.remove_keyframes drops the erased keyframes'
    observations), cut the descriptor rows the same way and refresh."""
    m = synth.make_map(synth.config_named("small"))
    desc = lu.map_descriptors(m, seed=5)
    before = np.diff(m.lm_obs_ptr).copy()
    r = pu.map_exact("small", False, "half")
    gone = np.zeros(m.K, bool); gone[r["round_kf"][r["round_action"] == 0]] = True
    keep = ~gone[m.obs_kf]
    m.remove_keyframes(r)
    desc = desc[keep]
    assert len(desc) == m.O and (np.diff(m.lm_obs_ptr) < before).sum() > m.L // 4
    info = {}
    optimization.refresh_landmarks(m, desc, ctx, info=info)
    lr.assert_same(info, lr.refresh_exact(lu.inputs_of_map(m, desc)), "pruned")
    assert (info["lm_status"][np.diff(m.lm_obs_ptr) < before] == 0).all()            # (a touched landmark's reference is its first observer)


def test_facade_equals_the_python_mirror(ctx):
    """LandmarkRefreshT::Refresh on stand-in objects built from `small`: the landmarks' members after the call are the mirror's outputs;
    a landmark without a valid observer would end the process as in the reference, so the facade's map has none."""
    inp = lu.map_case("small")
    ref = lu.exact("map", "small")
    ok = (ref["lm_status"] & 3) == 0                                                # (UpdateNormal exits on the others)
    inp = dict(inp, lm_invalid=inp["lm_invalid"] | ~ok)
    want = lr.refresh_exact(inp)
    lr.assert_same(run(ctx, inp), want, "mirror")
    sm = lu.StandinRefreshMap(inp)
    try:
        got = sm.facade()
    finally:
        sm.close()
        lu.refresh_shim().refresh_shutdown()
    live = want["lm_status"] == 0
    assert live.sum() > inp["L"] // 2
    assert np.array_equal(got["has_desc"], live) and np.array_equal(got["lm_desc"][live], want["lm_desc"][live])
    for k in ("lm_normal", "lm_min_distance", "lm_max_distance"):
        assert np.array_equal(got[k][live].view(np.uint64), np.ascontiguousarray(want[k][live]).view(np.uint64)), k
        assert not got[k][~live].any()                                              # skipped landmarks keep their members
    assert np.array_equal(got["form_count"], want["form_count"])
