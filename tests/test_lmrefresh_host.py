"""Landmark refresh, host side: the C structs against the header, the argument checks of covgpu_landmark_refresh
(covgpu_landmark_refresh_check runs them without a context), the numpy restatement tests/lmrefresh_ref.py against a serial C++
restatement of the reference's literal arithmetic (tests/cpp/facade_refresh_shim.cpp: a double distance matrix, std::sort per row, the
0.5 * (n - 1) index, the `<` scan) bit for bit, and mapio.load_observation_features against load_map. No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from covins_amd import backend, capi, mapio, optimization, synth
from tests import lmrefresh_ref as lr
from tests import lmrefresh_util as lu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_struct_sizes_and_limits_match_the_header(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "covgpu.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %d %d %d %d %d\\n", '
                   "sizeof(covgpu_landmark_refresh_t), sizeof(covgpu_landmark_refresh_opts), offsetof(covgpu_landmark_refresh_t, lm_desc_obs), "
                   "offsetof(covgpu_landmark_refresh_t, kernel_ms), offsetof(covgpu_landmark_refresh_opts, num_octaves), "
                   "COVGPU_LMR_GROUP_MAX, COVGPU_LMR_WAVE, COVGPU_LMR_LONG_THREADS, COVGPU_LMR_STAGE, COVGPU_LMR_FORMS); return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[:5] == [C.sizeof(capi.LandmarkRefresh), C.sizeof(capi.LandmarkRefreshOpts), capi.LandmarkRefresh.lm_desc_obs.offset,
                       capi.LandmarkRefresh.kernel_ms.offset, capi.LandmarkRefreshOpts.num_octaves.offset]
    assert tuple(got[5:9]) == lu.limits() and got[9] == capi.LMR_FORMS == len(lr.FORM_LANES) + 1
    assert lr.FORM_LANES[-1] == lu.limits()[0]


def test_defaults_and_null_context():
    o = capi.LandmarkRefreshOpts()
    backend.lib().covgpu_default_landmark_refresh_opts(C.byref(o))
    assert (o.scale_factor, o.num_octaves) == (2.0, 1) == (lr.DEFAULT_OPTS["scale_factor"], lr.DEFAULT_OPTS["num_octaves"])
    assert backend.lib().covgpu_landmark_refresh(None, C.byref(capi.LandmarkRefresh()), C.byref(o)) == 1
    assert backend.lib().covgpu_last_error() == b"covgpu_landmark_refresh: NULL context"


def _check(inp, drop=(), **opts):
    """covgpu_landmark_refresh_check of the inputs; `drop`: struct fields passed as NULL."""
    s, o, out, keep = backend.Context._refresh_batch(inp["lm_obs_ptr"], inp["obs_kf"], inp["obs_desc"], inp["obs_octave"], inp["lm_ref_obs"],
                                                     inp["lm_pos"], inp["kf_center"], inp["kf_invalid"], inp["lm_invalid"], opts)
    for f in drop:
        setattr(s, f, None)
    rc = backend.lib().covgpu_landmark_refresh_check(C.byref(s), C.byref(o))
    return rc, backend.lib().covgpu_last_error().decode()


def test_invalid_arguments_are_rejected_before_any_device_work():
    good = lu.hand_case()[0]
    assert _check(good)[0] == 0
    assert _check(lu.Builder(0).inputs())[0] == 0                                  # K = 0, L = 0
    assert _check(lu.octave_case(), num_octaves=8, scale_factor=1.2)[0] == 0
    # every optional array may be NULL
    assert _check(good, drop=("obs_desc", "kf_invalid", "lm_invalid", "lm_desc_obs", "lm_desc", "lm_normal", "lm_min_distance",
                              "lm_max_distance", "lm_status", "form_count"))[0] == 0

    def bad(msg, inp=good, **kw):
        rc, err = _check(inp, **kw)
        assert rc == 1 and err.startswith("covgpu_landmark_refresh_check: ") and msg in err, (msg, rc, err)

    for f in ("lm_obs_ptr", "obs_kf", "obs_octave", "lm_ref_obs", "lm_pos", "kf_center"):
        bad("NULL", drop=(f,))
    assert backend.lib().covgpu_landmark_refresh_check(None, None) == 1
    ptr = good["lm_obs_ptr"].copy(); ptr[2], ptr[3] = ptr[3], ptr[2] - 1
    bad("not monotone", dict(good, lm_obs_ptr=ptr))
    ptr = good["lm_obs_ptr"].copy(); ptr[0] = 1
    bad("lm_obs_ptr[0]", dict(good, lm_obs_ptr=ptr))
    for v in (-1, good["K"]):
        obs = good["obs_kf"].copy(); obs[5] = v
        bad("obs_kf out of range", dict(good, obs_kf=obs))
    n4 = lu.hand_case()[1]["n4"]
    for v in (-2, 4):                                                              # the list of n4 has positions 0..3
        ref = good["lm_ref_obs"].copy(); ref[n4] = v
        bad("lm_ref_obs outside", dict(good, lm_ref_obs=ref))
    ref = good["lm_ref_obs"].copy(); ref[lu.hand_case()[1]["no_observations"]] = 0  # an empty list has no position 0
    bad("lm_ref_obs outside", dict(good, lm_ref_obs=ref))
    at = good["lm_obs_ptr"][n4] + good["lm_ref_obs"][n4]
    for v in (-1, 64):
        octv = good["obs_octave"].copy(); octv[at] = v
        bad("octave", dict(good, obs_octave=octv))
    octv = good["obs_octave"].copy(); octv[good["lm_obs_ptr"][n4] + (good["lm_ref_obs"][n4] + 1) % 4] = 99   # not the reference observation
    assert _check(dict(good, obs_octave=octv))[0] == 0
    for v in (0, 65, -3):
        bad("num_octaves", num_octaves=v)
    assert _check(good, num_octaves=64)[0] == 0
    for v in (np.nan, np.inf, 0.0, -1.2):
        bad("scale_factor", scale_factor=v)
    for v in (np.nan, np.inf):
        a = good["lm_pos"].copy(); a[3, 1] = v
        bad("non-finite lm_pos", dict(good, lm_pos=a))
        a = good["kf_center"].copy(); a[2, 0] = v
        bad("non-finite kf_center", dict(good, kf_center=a))


def test_hand_cases_do_what_they_are_for():
    inp, at = lu.hand_case()
    r = lu.exact("hand")
    ptr = inp["lm_obs_ptr"]
    rows = lambda name: inp["obs_desc"][ptr[at[name]]:ptr[at[name] + 1]]
    get = lambda k, name: r[k][at[name]]
    assert get("lm_desc_obs", "n0") == -1 and get("lm_status", "n0") == 1 and not get("lm_desc", "n0").any() and not get("lm_normal", "n0").any()
    assert get("lm_max_distance", "n0") > 0                                         # the reference keyframe is listed, if invalid
    assert get("lm_desc_obs", "n1") == 0 and get("lm_status", "n1") == 0
    assert lr.choose_descriptor(rows("n2"))[1].tolist() == [0, 0] and get("lm_desc_obs", "n2") == 0
    assert lr.hamming_matrix(rows("n2"))[0, 1] == 40
    med = lr.choose_descriptor(rows("n3"))[1]
    assert med[0] == 10 == med[1] and get("lm_desc_obs", "n3") == 0
    assert lr.choose_descriptor(rows("identical"))[1].tolist() == [0] * 6 and get("lm_desc_obs", "identical") == 0
    assert get("lm_desc_obs", "invalid_between") == 3                               # a list position: the candidates are 1, 3, 4
    assert np.array_equal(get("lm_desc", "invalid_between"), rows("invalid_between")[3])
    d = lr.hamming_matrix(rows("complementary"))
    assert d[0].tolist() == [0, 256, 256] and lr.choose_descriptor(rows("complementary"))[1].tolist() == [256, 0, 0]
    assert get("lm_desc_obs", "complementary") == 1
    assert get("lm_desc_obs", "listed_twice") == 0 and get("lm_status", "listed_twice") == 0
    assert get("lm_status", "invalid_lm") == 4 and get("lm_desc_obs", "invalid_lm") == -1 and get("lm_max_distance", "invalid_lm") == 0
    assert get("lm_status", "no_reference") == 2 and get("lm_max_distance", "no_reference") == 0 and get("lm_normal", "no_reference").any()
    assert get("lm_status", "reference_invalid") == 0
    c9 = inp["kf_center"][9]; p = inp["lm_pos"][at["reference_invalid"]]
    assert get("lm_max_distance", "reference_invalid") == np.sqrt(((p - c9) ** 2)[0] + ((p - c9) ** 2)[1] + ((p - c9) ** 2)[2])
    assert get("lm_status", "no_observations") == 3 and get("lm_desc_obs", "no_observations") == -1
    med = lr.choose_descriptor(rows("tie_1_2"))[1]
    assert med[1] == med[2] < min(med[0], med[3]) and get("lm_desc_obs", "tie_1_2") == 1
    # a wrapped byte distance would pick another row of `complementary`
    wrapped = np.sort(d % 256, axis=1)[:, 1]
    assert int(np.argmin(wrapped)) == 0


def _serial(inp, **opts):
    sm = lu.StandinRefreshMap(inp)
    try:
        return sm.serial(**opts)
    finally:
        sm.close()


def _same_as_serial(inp, ref, what, **opts):
    got = _serial(inp, **opts)
    got["form_count"] = ref["form_count"]                                           # (the serial loop has no forms)
    # the serial loop finds the reference keyframe's first observation; a case that points at a later copy is not its business
    lr.assert_same(got, ref, what)


def test_restatement_equals_the_literal_arithmetic_on_hand_cases():
    _same_as_serial(lu.hand_case()[0], lu.exact("hand"), "hand")
    inp = lu.octave_case()
    for opts in (dict(scale_factor=1.2, num_octaves=8), dict(scale_factor=2.0, num_octaves=1), dict(scale_factor=1.2, num_octaves=1)):
        _same_as_serial(inp, lr.refresh_exact(inp, **opts), opts, **opts)
    r = lr.refresh_exact(inp, scale_factor=1.2, num_octaves=8)
    dist = np.linalg.norm(inp["lm_pos"] - inp["kf_center"][3], axis=1)               # the reference observation is keyframe 3's
    assert np.allclose(r["lm_max_distance"], dist * 1.2 ** np.array([0, 7, 3, 7, 0]), rtol=1e-14)
    assert np.allclose(r["lm_min_distance"] * 1.2 ** 7, r["lm_max_distance"], rtol=1e-14)


def test_restatement_equals_the_literal_arithmetic_on_every_length():
    for inv in (False, True):
        _same_as_serial(lu.lengths_case(inv), lu.exact("lengths", inv), ("lengths", inv))
    r = lu.exact("lengths", False)
    assert r["form_count"].tolist() == np.bincount(np.searchsorted(lr.FORM_LANES, lu.edge_lengths()), minlength=6).tolist()
    assert r["form_count"][5] >= 8 and (r["form_count"][:5] >= 3).all()


def test_restatement_equals_the_literal_arithmetic_on_mixed_lengths():
    _same_as_serial(lu.mixed_case(), lu.exact("mixed"), "mixed")


@pytest.mark.parametrize("name", ["tiny", "small"])
def test_restatement_equals_the_literal_arithmetic_on_the_maps(name):
    inp, ref = lu.map_case(name), lu.exact("map", name)
    _same_as_serial(inp, ref, name)
    # noisy copies of one pattern: the tie rule decides for a good part of the landmarks
    tied = 0
    ptr = inp["lm_obs_ptr"]
    for l in range(0, inp["L"], 7):
        cand = np.flatnonzero(~inp["kf_invalid"][inp["obs_kf"][ptr[l]:ptr[l + 1]]])
        if len(cand) > 1 and not inp["lm_invalid"][l]:
            med = lr.choose_descriptor(inp["obs_desc"][ptr[l] + cand])[1]
            tied += (med == med.min()).sum() > 1
    assert tied >= 5


def test_reference_observations_and_centres_of_a_map():
    m = synth.make_map(synth.config_named("tiny"))
    ref = optimization.reference_observations(m)
    for l in range(m.L):
        lst = m.obs_kf[m.lm_obs_ptr[l]:m.lm_obs_ptr[l + 1]].tolist()
        assert ref[l] == (lst.index(m.lm_ref_kf[l]) if m.lm_ref_kf[l] in lst else -1)
    from tests.abspose_util import pose_matrix
    c = optimization.kf_centers(m)
    for k in range(0, m.K, 5):
        T = pose_matrix(m.kf_pose[k]) @ pose_matrix(m.cam_extr[int(m.kf_cam[k])])
        assert np.allclose(c[k], T[:3, 3], rtol=0, atol=1e-12)


def test_load_observation_features_is_aligned_with_load_map(tmp_path):
    """A saved map with descriptors (mapio.save_map, the descriptor matrices filled in by the test's writer): load_observation_features
    returns, observation by observation of load_map's order, the row of the observing keypoint."""
    m = synth.make_map(synth.config_named("tiny"))
    desc = lu.map_descriptors(m, seed=9)
    path = str(tmp_path / "map")
    lu.save_map_with_descriptors(path, m, desc)
    # one landmark archive names a keyframe that is not in the map: the observation is skipped by both readers
    lm_files = sorted(os.listdir(os.path.join(path, "mappoints")))
    f = os.path.join(path, "mappoints", lm_files[0])
    lm = mapio.read_landmark(open(f, "rb").read())
    w = mapio.Writer()
    w.idpair(lm["id"]); w.colvec(lm["pos_w"])
    ent = lm["observations"] + [((4000, 0), 0)]
    w.u64(len(ent))
    for kid, feat in ent:
        w.idpair(kid); w.i32(feat)
    w.idpair(lm["id_reference"])
    open(f, "wb").write(w.bytes())
    m2 = mapio.load_map(path)
    obs_desc, obs_feat = mapio.load_observation_features(path)
    assert obs_desc.shape == (m2.O, 32) and obs_desc.dtype == np.uint8 and obs_feat.shape == (m2.O,) and m2.O > 0
    # the descriptor of (landmark, keyframe) in the map that was written
    row_of = {(int(a), int(b)): i for i, (a, b) in enumerate(zip(m.kf_id, m.kf_client))}
    kept = [l for l in range(m.L) if m.lm_obs_ptr[l + 1] - m.lm_obs_ptr[l] >= 2 and m.lm_ref_kf[l] >= 0]   # what SaveToFile writes
    assert m2.L == len(kept)
    want = {}
    for l2, l in enumerate(kept):
        for o in range(m.lm_obs_ptr[l], m.lm_obs_ptr[l + 1]):
            want[(l2, int(m.obs_kf[o]))] = desc[o]
    seen = 0
    for l2 in range(m2.L):
        for o in range(m2.lm_obs_ptr[l2], m2.lm_obs_ptr[l2 + 1]):
            k = row_of[(int(m2.kf_id[m2.obs_kf[o]]), int(m2.kf_client[m2.obs_kf[o]]))]
            assert np.array_equal(obs_desc[o], want[(l2, k)]), (l2, o)
            seen += 1
    assert seen == m2.O == sum(m.lm_obs_ptr[l + 1] - m.lm_obs_ptr[l] for l in kept)
    # the same keypoint load_map took the pixel from
    kfs = {}
    for fn in os.listdir(os.path.join(path, "keyframes")):
        k = mapio.read_keyframe(open(os.path.join(path, "keyframes", fn), "rb").read())
        kfs[k["id"]] = k
    for o in range(0, m2.O, 11):
        kf = kfs[(int(m2.kf_id[m2.obs_kf[o]]), int(m2.kf_client[m2.obs_kf[o]]))]
        assert np.array_equal(kf["keypoints_distorted"][obs_feat[o]], m2.obs_uv[o]) and np.array_equal(kf["descriptors"][obs_feat[o]], obs_desc[o])
