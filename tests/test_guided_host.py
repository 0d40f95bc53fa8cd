"""Host-side checks of the guided matching: the numpy restatement (tests/guided_ref.py) on hand-computed examples, one
per quirk of the reference; the cap on fragile points of every generated input the GPU tests compare on; the header's declarations and
the library's defaults; the visiting orders."""
import ctypes as C
import pathlib
import re

import numpy as np
import pytest

from tests import guided_ref as gr
from tests import guided_util as gu

ROOT = pathlib.Path(__file__).resolve().parents[1]


def _case(cases, name):
    return next(c for c in cases if c["name"] == name)


def _se3(case, job=0, **kw):
    a, b, T = case["jobs"][job]
    o = dict(case["opts"]); o.update(kw)
    return gr.search_se3(case["kfs"][a], case["kfs"][b], T, **o)


def test_hamming_is_the_popcount_of_the_xor():
    rng = np.random.default_rng(0)
    a, b = rng.integers(0, 256, (2, 32), dtype=np.uint8)
    want = sum(bin(int(x) ^ int(y)).count("1") for x, y in zip(a, b))
    assert gr.hamming(a, b) == want == gr.hamming_rows(a, b[None])[0]
    assert gr.hamming(a, a) == 0 and gr.hamming(a, ~a) == 256


def test_predict_scale_narrows_the_distance_to_float_and_clamps():
    # log2(8 / 1) = 3 exactly -> ceil 3; a distance a hair under 1 in double is 1.0f as a float, so it stays 3 and not 4
    assert gr.predict_scale(1.0, 8.0, 2.0, 8)[0] == 3
    assert gr.predict_scale(1.0 - 1e-12, 8.0, 2.0, 8)[0] == 3
    assert gr.predict_scale(1.0, 8.0 * 1.001, 2.0, 8)[0] == 4
    assert gr.predict_scale(1.0, 1e6, 2.0, 8)[0] == 7 and gr.predict_scale(1.0, 1e-6, 2.0, 8)[0] == 0      # the clamps
    assert gr.predict_scale(3.0, 100.0, 2.0, 1)[0] == 0                                                 # the reference's configuration
    assert gr.predict_scale(1.0, 8.0, 2.0, 8)[1] and not gr.predict_scale(1.0, 9.0, 2.0, 8)[1]            # on an integer: fragile


def test_area_test_is_float32_and_inclusive():
    kp = np.array([[3, 4], [6, 8], [5.7, 7.6], [0, 9.5]], np.float32)          # distances 5, 10, 9.5 (as floats), 9.5
    got, frag = gr.features_in_area(kp, np.arange(4), 0.0, 0.0, 9.5)
    assert got == [0, 2, 3] or got == [0, 3]                                   # row 2 is float rounding's to decide, and so fragile
    assert frag
    got, frag = gr.features_in_area(kp[:2], np.arange(2), 0.0, 0.0, 9.5)
    assert got == [0] and not frag
    assert gr.features_in_area(kp[:2], np.arange(2), 0.0, 0.0, 10.0)[0] == [0, 1]   # <= radius


def test_visiting_orders():
    kp = np.array([(103, 104), (97, 96), (94, 100), (700, 470), (-3, 5)], np.float32)
    assert gr.visiting_order(kp, None).tolist() == [0, 1, 2, 3, 4]
    # cells (10, 10), (10, 10), (9, 10), (70 -> 63, 47), (-0 -> 0, 1): a cell outside the grid is clamped
    assert gr.visiting_order(kp, (0.1, 0.1)).tolist() == [4, 2, 0, 1, 3]


@pytest.mark.parametrize("grid", [False, True])
def test_se3_quirks_by_hand(grid):
    cases = gu.adversarial_se3(grid)
    r = _se3(_case(cases, "ties"))                         # first visited wins: index order row 0, grid order row 2 (cell_x 9)
    assert r["match1"].tolist() == ([2, 3, -1, -1] if grid else [0, 3, -1, -1])
    r = _se3(_case(cases, "thresholds"))                   # 4. <= 50 one way, < 50 the other
    assert r["match1"].tolist() == [0, 1, -1] and r["match2"].tolist() == [0, -1, -1] and r["match"].tolist() == [0, -1, -1]
    c = _case(cases, "agreement")                          # 5. literal against intended agreement
    assert _se3(c)["match"].tolist() == [1, -1, -1] and _se3(c, agreement=1)["match"].tolist() == [-1, 2, -1]
    c = _case(cases, "n1>n2")                              # 5. rows i >= n2 never agree literally
    assert _se3(c)["match1"].tolist() == [0, -1, -1, 0, 2] and _se3(c)["nfound"] == 0
    assert _se3(c, agreement=1)["match"].tolist() == [-1, -1, -1, 0, 2]
    c = _case(cases, "depth+bounds")                       # 6. z < 0; bounds inclusive below, exclusive above; 3. keyframe 2's bounds
    r = _se3(c)
    assert r["match1"].tolist() == [-1, 1, 2, -1, -1, 5, 6, -1, -1, 9]
    assert r["match2"].tolist() == r["match1"].tolist()    # into keyframe 1 (320 x 240) with keyframe 2's 640 x 480 bounds
    assert _se3(c, 1)["match1"].tolist() == [-1, 1, -1, -1, -1, 5, -1, -1, -1, -1]      # roles swapped: the small bounds both ways
    r = _se3(_case(cases, "levels"))                       # window [predicted - 1, predicted] = [2, 3]; 2. radius 9.5 * 2^3 reaches 50 px
    assert r["match1"].tolist() == [-1, 1, 2, -1, -1]
    assert _se3(_case(cases, "levels"), num_octaves=1)["match1"].tolist() == [-1] * 5   # level 0: radius 9.5, window [-1, 0]
    for c in cases:                                        # exactly representable: nothing fragile
        for j in range(len(c["jobs"])):
            r = _se3(c, j)
            assert not r["fragile1"].any() and not r["fragile2"].any(), c["name"]


def test_se3_projection_is_k_p_over_z_and_z_zero_goes_on():
    x = np.zeros(32, np.uint8)
    mk = lambda p: gu._kf([(100, 100)], desc=x, lm_pos=[p], lm_desc=x, lm_free=[1])
    k2 = mk((0, 0, 1)); k2["K"] = np.array([50.0, 25.0, 60.0, 80.0])
    T = gu.IDENT
    assert gr.search_se3(mk((2.0, 2.0, 2.5), ), k2, T)["match1"].tolist() == [0]       # 50 * 0.8 + 60 = 100, 25 * 0.8 + 80 = 100
    assert gr.search_se3(mk((2.0, 2.0, -2.5)), k2, T)["match1"].tolist() == [-1]
    r = gr.search_se3(mk((2.0, 2.0, 0.0)), k2, T)                                      # u = v = inf: IsInImage refuses, nothing fragile
    assert r["match1"].tolist() == [-1] and not r["fragile1"].any() and r["evaluated"] >= 1


@pytest.mark.parametrize("grid", [False, True])
def test_projection_by_hand(grid):
    cases = gu.adversarial_projection(grid)
    run = lambda c: gr.search_projection(c["kfs"][c["jobs"][0][0]], c["jobs"][0][1], c["jobs"][0][2], **c["opts"])
    r = run(_case(cases, "cluster"))                       # 40 points, 12 keypoints: the first 12 claim them all
    assert sorted(r["claimed"][:12].tolist()) == list(range(12)) and np.all(r["claimed"][12:] == -1) and r["nmatches"] == 12
    r = run(_case(cases, "cluster+taken+skip"))
    assert not set(r["claimed"].tolist()) & {0, 5, 7} and np.all(r["claimed"][1::3] == -1) and r["nmatches"] == 9
    r = run(_case(cases, "existing"))                      # dist_old 9 < 10 keeps; 10 and 11 propose the remap; nothing is claimed
    assert r["remap_to"].tolist() == [-1, 2, 4, -1] and r["nmatches"] == 0 and r["best_dist"].tolist() == [10, 10, 10, -1]
    r = run(_case(cases, "ties+taken+thresholds"))         # the second point sees what the first left; taken best; 50 in, 51 out
    assert r["claimed"].tolist() == ([2, 0, 4, 5, -1] if grid else [0, 1, 4, 5, -1])
    r = run(_case(cases, "filters"))
    assert r["claimed"].tolist() == [-1, -1, 2, 3, -1, -1, 6, 7, -1, -1, -1, -1, 12]
    r = run(_case(cases, "levels"))                        # radius 10 * 1.2^3 = 17.28: 15 px in, 20 px out; levels 2 and 3 pass
    assert r["claimed"].tolist() == [-1, 1, 2, -1, -1]
    for c in cases:
        assert not run(c)["fragile"].any(), c["name"]


def test_grid_order_equals_index_order_without_ties():
    """The two branches of GetFeaturesInArea return the same set; with distinct distances inside every radius the winner is the same."""
    case = gu.map_se3_case("pyr")
    kfs = case["kfs"]
    for a, b, T in case["jobs"][:6]:
        ga = [dict(kfs[k], grid_inv=gu.GRID_INV) for k in (a, b)]
        ia = [dict(kfs[k], grid_inv=None) for k in (a, b)]
        rg = gr.search_se3(ga[0], ga[1], T, **case["opts"]); ri = gr.search_se3(ia[0], ia[1], T, **case["opts"])
        diff = np.flatnonzero(rg["match1"] != ri["match1"])
        for i in diff:                                     # a different winner only on an exact tie of the two winners' distances
            d = [gr.hamming(kfs[a]["lm_desc"][i], kfs[b]["desc"][r[i]]) for r in (rg["match1"], ri["match1"])]
            assert d[0] == d[1]
        assert len(diff) <= 0.02 * max(1, int((ri["match1"] >= 0).sum()))


@pytest.mark.parametrize("config", ["ref", "pyr"])
def test_fragile_points_are_rare(config):
    """At most 1 % of the points that pass the depth test, in every generated input the GPU tests compare on."""
    refs = gu.ref_se3(gu.map_se3_case(config))
    f = sum(int(r["fragile1"].sum() + r["fragile2"].sum()) for r in refs); ev = sum(r["evaluated"] for r in refs)
    print(f"SE3 {config}: {f} fragile of {ev} evaluated ({f / ev:.2e})")
    assert ev > 10000 and f <= 0.01 * ev
    refs = gu.ref_projection(gu.map_projection_case(config))
    f = sum(int(r["fragile"].sum()) for r in refs); ev = sum(r["evaluated"] for r in refs)
    print(f"PROJECTION {config}: {f} fragile of {ev} evaluated ({f / ev:.2e})")
    assert ev > 5000 and f <= 0.01 * ev
    for r in refs:                                         # and every job keeps a comparable prefix
        assert gr.projection_comparable(r).sum() > 0


def test_header_declares_the_entry_points_and_defaults():
    h = (ROOT / "include" / "covgpu.h").read_text()
    for name in ("covgpu_search_se3_batch", "covgpu_search_projection_batch", "covgpu_default_guided_opts"):
        assert re.search(r"\b" + name + r"\s*\(", h), name
    for field in ("th_low", "radius", "scale_factor", "num_octaves", "agreement"):
        assert re.search(r"\b" + field + r";", h), field
    assert "#define COVGPU_GUIDED_SE3 0" in h and "#define COVGPU_GUIDED_PROJECTION 1" in h


def test_library_defaults():
    from covins_amd import backend, capi
    for mode, radius in ((capi.GUIDED_SE3, 9.5), (capi.GUIDED_PROJECTION, 10.0)):
        o = capi.GuidedOpts()
        backend.lib().covgpu_default_guided_opts(C.byref(o), mode)
        assert (o.th_low, o.radius, o.scale_factor, o.num_octaves, o.agreement) == (50, radius, 2.0, 1, 0)


def test_facade_guided_shim_compiles():
    """LoopMatcherT::SearchBySE3Batch / SearchByProjection instantiate on the stand-in map (tests/test_gpu_guided.py drives them)."""
    lib = gu.guided_shim()
    assert lib.guided_se3 is not None and lib.guided_projection is not None
