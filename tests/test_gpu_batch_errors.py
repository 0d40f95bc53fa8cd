"""Every stateless batch entry point rejects a malformed argument set under its own name, through a real context: the message is
"<function>: <message>" with the message of tests/test_batch_check_host.py's table for that case, which ties each entry point to its
check. After the rejections the context still works: one valid two-set covgpu_match_batch call returns the expected match."""
import os
import re

import numpy as np
import pytest

from covins_amd import backend, capi
from tests.test_batch_check_host import TABLE

pytestmark = pytest.mark.gpu

MESSAGE = {(r[0], r[1]): r[2] for r in (l.split("\t") for l in TABLE.splitlines())}


@pytest.fixture(scope="module")
def ctx():
    c = backend.Context(0)
    yield c
    c.close()


def _sets():
    """Sets of 3 and 2 ORB rows: a0 = b1 and a1 = b0, a2 is 128 bits from both."""
    desc = np.zeros((5, 32), np.uint8)
    desc[1] = 0xFF; desc[2] = 0x0F; desc[3] = 0xFF
    return dict(row_ptr=[0, 3, 5], desc=desc)


def _keypoint_sets():
    s = _sets()
    s.update(kp=np.ones((5, 2), np.float32), level=np.zeros(5, np.int32), bounds=np.tile([0.0, 100.0, 0.0, 100.0], (2, 1)))
    return s


def _relpose(c):
    bt = dict(ptr=[0, 4, 3], pA=np.ones((3, 3)), pB=np.ones((3, 3)), kpA=np.ones((3, 2)), kpB=np.ones((3, 2)), sigA=np.ones(3), sigB=np.ones(3),
              camA=np.ones((2, 8)), camB=np.ones((2, 8)), distA=[0, 0], distB=[0, 0], T0=np.tile([0, 0, 0, 1.0, 0, 0, 0], (2, 1)))
    c.relpose_batch(bt)


def _abspose(c):
    c.abspose_ransac_batch(dict(ptr=[0, 2, 3], bearing=np.full((3, 3), 0.5), point_w=np.full((3, 3), 2.0), sigma_angle=np.ones(3)), max_iterations=0)


def _p3p(c):
    P = np.full((1, 4, 3), 2.0); P[0, 3, 2] = np.nan
    c.p3p_batch(np.full((1, 4, 3), 0.5), P)


def _match(c):
    c.match_batch(_sets(), [0], [1], "dense", dist_threshold=0.0)


def _match_float(c):
    c.match_float_batch(dict(row_ptr=[0, 3, 5], desc=np.ones((5, 4), np.float32)), [0], [1], mode="dense")


def _search_se3(c):
    s = _keypoint_sets()
    s.update(K=np.ones((2, 4)), lm_pos=np.ones((5, 3)), lm_max_distance=np.ones(5), lm_desc=s["desc"], lm_free=np.ones(5, np.uint8))
    c.search_se3_batch(s, [0], [1], [[0, 0, 0, 1.0, 0, 0, 0]], th_low=256)


def _search_projection(c):
    s = _keypoint_sets()
    s.update(cam=np.ones((2, 8)), dist_type=[0, 2])
    jobs = dict(set=[0], T_cw=[[0, 0, 0, 1.0, 0, 0, 0]], point_ptr=[0, 2], p_w=np.ones((2, 3)), normal=np.ones((2, 3)), min_distance=[1.0, 1.0],
                max_distance=[2.0, 2.0], desc=np.ones((2, 32), np.uint8))
    c.search_projection_batch(s, jobs)


def _reanchor(c):
    c.pgo_reanchor(np.zeros((3, 7)), np.zeros((3, 7)), None, [3, -1], np.zeros((2, 3)))


_VOC = dict(num_words=2, k=2, L=1, scoring=capi.BOW_L1_NORM, weighting=capi.BOW_TF_IDF, parent=[-1, 0, 0], child_ptr=[0, 2, 2, 2], child=[1, 2],
            desc=np.ones((3, 32), np.uint8), word_id=[-1, 0, 1], weight=[0.0, 1.0, 1.0])
_BOW = dict(bow_ptr=[0, 2, 3, 3], word=[0, 1, 1], value=[0.5, 0.5, 1.0])


def _bow_transform(c):
    c.bow_transform_batch(dict(_VOC, scoring=1), _sets())


def _bow_score_pairs(c):
    c.bow_score_pairs(_BOW["bow_ptr"], [0, 0, 1], _BOW["value"], [0, 1], [1, 2])


def _detect(c):
    table = dict(_BOW, id=[7, 8, 9], client=[0, 0, 1], nb_ptr=[0, 1, 2, 3], nb=[1, 0, 0])
    c.detect_candidates_batch(table, [1, 1], [0], [2])


def _prune(c):
    c.prune_redundant([0, 2, 3], [0, 1, 2], [-1, 0, 1], [2, 2, -1], [0.0, 1.0, 2.0])


def _refresh(c):
    c.refresh_landmarks([0, 2, 3], [0, 1, 2], None, [0, 1, 0], [1, 1], np.ones((2, 3)), np.zeros((3, 3)))


def _voc_train(c):
    c.train_vocabulary([0, 3, 5], np.ones((5, 32), np.uint8), 1, 5)


REJECTIONS = [
    ("covgpu_relpose_batch", _relpose, ("relpose", "corr_ptr_not_monotone")),
    ("covgpu_abspose_ransac_batch", _abspose, ("abspose", "max_iterations_zero")),
    ("covgpu_p3p_batch", _p3p, ("p3p", "point_nan")),
    ("covgpu_match_batch", _match, ("match", "dist_threshold_zero")),
    ("covgpu_match_float_batch", _match_float, ("match_float", "dense_mode")),
    ("covgpu_search_se3_batch", _search_se3, ("search_se3", "th_low_256")),
    ("covgpu_search_projection_batch", _search_projection, ("search_projection", "unknown_distortion")),
    ("covgpu_pgo_reanchor", _reanchor, ("pgo_reanchor", "ref_kf_out_of_range")),
    ("covgpu_bow_transform_batch", _bow_transform, ("bow_vocab", "scoring")),
    ("covgpu_bow_score_pairs", _bow_score_pairs, ("bow_score_pairs", "words_not_ascending")),
    ("covgpu_detect_candidates_batch", _detect, ("detect_candidates", "db_order_repeats")),
    ("covgpu_prune_redundant", _prune, ("prune", "not_mutual")),
    ("covgpu_landmark_refresh", _refresh, ("landmark_refresh", "lm_ref_obs_outside")),
    ("covgpu_voc_train", _voc_train, ("voc_train", "k_one")),
]


def test_every_entry_point_rejects_under_its_own_name_and_the_context_survives(ctx):
    csrc = os.path.join(os.path.dirname(os.path.abspath(backend.__file__)), "csrc")
    src = open(os.path.join(csrc, "batch.hip")).read() + open(os.path.join(csrc, "voctrain.hip")).read()
    assert sorted(re.findall(r'batch_entry\("(\w+)"', src)) == sorted(r[0] for r in REJECTIONS)   # every entry point of the front end
    for fn, call, case in REJECTIONS:
        assert not MESSAGE[case].startswith("ok")
        with pytest.raises(backend.CovGpuError) as e:
            call(ctx)
        assert str(e.value) == f"covgpu error 1: {fn}: {MESSAGE[case]}", fn
    res = ctx.match_batch(_sets(), [0], [1], "dense")
    assert res["match"].tolist() == [1, 0, -1] and res["dist"].tolist() == [0, 0, -1] and res["nmatches"].tolist() == [2]
