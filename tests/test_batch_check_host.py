"""Every argument check of the batch front end, run without a device (covins_amd/csrc/batch_check.hpp): tests/cpp/batch_check_main.cpp
builds the smallest valid arguments of every entry point, applies one mutation per check and prints entry, case and message. The
program is built with AddressSanitizer and UBSan, so a check that reads past an array, or before it has tested a pointer, fails here.
TABLE holds the expected lines; its messages were written from the entry points' source as it stood before the checks moved into
the shared header (batch.hip, voctrain.hip and upload.hip), case by case, and are what a caller of the library sees behind
"<function>: ". The four checks that the library exports are called through ctypes on the same cases and must give the same message.
Five returns have no case: see the header of batch_check_main.cpp."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from covins_amd import backend, capi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

TABLE = """\
relpose	valid	ok corr=3 unified=0 model_b=[0,0] xi_b=[0.000000,0.000000]
relpose	zero_pairs	ok corr=0 unified=0 model_b=[] xi_b=[]
relpose	empty_last_pair	ok corr=2 unified=0 model_b=[0,0] xi_b=[0.000000,0.000000]
relpose	corr_ptr_first_not_zero	ok corr=3 unified=0 model_b=[0,0] xi_b=[0.000000,0.000000]
relpose	unified_b	ok corr=3 unified=1 model_b=[0,1] xi_b=[0.000000,0.250000]
relpose	null_batch	NULL array
relpose	negative_pairs	NULL array
relpose	null_inliers	NULL array
relpose	corr_ptr_not_monotone	corr_ptr not monotone
relpose	unknown_model	unknown camera model
relpose	unknown_model_before_missing_xi	unknown camera model
relpose	unified_without_xi	unified camera without xi
relpose	xi_negative	xi of a unified camera is negative or not finite
relpose	xi_nan	xi of a unified camera is negative or not finite
relpose	null_outlier	NULL correspondence array
abspose	valid	ok corr=3 max_n=2 seeds=[5,6]
abspose	seeds_given	ok corr=3 max_n=2 seeds=[11,12]
abspose	zero_candidates	ok corr=0 max_n=0 seeds=[]
abspose	empty_last_candidate	ok corr=2 max_n=2 seeds=[5,6]
abspose	null_options	NULL batch or options
abspose	negative_num	num < 0
abspose	max_iterations_zero	max_iterations <= 0
abspose	max_iterations_too_large	max_iterations > 100000 (a candidate makes up to 11 max_iterations draws in one launch)
abspose	probability_one	probability outside (0, 1)
abspose	threshold_nan	threshold not finite or not positive
abspose	null_T_wc	NULL array
abspose	corr_ptr_first	corr_ptr[0] != 0
abspose	corr_ptr_not_monotone	corr_ptr not monotone
abspose	null_inlier	NULL correspondence array
abspose	bearing_inf	non-finite bearing or point
abspose	point_nan	non-finite bearing or point
p3p	valid	ok
p3p	zero	ok
p3p	negative_n	n < 0
p3p	null_chosen	NULL array
p3p	point_nan	non-finite bearing or point
match	valid	ok rows=5 total_a=3 max_a=3 max_b=2 off=[0]
match	knn2	ok rows=5 total_a=3 max_a=3 max_b=2 off=[0]
match	zero_sets	ok rows=0 total_a=0 max_a=0 max_b=0 off=[0]
match	zero_jobs	ok rows=5 total_a=0 max_a=0 max_b=0 off=[0]
match	empty_last_set	ok rows=3 total_a=3 max_a=3 max_b=0 off=[0]
match	null_batch	NULL batch or options
match	unknown_mode	unknown mode
match	dist_threshold_zero	dist_threshold not finite or not positive
match	ratio_inf	ratio not finite or not positive
match	negative_jobs	num_sets or num_jobs < 0
match	skip_in_knn2	skip must be NULL in KNN2
match	null_row_ptr	NULL row_ptr
match	row_ptr_first	row_ptr[0] != 0
match	row_ptr_not_monotone	row_ptr not monotone
match	set_too_long	a set holds more than COVGPU_MATCH_MAX_ROWS rows
match	null_desc	NULL desc
match	null_nmatches	NULL job array
match	set_index_out_of_range	set index out of range
match	too_many_output_rows	more than 2^31 - 1 output rows
match	null_match	NULL match
match_float	valid	ok rows=5 total_a=3 max_a=3 max_b=2 off=[0]
match_float	zero_sets	ok rows=0 total_a=0 max_a=0 max_b=0 off=[0]
match_float	zero_jobs	ok rows=5 total_a=0 max_a=0 max_b=0 off=[0]
match_float	empty_last_set	ok rows=3 total_a=3 max_a=3 max_b=0 off=[0]
match_float	null_options	NULL batch or options
match_float	dense_mode	mode must be COVGPU_MATCH_KNN2
match_float	dist_threshold_nan	dist_threshold not finite or not positive
match_float	ratio_zero	ratio not finite or not positive
match_float	dim_not_multiple_of_4	dim must be a positive multiple of 4 up to 256
match_float	dim_too_large	dim must be a positive multiple of 4 up to 256
match_float	negative_sets	num_sets or num_jobs < 0
match_float	null_row_ptr	NULL row_ptr
match_float	row_ptr_first	row_ptr[0] != 0
match_float	row_ptr_not_monotone	row_ptr not monotone
match_float	set_too_long	a set holds more than COVGPU_MATCH_MAX_ROWS rows
match_float	null_desc	NULL desc
match_float	null_set_b	NULL job array
match_float	set_index_out_of_range	set index out of range
match_float	too_many_output_rows	more than 2^31 - 1 output rows
match_float	null_match	NULL match
match_float	descriptor_nan	descriptor value not finite or above 1e18 in magnitude
match_float	descriptor_too_large	descriptor value not finite or above 1e18 in magnitude
search_se3	valid	ok rows=5 tot1=3 tot2=2 off1=[0] off2=[0] tiles=(0,0,0,3)(0,1,0,2)
search_se3	zero_sets	ok rows=0 tot1=0 tot2=0 off1=[0] off2=[0] tiles=
search_se3	zero_jobs	ok rows=5 tot1=0 tot2=0 off1=[0] off2=[0] tiles=
search_se3	empty_last_set	ok rows=3 tot1=3 tot2=0 off1=[0] off2=[0] tiles=(0,0,0,3)
search_se3	null_batch	NULL batch
search_se3	null_options	NULL options
search_se3	th_low_256	th_low outside [0, 255]
search_se3	radius_zero	radius not finite or not positive
search_se3	num_octaves_zero	num_octaves < 1
search_se3	scale_factor_one	scale_factor not finite or not above 1
search_se3	agreement_two	agreement is neither 0 nor 1
search_se3	negative_sets	num_sets < 0
search_se3	null_row_ptr	NULL row_ptr
search_se3	row_ptr_first	row_ptr[0] != 0
search_se3	row_ptr_not_monotone	row_ptr not monotone
search_se3	set_too_long	a set holds more than COVGPU_MATCH_MAX_ROWS rows
search_se3	null_bounds	NULL bounds
search_se3	null_level	NULL keypoint array
search_se3	negative_jobs	num_jobs < 0
search_se3	null_K	NULL K
search_se3	null_lm_free	NULL landmark array
search_se3	null_nfound	NULL job array
search_se3	set_index_out_of_range	set index out of range
search_se3	T12_nan	non-finite T12
search_se3	null_match	NULL match
search_projection	valid	ok rows=5 points=2 xi=[0.000000,0.000000] tiles=(0,0,0,2)
search_projection	unified	ok rows=5 points=2 xi=[0.000000,0.500000] tiles=(0,0,0,2)
search_projection	zero_sets	ok rows=0 points=0 xi=[] tiles=
search_projection	zero_jobs	ok rows=5 points=0 xi=[0.000000,0.000000] tiles=
search_projection	empty_point_list	ok rows=5 points=0 xi=[0.000000,0.000000] tiles=
search_projection	null_batch	NULL batch
search_projection	null_options	NULL options
search_projection	row_ptr_first	row_ptr[0] != 0
search_projection	row_ptr_not_monotone	row_ptr not monotone
search_projection	set_too_long	a set holds more than COVGPU_MATCH_MAX_ROWS rows
search_projection	negative_jobs	num_jobs < 0
search_projection	null_cam	NULL camera array
search_projection	unknown_distortion	unknown distortion type
search_projection	unknown_model	unknown camera model
search_projection	unified_without_xi	unified camera without xi
search_projection	xi_inf	xi of a unified camera is negative or not finite
search_projection	null_point_ptr	NULL job array
search_projection	point_ptr_first	point_ptr[0] != 0
search_projection	set_index_out_of_range	set index out of range
search_projection	set_index_before_point_ptr	set index out of range
search_projection	point_ptr_not_monotone	point_ptr not monotone
search_projection	T_cw_inf	non-finite T_cw
search_projection	null_remap_to	NULL point array
search_projection	existing_idx_out_of_range	existing_idx out of range
pgo_reanchor	valid	ok
pgo_reanchor	nothing	ok
pgo_reanchor	negative_K	NULL array
pgo_reanchor	null_lm_pos	NULL array
pgo_reanchor	ref_kf_out_of_range	ref_kf out of range
bow_vocab	valid	ok
bow_vocab	null	NULL vocabulary
bow_vocab	scoring	only L1_NORM scoring is supported
bow_vocab	weighting	unknown weighting
bow_vocab	root_only	the vocabulary has no node below the root
bow_vocab	num_words_zero	num_words is not in 1..COVGPU_BOW_MAX_WORDS
bow_vocab	k_zero	k < 1 or L < 0
bow_vocab	null_weight	NULL vocabulary array
bow_vocab	parent_of_root	parent[0] != -1
bow_vocab	parent_not_before	parent[n] is not in 0..n-1
bow_vocab	child_ptr_first	child_ptr[0] != 0
bow_vocab	child_ptr_not_monotone	child_ptr not monotone
bow_vocab	child_ptr_last	child_ptr[num_nodes] != num_nodes - 1
bow_vocab	child_out_of_range	child index out of range
bow_vocab	child_of_another_parent	child lists inconsistent with parent
bow_vocab	children_descending	children not in ascending (line) order
bow_vocab	leaf_without_word	leaves are not exactly the nodes with a word id
bow_vocab	word_id_out_of_range	word id out of range
bow_vocab	word_id_twice	word ids are not a permutation of 0..num_words-1
bow_vocab	weight_nan	non-finite weight
bow_vocab	word_id_missing	word ids are not a permutation of 0..num_words-1
bow_transform	valid	ok rows=5
bow_transform	zero_sets	ok rows=0
bow_transform	empty_last_set	ok rows=3
bow_transform	null_batch	NULL batch
bow_transform	null_vocabulary	NULL vocabulary
bow_transform	negative_capacity	num_sets or capacity < 0
bow_transform	null_bow_ptr	NULL row_ptr or bow_ptr
bow_transform	row_ptr_first	row_ptr[0] != 0
bow_transform	row_ptr_not_monotone	row_ptr not monotone
bow_transform	set_too_long	a set holds more than COVGPU_MATCH_MAX_ROWS rows
bow_transform	null_desc	NULL desc
bow_transform	null_value	NULL word or value
bow_score_pairs	valid	ok
bow_score_pairs	nothing	ok
bow_score_pairs	negative_rows	negative row count
bow_score_pairs	null_bow_ptr	NULL bow_ptr
bow_score_pairs	bow_ptr_first	bow_ptr[0] != 0
bow_score_pairs	bow_ptr_not_monotone	bow_ptr not monotone
bow_score_pairs	null_word	NULL word or value
bow_score_pairs	negative_word	negative word id
bow_score_pairs	words_not_ascending	word ids of a bow row not ascending and duplicate-free
bow_score_pairs	value_nan	non-finite bow value
bow_score_pairs	negative_pairs	num_pairs < 0
bow_score_pairs	null_score	NULL pair array
bow_score_pairs	pair_out_of_range	pair index out of range
detect_candidates	valid	ok num_nb=3 max_words=2 pos_of=[1,0,-1] pairs=[0][1][0,1] inv=[0,1,3][1,0,1]
detect_candidates	min_score_given	ok num_nb=3 max_words=2 pos_of=[1,0,-1] pairs=[][][0,0] inv=[0,1,3][1,0,1]
detect_candidates	invalid_neighbour	ok num_nb=3 max_words=2 pos_of=[1,0,-1] pairs=[][][0,0] inv=[0,1,3][1,0,1]
detect_candidates	zero_queries	ok num_nb=3 max_words=0 pos_of=[1,0,-1] pairs=[][][] inv=[][]
detect_candidates	empty_database	ok num_nb=3 max_words=2 pos_of=[-1,-1,-1] pairs=[0][1][0,1] inv=[0][]
detect_candidates	null_options	NULL batch or options
detect_candidates	min_score_factor_nan	non-finite min_score_factor
detect_candidates	negative_scratch	scratch_kib < 0
detect_candidates	negative_cap	negative count
detect_candidates	null_client	NULL keyframe array
detect_candidates	negative_id	negative keyframe id
detect_candidates	bow_ptr_not_monotone	bow_ptr not monotone
detect_candidates	nb_ptr_first	nb_ptr[0] != 0
detect_candidates	nb_ptr_not_monotone	nb_ptr not monotone
detect_candidates	null_nb	NULL nb
detect_candidates	neighbour_out_of_range	neighbour index out of range
detect_candidates	null_db_order	NULL db_order
detect_candidates	db_order_out_of_range	db_order index out of range
detect_candidates	db_order_repeats	db_order repeats a keyframe
detect_candidates	null_db_visible	NULL query array
detect_candidates	null_candidates	NULL candidates
detect_candidates	query_kf_out_of_range	query_kf out of range
detect_candidates	db_visible_too_large	db_visible is not in 0..num_db
detect_candidates	min_score_in_nan	min_score_in is NaN
detect_candidates	too_many_query_neighbours	more than 2^31 - 1 query neighbours
prune	valid	ok
prune	nothing	ok
prune	empty_last_landmark	ok
prune	null_problem	NULL problem or options
prune	th_red_nan	non-finite th_red or max_time_dist
prune	negative_capacity	negative count
prune	null_lm_obs_ptr	NULL lm_obs_ptr
prune	lm_obs_ptr_first	lm_obs_ptr[0] != 0
prune	lm_obs_ptr_not_monotone	lm_obs_ptr not monotone
prune	null_obs_kf	NULL obs_kf
prune	obs_kf_out_of_range	obs_kf out of range
prune	null_kf_time	NULL keyframe array
prune	null_round_action	NULL round array
prune	kf_time_inf	non-finite kf_time
prune	kf_succ_out_of_range	kf_pred or kf_succ out of range
prune	not_mutual	kf_pred and kf_succ are not mutual
landmark_refresh	valid	ok
landmark_refresh	nothing	ok
landmark_refresh	empty_last_landmark	ok
landmark_refresh	null_options	NULL problem or options
landmark_refresh	scale_factor_zero	scale_factor not finite or not positive
landmark_refresh	num_octaves_65	num_octaves outside [1, 64]
landmark_refresh	negative_kf	negative count
landmark_refresh	null_lm_obs_ptr	NULL lm_obs_ptr
landmark_refresh	lm_obs_ptr_first	lm_obs_ptr[0] != 0
landmark_refresh	lm_obs_ptr_not_monotone	lm_obs_ptr not monotone
landmark_refresh	null_obs_octave	NULL obs_kf or obs_octave
landmark_refresh	null_lm_pos	NULL lm_ref_obs or lm_pos
landmark_refresh	null_kf_center	NULL kf_center
landmark_refresh	obs_kf_out_of_range	obs_kf out of range
landmark_refresh	lm_ref_obs_outside	lm_ref_obs outside its landmark's list
landmark_refresh	reference_octave_64	octave of a reference observation outside [0, 64)
landmark_refresh	lm_pos_nan	non-finite lm_pos
landmark_refresh	kf_center_inf	non-finite kf_center
voc_train	valid	ok
voc_train	empty_last_set	ok
voc_train	null_problem	NULL problem or options
voc_train	k_one	k < 2
voc_train	k_33	k > COVGPU_VOCTRAIN_MAX_K
voc_train	L_zero	L < 1
voc_train	too_many_words	k^L > COVGPU_BOW_MAX_WORDS
voc_train	weighting	unknown weighting
voc_train	scoring	only L1_NORM scoring is supported
voc_train	max_iterations_zero	max_iterations < 1
voc_train	scratch_too_small	scratch_kib below one set's word bitmap, ceil(k^L / 8192)
voc_train	negative_node_capacity	num_sets or node_capacity < 0
voc_train	zero_sets	no descriptor rows
voc_train	null_row_ptr	NULL row_ptr
voc_train	row_ptr_first	row_ptr[0] != 0
voc_train	row_ptr_not_monotone	row_ptr not monotone
voc_train	long_set_allowed	ok
voc_train	empty_sets_only	no descriptor rows
voc_train	too_many_rows	more than 2^31 - 1 - COVGPU_VOCTRAIN_TILE rows
voc_train	null_desc	NULL desc
voc_train	null_num_words	NULL num_nodes or num_words
voc_train	null_weight	NULL output array
upload_cam	valid	ok
upload_cam	all_pinhole	ok
upload_cam	unknown_model	unknown camera model
upload_cam	unified_without_cam_xi	unified camera without cam_xi
upload_cam	xi_negative	xi of a unified camera is negative or not finite
"""


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("batch_check") / "batch_check_main")
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(HERE, "cpp", "batch_check_main.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    return r.stdout.splitlines()


def test_every_check_gives_its_message_under_sanitizers(lines):
    want = TABLE.splitlines()
    for g, w in zip(lines, want):
        assert g == w
    assert len(lines) == len(want)


def test_the_table_covers_every_entry_point_and_its_edges():
    rows = [l.split("\t") for l in TABLE.splitlines()]
    assert all(len(r) == 3 for r in rows) and len({(r[0], r[1]) for r in rows}) == len(rows)
    entries = {r[0] for r in rows}
    assert entries == {"relpose", "abspose", "p3p", "match", "match_float", "search_se3", "search_projection", "pgo_reanchor", "bow_vocab",
                       "bow_transform", "bow_score_pairs", "detect_candidates", "prune", "landmark_refresh", "voc_train", "upload_cam"}
    for e in entries:
        kinds = [r[2].startswith("ok") for r in rows if r[0] == e]
        assert kinds[0] and not all(kinds), e                      # the valid arguments first, then at least one violation
    ok = {(r[0], r[1]) for r in rows if r[2].startswith("ok")}
    for e in ("match", "match_float", "search_se3", "search_projection"):
        assert {(e, "zero_sets"), (e, "zero_jobs")} <= ok
    for e in ("match", "match_float", "search_se3", "bow_transform", "voc_train"):
        assert (e, "empty_last_set") in ok
    messages = {r[2] for r in rows if not r[2].startswith("ok")}
    for name in ("row_ptr", "corr_ptr", "point_ptr", "nb_ptr", "lm_obs_ptr", "bow_ptr"):
        assert {name + "[0] != 0", name + " not monotone"} <= messages


# ---- the four exported checks on the same cases ----

class _Args:
    """A struct of the C ABI over numpy arrays. A mutation changes `arr` (in place), `val` (scalar fields), `opt` (option fields), or
    adds a field to `null`; no_batch / no_opts pass NULL for the whole struct."""

    def __init__(self, cls, opts_cls, arr, val, opt):
        self.cls, self.opts_cls, self.arr, self.val, self.opt, self.null = cls, opts_cls, arr, val, opt, set()
        self.no_batch = self.no_opts = False

    def structs(self):
        s, o = self.cls(), self.opts_cls()
        for name, typ in self.cls._fields_:
            if name in self.val:
                setattr(s, name, self.val[name])
            elif name in self.arr and name not in self.null:
                setattr(s, name, self.arr[name].ctypes.data_as(typ))
        for k, v in self.opt.items():
            setattr(o, k, v)
        return (None if self.no_batch else C.byref(s)), (None if self.no_opts else C.byref(o)), (s, o)


def _i(*v):
    return np.array(v, np.int32)


def _match_float():
    return _Args(capi.MatchFloatBatch, capi.MatchOpts,
                 dict(row_ptr=_i(0, 3, 5), desc=np.ones(20, np.float32), set_a=_i(0), set_b=_i(1), match=_i(0, 0, 0), dist=np.zeros(3, np.float32),
                      nmatches=_i(0)),
                 dict(num_sets=2, dim=4, num_jobs=1), dict(mode=capi.MATCH_KNN2, dist_threshold=500.0, ratio=0.8))


def _prune():
    return _Args(capi.PruneBatch, capi.PruneOpts,
                 dict(lm_obs_ptr=_i(0, 2, 3), obs_kf=_i(0, 1, 2), kf_pred=_i(-1, 0, 1), kf_succ=_i(1, 2, -1), kf_time=np.array([0.0, 1.0, 2.0]),
                      round_kf=_i(0, 0, 0), round_action=_i(0, 0, 0)),
                 dict(num_kf=3, num_lm=2, capacity=3), dict(th_red=0.95, max_time_dist=1.0, max_kfs=-1, max_rounds=0))


def _refresh():
    return _Args(capi.LandmarkRefresh, capi.LandmarkRefreshOpts,
                 dict(lm_obs_ptr=_i(0, 2, 3), obs_kf=_i(0, 1, 2), obs_octave=_i(0, 1, 0), lm_ref_obs=_i(1, -1), lm_pos=np.ones(6), kf_center=np.zeros(9)),
                 dict(num_kf=3, num_lm=2), dict(scale_factor=2.0, num_octaves=1))


def _voc_train():
    return _Args(capi.VocTrain, capi.VocTrainOpts,
                 dict(row_ptr=_i(0, 3, 5), desc=np.ones(160, np.uint8), num_nodes=_i(0), num_words=_i(0), parent=_i(0, 0, 0, 0),
                      desc_out=np.zeros(128, np.uint8), word_id=_i(0, 0, 0, 0), weight=np.zeros(4)),
                 dict(num_sets=2, node_capacity=4),
                 dict(k=10, L=5, weighting=capi.BOW_TF_IDF, scoring=0, seed=0, max_iterations=100, scratch_kib=65536))


def _set(name, i, v):
    return lambda x: x.arr[name].__setitem__(i, v)


def _null(name):
    return lambda x: x.null.add(name)


def _val(**kw):
    return lambda x: x.val.update(kw)


def _opt(**kw):
    return lambda x: x.opt.update(kw)


def _many_rows(x):
    x.arr["row_ptr"][:] = (0, 4096, 4096)
    x.arr["desc"] = np.ones(4096 * 4, np.float32)
    x.arr["set_a"] = x.arr["set_b"] = np.zeros(524288, np.int32)
    x.val["num_jobs"] = 524288


def _long_set(x):
    x.arr["row_ptr"][:] = (0, 4097, 4099)
    x.arr["desc"] = np.ones(32 * 4099, np.uint8)


def _nothing(x):
    x.val.update(num_kf=0, num_lm=0)
    x.arr["lm_obs_ptr"] = _i(0)
    x.null.update(k for k in ("kf_pred", "kf_center", "lm_pos") if k in x.arr)


NAN, INF = float("nan"), float("inf")
_ROW_PTR = dict(row_ptr_first=_set("row_ptr", 0, 1), row_ptr_not_monotone=_set("row_ptr", 1, 6))
_LM_PTR = dict(null_lm_obs_ptr=_null("lm_obs_ptr"), lm_obs_ptr_first=_set("lm_obs_ptr", 0, 1), lm_obs_ptr_not_monotone=_set("lm_obs_ptr", 1, 4),
               empty_last_landmark=_set("lm_obs_ptr", 2, 2), nothing=_nothing, valid=lambda x: None)
EXPORTS = {
    "match_float": ("covgpu_match_float_check", _match_float, dict(
        _ROW_PTR, valid=lambda x: None, zero_sets=lambda x: (x.val.update(num_sets=0, num_jobs=0), x.null.add("row_ptr")),
        zero_jobs=lambda x: (x.val.update(num_jobs=0), x.null.add("set_a")), empty_last_set=_set("row_ptr", 2, 3),
        null_options=lambda x: setattr(x, "no_opts", True), dense_mode=_opt(mode=capi.MATCH_DENSE), dist_threshold_nan=_opt(dist_threshold=NAN),
        ratio_zero=_opt(ratio=0.0), dim_not_multiple_of_4=_val(dim=6), dim_too_large=_val(dim=260), negative_sets=_val(num_sets=-1),
        null_row_ptr=_null("row_ptr"), set_too_long=lambda x: x.arr["row_ptr"].__setitem__(slice(None), (0, 4097, 4099)), null_desc=_null("desc"),
        null_set_b=_null("set_b"), set_index_out_of_range=_set("set_a", 0, -1), too_many_output_rows=_many_rows, null_match=_null("match"),
        descriptor_nan=_set("desc", 19, NAN), descriptor_too_large=_set("desc", 0, -1e19))),
    "prune": ("covgpu_prune_check", _prune, dict(
        _LM_PTR, null_problem=lambda x: setattr(x, "no_batch", True), th_red_nan=_opt(th_red=NAN), negative_capacity=_val(capacity=-1),
        null_obs_kf=_null("obs_kf"), obs_kf_out_of_range=_set("obs_kf", 2, 3), null_kf_time=_null("kf_time"), null_round_action=_null("round_action"),
        kf_time_inf=_set("kf_time", 1, INF), kf_succ_out_of_range=_set("kf_succ", 2, 3), not_mutual=_set("kf_succ", 0, 2))),
    "landmark_refresh": ("covgpu_landmark_refresh_check", _refresh, dict(
        _LM_PTR, null_options=lambda x: setattr(x, "no_opts", True), scale_factor_zero=_opt(scale_factor=0.0), num_octaves_65=_opt(num_octaves=65),
        negative_kf=_val(num_kf=-1), null_obs_octave=_null("obs_octave"), null_lm_pos=_null("lm_pos"), null_kf_center=_null("kf_center"),
        obs_kf_out_of_range=_set("obs_kf", 0, -1), lm_ref_obs_outside=_set("lm_ref_obs", 1, 1), reference_octave_64=_set("obs_octave", 1, 64),
        lm_pos_nan=_set("lm_pos", 5, NAN), kf_center_inf=_set("kf_center", 8, INF))),
    "voc_train": ("covgpu_voc_train_check", _voc_train, dict(
        _ROW_PTR, valid=lambda x: None, empty_last_set=_set("row_ptr", 2, 3), null_problem=lambda x: setattr(x, "no_batch", True), k_one=_opt(k=1),
        k_33=_opt(k=33), L_zero=_opt(L=0), too_many_words=_opt(k=32, L=5), weighting=_opt(weighting=-1), scoring=_opt(scoring=1),
        max_iterations_zero=_opt(max_iterations=0), scratch_too_small=_opt(scratch_kib=12), negative_node_capacity=_val(node_capacity=-1),
        zero_sets=_val(num_sets=0), null_row_ptr=_null("row_ptr"), long_set_allowed=_long_set,
        empty_sets_only=lambda x: x.arr["row_ptr"].__setitem__(slice(None), 0), too_many_rows=_set("row_ptr", 2, 2 ** 31 - 1 - 2047),
        null_desc=_null("desc"), null_num_words=_null("num_words"), null_weight=_null("weight"))),
}


@pytest.mark.parametrize("entry", sorted(EXPORTS))
def test_exported_checks_give_the_same_messages(entry):
    fn, make, cases = EXPORTS[entry]
    want = {r[1]: r[2] for r in (l.split("\t") for l in TABLE.splitlines()) if r[0] == entry}
    assert set(cases) == set(want)                                  # every case of the table, no other
    lib = backend.lib()
    for name, mutate in cases.items():
        x = make()
        mutate(x)
        b, o, keep = x.structs()
        rc = getattr(lib, fn)(b, o)
        got = lib.covgpu_last_error().decode() if rc else "ok"
        if want[name].startswith("ok"):
            assert rc == 0, (name, got)
        else:
            assert rc == 1 and got == f"{fn}: {want[name]}", (name, got)
