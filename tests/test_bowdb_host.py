"""Host side of the resident keyframe database: the restatement tests/bowdb_ref.py against the literal stateful form of
the reference with EraseKeyframe, and what the C entry points refuse before they touch a device. The argument checks that need a
handle, and with it a device, are in tests/test_gpu_bowdb.py."""
import ctypes as C

import numpy as np

from covins_amd import backend, capi
from tests import bow_util as bu
from tests import bowdb_ref as dr


def test_stateless_reading_equals_the_stateful_replay_with_erasures():
    """Each keyframe is queried once, as DetectLoop does: then the reference's scratch fields on the keyframes (loop_query_,
    loop_words_, loop_score_) never carry anything from one query into another, with EraseKeyframe in between too."""
    refs, live, erased = dr.replay()
    lit, live_lit = dr.replay_stateful()
    assert erased == 45 and live == live_lit and len(live) == len(refs) - 45
    assert len(refs) == len(lit) == len(bu.map_table())
    for q, (a, b) in enumerate(zip(refs, lit)):
        assert dr.same(a, b), q
    assert sum(len(r["candidates"]) > 0 for r in refs) >= 100
    _, plain = bu.map_queries()
    assert sum(not dr.same(a, b) for a, b in zip(refs, plain)) >= 40


def test_database_restatement_on_a_hand_case():
    """put / add / erase / re-add: the erased slot returns at the end of the insertion order."""
    db = dr.Database(dict(min_score_factor=0.8, min_loop_dist=100, exclude_kfs_with_id_less_than=7, inter_map_matches_only=0))
    q = bu.unit(range(10))
    db.put(0, 1000, 0, q)
    for s, words in ((1, range(2, 10)), (2, range(1, 9)), (3, range(0, 8))):
        db.put(s, 1000 + 200 * s, 0, bu.unit(words)); db.add(s)
    assert db.query(0, [], 0.05)["candidates"] == [3, 2, 1]
    db.erase(3); db.erase(3)
    assert db.query(0, [], 0.05)["candidates"] == [2, 1] and db.order == [1, 2]
    db.put(3, 1600, 0, bu.unit(range(1, 9))); db.add(3)
    assert db.order == [1, 2, 3] and db.query(0, [], 0.05)["candidates"] == [2, 3, 1]
    assert db.query(0, [2], 0.05)["candidates"] == [3, 1]                # a connected keyframe never joins


def _err(lib):
    return lib.covgpu_last_error().decode()


def test_null_arguments_are_refused_before_any_device_call():
    lib = backend.lib()
    h = C.c_void_p()
    assert lib.covgpu_bowdb_create(None, None, None, C.byref(h)) == 1 and "NULL context" in _err(lib) and not h
    one = np.zeros(1, np.int32)
    ip = capi.iptr(one)
    calls = dict(put=lambda: lib.covgpu_bowdb_put(None, 1, ip, ip, ip, ip, ip, None),
                 put_descriptors=lambda: lib.covgpu_bowdb_put_descriptors(None, ip, ip, ip, None),
                 set_neighbours=lambda: lib.covgpu_bowdb_set_neighbours(None, 1, ip, ip, ip),
                 set_invalid=lambda: lib.covgpu_bowdb_set_invalid(None, 1, ip, None),
                 add=lambda: lib.covgpu_bowdb_add(None, 1, ip), erase=lambda: lib.covgpu_bowdb_erase(None, 1, ip),
                 query=lambda: lib.covgpu_bowdb_query(None, None), compact=lambda: lib.covgpu_bowdb_compact(None),
                 order=lambda: lib.covgpu_bowdb_order(None, 0, None, None), stats=lambda: lib.covgpu_bowdb_stats(None, None))
    for name, call in calls.items():
        assert call() == 1, name
        assert _err(lib).startswith("covgpu_bowdb_" + name + ": NULL handle"), name
    lib.covgpu_bowdb_destroy(None)                                      # a no-op


def test_default_options_and_struct_layout():
    lib = backend.lib()
    assert C.sizeof(capi.BowDbOpts) == 48 and C.sizeof(capi.DetectOpts) == 24    # include/covgpu.h (LP64)
    assert C.sizeof(capi.BowDbQuery) == 13 * 8
    for mode, factor in ((capi.DETECT_COVINS, 0.8), (capi.DETECT_COVINS_G, 0.7)):
        o = capi.BowDbOpts()
        lib.covgpu_default_bowdb_opts(C.byref(o), mode)
        d = capi.DetectOpts()
        lib.covgpu_default_detect_opts(C.byref(d), mode)
        assert bytes(o.detect) == bytes(d) and o.detect.min_score_factor == factor
        assert (o.levelsup, o.tail_limit, o.reserve_kf, o.reserve_words, o.num_words) == (4, 256, 1024, 1 << 18, 0)
    assert len(capi.BOWDB_STATS) == 15


def test_facade_shim_compiles():
    """ResidentKeyframeDatabaseT instantiates on the stand-in map beside KeyframeDatabaseT (tests/cpp/facade_bowdb_shim.cpp)."""
    lib = dr.bowdb_shim()
    assert lib.bowdb_replay and lib.bowdb_detect and lib.bow_set_keyframe
