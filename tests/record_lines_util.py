"""Points for the whole-record transport of the landmark Schur pass (k_visual.hip): k_pair_blocks gathers the 144-byte Z records of a trip
cooperatively (lane q of a pair's sixteen loads 16-byte segment 16 m + q of the trip's record list), k_lm_lin stores them through a per-wave LDS
tile (lane q of the wave stores segment 64 m + q). ONE table of points shared by the host test (tests/test_record_lines_host.py: every point has
the property it is named for), the device test (tests/test_gpu_record_lines.py) and tools/make_record_lines_golden.py, which records what the
commit BEFORE that transport computed on these points (tests/golden/record_lines_parent.npz). Built on tests/structure_util.ring_problem / relabel.
No GPU code here.

Points (the smallest shapes at which the cooperative forms can go wrong; none is at the workload's size):
  common-1..72      72 pairs of free keyframes that share exactly n = 1, 2, ..., 72 landmarks, each landmark pinned by a constant third observer
                    (as structure_util._lanes_tracks): every tail of a sixteen-term trip over up to five trips, and every n for which the 9 n
                    segments of one half of the record list, or the 18 n of both, are one below, at or one above a multiple of 16 and of 64.
                    146 keyframes, 2 628 landmarks, 7 884 observations.
  slot-ends         a pair of free keyframes (the lowest and the highest index) whose common landmarks own the FIRST and the LAST record of the
                    array: keyframe-major slot 0 and slot O - 1; the free keyframe with the highest index observes last. Two more pairs share only
                    those two landmarks. The gather and the store at both ends of obsZ.
  common-scattered  relabel() of common-1..72: tracks no longer sorted by keyframe, the row keyframe of a pair the lower or the higher index, the
                    common landmarks of a pair scattered over the landmark range.
  stores-G4/8/16    track lengths cycle through every value 2 .. 4 G + 1 (one to five chunks of G), mixed with two-observation tracks so that
                    covgpu_lm_group(O, L) returns that G; L is one above a multiple of 256 / G: the last workgroup holds one landmark and
                    otherwise empty groups, and a wave's store tile mixes full, partial and empty records.
"""
from collections import namedtuple

import numpy as np

from tests import structure_util as su
from tests.lm_forms_util import MU_STEP, MUS_SCHUR, rel, scaled_err

Point = namedtuple("Point", "id kind arg")
Built = namedtuple("Built", "p info orig maps")

COMMON_N = tuple(range(1, 73))
COMMON_FIXED = (0, 9)
SLOT_K, SLOT_FIXED, SLOT_MIDDLE = 5, (2, 3), 20
# per G: two-observation tracks mixed into one cycle of 2 .. 4 G + 1, landmarks (one above a multiple of 256 / G), keyframes (4 G + 1 observers + 3)
STORES = {4: dict(twos=26, L=129, K=20), 8: dict(twos=56, L=97, K=36), 16: dict(twos=0, L=81, K=68)}
STORES_FIXED = (1, 7)
SCATTER_SEED = 5

POINTS = ([Point("common-1..72", "common", None), Point("slot-ends", "slot-ends", None), Point("common-scattered", "scattered", None)]
          + [Point(f"stores-G{G}", "stores", G) for G in (4, 8, 16)])
IDS = [pt.id for pt in POINTS]
BY_ID = {pt.id: pt for pt in POINTS}
_built, _ref = {}, {}


def _common_tracks():
    fixed = COMMON_FIXED
    pair_kf, k = [], 0

    def take():
        nonlocal k
        while k in fixed:
            k += 1
        k += 1
        return k - 1
    for _ in COMMON_N:
        pair_kf.append((take(), take()))
    K = k
    tracks = []
    for m, ((a, b), n) in enumerate(zip(pair_kf, COMMON_N)):        # a constant observer pins the shared landmarks and adds no pair
        for s in range(n):
            tracks.append([(b, fixed[0], a), (a, b, fixed[1]), (fixed[1], b, a)][(m + s) % 3])
    return K, tracks, fixed, dict(pair_kf=pair_kf)


def _slot_ends_tracks():
    K, fixed = SLOT_K, SLOT_FIXED
    lo, mid, hi = 0, 1, K - 1                                        # free keyframes
    tracks = [(lo, mid, hi, fixed[0])]                               # landmark 0: its first observation is the first one of keyframe 0 -> slot 0
    for s in range(SLOT_MIDDLE):
        tracks.append([(hi, fixed[0], lo), (lo, hi, fixed[1]), (fixed[1], hi, lo)][s % 3])
    tracks.append((fixed[0], lo, mid, hi))                           # landmark L - 1: its last observation is the last one of keyframe K - 1 -> slot O - 1
    return K, tracks, fixed, dict(lo=lo, mid=mid, hi=hi)


def stores_lengths(G):
    """Track length of every landmark of stores-G: cycles of 2 .. 4 G + 1 with STORES[G]['twos'] two-observation tracks spread evenly between them."""
    base = list(range(2, 4 * G + 2))
    twos, cyc = STORES[G]["twos"], []
    for i, n in enumerate(base):
        cyc.append(n)
        cyc += [2] * (twos * (i + 1) // len(base) - twos * i // len(base))
    return np.resize(np.asarray(cyc, np.int64), STORES[G]["L"])


def _stores_tracks(G):
    rng = np.random.default_rng(9000 + G)
    K = STORES[G]["K"]
    return K, [rng.permutation(K)[:n].tolist() for n in stores_lengths(G)], STORES_FIXED


def slots_of(p):
    """Keyframe-major slot of every observation (DevProblem::obs_zpos): its rank in a stable sort of the observation stream by keyframe."""
    order = np.argsort(p.obs_kf, kind="stable")
    z = np.empty(p.O, np.int64); z[order] = np.arange(p.O)
    return z


def build(pt):
    """Built(problem, facts the tests rely on, the original problem and the Relabel maps of the relabelled point); cached, treat as read-only."""
    if pt.id in _built:
        return _built[pt.id]
    info, orig, maps = {}, None, None
    if pt.kind == "common":
        K, tracks, fixed, info = _common_tracks()
        p = su.ring_problem(K, tracks, fixed, seed=72)
    elif pt.kind == "slot-ends":
        K, tracks, fixed, info = _slot_ends_tracks()
        p = su.ring_problem(K, tracks, fixed, seed=73)
    elif pt.kind == "scattered":
        b = build(BY_ID["common-1..72"])
        orig, info = b.p, b.info
        p, maps = su.relabel(orig, seed=SCATTER_SEED)
    else:
        K, tracks, fixed = _stores_tracks(pt.arg)
        p = su.ring_problem(K, tracks, fixed, seed=90 + pt.arg)
        info = dict(G=pt.arg)
    p.validate()
    _built[pt.id] = Built(p, info, orig, maps)
    return _built[pt.id]


def host_reference(pt):
    """Per point, computed once and shared (read-only), as structure_util.host_reference: the oracle's Schur complements {mu: (S, b, cost)} at
    MUS_SCHUR and MU_STEP, the whole-system reference step (x0, l0) at MU_STEP with d = sqrt(diag S), and the spread of the oracle's two solvers of
    that step in the metrics the device is held to."""
    if pt.id in _ref:
        return _ref[pt.id]
    from oracle import covo
    p = build(pt).p
    o = covo.default_options(visual_only=1)
    schur = {mu: covo.schur(p, o, mu) for mu in MUS_SCHUR + (MU_STEP,)}
    N = 6 * p.K + 3 * p.L
    xs, ls = covo.step(p, o, MU_STEP, dense=False)
    xd, ld = covo.step(p, o, MU_STEP, dense=True) if N <= su.DENSE_MAX_N else su.sparse_full_step(p, o, MU_STEP)
    d = np.sqrt(np.abs(np.diag(schur[MU_STEP][0])))
    _ref[pt.id] = dict(schur=schur, x0=xd, l0=ld, d=d, h_pose=scaled_err(xs, xd, d), h_lm=rel(ls, ld), N=N, whole="dense" if N <= su.DENSE_MAX_N else "sparse")
    return _ref[pt.id]


# ------------------------------------------------------------------------------------------------ what the parent commit computed (tests/golden)
GOLDEN = "record_lines_parent.npz"
GOLDEN_FULL_S = {"common-1..72": MUS_SCHUR, "slot-ends": MUS_SCHUR, "common-scattered": MUS_SCHUR, "stores-G4": MUS_SCHUR[1:], "stores-G8": MUS_SCHUR[1:],
                 "stores-G16": ()}      # where the 6 x 6 blocks of S are kept besides its digest (the file stays under 1 MB)


def lower_blocks(S):
    """(index [m,2] of the non-zero 6 x 6 blocks of the lower triangle of S, diagonal included, row-major; the blocks [m,6,6])."""
    K = S.shape[0] // 6
    B = S.reshape(K, 6, K, 6).transpose(0, 2, 1, 3)
    i, j = np.nonzero(np.tril(np.abs(B).max(axis=(2, 3)) > 0))
    return np.stack([i, j], 1).astype(np.int32), np.ascontiguousarray(B[i, j])


def digest(a):
    import hashlib
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8).copy()


def device_record(ctx, pt):
    """{name: array} of what a device context computes on the point, in the form the golden file keeps: per mu of MUS_SCHUR the digest of S, b and the
    cost (and the lower blocks of S where GOLDEN_FULL_S says so), and the step at MU_STEP. Uses Context.schur / gn_step only."""
    from covins_amd import backend
    p = build(pt).p
    g = backend.default_options(visual_only=1)
    out = {}
    for mu in MUS_SCHUR:
        S, b, c = ctx.schur(p, g, mu)
        assert np.array_equal(S, S.T)
        k = f"{pt.id}/mu={mu:g}/"
        out[k + "S_sha256"], out[k + "b"], out[k + "cost"] = digest(S), b, np.array([c])
        if mu in GOLDEN_FULL_S[pt.id]:
            out[k + "S_index"], out[k + "S_blocks"] = lower_blocks(S)
    dx, dl, c = ctx.gn_step(p, g, MU_STEP)
    k = f"{pt.id}/step/"
    out[k + "dx"], out[k + "dl"], out[k + "cost"] = dx, dl, np.array([c])
    return out
