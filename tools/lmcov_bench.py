#!/usr/bin/env python3
"""Times Context.landmark_covariances_resident on the 5-agent synthetic map, visual-inertial, mu = 0, through the Python
binding, against the only route there was before it: Context.keyframe_covariances_resident with every off-diagonal block pair of the
oracle's S, and the block formula Sigma_l = H_ll^-1 + H_ll^-1 (sum over a, b of W_a^T Sigma_ab W_b) H_ll^-1 combined in numpy on the host. All
figures come from one run, medians after one warm-up: one covgpu_gn_step; the old route with its call and its host part timed separately
(the host part starts from the Jacobians of the oracle's linearisation, which is not timed); the new call, without and with kf_cov. With them:
the call's statistics, the landmarks served, the gather's size sum n_l^2, and the largest difference between the two results relative to the
largest entry. Acceptance: the one call is faster than the old route in this run. Writes one JSON file (default profiles/lmcov_bench.json).
Needs an MI355X."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from covins_amd import backend, mapdata, synth  # noqa: E402


def _median_ms(fn, repeats):
    fn()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(t), t, out


def _system_pairs(prob):
    from oracle import covo
    ptr, col, blocks, b, cost = covo.schur_sparse(prob, covo.default_options(visual_only=0), 0.0)
    blocks = np.asarray(blocks)
    out = []
    for i in range(len(ptr) - 1):
        for e in range(ptr[i], ptr[i + 1]):
            j = int(col[e])
            if j != i and not prob.kf_fixed[i] and not prob.kf_fixed[j] and np.any(blocks[e] != 0):
                out.append((i, j))
    return sorted(set(out) | {(j, i) for i, j in out})


def host_combination(prob, Jp, Jl, kf_cov, pair_cov, pairs, chunk=2048):
    """The block formula on the host: every (a, b) of a landmark's free observers looks its 6x6 block up (a diagonal block, or the pair's
    in the order (keyframe of a, keyframe of b)), landmarks in chunks."""
    K, L, O = prob.K, prob.L, prob.O
    ptr = np.asarray(prob.lm_obs_ptr, np.int64)
    lm_of = np.repeat(np.arange(L), np.diff(ptr))
    Jp, Jl = Jp.reshape(O, 2, 6), Jl.reshape(O, 2, 3)
    W = np.einsum("oki,okj->oij", Jp, Jl)
    H = np.zeros((L, 3, 3))
    np.add.at(H, lm_of, np.einsum("oki,okj->oij", Jl, Jl))
    Hi = np.linalg.inv(H)
    pr = np.asarray(pairs, np.int64).reshape(-1, 2)
    keys = np.concatenate([pr[:, 0] * K + pr[:, 1], np.arange(K, dtype=np.int64) * (K + 1)])
    blocks = np.concatenate([pair_cov, kf_cov])
    order = np.argsort(keys)
    keys = keys[order]
    free = np.asarray(prob.kf_fixed)[prob.obs_kf] == 0
    kf = np.asarray(prob.obs_kf, np.int64)
    out = np.zeros((L, 3, 3))
    terms = 0
    for l0 in range(0, L, chunk):
        l1 = min(L, l0 + chunk)
        oa, ob, ll = [], [], []
        for l in range(l0, l1):
            o = np.arange(ptr[l], ptr[l + 1]); o = o[free[o]]
            g = np.meshgrid(o, o, indexing="ij")
            oa.append(g[0].ravel()); ob.append(g[1].ravel()); ll.append(np.full(len(o) ** 2, l - l0))
        oa, ob, ll = np.concatenate(oa), np.concatenate(ob), np.concatenate(ll)
        terms += len(oa)
        q = np.searchsorted(keys, kf[oa] * K + kf[ob])
        assert np.array_equal(keys[q], kf[oa] * K + kf[ob]), "a covisible pair without a block"
        T = np.einsum("pij,pjk->pik", blocks[order[q]], W[ob])
        M = np.zeros((l1 - l0, 3, 3))
        np.add.at(M, ll, np.einsum("pji,pjk->pik", W[oa], T))
        out[l0:l1] = Hi[l0:l1] + Hi[l0:l1] @ M @ Hi[l0:l1]
    return out, terms


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--map", default="mh12345")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lmcov_bench.json"))
    a = ap.parse_args()
    from oracle import covo
    m = synth.make_map(synth.config_named(a.map))
    prob, idx = mapdata.flatten_gba(m, visual_only=False, loop_loss=True)
    opt = backend.default_options()
    pairs = _system_pairs(prob)
    r, Jp, Jl, c = covo.linearize_reprojection(prob, covo.default_options(visual_only=0))
    ctx = backend.Context(0)
    gn_ms, gn_all, _ = _median_ms(lambda: ctx.gn_step(prob, opt, 0.0), a.repeats)
    ctx.upload(prob, opt)
    call_ms, call_all, (kc, pc, ok, st_old) = _median_ms(lambda: ctx.keyframe_covariances_resident(opt, block="pose", mu=0.0, pairs=pairs), a.repeats)
    assert ok.all()
    host_ms, host_all, (old, terms) = _median_ms(lambda: host_combination(prob, Jp, Jl, kc, pc, pairs), a.repeats)
    new_ms, new_all, (cov, lm_ok, _, st) = _median_ms(lambda: ctx.landmark_covariances_resident(opt, mu=0.0), a.repeats)
    kf_ms, kf_all, (cov2, _, kf_cov, st2) = _median_ms(lambda: ctx.landmark_covariances_resident(opt, mu=0.0, want_kf=True), a.repeats)
    ctx.close()
    good = lm_ok != 0
    nobs = np.diff(prob.lm_obs_ptr)
    row = dict(landmarks=int(prob.L), observations=int(prob.O), served=int(good.sum()), gather_terms=int(terms), mean_track=float(nobs.mean()),
               max_track=int(nobs.max()), stats=st, stats_with_kf=st2, gn_step_ms=gn_ms,
               old_call_ms=call_ms, old_call_ms_all=call_all, old_pairs=len(pairs), old_blocks_mb=float(pc.nbytes / 1e6),
               old_host_ms=host_ms, old_host_ms_all=host_all, old_route_ms=call_ms + host_ms,
               one_call_ms=new_ms, one_call_ms_all=new_all, one_call_with_kf_ms=kf_ms, one_call_with_kf_ms_all=kf_all,
               old_route_over_one_call=(call_ms + host_ms) / new_ms, old_call_alone_over_one_call=call_ms / new_ms,
               one_call_over_gn_step=new_ms / gn_ms, one_call_faster_than_old_route=bool(new_ms < call_ms + host_ms),
               same_bits_with_kf=bool(np.array_equal(cov, cov2)), kf_cov_equals_old_call=bool(np.array_equal(kf_cov, kc)),
               symmetric=bool(np.array_equal(cov, cov.transpose(0, 2, 1))), min_eigenvalue=float(np.linalg.eigvalsh(cov[good]).min()),
               max_diff_to_old_route_rel=float(np.abs(cov[good] - old[good]).max() / np.abs(old[good]).max()),
               max_diff_per_landmark_rel=float((np.abs(cov[good] - old[good]).reshape(-1, 9).max(1) / np.abs(old[good]).reshape(-1, 9).max(1)).max()))
    print(json.dumps(row), flush=True)
    out = dict(tool="tools/lmcov_bench.py", map=a.map, unknowns=int(15 * prob.K), keyframes=int(prob.K), repeats=a.repeats, gn_step_ms_all=gn_all,
               note="one_call_ms: Context.landmark_covariances_resident through the Python binding (linearisation, factorisation at mu = 0, the "
               "top-down sweep, the landmark pass, download); old_call_ms: Context.keyframe_covariances_resident with every off-diagonal block "
               "pair of the oracle's S, both orders; old_host_ms: the block formula combined in numpy from those blocks and the oracle's "
               "Jacobians (the linearisation itself is not timed); gn_step_ms: Context.gn_step of the same context and problem. Medians of "
               "`repeats` after one warm-up, all from one run on one machine. Wall-clock times of whole "
               "calls: the landmark kernel's own time between events and the bytes its gather moves were not measured.", rows=[row])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    if not row["one_call_faster_than_old_route"]:
        sys.exit("the one call is not faster than the old route")


if __name__ == "__main__":
    main()
