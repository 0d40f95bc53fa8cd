#!/usr/bin/env python3
"""Times Context.observation_covariances_resident with all its outputs on the 5-agent synthetic map, visual-inertial, mu = 0,
through the Python binding, against Context.landmark_covariances_resident and against the only route there was before it:
Context.keyframe_covariances_resident with every off-diagonal block pair of the oracle's S, and the blocks combined in numpy on the host
(Sigma_al = -sum_b Sigma_ab W_b H_ll^-1, Sigma_l by the block formula, C_o = J Sigma J^T). All figures come from one run, medians of `repeats`
after one warm-up; the host part starts from the Jacobians of the oracle's linearisation, which is not timed. Acceptance: the one call is
faster than the old route in this run; the ratio to the landmark call is recorded. Writes one JSON file (default
profiles/obscov_bench.json). Needs an MI355X."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

from covins_amd import backend, mapdata, synth  # noqa: E402
from lmcov_bench import _median_ms, _system_pairs  # noqa: E402


def host_combination(prob, Jp, Jl, kf_cov, pair_cov, pairs, chunk=2048):
    """(C_o [O, 2, 2], Sigma_al [O, 6, 3]) on the host from the pose-pose blocks: every (a, b) of a landmark's free observers looks its 6x6
    block up (a diagonal block, or the pair's in the order (keyframe of a, keyframe of b)), landmarks in chunks."""
    K, L, O = prob.K, prob.L, prob.O
    ptr = np.asarray(prob.lm_obs_ptr, np.int64)
    lm_of = np.repeat(np.arange(L), np.diff(ptr))
    kf = np.asarray(prob.obs_kf, np.int64)
    free = np.asarray(prob.kf_fixed)[kf] == 0
    Jp, Jl = np.array(Jp).reshape(O, 2, 6), np.asarray(Jl).reshape(O, 2, 3)
    Jp[~free] = 0.0
    W = np.einsum("oki,okj->oij", Jp, Jl)
    H = np.zeros((L, 3, 3))
    np.add.at(H, lm_of, np.einsum("oki,okj->oij", Jl, Jl))
    Hi = np.linalg.inv(H)
    pr = np.asarray(pairs, np.int64).reshape(-1, 2)
    keys = np.concatenate([pr[:, 0] * K + pr[:, 1], np.arange(K, dtype=np.int64) * (K + 1)])
    blocks = np.concatenate([pair_cov, kf_cov])
    order = np.argsort(keys)
    keys = keys[order]
    G = np.zeros((O, 6, 3))           # sum_b Sigma_ab W_b per observation a
    for l0 in range(0, L, chunk):
        l1 = min(L, l0 + chunk)
        oa, ob = [], []
        for l in range(l0, l1):
            o = np.arange(ptr[l], ptr[l + 1]); o = o[free[o]]
            g = np.meshgrid(o, o, indexing="ij")
            oa.append(g[0].ravel()); ob.append(g[1].ravel())
        oa, ob = np.concatenate(oa), np.concatenate(ob)
        q = np.searchsorted(keys, kf[oa] * K + kf[ob])
        assert np.array_equal(keys[q], kf[oa] * K + kf[ob]), "a covisible pair without a block"
        np.add.at(G, oa, np.einsum("pij,pjk->pik", blocks[order[q]], W[ob]))
    M = np.zeros((L, 3, 3))
    np.add.at(M, lm_of, np.einsum("oji,ojk->oik", W, G))
    Sl = Hi + Hi @ M @ Hi
    X = -G @ Hi[lm_of]
    cx = Jp @ X @ Jl.transpose(0, 2, 1)
    C = Jp @ kf_cov[kf] @ Jp.transpose(0, 2, 1) + cx + cx.transpose(0, 2, 1) + Jl @ Sl[lm_of] @ Jl.transpose(0, 2, 1)
    return C, X


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--map", default="mh12345")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "obscov_bench.json"))
    a = ap.parse_args()
    from oracle import covo
    m = synth.make_map(synth.config_named(a.map))
    prob, idx = mapdata.flatten_gba(m, visual_only=False, loop_loss=True)
    opt = backend.default_options()
    pairs = _system_pairs(prob)
    r, Jp, Jl, c = covo.linearize_reprojection(prob, covo.default_options(visual_only=0))
    ctx = backend.Context(0)
    ctx.upload(prob, opt)
    every = dict(want_cross=True, want_res=True, want_lm=True, want_kf=True)
    new_ms, new_all, res = _median_ms(lambda: ctx.observation_covariances_resident(opt, mu=0.0, **every), a.repeats)
    bare_ms, bare_all, bare = _median_ms(lambda: ctx.observation_covariances_resident(opt, mu=0.0, want_cross=False, want_res=False), a.repeats)
    lm_ms, lm_all, (lm_cov, lm_ok, kf_cov, st_lm) = _median_ms(lambda: ctx.landmark_covariances_resident(opt, mu=0.0, want_kf=True), a.repeats)
    call_ms, call_all, (kc, pc, ok, st_old) = _median_ms(lambda: ctx.keyframe_covariances_resident(opt, block="pose", mu=0.0, pairs=pairs), a.repeats)
    assert ok.all()
    ctx.close()
    host_ms, host_all, (C_old, X_old) = _median_ms(lambda: host_combination(prob, Jp, Jl, kc, pc, pairs), a.repeats)
    good = res["obs_ok"] != 0
    C, X = res["obs_cov"], res["cross_cov"]
    w = np.linalg.eigvalsh(C[good])
    nobs = np.diff(prob.lm_obs_ptr)
    row = dict(landmarks=int(prob.L), observations=int(prob.O), served=int(good.sum()), gather_terms=int((nobs.astype(np.int64) ** 2).sum()),
               mean_track=float(nobs.mean()), stats=res["stats"], stats_landmark_call=st_lm,
               old_call_ms=call_ms, old_call_ms_all=call_all, old_pairs=len(pairs), old_host_ms=host_ms, old_host_ms_all=host_all,
               old_route_ms=call_ms + host_ms, one_call_ms=new_ms, one_call_ms_all=new_all, one_call_obs_cov_only_ms=bare_ms,
               one_call_obs_cov_only_ms_all=bare_all, landmark_call_ms=lm_ms, landmark_call_ms_all=lm_all,
               old_route_over_one_call=(call_ms + host_ms) / new_ms, one_call_over_landmark_call=new_ms / lm_ms,
               one_call_faster_than_old_route=bool(new_ms < call_ms + host_ms), download_mb=float(sum(v.nbytes for v in res.values() if hasattr(v, "nbytes")) / 1e6),
               same_bits_without_optional_outputs=bool(np.array_equal(bare["obs_cov"], C) and np.array_equal(bare["obs_ok"], res["obs_ok"])),
               landmark_outputs_equal_landmark_call=bool(np.array_equal(lm_cov, res["lm_cov"]) and np.array_equal(lm_ok, res["lm_ok"]) and
                                                         np.array_equal(kf_cov, res["kf_cov"])),
               symmetric=bool(np.array_equal(C[:, 0, 1], C[:, 1, 0])), min_eigenvalue=float(w.min()), max_eigenvalue=float(w.max()),
               max_diff_to_old_route_block=float(np.abs(C[good] - C_old[good]).max()),
               max_diff_to_old_route_cross_rel=float(np.abs(X[good] - X_old[good]).max() / np.abs(X_old[good]).max()))
    print(json.dumps(row), flush=True)
    out = dict(tool="tools/obscov_bench.py", map=a.map, unknowns=int(15 * prob.K), keyframes=int(prob.K), repeats=a.repeats,
               note="one_call_ms: Context.observation_covariances_resident with every output through the Python binding (linearisation, "
               "factorisation at mu = 0, the top-down sweep, the observation pass, download); one_call_obs_cov_only_ms: the same with obs_cov and "
               "obs_ok alone; landmark_call_ms: Context.landmark_covariances_resident with kf_cov; old_call_ms: "
               "Context.keyframe_covariances_resident with every off-diagonal block pair of the oracle's S, both orders; old_host_ms: the blocks "
               "combined in numpy from those and the oracle's Jacobians (the linearisation itself is not timed). Medians of `repeats` after one "
               "warm-up, all from one run on one machine. Wall-clock times of whole calls: the kernel's own time between events and the "
               "bytes it moves were not measured.", rows=[row])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    if not row["one_call_faster_than_old_route"]:
        sys.exit("the one call is not faster than the old route")


if __name__ == "__main__":
    main()
