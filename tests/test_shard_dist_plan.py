"""Shard policy 1, "distributed top"  — host part: covgpu_shard_plan with options.shard_policy = 1 on the 5-agent map and on
configs[4]'s shape at 12 x 1000 keyframes, at 2, 4 and 8 ranks. Policy 0 stays what it was (same plan, same digest); policy 1's top is
ancestor-closed and holds every front of 4 096 unknowns or more; the tile rows of every top front's trailing block are dealt to exactly one
rank each; the busiest rank's share of the factorisation flops (the library's own accounting) is strictly below policy 0's."""
import threading

import numpy as np
import pytest

from covins_amd import backend, capi, distrib, mapdata, synth

_cache = {}
MIN_ORDER = 4096   # nd_shard_assign_dist


def problem(name):
    if name not in _cache:
        _cache[name] = mapdata.flatten_gba(synth.make_map(synth.config_named(name)), False, True)[0]
    return _cache[name]


def options(policy):
    o = backend.default_options()
    o.shard_policy = policy
    return o


def fronts(plan):
    """parent, own order, border order per tree node, and the plan's total flops (covgpu_nd_plan_info / covgpu_nd_plan_arrays)."""
    import ctypes as C
    lib = backend.lib()
    info = (C.c_int64 * 16)()
    lib.covgpu_nd_plan_info(plan.handle, info)
    nn = int(info[0])
    parent = np.zeros(nn, np.int32); level = np.zeros(nn, np.int32); optr = np.zeros(nn + 1, np.int32); sptr = np.zeros(nn + 1, np.int32)
    ov = np.zeros(max(int(info[3]), 1), np.int32); sv = np.zeros(max(int(info[4]), 1), np.int32)
    lib.covgpu_nd_plan_arrays(plan.handle, capi.iptr(parent), capi.iptr(level), capi.iptr(optr), capi.iptr(ov), capi.iptr(sptr), capi.iptr(sv))
    dim = lambda v: np.where(v & 1, 9, 6)
    own = np.array([dim(ov[optr[n]:optr[n + 1]]).sum() for n in range(nn)])
    st = np.array([dim(sv[sptr[n]:sptr[n + 1]]).sum() for n in range(nn)])
    return parent, own, st, float(info[6]), int(info[13])


@pytest.mark.parametrize("name", ["mh12345", "a12x1000"])
def test_distributed_top_plan(name):
    p = problem(name)
    for world in (2, 4, 8):
        pl0 = distrib.shard_plan(p, backend.default_options(), world)
        pl0b = distrib.shard_plan(p, options(0), world)
        assert pl0.shard_policy == 0 and pl0b.shard_policy == 0
        assert distrib.plan_digest(pl0) == distrib.plan_digest(pl0b)           # policy 0 is the default, bit for bit
        pl1 = distrib.shard_plan(p, options(1), world)
        assert pl1 is not None and pl1.shard_policy == 1 and pl1.world == world
        assert distrib.plan_digest(pl1) != distrib.plan_digest(pl0)
        parent, own, st, total, pol = fronts(pl1)
        assert pol == 1
        top = pl1.node_rank < 0
        assert top[parent < 0].all()
        assert all(top[parent[n]] for n in np.nonzero(top)[0] if parent[n] >= 0)   # ancestor-closed
        assert top[own + st >= MIN_ORDER].all()                                    # every big front is distributed
        assert ((pl1.node_rank >= -1) & (pl1.node_rank < world)).all()
        # the busiest rank's share of the factorisation under the library's own accounting: strictly below the replicated top's
        f0, f1 = distrib.rank_flops(pl0), distrib.rank_flops(pl1)
        assert f0.size == world and f1.size == world
        print(f"{name} world {world}: busiest rank {f1.max() / total:.3f} of the flops (distributed top) against {f0.max() / total:.3f} (replicated), "
              f"{distrib.exchange(pl1)['bytes'] / 1e6:.1f} MB / {distrib.exchange(pl1)['collectives']} collectives per linear solve against "
              f"{distrib.exchange(pl0)['bytes'] / 1e6:.1f} MB / 1")
        assert f1.max() < f0.max()
        # the accounting covers the whole factorisation: the sum over the ranks is the plan's flops plus the redundant panel chains
        assert f1.sum() >= 0.99 * total and f0.sum() >= 0.99 * total
        for pl in (pl0, pl0b, pl1):
            pl.close()


def test_tile_rows_of_the_top_partition_over_the_ranks():
    """nd_tile_owner: (tile row + node) mod world — each tile row of a top front's trailing block has exactly one owner, and the owned update flops
    of the accounting add up to the update flops of the whole top."""
    p = problem("mh12345")
    for world in (2, 4, 8):
        pl = distrib.shard_plan(p, options(1), world)
        parent, own, st, total, _ = fronts(pl)
        top = np.nonzero(pl.node_rank < 0)[0]
        f = distrib.rank_flops(pl)
        # subtrees by rank, from the plan's node owners
        sub = np.zeros(world)
        fl = own ** 3 / 3.0 + own.astype(float) ** 2 * st + own * st.astype(float) ** 2
        for n in np.nonzero(pl.node_rank >= 0)[0]:
            sub[pl.node_rank[n]] += fl[n]
        upd = np.zeros(world); chain = 0.0
        for n in top:
            nIr, nO = -(-own[n] // 128), -(-st[n] // 128)
            rows = [min(128, own[n] - 128 * q) for q in range(nIr)] + [min(128, st[n] - 128 * q) for q in range(nO)]
            for P in range(-(-own[n] // 256)):
                k = min(256, own[n] - 256 * P)
                chain += k ** 3 / 3.0 + k * k * (own[n] - 256 * P - k + st[n])
                left = 0.0
                owners = [(q + n) % world for q in range(2 * P + 2, nIr + nO)]
                assert all(0 <= r < world for r in owners)
                for q, r in zip(range(2 * P + 2, nIr + nO), owners):
                    upd[r] += k * rows[q] * (2.0 * left + rows[q])
                    left += rows[q]
        assert np.allclose(f, sub + chain + upd, rtol=1e-12)
        pl.close()


def test_ranks_with_different_policies_refuse_before_any_collective():
    """The digest exchange of distrib.attach (distrib.check_plan_digest) refuses ranks whose plans differ only in the policy: every rank raises."""
    import torch.distributed as dist
    p = problem("mh12345")
    d0 = distrib.plan_digest(distrib.shard_plan(p, options(0), 2))
    d1 = distrib.plan_digest(distrib.shard_plan(p, options(1), 2))
    store = dist.HashStore()
    errs = [None, None]

    def rank(r, digest):
        try:
            distrib.check_plan_digest(store, r, 2, digest)
        except Exception as e:
            errs[r] = e

    th = [threading.Thread(target=rank, args=(0, d0)), threading.Thread(target=rank, args=(1, d1))]
    for t in th: t.start()
    for t in th: t.join(timeout=120)
    assert all(e is not None and "digest" in str(e) for e in errs), errs
