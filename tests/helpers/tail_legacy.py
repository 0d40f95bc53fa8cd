"""The runs of the trust-region tail's points (tests/tail_util.POINTS) on a context: run_point() is what tests/test_gpu_tail.py calls in its own
process; as a program it is that test's worker for the COVGPU_TAIL=0 form — the library reads the switch once per process, so the legacy ladders
run in THIS process (the parent sets the variable) and their records travel back as a pickle."""
import os
import pickle
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def run_point(ctx, pt):
    """One traced resident solve per run of the point: [dict(kw = the options, trace [rounds, TR_COUNT], ts = what the last iteration left on the
    device, after = the estimate the solve left, res = the result's fields)]."""
    from covins_amd import backend, capi
    T = capi.TR
    p = pt.build()
    recs = []
    for run in pt.runs:
        kw = dict(pt.opt, **run.kw)
        if kw.get("initial_radius") == "interp":   # between the Cauchy point and the Gauss-Newton step of the point's first run (tail_util.Run)
            row = recs[0]["trace"][-1]
            kw["initial_radius"] = float(np.sqrt(np.sqrt(row[T["GN2"]]) * np.sqrt(row[T["GG"]]) * row[T["ALPHA"]]))
        o = backend.default_options(**kw)
        if not recs:
            ctx.upload(p, o, pgo=pt.pgo)
        res, trace = ctx.solve_resident_traced(o)
        ts = ctx.fetch_tail_state(o)
        q = ctx.download()
        n = res.iterations
        recs.append(dict(kw=kw, trace=trace, ts=ts, after=dict(pose=q.kf_pose.copy(), sb=q.kf_speed_bias.copy(), lm=q.lm_pos.copy()),
                         res=dict(iterations=n, accepted=res.accepted, termination=res.termination, initial_cost=res.initial_cost,
                                  final_cost=res.final_cost, cost_trace=list(res.cost_trace[:n]), radius_trace=list(res.radius_trace[:n]),
                                  accepted_trace=list(res.accepted_trace[:n]))))
    return recs


if __name__ == "__main__":
    out = sys.argv[1]
    import torch
    torch.cuda.init()
    from covins_amd import backend
    from tests import tail_util as tu
    ctx = backend.Context(0)
    records = {name: run_point(ctx, tu.POINT[name]) for name in tu.LEGACY_POINTS}
    ctx.close()
    with open(out, "wb") as f:
        pickle.dump(dict(tail=os.environ.get("COVGPU_TAIL"), records=records), f)
