"""Reference restatement of Map::RemoveRedundantData (map_be.cpp:745-811) for the tests of covgpu_prune_redundant.

The rule, in this project's words.

Value of a keyframe (Keyframe::ComputeRedundancyValue, keyframe_be.cpp:228-256). A landmark seen by n live observations is worth
v(n) tenths: 0 for n <= 2, then 4, 7, 9 for n = 3, 4, 5 and 10 from 6 on. An observation is live while its keyframe is valid and has not
been erased. For keyframe k, over its live observations of valid landmarks with n >= 2: num[k] = sum of v(n), den[k] = how many there are;
the redundancy value is num / (10 den). A (keyframe, landmark) pair listed twice counts twice, in n and in num / den.

Candidates (:752-759): valid keyframes with id_.first != 0 that have a predecessor and a successor, fixed before the first round.

A round: pick the candidate of largest value (den == 0 after every den > 0, equal values to the lowest table index). Stop before picking
when, in this order: count mode and no more than max_kfs valid keyframes are left (reason 2); no candidate is left (0); threshold mode and
the pick has den == 0 or (double)num / (double)(10 den) < th_red (1); max_rounds rounds have run (3). The pick leaves the candidate list.
It stays in the map when time[succ] - time[pred] >= max_time_dist (action 1), else when it is a loop keyframe (2), else when not_erase is
set (3: SetInvalid refuses, keyframe_be.cpp:510, yet the reference counts it as removed). Otherwise it is erased (0, SetInvalid :514-526):
its observations stop being live, succ[pred] = succ, pred[succ] = pred, one valid keyframe less.

Three departures from the letter of the reference, each one legitimate outcome of it: std::sort leaves the order of equal values to the
implementation (here: lowest index); a 0/0 value is NaN there and makes its comparator no strict weak order (here: den == 0 ranks last);
the reference sums the doubles 0.4 / 0.7 / 0.9 / 1.0 in feature order (here: integer tenths, compared by cross-multiplication).

`prune_exact` is that rule, recomputed from nothing every round: the yardstick the library is compared with bit for bit.
`validate_literal` replays a round list and checks every choice against the values computed the reference's way.
"""
import numpy as np

V10 = np.array([0, 0, 0, 4, 7, 9, 10], np.int64)          # tenths, by min(n, 6)
VLIT = np.array([0.0, 0.0, 0.0, 0.4, 0.7, 0.9, 1.0])      # the reference's doubles
DEFAULT_OPTS = dict(th_red=0.95, max_time_dist=1.0, max_kfs=-1, max_rounds=0)   # config_backend.yaml:58-59


def make_inputs(lm_obs_ptr, obs_kf, kf_pred, kf_succ, kf_time, lm_invalid=None, kf_invalid=None, kf_first=None, kf_loop=None,
                kf_not_erase=None):
    K, L = len(kf_pred), len(lm_obs_ptr) - 1
    flag = lambda a, n: np.zeros(n, bool) if a is None else np.asarray(a).astype(bool)
    return dict(K=K, L=L, lm_obs_ptr=np.asarray(lm_obs_ptr, np.int32), obs_kf=np.asarray(obs_kf, np.int32).reshape(-1),
                kf_pred=np.asarray(kf_pred, np.int32), kf_succ=np.asarray(kf_succ, np.int32), kf_time=np.asarray(kf_time, np.float64),
                lm_invalid=flag(lm_invalid, L), kf_invalid=flag(kf_invalid, K), kf_first=flag(kf_first, K), kf_loop=flag(kf_loop, K),
                kf_not_erase=flag(kf_not_erase, K))


def inputs_of_map(m, kf_not_erase=None):
    """The call's inputs from a SlamMap: id_.first == 0, the keyframes of the map's loop constraints as loop keyframes."""
    loop = np.zeros(m.K, bool)
    for l in m.loops:
        loop[l.kf1] = loop[l.kf2] = True
    return make_inputs(m.lm_obs_ptr, m.obs_kf, m.kf_pred, m.kf_succ, m.kf_time, m.lm_invalid, m.kf_invalid, m.kf_id == 0, loop, kf_not_erase)


def thinned(inp, keep=0.45, seed=0):
    """The same inputs with a seeded ~`keep` share of the observations: tracks come down to 2..7, where the buckets change."""
    mask = np.random.default_rng(seed).random(len(inp["obs_kf"])) < keep
    obs_lm = np.repeat(np.arange(inp["L"]), np.diff(inp["lm_obs_ptr"]))
    cnt = np.bincount(obs_lm[mask], minlength=inp["L"])
    return dict(inp, obs_kf=inp["obs_kf"][mask], lm_obs_ptr=np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32))


def candidates(inp):
    return ~inp["kf_invalid"] & ~inp["kf_first"] & (inp["kf_pred"] >= 0) & (inp["kf_succ"] >= 0)


def counts(inp, live_kf):
    """(lm_nobs [L], num [K], den [K]) of the map with the keyframes `live_kf` [K] bool."""
    K, L = inp["K"], inp["L"]
    obs_lm = np.repeat(np.arange(L), np.diff(inp["lm_obs_ptr"]))
    live = live_kf[inp["obs_kf"]] if len(obs_lm) else np.zeros(0, bool)
    nobs = np.bincount(obs_lm[live], minlength=L).astype(np.int64)
    counted = live & ~inp["lm_invalid"][obs_lm] & (nobs[obs_lm] >= 2)
    v = V10[np.minimum(nobs, 6)]
    num = np.bincount(inp["obs_kf"][counted], weights=v[obs_lm[counted]], minlength=K).astype(np.int64)   # (sums of small integers: exact)
    den = np.bincount(inp["obs_kf"][counted], minlength=K).astype(np.int64)
    return nobs, num, den


def gate(inp, k, pred, succ, opts):
    if inp["kf_time"][succ[k]] - inp["kf_time"][pred[k]] >= opts["max_time_dist"]:
        return 1
    if inp["kf_loop"][k]:
        return 2
    if inp["kf_not_erase"][k]:
        return 3
    return 0


def prune_exact(inp, **kw):
    opts = dict(DEFAULT_OPTS, **kw)
    K = inp["K"]
    live = ~inp["kf_invalid"]
    cand = candidates(inp)
    pred, succ = inp["kf_pred"].copy(), inp["kf_succ"].copy()
    valid = int(live.sum())
    max_rounds = opts["max_rounds"] if opts["max_rounds"] > 0 else K
    count_mode = opts["max_kfs"] >= 0
    rounds, actions = [], []
    nobs, num, den = counts(inp, live)
    out_num, out_den = np.zeros(K, np.int64), np.zeros(K, np.int64)
    handled = np.zeros(K, bool)
    while True:
        if count_mode and valid <= opts["max_kfs"]:
            stop = 2; break
        c = np.flatnonzero(cand)
        if len(c) == 0:
            stop = 0; break
        assert den.max(initial=0) < 2 ** 26   # then two different ratios of such integers differ in double, and equal ones are the same double
        ratio = np.where(den[c] > 0, num[c] / np.maximum(den[c], 1), -1.0)
        k = int(c[np.argmax(ratio)])           # the first maximum: the lowest index
        if not count_mode and (den[k] == 0 or float(num[k]) / float(10 * den[k]) < opts["th_red"]):
            stop = 1; break
        if len(rounds) == max_rounds:
            stop = 3; break
        a = gate(inp, k, pred, succ, opts)
        rounds.append(k); actions.append(a)
        cand[k] = False
        handled[k] = True; out_num[k], out_den[k] = num[k], den[k]
        if a == 0:
            live[k] = False
            valid -= 1
            succ[pred[k]] = succ[k]; pred[succ[k]] = pred[k]
            nobs, num, den = counts(inp, live)
    out_num[~handled], out_den[~handled] = num[~handled], den[~handled]
    actions = np.array(actions, np.int32)
    return dict(round_kf=np.array(rounds, np.int32), round_action=actions, num_rounds=len(rounds),
                removed=int(((actions == 0) | (actions == 3)).sum()), stop_reason=stop, kf_pred=pred, kf_succ=succ,
                lm_nobs=nobs.astype(np.int32), red_num=out_num.astype(np.int32), red_den=out_den.astype(np.int32))


def literal_values(inp, live_kf):
    """Every keyframe's value the reference's way: a sequential double sum of 0.4 / 0.7 / 0.9 / 1.0 over its landmarks in landmark order,
    one division by the double count. NaN where nothing counts. (A row-wise cumsum adds strictly left to right; the zeros of the
    landmarks that do not count change no partial sum.)"""
    K, L = inp["K"], inp["L"]
    obs_lm = np.repeat(np.arange(L), np.diff(inp["lm_obs_ptr"]))
    live = live_kf[inp["obs_kf"]] if len(obs_lm) else np.zeros(0, bool)
    nobs = np.bincount(obs_lm[live], minlength=L)
    counted = live & ~inp["lm_invalid"][obs_lm] & (nobs[obs_lm] >= 2)
    order = np.argsort(inp["obs_kf"], kind="stable")              # keyframe-major, landmarks ascending within a keyframe
    kf = inp["obs_kf"][order]
    per = np.bincount(kf, minlength=K)
    col = np.arange(len(kf)) - np.repeat(np.cumsum(per) - per, per)
    tab = np.zeros((K, max(int(per.max(initial=0)), 1)))
    tab[kf, col] = np.where(counted[order], VLIT[np.minimum(nobs[obs_lm[order]], 6)], 0.0)
    red_sum = np.cumsum(tab, axis=1)[:, -1]
    n_lms = np.bincount(inp["obs_kf"][counted], minlength=K).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return red_sum / n_lms


def validate_literal(inp, rounds, stop_reason=None, final=None, tol=1e-12, **kw):
    """Replays `rounds` = [(keyframe, action), ...] and asserts that each is a choice the reference could have made: the chosen
    keyframe is a remaining candidate whose literal value is within `tol` of the literal maximum, going on or stopping agrees with the
    literal decision wherever the literal top value is further than `tol` from th_red, the action is the gate's, and the relinked chain is
    the one SetInvalid leaves. `final`: a result dict whose kf_pred / kf_succ / removed / lm_nobs are compared with the replay's.
    Returns the number of rounds whose two best literal values were within `tol` of each other."""
    opts = dict(DEFAULT_OPTS, **kw)
    live = ~inp["kf_invalid"]
    cand = candidates(inp)
    pred, succ = inp["kf_pred"].copy(), inp["kf_succ"].copy()
    valid = int(live.sum())
    count_mode = opts["max_kfs"] >= 0
    near_ties = removed = 0

    def top_of(val):
        c = np.flatnonzero(cand)
        v = val[c]
        return (np.nanmax(v) if np.isfinite(v).any() else np.nan), v

    for r, (k, a) in enumerate(rounds):
        assert cand[k], f"round {r}: keyframe {k} is no remaining candidate"
        if count_mode:
            assert valid > opts["max_kfs"], f"round {r}: ran although only {valid} keyframes were left"
        val = literal_values(inp, live)
        top, v = top_of(val)
        if np.isnan(top):
            assert count_mode, f"round {r}: threshold mode went on with nothing to rank"
        else:
            assert val[k] >= top - tol, f"round {r}: keyframe {k} has value {val[k]}, the maximum is {top}"
            near_ties += int((np.sort(v[np.isfinite(v)])[-2:] >= top - tol).sum() == 2)
            if not count_mode and abs(top - opts["th_red"]) > tol:
                assert top >= opts["th_red"], f"round {r}: went on below the threshold ({top})"
        assert a == gate(inp, k, pred, succ, opts), f"round {r}: action {a}"
        cand[k] = False
        if a in (0, 3):
            removed += 1
        if a == 0:
            live[k] = False
            valid -= 1
            succ[pred[k]] = succ[k]; pred[succ[k]] = pred[k]
    if stop_reason is not None:
        top, _ = top_of(literal_values(inp, live))
        if stop_reason == 2:
            assert count_mode and valid <= opts["max_kfs"]
        elif stop_reason == 0:
            assert not cand.any() and not (count_mode and valid <= opts["max_kfs"])
        elif stop_reason == 1:
            assert not count_mode and cand.any()
            if not np.isnan(top) and abs(top - opts["th_red"]) > tol:
                assert top < opts["th_red"], f"stopped above the threshold ({top})"
        else:
            assert stop_reason == 3 and opts["max_rounds"] > 0 and len(rounds) == opts["max_rounds"] and cand.any()
    if final is not None:
        assert np.array_equal(final["kf_pred"], pred) and np.array_equal(final["kf_succ"], succ)
        assert final["removed"] == removed
        assert np.array_equal(final["lm_nobs"], counts(inp, live)[0])
    return near_ties
