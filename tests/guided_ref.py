"""numpy restatement of the loop candidates' guided matching (covgpu_search_se3_batch / covgpu_search_projection_batch):
COVINS's FeatureMatcher::SearchBySE3 (feature_matcher_be.cpp:293-498) and FeatureMatcher::SearchByProjection (:168-291), line by line,
quirks included. It is the yardstick of the kernels: the reference's own FeatureMatcher needs OpenCV, Eigen and the Keyframe classes.

Common parts
  hamming()           popcount of the eight 32-bit XORs (:49-64).
  in_image()          KeyframeBase::IsInImage, keyframe_base.cpp:414-416: x >= xmin && x < xmax && y >= ymin && y < ymax.
  predict_scale()     LandmarkBase::PredictScale, landmark_base.cpp:120-133: the distance arrives through a `const float&`, so
                      ratio = max_distance / (double)(float)dist; n = ceil(log(ratio) / log(scale_factor)) clamped to [0, num_octaves - 1].
  visiting_order()    the order in which GetFeaturesInArea (keyframe_base.cpp:262-318) returns keypoints. Its grid branch and its
                      brute-force branch return the same set (a keypoint within the radius has its rounded cell inside the floor / ceil
                      cell window); brute force visits by ascending index (:276), the grid by ascending (cell_x, cell_y, index) (:301-313)
                      with cell = (int)std::round((double)kp * grid_inv) (AssignFeaturesToGrid, :134-139), grid_inv = 64 / width and
                      48 / height (typedefs_base.hpp:59-60). A cell outside the 64 x 48 grid is clamped to it: the reference writes out of
                      bounds there. The order matters because the best distance is taken with `<`: the first visited wins a tie.
  features_in_area()  the target narrowed to float (KeypointType is Matrix<float,2,1>, :263), distance = the float32
                      sqrt(dx*dx + dy*dy) of float differences, kept iff (double)distance <= radius (:277-278, :308-309).
  Level window        (int)keypoints_aors_[idx][1] in [predicted - 1, predicted] (:244, :380, :458).

search_se3(): one (query keyframe 1, candidate keyframe 2, T12) job. A keyframe is a dict: kp [n,2] float32 keypoints_distorted_,
level [n], desc [n,32], bounds (xmin, xmax, ymin, ymax), grid_inv (pair, or None for index order), K (fx, fy, cx, cy), and per row
lm_pos [n,3] (the row's landmark in the keyframe's own camera frame, Tcw * p_w: :343, :422), lm_max_distance, lm_desc
(Landmark::GetDescriptor(), not the keypoint's row), lm_free (landmark present, valid, not alreadyMatched: :313-339, :412-418).
Reproduced as they are:
  1. Projection: K * p / z only (:351-352, :431-432) — no distortion, no unified model — compared against *distorted* keypoints.
  2. Radius: th * 2.0^level, a hard-coded 2.0 and not scale_factor (:366, :443).
  3. Image test of the second direction: the projection into keyframe 1 is tested with keyframe 2's bounds (:433).
  4. Acceptance: first direction bestDist <= th_low (:403), second direction bestDist < th_low (:479).
  5. Agreement: match2[i] == i with i the *query* row (:486-495), not match2[match1[i]] == i. agreement = 0 is this literal test; rows
     i >= n2 never agree (the reference reads past match2 there). agreement = 1 is the evident intent, match2[match1[i]] == i.
  6. Depth: z < 0 skips the point (:347, :426); z == 0 goes on as IEEE arithmetic has it (inf or NaN, which IsInImage then refuses or
     not).
  7. No min/max-distance test and no viewing-angle test in this mode.

search_projection(): one (keyframe, Tcw, points) job; the keyframe dict has cam (fx fy cx cy d0..d3), dist_type, cam_model, xi instead
of K and `taken` [n] (vpMatched[idx] != NULL on entry, :240); points: p_w, normal, min_distance, max_distance, desc, skip (invalid or in
spAlreadyFound, :184), existing_idx (GetFeatureIndex(kf), :260). camera_->project3 is the keyframe's full model (pinhole or unified,
RadTan or equidistant: the formulas of DESIGN.md §2 row R5, as dev_math.hpp's project_camera, which refuses z <= 1e-10 — such a point
is skipped). Filters: z < 0 (:195), IsInImage (:204), 0.8 min_distance <= dist <= 1.2 max_distance with dist = |p_w - O_w| (:208-215,
landmark_base.cpp:68-76), PO . n >= 0.5 dist (:220). Radius th * scale_factor^level (:227). The points are sequential: a point only
sees keypoints that are not taken and that no earlier point has claimed (:240, :284); with bestDist <= th_low it claims its best
keypoint when existing_idx == -1 (:284-285), else nothing is claimed and the outcome is a remap proposal remap_to = bestIdx unless
hamming(desc_p, kp_desc[existing_idx]) < bestDist (:264-281). The dist_newplace test (:270-277) compares bestDist with the distance it
was taken from and can never fire; it is omitted. best_dist = bestDist when it is <= th_low, else -1.

Fragile points. A floating-point decision that sits on its boundary may fall on the other side on another machine (log, sqrt, a fused
multiply-add). A point is *fragile* when one of its decisions is within 1e-9 (relative) of the depth, min/max-distance or viewing-angle
test, 1e-6 px of an image bound, 1e-9 of an integer in log(ratio) / log(scale_factor) (only when num_octaves > 1), or 1e-3 px of the
radius for some keypoint's distance. Comparisons leave fragile points out; `evaluated` counts the points that passed the depth test."""
from __future__ import annotations

import math

import numpy as np

GRID_COLS, GRID_ROWS = 64, 48


def hamming(a, b):
    """Popcount of the eight 32-bit XORs of two 32-byte rows (feature_matcher_be.cpp:49-64)."""
    a = np.ascontiguousarray(a, np.uint8).view(np.uint32); b = np.ascontiguousarray(b, np.uint8).view(np.uint32)
    return int(np.bitwise_count(a ^ b).sum())


def hamming_rows(a, B):
    """Distances of row a to every row of B [n,32]."""
    B = np.ascontiguousarray(B, np.uint8).reshape(-1, 32).view(np.uint64)
    a = np.ascontiguousarray(a, np.uint8).reshape(1, 32).view(np.uint64)
    return np.bitwise_count(a ^ B).sum(-1).astype(np.int64)


def quat_matrix(q):
    """Rotation matrix of a Hamilton quaternion [x, y, z, w]."""
    x, y, z, w = (float(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def in_image(u, v, bounds):
    xmin, xmax, ymin, ymax = bounds
    return bool(u >= xmin and u < xmax and v >= ymin and v < ymax)


def near_image_bound(u, v, bounds, tol=1e-6):
    xmin, xmax, ymin, ymax = bounds
    if not (math.isfinite(u) and math.isfinite(v)):
        return False
    return bool(min(abs(u - xmin), abs(u - xmax)) <= tol or min(abs(v - ymin), abs(v - ymax)) <= tol)


def predict_scale(dist, max_distance, scale_factor, num_octaves):
    """(level, fragile). landmark_base.cpp:120-133."""
    ratio = float(max_distance) / float(np.float32(dist))
    x = math.log(ratio) / math.log(scale_factor)
    n = int(math.ceil(x))
    n = 0 if n < 0 else (num_octaves - 1 if n >= num_octaves else n)
    return n, num_octaves > 1 and abs(x - round(x)) <= 1e-9


def visiting_order(kp, grid_inv):
    """Keypoint indices in the order GetFeaturesInArea visits them (module doc): index order, or grid order with clamped cells."""
    kp = np.asarray(kp, np.float32).reshape(-1, 2)
    if grid_inv is None or not grid_inv[0] > 0:
        return np.arange(len(kp))
    rnd = lambda a: np.where(a >= 0, np.floor(a + 0.5), -np.floor(-a + 0.5))   # std::round: halves away from zero
    cx = np.clip(rnd(kp[:, 0].astype(np.float64) * grid_inv[0]), 0, GRID_COLS - 1).astype(np.int64)
    cy = np.clip(rnd(kp[:, 1].astype(np.float64) * grid_inv[1]), 0, GRID_ROWS - 1).astype(np.int64)
    return np.lexsort((np.arange(len(kp)), cy, cx))


def features_in_area(kp, order, u, v, radius):
    """(indices in visiting order, fragile). keyframe_base.cpp:262-318."""
    kp = np.asarray(kp, np.float32).reshape(-1, 2)
    dx = kp[:, 0] - np.float32(u); dy = kp[:, 1] - np.float32(v)                 # float32 throughout
    d = np.sqrt(dx * dx + dy * dy).astype(np.float64)
    inside = d <= radius
    order = np.asarray(order, np.int64)
    return order[inside[order]].tolist(), bool((np.abs(d - radius) <= 1e-3).any())


def _best(cands, levels, descs, desc, predicted, blocked=None):
    """The inner loop (:377-401, :453-478, :238-256) over the candidates in visiting order: `dist < bestDist`, so the first visited of
    the smallest distance wins (np.argmin returns the first)."""
    c = np.asarray(cands, np.int64)
    if blocked is not None:
        c = c[~blocked[c]]                                                         # if (vpMatched[idx]) continue;
    c = c[(levels[c] >= predicted - 1) & (levels[c] <= predicted)]
    if not len(c):
        return None, -1
    d = hamming_rows(desc, np.asarray(descs)[c])
    k = int(np.argmin(d))
    return int(d[k]), int(c[k])


def _se3_direction(src, dst, R, t, bounds, th, th_low, strict, scale_factor, num_octaves, order):
    """One direction of SearchBySE3: the free landmarks of `src` moved by (R, t) and projected into `dst` with dst's K; IsInImage with
    `bounds`. Returns match [n_src], fragile [n_src], evaluated (points that passed the depth test)."""
    n = len(src["kp"])
    match = np.full(n, -1, np.int64); fragile = np.zeros(n, bool)
    evaluated = 0
    fx, fy, cx, cy = (float(v) for v in dst["K"])
    levels = np.asarray(dst["level"]).astype(np.int64)
    for i in range(n):
        if not src["lm_free"][i]:
            continue
        p = R @ np.asarray(src["lm_pos"][i], np.float64) + t
        dist3d = float(np.sqrt(p @ p))
        if 0.0 < abs(p[2]) <= 1e-9 * dist3d:                                    # (an exact zero is no rounding matter: quirk 6)
            fragile[i] = True; evaluated += 1
            continue
        if p[2] < 0.0:
            continue
        evaluated += 1
        with np.errstate(divide="ignore", invalid="ignore"):
            u = (fx * p[0] + cx * p[2]) / p[2]; v = (fy * p[1] + cy * p[2]) / p[2]   # proj = K * p; proj / proj[2]
        if near_image_bound(u, v, bounds):
            fragile[i] = True
            continue
        if not in_image(u, v, bounds):
            continue
        level, frag = predict_scale(dist3d, src["lm_max_distance"][i], scale_factor, num_octaves)
        radius = th * 2.0 ** level
        cands, frag2 = features_in_area(dst["kp"], order, u, v, radius)
        if frag or frag2:
            fragile[i] = True
            continue
        bd, bi = _best(cands, levels, dst["desc"], src["lm_desc"][i], level)
        if bd is not None and (bd < th_low if strict else bd <= th_low):
            match[i] = bi
    return match, fragile, evaluated


def agree(match1, match2, agreement):
    """:485-495 from the two directions' matches."""
    n1, n2 = len(match1), len(match2)
    out = np.full(n1, -1, np.int64)
    for i in range(n1):
        idx2 = match1[i]
        if idx2 >= 0:
            ok = (match2[idx2] == i) if agreement else (i < n2 and match2[i] == i)
            if ok:
                out[i] = idx2
    return out


def search_se3(kf1, kf2, T12, radius=9.5, th_low=50, scale_factor=2.0, num_octaves=1, agreement=0):
    """dict(match [n1], match1 [n1], match2 [n2], nfound, fragile1 [n1], fragile2 [n2], evaluated)."""
    R12 = quat_matrix(T12[:4]); t12 = np.asarray(T12[4:7], np.float64)
    R21 = R12.T; t21 = -R12.T @ t12                                                # T21 = T12.inverse(), :303
    m1, f1, e1 = _se3_direction(kf1, kf2, R21, t21, kf2["bounds"], radius, th_low, False, scale_factor, num_octaves,
                                visiting_order(kf2["kp"], kf2.get("grid_inv")))
    m2, f2, e2 = _se3_direction(kf2, kf1, R12, t12, kf2["bounds"], radius, th_low, True, scale_factor, num_octaves,
                                visiting_order(kf1["kp"], kf1.get("grid_inv")))
    match = agree(m1, m2, agreement)
    return dict(match=match, match1=m1, match2=m2, nfound=int((match >= 0).sum()), fragile1=f1, fragile2=f2, evaluated=e1 + e2)


def se3_comparable(ref, agreement):
    """Rows of `match` whose value does not hang on a fragile point: the row's own first-direction point and the second-direction
    entry the agreement test reads for it."""
    n1, n2 = len(ref["match1"]), len(ref["match2"])
    ok = ~ref["fragile1"]
    for i in range(n1):
        k = ref["match1"][i] if agreement else (i if i < n2 else -1)
        if ok[i] and k >= 0 and ref["fragile2"][k]:
            ok[i] = False
    return ok


def project_camera(p, cam, dist_type, cam_model, xi):
    """The keyframe's camera: pinhole or unified, RadTan (0) or equidistant (1). None when it refuses the point."""
    fx, fy, cx, cy, d0, d1, d2, d3 = (float(v) for v in cam)
    X, Y, Z = (float(v) for v in p)
    if cam_model == 1:
        d = math.sqrt(X * X + Y * Y + Z * Z)
        D = Z + xi * d
        fxi = xi if xi <= 1.0 else 1.0 / xi
        if not Z > -fxi * d or not D > 1e-10:
            return None
        x, y = X / D, Y / D
    else:
        if not Z > 1e-10:
            return None
        x, y = X / Z, Y / Z
    r2 = x * x + y * y
    if dist_type == 0:
        rad = (d0 + d1 * r2) * r2
        xd = x + x * rad + 2.0 * d2 * x * y + d3 * (r2 + 2.0 * x * x)
        yd = y + y * rad + 2.0 * d3 * x * y + d2 * (r2 + 2.0 * y * y)
    else:
        rho = math.sqrt(r2)
        if rho < 1e-8:
            xd, yd = x, y
        else:
            th = math.atan(rho); t2 = th * th
            sc = th * (1.0 + t2 * (d0 + t2 * (d1 + t2 * (d2 + t2 * d3)))) / rho
            xd, yd = sc * x, sc * y
    return fx * xd + cx, fy * yd + cy


def search_projection(kf, T_cw, pts, radius=10.0, th_low=50, scale_factor=2.0, num_octaves=1, agreement=0):
    """dict(claimed [P], remap_to [P], best_dist [P], nmatches, fragile [P], evaluated)."""
    R = quat_matrix(T_cw[:4]); t = np.asarray(T_cw[4:7], np.float64)
    Ow = -R.T @ t                                                                  # :172
    P = len(pts["p_w"]); n = len(kf["kp"])
    claimed = np.full(P, -1, np.int64); remap = np.full(P, -1, np.int64); best = np.full(P, -1, np.int64)
    fragile = np.zeros(P, bool)
    evaluated = nmatches = 0
    blocked = np.zeros(n, bool) if kf.get("taken") is None else np.asarray(kf["taken"]).astype(bool).copy()   # vpMatched[idx] != NULL
    order = visiting_order(kf["kp"], kf.get("grid_inv"))
    levels = np.asarray(kf["level"]).astype(np.int64)
    skip = pts.get("skip"); existing = pts.get("existing_idx")
    for p in range(P):
        if skip is not None and skip[p]:
            continue
        pw = np.asarray(pts["p_w"][p], np.float64)
        pc = R @ pw + t
        if 0.0 < abs(pc[2]) <= 1e-9 * float(np.sqrt(pc @ pc)):
            fragile[p] = True; evaluated += 1
            continue
        if pc[2] < 0.0:
            continue
        evaluated += 1
        uv = project_camera(pc, kf["cam"], int(kf["dist_type"]), int(kf.get("cam_model") or 0), float(kf.get("xi") or 0.0))
        if uv is None:
            continue
        if near_image_bound(uv[0], uv[1], kf["bounds"]):
            fragile[p] = True
            continue
        if not in_image(uv[0], uv[1], kf["bounds"]):
            continue
        PO = pw - Ow
        dist = float(np.sqrt(PO @ PO))
        lo, hi = 0.8 * float(pts["min_distance"][p]), 1.2 * float(pts["max_distance"][p])
        dotn = float(PO @ np.asarray(pts["normal"][p], np.float64))
        if abs(dist - lo) <= 1e-9 * lo or abs(dist - hi) <= 1e-9 * hi or abs(dotn - 0.5 * dist) <= 1e-9 * dist:
            fragile[p] = True
            continue
        if dist < lo or dist > hi:
            continue
        if dotn < 0.5 * dist:
            continue
        level, frag = predict_scale(dist, pts["max_distance"][p], scale_factor, num_octaves)
        rad = radius * scale_factor ** level
        cands, frag2 = features_in_area(kf["kp"], order, uv[0], uv[1], rad)
        if frag or frag2:
            fragile[p] = True
            continue
        bd, bi = _best(cands, levels, kf["desc"], pts["desc"][p], level, blocked)
        if bd is not None and bd <= th_low:
            best[p] = bd
            ex = -1 if existing is None else int(existing[p])
            if ex != -1:
                if not hamming(pts["desc"][p], kf["desc"][ex]) < bd:
                    remap[p] = bi
            else:
                blocked[bi] = True; claimed[p] = bi; nmatches += 1
    return dict(claimed=claimed, remap_to=remap, best_dist=best, nmatches=nmatches, fragile=fragile, evaluated=evaluated)


def projection_comparable(ref):
    """The points are sequential, so a fragile point can change what every later point sees: the comparable points are those before the
    first fragile one."""
    f = np.flatnonzero(ref["fragile"])
    ok = np.ones(len(ref["fragile"]), bool)
    if len(f):
        ok[f[0]:] = False
    return ok
