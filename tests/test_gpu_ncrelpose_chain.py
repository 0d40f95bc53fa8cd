"""The whole loop verification of COVINS-G through the C++ facade (RelPoseSolverT::ComputeNonCentralRelPoseBatch and
computeNonCentralRelPose on the stand-in of tests/cpp/facade_ncrelpose_shim.cpp): the scene of
fivept_util.grid_scene() through the image matching, the six five-point RANSACs and the 17-point stage of every candidate in one call;
then one found covariance as the information of a loop edge in a small covgpu_pgo_solve."""
import ctypes as C

import numpy as np
import pytest

from covins_amd import backend, capi, mapdata
from tests import fivept_util as fu
from tests import ncrelpose_ref as nr
from tests import ncrelpose_util as nu

pytestmark = pytest.mark.gpu

# rp_error (the scene's bearings carry 1e-3 rad of noise: 3 px of 800), rp_error_cov, min_inliers, max_iters, cov_thres, cov_iters, cov_max_iters
NC7 = np.array([3.0, 10.0, 100.0, 600.0, 10.0, 30.0, 300.0])


@pytest.fixture(scope="module")
def chain():
    sc = fu.grid_scene()
    rng = np.random.default_rng(5)
    T_sc = np.tile(np.eye(4), (11, 1, 1))
    for k in range(11):
        T_sc[k, :3, :3] = nr.exp_so3(rng.normal(size=3) * 0.2); T_sc[k, :3, 3] = rng.normal(0.0, 0.05, 3)
    lib = nu.facade_shim()
    h = nu.shim_scene(lib, sc, T_sc)
    ip, dp, bp = C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_ubyte)
    cand = np.array([2, 5, 8], np.int32)
    found = np.zeros(3, np.uint8); status = np.zeros(3, np.int32); inl = np.zeros(3, np.int32)
    Tc = np.full((3, 4, 4), -7.0); Ts = np.full((3, 4, 4), -7.0); cov = np.zeros((3, 6, 6))
    lib.n17_batch(h, 0, 3, cand.ctypes.data_as(ip), 16.0, 20, 200, 20, 40.0, 0.8, NC7.ctypes.data_as(dp), found.ctypes.data_as(bp), status.ctypes.data_as(ip),
                  inl.ctypes.data_as(ip), Tc.ctypes.data_as(dp), Ts.ctypes.data_as(dp), cov.ctypes.data_as(dp))
    T1 = np.full((4, 4), -7.0); cov1 = np.zeros((6, 6))
    ok1 = lib.n17_single(h, 0, 2, 16.0, 20, 200, 20, 40.0, 0.8, NC7.ctypes.data_as(dp), T1.ctypes.data_as(dp), cov1.ctypes.data_as(dp))
    seeds = (lib.n17_seed(h, 0, 2), lib.n17_seed(h, 0, 5), lib.n17_seed(h, 2, 0))
    lib.n17_free(h)
    lib.n17_shutdown()
    return dict(sc=sc, T_sc=T_sc, found=found, status=status, inl=inl, Tc=Tc, Ts=Ts, cov=cov, T1=T1, cov1=cov1, ok1=ok1, seeds=seeds)


def test_true_candidate_is_found_and_bad_chains_are_not(chain):
    c, sc = chain, chain["sc"]
    print("statuses", c["status"].tolist(), "inliers", c["inl"].tolist(), "trace", float(np.trace(c["cov"][0])))
    assert c["found"].tolist() == [1, 0, 0] and c["status"].tolist() == [0, -1, -1]
    assert np.all(c["Tc"][1:] == -7.0) and np.array_equal(c["cov"][1], np.eye(6)) and np.array_equal(c["cov"][2], np.eye(6))
    T_true = sc["T_cw"][0] @ sc["T_wc"][2]
    dr, dt = nr.pose_error(c["Tc"][0][:3, :3], c["Tc"][0][:3, 3], T_true[:3, :3], T_true[:3, 3])
    Ts_true = c["T_sc"][0] @ T_true @ np.linalg.inv(c["T_sc"][2])
    sr, st = nr.pose_error(c["Ts"][0][:3, :3], c["Ts"][0][:3, 3], Ts_true[:3, :3], Ts_true[:3, 3])
    print(f"T_c1c2 against the truth: {dr:.2e} rad {dt:.2e}; T_s1s2: {sr:.2e} rad {st:.2e}")
    assert dr < 5e-3 and dt < 5e-2 and sr < 5e-3 and st < 5e-2           # bearings with 1e-3 rad of noise, points at 5-14, baselines of 1
    cov = c["cov"][0]
    assert np.array_equal(cov, cov.T) and np.linalg.eigvalsh(cov).min() > 0 and np.trace(cov) < NC7[4]
    # the reference's own signature gives the same job: same seed, same result, bit for bit
    assert c["ok1"] == 1 and np.array_equal(c["T1"], c["Tc"][0]) and np.array_equal(c["cov1"], cov)
    assert len(set(c["seeds"])) == 3


def test_found_covariance_weights_a_loop_edge(chain, tiny_map):
    """Three keyframes on a chain with two odometry edges that disagree with the loop edge 0 -> 2, whose information is the inverse of the
    sampled covariance (sqrt_info = chol(cov^-1)^T): the solve runs and the cost goes down."""
    ctx = backend.Context(0)
    p = mapdata.flatten_pgo(tiny_map, {}, mapdata.PgoParams())[0]
    Ts = chain["Ts"][0]
    meas = nr.pose7(Ts[:3, :3], Ts[:3, 3])
    L = np.linalg.cholesky(np.linalg.inv(chain["cov"][0]))
    pose = np.array([[0, 0, 0, 1.0, 0, 0, 0], [0, 0, 0, 1.0, 0.6, 0.1, 0.0], [0, 0, 0, 1.0, 1.2, 0.2, 0.0]])
    prob = capi.FlatProblem(kf_pose=pose, kf_speed_bias=p.kf_speed_bias[:3], kf_fixed=[1, 0, 0], kf_cam=[0, 0, 0], cam_extr=p.cam_extr,
                            cam_intr=p.cam_intr, cam_dist=p.cam_dist, cam_dist_type=p.cam_dist_type, edge_i=[0, 1, 0], edge_j=[1, 2, 2],
                            edge_meas=[[0, 0, 0, 1.0, 0.6, 0.1, 0.0], [0, 0, 0, 1.0, 0.6, 0.1, 0.0], list(meas)],
                            edge_sqrt_info=np.stack([np.eye(6).ravel() * 10, np.eye(6).ravel() * 10, L.T.ravel()]), edge_loss_a=[0.0, 0.0, 0.0])
    sol, res = ctx.pgo_solve(prob, backend.default_options(max_iterations=10))
    ctx.close()
    print(f"pgo with the sampled covariance on the loop edge: cost {res.initial_cost:.4e} -> {res.final_cost:.4e} in {res.iterations} iterations")
    assert res.iterations >= 1 and np.isfinite(res.final_cost) and res.final_cost < res.initial_cost
    assert np.all(np.isfinite(sol.kf_pose))
