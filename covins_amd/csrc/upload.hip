// upload.hip — HBM residency of libcovgpu's solver: validation of a problem, its upload (upload_impl: a list of steps, each
// leaving one part of DevProblem / NdDev on the device), the reset to the uploaded state and the download of the estimate;
// covgpu_upload, covgpu_upload_pgo, covgpu_download. The covisible pair lists (upload_pair_lists) also serve the second
// round of covgpu_gba_two_round (solver.hip).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "host.hpp"

using namespace covgpu;

int validate(const covgpu_problem* p, bool pgo, bool vi) {
  auto bad = [](const char* m) { g_err = std::string("invalid problem: ") + m; return COVGPU_ERR_INVALID_ARG; };
  if (!p || p->num_kf <= 0) return bad("no keyframes");
  if (p->num_cam < 0 || p->num_lm < 0 || p->num_obs < 0 || p->num_imu < 0 || p->num_edge < 0 || p->num_imu_samples < 0) return bad("negative count");
  if (!p->kf_pose || !p->kf_fixed || !p->kf_cam) return bad("NULL keyframe array");
  if (vi && !p->kf_speed_bias) return bad("NULL speed-bias array in visual-inertial mode");
  const int K = p->num_kf;
  if (!pgo) {
    if (p->num_lm > 0 && (!p->lm_pos || !p->lm_obs_ptr)) return bad("NULL landmark array");
    if (p->num_obs > 0 && (!p->obs_kf || !p->obs_uv || !p->obs_sigma)) return bad("NULL observation array");
    if (p->num_lm > 0 && (p->lm_obs_ptr[0] != 0 || p->lm_obs_ptr[p->num_lm] != p->num_obs)) return bad("lm_obs_ptr does not span the observations");
    for (int l = 0; l < p->num_lm; ++l) if (p->lm_obs_ptr[l + 1] < p->lm_obs_ptr[l]) return bad("lm_obs_ptr not monotone");
    for (int o = 0; o < p->num_obs; ++o) if (p->obs_kf[o] < 0 || p->obs_kf[o] >= K) return bad("obs_kf out of range");
    {  // one observation per (landmark, keyframe): the pair lists skip a keyframe paired with itself, so the cross terms of two observations
       // of one landmark by one keyframe would be missing from that keyframe's diagonal block of the reduced system
      std::vector<int> stamp(K, -1);
      for (int l = 0; l < p->num_lm; ++l)
        for (int o = p->lm_obs_ptr[l]; o < p->lm_obs_ptr[l + 1]; ++o) {
          if (stamp[p->obs_kf[o]] == l) return bad("landmark observed twice by one keyframe");
          stamp[p->obs_kf[o]] = l;
        }
    }
    if (p->num_cam <= 0 || !p->cam_extr || !p->cam_intr || !p->cam_dist || !p->cam_dist_type) return bad("NULL camera array");
    for (int k = 0; k < K; ++k) if (p->kf_cam[k] < 0 || p->kf_cam[k] >= p->num_cam) return bad("kf_cam out of range");
    for (int a = 0; a < p->num_cam; ++a) if (p->cam_dist_type[a] != COVGPU_DIST_RADTAN && p->cam_dist_type[a] != COVGPU_DIST_EQUIDISTANT) return bad("unknown distortion type");
    for (int a = 0; a < p->num_cam; ++a) if (const char* m = cam_check(p->cam_model, p->cam_xi, (size_t)a, kNoCamXi)) return bad(m);
    if (vi && p->num_imu > 0 && (!p->imu_kf_i || !p->imu_kf_j || !p->imu_sample_ptr || !p->imu_first)) return bad("NULL IMU array");
    if (vi && p->num_imu > 0 && p->imu_sample_ptr[p->num_imu] > 0 && !p->imu_samples) return bad("NULL IMU sample array");
    if (vi && p->num_imu > 0 && (p->imu_sample_ptr[0] != 0 || p->imu_sample_ptr[p->num_imu] != p->num_imu_samples)) return bad("imu_sample_ptr does not span the IMU samples");
    if (vi) for (int f = 0; f < p->num_imu; ++f) {
      if (p->imu_kf_i[f] < 0 || p->imu_kf_i[f] >= K || p->imu_kf_j[f] < 0 || p->imu_kf_j[f] >= K) return bad("imu keyframe out of range");
      if (p->imu_sample_ptr[f + 1] < p->imu_sample_ptr[f]) return bad("imu_sample_ptr not monotone");
    }
  }
  if (p->num_edge > 0 && (!p->edge_i || !p->edge_j || !p->edge_meas || !p->edge_sqrt_info || !p->edge_loss_a)) return bad("NULL edge array");
  for (int e = 0; e < p->num_edge; ++e)
    if (p->edge_i[e] < 0 || p->edge_i[e] >= K || p->edge_j[e] < 0 || p->edge_j[e] >= K) return bad("edge keyframe out of range");
  return COVGPU_OK;
}

void free_problem(covgpu_context* c) {
  for (void* p : c->allocs) (void)hipFree(p);
  c->allocs.clear();
  c->alloc_bytes = 0;
  c->chol.tri_clear();
  c->have = false; c->second_round = false; c->state_set = false;
  c->pgo_plan.active = false;  // its device buffers were in `allocs`
  c->d_pairkey = nullptr;
  c->nd = NdDev();
}

// The host-side values of ONE upload that live across its steps: the arguments, the environment switches (read once per upload, in
// read_switches — per upload, not per process: the tests flip them between uploads), the forms chosen, and the host lists a later step reads.
struct Upload {
  const covgpu_options* opt; const covgpu_problem* p;
  bool pgo, allow_arrow;
  // environment switches
  bool plan_timing;            // COVGPU_PLAN_TIMING
  bool pgo_nd_on, pgo_dense;   // COVGPU_PGO_ND (default on), COVGPU_PGO_DENSE=1
  bool one_front;              // COVGPU_GBA_DENSE=1
  int leaf, top_env; double frac_env; bool merge_on;   // COVGPU_ND_LEAF, COVGPU_ND_TOP, COVGPU_ND_GROUP_FRAC, COVGPU_ND_MERGE as nd_plan_build reads them (the plan cache's key)
  // forms
  bool vi, pgo_nd, use_nd;
  // host lists
  std::vector<int> ptr0;                     // {0}: the row pointer of an empty list
  std::vector<int> perm, pos_kf, chain_ptr;  // keyframe -> chain-major position, its inverse, positions of each chain
  std::vector<int> h_pair_i, h_pair_j;       // covisible pairs (positions, i > j), read back from the device for the plan
  std::vector<int> ei, ej;                   // unique loop-edge pairs (positions, i > j)
  NdHostPlan nhp;                            // the elimination tree the fronts are laid out for
  std::chrono::steady_clock::time_point tm_last;
};
static void read_switches(Upload& u) {
  u.plan_timing = plan_timing_on();
  u.pgo_nd_on = env_int("COVGPU_PGO_ND", 1) != 0;
  const char* e_pgo_dense = getenv("COVGPU_PGO_DENSE");
  u.pgo_dense = e_pgo_dense && e_pgo_dense[0] == '1';
  const char* e_dense = getenv("COVGPU_GBA_DENSE");
  u.one_front = e_dense && e_dense[0] == '1';
  u.leaf = u.one_front ? 0x3fffffff : nd_leaf_dims(0);
  // (nd_plan_build reads both on every call: a tree built under another value is another tree)
  const char *e_top = getenv("COVGPU_ND_TOP"), *e_frac = getenv("COVGPU_ND_GROUP_FRAC");
  u.top_env = e_top ? (atoi(e_top) != 0 ? 1 : 0) : -1;
  u.frac_env = e_frac ? std::max(2.0, atof(e_frac)) : 0.0;
  u.merge_on = nd_merge_enabled();
}
// dev aid (COVGPU_PLAN_TIMING=1): where the host side of an upload goes
static void tm(Upload& u, const char* what) {
  if (!u.plan_timing) return;
  const auto now = std::chrono::steady_clock::now();
  std::fprintf(stderr, "[covgpu] upload: %-28s %.2f ms\n", what, std::chrono::duration<double>(now - u.tm_last).count() * 1e3);
  u.tm_last = now;
}
static int up_or_zero(covgpu_context* c, int** dst, const std::vector<int>& h, size_t least) {
  return dev_upload(c, dst, h.empty() ? (const int*)nullptr : h.data(), std::max(h.size(), least));
}

// step 1 — leaves the sizes and switches of DevProblem (everything else zero) and, in `u`, the chain-major keyframe order and the forms
static int up_sizes_and_chains(covgpu_context* c, Upload& u) {
  const covgpu_options* opt = u.opt; const covgpu_problem* p = u.p;
  const bool pgo = u.pgo, vi = u.vi;
  std::vector<int>&perm = u.perm, &pos_kf = u.pos_kf, &chain_ptr = u.chain_ptr;
  DevProblem& P = c->P;
  std::memset(&P, 0, sizeof(P));
  P.K = p->num_kf; P.A = p->num_cam;
  P.L = pgo ? 0 : p->num_lm; P.O = pgo ? 0 : p->num_obs;
  P.I = vi ? p->num_imu : 0; P.E = p->num_edge;
  P.S = P.I ? p->imu_sample_ptr[P.I] : 0;
  P.vi = vi; P.D = vi ? 15 : 6; P.n = P.D * P.K;
  P.lm_group = covgpu_lm_group(P.O, P.L);   // lanes per landmark of the landmark-major kernels, from the mean track length
  P.npad = ((6 * P.K + kTile - 1) / kTile) * kTile;  // dense stage = pose-pose system only (k_struct.hip)
  P.N = P.n + 3 * P.L;
  // IMU chains -> chain-major keyframe order
  // pose graph on the elimination tree (round 6; COVGPU_PGO_ND=0: round 2's block-arrow scheme of k_pgo.hip on a dense matrix)
  u.pgo_nd = pgo && u.pgo_nd_on && u.allow_arrow && p->num_edge > 0 && !u.pgo_dense && !c->sharded;
  if (u.pgo_nd) build_chains_pgo(p, perm, pos_kf, chain_ptr);
  else RC(build_chains(p, vi, perm, pos_kf, chain_ptr));
  P.nchains = (int)chain_ptr.size() - 1;
  P.max_chain_len = 1;
  for (int ci = 0; ci < P.nchains; ++ci) P.max_chain_len = std::max(P.max_chain_len, chain_ptr[ci + 1] - chain_ptr[ci]);
  P.reproj_loss_a = opt->reproj_loss_a; P.gravity = opt->gravity;
  // ---- form of the reduced camera system: multifrontal fronts over a nested-dissection tree (k_front.hip) for every GBA.
  //      COVGPU_GBA_DENSE=1: the same code with ONE front = the dense system (equality tests). The dense row-major matrix
  //      Sred remains for the pose graph (k_pgo.hip builds its own block plan on it) and for covgpu_schur (reads it back).
  u.use_nd = (!pgo && u.allow_arrow) || u.pgo_nd;
  if (c->sharded && !u.use_nd) { g_err = "the agent-sharded solve is for GBA problems (covgpu_upload)"; return COVGPU_ERR_INVALID_ARG; }
  return COVGPU_OK;
}

// step 2 — leaves the uploaded state (pose0, sb0, lm0), the working and candidate states, the constant-pose flags and the camera tables
static int up_states_and_cameras(covgpu_context* c, Upload& u) {
  const covgpu_problem* p = u.p; const bool pgo = u.pgo;
  DevProblem& P = c->P;
  const size_t K = P.K;
  RC(dev_upload(c, &P.pose0, p->kf_pose, 7 * K));
  if (p->kf_speed_bias) RC(dev_upload(c, &P.sb0, p->kf_speed_bias, 9 * K)); else { RC(dev_alloc(c, &P.sb0, 9 * K)); HIPCHK(hipMemsetAsync(P.sb0, 0, 9 * K * sizeof(double), c->st)); }
  RC(dev_upload(c, &P.lm0, p->lm_pos, (size_t)3 * P.L));
  RC(dev_alloc(c, &P.pose, 7 * K)); RC(dev_alloc(c, &P.sb, 9 * K)); RC(dev_alloc(c, &P.lm, (size_t)3 * P.L));
  RC(dev_alloc(c, &P.pose_c, 7 * K)); RC(dev_alloc(c, &P.sb_c, 9 * K)); RC(dev_alloc(c, &P.lm_c, (size_t)3 * P.L));
  RC(dev_upload(c, &P.fixed, (const uint8_t*)p->kf_fixed, K));
  RC(dev_upload(c, &P.kf_cam, (const int*)p->kf_cam, K));
  RC(dev_upload(c, &P.cam_extr, p->cam_extr, (size_t)7 * P.A));
  RC(dev_upload(c, &P.cam_intr, p->cam_intr, (size_t)4 * P.A));
  RC(dev_upload(c, &P.cam_dist, p->cam_dist, (size_t)4 * P.A));
  RC(dev_upload(c, &P.cam_dist_type, (const int*)p->cam_dist_type, (size_t)P.A));
  if (!pgo && p->cam_model) {   // unified cameras: their model and xi go up and the reprojection kernels run their UNI forms (DevProblem::uni)
    std::vector<int> model(P.A);
    std::vector<double> xi(P.A, 0.0);
    for (int a = 0; a < P.A; ++a) {
      model[a] = p->cam_model[a];
      if (model[a] == COVGPU_CAM_UNIFIED) { xi[a] = p->cam_xi[a]; P.uni = 1; }
    }
    if (P.uni) {
      RC(dev_upload(c, &P.cam_model, (const int*)model.data(), (size_t)P.A));
      RC(dev_upload(c, &P.cam_xi, (const double*)xi.data(), (size_t)P.A));
      HIPCHK(hipStreamSynchronize(c->st));   // (the host vectors die here)
    }
  }
  return COVGPU_OK;
}

// step 3 — leaves the observation stream as SoA (obs_*, lm_obs_ptr) and the keyframe-major observation lists (kf_obs_ptr, kf_obs_idx).
// The interleaved keypoints are split, the landmark index of every observation is filled and the
// keyframe-major lists are built ON THE DEVICE (k_pairs.hip) — three host loops over O and two more uploads before (12 of the 18 ms of an
// upload of the 5-agent map)
static int up_observations(covgpu_context* c, Upload& u) {
  const covgpu_problem* p = u.p;
  DevProblem& P = c->P;
  RC(dev_upload(c, &P.lm_obs_ptr, P.L ? (const int*)p->lm_obs_ptr : u.ptr0.data(), (size_t)P.L + 1));
  RC(dev_upload(c, &P.obs_kf, (const int*)p->obs_kf, (size_t)P.O));
  RC(dev_upload(c, &P.obs_sigma, p->obs_sigma, (size_t)P.O));
  RC(dev_alloc(c, &P.obs_lm, (size_t)P.O)); RC(dev_alloc(c, &P.obs_u, (size_t)P.O)); RC(dev_alloc(c, &P.obs_v, (size_t)P.O));
  RC(dev_alloc(c, &P.kf_obs_ptr, (size_t)P.K + 1)); RC(dev_alloc(c, &P.kf_obs_idx, (size_t)P.O));
  {
    DeviceScratch U(c->st);
    double* d_uv = nullptr; int* d_iota = nullptr;
    HIPCHK(U.upload(&d_uv, p->obs_uv, (size_t)2 * P.O)); HIPCHK(U.alloc(&d_iota, (size_t)P.O));
    launch_obs_unpack(P.L, P.O, P.lm_obs_ptr, d_uv, P.obs_lm, P.obs_u, P.obs_v, d_iota, c->st);
    const bool ok = build_kf_lists_device(P.O, P.K, P.obs_kf, d_iota, P.kf_obs_ptr, P.kf_obs_idx, c->st);   // (ends with a stream synchronisation)
    (void)hipStreamSynchronize(c->st);
    if (!ok) { g_err = "upload: device-side observation lists failed (allocation)"; return COVGPU_ERR_OUT_OF_MEMORY; }
  }
  return COVGPU_OK;
}

// Covisible pairs of the resident observation stream under the keys of c->d_pairkey (i > j in chain-major positions, free keyframes only —
// fixed keyframes carry no pose block) with, per pair, the observations of every common landmark in landmark order: built on the device
// (k_pairs.hip: key emission + one stable radix sort + run-length encoding). Leaves P.npairs, P.pair_ptr / _i / _j / _oa / _ob (owned by
// the context), P.pair_order and the per-keyframe observation records of launch_kobs_build. All of it is enqueued: the caller synchronises.
// Two callers that differ on purpose:
//   an upload (second_round = false) counts the lists into alloc_bytes, starts the read-back of the pairs into host_i / host_j (for the plan)
//   and allocates the per-observation records (obsZ, lmRT, kobs, kobs_lm, obs_zpos) between the lists and pair_order;
//   the second round of covgpu_gba_two_round (second_round = true) keeps those records, does NOT count the new lists into alloc_bytes
//   (covgpu_get_layout keeps reporting the first round's footprint) and starts from P.pair_order = nullptr, so that no pairs leave no order.
int upload_pair_lists(covgpu_context* c, bool second_round, std::vector<int>* host_i, std::vector<int>* host_j) {
  DevProblem& P = c->P;
  PairLists pl;
  if (!build_pairs_device(P.L, P.K, P.lm_obs_ptr, P.obs_kf, c->d_pairkey, true, c->st, pl)) {
    g_err = second_round ? "covisible pair lists: device allocation failed" : "covisible pair lists: device allocation failed (or more than 2^31 entries)";
    return COVGPU_ERR_OUT_OF_MEMORY;
  }
  for (int* q : {pl.pair_ptr, pl.pair_i, pl.pair_j, pl.pair_oa, pl.pair_ob}) if (q) c->allocs.push_back(q);
  if (!second_round) c->alloc_bytes += ((size_t)pl.npairs * 3 + 1 + 2 * pl.nent) * sizeof(int);
  P.npairs = pl.npairs; P.pair_ptr = pl.pair_ptr; P.pair_i = pl.pair_i; P.pair_j = pl.pair_j; P.pair_oa = pl.pair_oa; P.pair_ob = pl.pair_ob;
  if (second_round) P.pair_order = nullptr;
  else {
    host_i->resize(P.npairs); host_j->resize(P.npairs);
    if (P.npairs) {
      HIPCHK(hipMemcpyAsync(host_i->data(), P.pair_i, (size_t)P.npairs * sizeof(int), hipMemcpyDeviceToHost, c->st));
      HIPCHK(hipMemcpyAsync(host_j->data(), P.pair_j, (size_t)P.npairs * sizeof(int), hipMemcpyDeviceToHost, c->st));
    }
    RC(dev_alloc(c, &P.obsZ, (size_t)18 * P.O)); RC(dev_alloc(c, &P.lmRT, (size_t)9 * P.L));
    RC(dev_alloc(c, &P.kobs, (size_t)3 * P.O)); RC(dev_alloc(c, &P.kobs_lm, (size_t)P.O)); RC(dev_alloc(c, &P.obs_zpos, (size_t)P.O));
  }
  if (P.npairs) RC(dev_alloc(c, &P.pair_order, pair_order_slots(P.npairs)));
  launch_kobs_build(P, P.pair_oa, P.pair_ob, pl.nent, c->st);
  return COVGPU_OK;
}

// step 4 — leaves the pair keys (c->d_pairkey, c->h_perm), the covisible pair lists (upload_pair_lists), cost_part, and in `u` the pairs for the plan
static int up_covisible_pairs(covgpu_context* c, Upload& u) {
  DevProblem& P = c->P;
  std::vector<int> key(P.K);
  for (int k = 0; k < P.K; ++k) key[k] = u.p->kf_fixed[k] ? -1 : u.perm[k];
  int* d_key = nullptr;
  RC(dev_upload(c, &d_key, key.data(), key.size()));
  c->d_pairkey = d_key; c->h_perm = u.perm;
  RC(upload_pair_lists(c, false, &u.h_pair_i, &u.h_pair_j));
  RC(dev_alloc(c, &P.cost_part, (size_t)(P.L / 4 + 64)));
  HIPCHK(hipStreamSynchronize(c->st));
  return COVGPU_OK;
}

// step 5 — leaves the IMU factors, their samples and per-factor calibration, and the preintegration buffers
static int up_imu(covgpu_context* c, Upload& u) {
  const covgpu_options* opt = u.opt; const covgpu_problem* p = u.p;
  DevProblem& P = c->P;
  RC(dev_upload(c, &P.imu_i, (const int*)p->imu_kf_i, (size_t)P.I));
  RC(dev_upload(c, &P.imu_j, (const int*)p->imu_kf_j, (size_t)P.I));
  RC(dev_upload(c, &P.imu_ptr, P.I ? (const int*)p->imu_sample_ptr : u.ptr0.data(), (size_t)P.I + 1));
  RC(dev_upload(c, &P.imu_samples, p->imu_samples, (size_t)7 * P.S));
  RC(dev_upload(c, &P.imu_first, p->imu_first, (size_t)6 * P.I));
  {  // per-factor calibration; the options' single set is the fallback for callers that have one IMU model only
    std::vector<double> nz((size_t)5 * P.I);
    for (int f = 0; f < P.I; ++f) {
      double* r = &nz[(size_t)5 * f];
      if (p->imu_noise) std::memcpy(r, p->imu_noise + (size_t)5 * f, 5 * sizeof(double));
      else { r[0] = opt->sigma_a; r[1] = opt->sigma_g; r[2] = opt->sigma_aw; r[3] = opt->sigma_gw; r[4] = opt->gravity; }
      if (!(r[0] > 0 && r[1] > 0 && r[2] > 0 && r[3] > 0) || !(r[4] >= 9.0)) {  // keyframe_base.cpp:51-55 rejects g < 9
        g_err = "invalid problem: IMU noise must be positive and gravity >= 9 (factor " + std::to_string(f) + ")";
        return COVGPU_ERR_INVALID_ARG;
      }
    }
    RC(dev_upload(c, &P.imu_noise, nz.data(), nz.size()));
    HIPCHK(hipStreamSynchronize(c->st));
  }
  RC(dev_alloc(c, &P.pre_delta, (size_t)11 * P.I)); RC(dev_alloc(c, &P.pre_J, (size_t)225 * P.I));
  RC(dev_alloc(c, &P.pre_P, (size_t)225 * P.I)); RC(dev_alloc(c, &P.pre_W, (size_t)225 * P.I));
  RC(dev_alloc(c, &P.pre_bias, (size_t)6 * P.I));
  RC(dev_alloc(c, &P.imu_Jw, (size_t)450 * P.I));   // (3.6 KB per factor: 7.9 MB on the 5-agent map, 72 MB on the 12-agent map)
  return COVGPU_OK;
}

// step 6 — leaves the loop-edge tables. (Their keyframe and pair lists follow the system vectors: up_edge_lists. The order of the
// device allocations is part of what an upload promises: covgpu_get_layout and the results depend on it.)
static int up_edges(covgpu_context* c, Upload& u) {
  const covgpu_problem* p = u.p;
  DevProblem& P = c->P;
  RC(dev_upload(c, &P.edge_i, (const int*)p->edge_i, (size_t)P.E));
  RC(dev_upload(c, &P.edge_j, (const int*)p->edge_j, (size_t)P.E));
  RC(dev_upload(c, &P.edge_meas, p->edge_meas, (size_t)7 * P.E));
  RC(dev_upload(c, &P.edge_sqrt_info, p->edge_sqrt_info, (size_t)36 * P.E));
  RC(dev_upload(c, &P.edge_loss_a, p->edge_loss_a, (size_t)P.E));
  return COVGPU_OK;
}

// step 7 — leaves the keyframe order tables, the blocks and vectors of the linear system and of the step, the scalars, and the partial-sum slots
static int up_system_vectors(covgpu_context* c, Upload& u) {
  const bool vi = u.vi;
  const std::vector<int>&perm = u.perm, &pos_kf = u.pos_kf, &chain_ptr = u.chain_ptr;
  DevProblem& P = c->P;
  const size_t K = P.K;
  std::vector<int> chain_end(P.K);
  for (int ch = 0; ch < P.nchains; ++ch)
    for (int q = chain_ptr[ch]; q < chain_ptr[ch + 1]; ++q) chain_end[q] = chain_ptr[ch + 1];
  RC(dev_upload(c, &P.perm, perm.data(), K)); RC(dev_upload(c, &P.pos_kf, pos_kf.data(), K));
  RC(dev_upload(c, &P.chain_ptr, chain_ptr.data(), chain_ptr.size()));
  RC(dev_upload(c, &P.pos_chain_end, chain_end.data(), K));
  RC(dev_alloc(c, &P.bred, (size_t)P.n));
  RC(dev_alloc(c, &P.bp, (size_t)2 * P.npad));
  const size_t Kv = vi ? K : 0;
  RC(dev_alloc(c, &P.Ad, 81 * Kv)); RC(dev_alloc(c, &P.Ae, 81 * Kv));
  RC(dev_alloc(c, &P.Bp, 54 * Kv)); RC(dev_alloc(c, &P.Bs, 54 * Kv)); RC(dev_alloc(c, &P.Bn, 54 * Kv));
  {
    std::vector<int> cbeg(P.K);
    for (int ch = 0; ch < P.nchains; ++ch) for (int q = chain_ptr[ch]; q < chain_ptr[ch + 1]; ++q) cbeg[q] = chain_ptr[ch];
    RC(dev_upload(c, &P.pos_chain_begin, cbeg.data(), cbeg.size()));
    HIPCHK(hipStreamSynchronize(c->st));
  }
  RC(dev_alloc(c, &P.grad, (size_t)P.N)); RC(dev_alloc(c, &P.hdiag, (size_t)P.N));
  RC(dev_alloc(c, &P.HllInv, (size_t)6 * P.L));
  RC(dev_alloc(c, &P.gn, (size_t)P.N)); RC(dev_alloc(c, &P.step, (size_t)P.N)); RC(dev_alloc(c, &P.vtmp, (size_t)P.N));
  // (sharded solve: the entries of other ranks' unknowns are never written — they must read as 0, not as what hipMalloc left)
  HIPCHK(hipMemsetAsync(P.gn, 0, (size_t)P.N * sizeof(double), c->st)); HIPCHK(hipMemsetAsync(P.step, 0, (size_t)P.N * sizeof(double), c->st));
  HIPCHK(hipMemsetAsync(P.vtmp, 0, (size_t)P.N * sizeof(double), c->st));
  RC(dev_alloc(c, &P.scal, (size_t)SC_COUNT)); RC(dev_alloc(c, &P.flag, (size_t)4));
  RC(dev_alloc(c, &P.tr, (size_t)TR_COUNT));
  P.scal_r = P.scal; P.flag_r = P.flag;  // what the device-side trust region reads (sharded solve: the all-reduced copies, set below)
  // deterministic reductions / scatters
  P.part_imu = 8192; P.part_edge = P.part_imu + ((P.I + 3) / 4) * 4; P.part_vec = P.part_edge + (P.E + 63) / 64;
  P.part_n = P.part_vec + 8192;
  RC(dev_alloc(c, &P.part, (size_t)SC_COUNT * P.part_n));
  HIPCHK(hipMemsetAsync(P.part, 0, (size_t)SC_COUNT * P.part_n * sizeof(double), c->st));
  RC(dev_alloc(c, &P.imuAd, 2 * 81 * Kv)); RC(dev_alloc(c, &P.imuBs, 2 * 54 * Kv));
  RC(dev_alloc(c, &P.imuCd, 3 * 36 * Kv)); RC(dev_alloc(c, &P.imuG, 2 * 30 * Kv));
  RC(dev_alloc(c, &P.edgeOut, (size_t)132 * P.E));
  return COVGPU_OK;
}

// step 8 — leaves keyframe -> incident edges (ascending edge index) and unique pose pairs -> edges, c->edge_beside_imu, and in `u` the edge pairs for the plan
static int up_edge_lists(covgpu_context* c, Upload& u) {
  const covgpu_problem* p = u.p;
  const std::vector<int>& perm = u.perm;
  std::vector<int>&ei = u.ei, &ej = u.ej;
  DevProblem& P = c->P;
  std::vector<int> kptr(P.K + 1, 0), kent(2 * (size_t)P.E);
  for (int e = 0; e < P.E; ++e) {
    if (p->edge_i[e] == p->edge_j[e]) { g_err = "invalid problem: self edge"; return COVGPU_ERR_INVALID_ARG; }
    kptr[p->edge_i[e] + 1]++; kptr[p->edge_j[e] + 1]++;
  }
  for (int k = 0; k < P.K; ++k) kptr[k + 1] += kptr[k];
  { std::vector<int> cur(kptr.begin(), kptr.end() - 1);
    for (int e = 0; e < P.E; ++e) { kent[cur[p->edge_i[e]]++] = 2 * e; kent[cur[p->edge_j[e]]++] = 2 * e + 1; } }
  struct PE { int i, j, ent; };
  std::vector<PE> pe(P.E);
  for (int e = 0; e < P.E; ++e) {
    const int a = perm[p->edge_i[e]], b = perm[p->edge_j[e]];
    pe[e] = (a > b) ? PE{a, b, 2 * e} : PE{b, a, 2 * e + 1};
  }
  std::stable_sort(pe.begin(), pe.end(), [](const PE& x, const PE& y) { return x.i != y.i ? x.i < y.i : x.j < y.j; });
  std::vector<int> eptr, eent(P.E);
  for (int q = 0; q < P.E; ++q) {
    if (q == 0 || pe[q].i != pe[q - 1].i || pe[q].j != pe[q - 1].j) { eptr.push_back(q); ei.push_back(pe[q].i); ej.push_back(pe[q].j); }
    eent[q] = pe[q].ent;
  }
  eptr.push_back(P.E);
  P.nepairs = (int)ei.size();
  c->edge_beside_imu = false;
  for (size_t q = 0; q < ei.size(); ++q) if (ei[q] - ej[q] == 1) c->edge_beside_imu = true;
  RC(dev_upload(c, &P.kf_edge_ptr, kptr.data(), kptr.size())); RC(dev_upload(c, &P.kf_edge_ent, kent.data(), kent.size()));
  RC(dev_upload(c, &P.epair_ptr, eptr.data(), eptr.size())); RC(dev_upload(c, &P.epair_i, ei.data(), ei.size()));
  RC(dev_upload(c, &P.epair_j, ej.data(), ej.size())); RC(dev_upload(c, &P.epair_ent, eent.data(), eent.size()));
  HIPCHK(hipStreamSynchronize(c->st));
  return COVGPU_OK;
}

// step 9 (host only) — leaves in u.nhp the elimination tree of this problem: the shard plan in this sub-problem's positions, the
// previous upload's tree (plan cache), or a new one
static int up_choose_plan(covgpu_context* c, Upload& u) {
  const bool pgo = u.pgo, vi = u.vi;
  const int leaf = u.leaf, top_env = u.top_env; const double frac_env = u.frac_env;
  const std::vector<int>&perm = u.perm, &pos_kf = u.pos_kf, &chain_ptr = u.chain_ptr, &h_pair_i = u.h_pair_i, &h_pair_j = u.h_pair_j, &ei = u.ei, &ej = u.ej;
  NdHostPlan& nhp = u.nhp;
  const DevProblem& P = c->P;
  if (c->sharded) {
    // the global plan (covgpu_shard_plan on the FULL problem, the same on every rank), from IR keyframes to this
    // sub-problem's chain positions; this rank holds the fronts of its subtrees and of the replicated top nodes
    if ((int)c->shard_plan->K != P.K || (c->shard_plan->vi != 0) != vi) { g_err = "sharded solve: the problem does not match the shard plan"; return COVGPU_ERR_INVALID_ARG; }
    nhp = *c->shard_plan;
    std::vector<int> to_pos(2 * (size_t)P.K);
    for (int k = 0; k < P.K; ++k) { to_pos[2 * k] = 2 * perm[k]; to_pos[2 * k + 1] = 2 * perm[k] + 1; }
    nd_plan_remap(nhp, to_pos);
  } else {
    // The plan of the previous upload serves again if this problem has the same keyframes in the same chain positions and its
    // couplings are a SUBSET of the ones the plan was built for (a tree stays a valid elimination order when couplings
    // disappear: the second round of a GlobalBundleAdjustment call is the first one minus the erased observations).
    std::vector<uint64_t> keys(h_pair_i.size() + ei.size());
    {
      std::vector<uint64_t> ka(h_pair_i.size()), kb(ei.size());
      for (size_t q = 0; q < ka.size(); ++q) ka[q] = ((uint64_t)(uint32_t)h_pair_i[q] << 32) | (uint32_t)h_pair_j[q];
      for (size_t q = 0; q < kb.size(); ++q) kb[q] = ((uint64_t)(uint32_t)ei[q] << 32) | (uint32_t)ej[q];
      if (!std::is_sorted(ka.begin(), ka.end())) std::sort(ka.begin(), ka.end());
      std::merge(ka.begin(), ka.end(), kb.begin(), kb.end(), keys.begin());
      keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    }
    PlanCache& pc = c->plan_cache;
    const bool merge_env = u.merge_on && !pgo;   // (the pose graph is never merged)
    const bool hit = pc.valid && pc.K == P.K && pc.vi == vi && pc.leaf == leaf && pc.top_env == top_env && pc.frac_env == frac_env && pc.merge_env == merge_env && pc.chain_ptr == chain_ptr && pc.pos_kf == pos_kf &&
                     std::includes(pc.keys.begin(), pc.keys.end(), keys.begin(), keys.end());
    if (hit) nhp = pc.hp;
    else {
      if (!nd_plan_build(P.K, vi, P.nchains, chain_ptr.data(), (int)h_pair_i.size(), h_pair_i.data(), h_pair_j.data(), P.nepairs, ei.data(), ej.data(), leaf, nhp, -1, !pgo)) {
        g_err = "nested-dissection plan: a coupling joins two branches"; return COVGPU_ERR_INVALID_ARG;
      }
      pc.valid = true; pc.K = P.K; pc.vi = vi; pc.leaf = leaf; pc.top_env = top_env; pc.frac_env = frac_env; pc.merge_env = merge_env; pc.chain_ptr = chain_ptr; pc.pos_kf = pos_kf; pc.keys.swap(keys); pc.hp = nhp;
    }
  }
  if (nhp.maxdepth > 64) { g_err = "nested-dissection plan: tree deeper than 64 levels"; return COVGPU_ERR_INVALID_ARG; }
  return COVGPU_OK;
}

// step 10 — leaves the front tables of the tree (NdDev, the nd_* fields of DevProblem), the fronts with their right-hand sides, and the
// tiles' inverses: allocated and initialised (launch_nd_init)
static int up_fronts(covgpu_context* c, Upload& u) {
  const NdHostPlan& nhp = u.nhp;
  DevProblem& P = c->P;
  NdDev& nd = c->nd;
  nd_tables(nhp, u.pos_kf.data(), P.D, c->rank, nd);
  tm(u, "front tables");
  P.nd = 1; P.nd_nnodes = nd.nnodes; P.nd_nlev = (int)nd.lev.size(); P.nd_maxd = nhp.maxdepth;
  RC(dev_upload(c, &P.nd_vnode, nd.h_vnode.data(), nd.h_vnode.size())); RC(dev_upload(c, &P.nd_voff, nd.h_voff.data(), nd.h_voff.size()));
  RC(dev_upload(c, &P.nd_vord, nd.h_vord.data(), nd.h_vord.size()));
  if (c->sharded) RC(dev_upload(c, &P.nd_vown, nd.h_vown.data(), nd.h_vown.size()));
  RC(dev_upload(c, &P.nd_ndepth, nd.h_ndepth.data(), nd.h_ndepth.size())); RC(dev_upload(c, &P.nd_nI, nd.h_nI.data(), nd.h_nI.size()));
  RC(dev_upload(c, &P.nd_ntab, nd.h_ntab.data(), nd.h_ntab.size()));
  RC(dev_upload(c, &P.nd_abase, nd.h_abase.data(), nd.h_abase.size())); RC(dev_upload(c, &P.nd_fidx, nd.h_fidx.data(), nd.h_fidx.size()));
  RC(dev_upload(c, &nd.own_dims, nd.h_own_dims.data(), nd.h_own_dims.size())); RC(dev_upload(c, &nd.st_dims, nd.h_st_dims.data(), nd.h_st_dims.size()));
  RC(dev_upload(c, &nd.own_g, nd.h_own_g.data(), nd.h_own_g.size())); RC(dev_upload(c, &nd.st_g, nd.h_st_g.data(), nd.h_st_g.size()));
  RC(dev_upload(c, &nd.gidx, nd.h_gidx.data(), nd.h_gidx.size()));
  RC(dev_upload(c, &nd.tree_fill, nd.h_tree_fill.empty() ? (const int*)nullptr : nd.h_tree_fill.data(), std::max<size_t>(nd.h_tree_fill.size(), 1)));
  RC(dev_upload(c, &nd.inv_off, nd.h_inv_off.data(), nd.h_inv_off.size())); RC(dev_upload(c, &nd.inv, nd.h_inv.data(), nd.h_inv.size()));
  RC(dev_upload(c, &nd.rhs_node, nd.h_rhs_node.data(), nd.h_rhs_node.size()));
  RC(up_or_zero(c, &nd.extw, nd.h_extw, 8)); RC(up_or_zero(c, &nd.extc, nd.h_extc, 6)); RC(up_or_zero(c, &nd.extc2, nd.h_extc2, 6));
  RC(up_or_zero(c, &nd.extr, nd.h_extr, kExtRec));
  RC(dev_upload(c, &nd.bb_off, nd.h_bb_off.data(), nd.h_bb_off.size()));
  RC(dev_upload(c, &nd.bb, nd.h_bb.data(), std::max<size_t>(nd.h_bb.size(), 1)));
  RC(dev_upload(c, &nd.top_var, nd.h_top_var.data(), nd.h_top_var.size())); RC(dev_upload(c, &nd.top_r, nd.h_top_r.data(), nd.h_top_r.size()));
  RC(dev_upload(c, &nd.top_g, nd.h_top_g.data(), nd.h_top_g.size()));
  for (NdLevel& L : nd.lev) { RC(dev_upload(c, &L.live, L.live_h.data(), L.live_h.size())); RC(dev_upload(c, &L.plist, L.plist_h.data(), L.plist_h.size())); }
  // one allocation: [subtree fronts | top fronts][top right-hand sides | grad, hdiag of the top unknowns | subtree right-hand
  // sides] — what a sharded solve all-reduces is one contiguous range of it
  RC(dev_alloc(c, &P.nd_M, nd.M_elems + nd.rhs_elems));
  P.nd_rhs = P.nd_M + nd.M_elems;
  RC(dev_alloc(c, &P.nd_Linv, nd.linv_elems));
  RC(dev_alloc(c, &P.nd_dummy, (size_t)64));
  launch_nd_init(P, nd, c->st);
  c->chol.tri_clear();   // the live-tile lists of the bulk updates belong to the previous problem
  HIPCHK(hipStreamSynchronize(c->st));
  return COVGPU_OK;
}

// step 11 (sharded solve only) — leaves the trust-region weights of the unknowns (P.vw), the scratch of the scalar all-reduce, the tables and
// buffers of the top's exchange (replicated or distributed), and the all-reduced copies of scalars and flag (P.scal_r, P.flag_r)
static int up_sharded_top(covgpu_context* c, Upload& u) {
  const std::vector<int>& perm = u.perm;
  DevProblem& P = c->P;
  NdDev& nd = c->nd;
  P.shard = 1;
  // weight of every unknown in the trust-region norms: counted by exactly one rank (own subtree: here; top: rank 0)
  std::vector<double> vw((size_t)P.N, 1.0);  // landmarks: all mine (the sub-problem holds this rank's landmarks only)
  for (int k = 0; k < P.K; ++k) {
    const int op = nd.h_vown[2 * perm[k]], os = nd.h_vown[2 * perm[k] + 1];
    const double wp = op == 1 ? 1.0 : (op == 2 && c->rank == 0 ? 1.0 : 0.0), ws = os == 1 ? 1.0 : (os == 2 && c->rank == 0 ? 1.0 : 0.0);
    for (int r = 0; r < 6; ++r) vw[(size_t)P.D * k + r] = wp;
    for (int r = 6; r < P.D; ++r) vw[(size_t)P.D * k + r] = ws;
  }
  RC(dev_upload(c, &P.vw, vw.data(), vw.size()));
  RC(dev_alloc(c, &c->d_red, (size_t)SC_COUNT + 2 * (size_t)c->world));
  if (nd.dist) {   // distributed top (shard policy 1): per-panel exchange entries, owned trailing-update tiles, one reduce buffer for the largest panel
    RC(up_or_zero(c, &nd.dist_ent, nd.h_dist_ent, 4)); RC(up_or_zero(c, &nd.dist_tri, nd.h_dist_tri, 1));
    RC(dev_alloc(c, &nd.dist_buf, std::max<size_t>(nd.dist_buf_elems, 1)));
    for (NdLevel& L : nd.lev) {
      L.dt_dev.assign(L.dt_cnt.size(), nullptr);
      for (size_t q = 0; q < L.dt_cnt.size(); ++q) if (L.dt_cnt[q] > 0) L.dt_dev[q] = nd.dist_tri + L.dt_first[q];
    }
  } else {
    RC(dev_upload(c, &nd.top_tiles, nd.h_top_tiles.data(), nd.h_top_tiles.size()));
    RC(dev_alloc(c, &nd.top_pack, (size_t)nd.n_top_tiles * kTile * kTile + nd.rhs_top + 2 * (size_t)nd.ntop));
  }
  RC(dev_alloc(c, &P.scal_r, (size_t)SC_COUNT)); RC(dev_alloc(c, &P.flag_r, (size_t)4));
  return COVGPU_OK;
}

static void print_plan(const covgpu_context* c, const Upload& u) {
  const NdDev& nd = c->nd;
  int panels = 0;
  for (const NdLevel& L : nd.lev) panels += L.nI / 256;
  std::printf("[covgpu] multifrontal plan: %d fronts in %d levels (%d serial 256-column panels), %.2e flops, fronts %.2f GB%s\n", nd.nnodes,
              (int)nd.lev.size(), panels, u.nhp.flops, nd.M_elems * 8e-9, c->sharded ? " (this rank's share)" : "");
}

// step 12 (pose graph off the elimination tree) — leaves the block-arrow plan of the pose-graph solve (k_pgo.hip) in c->pgo_plan, if the
// graph has that shape; COVGPU_PGO_DENSE=1 keeps the plain dense solve
static int up_pgo_arrow_plan(covgpu_context* c, Upload& u) {
  const covgpu_problem* p = u.p;
  const DevProblem& P = c->P;
  PgoHostPlan hp;
  if (u.pgo_dense || !pgo_plan_analyse(P.K, P.E, p->edge_i, p->edge_j, hp)) return COVGPU_OK;
  PgoPlan& plan = c->pgo_plan;
  std::vector<int> idxb;
  for (int kf : hp.border_kf) for (int r = 0; r < 6; ++r) idxb.push_back(6 * kf + r);
  plan.nb = (((int)idxb.size() + kTile - 1) / kTile) * kTile;
  if (plan.nb == 0) plan.nb = kTile;
  idxb.resize(plan.nb, -1);
  RC(dev_upload(c, &plan.idx_b, idxb.data(), idxb.size()));
  RC(dev_alloc(c, &plan.Sb, (size_t)plan.nb * plan.nb)); RC(dev_alloc(c, &plan.rhs_b, (size_t)2 * plan.nb));
  RC(dev_alloc(c, &plan.Linv_b, (size_t)plan.nb * kTile));
  plan.nblk = (int)hp.block_kf.size();
  size_t big = 0;
  for (auto& bk : hp.block_kf) big = std::max(big, bk.size());
  plan.nIpad = (((int)big * 6 + 2 * kTile - 1) / (2 * kTile)) * (2 * kTile);  // whole big panels: tstop is even
  plan.ntot = plan.nIpad + plan.nb;
  std::vector<int> idx((size_t)plan.nblk * plan.ntot, -1);
  for (int a = 0; a < plan.nblk; ++a) {
    int* row = idx.data() + (size_t)a * plan.ntot;
    int q = 0;
    for (int kf : hp.block_kf[a]) for (int r = 0; r < 6; ++r) row[q++] = 6 * kf + r;
    std::copy(idxb.begin(), idxb.end(), row + plan.nIpad);
  }
  RC(dev_upload(c, &plan.idx, idx.data(), idx.size()));
  RC(dev_alloc(c, &plan.M, (size_t)plan.nblk * plan.ntot * plan.ntot)); RC(dev_alloc(c, &plan.rhs, (size_t)plan.nblk * 2 * plan.ntot));
  RC(dev_alloc(c, &plan.Linv, (size_t)plan.nblk * plan.nIpad * kTile));
  plan.active = true;
  return COVGPU_OK;
}

// The upload of a problem: the steps above, in the order of their device operations (allocations, copies, launches, synchronisations),
// which covgpu_get_layout, the allocation order and the results depend on.
int upload_impl(covgpu_context* c, const covgpu_options* opt, const covgpu_problem* p, bool pgo, bool allow_arrow) {
  HIPCHK(hipSetDevice(c->device));
  Upload u;
  u.opt = opt; u.p = p; u.pgo = pgo; u.allow_arrow = allow_arrow;
  u.vi = !pgo && !opt->visual_only;
  u.ptr0.assign(1, 0);
  read_switches(u);
  u.tm_last = std::chrono::steady_clock::now();
  RC(validate(p, pgo, u.vi));
  free_problem(c);
  c->chol.forms = FormCensus();   // the census counts from the last upload
  DevProblem& P = c->P;
  RC(up_sizes_and_chains(c, u));
  RC(up_states_and_cameras(c, u));
  RC(up_observations(c, u));
  tm(u, "validate, chains, states, observation stream");
  RC(up_covisible_pairs(c, u));
  tm(u, "covisible pair lists");
  RC(up_imu(c, u));
  RC(up_edges(c, u));
  RC(up_system_vectors(c, u));
  RC(up_edge_lists(c, u));
  tm(u, "IMU, edges, vectors");
  if (u.use_nd) {
    RC(up_choose_plan(c, u));
    tm(u, "nested-dissection plan");
    RC(up_fronts(c, u));
    tm(u, "table upload, front allocation");
    if (c->sharded) RC(up_sharded_top(c, u));
    HIPCHK(hipStreamSynchronize(c->st));
    if (opt->verbose) print_plan(c, u);
  } else {
    // the dense row-major system: the pose graph off the tree (k_pgo.hip builds its block plan on it) and covgpu_schur (reads it back)
    RC(dev_alloc(c, &P.Sred, (size_t)P.npad * P.npad));
    RC(dev_alloc(c, &P.Linv, (size_t)(P.npad / kTile) * kTile * kTile));
  }
  if (pgo && P.E && !u.pgo_nd) RC(up_pgo_arrow_plan(c, u));
  HIPCHK(hipMemsetAsync(P.scal, 0, SC_COUNT * sizeof(double), c->st));
  HIPCHK(hipMemsetAsync(P.flag, 0, 4 * sizeof(int), c->st));
  HIPCHK(hipStreamSynchronize(c->st));  // host staging vectors go out of scope
  c->have = true; c->pgo = pgo;
  return COVGPU_OK;
}

int reset_state(covgpu_context* c) {
  DevProblem& P = c->P;
  HIPCHK(hipMemcpyAsync(P.pose, P.pose0, (size_t)7 * P.K * sizeof(double), hipMemcpyDeviceToDevice, c->st));
  HIPCHK(hipMemcpyAsync(P.sb, P.sb0, (size_t)9 * P.K * sizeof(double), hipMemcpyDeviceToDevice, c->st));
  if (P.L) HIPCHK(hipMemcpyAsync(P.lm, P.lm0, (size_t)3 * P.L * sizeof(double), hipMemcpyDeviceToDevice, c->st));
  c->state_set = true;
  return COVGPU_OK;
}

// poses and speed-bias of the resident estimate -> the caller's arrays (enqueued: the caller synchronises)
int download_states(covgpu_context* c, covgpu_problem* p) {
  const DevProblem& P = c->P;
  HIPCHK(hipMemcpyAsync(p->kf_pose, P.pose, (size_t)7 * P.K * sizeof(double), hipMemcpyDeviceToHost, c->st));
  if (P.vi && p->kf_speed_bias) HIPCHK(hipMemcpyAsync(p->kf_speed_bias, P.sb, (size_t)9 * P.K * sizeof(double), hipMemcpyDeviceToHost, c->st));
  return COVGPU_OK;
}
int download_impl(covgpu_context* c, covgpu_problem* p) {
  if (!c->have) { g_err = "no problem uploaded"; return COVGPU_ERR_INVALID_ARG; }
  const DevProblem& P = c->P;
  RC(download_states(c, p));
  if (P.L) HIPCHK(hipMemcpyAsync(p->lm_pos, P.lm, (size_t)3 * P.L * sizeof(double), hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  return COVGPU_OK;
}

extern "C" int covgpu_upload(covgpu_context* c, const covgpu_options* opt, const covgpu_problem* p) { return guarded([&] { return upload_impl(c, opt, p, false); }); }
extern "C" int covgpu_upload_pgo(covgpu_context* c, const covgpu_options* opt, const covgpu_problem* p) { return guarded([&] { return upload_impl(c, opt, p, true); }); }
extern "C" int covgpu_download(covgpu_context* c, covgpu_problem* p) { return guarded([&] { return download_impl(c, p); }); }
