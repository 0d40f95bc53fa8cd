// solver.hip — the solve of libcovgpu: the context (create, destroy, options, profile, layout), one trust-region iteration as
// enqueued work (enqueue_*), its end on the host (end_iteration), the trust-region driver (solve_impl_dev, solve_any) and the
// extern "C" entry points of the GBA / PGO solves, both rounds of a GlobalBundleAdjustment call, the outlier pass and covisibility.
// Around it, all on host.hpp: upload.hip (HBM residency), plan_api.hip (plans), shard.hip (collectives), multi.hip (in-process
// multi-GPU call), probe_api.hip (test entry points); the stateless batch front end is batch.hip.
//
// This is the thin extern "C" shim of BASELINE.json's north_star. It replaces what ceres::Solve does between
// optimization_be.cpp:560-567 (GBA), :257-265 (GBA outlier round) and :1024-1031 (PGO): only scalars cross
// PCIe inside the loop (three small read-backs per trust-region iteration); residuals, Jacobians, the Schur
// complement, the reduced system and every vector of the step live in HBM for the whole solve.
// Loop structure and constants follow SURVEY.md A.6 (Ceres 1.x TrustRegionMinimizer + DoglegStrategy /
// LevenbergMarquardtStrategy defaults).
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "host.hpp"

using namespace covgpu;

thread_local std::string g_err;
extern "C" const char* covgpu_last_error(void) { return g_err.c_str(); }

extern "C" void covgpu_default_options(covgpu_options* o) {
  std::memset(o, 0, sizeof(*o));
  o->strategy = COVGPU_DOGLEG;   // optimization_be.cpp:564
  o->max_iterations = 10;        // config_backend.yaml:115  opt.gba_iteration_limit
  o->reproj_loss_a = 1.0;        // optimization_be.cpp:302
  o->initial_radius = 1e4; o->max_radius = 1e16; o->min_relative_decrease = 1e-3;
  o->function_tolerance = 1e-6; o->parameter_tolerance = 1e-8; o->gradient_tolerance = 1e-10;
  const double sf = std::sqrt(200.0);  // EuRoC.yaml:40-44 at 200 Hz (orb_slam3/src/Tracking.cc:1203-1211)
  o->sigma_g = 1.7e-4 * sf; o->sigma_a = 2.0e-3 * sf; o->sigma_gw = 1.9393e-5 / sf; o->sigma_aw = 3.0e-3 / sf;
  o->gravity = 9.81;             // orb_slam3/include/ImuTypes.h:43
}

extern "C" int32_t covgpu_reduced_dim(const covgpu_options* opt, const covgpu_problem* p) {
  return (opt->visual_only ? 6 : 15) * p->num_kf;
}

// lanes per landmark of the landmark-major kernels (k_visual.hip: k_lm_lin, k_lm_backsub, k_lm_outliers) from the mean track length O/L:
// configs[4] (4.1): linearise+Schur 4.65 ms at 16 lanes, 4.24 at 8, 4.11 at 4; 5-agent map (10.0): 16 and 8 alike
extern "C" int32_t covgpu_lm_group(int64_t num_obs, int32_t num_lm) {
  const double mean_track = num_lm > 0 ? (double)num_obs / num_lm : 0.0;
  return mean_track <= 5.0 ? 4 : (mean_track <= 8.0 ? 8 : 16);
}

extern "C" int covgpu_create(const covgpu_options* opt, covgpu_context** out) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    g_err = "no HIP device visible: libcovgpu has no CPU fallback";
    return COVGPU_ERR_NO_DEVICE;
  }
  covgpu_context* c = new covgpu_context();
  c->device = opt ? opt->device : 0;
  if (c->device < 0 || c->device >= ndev) { g_err = "device ordinal out of range"; delete c; return COVGPU_ERR_INVALID_ARG; }
  HIPCHK(hipSetDevice(c->device));
  {
    // the main stream carries the serial panel chain of the factorisation: give it dispatch priority over the
    // auxiliary stream's bulk trailing updates (k_chol.hip look-ahead)
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
    HIPCHK(hipStreamCreateWithPriority(&c->st, hipStreamDefault, hi));
  }
  HIPCHK(hipHostMalloc((void**)&c->h_scal, (SC_COUNT + 4) * sizeof(double), hipHostMallocDefault));
  HIPCHK(hipHostMalloc((void**)&c->h_tr, TR_COUNT * sizeof(double), hipHostMallocDefault));
  {
    if (hipHostMalloc((void**)&c->h_box, (TR_COUNT + 1) * sizeof(double), hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess) {
      std::memset(c->h_box, 0, (TR_COUNT + 1) * sizeof(double));
      if (hipHostGetDevicePointer((void**)&c->d_box, c->h_box, 0) != hipSuccess) c->d_box = nullptr;
    } else { (void)hipGetLastError(); c->h_box = nullptr; }
  }
  for (auto& e : c->ev) HIPCHK(hipEventCreate(&e));
  std::memset(&c->P, 0, sizeof(c->P));
  *out = c;
  return COVGPU_OK;
}

extern "C" void covgpu_destroy(covgpu_context* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  while (!c->bowdbs.empty()) covgpu_bowdb_destroy(c->bowdbs.back());   // (each removes itself from the list)
  free_problem(c);
  for (auto& e : c->ev) if (e) (void)hipEventDestroy(e);
  c->chol.destroy();
  if (c->h_scal) (void)hipHostFree(c->h_scal);
  if (c->h_tr) (void)hipHostFree(c->h_tr);
  if (c->h_box) (void)hipHostFree(c->h_box);
  clear_shard(c);
  if (c->st) (void)hipStreamDestroy(c->st);
  delete c;
}

extern "C" void covgpu_set_profiling(covgpu_context* c, int on) {
  c->profiling = on; c->prof = covgpu_profile_t();
  c->chol.profile = on != 0; c->chol.syrk_ms = 0; c->chol.syrk_flops = 0; c->chol.n_syrk = 0;
  c->chol.potrf_ms = 0; c->chol.potrf_flops = 0; c->chol.n_potrf = 0;
}
// out[0..7] = build ms, n_build, factor ms, n_factor, syrk ms, n_syrk launches, syrk flops, tri-solve ms
extern "C" void covgpu_get_profile(covgpu_context* c, double* out) {
  out[0] = c->prof.t_build_ms; out[1] = (double)c->prof.n_build; out[2] = c->prof.t_factor_ms; out[3] = (double)c->prof.n_factor;
  out[4] = c->chol.syrk_ms; out[5] = (double)c->chol.n_syrk; out[6] = c->chol.syrk_flops;
  out[7] = (double)(c->have ? c->P.npairs + c->P.nepairs : 0);  // off-diagonal 6x6 pose-pose blocks of the reduced system (nnzS - K)
}
// out[0..7] as covgpu_get_profile; out[8] = k_potrf_panel ms (sum over its launches), [9] = its launches, [10] = its algorithmic flops,
// [11] = flops of ONE multifrontal factorisation of the resident problem's plan (Cholesky of every front incl. its border updates),
// [12..15] = 0
extern "C" void covgpu_get_profile2(covgpu_context* c, double* out) {
  covgpu_get_profile(c, out);
  out[8] = c->chol.potrf_ms; out[9] = (double)c->chol.n_potrf; out[10] = c->chol.potrf_flops; out[11] = c->have ? c->nd.plan_flops : 0.0;
  out[12] = out[13] = out[14] = out[15] = 0.0;
}

// out[16] = { shard world, shard rank, scalar unknowns of the replicated top, top levels, KiB all-reduced per linear solve, stream ordering (1 flags | 0 events | -1 fell back: events and no in-launch hand-overs),
//             dense order npad, covisible pairs, edge pairs, IMU chains, device MiB allocated for the problem,
//             fronts, levels, serial 256-column panels, order of the root level, MiB of fronts } (include/covgpu.h)
// launches per kernel form of the linear solves since the last upload (include/covgpu.h lists the forms)
extern "C" int covgpu_get_kernel_forms(covgpu_context* c, int64_t* out, int32_t n) {
  for (int i = 0; i < n && i < KF_COUNT; ++i) out[i] = c != nullptr ? (int64_t)c->chol.forms.n[i] : 0;
  return KF_COUNT;
}
extern "C" const char* covgpu_kernel_form_name(int32_t i) { return i >= 0 && i < KF_COUNT ? kFormNames[i] : nullptr; }

extern "C" void covgpu_get_layout(covgpu_context* c, int64_t* out) {
  for (int i = 0; i < 16; ++i) out[i] = 0;
  if (!c->have) return;
  const DevProblem& P = c->P;
  out[0] = c->sharded ? c->world : 0; out[1] = c->sharded ? c->rank : 0; out[2] = c->nd.ntop;   // ranks | rank | scalar unknowns of the replicated top nodes
  out[3] = (int64_t)c->nd.lev.size() - c->nd.top_lev0;                                          // top levels
  out[4] = c->nd.dist ? (int64_t)((c->nd.dist_solve_elems * sizeof(double)) >> 10)   // distributed top: every panel's exchange + gradient, diag(J^T J) of the top unknowns
                      : (int64_t)(((size_t)c->nd.n_top_tiles * kTile * kTile + c->nd.rhs_top + 2 * (size_t)c->nd.ntop) * sizeof(double)) >> 10;  // KiB all-reduced per linear solve
  out[5] = c->chol.pipe_broken ? -1 : c->chol.gates_on ? 1 : 0;   // stream ordering: 1 device flags | 0 HIP events (COVGPU_GATES=0) | -1 a gate or the backward pipeline timed out: events and the launch-per-tile substitution from then on
  out[6] = P.npad; out[7] = P.npairs; out[8] = P.nepairs; out[9] = P.nchains; out[10] = (int64_t)(c->alloc_bytes >> 20);
  if (P.nd) {  // multifrontal form: nodes, levels, serial 256-column panels (sum of the levels' interior orders / 256), root order, front bytes (MiB)
    out[11] = P.nd_nnodes; out[12] = P.nd_nlev;
    for (const NdLevel& L : c->nd.lev) out[13] += L.nI / 256;
    out[14] = c->nd.lev.empty() ? 0 : c->nd.lev.back().nI; out[15] = (int64_t)((c->nd.M_elems * sizeof(double)) >> 20);
  }
}

int read_scalars(covgpu_context* c) {
  HIPCHK(hipMemcpyAsync(c->h_scal, c->P.scal, SC_COUNT * sizeof(double), hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipMemcpyAsync(c->h_scal + SC_COUNT, c->P.flag, sizeof(int), hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  HIPCHK(hipGetLastError());  // a failed kernel launch anywhere in the batch just drained surfaces here
  return COVGPU_OK;
}
int chol_failed(covgpu_context* c) { int f; std::memcpy(&f, c->h_scal + SC_COUNT, sizeof(int)); return f; }

// linearise at the current state and form the damped reduced system (A.6): cost, grad, hdiag, Sred, bred
void enqueue_build(covgpu_context* c, double mu) {
  const DevProblem& P = c->P;
  c->cur_damp = mu;
  if (c->profiling) (void)hipEventRecord(c->ev[0], c->st);
  // the clearing of the fronts' live tiles (1.1 GB of fronts on the 5-agent map) runs on its own stream beside the inertial
  // kernels and the landmark linearisation, which only write per-factor / per-observation records; its first writers
  // (k_kf_reduce ...) wait for it. Every reader of the previous system has finished: the host enqueues an iteration only after it has
  // seen the end of the previous one (end_iteration: the mailbox word posted by the iteration's last kernel, or a stream synchronisation),
  // and that last kernel runs behind the linear solve, whose step it applies.
  c->chol.init();
  // Enqueue order = host time: every iteration starts behind a host synchronisation with the chip empty, and a launch is ~6 us of host
  // work. The main stream's own first kernels (the small clears, the landmark linearisation: 0.17 ms, on nobody's results) go out FIRST;
  // the clearing of the fronts (head stream) and the inertial kernels (side stream) follow underneath them. (Before: seven clearing
  // launches ahead of everything, the linearisation started ~0.1 ms into the iteration.)
  // (measured, round 4: clearing the fronts BEHIND the previous linear solve instead — under the trust-region tail — takes 0.11 ms off
  //  this pass and puts 0.12 ms onto the tail and the solve: the 0.65 GB of stores contend with the tail's re-linearisations)
  // (round 6: the landmark linearisation — the head of the pass's critical path — is the FIRST launch of the iteration on the main stream; the small
  //  clears, which it does not depend on, open the side stream instead: their first readers are the inertial kernels there and, on the main
  //  stream, kernels behind the join of the side stream (ev_kf). Before: clears, a fill and a record in front of it, ~12 us.)
  // The side stream's kernels read the estimate (and the preintegration): they follow "the main stream is complete up to here", published by the
  // landmark linearisation's own first thread (no launch in front of it) — or, without landmarks / device flags, by a record.
  hipStream_t side = c->chol.mid;
  {
    DevSignal sig = P.L > 0 ? c->chol.publish_handle(c->chol.ev_zero, c->st, 1) : DevSignal();
    if (sig.flag == nullptr) c->chol.record(c->chol.ev_zero, c->st, 1);
    launch_lm_lin(P, mu, c->st, sig);   // writes per-observation records, per-landmark blocks (incl. the landmark part of grad / hdiag) and cost partials only
  }
  c->chol.wait(side, c->chol.ev_zero);
  launch_zero_system(P, side);
  const bool forked = P.L > 0 && P.npairs > 0;   // (launch_lm_build's condition: its per-keyframe reduction and cost finisher run on `side`)
  if (!forked) { c->chol.record(c->chol.ev_lin, side, 2); c->chol.wait(c->st, c->chol.ev_lin); }   // ... else on the main stream: behind the clears (ev_lin is free: no fork)
  // (the head stream waits for nobody: every reader of the previous system has finished — see above)
  if (P.nd) { launch_nd_zero(P, c->nd, c->chol.head); (void)hipMemsetAsync(P.nd_rhs, 0, c->nd.rhs_elems * sizeof(double), c->chol.head); }   // (the fronts' right-hand sides: was a fill on the chain, in front of the assembly)
  else (void)hipMemsetAsync(P.Sred, 0, (size_t)P.npad * P.npad * sizeof(double), c->chol.head);
  c->chol.record(c->chol.ev_fill, c->chol.head, 3);
  // inertial factors (one wave per factor: latency, not throughput) on the side stream beside the landmark pass; their speed-bias
  // blocks are final before anything of the pose system is touched, the pose-dimension part is gathered after the visual blocks
  launch_imu_build(P, side);
  if (P.vi) {
    launch_imu_gather(P, 1, side);
    launch_finalize_diag(P, mu, 1, side);
  }
  // The bottom level of the elimination tree, where it consists of speed-bias leaf fronts only (NdLevel::leaf_one): everything those fronts hold is
  // final here, long before the pose system is. They are assembled and factored whole — one launch each, no gate inside (k_panel.hip: k_potrf_leaf) —
  // on the head stream, which has just cleared them and is idle during the landmark pass; the serial chain of the solve then starts at level 1.
  // One dependency in (the record below), one out (ev_leaf, which the main stream takes with its join of the side stream further down). In the
  // first iteration of a solve the side stream carries the preintegration: the leaves then finish late, and the join waits for them as it waits
  // for the side stream itself.
  bool leaves_early = false;
  if (P.nd && P.vi && nd_leaves_beside_pass(c->nd)) {
    c->chol.record(c->chol.ev_sb, side, 7);
    c->chol.wait(c->chol.head, c->chol.ev_sb);
    FormScope census(&c->chol.forms);
    leaves_early = launch_nd_leaves(P, c->nd, c->chol.head, c->chol);
    c->chol.record(c->chol.ev_leaf, c->chol.head, 8);
  }
  // Between the pair pass and the first factorisation every launch is a link of the chain (~6 us each): the loop edges are linearised
  // on the side stream beside the landmark pass (they depend on the estimate only), and the cost partials are summed there too — behind
  // the last kernel that writes one (the landmark pass's own finisher runs on the side stream when the pass forks).
  launch_edge_build(P, side);
  launch_lm_build(P, mu, c->st, c->chol.ev_fill, side, c->chol.ev_lin, c->chol.ev_kf, &c->chol);
  if (forked) launch_part_finish(P, SC_COST, 1, side);
  c->chol.record(c->chol.ev_kf, side, 4);
  c->chol.wait(c->st, c->chol.ev_kf, leaves_early ? c->chol.ev_leaf : nullptr);
  // pose-dimension part: adds onto the blocks k_kf_reduce assigned (fixed order: visual, inertial, loop), then the damping. Visual-inertial: one launch
  // (k_pose_finish: every entry gets the same operands in the same order from ONE thread). Not where a loop edge joins two neighbouring chain positions:
  // that pair block can be an IMU factor's cross block as well, and the two additions onto it are ordered by the launches only. Visual-only problems and
  // pose graphs (no inertial part, both halves of the damping, the padding rows of the dense matrix) keep their launches too.
  if (P.vi && !c->edge_beside_imu) launch_pose_finish(P, mu, c->st);
  else {
    launch_imu_gather(P, 0, c->st);
    launch_edge_gather(P, c->st);
    launch_finalize_diag(P, mu, P.vi ? 0 : 2, c->st);
  }
  if (!forked) launch_part_finish(P, SC_COST, 1, c->st);
  if (c->profiling) (void)hipEventRecord(c->ev[1], c->st);
}

void enqueue_solve(covgpu_context* c, double* dst_all) {
  const DevProblem& P = c->P;
  // with profiling on, every bulk trailing-update (SYRK) launch gets its own event pair on its stream so that
  // bench.py can quote the dominant kernel's duration
  if (c->profiling) (void)hipEventRecord(c->ev[2], c->st);
  FormScope census(&c->chol.forms);   // the launchers below count their forms into this context (covgpu_get_kernel_forms)
  if (P.nd) {   // GBA: multifrontal solve of the whole system (k_front.hip)
    if (!launch_nd_solve(P, c->nd, dst_all, c->cur_damp, c->st, c->chol) && !c->coll_failed) { c->coll_failed = true; c->coll_err = "scratch allocation of the backward substitution failed"; }
  }
  else launch_pose_graph_solve(P, dst_all, c->st, c->chol, c->pgo_plan.active ? &c->pgo_plan : nullptr);  // pose graph (k_pgo.hip)
  if (c->profiling) (void)hipEventRecord(c->ev[3], c->st);
  launch_lm_backsub(P, dst_all, dst_all, c->st);
}

static void collect_profile(covgpu_context* c, bool built, bool solved) {
  if (solved && !c->profiling) c->chol.collect();  // (prints the COVGPU_TRACE_PANELS marks; nothing else without profiling)
  if (!c->profiling) return;
  float ms = 0;
  if (built && hipEventElapsedTime(&ms, c->ev[0], c->ev[1]) == hipSuccess) { c->prof.t_build_ms += ms; c->prof.n_build++; }
  if (solved && hipEventElapsedTime(&ms, c->ev[2], c->ev[3]) == hipSuccess) { c->prof.t_factor_ms += ms; c->prof.n_factor++; }
  if (solved) c->chol.collect();
}

// (no clearing of the partial sums before these: every wave of a reduction kernel stores its slot, the same slots at every launch.
//  Measured and dropped: the inertial / loop-edge kernels on a side stream beside the observation kernel, and the whole Cauchy
//  leg underneath the linear solve — both within the +-1 % run-to-run noise, the event hops cost what the overlap buys.)
static void enqueue_jvp(covgpu_context* c, const double* v_all) {
  const DevProblem& P = c->P;
  launch_obs_jvp(P, v_all, c->st);
  launch_imu_jvp(P, v_all, c->st);
  launch_edge_jvp(P, v_all, c->st);
  launch_part_finish(P, SC_JV2, 1, c->st);
}

static void enqueue_cost_candidate(covgpu_context* c) {
  const DevProblem& P = c->P;
  launch_obs_cost(P, P.pose_c, P.lm_c, c->st);
  launch_imu_cost(P, P.pose_c, P.sb_c, c->st);
  launch_edge_cost(P, P.pose_c, c->st);
  launch_part_finish(P, SC_COST, 1, c->st);
}

// Distributed top (shard policy 1): a solve issues a collective per panel of the top. A rank that repeated its solve alone after a gate or
// pipeline time-out (what a sharded context of policy 0 does: solve_any) would pair its reductions with its peers' reductions of other panels —
// under policy 1 any failure ends the call on EVERY rank: the collective is aborted, the peers' give-up flag raised, an error returned. A failed
// collective is reported before a gate that timed out (the gate most likely waited behind it).
static bool dist_sharded(const covgpu_context* c) { return c->sharded && c->shard_plan && c->shard_plan->shard_policy == 1; }
static int dist_fail(covgpu_context* c) {
  if (c->reducer) c->reducer->abort();
  if (c->peer_fail) c->peer_fail->store(1);
  const std::string why = c->coll_failed ? c->coll_err
                                         : std::string("a device-flag gate or a hand-over of the backward substitution timed out (the distributed top does not repeat a solve on one rank)");
  g_err = "sharded solve, rank " + std::to_string(c->rank) + ": " + why;
  return COVGPU_ERR_NO_DEVICE;
}

// Host wait for the iteration just enqueued. One GPU: hipStreamSynchronize. Sharded: polled, so that a collective that never
// completes (a peer died, gave up before its first collective, or never arrived) ends in an ERROR after COVGPU_COLL_TIMEOUT_S
// (default 300 s) instead of a hang; RCCL's asynchronous communicator errors and the give-up flag of an in-process multi-GPU call
// are seen here too. On any of these the collective is aborted (ncclCommAbort / group abort: the peers return as well).
static int wait_iteration(covgpu_context* c) {
  if (c->sharded && c->reducer) {
    static const double limit = getenv("COVGPU_COLL_TIMEOUT_S") ? std::max(1.0, atof(getenv("COVGPU_COLL_TIMEOUT_S"))) : 300.0;
    const auto t0 = std::chrono::steady_clock::now();
    long spins = 0;
    for (;;) {
      const hipError_t q = hipStreamQuery(c->st);
      if (q == hipSuccess) break;
      if (q != hipErrorNotReady) { g_err = std::string("hipStreamQuery: ") + hipGetErrorString(q); return COVGPU_ERR_NO_DEVICE; }
      ++spins;
      // fail checks: after the first 256 busy polls, then every 64 sleeping polls (~4 ms)
      if (spins == 256 || (spins > 256 && (spins & 63) == 0)) {
        const char* why = nullptr;
        if (c->peer_fail && c->peer_fail->load(std::memory_order_relaxed)) why = "another rank of the call gave up";
        else if (c->reducer->async_error() != 0) why = "RCCL reported an asynchronous communicator error";
        else if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > limit) why = "collective timed out (COVGPU_COLL_TIMEOUT_S)";
        if (why) { if (!c->coll_failed) { c->coll_failed = true; c->coll_err = why; } c->reducer->abort(); break; }
      } else if (spins > 256) std::this_thread::sleep_for(std::chrono::microseconds(50));   // (a rank's host thread sleeps between polls instead of burning a core for the whole iteration)
    }
  }
  HIPCHK(hipStreamSynchronize(c->st));
  return COVGPU_OK;
}

// Status of an iteration whose last kernel the host has seen complete — the ONE check behind both ends of an iteration (mailbox, stream
// synchronisation): a failed launch, then a failure under the distributed top, a gate that gave up, a latched collective / scratch failure.
static int iteration_status(covgpu_context* c) {
  HIPCHK(hipGetLastError());  // a failed kernel launch anywhere in the batch just drained surfaces here
  if (dist_sharded(c) && (c->coll_failed || c->chol.gate_failed())) return dist_fail(c);
  if (c->chol.gate_failed()) {   // a device-flag gate between two streams gave up (CholAux::wait): what this iteration computed is not ordered
    g_err = "solve: a device-flag gate between the context's streams timed out (COVGPU_GATE_TIMEOUT_S; COVGPU_GATES=0 selects HIP events)";
    return COVGPU_ERR_GATE_TIMEOUT;
  }
  if (c->coll_failed) {
    if (c->reducer) c->reducer->abort();
    if (c->peer_fail) c->peer_fail->store(1);
    g_err = (c->sharded ? "sharded solve, rank " + std::to_string(c->rank) + ": " : std::string("solve: ")) + c->coll_err;
    return COVGPU_ERR_NO_DEVICE;
  }
  return COVGPU_OK;
}

// End of an iteration on the host: the trust-region state the iteration's last kernel left (P.tr) arrives in c->h_tr — through the pinned
// mailbox (use_box: the kernel posted it there; no D2H copy, no sleeping wait) or by a D2H copy behind wait_iteration — then the one status check.
static int end_iteration(covgpu_context* c, bool use_box) {
  double* h = c->h_tr;
  bool got = false;
  if (use_box) {
    // poll the sequence word (the kernel stores it with release semantics behind the state); every 4096 polls look at the stream: an error, or a stream
    // that drained without the word arriving (never observed), ends in the ordinary path
    volatile double* box = c->h_box;
    for (unsigned spins = 1; !got; ++spins) {
      if (box[TR_COUNT] == c->box_seq) { got = true; break; }
      if ((spins & 4095u) == 0) { const hipError_t q = hipStreamQuery(c->st); if (q != hipErrorNotReady) break; }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    if (got) for (int i = 0; i < TR_COUNT; ++i) h[i] = box[i];
  }
  if (!got) {
    HIPCHK(hipMemcpyAsync(h, c->P.tr, TR_COUNT * sizeof(double), hipMemcpyDeviceToHost, c->st));
    RC(wait_iteration(c));
  }
  const int rc = iteration_status(c);
  if (rc != COVGPU_OK && got) (void)hipStreamSynchronize(c->st);   // (the word has arrived, the other streams may still run: the caller repeats the solve, or gives up, on a drained device)
  return rc;
}

// The iteration behind the host's decision `reuse` (the step was rejected: the system stands, the radius shrank) or a rebuild at damping
// `damp`, fused form (k_tail.hip). Returns whether the iteration's last kernel posts the state to the pinned mailbox.
static bool enqueue_tail_fused(covgpu_context* c, const TrConsts& tc, bool reuse, double damp) {
  const DevProblem& P = c->P;
  const bool two = tc.strategy == COVGPU_DOGLEG;
  const bool coll = c->sharded && c->reducer != nullptr;   // scalar all-reduce between a finish and the step logic that reads it
  if (!reuse) {
    enqueue_build(c, damp);
    enqueue_solve(c, P.gn);
    launch_tail_stats(P, c->st);
    launch_tail_jvp(P, two, c->st);
    launch_tail_finish(P, tc, 1, two, !coll, 1, c->st);
    if (coll) { reduce_scalars(c); launch_tail_logic(P, tc, 1, 1, c->st); }
  } else launch_tail_logic(P, tc, 1, 0, c->st);
  launch_tail_apply(P, c->st);
  launch_tail_cost(P, c->st);
  launch_tail_finish(P, tc, 2, two, !coll, 0, c->st);
  if (coll) { reduce_scalars(c); launch_tail_logic(P, tc, 2, 0, c->st); }
  // (one GPU, no profiling events to collect: the state the host needs travels through the pinned mailbox, no D2H copy, no sleeping wait)
  static const bool dev_aids = getenv("COVGPU_TRACE_PANELS") != nullptr || getenv("COVGPU_GATE_LOG") != nullptr;   // (their print-outs read events / device logs behind a synchronisation)
  const bool use_box = c->d_box != nullptr && !coll && !c->profiling && !dev_aids;
  if (use_box) c->box_seq += 1.0;
  launch_tr_accept(P, c->st, use_box ? c->d_box : nullptr, c->box_seq);
  return use_box;
}
// The same iteration, legacy form (COVGPU_TAIL=0). Never uses the mailbox.
static bool enqueue_tail_legacy(covgpu_context* c, const TrConsts& tc, bool reuse, double damp) {
  const DevProblem& P = c->P;
  if (!reuse) {
    enqueue_build(c, damp);
    enqueue_solve(c, P.gn);
    // (Cauchy direction after the solve: a sharded solve completes gradient and diag(J^T J) of the top unknowns inside it)
    if (tc.strategy == COVGPU_DOGLEG) { launch_cauchy_vec(P, c->st); enqueue_jvp(c, P.vtmp); }
    launch_dogleg_stats(P, c->st);
    reduce_scalars(c);
  }
  launch_tr_after_solve(P, tc, reuse ? 0 : 1, c->st);
  launch_combine_step_dev(P, c->st);
  enqueue_jvp(c, P.step);
  launch_xnorm(P, c->st);
  reduce_scalars(c);
  launch_tr_after_model(P, tc, c->st);
  launch_apply_step(P, c->st);
  enqueue_cost_candidate(c);
  reduce_scalars(c);
  launch_tr_decide(P, tc, c->st);
  return false;
}

// Trust-region loop with the step logic on the device (k_dense.hip: k_tr_*): ONE host read-back per iteration — what the
// host needs to enqueue the next one (rebuild or reuse, damping value) and the trace. Sharded solve: the same loop on every
// rank; four collectives per iteration (the top of the tree inside the linear solve, three scalar exchanges), all enqueued on
// the stream.
static int solve_impl_dev(covgpu_context* c, const covgpu_options* opt, covgpu_result* res) {
  if (!c->have) { g_err = "no problem uploaded"; return COVGPU_ERR_INVALID_ARG; }
  HIPCHK(hipSetDevice(c->device));
  DevProblem& P = c->P;
  const covgpu_options& o = *opt;
  P.reproj_loss_a = o.reproj_loss_a;
  std::memset(res, 0, sizeof(*res));
  c->coll_failed = false; c->coll_err.clear();   // (an aborted collective fails again at once and is latched again)
  const auto t_begin = std::chrono::steady_clock::now();
  c->chol.init();
  if (c->sharded) c->chol.gate_timeout_s = std::max(c->chol.gate_timeout_s, 120.0);   // (a gate may stand behind a collective that waits for a slower rank)
  c->trace_n = 0;
  RC(reset_state(c));
  // R2: repropagate at the initial bias estimate (opt_be.cpp:396) — in every solve, on the side stream, behind reset_state (it reads the biases).
  // Nothing else orders it: every reader of pre_* is either on that stream behind it (k_imu_build) or on the main stream behind the join ev_kf of
  // the same first iteration (k_pose_finish, k_tail_jvp, k_tail_cost), so the first landmark linearisation and the pair pass run beside it and
  // the synchronisation below does not wait for it. Its previous readers have finished: a solve returns behind its last iteration.
  c->chol.record(c->chol.ev_zero, c->st, 1);
  c->chol.wait(c->chol.mid, c->chol.ev_zero);
  HIPCHK(hipMemsetAsync(P.flag + 1, 0, sizeof(int), c->chol.mid));
  launch_preintegrate(P, c->chol.mid);
  double* h = c->h_tr;
  std::memset(h, 0, TR_COUNT * sizeof(double));
  h[TR_RADIUS] = o.initial_radius; h[TR_MU] = 1e-8; h[TR_LMDF] = 2.0; h[TR_FIRST] = 1.0; h[TR_OK] = 1.0;
  HIPCHK(hipMemcpyAsync(P.tr, h, TR_COUNT * sizeof(double), hipMemcpyHostToDevice, c->st));
  HIPCHK(hipStreamSynchronize(c->st));  // (h is reused as the read-back mirror below)
  const TrConsts tc{o.strategy, o.max_radius, o.min_relative_decrease, o.function_tolerance, o.parameter_tolerance, o.gradient_tolerance};
  bool reuse = false, got_initial = false;
  int it = 0, accepted = 0, term = 0;
  // COVGPU_TAIL=0: the round-3 tail (two J*v passes of three kernels, seven partial-sum finishers, four one-thread logic kernels:
  // ~25 dependent launches); default: the fused tail of k_tail.hip (8 launches, one J*v pass for both dogleg directions)
  static const bool fused_tail = env_int("COVGPU_TAIL", 1) != 0;
  while (it < o.max_iterations) {
    const double damp = (o.strategy == COVGPU_LM) ? 1.0 / h[TR_RADIUS] : h[TR_MU];   // (of the system a rebuild forms)
    const bool use_box = fused_tail ? enqueue_tail_fused(c, tc, reuse, damp) : enqueue_tail_legacy(c, tc, reuse, damp);
    RC(end_iteration(c, use_box));
    if (c->trace != nullptr) {   // (test hook: covgpu_solve_resident_traced)
      if (c->trace_n < c->trace_cap) std::memcpy(c->trace + (size_t)TR_COUNT * c->trace_n, h, TR_COUNT * sizeof(double));
      ++c->trace_n;
    }
    collect_profile(c, !reuse, !reuse);
    if (!got_initial) { res->initial_cost = h[TR_INITCOST]; got_initial = true; }
    if (h[TR_RETRY] != 0.0) { reuse = false; continue; }  // factorisation failed: same iteration again with the raised damping
    term = (int)h[TR_TERM];
    if (term == 3 || term == 2) break;
    const int acc = h[TR_ACC] != 0.0;
    accepted += acc;
    if (it < COVGPU_MAX_TRACE) { res->cost_trace[it] = h[TR_COST]; res->radius_trace[it] = h[TR_RADIUS]; res->accepted_trace[it] = acc; }
    if (o.verbose) std::printf("[covgpu] it %2d cost %.9e rho %.3f radius %.3e %s\n", it, h[TR_COST], h[TR_RHO], h[TR_RADIUS], acc ? "ok" : "rej");
    reuse = h[TR_REUSE] != 0.0;
    ++it;
    if (term == 1 || term == 4) break;
  }
  if (it == 0) HIPCHK(hipStreamSynchronize(c->chol.mid));   // (no iteration ran: nothing has joined the preintegration yet)
  {  // IMU factors whose preintegrated covariance was not positive definite (e.g. zero samples) carry no weight: reported
    int dropped = 0;
    HIPCHK(hipMemcpy(&dropped, P.flag + 1, sizeof(int), hipMemcpyDeviceToHost));
    res->reserved = dropped;
  }
  res->iterations = it; res->accepted = accepted; res->termination = term;
  res->final_cost = h[TR_COST];
  res->t_solve_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count();
  res->t_linear_solve_s = 0.0;  // (not separable without extra synchronisation: covgpu_get_profile has the phase times)
  return COVGPU_OK;
}

// A solve whose stream ordering through device flags failed (CholAux::wait timed out: a tool that serialises kernels out of submission order, a
// lost dispatch) is repeated ONCE with HIP events — every solve restarts from the uploaded state (reset_state) — and the context keeps events from then on.
int solve_any(covgpu_context* c, const covgpu_options* opt, covgpu_result* out) {
  int rc = solve_impl_dev(c, opt, out);
  if (rc == COVGPU_ERR_GATE_TIMEOUT) {
    if (c->chol.gate_dead_h[1] == -2)   // (k_bwd.hip: pipe_take)
      std::fprintf(stderr, "[covgpu] warning: a hand-over inside the pipelined backward substitution timed out (workgroup %d of front %d of its level); repeating the solve with a launch per tile and HIP events (this context keeps them)\n",
                   c->chol.gate_dead_h[2], c->chol.gate_dead_h[3]);
    else
    std::fprintf(stderr, "[covgpu] warning: device-flag stream ordering timed out (slot %d awaited %d, found %d; %ld signals, %ld gates so far); repeating the solve with HIP events (this context keeps them)\n",
                 c->chol.gate_dead_h[1], c->chol.gate_dead_h[2], c->chol.gate_dead_h[3], c->chol.gate_signals, c->chol.gate_waits);
    if (c->chol.gate_dead_h[1] >= 0 && c->chol.gate_dead_h[1] < (int)c->chol.gate_tag_of_slot.size()) std::fprintf(stderr, "[covgpu]          (tag of that slot: %d)\n", c->chol.gate_tag_of_slot[c->chol.gate_dead_h[1]]);
    (void)hipDeviceSynchronize();
    c->chol.gates_disable();
    rc = solve_impl_dev(c, opt, out);
    if (rc == COVGPU_ERR_GATE_TIMEOUT) { g_err = "solve: stream ordering failed"; rc = COVGPU_ERR_NO_DEVICE; }
  }
  return rc;
}
extern "C" int covgpu_solve_resident(covgpu_context* c, const covgpu_options* opt, covgpu_result* out) { return guarded([&] { return solve_any(c, opt, out); }); }
static_assert(COVGPU_TR_COUNT == TR_COUNT && COVGPU_SC_COUNT == SC_COUNT, "include/covgpu.h states the sizes of the test entry points' buffers");
extern "C" int covgpu_solve_resident_traced(covgpu_context* c, const covgpu_options* opt, covgpu_result* out, double* trace, int32_t capacity, int32_t* count) {
  if (!c) { g_err = "covgpu_solve_resident_traced: NULL context"; return COVGPU_ERR_INVALID_ARG; }
  if (!opt || !out || !trace || !count || capacity < 0) { g_err = "covgpu_solve_resident_traced: NULL argument"; return COVGPU_ERR_INVALID_ARG; }
  c->trace = trace; c->trace_cap = capacity;
  const int rc = guarded([&] { return solve_any(c, opt, out); });
  *count = c->trace_n;
  c->trace = nullptr; c->trace_cap = 0;
  return rc;
}

static int full_solve(covgpu_context* c, const covgpu_options* opt, covgpu_problem* p, covgpu_result* out, bool pgo) {
  covgpu_result local;
  auto t0 = std::chrono::steady_clock::now();
  RC(upload_impl(c, opt, p, pgo));
  const double t_up = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  RC(solve_any(c, opt, &local));
  t0 = std::chrono::steady_clock::now();
  RC(download_impl(c, p));
  local.t_download_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  local.t_upload_s = t_up;
  if (out) *out = local;
  return COVGPU_OK;
}
extern "C" int covgpu_gba_solve(covgpu_context* c, const covgpu_options* opt, covgpu_problem* p, covgpu_result* out) { return guarded([&] { return full_solve(c, opt, p, out, false); }); }
extern "C" int covgpu_pgo_solve(covgpu_context* c, const covgpu_options* opt, covgpu_problem* p, covgpu_result* out) { return guarded([&] { return full_solve(c, opt, p, out, true); }); }

// ------------------------------------------------------------------------------------------------ both rounds of a GlobalBundleAdjustment call
// optimization_be.cpp:56-618 builds and solves TWO problems: the outlier round (5 iterations, loop edges without loss, :62-265), then —
// after erasing the observations whose loss-corrected residual exceeds th_gba_outlier_global (:270-290) — the main round on the rebuilt
// problem (:296-567), restarted from the SAME map state (the outlier round's estimate is discarded). The second problem is the first
// minus the erased observations, minus the landmarks left with fewer than two (:428-440), with the loop edges' loss switched on (:555)
// and optionally more constant poses (:338-341): nothing a second Map -> IR flatten and a second H2D upload would have to tell the
// device. Here it is derived ON the device from the resident first round (k_pairs.hip: round2_compact_device; pair lists rebuilt by
// the same device code as an upload; the elimination tree stays — couplings only disappear), and only the erase flags travel back for
// the caller's map bookkeeping. p: the FIRST round's problem; on return its poses / speed-bias hold the second round's estimate and
// lm_pos[l] the second round's for every landmark with lm_left[l] >= 2 (the others took no part, as in the reference).
// State of the context afterwards: the resident problem is the SECOND round's (compacted landmark / observation indexing), which the
// caller's covgpu_problem does not describe — so the context is marked as holding no problem when the call returns, successfully or not:
// covgpu_download / covgpu_outlier_pass / covgpu_solve_resident after it fail with "no problem uploaded" instead of scattering into the
// first round's slots, and an error half-way cannot leave a half-switched problem behind. (Everything the caller needs came back through
// p, obs_erase, lm_left and the two results.)
extern "C" int covgpu_gba_two_round(covgpu_context* c, const covgpu_options* opt, covgpu_problem* p, const covgpu_two_round* tr, uint8_t* obs_erase,
                                    int32_t* lm_left, int64_t* counts, covgpu_result* round1, covgpu_result* round2) {
  const int rc = gba_two_round_impl(c, opt, p, tr, obs_erase, lm_left, counts, round1, round2);
  if (c) { c->second_round = rc == COVGPU_OK && c->have; c->have = false; }
  return rc;
}
int gba_two_round_impl(covgpu_context* c, const covgpu_options* opt, covgpu_problem* p, const covgpu_two_round* tr, uint8_t* obs_erase,
                       int32_t* lm_left, int64_t* counts, covgpu_result* round1, covgpu_result* round2) {
  return guarded([&]() -> int {
    if (!tr || !obs_erase || !lm_left) { g_err = "covgpu_gba_two_round: NULL argument"; return (int)COVGPU_ERR_INVALID_ARG; }
    // (round 6: a sharded context takes the call too — every rank derives the second round of ITS share on its device: its landmarks' outlier decisions,
    //  compaction and pair lists are local, the elimination tree stays, and both solves issue the same collectives on every rank. The caller merges the
    //  ranks' flags and estimates: covgpu_gba_two_round_multi.)
    covgpu_options o1 = *opt;
    o1.max_iterations = tr->round1_iterations > 0 ? tr->round1_iterations : 5;   // :262
    auto t0 = std::chrono::steady_clock::now();
    RC(upload_impl(c, &o1, p, false));
    covgpu_result a, b;
    const double t_up = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    RC(solve_any(c, &o1, &a));
    a.t_upload_s = t_up;
    DevProblem& P = c->P;
    t0 = std::chrono::steady_clock::now();
    // ---- outlier decisions at the resident estimate (:270-290); the flags stay on the device and a copy goes to the caller
    unsigned char* de = nullptr; int* dl = nullptr; unsigned long long* dc = nullptr;
    RC(dev_alloc(c, &de, (size_t)std::max(P.O, 1))); RC(dev_alloc(c, &dl, (size_t)std::max(P.L, 1))); RC(dev_alloc(c, &dc, (size_t)2));
    HIPCHK(hipMemsetAsync(dc, 0, 2 * sizeof(unsigned long long), c->st));
    launch_lm_outliers(P, tr->outlier_threshold, de, dl, dc, c->st);
    unsigned long long hc[2] = {0, 0};
    if (P.O) HIPCHK(hipMemcpyAsync(obs_erase, de, (size_t)P.O, hipMemcpyDeviceToHost, c->st));
    if (P.L) HIPCHK(hipMemcpyAsync(lm_left, dl, sizeof(int) * (size_t)P.L, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipMemcpyAsync(hc, dc, sizeof(hc), hipMemcpyDeviceToHost, c->st));
    // ---- the second round's observation stream, compacted on the device
    Round2Lists R;
    if (!round2_compact_device(P.L, P.O, P.K, de, dl, P.obs_kf, P.obs_lm, P.obs_u, P.obs_v, P.obs_sigma, P.lm0, c->st, R)) {
      g_err = "covgpu_gba_two_round: device allocation failed while compacting the observation stream"; return (int)COVGPU_ERR_OUT_OF_MEMORY;
    }
    for (void* q : {(void*)R.lm0, (void*)R.obs_u, (void*)R.obs_v, (void*)R.obs_sigma, (void*)R.lm_obs_ptr, (void*)R.lm_old, (void*)R.obs_kf, (void*)R.obs_lm, (void*)R.kf_obs_ptr,
                    (void*)R.kf_obs_idx})
      if (q) c->allocs.push_back(q);
    if (counts) { counts[0] = (int64_t)hc[0]; counts[1] = (int64_t)hc[1]; }   // (round2_compact_device ends with a stream synchronisation)
    const int L1 = P.L;
    if (R.L2 > 0 && R.O2 > 0) {
      P.L = R.L2; P.O = R.O2; P.N = P.n + 3 * P.L;
      P.lm0 = R.lm0; P.lm_obs_ptr = R.lm_obs_ptr; P.obs_kf = R.obs_kf; P.obs_lm = R.obs_lm; P.obs_u = R.obs_u; P.obs_v = R.obs_v; P.obs_sigma = R.obs_sigma;
      P.kf_obs_ptr = R.kf_obs_ptr; P.kf_obs_idx = R.kf_obs_idx;
    } else { P.L = 0; P.O = 0; P.N = P.n; }
    if (tr->kf_fixed_round2 != nullptr) {   // opt.gba_fix_poses_loaded_maps (:338-341): more constant poses in the second round
      HIPCHK(hipMemcpyAsync(P.fixed, tr->kf_fixed_round2, (size_t)P.K, hipMemcpyHostToDevice, c->st));
      std::vector<int> key(P.K);
      for (int k = 0; k < P.K; ++k) key[k] = tr->kf_fixed_round2[k] ? -1 : c->h_perm[k];
      HIPCHK(hipMemcpyAsync(c->d_pairkey, key.data(), sizeof(int) * (size_t)P.K, hipMemcpyHostToDevice, c->st));
      HIPCHK(hipStreamSynchronize(c->st));
    }
    // covisible pairs of what is left (same device code as an upload); the elimination tree stays: couplings only disappear
    RC(upload_pair_lists(c, true, nullptr, nullptr));
    // (the reductions store one partial sum per wave into fixed slots and never clear them: fewer observations = fewer waves, and the
    //  first round's partials beyond them would be summed again)
    HIPCHK(hipMemsetAsync(P.part, 0, (size_t)SC_COUNT * P.part_n * sizeof(double), c->st));
    if (!tr->use_loops_round2) { P.E = 0; P.nepairs = 0; }   // opt.gba_use_map_loop_constraints (:534)
    else if (P.E > 0) {
      std::vector<double> la((size_t)P.E, tr->loop_loss_round2);   // Cauchy on the loop edges in the second round (:555)
      HIPCHK(hipMemcpyAsync(P.edge_loss_a, la.data(), sizeof(double) * (size_t)P.E, hipMemcpyHostToDevice, c->st));
    }
    HIPCHK(hipStreamSynchronize(c->st));
    const double t_prep = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    RC(solve_any(c, opt, &b));
    b.t_upload_s = t_prep;   // (what replaces the second upload: outlier pass, compaction, pair lists)
    // ---- estimate of the second round -> caller's arrays; landmarks through the first-round index of every kept one
    t0 = std::chrono::steady_clock::now();
    RC(download_states(c, p));
    std::vector<double> lm2((size_t)3 * P.L);
    std::vector<int> old((size_t)P.L);
    if (P.L) {
      HIPCHK(hipMemcpyAsync(lm2.data(), P.lm, lm2.size() * sizeof(double), hipMemcpyDeviceToHost, c->st));
      HIPCHK(hipMemcpyAsync(old.data(), R.lm_old, old.size() * sizeof(int), hipMemcpyDeviceToHost, c->st));
    }
    HIPCHK(hipStreamSynchronize(c->st));
    for (int q = 0; q < P.L; ++q) {
      if (old[q] < 0 || old[q] >= L1) { g_err = "covgpu_gba_two_round: landmark map out of range"; return (int)COVGPU_ERR_INVALID_ARG; }
      std::memcpy(p->lm_pos + 3 * (size_t)old[q], lm2.data() + 3 * (size_t)q, 3 * sizeof(double));
    }
    b.t_download_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (round1) *round1 = a;
    if (round2) *round2 = b;
    return (int)COVGPU_OK;
  });
}

// Outlier decisions + landmark bookkeeping at the RESIDENT estimate (the state covgpu_gba_solve / covgpu_solve_resident
// left on the device): no re-upload, only flags and counts come back.
extern "C" int covgpu_outlier_pass(covgpu_context* c, double threshold, uint8_t* obs_erase, int32_t* lm_left, int64_t* counts) {
  if (!c->have || c->pgo) { g_err = "covgpu_outlier_pass needs a resident GBA problem (call covgpu_gba_solve or covgpu_upload + covgpu_solve_resident first)"; return COVGPU_ERR_INVALID_ARG; }
  HIPCHK(hipSetDevice(c->device));
  const DevProblem& P = c->P;
  unsigned long long hc[2] = {0, 0};   // (receives a fetch: declared before the scratch)
  DeviceScratch U(c->st);
  unsigned char* de = nullptr; int* dl = nullptr; unsigned long long* dc = nullptr;
  HIPCHK(U.alloc(&de, (size_t)P.O)); HIPCHK(U.alloc(&dl, (size_t)P.L)); HIPCHK(U.zeroed(&dc, 2));
  launch_lm_outliers(P, threshold, de, dl, dc, c->st);
  HIPCHK(U.fetch(obs_erase, de, (size_t)P.O)); HIPCHK(U.fetch(lm_left, dl, (size_t)P.L)); HIPCHK(U.fetch(hc, dc, 2));
  HIPCHK(hipStreamSynchronize(c->st));
  if (counts) { counts[0] = (int64_t)hc[0]; counts[1] = (int64_t)hc[1]; }
  return COVGPU_OK;
}

// Covisibility recount on the RESIDENT problem (Keyframe::UpdateCovisibilityConnections, keyframe_be.cpp:559-608, which
// backend.cpp:164-167 runs over every keyframe after a GBA): weight(i, j) = number of landmarks both keyframes observe; pairs
// with weight >= threshold (sys.covis_thres) come back as (kf_i > kf_j, weight), sorted by (kf_i, kf_j). All keyframes take
// part, constant ones included. The counting runs on the device (k_pairs.hip); *count = pairs found (may exceed capacity).
extern "C" int covgpu_covisibility(covgpu_context* c, int32_t threshold, int64_t capacity, int32_t* kf_i, int32_t* kf_j, int32_t* weight, int64_t* count) {
  return guarded([&]() -> int {
    if (!c->have || c->pgo) { g_err = "covgpu_covisibility needs a resident GBA problem"; return (int)COVGPU_ERR_INVALID_ARG; }
    HIPCHK(hipSetDevice(c->device));
    const DevProblem& P = c->P;
    std::vector<int> iota(P.K);
    for (int k = 0; k < P.K; ++k) iota[k] = k;
    std::vector<int> pi, pj, pp;   // (receive a fetch: declared before the scratch)
    DeviceScratch U(c->st);
    int* d_key = nullptr;
    HIPCHK(U.upload(&d_key, iota.data(), iota.size()));
    PairLists pl;
    const bool ok = build_pairs_device(P.L, P.K, P.lm_obs_ptr, P.obs_kf, d_key, false, c->st, pl);
    if (!ok) { g_err = "covgpu_covisibility: device allocation failed"; return (int)COVGPU_ERR_OUT_OF_MEMORY; }
    for (int* q : {pl.pair_ptr, pl.pair_i, pl.pair_j}) U.adopt(q);   // allocated in k_pairs.hip, released with the rest
    const size_t np = (size_t)pl.npairs;
    pi.resize(np); pj.resize(np); pp.resize(np + 1);
    HIPCHK(U.fetch(pi.data(), pl.pair_i, np)); HIPCHK(U.fetch(pj.data(), pl.pair_j, np)); HIPCHK(U.fetch(pp.data(), pl.pair_ptr, np + 1));
    HIPCHK(hipStreamSynchronize(c->st));
    int64_t n = 0;
    for (int q = 0; q < pl.npairs; ++q) {
      const int w = pp[q + 1] - pp[q];
      if (w < threshold) continue;
      if (n < capacity) { kf_i[n] = pi[q]; kf_j[n] = pj[q]; weight[n] = w; }
      ++n;
    }
    *count = n;
    return (int)COVGPU_OK;
  });
}

