// multi.hip — the in-process multi-GPU solve of libcovgpu: covgpu_gba_solve_multi and covgpu_gba_two_round_multi with the
// splitter of one problem into the ranks' sub-problems. It drives the other files through the C entry points (plan, group,
// shard, context) and through upload_impl / solve_any / download_impl / gba_two_round_impl (host.hpp).
//
// What a covins_backend process (one process, several GPUs) calls: the whole sharded GlobalBundleAdjustment solve behind one
// C entry point — plan on the full problem, one context and one host thread per rank, the native collective (RCCL when the
// ranks sit on different devices; the in-process group when they share one: virtual ranks, the one-GPU test form), merge.
// Optionally also the outlier decisions of optimization_be.cpp:270-290 at the estimate the solve left resident on each rank.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "host.hpp"

using namespace covgpu;

namespace {
struct SubProblem {
  std::vector<double> lm_pos, obs_uv, obs_sigma, imu_samples, imu_first, imu_noise, edge_meas, edge_info, edge_loss, pose, sb;
  std::vector<int32_t> lm_obs_ptr, obs_kf, imu_i, imu_j, imu_ptr, edge_i, edge_j, lm_id, obs_id;
  covgpu_problem view;
};
void make_sub(const covgpu_problem& p, int r, const int32_t* lm_rank, const int32_t* imu_rank, const int32_t* edge_rank, SubProblem& s) {
  s.pose.assign(p.kf_pose, p.kf_pose + 7 * (size_t)p.num_kf);
  if (p.kf_speed_bias) s.sb.assign(p.kf_speed_bias, p.kf_speed_bias + 9 * (size_t)p.num_kf);
  s.lm_obs_ptr.assign(1, 0);
  for (int l = 0; l < p.num_lm; ++l) {
    if (lm_rank[l] != r) continue;
    s.lm_id.push_back(l);
    s.lm_pos.insert(s.lm_pos.end(), p.lm_pos + 3 * (size_t)l, p.lm_pos + 3 * (size_t)l + 3);
    for (int o = p.lm_obs_ptr[l]; o < p.lm_obs_ptr[l + 1]; ++o) {
      s.obs_id.push_back(o); s.obs_kf.push_back(p.obs_kf[o]);
      s.obs_uv.push_back(p.obs_uv[2 * (size_t)o]); s.obs_uv.push_back(p.obs_uv[2 * (size_t)o + 1]); s.obs_sigma.push_back(p.obs_sigma[o]);
    }
    s.lm_obs_ptr.push_back((int32_t)s.obs_kf.size());
  }
  s.imu_ptr.assign(1, 0);
  for (int f = 0; f < p.num_imu; ++f) {
    if (imu_rank[f] != r) continue;
    s.imu_i.push_back(p.imu_kf_i[f]); s.imu_j.push_back(p.imu_kf_j[f]);
    s.imu_samples.insert(s.imu_samples.end(), p.imu_samples + 7 * (size_t)p.imu_sample_ptr[f], p.imu_samples + 7 * (size_t)p.imu_sample_ptr[f + 1]);
    s.imu_ptr.push_back((int32_t)(s.imu_samples.size() / 7));
    s.imu_first.insert(s.imu_first.end(), p.imu_first + 6 * (size_t)f, p.imu_first + 6 * (size_t)f + 6);
    if (p.imu_noise) s.imu_noise.insert(s.imu_noise.end(), p.imu_noise + 5 * (size_t)f, p.imu_noise + 5 * (size_t)f + 5);
  }
  for (int e = 0; e < p.num_edge; ++e) {
    if (edge_rank[e] != r) continue;
    s.edge_i.push_back(p.edge_i[e]); s.edge_j.push_back(p.edge_j[e]);
    s.edge_meas.insert(s.edge_meas.end(), p.edge_meas + 7 * (size_t)e, p.edge_meas + 7 * (size_t)e + 7);
    s.edge_info.insert(s.edge_info.end(), p.edge_sqrt_info + 36 * (size_t)e, p.edge_sqrt_info + 36 * (size_t)e + 36);
    s.edge_loss.push_back(p.edge_loss_a[e]);
  }
  covgpu_problem& v = s.view;
  v = p;
  v.kf_pose = s.pose.data(); v.kf_speed_bias = p.kf_speed_bias ? s.sb.data() : nullptr;
  v.num_lm = (int32_t)s.lm_id.size(); v.num_obs = (int32_t)s.obs_kf.size(); v.num_imu = (int32_t)s.imu_i.size(); v.num_edge = (int32_t)s.edge_i.size();
  v.num_imu_samples = (int32_t)(s.imu_samples.size() / 7);
  v.lm_pos = s.lm_pos.data(); v.lm_obs_ptr = s.lm_obs_ptr.data(); v.obs_kf = s.obs_kf.data(); v.obs_uv = s.obs_uv.data(); v.obs_sigma = s.obs_sigma.data();
  v.imu_kf_i = s.imu_i.data(); v.imu_kf_j = s.imu_j.data(); v.imu_sample_ptr = s.imu_ptr.data(); v.imu_samples = s.imu_samples.data();
  v.imu_first = s.imu_first.data(); v.imu_noise = p.imu_noise ? s.imu_noise.data() : nullptr;
  v.edge_i = s.edge_i.data(); v.edge_j = s.edge_j.data(); v.edge_meas = s.edge_meas.data(); v.edge_sqrt_info = s.edge_info.data(); v.edge_loss_a = s.edge_loss.data();
}
}  // namespace

// tr == nullptr: ONE solve per rank (+ the outlier decisions at its estimate when obs_erase is given) | tr != nullptr: both rounds of a GlobalBundleAdjustment
// call per rank (gba_two_round_impl on the rank's sharded context; `out1` = the first round's result)
static int gba_multi_impl(const covgpu_options* opt, covgpu_problem* p, covgpu_result* out, int32_t n_ranks, const int32_t* devices,
                          double outlier_threshold, uint8_t* obs_erase, int32_t* lm_left, int64_t* counts, const covgpu_two_round* tr, covgpu_result* out1) {
  return guarded([&] {
    if (n_ranks < 1 || n_ranks > 16 || !devices) { g_err = "covgpu_gba_solve_multi: 1..16 ranks with a device each"; return (int)COVGPU_ERR_INVALID_ARG; }
    std::vector<int32_t> lm_rank(std::max(p->num_lm, 1)), imu_rank(std::max(p->num_imu, 1)), edge_rank(std::max(p->num_edge, 1));
    covgpu_nd_plan* plan = nullptr;
    const int nsub = covgpu_shard_plan(opt, p, n_ranks, &plan, lm_rank.data(), imu_rank.data(), edge_rank.data());
    if (nsub <= 0) { g_err = "covgpu_gba_solve_multi: the problem does not split (" + g_err + ")"; return (int)COVGPU_ERR_INVALID_ARG; }
    struct PlanGuard { covgpu_nd_plan* p; ~PlanGuard() { covgpu_nd_plan_destroy(p); } } plan_guard{plan};   // freed on every exit path
    bool shared_device = false;
    for (int a = 0; a < n_ranks; ++a) for (int b = 0; b < a; ++b) shared_device |= devices[a] == devices[b];
    covgpu_group* grp = nullptr;
    uint8_t uid[128];
    if (shared_device || n_ranks == 1) { RC(covgpu_group_create(n_ranks, &grp)); }
    else { RC(covgpu_rccl_unique_id(uid)); }
    struct GroupGuard { covgpu_group* g; ~GroupGuard() { if (g) covgpu_group_destroy(g); } } grp_guard{grp};
    std::vector<SubProblem> sub(n_ranks);
    for (int r = 0; r < n_ranks; ++r) make_sub(*p, r, lm_rank.data(), imu_rank.data(), edge_rank.data(), sub[r]);
    std::vector<covgpu_result> res(n_ranks), res1(n_ranks);
    std::vector<int> rcs(n_ranks, COVGPU_OK);
    std::vector<std::string> errs(n_ranks);
    std::vector<std::vector<uint8_t>> er(n_ranks);
    std::vector<std::vector<int32_t>> ll(n_ranks);
    std::vector<int64_t> cnt(2 * (size_t)n_ranks, 0);
    // Failure protocol. A rank that fails raises `fail`; the stages that cannot block (context creation, validation + upload of the
    // sub-problem) are separated from the next one by a host barrier after which EVERY rank checks the flag — so no rank enters
    // ncclCommInitRank or its first all-reduce while a peer has already given up. Inside the solve the peers poll the flag while they
    // wait for an iteration (wait_iteration) and abort their communicator; the in-process group is aborted directly.
    std::atomic<int> fail{0};
    struct HostBarrier {
      std::mutex m; std::condition_variable cv; int count = 0, n = 0; long gen = 0;
      void wait() { std::unique_lock<std::mutex> lk(m); const long g0 = gen; if (++count == n) { count = 0; ++gen; cv.notify_all(); } else cv.wait(lk, [&] { return gen != g0; }); }
    } bar;
    bar.n = n_ranks;
    auto work = [&](int r) {
      covgpu_context* c = nullptr;
      covgpu_options o = *opt; o.device = devices[r];
      int rc = COVGPU_OK;
      auto give_up = [&](int code) { if (rc == COVGPU_OK && code != COVGPU_OK) { rc = code; errs[r] = covgpu_last_error(); fail.store(1); if (grp) covgpu_group_abort(grp); } };
      give_up(covgpu_create(&o, &c));                                     // stage 1: a context on the rank's device
      bar.wait();
      if (!fail.load()) give_up(grp ? covgpu_set_shard_group(c, plan, r, grp) : covgpu_set_shard_rccl(c, plan, r, n_ranks, uid));   // stage 2: the collective (ncclCommInitRank: every rank is here)
      if (c) c->peer_fail = &fail;
      bar.wait();
      if (tr != nullptr) {
        // both rounds behind one call on this rank's share (upload, outlier round, device-side second round, solve, download into the share's arrays)
        if (!fail.load()) {
          er[r].assign(sub[r].obs_kf.size() + 1, 0); ll[r].assign(sub[r].lm_id.size() + 1, 0);
          give_up(gba_two_round_impl(c, &o, &sub[r].view, tr, er[r].data(), ll[r].data(), &cnt[2 * (size_t)r], &res1[r], &res[r]));
          if (c) c->have = false;
        }
        rcs[r] = rc;
        if (c) covgpu_destroy(c);
        return;
      }
      const auto t_up0 = std::chrono::steady_clock::now();
      if (!fail.load()) give_up(guarded([&] { return upload_impl(c, &o, &sub[r].view, false); }));  // (guarded: a host exception in a rank's thread would otherwise terminate the process with the peers parked at the barrier) stage 3: validation + H2D of the rank's share (OOM, malformed share)
      const double t_up = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_up0).count();
      bar.wait();
      if (!fail.load()) give_up(guarded([&] { return solve_any(c, &o, &res[r]); }));               // stage 4: the solve (peers of a rank that fails in here: wait_iteration)
      if (!fail.load() && rc == COVGPU_OK) {
        const auto t_dn0 = std::chrono::steady_clock::now();
        give_up(guarded([&] { return download_impl(c, &sub[r].view); }));
        res[r].t_download_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_dn0).count();
        res[r].t_upload_s = t_up;
      }
      if (!fail.load() && rc == COVGPU_OK && obs_erase) {
        give_up(guarded([&] {
          er[r].assign(sub[r].obs_kf.size() + 1, 0); ll[r].assign(sub[r].lm_id.size() + 1, 0);
          return covgpu_outlier_pass(c, outlier_threshold, er[r].data(), ll[r].data(), &cnt[2 * (size_t)r]);
        }));
      }
      rcs[r] = rc;
      if (c) covgpu_destroy(c);
    };
    std::vector<std::thread> th;
    for (int r = 1; r < n_ranks; ++r) th.emplace_back(work, r);
    work(0);
    for (auto& t : th) t.join();
    int rc = COVGPU_OK;
    for (int r = 0; r < n_ranks; ++r) if (rcs[r]) { rc = rcs[r]; g_err = "rank " + std::to_string(r) + ": " + errs[r]; break; }
    if (!rc && fail.load()) { rc = COVGPU_ERR_NO_DEVICE; g_err = "covgpu_gba_solve_multi: a rank gave up"; }
    if (!rc) {
      std::vector<int32_t> pr(p->num_kf), sr(p->num_kf);
      covgpu_nd_plan_owner(plan, pr.data(), sr.data());
      for (int k = 0; k < p->num_kf; ++k) {
        const int a = pr[k] < 0 ? 0 : pr[k], b = sr[k] < 0 ? 0 : sr[k];
        std::memcpy(p->kf_pose + 7 * (size_t)k, sub[a].pose.data() + 7 * (size_t)k, 7 * sizeof(double));
        if (p->kf_speed_bias) std::memcpy(p->kf_speed_bias + 9 * (size_t)k, sub[b].sb.data() + 9 * (size_t)k, 9 * sizeof(double));
      }
      if (counts) { counts[0] = 0; counts[1] = 0; }
      for (int r = 0; r < n_ranks; ++r) {
        for (size_t i = 0; i < sub[r].lm_id.size(); ++i) {
          std::memcpy(p->lm_pos + 3 * (size_t)sub[r].lm_id[i], sub[r].lm_pos.data() + 3 * i, 3 * sizeof(double));
          if (obs_erase && lm_left) lm_left[sub[r].lm_id[i]] = ll[r][i];
        }
        if (obs_erase) for (size_t i = 0; i < sub[r].obs_id.size(); ++i) obs_erase[sub[r].obs_id[i]] = er[r][i];
        if (counts) { counts[0] += cnt[2 * (size_t)r]; counts[1] += cnt[2 * (size_t)r + 1]; }
      }
      auto combine = [&](covgpu_result* dst, const std::vector<covgpu_result>& rs) {
        if (!dst) return;
        // the trust-region trace, costs and counts are identical on every rank (all-reduced scalars): rank 0's. Per-rank fields
        // are combined: IMU factors dropped for a non-PD covariance are counted where the factor lives (sum), timings are the slowest rank's
        *dst = rs[0];
        for (int r = 1; r < n_ranks; ++r) {
          dst->reserved += rs[r].reserved;
          dst->t_upload_s = std::max(dst->t_upload_s, rs[r].t_upload_s); dst->t_download_s = std::max(dst->t_download_s, rs[r].t_download_s);
          dst->t_solve_s = std::max(dst->t_solve_s, rs[r].t_solve_s);
        }
      };
      combine(out, res);
      if (tr != nullptr) combine(out1, res1);
    }
    return rc;
  });
}
extern "C" int covgpu_gba_solve_multi(const covgpu_options* opt, covgpu_problem* p, covgpu_result* out, int32_t n_ranks, const int32_t* devices,
                                      double outlier_threshold, uint8_t* obs_erase, int32_t* lm_left, int64_t* counts) {
  return gba_multi_impl(opt, p, out, n_ranks, devices, outlier_threshold, obs_erase, lm_left, counts, nullptr, nullptr);
}
// Both rounds of a GlobalBundleAdjustment call on n_ranks devices (round 6): ONE flatten and ONE upload per rank, the second round derived on every rank's
// device from its share (covgpu_gba_two_round's scheme); obs_erase / lm_left / counts / the estimates merged as covgpu_gba_solve_multi merges them.
extern "C" int covgpu_gba_two_round_multi(const covgpu_options* opt, covgpu_problem* p, const covgpu_two_round* tr, int32_t n_ranks, const int32_t* devices,
                                          uint8_t* obs_erase, int32_t* lm_left, int64_t* counts, covgpu_result* round1, covgpu_result* round2) {
  if (!tr || !obs_erase || !lm_left) { g_err = "covgpu_gba_two_round_multi: NULL argument"; return COVGPU_ERR_INVALID_ARG; }
  return gba_multi_impl(opt, p, round2, n_ranks, devices, tr->outlier_threshold, obs_erase, lm_left, counts, tr, round1);
}
