// ncrelpose_check_main.cpp — the argument checks of the 17-point batch (covins_amd/csrc/ncrelpose_check.hpp) as a stand-alone host
// program: valid and malformed batches, one line per case ("ok" or the message). tests/test_ncrelpose_host.py compiles it with
// -fsanitize=address,undefined and compares the lines; the sanitizers watch the check walk corr_ptr, cell_ptr, the camera indices, the
// camera table and the bearings.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "ncrelpose_check.hpp"

static void line(const char* tag, const char* msg) { std::printf("%s: %s\n", tag, msg ? msg : "ok"); }

int main() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  // two jobs of 20 and 0 correspondences, 2 cells, 3 and 2 cameras
  std::vector<int32_t> ptr{0, 20, 20}, cell{0, 12, 20, 0, 0, 0}, cam_ptr{0, 3, 5}, c1(20, 0), c2(20, 2);
  std::vector<double> f1(60, 0.5), f2(60, 0.25), cam(60, 0.1), Tq(14, 0.5), Tc(14, 0.5), T(14), Tr(14), Ts(14), cov(72);
  std::vector<uint8_t> mask(20);
  std::vector<int32_t> inl(2), st(2), it(2), bd(2), cr(2), cd(2);
  std::vector<uint64_t> seed{7, 9};
  covgpu_ncrelpose_batch_t b{};
  covgpu_ncrelpose_opts o{1.5, 10.0, 100, 4000, 10.0, 30, 300, 0.99, 5, 0};
  b.num = 2; b.cells = 2; b.corr_ptr = ptr.data(); b.cell_ptr = cell.data(); b.bearing1 = f1.data(); b.bearing2 = f2.data(); b.cam1 = c1.data();
  b.cam2 = c2.data(); b.cam_ptr = cam_ptr.data(); b.cam = cam.data(); b.T_sc_q = Tq.data(); b.T_sc_c = Tc.data(); b.T_c1c2 = T.data();
  b.T_c1c2_ransac = Tr.data(); b.T_s1s2 = Ts.data(); b.cov = cov.data(); b.inlier = mask.data(); b.inliers = inl.data(); b.status = st.data();
  b.iterations = it.data(); b.best_draw = bd.data(); b.cov_rows = cr.data(); b.cov_draws = cd.data();
  auto chk = [&](const char* tag) {
    covgpu::NcrelposePlan P;
    line(tag, covgpu::ncrelpose_check(&b, &o, P));
    return P;
  };
  {
    const covgpu::NcrelposePlan P = chk("valid");
    std::printf("plan: %zu %zu %d %llu %llu %.17g %.17g\n", P.corr, P.cams, P.max_n, P.seeds[0], P.seeds[1], P.threshold, P.th_cov);
  }
  b.seed = seed.data();
  {
    const covgpu::NcrelposePlan P = chk("seeds");
    std::printf("plan: %llu %llu\n", P.seeds[0], P.seeds[1]);
  }
  b.seed = nullptr;
  { covgpu::NcrelposePlan P; line("null batch", covgpu::ncrelpose_check(nullptr, &o, P)); line("null options", covgpu::ncrelpose_check(&b, nullptr, P)); }
  b.num = -1; chk("negative num"); b.num = 0; chk("no jobs"); b.num = 2;
  o.max_iterations = 0; chk("max_iterations 0"); o.max_iterations = 100001; chk("max_iterations 100001"); o.max_iterations = 100000; chk("max_iterations 100000");
  o.max_iterations = 4000;
  o.cov_iters = 1; chk("cov_iters 1"); o.cov_iters = 257; chk("cov_iters 257"); o.cov_iters = 256; chk("cov_iters 256"); o.cov_iters = 2; chk("cov_iters 2");
  o.cov_iters = 30;
  o.cov_max_iters = -1; chk("cov_max_iters -1"); o.cov_max_iters = 300;
  o.min_inliers = -1; chk("min_inliers -1"); o.min_inliers = 100;
  o.stage_cap = -1; chk("stage_cap -1"); o.stage_cap = 0;
  o.probability = 0.0; chk("probability 0"); o.probability = 1.0; chk("probability 1"); o.probability = nan; chk("probability nan"); o.probability = 0.99;
  o.rp_error = 0.0; chk("rp_error 0"); o.rp_error = nan; chk("rp_error nan"); o.rp_error = 1.5;
  o.rp_error_cov = -1.0; chk("rp_error_cov negative"); o.rp_error_cov = inf; chk("rp_error_cov inf"); o.rp_error_cov = 10.0;
  o.cov_thres = nan; chk("cov_thres nan"); o.cov_thres = 10.0;
  b.cells = 0; chk("cells 0"); b.cells = 17; chk("cells 17"); b.cells = 2;
  b.corr_ptr = nullptr; chk("null corr_ptr"); b.corr_ptr = ptr.data();
  b.cell_ptr = nullptr; chk("null cell_ptr"); b.cell_ptr = cell.data();
  b.cam_ptr = nullptr; chk("null cam_ptr"); b.cam_ptr = cam_ptr.data();
  b.T_sc_q = nullptr; chk("null T_sc_q"); b.T_sc_q = Tq.data();
  b.cov = nullptr; chk("null cov"); b.cov = cov.data();
  b.cov_draws = nullptr; chk("null cov_draws"); b.cov_draws = cd.data();
  b.cam = nullptr; chk("null cam"); b.cam = cam.data();
  b.bearing1 = nullptr; chk("null bearing1"); b.bearing1 = f1.data();
  b.cam2 = nullptr; chk("null cam2"); b.cam2 = c2.data();
  b.inlier = nullptr; chk("null inlier"); b.inlier = mask.data();
  ptr[0] = 1; chk("first not 0"); ptr[0] = 0;
  ptr[2] = 19; chk("not monotone"); ptr[2] = 20;
  cam_ptr[0] = 1; chk("cam first not 0"); cam_ptr[0] = 0;
  cam_ptr[2] = 2; chk("cam not monotone"); cam_ptr[2] = 5;
  cell[0] = 1; chk("cell first not 0"); cell[0] = 0;
  cell[2] = 19; chk("cell short"); cell[2] = 20;
  cell[1] = 21; chk("cell not monotone"); cell[1] = 12;
  c1[19] = 3; chk("cam1 too large"); c1[19] = 0;
  c2[0] = -1; chk("cam2 negative"); c2[0] = 2;
  cam[59] = nan; chk("nan camera"); cam[59] = 0.1;
  Tq[13] = inf; chk("inf extrinsics"); Tq[13] = 0.5;
  for (int i = 0; i < 4; ++i) Tc[7 + i] = 0.0;
  chk("zero quaternion");
  for (int i = 0; i < 4; ++i) Tc[7 + i] = 0.5;
  f2[59] = nan; chk("nan bearing"); f2[59] = 0.25;
  f1[0] = inf; chk("inf bearing"); f1[0] = 0.5;
  chk("restored");
  std::vector<double> r1(6 * 17, 0.5), r2(6 * 17, 0.25), sv(3);
  line("solve n 0", covgpu::ncrelpose_solve_check(0, 17, nullptr, nullptr, nullptr, nullptr, nullptr));
  line("solve n -1", covgpu::ncrelpose_solve_check(-1, 17, nullptr, nullptr, nullptr, nullptr, nullptr));
  line("solve N 16", covgpu::ncrelpose_solve_check(1, 16, r1.data(), r2.data(), T.data(), st.data(), sv.data()));
  line("solve N 65", covgpu::ncrelpose_solve_check(1, 65, r1.data(), r2.data(), T.data(), st.data(), sv.data()));
  line("solve null", covgpu::ncrelpose_solve_check(1, 17, r1.data(), nullptr, T.data(), st.data(), sv.data()));
  line("solve ok", covgpu::ncrelpose_solve_check(1, 17, r1.data(), r2.data(), T.data(), st.data(), sv.data()));
  r2[6 * 17 - 1] = nan;
  line("solve nan", covgpu::ncrelpose_solve_check(1, 17, r1.data(), r2.data(), T.data(), st.data(), sv.data()));
  return 0;
}
