// fivept_check_main.cpp — the argument checks of the five-point batch (covins_amd/csrc/fivept_check.hpp) as a stand-alone host
// program: valid and malformed batches, one line per case ("ok" or the message). tests/test_fivept_host.py compiles it with
// -fsanitize=address,undefined and compares the lines; the sanitizers watch the check walk corr_ptr and the bearings.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "fivept_check.hpp"

static void line(const char* tag, const char* msg) { std::printf("%s: %s\n", tag, msg ? msg : "ok"); }

int main() {
  const double nan = std::numeric_limits<double>::quiet_NaN();
  std::vector<int32_t> ptr{0, 9, 9, 12};
  std::vector<double> f1(36, 0.5), f2(36, 0.25), T(21);
  std::vector<uint8_t> mask(12);
  std::vector<int32_t> inl(3), st(3);
  std::vector<uint64_t> seed{7, 8, 9};
  covgpu_fivept_batch_t b{};
  covgpu_fivept_opts o{20, 200, 0.99, 16.0, 4.5e-6, 5};
  b.num = 3; b.corr_ptr = ptr.data(); b.bearing1 = f1.data(); b.bearing2 = f2.data(); b.T_12 = T.data(); b.inlier = mask.data();
  b.inliers = inl.data(); b.status = st.data();
  auto chk = [&](const char* tag) {
    covgpu::FiveptPlan P;
    const char* m = covgpu::fivept_check(&b, &o, P);
    line(tag, m);
    return P;
  };
  {
    const covgpu::FiveptPlan P = chk("valid");
    std::printf("plan: %zu %d %llu %llu\n", P.corr, P.max_n, P.seeds[0], P.seeds[2]);
  }
  b.seed = seed.data();
  {
    const covgpu::FiveptPlan P = chk("seeds");
    std::printf("plan: %llu %llu\n", P.seeds[0], P.seeds[2]);
  }
  b.seed = nullptr;
  { covgpu::FiveptPlan P; line("null batch", covgpu::fivept_check(nullptr, &o, P)); line("null options", covgpu::fivept_check(&b, nullptr, P)); }
  b.num = -1; chk("negative num"); b.num = 0; chk("no jobs"); b.num = 3;
  o.max_iterations = 0; chk("max_iterations 0"); o.max_iterations = 100001; chk("max_iterations 100001"); o.max_iterations = 100000; chk("max_iterations 100000");
  o.max_iterations = 200;
  o.probability = 0.0; chk("probability 0"); o.probability = 1.0; chk("probability 1"); o.probability = nan; chk("probability nan"); o.probability = 0.99;
  o.threshold = 0.0; chk("threshold 0"); o.threshold = nan; chk("threshold nan"); o.threshold = 16.0;
  o.sigma = -1.0; chk("sigma negative"); o.sigma = std::numeric_limits<double>::infinity(); chk("sigma inf"); o.sigma = 4.5e-6;
  b.corr_ptr = nullptr; chk("null corr_ptr"); b.corr_ptr = ptr.data();
  b.T_12 = nullptr; chk("null T_12"); b.T_12 = T.data();
  b.inliers = nullptr; chk("null inliers"); b.inliers = inl.data();
  b.status = nullptr; chk("null status"); b.status = st.data();
  b.bearing1 = nullptr; chk("null bearing1"); b.bearing1 = f1.data();
  b.bearing2 = nullptr; chk("null bearing2"); b.bearing2 = f2.data();
  b.inlier = nullptr; chk("null inlier"); b.inlier = mask.data();
  ptr[0] = 1; chk("first not 0"); ptr[0] = 0;
  ptr[2] = 8; chk("not monotone"); ptr[2] = 9;
  f2[35] = nan; chk("nan bearing"); f2[35] = 0.25;
  f1[0] = std::numeric_limits<double>::infinity(); chk("inf bearing"); f1[0] = 0.5;
  chk("restored");
  line("solve n 0", covgpu::fivept_solve_check(0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
  line("solve n -1", covgpu::fivept_solve_check(-1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
  line("solve null", covgpu::fivept_solve_check(1, f1.data(), nullptr, T.data(), inl.data(), T.data(), st.data()));
  line("solve ok", covgpu::fivept_solve_check(1, f1.data(), f2.data(), T.data(), inl.data(), T.data(), st.data()));
  f1[23] = nan;
  line("solve nan", covgpu::fivept_solve_check(1, f1.data(), f2.data(), T.data(), inl.data(), T.data(), st.data()));
  return 0;
}
