// lmcov_check_main.cpp — the argument checks of the landmark-covariance calls (covins_amd/csrc/lmcov_check.hpp) as a stand-alone host
// program: valid and malformed requests, one line per case ("ok" or the message). tests/test_lmcov_host.py compiles it with
// -fsanitize=address,undefined and compares the lines.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "lmcov_check.hpp"

static void line(const char* tag, const char* msg) { std::printf("%s: %s\n", tag, msg ? msg : "ok"); }

int main() {
  const int K = 4, L = 3;
  covgpu_problem p{};
  covgpu_options o{};
  p.num_kf = K; p.num_lm = L; p.num_obs = 7;
  std::vector<double> lm_cov((size_t)L * 9), kf_cov((size_t)K * 36);
  std::vector<uint8_t> ok(L);
  std::vector<int64_t> stats(8);
  covgpu_lmcov_t s{};
  s.mu = 0.0; s.lm_cov = lm_cov.data(); s.lm_ok = ok.data();
  line("plain", covgpu::lmcov_check(&p, &o, &s));
  s.kf_cov = kf_cov.data(); s.stats = stats.data();
  line("with kf_cov and stats", covgpu::lmcov_check(&p, &o, &s));
  s.mu = 1e300;
  line("large mu", covgpu::lmcov_check(&p, &o, &s));
  s.mu = -1e-300;
  line("negative mu", covgpu::lmcov_check(&p, &o, &s));
  s.mu = std::numeric_limits<double>::quiet_NaN();
  line("nan mu", covgpu::lmcov_check(&p, &o, &s));
  s.mu = std::numeric_limits<double>::infinity();
  line("inf mu", covgpu::lmcov_check(&p, &o, &s));
  s.mu = 0.0; s.lm_cov = nullptr;
  line("null lm_cov", covgpu::lmcov_check(&p, &o, &s));
  s.lm_cov = lm_cov.data(); s.lm_ok = nullptr;
  line("null lm_ok", covgpu::lmcov_check(&p, &o, &s));
  s.lm_ok = ok.data(); p.num_lm = 0;
  line("no landmarks", covgpu::lmcov_check(&p, &o, &s));
  p.num_lm = L; p.num_obs = 0;
  line("no observations", covgpu::lmcov_check(&p, &o, &s));
  p.num_obs = 7;
  line("request alone", covgpu::lmcov_request_check(&s));
  line("null problem", covgpu::lmcov_check(nullptr, &o, &s));
  line("null options", covgpu::lmcov_check(&p, nullptr, &s));
  line("null request", covgpu::lmcov_check(&p, &o, nullptr));
  line("restored", covgpu::lmcov_check(&p, &o, &s));
  return 0;
}
