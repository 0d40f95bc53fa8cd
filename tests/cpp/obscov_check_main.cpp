// obscov_check_main.cpp — the argument checks of the observation-covariance calls (covins_amd/csrc/obscov_check.hpp) as a stand-alone host
// program: valid and malformed requests, one line per case ("ok" or the message). tests/test_obscov_host.py compiles it with
// -fsanitize=address,undefined and compares the lines.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "obscov_check.hpp"

static void line(const char* tag, const char* msg) { std::printf("%s: %s\n", tag, msg ? msg : "ok"); }

int main() {
  const int K = 4, L = 3, O = 7;
  covgpu_problem p{};
  covgpu_options o{};
  p.num_kf = K; p.num_lm = L; p.num_obs = O;
  std::vector<double> obs_cov((size_t)O * 4), cross((size_t)O * 18), res((size_t)O * 2), lm_cov((size_t)L * 9), kf_cov((size_t)K * 36);
  std::vector<uint8_t> ok(O), lm_ok(L);
  std::vector<int64_t> stats(8);
  covgpu_obscov_t s{};
  s.mu = 0.0; s.obs_cov = obs_cov.data(); s.obs_ok = ok.data();
  line("plain", covgpu::obscov_check(&p, &o, &s));
  s.cross_cov = cross.data(); s.obs_res = res.data(); s.lm_cov = lm_cov.data(); s.lm_ok = lm_ok.data(); s.kf_cov = kf_cov.data(); s.stats = stats.data();
  line("with every output", covgpu::obscov_check(&p, &o, &s));
  s.lm_cov = nullptr;
  line("lm_ok alone", covgpu::obscov_check(&p, &o, &s));
  s.lm_cov = lm_cov.data(); s.lm_ok = nullptr;
  line("lm_cov without lm_ok", covgpu::obscov_check(&p, &o, &s));
  s.lm_ok = lm_ok.data();
  s.mu = 1e300;
  line("large mu", covgpu::obscov_check(&p, &o, &s));
  s.mu = -1e-300;
  line("negative mu", covgpu::obscov_check(&p, &o, &s));
  s.mu = std::numeric_limits<double>::quiet_NaN();
  line("nan mu", covgpu::obscov_check(&p, &o, &s));
  s.mu = std::numeric_limits<double>::infinity();
  line("inf mu", covgpu::obscov_check(&p, &o, &s));
  s.mu = 0.0; s.obs_cov = nullptr;
  line("null obs_cov", covgpu::obscov_check(&p, &o, &s));
  s.obs_cov = obs_cov.data(); s.obs_ok = nullptr;
  line("null obs_ok", covgpu::obscov_check(&p, &o, &s));
  s.obs_ok = ok.data(); p.num_lm = 0;
  line("no landmarks", covgpu::obscov_check(&p, &o, &s));
  p.num_lm = L; p.num_obs = 0;
  line("no observations", covgpu::obscov_check(&p, &o, &s));
  p.num_obs = O;
  line("request alone", covgpu::obscov_request_check(&s));
  line("null problem", covgpu::obscov_check(nullptr, &o, &s));
  line("null options", covgpu::obscov_check(&p, nullptr, &s));
  line("null request", covgpu::obscov_check(&p, &o, nullptr));
  line("restored", covgpu::obscov_check(&p, &o, &s));
  return 0;
}
