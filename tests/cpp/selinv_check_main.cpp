// selinv_check_main.cpp — the argument checks of the selected-inverse calls (covins_amd/csrc/selinv_check.hpp) as a stand-alone host
// program: valid and malformed requests, one line per case ("ok" or the message). tests/test_selinv_host.py compiles it with
// -fsanitize=address,undefined and compares the lines; the sanitizers watch the check walk the pair arrays.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "selinv_check.hpp"

static void line(const char* tag, const char* msg) { std::printf("%s: %s\n", tag, msg ? msg : "ok"); }

int main() {
  const int K = 5;
  std::vector<uint8_t> fixed(K, 0);
  fixed[0] = 1;
  covgpu_problem p{};
  covgpu_options o{};
  p.num_kf = K;
  p.kf_fixed = fixed.data();
  std::vector<double> kf_cov((size_t)K * 15 * 15), pair_cov((size_t)3 * 15 * 15);
  std::vector<int32_t> pi{1, 2, 4}, pj{2, 1, 3};
  std::vector<uint8_t> ok(3);
  covgpu_selinv_t s{};
  s.block = 1; s.mu = 0.0; s.kf_cov = kf_cov.data();
  line("no pairs", covgpu::selinv_check(&p, &o, &s));
  s.num_pairs = 3; s.pair_i = pi.data(); s.pair_j = pj.data(); s.pair_cov = pair_cov.data(); s.pair_ok = ok.data();
  line("three pairs", covgpu::selinv_check(&p, &o, &s));
  s.mu = 1e300;
  line("large mu", covgpu::selinv_check(&p, &o, &s));
  s.mu = -1.0;
  line("negative mu", covgpu::selinv_check(&p, &o, &s));
  s.mu = std::numeric_limits<double>::quiet_NaN();
  line("nan mu", covgpu::selinv_check(&p, &o, &s));
  s.mu = 0.0; s.block = 2;
  line("block 2", covgpu::selinv_check(&p, &o, &s));
  s.block = 0; s.kf_cov = nullptr;
  line("null kf_cov", covgpu::selinv_check(&p, &o, &s));
  s.kf_cov = kf_cov.data(); s.pair_j = nullptr;
  line("null pair_j", covgpu::selinv_check(&p, &o, &s));
  s.pair_j = pj.data(); s.pair_ok = nullptr;
  line("null pair_ok", covgpu::selinv_check(&p, &o, &s));
  s.pair_ok = ok.data(); pi[2] = K;
  line("index K", covgpu::selinv_check(&p, &o, &s));
  pi[2] = -1;
  line("index -1", covgpu::selinv_check(&p, &o, &s));
  pi[2] = 3;
  line("equal", covgpu::selinv_check(&p, &o, &s));
  pi[2] = 0;
  line("fixed", covgpu::selinv_check(&p, &o, &s));
  line("fixed unknown", covgpu::selinv_request_check(K, nullptr, &s));
  pi[2] = 4; s.num_pairs = -1;
  line("negative count", covgpu::selinv_check(&p, &o, &s));
  s.num_pairs = 3;
  line("null problem", covgpu::selinv_check(nullptr, &o, &s));
  line("null request", covgpu::selinv_check(&p, &o, nullptr));
  line("restored", covgpu::selinv_check(&p, &o, &s));
  return 0;
}
