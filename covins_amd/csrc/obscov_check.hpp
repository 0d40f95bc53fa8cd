// obscov_check.hpp — the argument checks of the observation-covariance calls (obscov.hip) and the shapes they share with the kernel
// (k_obscov.hip). Plain C++17 like lmcov_check.hpp: covgpu.h and the standard library, no HIP call and no HIP type, so the checks compile and
// run without a device. A check returns the message of the first violation, or nullptr.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/covgpu.h"
#include "lmcov_check.hpp"

namespace covgpu {

constexpr int kObscovMaxGroup = kLmcovMaxGroup;   // widest lane group per landmark (covgpu_lm_group: 4 | 8 | 16)
constexpr int kObscovThreads = kLmcovThreads;     // threads of a workgroup of the observation pass: 256 / group landmarks
constexpr int kObscovCrossDoubles = 18;           // Sigma_al, 6x3
constexpr int kObscovBlockDoubles = 4;            // C_o, 2x2

// The request alone (the resident form has no problem to check it against).
inline const char* obscov_request_check(const covgpu_obscov_t* s) {
  if (!s) return "NULL request";
  if (!s->obs_cov) return "NULL obs_cov";
  if (!s->obs_ok) return "NULL obs_ok";
  if (!std::isfinite(s->mu) || s->mu < 0.0) return "mu negative or not finite";
  if (s->lm_cov && !s->lm_ok) return "lm_cov without lm_ok";
  return nullptr;
}

inline const char* obscov_check(const covgpu_problem* p, const covgpu_options* o, const covgpu_obscov_t* s) {
  if (!p || !o) return "NULL problem or options";
  if (const char* m = obscov_request_check(s)) return m;
  if (p->num_lm <= 0 || p->num_obs <= 0) return "a problem without observations";
  return nullptr;
}

}  // namespace covgpu
