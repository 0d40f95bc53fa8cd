// lmcov_check.hpp — the argument checks of the landmark-covariance calls (lmcov.hip) and the shapes they share with the kernel (k_lmcov.hip).
// Plain C++17 like selinv_check.hpp: covgpu.h and the standard library, no HIP call and no HIP type, so the checks compile and run without a
// device. A check returns the message of the first violation, or nullptr.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/covgpu.h"

namespace covgpu {

constexpr int kLmcovMaxGroup = 16;    // widest lane group per landmark (covgpu_lm_group: 4 | 8 | 16)
constexpr int kLmcovThreads = 256;    // threads of a workgroup of the landmark pass: 256 / group landmarks

// The request alone (the resident form has no problem to check it against).
inline const char* lmcov_request_check(const covgpu_lmcov_t* s) {
  if (!s) return "NULL request";
  if (!s->lm_cov) return "NULL lm_cov";
  if (!s->lm_ok) return "NULL lm_ok";
  if (!std::isfinite(s->mu) || s->mu < 0.0) return "mu negative or not finite";
  return nullptr;
}

inline const char* lmcov_check(const covgpu_problem* p, const covgpu_options* o, const covgpu_lmcov_t* s) {
  if (!p || !o) return "NULL problem or options";
  if (const char* m = lmcov_request_check(s)) return m;
  if (p->num_lm <= 0 || p->num_obs <= 0) return "a problem without landmarks";
  return nullptr;
}

}  // namespace covgpu
