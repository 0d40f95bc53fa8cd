// selinv_check.hpp — the argument checks of the selected-inverse calls (selinv.hip) and the shapes they share with the kernels (k_selinv.hip).
// Plain C++17 like marginal_check.hpp: covgpu.h and the standard library, no HIP call and no HIP type, so the checks compile and run
// without a device. A check returns the message of the first violation, or nullptr.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/covgpu.h"

namespace covgpu {

constexpr int kSelBlock = 16;     // rows of a block step (one v_mfma_f64_16x16x4 tile)
constexpr int kSelPanel = 128;    // own columns one workgroup of a product works on

// The request against a problem of K keyframes whose constant poses are fixed[k] != 0 (fixed == nullptr: none).
inline const char* selinv_request_check(int K, const uint8_t* fixed, const covgpu_selinv_t* s) {
  if (!s) return "NULL request";
  if (s->block != 0 && s->block != 1) return "block outside {0, 1}";
  if (!std::isfinite(s->mu) || s->mu < 0.0) return "mu negative or not finite";
  if (!s->kf_cov) return "NULL kf_cov";
  if (s->num_pairs < 0) return "negative num_pairs";
  if (s->num_pairs > 0 && (!s->pair_i || !s->pair_j || !s->pair_cov || !s->pair_ok)) return "num_pairs > 0 with a NULL pair array";
  for (int64_t q = 0; q < s->num_pairs; ++q) {
    const int i = s->pair_i[q], j = s->pair_j[q];
    if (i < 0 || i >= K || j < 0 || j >= K) return "pair index out of range";
    if (i == j) return "a pair of equal indices";
    if (fixed && (fixed[i] || fixed[j])) return "a keyframe with a constant pose in a pair";
  }
  return nullptr;
}

inline const char* selinv_check(const covgpu_problem* p, const covgpu_options* o, const covgpu_selinv_t* s) {
  if (!p || !o) return "NULL problem or options";
  if (p->num_kf < 0) return "negative num_kf";
  return selinv_request_check(p->num_kf, p->kf_fixed, s);
}

}  // namespace covgpu
