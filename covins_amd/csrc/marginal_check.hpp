// marginal_check.hpp — the argument checks of the marginal-covariance calls (marginal.hip) and the shapes they share with the kernels
// (k_marginal.hip). Plain C++17 like batch_check.hpp: covgpu.h and the standard library, no HIP call and no HIP type, so the checks
// compile and run without a device. A check returns the message of the first violation, or nullptr.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/covgpu.h"

namespace covgpu {

constexpr int kMargBlock = 16;     // rows of a block step, columns of a chunk (one v_mfma_f64_16x16x4 tile)
constexpr int kMargPanel = 128;    // own rows of a panel step: a front's own unknowns are substituted 128 at a time

// The selection against a problem of K keyframes whose constant poses are fixed[k] != 0 (fixed == nullptr: none).
inline const char* marginal_selection_check(int K, const uint8_t* fixed, const covgpu_marginal_t* m) {
  if (!m) return "NULL selection";
  if (m->num_kf < 1 || m->num_kf > COVGPU_MARGINAL_MAX_KF) return "num_kf outside [1, COVGPU_MARGINAL_MAX_KF]";
  if (!m->kf) return "NULL kf";
  if (m->block != 0 && m->block != 1) return "block outside {0, 1}";
  if (!std::isfinite(m->mu) || m->mu < 0.0) return "mu negative or not finite";
  if (!m->cov) return "NULL cov";
  for (int i = 0; i < m->num_kf; ++i) if (m->kf[i] < 0 || m->kf[i] >= K) return "keyframe index out of range";
  for (int i = 0; i < m->num_kf; ++i)
    for (int j = 0; j < i; ++j) if (m->kf[i] == m->kf[j]) return "duplicate keyframe";
  if (fixed) for (int i = 0; i < m->num_kf; ++i) if (fixed[m->kf[i]]) return "a keyframe with a constant pose has no covariance";
  return nullptr;
}

inline const char* marginal_check(const covgpu_problem* p, const covgpu_options* o, const covgpu_marginal_t* m) {
  if (!p || !o) return "NULL problem or options";
  if (p->num_kf < 0) return "negative num_kf";
  return marginal_selection_check(p->num_kf, p->kf_fixed, m);
}

}  // namespace covgpu
