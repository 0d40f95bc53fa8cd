// facade_abspose_shim.cpp — the C++ facade's Se3Solver (include/covins_gpu/optimization_gpu.hpp) on the stand-in map with the OPTIONAL
// bearing trait: per keyframe a table of unit bearings (what Keyframe::bearings_ holds in COVINS, keyframe_be.cpp:209-218). The stand-in
// map and its entry points (shim_build, ...) are facade_shim.cpp's, compiled into this library as they are.
#include <array>
#include <unordered_map>
#include <vector>

#include "facade_shim.cpp"

namespace {
std::unordered_map<const standin::Keyframe*, std::vector<std::array<double, 3>>> g_bearings;

struct BearingTypes : standin::Types {
  static bool bearing(const standin::Keyframe& kf, size_t i, double* out) {
    auto it = g_bearings.find(&kf);
    if (it == g_bearings.end() || i >= it->second.size()) return false;
    for (int k = 0; k < 3; ++k) out[k] = it->second[i][k];
    return true;
  }
};
using Se3 = covins_gpu::Se3SolverT<BearingTypes>;
}  // namespace

extern "C" {

// bearings [n][3] and octaves [n] of the features of keyframe kf (the stand-in's keypoints_aors_ holds the octave)
void abspose_set_features(Handle* h, int kf, int n, const double* bearing, const int* octave) {
  auto& v = g_bearings[h->kfs[kf].get()];
  v.assign(n, {0, 0, 0});
  auto& aors = h->kfs[kf]->keypoints_aors_;
  if ((int)aors.size() < n) aors.resize(n);
  for (int i = 0; i < n; ++i) { for (int k = 0; k < 3; ++k) v[i][k] = bearing[3 * i + k]; aors[i][1] = (float)octave[i]; }
}

// Se3Solver::projectiveAlignment of query keyframe kf: matches[i] = map landmark match_lm[i] (-1: NULL); kept[i] = the match survived;
// Tws16 row-major; *seed = the seed the facade derived. cand >= 0: through ProjectiveAlignmentBatch with that candidate keyframe.
int abspose_align(Handle* h, int kf, int cand, int n, const int* match_lm, double threshold, int min_inliers, int max_iter, double* Tws16,
                  unsigned char* kept, unsigned long long* seed) {
  std::vector<LandmarkPtr> m(n);
  for (int i = 0; i < n; ++i) if (match_lm[i] >= 0) m[i] = h->lms[match_lm[i]];
  Se3 solver(min_inliers, 0.5, max_iter);   // ransacProb is stored and not used, as in the reference
  Mat4 T;
  for (int i = 0; i < 16; ++i) T.m[i] = -1.0;
  bool found;
  if (cand < 0) {
    found = solver.projectiveAlignment(h->kfs[kf], m, threshold, T);
  } else {
    std::vector<Se3::AbsPoseJob> jobs(1);
    jobs[0].kf = h->kfs[kf]; jobs[0].kf_candidate = h->kfs[cand]; jobs[0].matches = &m; jobs[0].threshold = threshold; jobs[0].Tws = &T;
    solver.ProjectiveAlignmentBatch(jobs);
    found = jobs[0].found;
  }
  for (int i = 0; i < 16; ++i) Tws16[i] = T.m[i];
  for (int i = 0; i < n; ++i) kept[i] = m[i] ? 1 : 0;
  *seed = covins_gpu::detail::abspose_seed(h->kfs[kf].get(), cand < 0 ? (const standin::Keyframe*)nullptr : h->kfs[cand].get());
  return found ? 1 : 0;
}

}  // extern "C"
