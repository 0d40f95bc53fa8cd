// facade_lmcov_shim.cpp — C entry point for tests/test_gpu_lmcov.py: OptimizationT::LandmarkCovariances of
// include/covins_gpu/optimization_gpu.hpp on the stand-in map of facade_shim.cpp (whose entry points — shim_build, shim_free, ... — this
// library carries as well: a map built by either library is the same Handle).
#include "facade_shim.cpp"

namespace {
struct Mat3 {   // what the facade writes through operator()(r, c): Eigen::Matrix3d in COVINS
  double m[9] = {};
  double& operator()(int r, int c) { return m[3 * r + c]; }
  double operator()(int r, int c) const { return m[3 * r + c]; }
};
}  // namespace

extern "C" {

// Block of every landmark of the map (table order of shim_build) -> lm_cov [L][3][3]; present [L] = 1 where the facade returned a block (a
// landmark that is not in the problem, or whose lm_ok is 0, has none: its block stays as the caller left it). 0: done | 1: the facade
// threw; the message goes to msg [256].
int shim_landmark_covariances(Handle* h, int visual_only, double mu, double* lm_cov, unsigned char* present, long long* stats8, char* msg) {
  try {
    int64_t st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const auto r = Opt::LandmarkCovariances<Mat3>(h->map, visual_only != 0, mu, st);
    for (size_t l = 0; l < h->lms.size(); ++l) {
      const auto it = r.find(h->lms[l]->id_);
      present[l] = it != r.end();
      if (it != r.end()) std::memcpy(lm_cov + 9 * l, it->second.m, 9 * sizeof(double));
    }
    if (stats8) for (int i = 0; i < 8; ++i) stats8[i] = st[i];
    return 0;
  } catch (const std::exception& e) {
    std::snprintf(msg, 256, "%s", e.what());
    return 1;
  }
}

}  // extern "C"
