// facade_obscov_shim.cpp — C entry point for tests/test_gpu_obscov.py: OptimizationT::ObservationCovariances of
// include/covins_gpu/optimization_gpu.hpp on the stand-in map of facade_shim.cpp (whose entry points — shim_build, shim_free, ... — this
// library carries as well: a map built by either library is the same Handle).
#include "facade_shim.cpp"

extern "C" {

// The records of the facade in its order (the landmark-major observation order of the problem), at most `cap` of them: obs_cov [cap][4],
// cross [cap][18], ok [cap], lm_id / kf_id [cap][2] (the two halves of the id pair). *count = the number of records the facade returned.
// 0: done | 1: the facade threw, or cap is too small; the message goes to msg [256].
int shim_observation_covariances(Handle* h, int visual_only, double mu, long long cap, double* obs_cov, double* cross, unsigned char* ok,
                                 long long* lm_id, long long* kf_id, long long* count, long long* stats8, char* msg) {
  try {
    int64_t st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const auto r = Opt::ObservationCovariances(h->map, visual_only != 0, mu, st);
    *count = (long long)r.size();
    if ((long long)r.size() > cap) { std::snprintf(msg, 256, "%zu records, room for %lld", r.size(), cap); return 1; }
    for (size_t i = 0; i < r.size(); ++i) {
      std::memcpy(obs_cov + 4 * i, r[i].cov, 4 * sizeof(double));
      std::memcpy(cross + 18 * i, r[i].cross, 18 * sizeof(double));
      ok[i] = r[i].ok;
      lm_id[2 * i] = (long long)r[i].lm.first; lm_id[2 * i + 1] = (long long)r[i].lm.second;
      kf_id[2 * i] = (long long)r[i].kf.first; kf_id[2 * i + 1] = (long long)r[i].kf.second;
    }
    if (stats8) for (int i = 0; i < 8; ++i) stats8[i] = st[i];
    return 0;
  } catch (const std::exception& e) {
    std::snprintf(msg, 256, "%s", e.what());
    return 1;
  }
}

}  // extern "C"
