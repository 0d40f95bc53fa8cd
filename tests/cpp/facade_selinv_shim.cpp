// facade_selinv_shim.cpp — C entry point for tests/test_gpu_selinv.py: OptimizationT::KeyframeCovariances of
// include/covins_gpu/optimization_gpu.hpp on the stand-in map of facade_shim.cpp (whose entry points — shim_build, shim_free, ... — this
// library carries as well: a map built by either library is the same Handle).
#include "facade_shim.cpp"

extern "C" {

// Diagonal block of every keyframe (table order of shim_build) -> kf_cov [K][d][d], d = full && !visual_only ? 15 : 6, and the blocks of the
// pairs (rows_i[q], rows_j[q]) -> pair_cov [n][d][d], pair_ok [n]. 0: done | 1: the facade threw; the message goes to msg [256].
int shim_keyframe_covariances(Handle* h, int visual_only, int full, double mu, int n, const int* rows_i, const int* rows_j, double* kf_cov,
                              double* pair_cov, unsigned char* pair_ok, long long* stats8, char* msg) {
  try {
    std::vector<std::pair<Opt::idpair, Opt::idpair>> pairs;
    for (int q = 0; q < n; ++q) pairs.emplace_back(h->kfs[rows_i[q]]->id_, h->kfs[rows_j[q]]->id_);
    const auto r = Opt::KeyframeCovariances(h->map, visual_only != 0, full != 0, mu, pairs);
    const size_t dd = (size_t)r.d * r.d;
    for (size_t k = 0; k < h->kfs.size(); ++k) {
      const auto it = r.kf.find(h->kfs[k]->id_);
      if (it == r.kf.end()) throw std::runtime_error("a keyframe of the map has no block");
      std::memcpy(kf_cov + k * dd, it->second.data(), dd * sizeof(double));
    }
    for (int q = 0; q < n; ++q) { std::memcpy(pair_cov + q * dd, r.pair[q].data(), dd * sizeof(double)); pair_ok[q] = r.pair_ok[q]; }
    if (stats8) for (int i = 0; i < 8; ++i) stats8[i] = r.stats[i];
    return 0;
  } catch (const std::exception& e) {
    std::snprintf(msg, 256, "%s", e.what());
    return 1;
  }
}

}  // extern "C"
