// facade_marginal_shim.cpp — C entry points for tests/test_gpu_marginal.py: OptimizationT::MarginalCovariance and RelativePoseCovariance of
// include/covins_gpu/optimization_gpu.hpp on the stand-in map of facade_shim.cpp (whose entry points — shim_build, shim_free, ... — this
// library carries as well: a map built by either library is the same Handle).
#include "facade_shim.cpp"

extern "C" {

// Joint covariance of the keyframes rows[0..n) (table order of shim_build) -> cov [m][m], m = n * (full && !visual_only ? 15 : 6).
// 0: done | 1: the facade threw; the message goes to msg [256].
int shim_marginal(Handle* h, int n, const int* rows, int visual_only, int full, double mu, double* cov, long long* stats8, char* msg) {
  try {
    std::vector<Opt::idpair> ids;
    for (int i = 0; i < n; ++i) ids.push_back(h->kfs[rows[i]]->id_);
    int64_t st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const std::vector<double> c = Opt::MarginalCovariance(h->map, ids, visual_only != 0, full != 0, mu, st);
    std::memcpy(cov, c.data(), c.size() * sizeof(double));
    if (stats8) for (int i = 0; i < 8; ++i) stats8[i] = st[i];
    return 0;
  } catch (const std::exception& e) {
    std::snprintf(msg, 256, "%s", e.what());
    return 1;
  }
}

// One double array of the problem the facade's walk of the map leaves (the second round's problem), by its name in detail::Flat: returns its
// length, copies it if out != NULL; -1: no such array. Poses, camera extrinsics and loop measurements pass through a 4x4 transform on their way
// (quaternion -> matrix -> quaternion moves last bits), so a caller that wants the facade's bits from the C ABI hands it the facade's arrays.
int shim_marginal_ir(Handle* h, int visual_only, const char* name, double* out) {
  covins_gpu::detail::Flat f; Opt::Index ix;
  Opt::FlattenGBA(h->map, visual_only != 0, true, f, ix);
  const std::map<std::string, const std::vector<double>*> fields = {
      {"pose", &f.pose}, {"sb", &f.sb}, {"cam_extr", &f.cam_extr}, {"cam_intr", &f.cam_intr}, {"cam_dist", &f.cam_dist}, {"lm", &f.lm}, {"uv", &f.uv},
      {"sigma", &f.sigma}, {"samples", &f.samples}, {"first", &f.first}, {"noise", &f.noise}, {"meas", &f.meas}, {"info", &f.info}, {"loss", &f.loss}};
  const auto it = fields.find(name);
  if (it == fields.end()) return -1;
  if (out) std::memcpy(out, it->second->data(), it->second->size() * sizeof(double));
  return (int)it->second->size();
}

// J cov12 J^T of keyframes rows a, b from their joint pose covariance cov12 [12][12] -> out [6][6]
void shim_relative_pose_covariance(Handle* h, int a, int b, const double* cov12, double* out) {
  const std::vector<double> c(cov12, cov12 + 144);
  const auto r = Opt::RelativePoseCovariance(c, h->kfs[a]->GetPoseTws(), h->kfs[b]->GetPoseTws());
  std::memcpy(out, r.data(), 36 * sizeof(double));
}

}  // extern "C"
