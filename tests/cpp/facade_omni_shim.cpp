// facade_omni_shim.cpp — the C++ facade (include/covins_gpu/optimization_gpu.hpp) on the stand-in map with the OPTIONAL camera_model
// trait: per keyframe a projection model and xi (what a COVINS binding reads from aslam's camera geometry). The stand-in
// map itself and its entry points (shim_build, shim_get_state, ...) are facade_shim.cpp's, compiled into this library as they are.
#include <unordered_map>
#include <utility>

#include "facade_shim.cpp"

namespace {
// camera model and xi of every keyframe (the stand-in Keyframe has no such fields: a side table, filled by omni_set_cameras)
std::unordered_map<const standin::Keyframe*, std::pair<int, double>> g_model;

struct OmniTypes : standin::Types {
  static bool camera_model(const standin::Keyframe& kf, int* model, double* xi) {
    auto it = g_model.find(&kf);
    if (it == g_model.end()) { *model = COVGPU_CAM_PINHOLE; *xi = 0.0; return true; }
    if (it->second.first != COVGPU_CAM_PINHOLE && it->second.first != COVGPU_CAM_UNIFIED) return false;
    *model = it->second.first; *xi = it->second.second;
    return true;
  }
};
using OptOmni = covins_gpu::OptimizationT<OmniTypes>;
}  // namespace

extern "C" {

// model / xi of keyframe k of the map arrays (h->kfs[k], the order shim_build got them in)
void omni_set_cameras(Handle* h, int K, const int* model, const double* xi) {
  for (int k = 0; k < K && k < (int)h->kfs.size(); ++k) g_model[h->kfs[k].get()] = {model[k], xi[k]};
}

// FlattenGBA through the omni binding: per IR keyframe its camera row, per camera row model / xi / fu fv cu cv; *has_model = 1 iff the
// problem handed to the library carries camera-model arrays (some camera unified)
int omni_flatten_cameras(Handle* h, int cap, int* ncam, int* kf_cam, int* model, double* xi, double* intr, int* has_model) {
  covins_gpu::detail::Flat f;
  OptOmni::Index ix;
  OptOmni::FlattenGBA(h->map, false, false, f, ix);
  covgpu_problem p = f.view();
  *ncam = p.num_cam;
  *has_model = p.cam_model != nullptr ? 1 : 0;
  for (int k = 0; k < p.num_kf && k < cap; ++k) kf_cam[k] = p.kf_cam[k];
  for (int c = 0; c < p.num_cam && c < cap; ++c) {
    model[c] = f.cam_model[c]; xi[c] = f.cam_xi[c];
    for (int i = 0; i < 4; ++i) intr[4 * c + i] = f.cam_intr[4 * c + i];
  }
  return 0;
}

void omni_gba(Handle* h, int iterations, int visual_only, int outlier_removal) {
  OptOmni::GlobalBundleAdjustment(h->map, iterations, -1.0, visual_only != 0, outlier_removal != 0, false);
}

}  // extern "C"
