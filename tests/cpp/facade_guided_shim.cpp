// facade_guided_shim.cpp — the C++ facade's guided matching (LoopMatcherT::SearchBySE3Batch / SearchByProjection,
// include/covins_gpu/optimization_gpu.hpp) on the stand-in map. The stand-in classes have no descriptors, image bounds, grid state,
// landmark descriptors / normals / scale distances and no RemapLandmark: the OPTIONAL traits supply them, from tables the test fills.
// The stand-in map and its entry points (shim_build, ...) are facade_shim.cpp's, compiled into this library as they are.
#include <array>
#include <cstdint>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "facade_shim.cpp"

namespace {
struct KfExtra {
  std::vector<uint8_t> desc;
  double bounds[4] = {0, 0, 0, 0}, grid[2] = {0, 0};
};
struct LmExtra {
  std::array<uint8_t, 32> desc;
  double normal[3], min_d, max_d;
};
std::unordered_map<const standin::Keyframe*, KfExtra> g_kf;
std::unordered_map<const standin::Landmark*, LmExtra> g_lm;
std::unordered_map<const standin::Landmark*, int> g_lm_index;

struct GuidedTypes : standin::Types {
  static bool descriptors(const standin::Keyframe& kf, int which, int* rows, const uint8_t** data) {
    auto it = g_kf.find(&kf);
    if (it == g_kf.end() || which != 0) return false;
    *rows = (int)(it->second.desc.size() / 32);
    *data = it->second.desc.data();
    return true;
  }
  static bool landmark_descriptor(const standin::Landmark& lm, uint8_t* out) {
    auto it = g_lm.find(&lm);
    if (it == g_lm.end()) return false;
    std::memcpy(out, it->second.desc.data(), 32);
    return true;
  }
  static void landmark_scale(const standin::Landmark& lm, double* n, double* mn, double* mx) {
    const LmExtra& e = g_lm.at(&lm);
    for (int k = 0; k < 3; ++k) n[k] = e.normal[k];
    *mn = e.min_d; *mx = e.max_d;
  }
  static void keyframe_image(const standin::Keyframe& kf, double* b, double* g) {
    const KfExtra& e = g_kf.at(&kf);
    for (int k = 0; k < 4; ++k) b[k] = e.bounds[k];
    g[0] = e.grid[0]; g[1] = e.grid[1];
  }
  // Keyframe::RemapLandmark (keyframe_be.cpp:484-495) on the stand-in classes
  static void remap_landmark(const KeyframePtr& kf, const LandmarkPtr& lm, size_t now, size_t to) {
    LandmarkPtr lm_new = kf->landmarks_[to];
    kf->landmarks_[now].reset();
    kf->landmarks_[to] = lm;
    lm->EraseObservation(kf);
    lm->AddObservation(kf, to);
    if (lm_new) lm_new->EraseObservation(kf);
  }
};
using Matcher = covins_gpu::LoopMatcherT<GuidedTypes>;

Mat4 pose7_to_mat(const double* p) {
  Mat4 T;
  covins_gpu::detail::pose_to_transform(p, T);
  return T;
}
}  // namespace

extern "C" {

void guided_set_params(int th_low, double scale_factor, int num_octaves, int agreement) {
  auto& g = Matcher::guided_params();
  g.th_low = th_low; g.scale_factor = scale_factor; g.num_octaves = num_octaves; g.agreement = agreement;
}

// per map landmark: descriptor, normal, min / max distance
void guided_set_landmarks(Handle* h, const uint8_t* desc, const double* normal, const double* min_d, const double* max_d) {
  for (size_t l = 0; l < h->lms.size(); ++l) {
    LmExtra e;
    std::memcpy(e.desc.data(), desc + 32 * l, 32);
    for (int k = 0; k < 3; ++k) e.normal[k] = normal[3 * l + k];
    e.min_d = min_d[l]; e.max_d = max_d[l];
    g_lm[h->lms[l].get()] = e;
    g_lm_index[h->lms[l].get()] = (int)l;
  }
}

// replaces the keypoint rows of keyframe kf: n keypoints with level, descriptor and landmark (map index or -1), bounds and grid state.
// The observations of the map's landmarks in this keyframe are rewritten to the new rows.
void guided_set_keyframe(Handle* h, int kf, int n, const float* kp, const int* level, const uint8_t* desc, const int* row_lm,
                         const double* bounds, const double* grid_inv) {
  KeyframePtr k = h->kfs[kf];
  for (auto& lm : k->landmarks_) if (lm) lm->EraseObservation(k);
  k->keypoints_distorted_.assign(n, {0.f, 0.f});
  k->keypoints_aors_.assign(n, {0.f, 0.f, 0.f, 0.f});
  k->landmarks_.assign(n, LandmarkPtr());
  for (int i = 0; i < n; ++i) {
    k->keypoints_distorted_[i] = {kp[2 * i], kp[2 * i + 1]};
    k->keypoints_aors_[i][1] = (float)level[i];
    if (row_lm[i] >= 0) { k->landmarks_[i] = h->lms[row_lm[i]]; h->lms[row_lm[i]]->AddObservation(k, (size_t)i); }
  }
  KfExtra& e = g_kf[k.get()];
  e.desc.assign(desc, desc + 32 * (size_t)n);
  for (int i = 0; i < 4; ++i) e.bounds[i] = bounds[i];
  e.grid[0] = grid_inv[0]; e.grid[1] = grid_inv[1];
}

// SearchBySE3Batch over J jobs. m12: per job the rows of kf1 back to back (offsets m12_ptr), in: the landmark matched so far (map index
// or -1), out: matches12 after the call.
void guided_se3(Handle* h, int J, const int* kf1, const int* kf2, const double* T12, const int* m12_ptr, int* m12, int* found, double th) {
  std::vector<Matcher::Se3SearchJob> jobs(J);
  std::vector<Matcher::LandmarkVector> m(J);
  std::vector<Mat4> T(J);
  for (int j = 0; j < J; ++j) {
    for (int i = m12_ptr[j]; i < m12_ptr[j + 1]; ++i) m[j].push_back(m12[i] >= 0 ? h->lms[m12[i]] : LandmarkPtr());
    T[j] = pose7_to_mat(T12 + 7 * j);
    jobs[j].kf1 = h->kfs[kf1[j]]; jobs[j].kf2 = h->kfs[kf2[j]]; jobs[j].matches12 = &m[j]; jobs[j].T12 = &T[j];
  }
  Matcher::SearchBySE3Batch(jobs, th);
  for (int j = 0; j < J; ++j) {
    for (int i = m12_ptr[j]; i < m12_ptr[j + 1]; ++i) { const LandmarkPtr& l = m[j][i - m12_ptr[j]]; m12[i] = l ? g_lm_index.at(l.get()) : -1; }
    found[j] = jobs[j].found;
  }
}

// SearchByProjection(kf, Tcw, points, matched, th): points / matched as map landmark indices (-1: none); matched is in/out
int guided_projection(Handle* h, int kf, const double* Tcw7, int P, const int* points, int n, int* matched, double th) {
  Matcher::LandmarkVector pts(P), mt(n);
  for (int p = 0; p < P; ++p) pts[p] = h->lms[points[p]];
  for (int i = 0; i < n; ++i) if (matched[i] >= 0) mt[i] = h->lms[matched[i]];
  const int nm = Matcher::SearchByProjection(h->kfs[kf], pose7_to_mat(Tcw7), pts, mt, th);
  for (int i = 0; i < n; ++i) matched[i] = mt[i] ? g_lm_index.at(mt[i].get()) : -1;
  return nm;
}

// the keyframe's landmark per row (map index or -1) and every map landmark's feature index in it (-1: not observed)
void guided_get_keyframe(Handle* h, int kf, int n, int* row_lm, int* feature_index) {
  KeyframePtr k = h->kfs[kf];
  for (int i = 0; i < n; ++i) row_lm[i] = k->landmarks_[i] ? g_lm_index.at(k->landmarks_[i].get()) : -1;
  for (size_t l = 0; l < h->lms.size(); ++l) feature_index[l] = h->lms[l]->GetFeatureIndex(k);
}

}  // extern "C"
