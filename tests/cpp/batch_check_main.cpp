// batch_check_main.cpp — drives every argument check of covins_amd/csrc/batch_check.hpp without a device. For each entry point it
// builds the smallest valid arguments, then applies one mutation per check and prints "entry<TAB>case<TAB>message" ("ok": no
// violation; an ok line of a planning check also carries what the plan derived). Every array has exactly the size its header
// comment promises, so a check that reads past one is caught by the sanitizers this program is built with
// (tests/test_batch_check_host.py compares the output with a table written from the messages of the entry points).
// Five returns have no case, because the smallest arguments that reach them are too large for a test that takes seconds: the grid
// limits of the two matchers (2^27 and 2^26 jobs: a gigabyte of job arrays), "more than 2^31 - 1 output rows" and "more than 2^31 - 1
// scan workgroups" of SearchBySE3 (2^23 and 2^31 tiles of 16 bytes pushed one by one) and "more than 2^31 - 1 database words" of
// the detect call (2^31 bow entries). The two matchers do take the output-row limit, which SearchBySE3 words the same way.
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "../../covins_amd/csrc/batch_check.hpp"

using namespace covgpu;

namespace {

const double kNaN = std::numeric_limits<double>::quiet_NaN(), kInf = std::numeric_limits<double>::infinity();

void emit(const char* entry, const char* name, const char* msg, const std::string& extra = "") {
  std::printf("%s\t%s\t%s%s\n", entry, name, msg ? msg : "ok", msg ? "" : extra.c_str());
  std::fflush(stdout);
}
template <class V> std::string list(const V& v) {
  std::string s = "[";
  for (size_t i = 0; i < v.size(); ++i) s += (i ? "," : "") + std::to_string(v[i]);
  return s + "]";
}

// One fixture per entry point: the arrays, the argument struct `a` over them and check(). CASE runs one mutation on a fresh fixture.
#define CASE(Fx, name, ...) do { Fx f; auto& a = f.a; (void)a; __VA_ARGS__; f.run(name); } while (0)

struct Relpose {
  std::vector<int32_t> ptr{0, 2, 3}, dist{0, 0, 0, 0}, inl{0, 0}, model{0, 0};
  std::vector<double> p = std::vector<double>(18, 1.0), kp = std::vector<double>(12, 1.0), sig = std::vector<double>(6, 1.0),
                      cam = std::vector<double>(32, 1.0), T = std::vector<double>(14, 0.0), xi{0.0, 0.0};
  std::vector<uint8_t> out = std::vector<uint8_t>(3, 0);
  covgpu_relpose_batch_t a{2, ptr.data(), p.data(), p.data() + 9, kp.data(), kp.data() + 6, sig.data(), sig.data() + 3, cam.data(), cam.data() + 16,
                           dist.data(), dist.data() + 2, T.data(), out.data(), inl.data(), nullptr, nullptr, nullptr, nullptr};
  const covgpu_relpose_batch_t* arg = &a;
  void run(const char* name) {
    RelposePlan P;
    const char* m = relpose_check(arg, P);
    emit("relpose", name, m, " corr=" + std::to_string(P.corr) + " unified=" + std::to_string(P.unified) + " model_b=" + list(P.model_b) + " xi_b=" + list(P.xi_b));
  }
};

struct Abspose {
  std::vector<int32_t> ptr{0, 2, 3}, inl{0, 0}, it{0, 0}, bd{0, 0};
  std::vector<double> f = std::vector<double>(9, 0.5), pw = std::vector<double>(9, 2.0), sig = std::vector<double>(3, 1.0), T = std::vector<double>(14, 0.0);
  std::vector<uint8_t> mask = std::vector<uint8_t>(3, 0);
  std::vector<uint64_t> seed{11, 12};
  covgpu_abspose_batch_t a{2, ptr.data(), f.data(), pw.data(), sig.data(), nullptr, T.data(), mask.data(), inl.data(), it.data(), bd.data()};
  covgpu_ransac_opts o{6, 300, 0.99, 25.0, 5};
  const covgpu_abspose_batch_t* arg = &a;
  const covgpu_ransac_opts* opt = &o;
  void run(const char* name) {
    AbsposePlan P;
    const char* m = abspose_check(arg, opt, P);
    emit("abspose", name, m, " corr=" + std::to_string(P.corr) + " max_n=" + std::to_string(P.max_n) + " seeds=" + list(P.seeds));
  }
};

struct P3p {
  std::vector<double> f = std::vector<double>(12, 0.5), pw = std::vector<double>(12, 2.0), T = std::vector<double>(28, 0.0);
  std::vector<int32_t> ns{0}, ch{0};
  struct { int32_t n; const double *f, *P, *T; const int32_t *nsol, *chosen; } a{1, f.data(), pw.data(), T.data(), ns.data(), ch.data()};
  void run(const char* name) { emit("p3p", name, p3p_check(a.n, a.f, a.P, a.T, a.nsol, a.chosen)); }
};

// the two matchers: sets of 3 and 2 rows, one job (set 0 against set 1)
template <class Batch, class Elem> struct MatchBase {
  std::vector<int32_t> ptr{0, 3, 5}, sa{0}, sb{1}, match{0, 0, 0}, nm{0};
  std::vector<Elem> desc;
  Batch a;
  covgpu_match_opts o;
  const Batch* arg = &a;
  const covgpu_match_opts* opt = &o;
  // `jobs` jobs, the first of set 0 and the others of set 1 against themselves, the sets holding `rows0` and 0 rows
  void many_jobs(size_t jobs, int rows0, size_t elems_per_row) {
    ptr = {0, rows0, rows0};
    desc.assign((size_t)rows0 * elems_per_row, Elem(1));
    sa.assign(jobs, 1); sa[0] = 0;
    a.row_ptr = ptr.data(); a.desc = desc.data(); a.num_jobs = (int32_t)jobs; a.set_a = a.set_b = sa.data();
  }
  static std::string plan(const MatchPlan& P) {
    return " rows=" + std::to_string(P.rows) + " total_a=" + std::to_string(P.total_a) + " max_a=" + std::to_string(P.max_a) + " max_b=" + std::to_string(P.max_b) +
           " off=" + list(P.off);
  }
};
struct Match : MatchBase<covgpu_match_batch_t, uint8_t> {
  std::vector<int32_t> dist{0, 0, 0};
  std::vector<uint8_t> skip = std::vector<uint8_t>(5, 0);
  Match() {
    desc.assign(5 * 32, 1);
    a = covgpu_match_batch_t{2, ptr.data(), desc.data(), nullptr, 1, sa.data(), sb.data(), match.data(), dist.data(), nm.data()};
    o = covgpu_match_opts{COVGPU_MATCH_DENSE, 50.0f, 0.8f};
  }
  void run(const char* name) { MatchPlan P; const char* m = match_check(arg, opt, P); emit("match", name, m, plan(P)); }
};
struct MatchFloat : MatchBase<covgpu_match_float_batch_t, float> {
  std::vector<float> dist{0, 0, 0};
  MatchFloat() {
    desc.assign(5 * 4, 1.0f);
    a = covgpu_match_float_batch_t{2, ptr.data(), 4, desc.data(), 1, sa.data(), sb.data(), match.data(), dist.data(), nm.data()};
    o = covgpu_match_opts{COVGPU_MATCH_KNN2, 500.0f, 0.8f};
  }
  void run(const char* name) { MatchPlan P; const char* m = match_float_check(arg, opt, P); emit("match_float", name, m, plan(P)); }
};

// keypoint sets of 3 and 2 rows
struct Sets {
  std::vector<int32_t> ptr{0, 3, 5}, level = std::vector<int32_t>(5, 0);
  std::vector<float> kp = std::vector<float>(10, 1.0f);
  std::vector<uint8_t> desc = std::vector<uint8_t>(160, 1);
  std::vector<double> bounds = std::vector<double>(8, 0.0);
  covgpu_keypoint_sets_t sets() { return covgpu_keypoint_sets_t{2, ptr.data(), kp.data(), level.data(), desc.data(), bounds.data(), nullptr}; }
  static std::string tiles(const GuidedPlan& P) {
    std::string s = " tiles=";
    for (const GuidedTile& t : P.tiles) s += "(" + std::to_string(t.job) + "," + std::to_string(t.dir) + "," + std::to_string(t.first) + "," + std::to_string(t.count) + ")";
    return s;
  }
};
struct Se3 : Sets {
  std::vector<double> K = std::vector<double>(8, 1.0), pos = std::vector<double>(15, 1.0), maxd = std::vector<double>(5, 1.0), T{0, 0, 0, 1, 0, 0, 0};
  std::vector<uint8_t> ldesc = std::vector<uint8_t>(160, 1), lfree = std::vector<uint8_t>(5, 1);
  std::vector<int32_t> s1{0}, s2{1}, match{0, 0, 0}, m1{0, 0, 0}, m2{0, 0}, nf{0};
  covgpu_search_se3_batch_t a{sets(), K.data(), pos.data(), maxd.data(), ldesc.data(), lfree.data(), 1, s1.data(), s2.data(), T.data(), match.data(), m1.data(),
                              m2.data(), nf.data()};
  covgpu_guided_opts o{50, 9.5, 2.0, 1, 0};
  const covgpu_search_se3_batch_t* arg = &a;
  const covgpu_guided_opts* opt = &o;
  void run(const char* name) {
    GuidedPlan P;
    const char* m = search_se3_check(arg, opt, P);
    emit("search_se3", name, m, " rows=" + std::to_string(P.rows) + " tot1=" + std::to_string(P.tot1) + " tot2=" + std::to_string(P.tot2) + " off1=" + list(P.off1) +
                                    " off2=" + list(P.off2) + tiles(P));
  }
};
struct Proj : Sets {
  std::vector<double> cam = std::vector<double>(16, 1.0), xi{0.0, 0.5}, T{0, 0, 0, 1, 0, 0, 0}, pw = std::vector<double>(6, 1.0), nrm = std::vector<double>(6, 1.0),
                      mind{1, 1}, maxd{2, 2};
  std::vector<int32_t> dt{0, 1}, cm{0, 0}, set{0}, pp{0, 2}, ex{-1, 2}, claimed{0, 0}, remap{0, 0}, bd{0, 0}, nm{0};
  std::vector<uint8_t> pdesc = std::vector<uint8_t>(64, 1), taken = std::vector<uint8_t>(5, 0);
  covgpu_search_projection_batch_t a{sets(), nullptr, cam.data(), dt.data(), nullptr, nullptr, 1, set.data(), T.data(), pp.data(), pw.data(), nrm.data(),
                                     mind.data(), maxd.data(), pdesc.data(), nullptr, nullptr, claimed.data(), remap.data(), bd.data(), nm.data()};
  covgpu_guided_opts o{50, 10.0, 2.0, 1, 0};
  const covgpu_search_projection_batch_t* arg = &a;
  const covgpu_guided_opts* opt = &o;
  void run(const char* name) {
    GuidedPlan P;
    const char* m = search_projection_check(arg, opt, P);
    emit("search_projection", name, m, " rows=" + std::to_string(P.rows) + " points=" + std::to_string(P.points) + " xi=" + list(P.xi) + tiles(P));
  }
};

struct Reanchor {
  std::vector<double> po = std::vector<double>(21, 0.0), pn = std::vector<double>(21, 0.0), lm = std::vector<double>(6, 0.0);
  std::vector<int32_t> ref{2, -1};
  struct { int32_t K; const double *po, *pn; int32_t L; const int32_t* ref; const double* lm; } a{3, po.data(), pn.data(), 2, ref.data(), lm.data()};
  void run(const char* name) { emit("pgo_reanchor", name, reanchor_check(a.K, a.po, a.pn, a.L, a.ref, a.lm)); }
};

// a root and two leaves
struct Vocab {
  std::vector<int32_t> parent{-1, 0, 0}, cptr{0, 2, 2, 2}, child{1, 2}, wid{-1, 0, 1};
  std::vector<uint8_t> vdesc = std::vector<uint8_t>(96, 1);
  std::vector<double> weight{0.0, 1.0, 1.0};
  covgpu_bow_vocab_t v{3, 2, 2, 1, COVGPU_BOW_L1_NORM, COVGPU_BOW_TF_IDF, parent.data(), cptr.data(), child.data(), vdesc.data(), wid.data(), weight.data()};
};
struct VocabOnly : Vocab {
  covgpu_bow_vocab_t& a = v;
  const covgpu_bow_vocab_t* arg = &v;
  void run(const char* name) { emit("bow_vocab", name, bow_vocab_check(arg)); }
};
struct Transform : Vocab {
  std::vector<int32_t> ptr{0, 3, 5}, bptr{0, 0, 0}, word = std::vector<int32_t>(5, 0), rw = std::vector<int32_t>(5, 0), rn = std::vector<int32_t>(5, 0);
  std::vector<uint8_t> desc = std::vector<uint8_t>(160, 1);
  std::vector<double> value = std::vector<double>(5, 0.0);
  int64_t total = 0;
  covgpu_bow_transform_batch_t a{2, ptr.data(), desc.data(), 0, 5, bptr.data(), word.data(), value.data(), &total, rw.data(), rn.data()};
  const covgpu_bow_vocab_t* voc = &v;
  const covgpu_bow_transform_batch_t* arg = &a;
  void run(const char* name) { size_t rows = 0; const char* m = bow_transform_check(voc, arg, rows); emit("bow_transform", name, m, " rows=" + std::to_string(rows)); }
};

// three bow vectors: {0: .5, 1: .5}, {1: 1}, {}
struct BowCsr {
  std::vector<int32_t> bptr{0, 2, 3, 3}, word{0, 1, 1};
  std::vector<double> value{0.5, 0.5, 1.0};
};
struct Score : BowCsr {
  std::vector<int32_t> pa{0, 1}, pb{1, 2};
  std::vector<double> score{0, 0};
  struct { int32_t n; const int32_t *ptr, *word; const double* value; int32_t np; const int32_t *a, *b; const double* score; } a{
      3, bptr.data(), word.data(), value.data(), 2, pa.data(), pb.data(), score.data()};
  void run(const char* name) { emit("bow_score_pairs", name, bow_score_pairs_check(a.n, a.ptr, a.word, a.value, a.np, a.a, a.b, a.score)); }
};
struct Detect : BowCsr {
  std::vector<int32_t> id{7, 8, 9}, client{0, 0, 1}, nptr{0, 1, 2, 3}, nb{1, 0, 0}, db{1, 0}, qk{0}, vis{2}, nc{0}, cand{0, 0}, nsh{0}, mcw{0}, nsc{0};
  std::vector<uint8_t> invalid{0, 0, 0};
  std::vector<float> acc{0, 0};
  std::vector<double> ms{0}, msin{0.1};
  covgpu_detect_batch_t a{3, id.data(), client.data(), bptr.data(), word.data(), value.data(), nptr.data(), nb.data(), nullptr, 2, db.data(), 1, qk.data(), vis.data(),
                          nullptr, 2, nc.data(), cand.data(), acc.data(), ms.data(), nsh.data(), mcw.data(), nsc.data()};
  covgpu_detect_opts o{0.8, 100, 7, 0, 0};
  const covgpu_detect_batch_t* arg = &a;
  const covgpu_detect_opts* opt = &o;
  void run(const char* name) {
    DetectPlan P;
    const char* m = detect_check(arg, opt, P);
    emit("detect_candidates", name, m, " num_nb=" + std::to_string(P.num_nb) + " max_words=" + std::to_string(P.max_words) + " pos_of=" + list(P.pos_of) +
                                           " pairs=" + list(P.pair_a) + list(P.pair_b) + list(P.pair_off) + " inv=" + list(P.inv_ptr) + list(P.inv_pos));
  }
};

// K = 3 keyframes in a chain, L = 2 landmarks, O = 3 observations
struct Prune {
  std::vector<int32_t> ptr{0, 2, 3}, okf{0, 1, 2}, pred{-1, 0, 1}, succ{1, 2, -1}, rkf{0, 0, 0}, ract{0, 0, 0};
  std::vector<double> time{0.0, 1.0, 2.0};
  covgpu_prune_t a{3, 2, ptr.data(), okf.data(), nullptr, nullptr, nullptr, nullptr, nullptr, pred.data(), succ.data(), time.data(), 3, rkf.data(), ract.data(),
                   nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  covgpu_prune_opts o{0.95, 1.0, -1, 0};
  const covgpu_prune_t* arg = &a;
  const covgpu_prune_opts* opt = &o;
  void run(const char* name) { emit("prune", name, prune_check(arg, opt)); }
};
struct Refresh {
  std::vector<int32_t> ptr{0, 2, 3}, okf{0, 1, 2}, ooc{0, 1, 0}, ref{1, -1};
  std::vector<double> pos = std::vector<double>(6, 1.0), cen = std::vector<double>(9, 0.0);
  covgpu_landmark_refresh_t a{3, 2, ptr.data(), okf.data(), nullptr, ooc.data(), ref.data(), pos.data(), cen.data(), nullptr, nullptr, nullptr, nullptr, nullptr,
                              nullptr, nullptr, nullptr, nullptr, nullptr};
  covgpu_landmark_refresh_opts o{2.0, 1};
  const covgpu_landmark_refresh_t* arg = &a;
  const covgpu_landmark_refresh_opts* opt = &o;
  void run(const char* name) { emit("landmark_refresh", name, lm_refresh_check(arg, opt)); }
};
struct VocTrain {
  std::vector<int32_t> ptr{0, 3, 5}, parent = std::vector<int32_t>(4, 0), wid = std::vector<int32_t>(4, 0);
  std::vector<uint8_t> desc = std::vector<uint8_t>(160, 1), dout = std::vector<uint8_t>(128, 0);
  std::vector<double> weight = std::vector<double>(4, 0.0);
  int32_t nn = 0, nw = 0;
  covgpu_voc_train_t a{2, ptr.data(), desc.data(), 4, &nn, &nw, parent.data(), dout.data(), wid.data(), weight.data(), nullptr, nullptr};
  covgpu_voc_train_opts o{10, 5, COVGPU_BOW_TF_IDF, COVGPU_BOW_L1_NORM, 0, 100, 65536};
  const covgpu_voc_train_t* arg = &a;
  const covgpu_voc_train_opts* opt = &o;
  void run(const char* name) { emit("voc_train", name, voc_train_check(arg, opt)); }
};

// the camera check as the solver's upload uses it: two cameras, the second unified
struct UploadCam {
  std::vector<int32_t> model{COVGPU_CAM_PINHOLE, COVGPU_CAM_UNIFIED};
  std::vector<double> xi{kNaN, 0.5};   // (the pinhole camera's xi is not read)
  struct { const int32_t* model; const double* xi; } a{model.data(), xi.data()};
  void run(const char* name) {
    const char* m = nullptr;
    for (size_t i = 0; i < 2 && !m; ++i) m = cam_check(a.model, a.xi, i, kNoCamXi);
    emit("upload_cam", name, m);
  }
};

// the descriptor-set cases that the two matchers, the guided searches and the BoW transform share (fixtures with `ptr` as row_ptr)
#define ROW_PTR_CASES(Fx)                                   \
  CASE(Fx, "row_ptr_first", f.ptr[0] = 1);                  \
  CASE(Fx, "row_ptr_not_monotone", f.ptr[1] = 6);           \
  CASE(Fx, "set_too_long", f.ptr = {0, 4097, 4099})

}  // namespace

int main() {
  CASE(Relpose, "valid", );
  CASE(Relpose, "zero_pairs", a.num_pairs = 0; a.corr_ptr = nullptr);
  CASE(Relpose, "empty_last_pair", f.ptr[2] = 2);
  CASE(Relpose, "corr_ptr_first_not_zero", f.ptr = {1, 2, 3});            // accepted: corr_ptr[0] == 0 is not required here
  CASE(Relpose, "unified_b", a.cam_model_b = f.model.data(); a.xi_b = f.xi.data(); f.model[1] = COVGPU_CAM_UNIFIED; f.xi = {kNaN, 0.25});
  CASE(Relpose, "null_batch", f.arg = nullptr);
  CASE(Relpose, "negative_pairs", a.num_pairs = -1);
  CASE(Relpose, "null_inliers", a.inliers = nullptr);
  CASE(Relpose, "corr_ptr_not_monotone", f.ptr[1] = 4);
  CASE(Relpose, "unknown_model", a.cam_model_b = f.model.data(); f.model[1] = 2);
  CASE(Relpose, "unknown_model_before_missing_xi", a.cam_model_a = a.cam_model_b = f.model.data(); f.model = {COVGPU_CAM_UNIFIED, 7});
  CASE(Relpose, "unified_without_xi", a.cam_model_a = f.model.data(); f.model[0] = COVGPU_CAM_UNIFIED);
  CASE(Relpose, "xi_negative", a.cam_model_a = f.model.data(); a.xi_a = f.xi.data(); f.model[0] = COVGPU_CAM_UNIFIED; f.xi[0] = -0.1);
  CASE(Relpose, "xi_nan", a.cam_model_a = f.model.data(); a.xi_a = f.xi.data(); f.model[1] = COVGPU_CAM_UNIFIED; f.xi[1] = kNaN);
  CASE(Relpose, "null_outlier", a.outlier = nullptr);

  CASE(Abspose, "valid", );
  CASE(Abspose, "seeds_given", a.seed = f.seed.data());
  CASE(Abspose, "zero_candidates", a.num = 0; a.corr_ptr = nullptr);
  CASE(Abspose, "empty_last_candidate", f.ptr[2] = 2);
  CASE(Abspose, "null_options", f.opt = nullptr);
  CASE(Abspose, "negative_num", a.num = -1);
  CASE(Abspose, "max_iterations_zero", f.o.max_iterations = 0);
  CASE(Abspose, "max_iterations_too_large", f.o.max_iterations = 100001);
  CASE(Abspose, "probability_one", f.o.probability = 1.0);
  CASE(Abspose, "threshold_nan", f.o.threshold = kNaN);
  CASE(Abspose, "null_T_wc", a.T_wc = nullptr);
  CASE(Abspose, "corr_ptr_first", f.ptr[0] = 1);
  CASE(Abspose, "corr_ptr_not_monotone", f.ptr[1] = 4);
  CASE(Abspose, "null_inlier", a.inlier = nullptr);
  CASE(Abspose, "bearing_inf", f.f[8] = kInf);
  CASE(Abspose, "point_nan", f.pw[0] = kNaN);

  CASE(P3p, "valid", );
  CASE(P3p, "zero", a.n = 0; a.f = nullptr);
  CASE(P3p, "negative_n", a.n = -1);
  CASE(P3p, "null_chosen", a.chosen = nullptr);
  CASE(P3p, "point_nan", f.pw[11] = kNaN);

  CASE(Match, "valid", );
  CASE(Match, "knn2", f.o.mode = COVGPU_MATCH_KNN2);
  CASE(Match, "zero_sets", a.num_sets = 0; a.num_jobs = 0; a.row_ptr = nullptr);
  CASE(Match, "zero_jobs", a.num_jobs = 0; a.set_a = nullptr);
  CASE(Match, "empty_last_set", f.ptr[2] = 3);
  CASE(Match, "null_batch", f.arg = nullptr);
  CASE(Match, "unknown_mode", f.o.mode = 2);
  CASE(Match, "dist_threshold_zero", f.o.dist_threshold = 0.0f);
  CASE(Match, "ratio_inf", f.o.ratio = (float)kInf);
  CASE(Match, "negative_jobs", a.num_jobs = -1);
  CASE(Match, "skip_in_knn2", f.o.mode = COVGPU_MATCH_KNN2; a.skip = f.skip.data());
  CASE(Match, "null_row_ptr", a.row_ptr = nullptr);
  ROW_PTR_CASES(Match);
  CASE(Match, "null_desc", a.desc = nullptr);
  CASE(Match, "null_nmatches", a.nmatches = nullptr);
  CASE(Match, "set_index_out_of_range", f.sb[0] = 2);
  CASE(Match, "too_many_output_rows", f.many_jobs(524288, 4096, 32); std::fill(f.sa.begin(), f.sa.end(), 0));
  CASE(Match, "null_match", a.match = nullptr);

  CASE(MatchFloat, "valid", );
  CASE(MatchFloat, "zero_sets", a.num_sets = 0; a.num_jobs = 0; a.row_ptr = nullptr);
  CASE(MatchFloat, "zero_jobs", a.num_jobs = 0; a.set_a = nullptr);
  CASE(MatchFloat, "empty_last_set", f.ptr[2] = 3);
  CASE(MatchFloat, "null_options", f.opt = nullptr);
  CASE(MatchFloat, "dense_mode", f.o.mode = COVGPU_MATCH_DENSE);
  CASE(MatchFloat, "dist_threshold_nan", f.o.dist_threshold = (float)kNaN);
  CASE(MatchFloat, "ratio_zero", f.o.ratio = 0.0f);
  CASE(MatchFloat, "dim_not_multiple_of_4", a.dim = 6);
  CASE(MatchFloat, "dim_too_large", a.dim = 260);
  CASE(MatchFloat, "negative_sets", a.num_sets = -1);
  CASE(MatchFloat, "null_row_ptr", a.row_ptr = nullptr);
  ROW_PTR_CASES(MatchFloat);
  CASE(MatchFloat, "null_desc", a.desc = nullptr);
  CASE(MatchFloat, "null_set_b", a.set_b = nullptr);
  CASE(MatchFloat, "set_index_out_of_range", f.sa[0] = -1);
  CASE(MatchFloat, "too_many_output_rows", f.many_jobs(524288, 4096, 4); std::fill(f.sa.begin(), f.sa.end(), 0));
  CASE(MatchFloat, "null_match", a.match = nullptr);
  CASE(MatchFloat, "descriptor_nan", f.desc[19] = (float)kNaN);
  CASE(MatchFloat, "descriptor_too_large", f.desc[0] = -1e19f);

  CASE(Se3, "valid", );
  CASE(Se3, "zero_sets", a.sets.num_sets = 0; a.num_jobs = 0; a.sets.row_ptr = nullptr);
  CASE(Se3, "zero_jobs", a.num_jobs = 0; a.set_1 = nullptr);
  CASE(Se3, "empty_last_set", f.ptr[2] = 3; a.sets = f.sets());
  CASE(Se3, "null_batch", f.arg = nullptr);
  CASE(Se3, "null_options", f.opt = nullptr);
  CASE(Se3, "th_low_256", f.o.th_low = 256);
  CASE(Se3, "radius_zero", f.o.radius = 0.0);
  CASE(Se3, "num_octaves_zero", f.o.num_octaves = 0);
  CASE(Se3, "scale_factor_one", f.o.num_octaves = 2; f.o.scale_factor = 1.0);
  CASE(Se3, "agreement_two", f.o.agreement = 2);
  CASE(Se3, "negative_sets", a.sets.num_sets = -1);
  CASE(Se3, "null_row_ptr", a.sets.row_ptr = nullptr);
  ROW_PTR_CASES(Se3);
  CASE(Se3, "null_bounds", a.sets.bounds = nullptr);
  CASE(Se3, "null_level", a.sets.level = nullptr);
  CASE(Se3, "negative_jobs", a.num_jobs = -1);
  CASE(Se3, "null_K", a.K = nullptr);
  CASE(Se3, "null_lm_free", a.lm_free = nullptr);
  CASE(Se3, "null_nfound", a.nfound = nullptr);
  CASE(Se3, "set_index_out_of_range", f.s2[0] = 2);
  CASE(Se3, "T12_nan", f.T[6] = kNaN);
  CASE(Se3, "null_match", a.match = nullptr);

  CASE(Proj, "valid", );
  CASE(Proj, "unified", a.cam_model = f.cm.data(); a.xi = f.xi.data(); f.cm[1] = COVGPU_CAM_UNIFIED; f.xi[0] = kNaN; a.existing_idx = f.ex.data(); a.taken = f.taken.data());
  CASE(Proj, "zero_sets", a.sets.num_sets = 0; a.num_jobs = 0; a.sets.row_ptr = nullptr);
  CASE(Proj, "zero_jobs", a.num_jobs = 0; a.set = nullptr);
  CASE(Proj, "empty_point_list", f.pp[1] = 0);
  CASE(Proj, "null_batch", f.arg = nullptr);
  CASE(Proj, "null_options", f.opt = nullptr);
  ROW_PTR_CASES(Proj);
  CASE(Proj, "negative_jobs", a.num_jobs = -1);
  CASE(Proj, "null_cam", a.cam = nullptr);
  CASE(Proj, "unknown_distortion", f.dt[1] = 2);
  CASE(Proj, "unknown_model", a.cam_model = f.cm.data(); f.cm[0] = -1);
  CASE(Proj, "unified_without_xi", a.cam_model = f.cm.data(); f.cm[1] = COVGPU_CAM_UNIFIED);
  CASE(Proj, "xi_inf", a.cam_model = f.cm.data(); a.xi = f.xi.data(); f.cm[0] = COVGPU_CAM_UNIFIED; f.xi[0] = kInf);
  CASE(Proj, "null_point_ptr", a.point_ptr = nullptr);
  CASE(Proj, "point_ptr_first", f.pp = {1, 2});
  CASE(Proj, "set_index_out_of_range", f.set[0] = 2);
  CASE(Proj, "set_index_before_point_ptr", f.set[0] = -1; f.pp = {0, -1});
  CASE(Proj, "point_ptr_not_monotone", f.pp = {0, -1});
  CASE(Proj, "T_cw_inf", f.T[0] = kInf);
  CASE(Proj, "null_remap_to", a.remap_to = nullptr);
  CASE(Proj, "existing_idx_out_of_range", a.existing_idx = f.ex.data(); f.ex[1] = 3);

  CASE(Reanchor, "valid", );
  CASE(Reanchor, "nothing", a.K = 0; a.L = 0; a.po = a.pn = a.lm = nullptr; a.ref = nullptr);
  CASE(Reanchor, "negative_K", a.K = -1);
  CASE(Reanchor, "null_lm_pos", a.lm = nullptr);
  CASE(Reanchor, "ref_kf_out_of_range", f.ref[0] = 3);

  CASE(VocabOnly, "valid", );
  CASE(VocabOnly, "null", f.arg = nullptr);
  CASE(VocabOnly, "scoring", a.scoring = 1);
  CASE(VocabOnly, "weighting", a.weighting = 4);
  CASE(VocabOnly, "root_only", a.num_nodes = 1);
  CASE(VocabOnly, "num_words_zero", a.num_words = 0);
  CASE(VocabOnly, "k_zero", a.k = 0);
  CASE(VocabOnly, "null_weight", a.weight = nullptr);
  CASE(VocabOnly, "parent_of_root", f.parent[0] = 0);
  CASE(VocabOnly, "parent_not_before", f.parent[2] = 2);
  CASE(VocabOnly, "child_ptr_first", f.cptr[0] = 1);
  CASE(VocabOnly, "child_ptr_not_monotone", f.cptr = {0, 2, 1, 2});
  CASE(VocabOnly, "child_ptr_last", f.cptr[3] = 3);
  CASE(VocabOnly, "child_out_of_range", f.child[0] = 0);
  CASE(VocabOnly, "child_of_another_parent", f.cptr = {0, 1, 2, 2});
  CASE(VocabOnly, "children_descending", f.child = {2, 1});
  CASE(VocabOnly, "leaf_without_word", f.wid[1] = -1);
  CASE(VocabOnly, "word_id_out_of_range", f.wid[2] = 2);
  CASE(VocabOnly, "word_id_twice", f.wid[2] = 0);
  CASE(VocabOnly, "weight_nan", f.weight[1] = kNaN);
  CASE(VocabOnly, "word_id_missing", a.num_words = 3);

  CASE(Transform, "valid", );
  CASE(Transform, "zero_sets", a.num_sets = 0; a.row_ptr = nullptr; a.bow_ptr = nullptr);
  CASE(Transform, "empty_last_set", f.ptr[2] = 3);
  CASE(Transform, "null_batch", f.arg = nullptr);
  CASE(Transform, "null_vocabulary", f.voc = nullptr);
  CASE(Transform, "negative_capacity", a.capacity = -1);
  CASE(Transform, "null_bow_ptr", a.bow_ptr = nullptr);
  ROW_PTR_CASES(Transform);
  CASE(Transform, "null_desc", a.desc = nullptr);
  CASE(Transform, "null_value", a.value = nullptr);

  CASE(Score, "valid", );
  CASE(Score, "nothing", a.n = 0; a.np = 0; a.ptr = nullptr);
  CASE(Score, "negative_rows", a.n = -1);
  CASE(Score, "null_bow_ptr", a.ptr = nullptr);
  CASE(Score, "bow_ptr_first", f.bptr[0] = 1);
  CASE(Score, "bow_ptr_not_monotone", f.bptr[2] = 1);
  CASE(Score, "null_word", a.word = nullptr);
  CASE(Score, "negative_word", f.word[2] = -1);
  CASE(Score, "words_not_ascending", f.word[1] = 0);
  CASE(Score, "value_nan", f.value[2] = kNaN);
  CASE(Score, "negative_pairs", a.np = -1);
  CASE(Score, "null_score", a.score = nullptr);
  CASE(Score, "pair_out_of_range", f.pb[1] = 3);

  CASE(Detect, "valid", );
  CASE(Detect, "min_score_given", a.min_score_in = f.msin.data());
  CASE(Detect, "invalid_neighbour", a.invalid = f.invalid.data(); f.invalid[1] = 1);
  CASE(Detect, "zero_queries", a.num_queries = 0; a.query_kf = nullptr);
  CASE(Detect, "empty_database", a.num_db = 0; a.db_order = nullptr; f.vis[0] = 0);
  CASE(Detect, "null_options", f.opt = nullptr);
  CASE(Detect, "min_score_factor_nan", f.o.min_score_factor = kNaN);
  CASE(Detect, "negative_scratch", f.o.scratch_kib = -1);
  CASE(Detect, "negative_cap", a.cap = -1);
  CASE(Detect, "null_client", a.client = nullptr);
  CASE(Detect, "negative_id", f.id[2] = -1);
  CASE(Detect, "bow_ptr_not_monotone", f.bptr[2] = 1);
  CASE(Detect, "nb_ptr_first", f.nptr[0] = 1);
  CASE(Detect, "nb_ptr_not_monotone", f.nptr[2] = 0);
  CASE(Detect, "null_nb", a.nb = nullptr);
  CASE(Detect, "neighbour_out_of_range", f.nb[2] = 3);
  CASE(Detect, "null_db_order", a.db_order = nullptr);
  CASE(Detect, "db_order_out_of_range", f.db[1] = 3);
  CASE(Detect, "db_order_repeats", f.db[1] = 1);
  CASE(Detect, "null_db_visible", a.db_visible = nullptr);
  CASE(Detect, "null_candidates", a.candidates = nullptr);
  CASE(Detect, "query_kf_out_of_range", f.qk[0] = -1);
  CASE(Detect, "db_visible_too_large", f.vis[0] = 3);
  CASE(Detect, "min_score_in_nan", a.min_score_in = f.msin.data(); f.msin[0] = kNaN);
  CASE(Detect, "too_many_query_neighbours", f.nb.assign(65536, 0); f.nptr = {0, 0, 0, 65536}; f.qk.assign(32769, 2); f.vis.assign(32769, 0); f.nc.assign(32769, 0);
       f.cand.assign(2 * 32769, 0); a.nb = f.nb.data(); a.num_queries = 32769; a.query_kf = f.qk.data(); a.db_visible = f.vis.data(); a.num_candidates = f.nc.data();
       a.candidates = f.cand.data());

  CASE(Prune, "valid", );
  CASE(Prune, "nothing", a.num_kf = 0; a.num_lm = 0; f.ptr = {0}; a.lm_obs_ptr = f.ptr.data(); a.kf_pred = nullptr);
  CASE(Prune, "empty_last_landmark", f.ptr[2] = 2);
  CASE(Prune, "null_problem", f.arg = nullptr);
  CASE(Prune, "th_red_nan", f.o.th_red = kNaN);
  CASE(Prune, "negative_capacity", a.capacity = -1);
  CASE(Prune, "null_lm_obs_ptr", a.lm_obs_ptr = nullptr);
  CASE(Prune, "lm_obs_ptr_first", f.ptr[0] = 1);
  CASE(Prune, "lm_obs_ptr_not_monotone", f.ptr[1] = 4);
  CASE(Prune, "null_obs_kf", a.obs_kf = nullptr);
  CASE(Prune, "obs_kf_out_of_range", f.okf[2] = 3);
  CASE(Prune, "null_kf_time", a.kf_time = nullptr);
  CASE(Prune, "null_round_action", a.round_action = nullptr);
  CASE(Prune, "kf_time_inf", f.time[1] = kInf);
  CASE(Prune, "kf_succ_out_of_range", f.succ[2] = 3);
  CASE(Prune, "not_mutual", f.succ[0] = 2);

  CASE(Refresh, "valid", );
  CASE(Refresh, "nothing", a.num_kf = 0; a.num_lm = 0; f.ptr = {0}; a.lm_obs_ptr = f.ptr.data(); a.kf_center = nullptr; a.lm_pos = nullptr);
  CASE(Refresh, "empty_last_landmark", f.ptr[2] = 2);
  CASE(Refresh, "null_options", f.opt = nullptr);
  CASE(Refresh, "scale_factor_zero", f.o.scale_factor = 0.0);
  CASE(Refresh, "num_octaves_65", f.o.num_octaves = 65);
  CASE(Refresh, "negative_kf", a.num_kf = -1);
  CASE(Refresh, "null_lm_obs_ptr", a.lm_obs_ptr = nullptr);
  CASE(Refresh, "lm_obs_ptr_first", f.ptr[0] = 1);
  CASE(Refresh, "lm_obs_ptr_not_monotone", f.ptr[1] = 4);
  CASE(Refresh, "null_obs_octave", a.obs_octave = nullptr);
  CASE(Refresh, "null_lm_pos", a.lm_pos = nullptr);
  CASE(Refresh, "null_kf_center", a.kf_center = nullptr);
  CASE(Refresh, "obs_kf_out_of_range", f.okf[0] = -1);
  CASE(Refresh, "lm_ref_obs_outside", f.ref[1] = 1);
  CASE(Refresh, "reference_octave_64", f.ooc[1] = 64);
  CASE(Refresh, "lm_pos_nan", f.pos[5] = kNaN);
  CASE(Refresh, "kf_center_inf", f.cen[8] = kInf);

  CASE(VocTrain, "valid", );
  CASE(VocTrain, "empty_last_set", f.ptr[2] = 3);
  CASE(VocTrain, "null_problem", f.arg = nullptr);
  CASE(VocTrain, "k_one", f.o.k = 1);
  CASE(VocTrain, "k_33", f.o.k = 33);
  CASE(VocTrain, "L_zero", f.o.L = 0);
  CASE(VocTrain, "too_many_words", f.o.k = 32; f.o.L = 5);
  CASE(VocTrain, "weighting", f.o.weighting = -1);
  CASE(VocTrain, "scoring", f.o.scoring = 1);
  CASE(VocTrain, "max_iterations_zero", f.o.max_iterations = 0);
  CASE(VocTrain, "scratch_too_small", f.o.scratch_kib = 12);
  CASE(VocTrain, "negative_node_capacity", a.node_capacity = -1);
  CASE(VocTrain, "zero_sets", a.num_sets = 0);
  CASE(VocTrain, "null_row_ptr", a.row_ptr = nullptr);
  CASE(VocTrain, "row_ptr_first", f.ptr[0] = 1);
  CASE(VocTrain, "row_ptr_not_monotone", f.ptr[1] = 6);
  CASE(VocTrain, "long_set_allowed", f.ptr = {0, 4097, 4099}; f.desc.assign(32 * 4099, 1); a.desc = f.desc.data());
  CASE(VocTrain, "empty_sets_only", f.ptr = {0, 0, 0});
  CASE(VocTrain, "too_many_rows", f.ptr[2] = INT32_MAX - 2047);
  CASE(VocTrain, "null_desc", a.desc = nullptr);
  CASE(VocTrain, "null_num_words", a.num_words = nullptr);
  CASE(VocTrain, "null_weight", a.weight = nullptr);

  CASE(UploadCam, "valid", );
  CASE(UploadCam, "all_pinhole", a.model = nullptr; a.xi = nullptr);
  CASE(UploadCam, "unknown_model", f.model[0] = 2);
  CASE(UploadCam, "unified_without_cam_xi", a.xi = nullptr);
  CASE(UploadCam, "xi_negative", f.xi[1] = -1.0);
  return 0;
}
