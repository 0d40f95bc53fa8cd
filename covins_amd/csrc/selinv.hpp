// selinv.hpp — what the top-down sweep of the selected inverse (k_selinv.hip) and its host side (selinv.hip) share: the per-call tables; and
// what the host side offers the other caller of the sweep (lmcov.hip): the plan, the rule that says where a block of Sigma lies, and the
// step that leaves Sigma in its scratch.
#pragma once
#include <functional>
#include <vector>

#include "common.hpp"
#include "selinv_check.hpp"

struct covgpu_context;
struct DeviceScratch;   // host.hpp

namespace covgpu {

// One front. Sigma's square and the temporaries W = L_OO^-1 / T = L_BO W live in two scratch buffers laid out like nd_M: the same element
// offset and leading dimension, own rows first, border rows from nI on (W over L_OO, T over L_BO).
struct SelFront {
  long long moff, linv, pmoff;   // element offset of the front | of its block inverses in nd_Linv | of its ancestor's front (-1: a root)
  int ld, nI, own, st;           // leading dimension | padded interior order of its level (where the border rows start) | own | border unknowns
  int nbo, pld;                  // 16-row blocks of its own unknowns | the ancestor's leading dimension
  int gmap, pad;                 // first entry of its border rows' map (border scalar -> row of the ancestor's square)
};
// One workgroup of a step: x = front, y = kind (0 gather | 1 W | 2 T | 3 Sigma_BO | 4 Sigma_OO | 5 the whole front in the vector form),
// z = 16-row block (kind 1: group of four 16-column chunks), w = panel of 128 own columns
struct SelArgs {
  const double *M, *Linv;
  double *S, *X;
  const SelFront* fr; const int* gmap; const int4* items;
};
void launch_selinv_gather(const SelArgs& a, int item0, int count, hipStream_t st);
void launch_selinv_step(const SelArgs& a, int item0, int count, int kind, hipStream_t st);
void launch_selinv_read(const double* S, const long long* src, double* out, long long n, hipStream_t st);

// ---- host side (selinv.hip)
struct SelLaunch { int first, count, kind; };   // kind 0: gather | 1 .. 4: matrix-core form | 5: vector form
// The sweep's plan. Everything in it is in SOLUTION indices (D * keyframe of the problem + component, the numbering of NdDev::h_gidx), fronts
// in the front order of NdDev (level order, leaves first).
struct SelPlan {
  int d = 0;
  std::vector<SelFront> fronts;
  std::vector<int> gmap;
  std::vector<int4> items;
  std::vector<SelLaunch> launches;   // stream order: root level first
  std::vector<int> gnode, goff, lev_of;   // [n] front that owns a solution index (-1: none), its column there | [fronts] level
  std::vector<long long> src;        // read-out of covgpu_selected_inverse: [K d d | num_pairs d d] element of Sigma behind every output entry (-1: zero)
  std::vector<uint8_t> pair_ok;
  long long served = 0;
};
// A block of Sigma somebody wants: rows [grow, grow + nrow) x columns [gcol, gcol + ncol) in solution indices, each range one variable's rows
// (or its first rows). sel_want says which front's square holds it: the square of whichever of the two owners is lower in the tree, with the
// other variable in its border. sel_locate finds it there: off = element of Sigma of its first entry, ld = the square's leading dimension;
// off < 0: the other variable is not in that square.
struct SelReq { int front, grow, nrow, gcol, ncol, sym; size_t out; long long off; int ld; };
bool sel_want(const SelPlan& pl, int grow, int nrow, int gcol, int ncol, int sym, size_t out, std::vector<SelReq>& reqs);
const char* sel_locate(const covgpu_context* c, const SelPlan& pl, std::vector<SelReq>& reqs);   // sorts reqs by front (stable)
// the read-out table of the keyframes' diagonal blocks and of rq's pairs (pl.src, pl.pair_ok, pl.served); nullptr or the plan error
const char* sel_plan_readout(const covgpu_context* c, const covgpu_selinv_t* rq, const uint8_t* fixed, SelPlan& pl);

// Step one of a call: plans the sweep, allocates its scratch in U, lets the caller plan and allocate what it adds (`prepare`, which sees
// the finished tree part of the plan; a non-zero return ends the call with nothing enqueued), then linearises at the resident estimate,
// builds and factors at mu and runs the sweep. Sigma is left in a.S, laid out like the fronts, ordered on the context's stream.
struct SelSweep {
  SelPlan pl;
  SelArgs a{};
  long long n_mfma = 0, n_vec = 0, n_gather = 0;
  size_t bytes = 0;                  // scratch of the sweep itself
};
int sel_factor_and_sweep(const char* fn, covgpu_context* c, double mu, ::DeviceScratch& U, SelSweep& sw, const std::function<int(SelPlan&)>& prepare);
// Step two of covgpu_selected_inverse, and the kf_cov of covgpu_landmark_covariance: the entries pl.src names, out of Sigma, to `out` (device,
// pl.src.size() doubles) through `src` (device, as many): both allocated by the caller's `prepare`. Enqueued; the caller fetches.
int sel_read_out(covgpu_context* c, const SelSweep& sw, long long* src, double* out);
int sel_fetch_fixed(covgpu_context* c, std::vector<uint8_t>& fixed);   // the constant-pose flags of the resident problem
// the refusals that depend on the context: the sweep reads the fronts of ONE device's elimination tree
int sel_context_check(const char* fn, const covgpu_context* c);
}  // namespace covgpu
