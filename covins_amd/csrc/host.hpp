// host.hpp — what the host files of libcovgpu (the solver's solver.hip, upload.hip, plan_api.hip, shard.hip, multi.hip and probe_api.hip; batch.hip,
// bowdb.hip, voctrain.hip) share: the context, the error plumbing of the extern "C" entry points (guarded, batch_entry, check_export), the
// per-call device scratch and event pair, and the declarations of the solver's functions that one of its files calls in another. The
// argument checks themselves are plain C++ in batch_check.hpp, which this header includes. Host-only: no kernel file includes it.
#pragma once
#include <atomic>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "batch_check.hpp"
#include "fivept_check.hpp"
#include "common.hpp"
#include "nd_plan.hpp"

// message of the calling thread's last failed call (covgpu_last_error); the one definition is in solver.hip
__attribute__((visibility("hidden"))) extern thread_local std::string g_err;

#define HIPCHK(expr)                                                                            \
  do {                                                                                          \
    hipError_t e_ = (expr);                                                                     \
    if (e_ != hipSuccess) {                                                                     \
      g_err = std::string(#expr) + ": " + hipGetErrorString(e_);                                \
      return e_ == hipErrorOutOfMemory ? COVGPU_ERR_OUT_OF_MEMORY : COVGPU_ERR_NO_DEVICE;       \
    }                                                                                           \
  } while (0)

struct covgpu_profile_t {
  double t_build_ms = 0, t_factor_ms = 0, t_syrk_ms = 0, syrk_flops = 0;
  long n_build = 0, n_factor = 0, n_syrk = 0;
};

// elimination tree of the last single-GPU GBA upload and what it was built for (upload_impl)
struct PlanCache {
  bool valid = false; int K = 0; bool vi = false; int leaf = 0;
  int top_env = -1; double frac_env = 0.0;   // COVGPU_ND_TOP / COVGPU_ND_GROUP_FRAC as nd_plan_build read them (-1 / 0: not set)
  bool merge_env = true;                     // COVGPU_ND_MERGE likewise (nd_merge_enabled), and false for a pose graph
  std::vector<int> chain_ptr, pos_kf;
  std::vector<uint64_t> keys;   // sorted (position i << 32 | position j) of every covisible / loop-edge pair
  covgpu::NdHostPlan hp;
};

constexpr int COVGPU_ERR_GATE_TIMEOUT = -1000;   // internal (solve_any): never returned through the C ABI
struct covgpu_group;
struct covgpu_nd_plan { covgpu::NdHostPlan hp; std::vector<int> pos_kf; };

// sum (op 0) / max (op 1) of n device doubles over all ranks, in place, ENQUEUED on the stream. The two native forms (RCCL, the in-process group of
// virtual ranks) are private to shard.hip.
struct Reducer {
  int rank = 0, world = 1;
  size_t calls = 0, bytes = 0;
  virtual ~Reducer() {}
  virtual int allreduce(double* dev, size_t n, int op, hipStream_t st) = 0;
  virtual void abort() {}                       // make every peer's pending and future collectives return
  virtual int async_error() { return 0; }       // asynchronous error of the communicator, polled by the host while it waits for an iteration (RCCL only)
  virtual std::string last_error() { return "all-reduce failed"; }
};
struct covgpu_context {
  int device = 0;
  hipStream_t st = nullptr;
  covgpu::DevProblem P;
  bool have = false, pgo = false;
  bool second_round = false; // a covgpu_gba_two_round that succeeded left the SECOND round's problem resident (compacted landmark / observation indexing) while
                             // `have` is false for every call that scatters into the caller's first-round arrays; a call whose outputs are in the resident
                             // indexing (covgpu_landmark_covariance_resident) may still use it. Cleared by the next upload.
  bool state_set = false;    // the working estimate (P.pose, P.sb, P.lm) holds the uploaded one or a solve's result (reset_state; cleared by an upload)
  std::vector<void*> allocs;
  size_t alloc_bytes = 0;  // device bytes behind `allocs` (the footprint covgpu_get_layout reports)
  double* h_scal = nullptr;  // pinned mirror of P.scal + flag
  double* h_tr = nullptr;    // pinned mirror of P.tr (device-side trust region)
  double* h_box = nullptr;   // pinned + mapped [TR_COUNT + 1]: the last kernel of an iteration posts P.tr and a sequence number here (k_tr_accept), the host polls it
  double* d_box = nullptr;   // its device address (nullptr: not available — D2H copy + stream synchronisation)
  double box_seq = 0.0;
  double* trace = nullptr; int trace_cap = 0, trace_n = 0;   // covgpu_solve_resident_traced: h_tr after every end_iteration (nullptr in the product path)
  int profiling = 0;
  covgpu_profile_t prof;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  covgpu::CholAux chol;
  covgpu::PgoPlan pgo_plan;  // block-arrow pose-graph solve (k_pgo.hip)
  PlanCache plan_cache;  // elimination tree of the previous single-GPU GBA upload (reused when the new problem's couplings are a subset)
  covgpu::NdDev nd;          // multifrontal GBA solve (k_front.hip)
  // agent-sharded solve: the global plan (variables as 2 * IR keyframe + kind, node -> rank), this rank's
  // identity and its collective
  bool sharded = false;
  int rank = 0, world = 1;
  std::shared_ptr<covgpu::NdHostPlan> shard_plan;
  Reducer* reducer = nullptr;
  double* d_red = nullptr;     // [SC_COUNT + 2 world] scratch of the scalar all-reduce
  double cur_damp = 0.0;       // damping of the system being built (the top unknowns get theirs after the all-reduce)
  // a collective (or a scratch allocation of the linear solve) that failed while the iteration was being enqueued (broken / timed-out
  // group barrier, scratch hipMalloc, non-zero ncclAllReduce): latched here, checked after the iteration's host synchronisation —
  // the solve then returns an error instead of an estimate computed from un-reduced top fronts
  bool coll_failed = false;
  bool edge_beside_imu = false;  // a loop edge joins two neighbouring chain positions: its pair block may be an IMU factor's cross block too (enqueue_build)
  std::string coll_err;
  covgpu_group* group = nullptr;   // the in-process group this context's reducer belongs to (aborted when this rank gives up)
  int* d_pairkey = nullptr;    // [K] key of every keyframe in the covisible-pair numbering (chain position, -1: constant pose), kept for the second round of a call
  std::vector<int> h_perm;     // [K] keyframe -> chain position of the resident problem
  std::atomic<int>* peer_fail = nullptr;   // covgpu_gba_solve_multi: raised by any rank of the call that gave up; polled while waiting
  std::vector<covgpu_bowdb*> bowdbs;       // resident keyframe databases of this context (bowdb.hip): destroyed with it
};

#define RC(expr) do { int rc_ = (expr); if (rc_) return rc_; } while (0)
// no C++ exception may cross the extern "C" boundary (std::bad_alloc from the host staging vectors, std::system_error from
// std::thread): map them to status codes
template <typename F>
static int guarded(F&& body) {
  try { return body(); }
  catch (const std::bad_alloc&) { g_err = "host allocation failed"; return COVGPU_ERR_OUT_OF_MEMORY; }
  catch (const std::exception& e) { g_err = std::string("host exception: ") + e.what(); return COVGPU_ERR_INVALID_ARG; }
}

// The prologue of every stateless device entry point (batch.hip, voctrain.hip): a NULL context is an argument error, and no C++
// exception leaves the call. `bad` is the body's argument-error return: "<function>: <message>".
template <typename F>
static int batch_entry(const char* fn, covgpu_context* c, F&& body) {
  auto bad = [fn](const std::string& m) -> int { g_err = std::string(fn) + ": " + m; return COVGPU_ERR_INVALID_ARG; };
  if (!c) return bad("NULL context");
  return guarded([&] { return body(bad); });
}

// A covgpu_*_check export: the entry point's own check without a context or a device. `check` returns the first violation or nullptr.
template <typename F>
static int check_export(const char* fn, F&& check) {
  return guarded([&]() -> int {
    if (const char* m = check()) { g_err = std::string(fn) + ": " + m; return COVGPU_ERR_INVALID_ARG; }
    return COVGPU_OK;
  });
}

// Two events around the kernels of a call whose caller asks for their device time; destroyed however the call returns.
struct EventPair {
  hipEvent_t a = nullptr, b = nullptr;
  EventPair() = default;
  EventPair(const EventPair&) = delete;
  EventPair& operator=(const EventPair&) = delete;
  ~EventPair() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
};

// Every device buffer of one call: freed when the call returns, however it returns. Counts are in elements of T; an empty buffer is
// still a valid pointer (16 B, which no kernel reads). Declare the host vectors that receive a fetch() BEFORE the scratch object:
// its hipFree waits for the device, so on an error return the copies into them have drained before they are destroyed.
struct DeviceScratch {
  explicit DeviceScratch(hipStream_t st) : st(st) {}
  DeviceScratch(const DeviceScratch&) = delete;
  DeviceScratch& operator=(const DeviceScratch&) = delete;
  ~DeviceScratch() { for (void* p : held) (void)hipFree(p); }
  void adopt(void* d) { if (d) held.push_back(d); }   // a buffer somebody else allocated (k_pairs.hip's pair lists)
  template <class T> hipError_t alloc(T** d, size_t count) {
    *d = nullptr;
    held.reserve(held.size() + 1);   // (a throwing push_back behind the hipMalloc would leak the buffer)
    void* p = nullptr;
    const hipError_t e = hipMalloc(&p, count ? count * sizeof(T) : 16);
    if (e == hipSuccess) { held.push_back(p); *d = (T*)p; }
    return e;
  }
  // alloc + asynchronous upload (T may be const-qualified: the device structs of common.hpp hold pointers to const)
  template <class T> hipError_t upload(T** d, const std::remove_const_t<T>* host, size_t count) {
    const hipError_t e = alloc(d, count);
    return e != hipSuccess || !count ? e : hipMemcpyAsync((void*)*d, host, count * sizeof(T), hipMemcpyHostToDevice, st);
  }
  template <class T> hipError_t zeroed(T** d, size_t count) {
    const hipError_t e = alloc(d, count);
    return e != hipSuccess || !count ? e : hipMemsetAsync((void*)*d, 0, count * sizeof(T), st);
  }
  // asynchronous download; nothing to do for an empty buffer or an output the caller did not ask for
  template <class T> hipError_t fetch(T* host, const T* d, size_t count) {
    return count && host ? hipMemcpyAsync(host, d, count * sizeof(T), hipMemcpyDeviceToHost, st) : hipSuccess;
  }
  hipStream_t st;
  std::vector<void*> held;
};

// device buffers of the RESIDENT problem: owned by the context (covgpu_context::allocs), freed by the next upload or with the context
template <typename T>
static int dev_alloc(covgpu_context* c, T** ptr, size_t count) {
  *ptr = nullptr;
  if (count == 0) count = 1;
  void* p = nullptr;
  hipError_t e = hipMalloc(&p, count * sizeof(T));
  if (e != hipSuccess) { g_err = std::string("hipMalloc: ") + hipGetErrorString(e); return COVGPU_ERR_OUT_OF_MEMORY; }
  c->allocs.push_back(p);
  c->alloc_bytes += count * sizeof(T);
  *ptr = (T*)p;
  return COVGPU_OK;
}
template <typename T>
static int dev_upload(covgpu_context* c, T** ptr, const T* host, size_t count) {
  int rc = dev_alloc(c, ptr, count);
  if (rc) return rc;
  if (count && host) HIPCHK(hipMemcpyAsync(*ptr, host, count * sizeof(T), hipMemcpyHostToDevice, c->st));
  else if (count) HIPCHK(hipMemsetAsync(*ptr, 0, count * sizeof(T), c->st));
  return COVGPU_OK;
}

// ---- the solver's functions that cross one of its files (none of them is exported)
#define COVGPU_HIDDEN __attribute__((visibility("hidden")))
// shard.hip
COVGPU_HIDDEN void clear_shard(covgpu_context* c);
COVGPU_HIDDEN void reduce_scalars(covgpu_context* c);
// plan_api.hip
COVGPU_HIDDEN int build_chains(const covgpu_problem* p, bool vi, std::vector<int>& perm, std::vector<int>& pos_kf, std::vector<int>& chain_ptr);
COVGPU_HIDDEN void build_chains_pgo(const covgpu_problem* p, std::vector<int>& perm, std::vector<int>& pos_kf, std::vector<int>& chain_ptr);
COVGPU_HIDDEN int nd_leaf_dims(int requested);
COVGPU_HIDDEN bool plan_timing_on();   // dev aid COVGPU_PLAN_TIMING=1: where the host side of an upload and of a plan goes (stderr)
// upload.hip
COVGPU_HIDDEN int validate(const covgpu_problem* p, bool pgo, bool vi);
COVGPU_HIDDEN void free_problem(covgpu_context* c);
COVGPU_HIDDEN int upload_impl(covgpu_context* c, const covgpu_options* opt, const covgpu_problem* p, bool pgo, bool allow_arrow = true);
COVGPU_HIDDEN int upload_pair_lists(covgpu_context* c, bool second_round, std::vector<int>* host_i, std::vector<int>* host_j);
COVGPU_HIDDEN int reset_state(covgpu_context* c);
COVGPU_HIDDEN int download_states(covgpu_context* c, covgpu_problem* p);
COVGPU_HIDDEN int download_impl(covgpu_context* c, covgpu_problem* p);
// solver.hip
COVGPU_HIDDEN int read_scalars(covgpu_context* c);
COVGPU_HIDDEN int chol_failed(covgpu_context* c);
COVGPU_HIDDEN void enqueue_build(covgpu_context* c, double mu);
COVGPU_HIDDEN void enqueue_solve(covgpu_context* c, double* dst_all);
COVGPU_HIDDEN int solve_any(covgpu_context* c, const covgpu_options* opt, covgpu_result* out);
COVGPU_HIDDEN int gba_two_round_impl(covgpu_context* c, const covgpu_options* opt, covgpu_problem* p, const covgpu_two_round* tr, uint8_t* obs_erase,
                                     int32_t* lm_left, int64_t* counts, covgpu_result* round1, covgpu_result* round2);
