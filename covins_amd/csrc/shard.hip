// shard.hip — the collectives of the agent-sharded solve and the entry points that give a context its shard:
// the two reducers behind host.hpp's Reducer, the in-process group, the RCCL shim, covgpu_set_shard_*, and the scalar
// all-reduce of the trust-region loop (reduce_scalars).
//
// A Reducer sums (op 0) / maximises (op 1) n device doubles over all ranks, in place, ENQUEUED on the stream (no host synchronisation in
// the RCCL form). Two native forms: RCCL (one process per GPU, or several devices in one process) and an in-process group
// of host threads whose contexts share one device (virtual ranks: how the sharded path runs on a one-GPU test box).
#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "host.hpp"

using namespace covgpu;

struct GroupPtrs { double* p[16]; };
__global__ __launch_bounds__(256) void k_group_reduce(GroupPtrs g, int world, size_t n, int op, double* __restrict__ out) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    double v = g.p[0][i];
    for (int r = 1; r < world; ++r) v = op == 0 ? v + g.p[r][i] : fmax(v, g.p[r][i]);  // rank order: identical on every rank
    out[i] = v;
  }
}
struct covgpu_group {
  int world = 1;
  std::mutex m; std::condition_variable cv; int count = 0; long gen = 0; bool broken = false;
  GroupPtrs ptrs;
  bool wait() {  // barrier of the group's host threads; false if a member gave up
    std::unique_lock<std::mutex> lk(m);
    const long g0 = gen;
    if (++count == world) { count = 0; ++gen; cv.notify_all(); return !broken; }
    cv.wait_for(lk, std::chrono::seconds(600), [&] { return gen != g0 || broken; });
    if (gen == g0) { broken = true; cv.notify_all(); return false; }
    return !broken;
  }
};
struct GroupReducer : Reducer {
  covgpu_group* g = nullptr;
  double* scratch = nullptr; size_t scratch_n = 0;
  ~GroupReducer() override { if (scratch) (void)hipFree(scratch); }
  void abort() override { std::lock_guard<std::mutex> lk(g->m); g->broken = true; g->cv.notify_all(); }
  std::string last_error() override { return "in-process group all-reduce failed (a member gave up, timed out, or the scratch allocation failed)"; }
  int allreduce(double* dev, size_t n, int op, hipStream_t st) override {
    if (n == 0) return 0;
    if (scratch_n < n) { if (scratch) (void)hipFree(scratch); if (hipMalloc((void**)&scratch, n * sizeof(double)) != hipSuccess) return 1; scratch_n = n; }
    (void)hipStreamSynchronize(st);  // this rank's contribution is final
    { std::lock_guard<std::mutex> lk(g->m); g->ptrs.p[rank] = dev; }
    if (!g->wait()) return 1;
    hipLaunchKernelGGL(k_group_reduce, dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, st, g->ptrs, world, n, op, scratch);
    (void)hipStreamSynchronize(st);
    if (!g->wait()) return 1;        // everybody has read everybody's buffer
    (void)hipMemcpyAsync(dev, scratch, n * sizeof(double), hipMemcpyDeviceToDevice, st);
    ++calls; bytes += n * sizeof(double);
    return 0;
  }
};

// RCCL, loaded at run time: the single-GPU path of libcovgpu has no dependency on it
struct RcclApi {
  void* h = nullptr;
  int (*GetUniqueId)(void*) = nullptr;
  int (*CommInitRank)(void**, int, struct RcclId, int) = nullptr;
  int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  int (*CommAbort)(void*) = nullptr;
  int (*CommGetAsyncError)(void*, int*) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
};
struct RcclId { char internal[128]; };   // ncclUniqueId (rccl.h:40-43)
static RcclApi* rccl_api() {
  static RcclApi api;
  static std::once_flag once;
  std::call_once(once, [] {
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) { api.h = dlopen(name, RTLD_NOW | RTLD_LOCAL); if (api.h) break; }
    if (!api.h) return;
    api.GetUniqueId = (int (*)(void*))dlsym(api.h, "ncclGetUniqueId");
    api.CommInitRank = (int (*)(void**, int, RcclId, int))dlsym(api.h, "ncclCommInitRank");
    api.AllReduce = (int (*)(const void*, void*, size_t, int, int, void*, hipStream_t))dlsym(api.h, "ncclAllReduce");
    api.CommDestroy = (int (*)(void*))dlsym(api.h, "ncclCommDestroy");
    api.GetErrorString = (const char* (*)(int))dlsym(api.h, "ncclGetErrorString");
    api.CommAbort = (int (*)(void*))dlsym(api.h, "ncclCommAbort");
    api.CommGetAsyncError = (int (*)(void*, int*))dlsym(api.h, "ncclCommGetAsyncError");
    if (!api.GetUniqueId || !api.CommInitRank || !api.AllReduce || !api.CommDestroy) { dlclose(api.h); api.h = nullptr; }
  });
  return api.h ? &api : nullptr;
}
struct RcclReducer : Reducer {
  void* comm = nullptr;
  bool aborted = false;
  int last_rc = 0;
  ~RcclReducer() override { if (comm && rccl_api()) rccl_api()->CommDestroy(comm); }
  int allreduce(double* dev, size_t n, int op, hipStream_t st) override {
    if (n == 0) return 0;
    if (aborted) return 1;
    ++calls; bytes += n * sizeof(double);
    last_rc = rccl_api()->AllReduce(dev, dev, n, /*ncclFloat64*/ 8, op == 0 ? /*ncclSum*/ 0 : /*ncclMax*/ 2, comm, st);
    return last_rc;
  }
  // asynchronous error of the communicator (a peer died, a link failed): polled by the host while it waits for the iteration
  int async_error() override {
    int e = 0;
    if (comm && rccl_api()->CommGetAsyncError && rccl_api()->CommGetAsyncError(comm, &e) == 0) return e;
    return 0;
  }
  void abort() override {   // tears the communicator down at once: collective kernels in flight on any stream of this rank return
    if (comm && rccl_api()->CommAbort) { rccl_api()->CommAbort(comm); comm = nullptr; }
    aborted = true;
  }
  std::string last_error() override {
    return std::string("RCCL all-reduce failed: ") + (rccl_api()->GetErrorString && last_rc ? rccl_api()->GetErrorString(last_rc) : "communicator aborted or asynchronous error");
  }
};

static void coll_latch(covgpu_context* c) {
  if (!c->coll_failed) { c->coll_failed = true; c->coll_err = c->reducer ? c->reducer->last_error() : "all-reduce failed"; }
}
static void ctx_reduce(void* vc, double* dev, size_t n, int op, hipStream_t st) {
  covgpu_context* c = (covgpu_context*)vc;
  if (c->reducer && n && c->reducer->allreduce(dev, n, op, st) != 0) coll_latch(c);
}
void clear_shard(covgpu_context* c) {
  delete c->reducer; c->reducer = nullptr;
  c->coll_failed = false; c->coll_err.clear(); c->group = nullptr;
  c->sharded = false; c->rank = 0; c->world = 1; c->shard_plan.reset();
  c->chol.reduce = nullptr; c->chol.reduce_ctx = nullptr;
}
extern "C" int covgpu_set_shard_none(covgpu_context* c) { clear_shard(c); return COVGPU_OK; }

extern "C" int covgpu_group_create(int32_t world, covgpu_group** out) {
  if (world < 1 || world > 16) { g_err = "covgpu_group_create: world must be 1..16"; return COVGPU_ERR_INVALID_ARG; }
  covgpu_group* g = new covgpu_group(); g->world = world;
  for (auto& q : g->ptrs.p) q = nullptr;
  *out = g;
  return COVGPU_OK;
}
extern "C" void covgpu_group_destroy(covgpu_group* g) { delete g; }
extern "C" void covgpu_group_abort(covgpu_group* g) { std::lock_guard<std::mutex> lk(g->m); g->broken = true; g->cv.notify_all(); }

static int set_shard_common(covgpu_context* c, const covgpu_nd_plan* plan, int rank, int world, Reducer* red) {
  if (!plan || plan->hp.node_rank.empty()) { delete red; g_err = "covgpu_set_shard: the plan carries no rank assignment (use covgpu_shard_plan)"; return COVGPU_ERR_INVALID_ARG; }
  if (rank < 0 || rank >= world) { delete red; g_err = "covgpu_set_shard: rank out of range"; return COVGPU_ERR_INVALID_ARG; }
  for (int r : plan->hp.node_rank) if (r >= world) { delete red; g_err = "covgpu_set_shard: the plan was made for more ranks"; return COVGPU_ERR_INVALID_ARG; }
  clear_shard(c);
  // keep the plan in IR terms (variable = 2 * keyframe + kind): a rank's sub-problem orders its keyframes differently
  auto hp = std::make_shared<NdHostPlan>(plan->hp);
  std::vector<int> to_ir(2 * (size_t)hp->K);
  for (int q = 0; q < hp->K; ++q) { to_ir[2 * q] = 2 * plan->pos_kf[q]; to_ir[2 * q + 1] = 2 * plan->pos_kf[q] + 1; }
  nd_plan_remap(*hp, to_ir);
  c->shard_plan = hp;
  red->rank = rank; red->world = world;
  c->reducer = red; c->sharded = true; c->rank = rank; c->world = world;
  c->chol.reduce = ctx_reduce; c->chol.reduce_ctx = c;
  return COVGPU_OK;
}
extern "C" int covgpu_set_shard_group(covgpu_context* c, const covgpu_nd_plan* plan, int32_t rank, covgpu_group* g) {
  if (!g) { g_err = "covgpu_set_shard_group: NULL group"; return COVGPU_ERR_INVALID_ARG; }
  GroupReducer* r = new GroupReducer(); r->g = g;
  const int rc = set_shard_common(c, plan, rank, g->world, r);
  if (rc == COVGPU_OK) c->group = g;
  return rc;
}
extern "C" int covgpu_rccl_unique_id(uint8_t* out128) {
  RcclApi* api = rccl_api();
  if (!api) { g_err = "librccl could not be loaded"; return COVGPU_ERR_NO_DEVICE; }
  RcclId id;
  const int rc = api->GetUniqueId(&id);
  if (rc != 0) { g_err = std::string("ncclGetUniqueId: ") + (api->GetErrorString ? api->GetErrorString(rc) : "error"); return COVGPU_ERR_NO_DEVICE; }
  std::memcpy(out128, id.internal, 128);
  return COVGPU_OK;
}
extern "C" int covgpu_set_shard_rccl(covgpu_context* c, const covgpu_nd_plan* plan, int32_t rank, int32_t world, const uint8_t* id128) {
  RcclApi* api = rccl_api();
  if (!api) { g_err = "librccl could not be loaded"; return COVGPU_ERR_NO_DEVICE; }
  HIPCHK(hipSetDevice(c->device));
  RcclId id; std::memcpy(id.internal, id128, 128);
  RcclReducer* r = new RcclReducer();
  const int rc = api->CommInitRank(&r->comm, world, id, rank);
  if (rc != 0) { delete r; g_err = std::string("ncclCommInitRank: ") + (api->GetErrorString ? api->GetErrorString(rc) : "error"); return COVGPU_ERR_NO_DEVICE; }
  return set_shard_common(c, plan, rank, world, r);
}
// host convenience through the context's collective (barriers / timing aggregates of a multi-process run): in place
extern "C" int covgpu_allreduce_host(covgpu_context* c, double* host, int64_t n, int32_t op) {
  if (!c->reducer || n <= 0) return COVGPU_OK;
  HIPCHK(hipSetDevice(c->device));
  DeviceScratch U(c->st);
  double* d = nullptr;
  HIPCHK(U.upload(&d, host, (size_t)n));
  const int rc = c->reducer->allreduce(d, (size_t)n, op, c->st);
  HIPCHK(U.fetch(host, d, (size_t)n));
  HIPCHK(hipStreamSynchronize(c->st));
  if (rc != 0) { g_err = "all-reduce failed"; return COVGPU_ERR_NO_DEVICE; }
  return COVGPU_OK;
}
// out[4] = { collectives issued, bytes all-reduced (per rank), rank, world }
extern "C" void covgpu_shard_stats(covgpu_context* c, int64_t* out) {
  out[0] = c->reducer ? (int64_t)c->reducer->calls : 0; out[1] = c->reducer ? (int64_t)c->reducer->bytes : 0; out[2] = c->rank; out[3] = c->world;
}

// sharded solve: the scalars the device-side trust region is about to read are sums over residuals / unknowns each counted
// by exactly one rank (DevProblem::vw), the gradient max-norm and the factorisation flag are maxima: ONE small all-reduce
// (sum) of [16 scalars | one slot per rank for the max-norm | one slot per rank for the flag] on a scratch copy, enqueued
// on the stream; the reduced values go to P.scal_r / P.flag_r, the rank's own partial sums in P.scal stay untouched.
__global__ void k_shard_scal_pack(DevProblem P, double* buf, int rank, int world) {
  const int t = threadIdx.x;
  if (t < SC_COUNT) buf[t] = (t == SC_GMAX) ? 0.0 : P.scal[t];
  if (t < world) { buf[SC_COUNT + t] = t == rank ? P.scal[SC_GMAX] : 0.0; buf[SC_COUNT + world + t] = t == rank ? (double)P.flag[0] : 0.0; }
}
__global__ void k_shard_scal_unpack(DevProblem P, const double* buf, int world) {
  const int t = threadIdx.x;
  if (t < SC_COUNT && t != SC_GMAX) P.scal_r[t] = buf[t];
  if (t == 0) {
    double gm = 0.0, fl = 0.0;
    for (int r = 0; r < world; ++r) { gm = fmax(gm, buf[SC_COUNT + r]); fl = fmax(fl, buf[SC_COUNT + world + r]); }
    P.scal_r[SC_GMAX] = gm; P.flag_r[0] = fl != 0.0 ? 1 : 0;
  }
}
void reduce_scalars(covgpu_context* c) {
  if (!c->sharded || !c->reducer) return;
  hipLaunchKernelGGL(k_shard_scal_pack, dim3(1), dim3(64), 0, c->st, c->P, c->d_red, c->rank, c->world);
  if (c->reducer->allreduce(c->d_red, (size_t)SC_COUNT + 2 * (size_t)c->world, 0, c->st) != 0) coll_latch(c);
  hipLaunchKernelGGL(k_shard_scal_unpack, dim3(1), dim3(64), 0, c->st, c->P, (const double*)c->d_red, c->world);
}
