// k_bowdb.hip — device side of the resident keyframe database (covgpu_bowdb): the vocabulary, the bag-of-words vectors
// and the inverted index of KeyframeDatabase stay on the device across calls and change incrementally.
//
// A query is the chain of k_bow.hip (§4.13) over the database's positions. Positions below the watermark are in the base index and are
// counted by k_bow_count; the positions added since the last rebuild (the tail) are counted here by k_bowdb_tail_count, one thread per
// (query, tail position), which owns its element of `common` and `first`: no atomics. The rest of this file maintains the structure:
// storing vectors and neighbour rows, AddKeyframe / EraseKeyframe on the position arrays, and the rebuild, which renumbers the live
// positions, compacts the vector pool and builds the base index with integer atomics only. No kernel here does floating-point
// arithmetic: values are copied.
#include "common.hpp"

namespace covgpu {

namespace {

constexpr int kThreads = 256;
constexpr int kScanItems = 4;                     // elements per thread of one scan block
constexpr int kScanBlock = kThreads * kScanItems;

inline unsigned blocks(size_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

// The sorted merge of the query's word list with one tail entry's: the number of common words and the smallest index into the
// query's list that is shared (what k_bow_count reaches with atomicAdd / atomicMin over the posting lists).
__global__ __launch_bounds__(kThreads) void k_bowdb_tail_count(DetectDev D, int q0, int nq, int* common, int* first) {
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= (size_t)nq * D.tail) return;
  const int qc = (int)(i / D.tail), p = D.M - D.tail + (int)(i % D.tail), q = q0 + qc;
  if (p >= D.db_visible[q] || (D.dead && D.dead[p])) return;
  const int kq = D.query_kf[q], ki = D.db_order[p];
  const int a0 = D.vec_beg[kq], a1 = D.vec_end[kq], b1 = D.vec_end[ki];
  int a = a0, b = D.vec_beg[ki], cnt = 0, fst = INT32_MAX;
  while (a < a1 && b < b1) {
    const int wa = D.word[a], wb = D.word[b];
    if (wa == wb) {
      if (cnt == 0) fst = a - a0;
      ++cnt; ++a; ++b;
    } else if (wa < wb) {
      ++a;
    } else {
      ++b;
    }
  }
  if (cnt > 0) {
    const size_t e = (size_t)qc * D.M + p;
    common[e] += cnt;                             // on top of k_bow_mark_connected's start value; this thread is the only writer
    first[e] = fst;
  }
}

__global__ __launch_bounds__(kThreads) void k_bowdb_store_meta(int n, const int* slot, const int* id, const int* client, const int* beg,
                                                               const int* end, BowDbDev B) {
  const int i = blockIdx.x * kThreads + (int)threadIdx.x;
  if (i >= n) return;
  const int s = slot[i];
  B.id[s] = id[i]; B.client[s] = client[i]; B.vec_beg[s] = beg[i]; B.vec_end[s] = end[i];
}

// One workgroup per set: the transform's output of set s (at its first row) goes to the pool at dst[s].
__global__ __launch_bounds__(kThreads) void k_bowdb_gather(const int* row_ptr, const int* count, const int* dst, const int* src_word,
                                                           const double* src_value, int* pool_word, double* pool_value) {
  const int s = blockIdx.x, r0 = row_ptr[s], n = count[s], d0 = dst[s];
  for (int i = (int)threadIdx.x; i < n; i += kThreads) { pool_word[d0 + i] = src_word[r0 + i]; pool_value[d0 + i] = src_value[r0 + i]; }
}

__global__ __launch_bounds__(kThreads) void k_bowdb_set_neighbours(int n, const int* slot, const int* rows, const int* count, BowDbDev B) {
  const int i = blockIdx.x * kThreads + (int)threadIdx.x;
  if (i >= n * kBowDbNeighbours) return;
  const int r = i / kBowDbNeighbours, j = i % kBowDbNeighbours, s = slot[r];
  B.nb[(size_t)s * kBowDbNeighbours + j] = rows[i];
  if (j == 0) { B.nb_beg[s] = s * kBowDbNeighbours; B.nb_end[s] = s * kBowDbNeighbours + count[r]; }
}

__global__ __launch_bounds__(kThreads) void k_bowdb_add(int n, const int* slot, int p0, BowDbDev B) {
  const int i = blockIdx.x * kThreads + (int)threadIdx.x;
  if (i >= n) return;
  const int s = slot[i];
  B.db_order[p0 + i] = s; B.dead[p0 + i] = 0; B.pos_of[s] = p0 + i;
}

__global__ __launch_bounds__(kThreads) void k_bowdb_erase(int n, const int* slot, BowDbDev B) {
  const int i = blockIdx.x * kThreads + (int)threadIdx.x;
  if (i >= n) return;
  const int s = slot[i], p = B.pos_of[s];
  if (p >= 0) { B.dead[p] = 1; B.pos_of[s] = -1; }
}

// ---- exclusive scan of ints, any length: blocks of kScanBlock elements, the block sums scanned by the same kernels ----
// out[i] = sum of in[0 .. i) within the block, for i < n_out; in[i] counts as 0 from n_in on. in may be out.
__global__ __launch_bounds__(kThreads) void k_bowdb_scan_block(const int* in, int n_in, int* out, int n_out, int* block_sum) {
  __shared__ int s[kThreads];
  const int tid = (int)threadIdx.x;
  const size_t base = (size_t)blockIdx.x * kScanBlock + (size_t)tid * kScanItems;
  int e[kScanItems], sum = 0;
  for (int k = 0; k < kScanItems; ++k) {
    e[k] = sum;
    sum += base + k < (size_t)n_in ? in[base + k] : 0;
  }
  s[tid] = sum;
  __syncthreads();
  for (int off = 1; off < kThreads; off <<= 1) {  // inclusive scan of the threads' sums
    const int v = tid >= off ? s[tid - off] : 0;
    __syncthreads();
    s[tid] += v;
    __syncthreads();
  }
  const int before = s[tid] - sum;
  for (int k = 0; k < kScanItems; ++k)
    if (base + k < (size_t)n_out) out[base + k] = before + e[k];
  if (block_sum && tid == kThreads - 1) block_sum[blockIdx.x] = s[tid];
}

__global__ __launch_bounds__(kThreads) void k_bowdb_scan_add(int* out, int n_out, const int* block_off) {
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < (size_t)n_out) out[i] += block_off[i / kScanBlock];
}

// ---- rebuild ----
__global__ __launch_bounds__(kThreads) void k_bowdb_live_flags(int P, const unsigned char* dead, int* flag) {
  const int p = blockIdx.x * kThreads + (int)threadIdx.x;
  if (p < P) flag[p] = dead[p] ? 0 : 1;
}

// new_pos: the exclusive scan of the live flags. The survivors keep their order.
__global__ __launch_bounds__(kThreads) void k_bowdb_renumber(int P, const int* new_pos, int* new_order, BowDbDev B) {
  const int p = blockIdx.x * kThreads + (int)threadIdx.x;
  if (p >= P || B.dead[p]) return;
  const int s = B.db_order[p], np = new_pos[p];
  new_order[np] = s; B.pos_of[s] = np;
}

__global__ __launch_bounds__(kThreads) void k_bowdb_lengths(int N, BowDbDev B, int* len) {
  const int s = blockIdx.x * kThreads + (int)threadIdx.x;
  if (s < N) len[s] = B.vec_end[s] - B.vec_beg[s];
}

// One workgroup per slot: its vector moves to new_beg[slot] of the new pool (slot order), and the slot's range follows.
__global__ __launch_bounds__(kThreads) void k_bowdb_compact_pool(const int* new_beg, const int* old_word, const double* old_value,
                                                                 int* new_word, double* new_value, BowDbDev B) {
  const int s = blockIdx.x, b0 = B.vec_beg[s], n = B.vec_end[s] - b0, d0 = new_beg[s];
  for (int i = (int)threadIdx.x; i < n; i += kThreads) { new_word[d0 + i] = old_word[b0 + i]; new_value[d0 + i] = old_value[b0 + i]; }
  __syncthreads();                                // every thread has read the old range
  if (threadIdx.x == 0) { B.vec_beg[s] = d0; B.vec_end[s] = d0 + n; }
}

// One workgroup per live position: the word histogram of the database.
__global__ __launch_bounds__(kThreads) void k_bowdb_histogram(BowDbDev B, int* word_count) {
  const int s = B.db_order[blockIdx.x];
  for (int i = B.vec_beg[s] + (int)threadIdx.x; i < B.vec_end[s]; i += kThreads) atomicAdd(&word_count[B.word[i]], 1);
}

// One workgroup per live position: each of its words claims the next free place of that word's posting list. The places of one list
// are handed out in arrival order, so the order of positions inside a list varies from rebuild to rebuild. That is harmless:
// k_bow_count only does integer atomicAdd and atomicMin over a list, and both commute.
__global__ __launch_bounds__(kThreads) void k_bowdb_scatter(BowDbDev B, int* cursor, int* inv_pos) {
  const int p = blockIdx.x, s = B.db_order[p];
  for (int i = B.vec_beg[s] + (int)threadIdx.x; i < B.vec_end[s]; i += kThreads) inv_pos[atomicAdd(&cursor[B.word[i]], 1)] = p;
}

}  // namespace

void launch_bowdb_tail_count(const DetectDev& D, int q0, int nq, int* common, int* first, hipStream_t st) {
  if (nq <= 0 || D.tail <= 0) return;
  hipLaunchKernelGGL(k_bowdb_tail_count, dim3(blocks((size_t)nq * D.tail)), dim3(kThreads), 0, st, D, q0, nq, common, first);
}

void launch_bowdb_store_meta(const BowDbDev& B, int n, const int* slot, const int* id, const int* client, const int* beg, const int* end,
                             hipStream_t st) {
  if (n > 0) hipLaunchKernelGGL(k_bowdb_store_meta, dim3(blocks(n)), dim3(kThreads), 0, st, n, slot, id, client, beg, end, B);
}

void launch_bowdb_gather(int num_sets, const int* row_ptr, const int* count, const int* dst, const int* src_word, const double* src_value,
                         int* pool_word, double* pool_value, hipStream_t st) {
  if (num_sets > 0)
    hipLaunchKernelGGL(k_bowdb_gather, dim3(num_sets), dim3(kThreads), 0, st, row_ptr, count, dst, src_word, src_value, pool_word, pool_value);
}

void launch_bowdb_set_neighbours(const BowDbDev& B, int n, const int* slot, const int* rows, const int* count, hipStream_t st) {
  if (n > 0)
    hipLaunchKernelGGL(k_bowdb_set_neighbours, dim3(blocks((size_t)n * kBowDbNeighbours)), dim3(kThreads), 0, st, n, slot, rows, count, B);
}

void launch_bowdb_add(const BowDbDev& B, int n, const int* slot, int p0, hipStream_t st) {
  if (n > 0) hipLaunchKernelGGL(k_bowdb_add, dim3(blocks(n)), dim3(kThreads), 0, st, n, slot, p0, B);
}

void launch_bowdb_erase(const BowDbDev& B, int n, const int* slot, hipStream_t st) {
  if (n > 0) hipLaunchKernelGGL(k_bowdb_erase, dim3(blocks(n)), dim3(kThreads), 0, st, n, slot, B);
}

size_t bowdb_scan_tmp_ints(int n_out) {
  size_t tot = 0;
  for (size_t nb = ((size_t)n_out + kScanBlock - 1) / kScanBlock; nb > 1; nb = (nb + kScanBlock - 1) / kScanBlock) tot += nb;
  return tot + 1;
}

void launch_bowdb_scan(const int* in, int n_in, int* out, int n_out, int* tmp, hipStream_t st) {
  if (n_out <= 0) return;
  const int nb = (int)(((size_t)n_out + kScanBlock - 1) / kScanBlock);
  hipLaunchKernelGGL(k_bowdb_scan_block, dim3(nb), dim3(kThreads), 0, st, in, n_in, out, n_out, nb > 1 ? tmp : nullptr);
  if (nb <= 1) return;
  launch_bowdb_scan(tmp, nb, tmp, nb, tmp + nb, st);
  hipLaunchKernelGGL(k_bowdb_scan_add, dim3(blocks(n_out)), dim3(kThreads), 0, st, out, n_out, tmp);
}

void launch_bowdb_renumber(const BowDbDev& B, int P, int* new_pos, int* new_order, int* scan_tmp, hipStream_t st) {
  if (P <= 0) return;
  hipLaunchKernelGGL(k_bowdb_live_flags, dim3(blocks(P)), dim3(kThreads), 0, st, P, B.dead, new_pos);
  launch_bowdb_scan(new_pos, P, new_pos, P + 1, scan_tmp, st);
  hipLaunchKernelGGL(k_bowdb_renumber, dim3(blocks(P)), dim3(kThreads), 0, st, P, new_pos, new_order, B);
}

void launch_bowdb_compact_pool(const BowDbDev& B, int num_slots, int* new_beg, int* new_word, double* new_value, int* scan_tmp,
                               hipStream_t st) {
  if (num_slots <= 0) return;
  hipLaunchKernelGGL(k_bowdb_lengths, dim3(blocks(num_slots)), dim3(kThreads), 0, st, num_slots, B, new_beg);
  launch_bowdb_scan(new_beg, num_slots, new_beg, num_slots + 1, scan_tmp, st);
  hipLaunchKernelGGL(k_bowdb_compact_pool, dim3(num_slots), dim3(kThreads), 0, st, new_beg, B.word, B.value, new_word, new_value, B);
}

void launch_bowdb_histogram(const BowDbDev& B, int live, int* word_count, hipStream_t st) {
  if (live > 0) hipLaunchKernelGGL(k_bowdb_histogram, dim3(live), dim3(kThreads), 0, st, B, word_count);
}

void launch_bowdb_scatter(const BowDbDev& B, int live, int* cursor, int* inv_pos, hipStream_t st) {
  if (live > 0) hipLaunchKernelGGL(k_bowdb_scatter, dim3(live), dim3(kThreads), 0, st, B, cursor, inv_pos);
}

}  // namespace covgpu
