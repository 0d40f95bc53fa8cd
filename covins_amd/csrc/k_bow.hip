// k_bow.hip — bag-of-words retrieval for the loop detector: DBoW2's TemplatedVocabulary::transform with L1
// normalisation (TemplatedVocabulary.h:1127-1259, BowVector.cpp:34-84), L1Scoring::score (ScoringObject.cpp:23-68), the reference
// minimum score of PlaceRecognition::DetectLoop (placerec_be.cpp:372-389) and KeyframeDatabase::DetectCandidates
// (kf_database.cpp:47-187). Every floating-point sum runs in the reference's order, one thread per sum, so values carry the
// reference's bits; all atomics are integer atomics.
//
// Transform: k_bow_descend walks the tree, one thread per descriptor (its row in 8 VGPRs, the lowest node ids staged in LDS);
// k_bow_reduce, one workgroup per set, sorts (word, row) keys in LDS, forms each word's sum in row order and the norm in word order.
// Query: k_bow_count walks the inverted index of the database with integer counters (the resident database of k_bowdb.hip counts the
// positions outside its index beside it); k_bow_filter applies the per-keyframe filters
// and takes maxCommonWords; k_bow_score_entries scores the entries above the common-word cut; k_bow_accumulate adds the scores of
// the first 10 neighbours; k_bow_select orders the retained entries by (first common word, insertion position) with a counting
// sort and replays the dedup in one lane.
#include "common.hpp"

namespace covgpu {

namespace {

constexpr int kThreads = 256;
constexpr int kStageNodes = 128;                  // nodes 0..127 (4 KiB of descriptors) are read from LDS by the descent
constexpr int kSortMax = COVGPU_MATCH_MAX_ROWS;   // rows per set
constexpr unsigned kNoKey = 0xffffffffu;          // a stopped row: sorts behind every (word, row) key
constexpr int kConnected = -(1 << 30);            // counter start of an entry connected to the query: never becomes positive

__device__ __forceinline__ int hamming256(const uint4& a0, const uint4& a1, const uint4& b0, const uint4& b1) {
  int d = __builtin_popcount(a0.x ^ b0.x);
  d += __builtin_popcount(a0.y ^ b0.y);
  d += __builtin_popcount(a0.z ^ b0.z);
  d += __builtin_popcount(a0.w ^ b0.w);
  d += __builtin_popcount(a1.x ^ b1.x);
  d += __builtin_popcount(a1.y ^ b1.y);
  d += __builtin_popcount(a1.z ^ b1.z);
  d += __builtin_popcount(a1.w ^ b1.w);
  return d;
}

// TemplatedVocabulary::transform(feature, word_id, weight, nid, levelsup): the first child of the smallest distance wins (strict <).
__global__ __launch_bounds__(kThreads) void k_bow_descend(BowVocabDev V, const uint4* desc, int rows, int nid_level, int* row_word,
                                                          int* row_node) {
  __shared__ uint4 sN[kStageNodes][2];
  const int staged = min(V.num_nodes, kStageNodes);
  for (int i = threadIdx.x; i < 2 * staged; i += kThreads) sN[i >> 1][i & 1] = V.desc[i];
  __syncthreads();
  const int r = blockIdx.x * kThreads + (int)threadIdx.x;
  if (r >= rows) return;
  const uint4 q0 = desc[2 * (size_t)r], q1 = desc[2 * (size_t)r + 1];
  int node = 0, level = 0, nid = nid_level <= 0 ? 0 : -1;
  do {
    ++level;
    const int c0 = V.child_ptr[node], c1 = V.child_ptr[node + 1];
    int best = -1, best_d = 1 << 20;
    for (int c = c0; c < c1; ++c) {
      const int n = V.child[c];
      const int d = n < staged ? hamming256(q0, q1, sN[n][0], sN[n][1])
                               : hamming256(q0, q1, V.desc[2 * (size_t)n], V.desc[2 * (size_t)n + 1]);
      if (d < best_d) { best_d = d; best = n; }
    }
    node = best;
    if (level == nid_level) nid = node;
  } while (V.word_id[node] < 0);
  if (nid < 0) nid = node;                        // the leaf lies above nid_level (irregular tree): the leaf itself
  const int w = V.word_id[node];
  row_word[r] = !V.word_weight || V.word_weight[w] > 0.0 ? w : -1;   // a stopped word is dropped (no weights: vocabulary training)
  row_node[r] = nid;
}

// One workgroup per set. Output: the set's words (ascending) and normalised values at [row_ptr[s], row_ptr[s] + count[s]).
__global__ __launch_bounds__(kThreads) void k_bow_reduce(const int* row_ptr, const int* row_word, const double* word_weight, int add_weight,
                                                         int* out_word, double* out_value, int* count) {
  __shared__ unsigned sKey[kSortMax];
  __shared__ double sVal[kSortMax];
  __shared__ int sCnt[kThreads];
  __shared__ double sNorm;
  const int s = blockIdx.x, tid = (int)threadIdx.x;
  const int r0 = row_ptr[s], n = row_ptr[s + 1] - r0;
  if (n <= 0) { if (tid == 0) count[s] = 0; return; }
  int P = 1;
  while (P < n) P <<= 1;                          // n <= kSortMax, a power of two
  for (int i = tid; i < P; i += kThreads) {
    const int w = i < n ? row_word[r0 + i] : -1;
    sKey[i] = w < 0 ? kNoKey : (((unsigned)w << 12) | (unsigned)i);   // word < 2^20 - 1, i < 2^12: never kNoKey
  }
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1) {              // bitonic sort, ascending
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < P; i += kThreads) {
        const int l = i ^ j;
        if (l > i) {
          const unsigned a = sKey[i], b = sKey[l];
          if (((i & k) == 0) == (a > b)) { sKey[i] = b; sKey[l] = a; }
        }
      }
      __syncthreads();
    }
  }
  // heads of the runs of equal words: thread t owns the sorted elements [t * per, t * per + per)
  const int per = (P + kThreads - 1) / kThreads, i0 = tid * per, i1 = min(P, i0 + per);
  int heads = 0;
  for (int i = i0; i < i1; ++i) {
    const unsigned k = sKey[i];
    if (k != kNoKey && (i == 0 || (sKey[i - 1] >> 12) != (k >> 12))) ++heads;
  }
  sCnt[tid] = heads;
  __syncthreads();
  for (int off = 1; off < kThreads; off <<= 1) {  // inclusive scan
    const int v = tid >= off ? sCnt[tid - off] : 0;
    __syncthreads();
    sCnt[tid] += v;
    __syncthreads();
  }
  const int U = sCnt[kThreads - 1];
  int p = sCnt[tid] - heads;
  for (int i = i0; i < i1; ++i) {
    const unsigned k = sKey[i];
    if (k == kNoKey || !(i == 0 || (sKey[i - 1] >> 12) != (k >> 12))) continue;
    const double w = word_weight[k >> 12];
    double v = w;                                 // addWeight: insert w, then += w once per further feature, in feature order
    if (add_weight)
      for (int e = i + 1; e < P && sKey[e] != kNoKey && (sKey[e] >> 12) == (k >> 12); ++e) v += w;
    out_word[r0 + p] = (int)(k >> 12);
    sVal[p] = v;
    ++p;
  }
  __syncthreads();
  if (tid == 0) {                                 // BowVector::normalize(L1): the sum in ascending word order
    double norm = 0.0;
    for (int i = 0; i < U; ++i) norm += fabs(sVal[i]);
    sNorm = norm;
    count[s] = U;
  }
  __syncthreads();
  const double norm = sNorm;
  for (int i = tid; i < U; i += kThreads) out_value[r0 + i] = norm > 0.0 ? sVal[i] / norm : sVal[i];
}

// L1Scoring::score over two sorted sparse vectors: the common words in ascending order, one sequential sum.
__device__ double bow_score(const int* word, const double* value, int a0, int a1, int b0, int b1) {
  double s = 0.0;
  int i = a0, j = b0;
  while (i < a1 && j < b1) {
    const int wi = word[i], wj = word[j];
    if (wi == wj) {
      const double vi = value[i], wv = value[j];
      s += fabs(vi - wv) - fabs(vi) - fabs(wv);
      ++i; ++j;
    } else if (wi < wj) {
      ++i;
    } else {
      ++j;
    }
  }
  return -s / 2.0;
}

__global__ __launch_bounds__(kThreads) void k_bow_score_pairs(const int* vec_beg, const int* vec_end, const int* word, const double* value,
                                                              int num_pairs, const int* pa, const int* pb, double* score) {
  const int i = blockIdx.x * kThreads + (int)threadIdx.x;
  if (i >= num_pairs) return;
  const int a = pa[i], b = pb[i];
  score[i] = bow_score(word, value, vec_beg[a], vec_end[a], vec_beg[b], vec_end[b]);
}

// placerec_be.cpp:374-389: float minScore = 1; the float of each valid neighbour's score; min_score = (double)minScore * factor.
__global__ __launch_bounds__(kThreads) void k_bow_min_score(int num_queries, const int* pair_off, const double* pair_score,
                                                            double factor, double* min_score) {
  const int q = blockIdx.x * kThreads + (int)threadIdx.x;
  if (q >= num_queries) return;
  float m = 1.0f;
  for (int i = pair_off[q]; i < pair_off[q + 1]; ++i) {
    const float s = (float)pair_score[i];
    if (s < m) m = s;
  }
  min_score[q] = (double)m * factor;
}

// Scratch of a chunk of queries: [chunk][M] each. common: the common-word counter (0 after the filter = not in the sharing list);
// first: the smallest index into the query's word list that the entry shares (the first-encounter key; later the dedup's mark).
__global__ __launch_bounds__(kThreads) void k_bow_init(int n, int* common, int* first) {
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= (size_t)n) return;
  common[i] = 0; first[i] = INT32_MAX;
}

__global__ __launch_bounds__(kThreads) void k_bow_mark_connected(DetectDev D, int q0, int* common) {
  const int qc = blockIdx.x, c = D.con_by_query ? q0 + qc : D.query_kf[q0 + qc];
  for (int i = D.con_beg[c] + (int)threadIdx.x; i < D.con_end[c]; i += kThreads) {
    const int p = D.pos_of[D.con[i]];
    if (p >= 0) common[(size_t)qc * D.M + p] = kConnected;
  }
}

constexpr int kCountSlices = 4;                   // workgroups per query in k_bow_count

__global__ __launch_bounds__(kThreads) void k_bow_count(DetectDev D, int q0, int* common, int* first) {
  const int qc = blockIdx.x / kCountSlices, slice = blockIdx.x % kCountSlices;
  const int q = q0 + qc, kf = D.query_kf[q], vis = D.db_visible[q];
  const int w0 = D.vec_beg[kf], nw = D.vec_end[kf] - w0;
  int* cm = common + (size_t)qc * D.M;
  int* fs = first + (size_t)qc * D.M;
  for (int j = slice; j < nw; j += kCountSlices) {
    const int w = D.word[w0 + j];
    if (w >= D.inv_words) continue;
    for (int e = D.inv_ptr[w] + (int)threadIdx.x; e < D.inv_ptr[w + 1]; e += kThreads) {
      const int p = D.inv_pos[e];
      if (p < vis) { atomicAdd(&cm[p], 1); atomicMin(&fs[p], j); }
    }
  }
}

__global__ __launch_bounds__(kThreads) void k_bow_filter(DetectDev D, DetectOptsDev O, int q0, int nq, int* common) {
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= (size_t)nq * D.M) return;
  const int qc = (int)(i / D.M), p = (int)(i % D.M), q = q0 + qc;
  int c = common[i];
  if (c == 0) return;
  if (D.dead && D.dead[p]) {
    c = 0;                                        // an erased position: its postings stay in the index until the next rebuild
  } else if (c > 0) {
    const int kq = D.query_kf[q], ki = D.db_order[p];
    const int idq = D.id[kq], idi = D.id[ki];
    const bool same = D.client[kq] == D.client[ki];
    if ((idi == idq && same) || (O.inter_only && same) || (same && abs(idq - idi) < O.min_loop_dist) || idi < O.exclude_below) c = 0;
  } else {
    c = 0;                                        // connected to the query: never joins the sharing list
  }
  common[i] = c;
  if (c > 0) { atomicMax(&D.max_common[q], c); atomicAdd(&D.num_sharing[q], 1); }
}

__device__ __forceinline__ int min_common_words(int max_common) { return (int)((float)max_common * 0.8f); }

__global__ __launch_bounds__(kThreads) void k_bow_score_entries(DetectDev D, int q0, int nq, const int* common, double* score) {
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= (size_t)nq * D.M) return;
  const int qc = (int)(i / D.M), p = (int)(i % D.M), q = q0 + qc;
  if (common[i] <= min_common_words(D.max_common[q])) return;       // common > 0 here: max_common >= 1 where any entry shares
  const int kq = D.query_kf[q], ki = D.db_order[p];
  score[i] = bow_score(D.word, D.value, D.vec_beg[kq], D.vec_end[kq], D.vec_beg[ki], D.vec_end[ki]);
  atomicAdd(&D.num_scored[q], 1);
}

// kf_database.cpp:129-164 for one lScoreAndMatch entry: best = -1 marks an entry that is not in lScoreAndMatch.
__global__ __launch_bounds__(kThreads) void k_bow_accumulate(DetectDev D, int q0, int nq, const int* common, const double* score, float* acc,
                                                             int* best) {
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= (size_t)nq * D.M) return;
  const int qc = (int)(i / D.M), p = (int)(i % D.M), q = q0 + qc;
  const int cut = min_common_words(D.max_common[q]);
  const size_t base = (size_t)qc * D.M;
  if (common[i] <= cut || !(score[i] >= D.min_score[q])) { acc[i] = -1.0f; best[i] = -1; return; }
  float best_score = (float)score[i], a = (float)score[i];
  int bp = p;
  const int ki = D.db_order[p], n0 = D.nb_beg[ki], n1 = min(D.nb_end[ki], n0 + 10), vis = D.db_visible[q];
  for (int e = n0; e < n1; ++e) {
    const int p2 = D.pos_of[D.nb[e]];
    if (p2 < 0 || p2 >= vis || common[base + p2] <= cut) continue;  // loop_query_ == kf->id_ && loop_words_ > minCommonWords
    const double s2 = score[base + p2];
    a = (float)((double)a + s2);                                    // float accScore += double loop_score_
    if (s2 > (double)best_score) { bp = p2; best_score = (float)s2; }
  }
  acc[i] = a; best[i] = bp;
}

// One workgroup per query: threshold, order, dedup.
__global__ __launch_bounds__(kThreads) void k_bow_select(DetectDev D, int q0, int cap, int hist_stride, const float* acc_all, const int* best_all,
                                                         int* first_all, int* order_all, int* hist_all) {
  __shared__ float sMax[kThreads];
  __shared__ int sBucket[kThreads];
  __shared__ int sIdx[kThreads];
  const int qc = blockIdx.x, q = q0 + qc, tid = (int)threadIdx.x, vis = D.db_visible[q];
  const size_t base = (size_t)qc * D.M;
  const float* acc = acc_all + base;
  const int* best = best_all + base;
  int* first = first_all + base;
  int* order = order_all + base;
  int* hist = hist_all + (size_t)qc * hist_stride;
  const int kq = D.query_kf[q], nw = D.vec_end[kq] - D.vec_beg[kq];
  float m = -INFINITY;
  for (int p = tid; p < vis; p += kThreads)
    if (best[p] >= 0) m = fmaxf(m, acc[p]);
  sMax[tid] = m;
  __syncthreads();
  for (int off = kThreads / 2; off > 0; off >>= 1) {
    if (tid < off) sMax[tid] = fmaxf(sMax[tid], sMax[tid + off]);
    __syncthreads();
  }
  double best_acc = D.min_score[q];                                 // precision_t bestAccScore = min_score
  if ((double)sMax[0] > best_acc) best_acc = (double)sMax[0];
  const float retain = (float)((double)0.75f * best_acc);           // float minScoreToRetain = 0.75f * bestAccScore
  for (int j = tid; j <= nw; j += kThreads) hist[j] = 0;
  __syncthreads();
  for (int p = tid; p < vis; p += kThreads)
    if (best[p] >= 0 && acc[p] > retain) atomicAdd(&hist[first[p]], 1);
  __syncthreads();
  if (tid == 0) {                                                   // exclusive scan: the first slot of each bucket
    int run = 0;
    for (int j = 0; j <= nw; ++j) { const int h = hist[j]; hist[j] = run; run += h; }
  }
  __syncthreads();
  const int kept = hist[nw];
  for (int c = 0; c < vis; c += kThreads) {                         // stable scatter, positions ascending
    const int p = c + tid;
    const bool on = p < vis && best[p] >= 0 && acc[p] > retain;
    const int b = on ? first[p] : -1;
    sBucket[tid] = b;
    __syncthreads();
    if (on) {
      int rank = 0;
      for (int t = 0; t < tid; ++t) rank += sBucket[t] == b;
      sIdx[tid] = hist[b] + rank;
    }
    __syncthreads();
    if (on) { order[sIdx[tid]] = p; atomicAdd(&hist[b], 1); }
    __syncthreads();
  }
  if (tid == 0) {                                                   // vpLoopCandidates: first occurrence of each best keyframe
    int n = 0;
    for (int i = 0; i < kept; ++i) {
      const int p = order[i], b = best[p];
      if (first[b] == -1) continue;
      first[b] = -1;
      if (n < cap) { D.candidates[(size_t)q * cap + n] = D.db_order[b]; D.acc_score[(size_t)q * cap + n] = acc[p]; }
      ++n;
    }
    D.num_candidates[q] = n;
  }
}

inline unsigned blocks(size_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

}  // namespace

void launch_bow_transform(const BowVocabDev& V, const unsigned char* desc, const int* row_ptr, int num_sets, int rows, int nid_level,
                          int add_weight, int* row_word, int* row_node, int* out_word, double* out_value, int* count, hipStream_t st) {
  if (rows > 0)
    hipLaunchKernelGGL(k_bow_descend, dim3(blocks(rows)), dim3(kThreads), 0, st, V, reinterpret_cast<const uint4*>(desc), rows, nid_level,
                       row_word, row_node);
  if (num_sets > 0)
    hipLaunchKernelGGL(k_bow_reduce, dim3(num_sets), dim3(kThreads), 0, st, row_ptr, row_word, V.word_weight, add_weight, out_word,
                       out_value, count);
}

void launch_bow_descend(const BowVocabDev& V, const unsigned char* desc, int rows, int* row_word, int* row_node, hipStream_t st) {
  if (rows > 0)
    hipLaunchKernelGGL(k_bow_descend, dim3(blocks(rows)), dim3(kThreads), 0, st, V, reinterpret_cast<const uint4*>(desc), rows, 0,
                       row_word, row_node);
}

void launch_bow_score_pairs(const int* vec_beg, const int* vec_end, const int* word, const double* value, int num_pairs, const int* a,
                            const int* b, double* score, hipStream_t st) {
  if (num_pairs > 0)
    hipLaunchKernelGGL(k_bow_score_pairs, dim3(blocks(num_pairs)), dim3(kThreads), 0, st, vec_beg, vec_end, word, value, num_pairs, a, b,
                       score);
}

void launch_bow_min_score(const DetectDev& D, int num_queries, const int* pair_off, const double* pair_score, double factor,
                          hipStream_t st) {
  if (num_queries > 0)
    hipLaunchKernelGGL(k_bow_min_score, dim3(blocks(num_queries)), dim3(kThreads), 0, st, num_queries, pair_off, pair_score, factor,
                       D.min_score);
}

void launch_bow_detect_chunk(const DetectDev& D, const DetectOptsDev& O, int q0, int nq, int cap, int hist_stride, int* common, int* first,
                             double* score, float* acc, int* best, int* order, int* hist, hipStream_t st) {
  if (nq <= 0) return;
  if (D.M <= 0) { return; }
  const size_t n = (size_t)nq * D.M;
  hipLaunchKernelGGL(k_bow_init, dim3(blocks(n)), dim3(kThreads), 0, st, (int)n, common, first);
  hipLaunchKernelGGL(k_bow_mark_connected, dim3(nq), dim3(kThreads), 0, st, D, q0, common);
  hipLaunchKernelGGL(k_bow_count, dim3(nq * kCountSlices), dim3(kThreads), 0, st, D, q0, common, first);
  launch_bowdb_tail_count(D, q0, nq, common, first, st);   // the positions outside the index (resident database only)
  hipLaunchKernelGGL(k_bow_filter, dim3(blocks(n)), dim3(kThreads), 0, st, D, O, q0, nq, common);
  hipLaunchKernelGGL(k_bow_score_entries, dim3(blocks(n)), dim3(kThreads), 0, st, D, q0, nq, common, score);
  hipLaunchKernelGGL(k_bow_accumulate, dim3(blocks(n)), dim3(kThreads), 0, st, D, q0, nq, common, score, acc, best);
  hipLaunchKernelGGL(k_bow_select, dim3(nq), dim3(kThreads), 0, st, D, q0, cap, hist_stride, acc, best, first, order, hist);
}

}  // namespace covgpu
