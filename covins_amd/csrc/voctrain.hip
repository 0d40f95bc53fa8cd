// voctrain.hip — host side of covgpu_voc_train: DBoW2's TemplatedVocabulary::create for ORB descriptors. The tree
// grows level by level: the host keeps the nodes, builds each level's segment and tile tables, drives the seeding rounds and the
// k-means iterations of k_voctrain.hip (one word read back per iteration: did any association change), reads the level's centres and
// group sizes, and renumbers the nodes depth first at the end. The weights come from k_bow.hip's tree descent over the training rows
// and a per-set unique word count. A stateless batch call: the context lends its device and its stream only; its argument check
// (voc_train_check) is in batch_check.hpp.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "host.hpp"

using namespace covgpu;

static_assert(kVtWaveMax == COVGPU_VOCTRAIN_WAVE_MAX && kVtTile == COVGPU_VOCTRAIN_TILE && kVtMaxK == COVGPU_VOCTRAIN_MAX_K &&
              kVtThreads == COVGPU_VOCTRAIN_THREADS, "covgpu.h names the limits of k_voctrain.hip");

extern "C" void covgpu_default_voc_train_opts(covgpu_voc_train_opts* o) {
  if (!o) return;
  o->k = 10; o->L = 5; o->weighting = COVGPU_BOW_TF_IDF; o->scoring = COVGPU_BOW_L1_NORM;
  o->seed = 0; o->max_iterations = 100; o->scratch_kib = 65536;
}

extern "C" void covgpu_voc_train_limits(int32_t out[4]) {
  if (!out) return;
  out[0] = kVtWaveMax; out[1] = kVtTile; out[2] = kVtMaxK; out[3] = kVtThreads;
}

namespace {

uint64_t mix64(uint64_t x) {                      // splitmix64
  uint64_t z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

struct HostNode {
  int parent, level, beg, n;                      // rows: positions [beg, beg + n) of the level that made the node
  int child0 = -1, nchild = 0;                    // children are consecutive in creation (breadth-first) order
  uint64_t key;
  uint4 d[2];
};

}  // namespace

extern "C" int covgpu_voc_train_check(const covgpu_voc_train_t* p, const covgpu_voc_train_opts* o) {
  return check_export("covgpu_voc_train_check", [&] { return voc_train_check(p, o); });
}

extern "C" int covgpu_voc_train(covgpu_context* c, const covgpu_voc_train_t* p, const covgpu_voc_train_opts* o) {
  return batch_entry("covgpu_voc_train", c, [&](auto bad) -> int {
    if (const char* m = voc_train_check(p, o)) return bad(m);
    const int S = p->num_sets, k = o->k, L = o->L;
    const size_t R = (size_t)p->row_ptr[S], ks = (size_t)k;
    int64_t st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int64_t& up = st[6];
    int64_t& down = st[7];
    // host staging of the level read-backs and of the weights (declared before the scratch that fills them)
    std::vector<int32_t> h_ncent, h_sizes, h_iters, h_done, h_ni;
    std::vector<uint4> h_cent;
    int h_any = 0;
    long long h_stats[8];
    HIPCHK(hipSetDevice(c->device));
    DeviceScratch U(c->st);
    VocTrainDev D{};
    D.k = k;
    unsigned char* ddesc = nullptr;
    int *perm_a = nullptr, *perm_b = nullptr;
    HIPCHK(U.upload(&ddesc, p->desc, 32 * R)); up += 32 * (int64_t)R;
    D.desc = reinterpret_cast<const uint4*>(ddesc);
    {
      std::vector<int32_t> iota(R);
      for (size_t r = 0; r < R; ++r) iota[r] = (int32_t)r;
      HIPCHK(U.upload(&perm_a, iota.data(), R)); up += 4 * (int64_t)R;
      HIPCHK(hipStreamSynchronize(c->st));        // iota goes out of scope
    }
    HIPCHK(U.alloc(&perm_b, R)); HIPCHK(U.alloc(&D.min_d, R)); HIPCHK(U.alloc(&D.assoc, R));
    HIPCHK(U.zeroed(&D.stats, 8)); HIPCHK(U.alloc(&D.any, 1));

    std::vector<HostNode> nodes(1);
    nodes[0].parent = -1; nodes[0].level = 0; nodes[0].beg = 0; nodes[0].n = (int)R; nodes[0].key = o->seed;
    nodes[0].d[0] = nodes[0].d[1] = uint4{0, 0, 0, 0};
    std::vector<int> cur(1, 0);
    for (int level = 1; level <= L && !cur.empty(); ++level) {
      st[5] = level;
      const size_t NS = cur.size();
      std::vector<int32_t> seg_beg(NS), seg_n(NS), seg_tile0(NS), seg_ntiles(NS), seg_slot(NS), slot_seg;
      std::vector<unsigned long long> seg_key(NS);
      std::vector<int4> wide, narrow;
      // tiles: the wide ones first, so a segment's tile numbers are known only once both lists are complete
      for (size_t s = 0; s < NS; ++s) {
        const HostNode& nd = nodes[cur[s]];
        seg_beg[s] = nd.beg; seg_n[s] = nd.n; seg_key[s] = nd.key; seg_slot[s] = -1; seg_tile0[s] = 0; seg_ntiles[s] = 0;
        if (nd.n <= k) continue;
        if (nd.n <= kVtWaveMax) { seg_tile0[s] = (int)narrow.size(); seg_ntiles[s] = 1; narrow.push_back(int4{(int)s, nd.beg, nd.beg + nd.n, 0}); continue; }
        seg_tile0[s] = (int)wide.size(); seg_ntiles[s] = (nd.n + kVtTile - 1) / kVtTile;
        for (int b = 0; b < nd.n; b += kVtTile) wide.push_back(int4{(int)s, nd.beg + b, nd.beg + std::min(nd.n, b + kVtTile), 0});
        if (seg_ntiles[s] > 1) { seg_slot[s] = (int)slot_seg.size(); slot_seg.push_back((int)s); }
      }
      const int NW = (int)wide.size(), NN = (int)narrow.size();
      for (size_t s = 0; s < NS; ++s) if (seg_n[s] > k && seg_n[s] <= kVtWaveMax) seg_tile0[s] += NW;
      std::vector<int4> tiles(wide);
      tiles.insert(tiles.end(), narrow.begin(), narrow.end());
      const size_t NT = tiles.size(), NSL = slot_seg.size();
      D.num_seg = (int)NS; D.num_slots = (int)NSL;
      D.perm = perm_a; D.perm_out = perm_b;
      HIPCHK(U.upload(&D.seg_beg, seg_beg.data(), NS)); HIPCHK(U.upload(&D.seg_n, seg_n.data(), NS));
      HIPCHK(U.upload(&D.seg_key, seg_key.data(), NS)); HIPCHK(U.upload(&D.seg_tile0, seg_tile0.data(), NS));
      HIPCHK(U.upload(&D.seg_ntiles, seg_ntiles.data(), NS)); HIPCHK(U.upload(&D.seg_slot, seg_slot.data(), NS));
      HIPCHK(U.upload(&D.tiles, tiles.data(), NT)); HIPCHK(U.upload(&D.slot_seg, slot_seg.data(), NSL));
      up += (int64_t)(NS * (5 * 4 + 8) + NT * 16 + NSL * 4);
      HIPCHK(U.alloc(&D.ncent, NS)); HIPCHK(U.alloc(&D.draws, NS)); HIPCHK(U.alloc(&D.seed_done, NS)); HIPCHK(U.alloc(&D.done, NS));
      HIPCHK(U.alloc(&D.iters, NS)); HIPCHK(U.alloc(&D.changed, NS)); HIPCHK(U.alloc(&D.cut, NS)); HIPCHK(U.alloc(&D.pick_tile, NS));
      HIPCHK(U.alloc(&D.pick_base, NS)); HIPCHK(U.alloc(&D.tile_sum, NT)); HIPCHK(U.alloc(&D.tile_cnt, NT * ks));
      HIPCHK(U.alloc(&D.cent, NS * ks * 2)); HIPCHK(U.zeroed(&D.sizes, NS * ks));
      HIPCHK(U.alloc(&D.gcnt, NSL * ks * 256)); HIPCHK(U.alloc(&D.gsize, NSL * ks));
      launch_vt_begin(D, c->st);
      if (NT) {
        for (int round = 1; round < k; ++round) launch_vt_seed_round(D, NW, NN, round == 1, c->st);
        for (int it = 1; it <= o->max_iterations; ++it) {
          if (it > 1) {
            if (NSL) { HIPCHK(hipMemsetAsync(D.gcnt, 0, NSL * ks * 256 * 4, c->st)); HIPCHK(hipMemsetAsync(D.gsize, 0, NSL * ks * 4, c->st)); }
            launch_vt_means(D, NW, NN, c->st);
          }
          HIPCHK(hipMemsetAsync(D.any, 0, 4, c->st));
          launch_vt_assoc(D, NW, NN, it == 1, c->st);
          HIPCHK(hipGetLastError());
          HIPCHK(hipMemcpyAsync(&h_any, D.any, 4, hipMemcpyDeviceToHost, c->st));
          HIPCHK(hipStreamSynchronize(c->st));
          down += 4;
          if (!h_any) break;
        }
        launch_vt_partition(D, NW, NN, c->st);
      }
      HIPCHK(hipGetLastError());
      h_ncent.resize(NS); h_sizes.resize(NS * ks); h_iters.resize(NS); h_done.resize(NS); h_cent.resize(NS * ks * 2);
      HIPCHK(U.fetch(h_ncent.data(), D.ncent, NS)); HIPCHK(U.fetch(h_sizes.data(), D.sizes, NS * ks));
      HIPCHK(U.fetch(h_iters.data(), D.iters, NS)); HIPCHK(U.fetch(h_done.data(), D.done, NS));
      HIPCHK(U.fetch(h_cent.data(), D.cent, NS * ks * 2));
      HIPCHK(hipStreamSynchronize(c->st));
      down += (int64_t)(NS * 12 + NS * ks * 36);
      std::vector<int> next;
      for (size_t s = 0; s < NS; ++s) {
        const int id = cur[s];
        st[0] += h_iters[s]; st[1] = std::max<int64_t>(st[1], h_iters[s]);
        if (seg_n[s] > k && !h_done[s]) ++st[2];
        nodes[id].child0 = (int)nodes.size(); nodes[id].nchild = h_ncent[s];
        int at = seg_beg[s];
        for (int cl = 0; cl < h_ncent[s]; ++cl) {
          HostNode ch;
          ch.parent = id; ch.level = level; ch.beg = at; ch.n = h_sizes[s * ks + cl];
          ch.key = mix64(nodes[id].key + 1 + (uint64_t)cl);
          ch.d[0] = h_cent[(s * ks + cl) * 2]; ch.d[1] = h_cent[(s * ks + cl) * 2 + 1];
          at += ch.n;
          if (level < L && ch.n > 1) next.push_back((int)nodes.size());
          nodes.push_back(ch);
        }
      }
      if (NT) std::swap(perm_a, perm_b);
      cur.swap(next);
    }
    HIPCHK(U.fetch(h_stats, D.stats, 8));
    HIPCHK(hipStreamSynchronize(c->st));
    down += 64;
    st[3] = h_stats[3]; st[4] = h_stats[4];

    // the reference's node ids: a node's children get consecutive ids when the node is processed, depth first
    const size_t N = nodes.size();
    std::vector<int32_t> newid(N, 0), order(N, 0);   // order: new id -> creation id
    {
      int nextid = 1;
      std::vector<std::pair<int, int>> stack;     // (node, next child to descend into)
      auto number = [&](int n) { for (int i = 0; i < nodes[n].nchild; ++i) { newid[nodes[n].child0 + i] = nextid; order[nextid++] = nodes[n].child0 + i; } };
      number(0);
      stack.emplace_back(0, 0);
      while (!stack.empty()) {
        auto& top = stack.back();
        if (top.second >= nodes[top.first].nchild) { stack.pop_back(); continue; }
        const int ch = nodes[top.first].child0 + top.second++;
        if (nodes[ch].nchild > 0) { number(ch); stack.emplace_back(ch, 0); }
      }
    }
    std::vector<int32_t> parent(N), word_id(N, -1), child_ptr(N + 1, 0), child(N - 1);
    std::vector<uint4> desc(2 * N);
    int W = 0;
    for (size_t i = 0; i < N; ++i) {
      const HostNode& nd = nodes[order[i]];
      parent[i] = i ? newid[nd.parent] : -1;
      desc[2 * i] = nd.d[0]; desc[2 * i + 1] = nd.d[1];
      if (i && nd.nchild == 0) word_id[i] = W++;
      child_ptr[i + 1] = child_ptr[i] + nd.nchild;
      for (int j = 0; j < nd.nchild; ++j) child[child_ptr[i] + j] = newid[nd.child0 + j];
    }
    if (W > COVGPU_BOW_MAX_WORDS) return bad("the tree has more than COVGPU_BOW_MAX_WORDS words");   // (only through emptied clusters)

    // setNodeWeights: the transform leaf of every row, then per word the sets that hold it
    std::vector<double> weight(N, 0.0);
    const bool idf = o->weighting == COVGPU_BOW_TF_IDF || o->weighting == COVGPU_BOW_IDF;
    const bool fits = N <= (size_t)p->node_capacity;
    if (fits && (idf || p->row_word)) {
      BowVocabDev V{};
      V.num_nodes = (int)N;
      int *drw = nullptr, *drn = nullptr;
      HIPCHK(U.upload(&V.child_ptr, child_ptr.data(), N + 1)); HIPCHK(U.upload(&V.child, child.data(), N - 1));
      HIPCHK(U.upload(&V.desc, desc.data(), 2 * N)); HIPCHK(U.upload(&V.word_id, word_id.data(), N));
      up += (int64_t)(N * 44);
      HIPCHK(U.alloc(&drw, R)); HIPCHK(U.alloc(&drn, R));
      launch_bow_descend(V, ddesc, (int)R, drw, drn, c->st);
      if (idf) {
        std::vector<int32_t> row_set(R);
        for (int s = 0; s < S; ++s) for (int r = p->row_ptr[s]; r < p->row_ptr[s + 1]; ++r) row_set[r] = s;
        int *dset = nullptr, *dni = nullptr;
        unsigned* dbits = nullptr;
        const size_t words32 = ((size_t)W + 31) / 32;
        const size_t chunk = std::min<size_t>((size_t)S, std::max<size_t>(1, (size_t)o->scratch_kib * 256 / words32));   // sets per pass
        HIPCHK(U.upload(&dset, row_set.data(), R)); up += 4 * (int64_t)R;
        HIPCHK(U.zeroed(&dni, (size_t)W)); HIPCHK(U.alloc(&dbits, chunk * words32));
        for (size_t s0 = 0; s0 < (size_t)S; s0 += chunk) {
          const size_t s1 = std::min<size_t>(S, s0 + chunk);
          if (p->row_ptr[s1] == p->row_ptr[s0]) continue;
          HIPCHK(hipMemsetAsync(dbits, 0, (s1 - s0) * words32 * 4, c->st));
          launch_vt_unique_words(dset, drw, p->row_ptr[s0], p->row_ptr[s1], (int)s0, (int)words32, dbits, dni, c->st);
        }
        HIPCHK(hipGetLastError());
        h_ni.resize(W);
        HIPCHK(U.fetch(h_ni.data(), dni, (size_t)W)); down += 4 * (int64_t)W;
        HIPCHK(hipStreamSynchronize(c->st));      // row_set goes out of scope
      }
      HIPCHK(hipGetLastError());
      if (p->row_word) { HIPCHK(U.fetch(p->row_word, drw, R)); down += 4 * (int64_t)R; }
      HIPCHK(hipStreamSynchronize(c->st));
    }
    *p->num_nodes = (int32_t)N;
    if (!fits) return bad("node_capacity too small: the tree has " + std::to_string(N) + " nodes");
    for (size_t i = 1; i < N; ++i) {
      if (word_id[i] < 0) continue;
      if (!idf) weight[i] = 1.0;
      else if (h_ni[word_id[i]] > 0) weight[i] = std::log((double)S / (double)h_ni[word_id[i]]);
    }
    *p->num_words = W;
    std::memcpy(p->parent, parent.data(), 4 * N); std::memcpy(p->desc_out, desc.data(), 32 * N);
    std::memcpy(p->word_id, word_id.data(), 4 * N); std::memcpy(p->weight, weight.data(), 8 * N);
    if (p->stats) std::memcpy(p->stats, st, sizeof st);
    return COVGPU_OK;
  });
}
