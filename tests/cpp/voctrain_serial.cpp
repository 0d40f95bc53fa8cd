// voctrain_serial.cpp — a serial C++ restatement of vocabulary training: create / HKmeansStep / k-means++ seeding /
// meanValue / distance / createWords / setNodeWeights for 32-byte binary descriptors, recursing depth first as DBoW2 does, with the
// departures D1-D4 (counter-based draws, an emptied cluster keeps its centre, the iteration cap, refused inputs). It shares no code with
// the library or with tests/voctrain_ref.py; tests/test_voctrain_host.py holds the numpy restatement to it bit for bit, and
// tools/voctrain_bench.py times it as the CPU side. Plain C++17, no dependencies.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

struct Desc { uint64_t w[4]; };

uint64_t mix(uint64_t x) {
  uint64_t z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

double draw(uint64_t key, int j) { return (double)(mix(mix(key) + (uint64_t)j) >> 11) * 0x1.0p-53; }

int dist(const Desc& a, const Desc& b) {
  int d = 0;
  for (int i = 0; i < 4; ++i) d += __builtin_popcountll(a.w[i] ^ b.w[i]);
  return d;
}

struct Trainer {
  int k, L, max_iterations;
  const Desc* rows;
  std::vector<int> parent;
  std::vector<Desc> centre;
  std::vector<int> nchild;
  int64_t stats[6] = {0, 0, 0, 0, 0, 0};

  // the centre of a non-empty group: bit b is set iff at least n / 2 + n % 2 members have it
  Desc mean(const std::vector<int>& members) const {
    const int n = (int)members.size();
    if (n == 1) return rows[members[0]];
    int cnt[256] = {0};
    for (int r : members)
      for (int q = 0; q < 4; ++q)
        for (uint64_t w = rows[r].w[q]; w; w &= w - 1) ++cnt[64 * q + __builtin_ctzll(w)];
    Desc m{{0, 0, 0, 0}};
    const int need = n / 2 + n % 2;
    for (int b = 0; b < 256; ++b)
      if (cnt[b] >= need) m.w[b >> 6] |= 1ull << (b & 63);
    return m;
  }

  std::vector<Desc> seed(const std::vector<int>& idx, uint64_t key) {
    const int n = (int)idx.size();
    int j = 0;
    std::vector<Desc> c;
    c.push_back(rows[idx[std::min((int)(draw(key, j++) * (double)n), n - 1)]]);
    std::vector<int> nearest(n);
    for (int i = 0; i < n; ++i) nearest[i] = dist(rows[idx[i]], c[0]);
    while ((int)c.size() < k) {
      uint64_t total = 0;
      for (int i = 0; i < n; ++i) { nearest[i] = std::min(nearest[i], dist(rows[idx[i]], c.back())); total += (uint64_t)nearest[i]; }
      if (total == 0) { ++stats[4]; break; }
      double cut = 0.0;
      for (int tries = 0; tries < 64 && cut == 0.0; ++tries) cut = draw(key, j++) * (double)total;
      int pick = n - 1;
      uint64_t run = 0;
      for (int i = 0; i < n; ++i) {
        run += (uint64_t)nearest[i];
        if ((double)run >= cut) { pick = i; break; }
      }
      c.push_back(rows[idx[pick]]);
    }
    return c;
  }

  void step(int node, const std::vector<int>& idx, int level, uint64_t key) {
    const int n = (int)idx.size();
    stats[5] = std::max<int64_t>(stats[5], level);
    std::vector<Desc> c;
    std::vector<int> which(n);
    if (n <= k) {
      for (int i = 0; i < n; ++i) { c.push_back(rows[idx[i]]); which[i] = i; }
    } else {
      c = seed(idx, key);
      std::vector<int> before;
      bool settled = false;
      int it = 0;
      while (it < max_iterations) {
        if (it > 0) {
          for (size_t q = 0; q < c.size(); ++q) {
            std::vector<int> members;
            for (int i = 0; i < n; ++i) if (before[i] == (int)q) members.push_back(idx[i]);
            if (members.empty()) ++stats[3];
            else c[q] = mean(members);
          }
        }
        for (int i = 0; i < n; ++i) {
          int best = 0, bd = dist(rows[idx[i]], c[0]);
          for (size_t q = 1; q < c.size(); ++q) { const int d = dist(rows[idx[i]], c[q]); if (d < bd) { bd = d; best = (int)q; } }
          which[i] = best;
        }
        ++it;
        if (it > 1 && which == before) { settled = true; break; }
        before = which;
      }
      stats[0] += it; stats[1] = std::max<int64_t>(stats[1], it);
      if (!settled) ++stats[2];
    }
    const int first = (int)parent.size();
    for (const Desc& d : c) { parent.push_back(node); centre.push_back(d); nchild.push_back(0); }
    nchild[node] = (int)c.size();
    if (level >= L) return;
    for (size_t q = 0; q < c.size(); ++q) {
      std::vector<int> sub;
      for (int i = 0; i < n; ++i) if (which[i] == (int)q) sub.push_back(idx[i]);
      if (sub.size() > 1) step(first + (int)q, sub, level + 1, mix(key + 1 + (uint64_t)q));
    }
  }
};

}  // namespace

// Returns the number of nodes (the root included), or -1 for a refused input (D4). Outputs as covgpu_voc_train_t; nothing but the
// return value is written if the tree has more than node_capacity nodes. stats [6].
extern "C" int voctrain_serial(int num_sets, const int32_t* row_ptr, const uint8_t* desc, int k, int L, int weighting, uint64_t seed,
                               int max_iterations, int node_capacity, int32_t* num_words, int32_t* parent, uint8_t* desc_out,
                               int32_t* word_id, double* weight, int32_t* row_word, int64_t* stats) {
  if (num_sets < 1 || row_ptr[num_sets] < 1 || k < 2 || L < 1 || max_iterations < 1 || weighting < 0 || weighting > 3) return -1;
  int64_t full = 1;
  for (int l = 0; l < L; ++l) { full *= k; if (full > (1 << 20) - 1) return -1; }
  const int R = row_ptr[num_sets];
  std::vector<Desc> rows(R);
  std::memcpy(rows.data(), desc, 32 * (size_t)R);
  Trainer T;
  T.k = k; T.L = L; T.max_iterations = max_iterations; T.rows = rows.data();
  T.parent.push_back(-1); T.centre.push_back(Desc{{0, 0, 0, 0}}); T.nchild.push_back(0);
  std::vector<int> all(R);
  for (int r = 0; r < R; ++r) all[r] = r;
  T.step(0, all, 1, seed);
  const int N = (int)T.parent.size();
  if (N > node_capacity) return N;
  // words: the leaves in node order, the root left out
  std::vector<int> word(N, -1);
  int W = 0;
  for (int i = 1; i < N; ++i) if (T.nchild[i] == 0) word[i] = W++;
  // children are consecutive: the first child of node i follows from the creation order, found here through the parents
  std::vector<int> first(N, -1);
  for (int i = N - 1; i >= 1; --i) first[T.parent[i]] = i;
  // the transform leaf of every row: descend from the root, the first nearest child wins
  std::vector<int> leaf_word(R);
  for (int r = 0; r < R; ++r) {
    int at = 0;
    while (T.nchild[at] > 0) {
      int best = first[at], bd = dist(rows[r], T.centre[best]);
      for (int q = 1; q < T.nchild[at]; ++q) { const int d = dist(rows[r], T.centre[first[at] + q]); if (d < bd) { bd = d; best = first[at] + q; } }
      at = best;
    }
    leaf_word[r] = word[at];
  }
  std::vector<double> wt(N, 0.0);
  if (weighting == 1 || weighting == 3) {
    for (int i = 1; i < N; ++i) if (word[i] >= 0) wt[i] = 1.0;
  } else {
    std::vector<int> ni(W, 0), last(W, -1);
    for (int s = 0; s < num_sets; ++s)
      for (int r = row_ptr[s]; r < row_ptr[s + 1]; ++r)
        if (last[leaf_word[r]] != s) { last[leaf_word[r]] = s; ++ni[leaf_word[r]]; }
    for (int i = 1; i < N; ++i)
      if (word[i] >= 0 && ni[word[i]] > 0) wt[i] = std::log((double)num_sets / (double)ni[word[i]]);
  }
  *num_words = W;
  std::memcpy(parent, T.parent.data(), 4 * (size_t)N);
  std::memcpy(desc_out, T.centre.data(), 32 * (size_t)N);
  std::memcpy(word_id, word.data(), 4 * (size_t)N);
  std::memcpy(weight, wt.data(), 8 * (size_t)N);
  if (row_word) std::memcpy(row_word, leaf_word.data(), 4 * (size_t)R);
  if (stats) std::memcpy(stats, T.stats, sizeof T.stats);
  return N;
}
