// facade_voctrain_shim.cpp — the C++ facade's CreateVocabulary (include/covins_gpu/optimization_gpu.hpp) on the
// stand-in types: descriptor sets as std::vector<std::vector<std::array<uint8_t, 32>>>, the result copied out in flat form. The
// stand-in map and its entry points are facade_shim.cpp's, compiled into this library as they are.
#include <array>
#include <cstring>
#include <vector>

#include "facade_shim.cpp"

extern "C" {

// Returns the number of nodes, or -needed if `capacity` entries are too few (nothing is written then). child_ptr [capacity + 1].
int voctrain_create(int num_sets, const int* row_ptr, const unsigned char* desc, int k, int L, int weighting, int scoring,
                    unsigned long long seed, int max_iterations, int capacity, int* num_words, int* parent, int* child_ptr, int* child,
                    unsigned char* desc_out, int* word_id, double* weight, long long* stats) {
  std::vector<std::vector<std::array<uint8_t, 32>>> sets((size_t)num_sets);
  for (int s = 0; s < num_sets; ++s) {
    sets[s].resize((size_t)(row_ptr[s + 1] - row_ptr[s]));
    if (!sets[s].empty()) std::memcpy(sets[s].data(), desc + 32 * (size_t)row_ptr[s], 32 * sets[s].size());
  }
  int64_t st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const covins_gpu::BowVocabulary v = covins_gpu::CreateVocabulary<standin::Types>(sets, k, L, weighting, scoring, seed, st, max_iterations);
  const int N = (int)v.parent.size();
  if (N > capacity) return -N;
  *num_words = v.num_words;
  std::memcpy(parent, v.parent.data(), 4 * (size_t)N); std::memcpy(child_ptr, v.child_ptr.data(), 4 * ((size_t)N + 1));
  std::memcpy(child, v.child.data(), 4 * ((size_t)N - 1)); std::memcpy(desc_out, v.desc.data(), 32 * (size_t)N);
  std::memcpy(word_id, v.word_id.data(), 4 * (size_t)N); std::memcpy(weight, v.weight.data(), 8 * (size_t)N);
  for (int i = 0; i < 8; ++i) stats[i] = st[i];
  return N;
}

}  // extern "C"
