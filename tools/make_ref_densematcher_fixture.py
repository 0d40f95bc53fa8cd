"""Makes tests/golden/densematcher_ref.npz — match lists COMPUTED BY THE REFERENCE'S OWN DenseMatcher.

Runs in the development container only (needs the reference tree, $COVINS_REF, default /root/reference). It compiles the reference's
src/dense_matcher/DenseMatcher.cpp, src/dense_matcher/ThreadPool.cpp and src/matcher/MatchingAlgorithm.cpp, where they lie, together
with a flat adapter of our own (below: a covins::MatchingAlgorithm over arrays whose distance() is the Hamming distance by
__builtin_popcount with LandmarkMatchingAlgorithm::distance's threshold, and whose skip flags are doSetup's) into a temporary
directory outside the tree, with g++ -std=c++17 -pthread. Nothing compiled is kept.

Every case regenerates its inputs from a seed (tests/match_util.py) and runs DenseMatcher::match with numMatcherThreads = 1, the order
DESIGN.md §4.11 takes as the contract; the same run with 8 threads is recorded as information only (it can depend on timing). The
fixture stores the seeds, the parameters, a sha256 of each case's regenerated inputs and the match lists, no descriptors.
tests/test_match_host.py checks the numpy restatement against it, tests/test_gpu_match.py the GPU."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REF = os.environ.get("COVINS_REF", "/root/reference")

ADAPTER = r'''
#include <cfloat>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "covins/dense_matcher/DenseMatcher.hpp"
#include "matcher/MatchingAlgorithm.h"

// A MatchingAlgorithm over flat arrays: LandmarkMatchingAlgorithm's distance() and skip flags, no keyframes.
struct FlatAlgorithm : public covins::MatchingAlgorithm {
  std::vector<uint8_t> A, B, skA, skB;
  float thr = 50.0f;
  std::vector<size_t> ia, ib;
  std::vector<double> d;
  size_t sizeA() const override { return skA.size(); }
  size_t sizeB() const override { return skB.size(); }
  float distanceThreshold() const override { return thr; }
  bool skipA(size_t i) const override { return skA[i] != 0; }
  bool skipB(size_t i) const override { return skB[i] != 0; }
  // the Hamming distance of two 32-byte rows (bits set in the XOR of the eight 32-bit words), d if d < thr, else FLT_MAX
  float distance(size_t a, size_t b) const override {
    uint32_t wa[8], wb[8];
    std::memcpy(wa, &A[32 * a], 32); std::memcpy(wb, &B[32 * b], 32);
    int d = 0;
    for (int w = 0; w < 8; ++w) d += __builtin_popcount(wa[w] ^ wb[w]);
    return static_cast<float>(d) < thr ? static_cast<float>(d) : FLT_MAX;
  }
  void reserveMatches(size_t) override {}
  void setBestMatch(size_t a, size_t b, double dist) override { ia.push_back(a); ib.push_back(b); d.push_back(dist); }
};

// stdin: threads nA nB thr, then A [nA*32] B [nB*32] skipA [nA] skipB [nB] as bytes; stdout: "a b d" per match
int main() {
  int threads, nA, nB; float thr;
  if (std::fread(&threads, 4, 1, stdin) != 1 || std::fread(&nA, 4, 1, stdin) != 1 || std::fread(&nB, 4, 1, stdin) != 1 ||
      std::fread(&thr, 4, 1, stdin) != 1) return 2;
  std::shared_ptr<FlatAlgorithm> alg(new FlatAlgorithm);
  alg->thr = thr;
  alg->A.resize(32 * (size_t)nA); alg->B.resize(32 * (size_t)nB); alg->skA.resize(nA); alg->skB.resize(nB);
  if (std::fread(alg->A.data(), 1, alg->A.size(), stdin) != alg->A.size() || std::fread(alg->B.data(), 1, alg->B.size(), stdin) != alg->B.size() ||
      std::fread(alg->skA.data(), 1, nA, stdin) != (size_t)nA || std::fread(alg->skB.data(), 1, nB, stdin) != (size_t)nB) return 3;
  std::unique_ptr<estd2::DenseMatcher> matcher(new estd2::DenseMatcher((unsigned char)threads));
  matcher->match<FlatAlgorithm>(*alg);
  for (size_t i = 0; i < alg->ia.size(); ++i) std::printf("%zu %zu %.17g\n", alg->ia[i], alg->ib[i], alg->d[i]);
  return 0;
}
'''

THR = 50.0
# (kind, seed, job): "map" = tests.match_util.map_batch(the `small` synthetic map, 4, seed), "adv" = adversarial_batch(seed)
CASES = [("map", 11, 0), ("map", 12, 1), ("map", 13, 2), ("map", 14, 3), ("adv", 0, 0), ("adv", 0, 1), ("adv", 0, 3), ("adv", 0, 6),
         ("adv", 0, -1)]


def case_inputs(kind, seed, job, small=None):
    """(A, B, skipA, skipB, digest) of one fixture case, regenerated from its seed."""
    import hashlib
    from tests import match_util as mu
    if kind == "map":
        from covins_amd import synth
        small = small if small is not None else synth.make_map(synth.config_named("small"))
        bt = mu.map_batch(small, 4, seed=seed)
    else:
        bt = mu.adversarial_batch(seed)
    job = job % len(bt["set_a"])
    A, sA = mu.rows(bt, int(bt["set_a"][job])); B, sB = mu.rows(bt, int(bt["set_b"][job]))
    h = hashlib.sha256()
    for x in (A, B, sA.astype(np.uint8), sB.astype(np.uint8)):
        h.update(np.ascontiguousarray(x).tobytes())
    return A, B, sA, sB, h.hexdigest()


def run(exe, threads, A, B, sA, sB):
    inp = np.array([threads, len(A), len(B)], np.int32).tobytes() + np.float32(THR).tobytes() + A.tobytes() + B.tobytes() + \
        sA.astype(np.uint8).tobytes() + sB.astype(np.uint8).tobytes()
    out = subprocess.run([exe], input=inp, stdout=subprocess.PIPE, check=True).stdout.decode().split()
    return np.array(out, np.float64).reshape(-1, 3)


if __name__ == "__main__":
    from covins_amd import synth
    tmp = tempfile.mkdtemp()
    src = os.path.join(tmp, "adapter.cpp")
    open(src, "w").write(ADAPTER)
    exe = os.path.join(tmp, "densematcher_ref")
    be = os.path.join(REF, "covins_backend")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-w", "-I" + os.path.join(be, "include"), "-I" + os.path.join(be, "include", "covins"),
                           src, os.path.join(be, "src", "dense_matcher", "DenseMatcher.cpp"), os.path.join(be, "src", "dense_matcher", "ThreadPool.cpp"),
                           os.path.join(be, "src", "matcher", "MatchingAlgorithm.cpp"), "-o", exe])
    small = synth.make_map(synth.config_named("small"))
    ptr, m1, digests, same8 = [0], [], [], []
    for kind, seed, job in CASES:
        A, B, sA, sB, dg = case_inputs(kind, seed, job, small)
        r1 = run(exe, 1, A, B, sA, sB)
        r8 = run(exe, 8, A, B, sA, sB)
        m1.append(r1); ptr.append(ptr[-1] + len(r1)); digests.append(dg)
        same8.append(r1.shape == r8.shape and bool(np.all(r1 == r8)))
        print(f"{kind} seed {seed} job {job}: {len(A)} x {len(B)} rows, {len(r1)} matches; 8 threads give the same list: {same8[-1]}")
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "densematcher_ref.npz"),
                        kind=np.array([c[0] for c in CASES]), seed=np.array([c[1] for c in CASES], np.int64),
                        job=np.array([c[2] for c in CASES], np.int64), thr=np.float32(THR), num_best=np.int32(4),
                        digest=np.array(digests), ptr=np.array(ptr, np.int64),
                        matches=np.concatenate(m1) if m1 else np.zeros((0, 3)), same_with_8_threads=np.array(same8))
