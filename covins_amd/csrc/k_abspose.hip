// k_abspose.hip — batched loop-candidate geometric verification: Se3Solver::projectiveAlignment (Se3Solver.cpp:59-110), an opengv
// RANSAC over 2D-3D matches with a minimal P3P, scored by FrameAbsolutePoseSacProblem::getSelectedDistancesToModel.
//
// The reference runs one RANSAC per loop candidate, serially, on the place-recognition thread (placerec_be.cpp:116-139). Here one
// workgroup of 256 threads verifies one candidate: its bearings, world points and sigma_angle are staged into LDS as SoA, then per
// chunk of 256 draws (a) every thread draws 4 correspondences and solves one P3P, (b) the four waves score the chunk's hypotheses,
// lanes over the correspondences, counting with a ballot, (c) thread 0 replays opengv's sequential loop (k update, failed draws,
// the max_iterations stop) over the chunk in draw order, and the workgroup decides uniformly whether another chunk is needed. The
// result is the sequential loop's, not an approximation of it. FP64 throughout.
#include "common.hpp"
#include "dev_math.hpp"

#include <cfloat>
#include <climits>

namespace covgpu {
using namespace covdev;

namespace {

constexpr int kAbsThreads = 256;      // draws per chunk = threads per workgroup
constexpr int kAbsStageCap = 2048;    // correspondences staged into LDS (56 B each); larger candidates read global memory

struct AbsBatch {
  int num;
  const int* ptr;
  const double *f, *P, *sig;          // [C][3], [C][3], [C]
  const unsigned long long* seed;     // [num]
  double* T;                          // [num][7]
  unsigned char* inlier;              // [C]
  int *inliers, *iterations, *best_draw;
  int min_inliers, max_iterations;
  double probability, threshold;
};

COV_DEV unsigned long long splitmix64(unsigned long long x) {
  unsigned long long z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// the 4 distinct indices of draw d: partial Fisher-Yates over [0, n), slot k swaps position k with k + splitmix64(seed + 4d + k) mod (n - k).
// Positions below k are never read again, so only the (at most 4) displaced values above the current slot are remembered.
COV_DEV void draw4(unsigned long long seed, unsigned long long d, int n, int idx[4]) {
  int opos[4], oval[4], no = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const unsigned long long x = splitmix64(seed + 4ull * d + (unsigned long long)k);
    const int j = k + (int)(x % (unsigned long long)(n - k));
    int vk = k, vj = j;
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      if (o < no && opos[o] == k) vk = oval[o];
      if (o < no && opos[o] == j) vj = oval[o];
    }
    bool put = false;                                   // a(j) = old a(k)
#pragma unroll
    for (int o = 0; o < 4; ++o) if (o < no && opos[o] == j) { oval[o] = vk; put = true; }
    if (!put) { opos[no] = j; oval[no] = vk; ++no; }
    idx[k] = vj;
  }
}

COV_DEV V3 nrm(V3 a) { return a * (1.0 / sqrt(dot(a, a))); }

// largest real root of m^3 + B m^2 + C m + D (Cardano / trigonometric form, then two Newton steps)
COV_DEV double cubic_max_root(double B, double C, double D) {
  const double P = C - B * B / 3.0, Q = 2.0 * B * B * B / 27.0 - B * C / 3.0 + D;
  const double disc = 0.25 * Q * Q + P * P * P / 27.0;
  double z;
  if (disc > 0.0) {
    const double sd = sqrt(disc);
    z = cbrt(-0.5 * Q + sd) + cbrt(-0.5 * Q - sd);
  } else {
    const double r = sqrt(fmax(-P / 3.0, 0.0));
    const double c = r > 0.0 ? fmin(fmax(-0.5 * Q / (r * r * r), -1.0), 1.0) : 0.0;
    z = 2.0 * r * cos(acos(c) / 3.0);
  }
  double m = z - B / 3.0;
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const double g = ((m + B) * m + C) * m + D, dg = (3.0 * m + 2.0 * B) * m + C;
    if (dg != 0.0) m -= g / dg;
  }
  return m;
}

// real roots of A[0] v^4 + ... + A[4] (Ferrari: depressed quartic, resolvent cubic, two quadratics), two Newton steps each, ascending;
// a root counts as real when its imaginary part is at most 1e-9 max(1, |re|) (the rule of tests/abspose_ref.py). Returns the count.
COV_DEV int quartic_real_roots(const double A[5], double v[4]) {
  const double ia = 1.0 / A[0];
  const double a = A[1] * ia, b = A[2] * ia, c = A[3] * ia, d = A[4] * ia;
  const double a2 = a * a;
  const double p = b - 0.375 * a2, q = c - 0.5 * a * b + 0.125 * a2 * a, r = d - 0.25 * a * c + a2 * b / 16.0 - 3.0 * a2 * a2 / 256.0;
  double re[4], im[4];
  const double m = cubic_max_root(p, 0.25 * p * p - r, -0.125 * q * q);
  if (m > 0.0) {
    const double s = sqrt(2.0 * m), h = q / (2.0 * s);
    const double D1 = s * s - 4.0 * (m + 0.5 * p + h), D2 = s * s - 4.0 * (m + 0.5 * p - h);
    const double r1 = 0.5 * sqrt(fabs(D1)), r2 = 0.5 * sqrt(fabs(D2));
    re[0] = 0.5 * s + (D1 >= 0.0 ? r1 : 0.0); re[1] = 0.5 * s - (D1 >= 0.0 ? r1 : 0.0); im[0] = im[1] = D1 >= 0.0 ? 0.0 : r1;
    re[2] = -0.5 * s + (D2 >= 0.0 ? r2 : 0.0); re[3] = -0.5 * s - (D2 >= 0.0 ? r2 : 0.0); im[2] = im[3] = D2 >= 0.0 ? 0.0 : r2;
  } else {                                             // q == 0: biquadratic y^4 + p y^2 + r
    const double e = p * p - 4.0 * r;
    double w[2], wi[2];
    if (e >= 0.0) { const double se = sqrt(e); w[0] = 0.5 * (-p + se); w[1] = 0.5 * (-p - se); wi[0] = wi[1] = 0.0; }
    else { w[0] = w[1] = -0.5 * p; wi[0] = 0.5 * sqrt(-e); wi[1] = -wi[0]; }
#pragma unroll
    for (int k = 0; k < 2; ++k) {                      // y = +-sqrt(w + i wi)
      const double mod = sqrt(w[k] * w[k] + wi[k] * wi[k]);
      const double x = sqrt(fmax(0.5 * (mod + w[k]), 0.0)), y = copysign(sqrt(fmax(0.5 * (mod - w[k]), 0.0)), wi[k]);
      re[2 * k] = x; im[2 * k] = y; re[2 * k + 1] = -x; im[2 * k + 1] = -y;
    }
  }
  int n = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    double x = re[k] - 0.25 * a;
    const bool real = fabs(im[k]) <= 1e-9 * fmax(1.0, fabs(x));
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const double fv = (((A[0] * x + A[1]) * x + A[2]) * x + A[3]) * x + A[4];
      const double dv = ((4.0 * A[0] * x + 3.0 * A[1]) * x + 2.0 * A[2]) * x + A[3];
      if (dv != 0.0) x -= fv / dv;
    }
    v[k] = real ? x : INFINITY;
    n += real ? 1 : 0;
  }
  // sorting network (invalid roots are +inf and sink to the end)
  auto cs = [&](int i, int j) { const double lo = fmin(v[i], v[j]), hi = fmax(v[i], v[j]); v[i] = lo; v[j] = hi; };
  cs(0, 1); cs(2, 3); cs(0, 2); cs(1, 3); cs(1, 2);
  return n;
}

// every real P3P solution with positive depths on correspondences 0..2 (Grunert's quartic in v = s3/s1, u = s2/s1 from its linear
// relation, two Newton steps on the three law-of-cosines equations, the pose from two orthonormal triads); emit(R, t) per solution
// in ascending v. Returns the number of solutions.
template <class Emit>
COV_DEV int p3p_solve(const V3 f[3], const V3 P[3], Emit&& emit) {
  const double ca = dot(f[1], f[2]), cb = dot(f[0], f[2]), cg = dot(f[0], f[1]);
  const V3 d12 = P[1] - P[2], d02 = P[0] - P[2], d01 = P[0] - P[1];
  const double a2 = dot(d12, d12), b2 = dot(d02, d02), c2 = dot(d01, d01);
  const double amc = (a2 - c2) / b2, apc = (a2 + c2) / b2;
  double A[5];
  A[0] = (amc - 1) * (amc - 1) - 4 * c2 / b2 * ca * ca;
  A[1] = 4 * (amc * (1 - amc) * cb - (1 - apc) * ca * cg + 2 * c2 / b2 * ca * ca * cb);
  A[2] = 2 * (amc * amc - 1 + 2 * amc * amc * cb * cb + 2 * (b2 - c2) / b2 * ca * ca - 4 * apc * ca * cb * cg + 2 * (b2 - a2) / b2 * cg * cg);
  A[3] = 4 * (-amc * (1 + amc) * cb + 2 * a2 / b2 * cg * cg * cb - (1 - apc) * ca * cg);
  A[4] = (1 + amc) * (1 + amc) - 4 * a2 / b2 * cg * cg;
  bool fin = A[0] != 0.0;
#pragma unroll
  for (int k = 0; k < 5; ++k) fin = fin && isfinite(A[k]);
  if (!fin) return 0;
  double vs[4];
  const int nr = quartic_real_roots(A, vs);
  int ns = 0;
  for (int k = 0; k < 4; ++k) {
    if (k >= nr) break;
    const double v = vs[k];
    const double den = 2 * (cg - v * ca);
    const double u = den != 0.0 ? ((-1 + amc) * v * v - 2 * amc * cb * v + 1 + amc) / den : NAN;
    const double qq = 1 + v * v - 2 * v * cb;
    if (!(v > 0 && u > 0 && qq > 0 && isfinite(u))) continue;
    const double s1 = sqrt(b2 / qq);
    double s[3] = {s1, u * s1, v * s1};
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const double F0 = s[1] * s[1] + s[2] * s[2] - 2 * s[1] * s[2] * ca - a2;
      const double F1 = s[0] * s[0] + s[2] * s[2] - 2 * s[0] * s[2] * cb - b2;
      const double F2 = s[0] * s[0] + s[1] * s[1] - 2 * s[0] * s[1] * cg - c2;
      const double j01 = 2 * (s[1] - s[2] * ca), j02 = 2 * (s[2] - s[1] * ca);
      const double j10 = 2 * (s[0] - s[2] * cb), j12 = 2 * (s[2] - s[0] * cb);
      const double j20 = 2 * (s[0] - s[1] * cg), j21 = 2 * (s[1] - s[0] * cg);
      // J = [[0 j01 j02] [j10 0 j12] [j20 j21 0]], Cramer
      const double det = -j01 * (-j12 * j20) + j02 * (j10 * j21);
      if (!(det != 0.0 && isfinite(det))) break;
      const double id = 1.0 / det;
      const double x0 = (j01 * j12 * F2 + j02 * j21 * F1 - j12 * j21 * F0) * id;
      const double x1 = (j12 * j20 * F0 + j02 * j10 * F2 - j02 * j20 * F1) * id;
      const double x2 = (j10 * j21 * F0 + j01 * j20 * F1 - j01 * j10 * F2) * id;
      s[0] -= x0; s[1] -= x1; s[2] -= x2;
    }
    if (!(s[0] > 0 && s[1] > 0 && s[2] > 0 && isfinite(s[0] + s[1] + s[2]))) continue;
    const V3 X0 = f[0] * s[0], X1 = f[1] * s[1], X2 = f[2] * s[2];
    const V3 e1 = nrm(X1 - X0), g1 = nrm(P[1] - P[0]);
    const V3 wx = X2 - X0, wp = P[2] - P[0];
    const V3 e2 = nrm(wx - e1 * dot(wx, e1)), g2 = nrm(wp - g1 * dot(wp, g1));
    const V3 e3 = cross(e1, e2), g3 = cross(g1, g2);
    M3 R;                                               // R = g1 e1^T + g2 e2^T + g3 e3^T: camera -> world
    const double G[9] = {g1.x, g2.x, g3.x, g1.y, g2.y, g3.y, g1.z, g2.z, g3.z}, E[9] = {e1.x, e2.x, e3.x, e1.y, e2.y, e3.y, e1.z, e2.z, e3.z};
#pragma unroll
    for (int rr = 0; rr < 3; ++rr)
#pragma unroll
      for (int cc = 0; cc < 3; ++cc) R.m[3 * rr + cc] = G[3 * rr] * E[3 * cc] + G[3 * rr + 1] * E[3 * cc + 1] + G[3 * rr + 2] * E[3 * cc + 2];
    const V3 cx = (X0 + X1 + X2) * (1.0 / 3.0), cp = (P[0] + P[1] + P[2]) * (1.0 / 3.0);
    const V3 t = cp - mul(R, cx);
    bool ok = isfinite(t.x + t.y + t.z);
#pragma unroll
    for (int k2 = 0; k2 < 9; ++k2) ok = ok && isfinite(R.m[k2]);
    if (!ok) continue;
    emit(ns, R, t);
    ++ns;
  }
  return ns;
}

// opengv's choice among the solutions: the smallest 1 - <normalize(R^T P4 - R^T t), f4>; the first wins a tie
COV_DEV double pick_score(const M3& R, V3 t, V3 f4, V3 P4) {
  const V3 b = mulT(R, P4) - mulT(R, t);
  return 1.0 - dot(nrm(b), f4);
}

// getSelectedDistancesToModel: inverse transform [R^T | -R^T t] applied to [P; 1], normalised, squared distance to f over sigma_angle
COV_DEV double abs_score(const double* Ri, const double* ti, V3 f, V3 P, double sig) {
  const V3 body = v3(Ri[0] * P.x + Ri[1] * P.y + Ri[2] * P.z + ti[0], Ri[3] * P.x + Ri[4] * P.y + Ri[5] * P.z + ti[1],
                     Ri[6] * P.x + Ri[7] * P.y + Ri[8] * P.z + ti[2]);
  const V3 e = nrm(body) - f;
  return dot(e, e) / sig;
}

COV_DEV void rot_to_quat(const double* R, double* q) {  // Hamilton x y z w, w >= 0
  const double tr = R[0] + R[4] + R[8];
  double x, y, z, w;
  if (tr > 0) { const double s = 0.5 / sqrt(tr + 1.0); w = 0.25 / s; x = (R[7] - R[5]) * s; y = (R[2] - R[6]) * s; z = (R[3] - R[1]) * s; }
  else if (R[0] > R[4] && R[0] > R[8]) { const double s = 2.0 * sqrt(1.0 + R[0] - R[4] - R[8]); w = (R[7] - R[5]) / s; x = 0.25 * s; y = (R[1] + R[3]) / s; z = (R[2] + R[6]) / s; }
  else if (R[4] > R[8]) { const double s = 2.0 * sqrt(1.0 + R[4] - R[0] - R[8]); w = (R[2] - R[6]) / s; x = (R[1] + R[3]) / s; y = 0.25 * s; z = (R[5] + R[7]) / s; }
  else { const double s = 2.0 * sqrt(1.0 + R[8] - R[0] - R[4]); w = (R[3] - R[1]) / s; x = (R[2] + R[6]) / s; y = (R[5] + R[7]) / s; z = 0.25 * s; }
  const double sg = w < 0 ? -1.0 : 1.0, in = sg / sqrt(x * x + y * y + z * z + w * w);
  q[0] = x * in; q[1] = y * in; q[2] = z * in; q[3] = w * in;
}

// correspondence i of a candidate: from the LDS stage (SoA, stride 1) or from global memory ([C][3], stride 3)
struct Src {
  const double *fx, *fy, *fz, *px, *py, *pz, *sg;
  int s3;
  COV_DEV V3 f(int i) const { return v3(fx[s3 * i], fy[s3 * i], fz[s3 * i]); }
  COV_DEV V3 p(int i) const { return v3(px[s3 * i], py[s3 * i], pz[s3 * i]); }
};

__global__ __launch_bounds__(kAbsThreads) void k_abspose(AbsBatch B, int cap) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  double* sH = sm;                                  // [256][12] hypotheses: R (row-major) | t
  double* sBest = sH + 12 * kAbsThreads;            // [12]
  double* sStage = sBest + 12;                      // [7][cap]
  __shared__ int sCnt[kAbsThreads];                 // inlier count per hypothesis of the chunk, -1: failed draw
  __shared__ int sIt, sSkip, sBestN, sBestD, sDone, sFinal;
  __shared__ double sK;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int o0 = B.ptr[b], n = B.ptr[b + 1] - o0;
  if (n < 4) {                                      // opengv: no sample can be drawn, no model
    for (int i = tid; i < n; i += kAbsThreads) B.inlier[o0 + i] = 0;
    if (tid == 0) {
      B.inliers[b] = 0;
      if (B.iterations) B.iterations[b] = 0;
      if (B.best_draw) B.best_draw[b] = -1;
    }
    return;
  }
  Src S;
  if (n <= cap) {
    for (int i = tid; i < n; i += kAbsThreads) {
      const size_t g = (size_t)(o0 + i);
      sStage[i] = B.f[3 * g]; sStage[cap + i] = B.f[3 * g + 1]; sStage[2 * cap + i] = B.f[3 * g + 2];
      sStage[3 * cap + i] = B.P[3 * g]; sStage[4 * cap + i] = B.P[3 * g + 1]; sStage[5 * cap + i] = B.P[3 * g + 2];
      sStage[6 * cap + i] = B.sig[g];
    }
    S = Src{sStage, sStage + cap, sStage + 2 * cap, sStage + 3 * cap, sStage + 4 * cap, sStage + 5 * cap, sStage + 6 * cap, 1};
  } else {
    const double *f = B.f + 3 * (size_t)o0, *P = B.P + 3 * (size_t)o0;
    S = Src{f, f + 1, f + 2, P, P + 1, P + 2, B.sig + o0, 3};
  }
  if (tid == 0) { sIt = 0; sSkip = 0; sBestN = INT_MIN; sBestD = -1; sDone = 0; sK = 1.0; }
  __syncthreads();
  const unsigned long long seed = B.seed[b];
  const double th = B.threshold;
  const int maxit = B.max_iterations, max_skip = 10 * maxit;
  for (int base = 0; ; base += kAbsThreads) {
    // (a) one draw and one P3P per thread
    {
      int idx[4];
      draw4(seed, (unsigned long long)(base + tid), n, idx);
      V3 f[3], P[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) { f[k] = S.f(idx[k]); P[k] = S.p(idx[k]); }
      const V3 f4 = S.f(idx[3]), P4 = S.p(idx[3]);
      double best = 1e6;
      int bi = -1;
      double* h = sH + 12 * tid;
      p3p_solve(f, P, [&](int i, const M3& R, V3 t) {
        const double sc = pick_score(R, t, f4, P4);
        if (sc < best) {
          best = sc; bi = i;
#pragma unroll
          for (int k = 0; k < 9; ++k) h[k] = R.m[k];
          h[9] = t.x; h[10] = t.y; h[11] = t.z;
        }
      });
      sCnt[tid] = bi >= 0 ? 0 : -1;
    }
    __syncthreads();
    // (b) inlier counts: wave w scores hypotheses w, w + 4, ...; lanes over the correspondences
    for (int hh = wave; hh < kAbsThreads; hh += kAbsThreads / 64) {
      if (sCnt[hh] < 0) continue;                   // wave-uniform (LDS broadcast)
      const double* h = sH + 12 * hh;
      double Ri[9], ti[3];
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) Ri[3 * r + c] = h[3 * c + r];
#pragma unroll
      for (int r = 0; r < 3; ++r) ti[r] = -(Ri[3 * r] * h[9] + Ri[3 * r + 1] * h[10] + Ri[3 * r + 2] * h[11]);
      int cnt = 0;
      for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        const bool in = i < n && abs_score(Ri, ti, S.f(i < n ? i : 0), S.p(i < n ? i : 0), S.sg[i < n ? i : 0]) < th;
        cnt += __popcll(__ballot(in));
      }
      if (lane == 0) sCnt[hh] = cnt;
    }
    __syncthreads();
    // (c) opengv's loop over the chunk, in draw order
    if (tid == 0) {
      int it = sIt, skipped = sSkip, bestn = sBestN, done = 0;
      double k = sK;
      for (int j = 0; j < kAbsThreads; ++j) {
        if (!(it < k && skipped < max_skip)) { done = 1; break; }
        const int c = sCnt[j];
        if (c < 0) { ++skipped; continue; }
        if (c > bestn) {
          bestn = c; sBestD = base + j;
          for (int q = 0; q < 12; ++q) sBest[q] = sH[12 * j + q];
          const double w = (double)bestn / (double)n;
          double pno = 1.0 - pow(w, 4.0);
          pno = fmax(DBL_EPSILON, pno);
          pno = fmin(1.0 - DBL_EPSILON, pno);
          k = log(1.0 - B.probability) / log(pno);
        }
        ++it;
        if (it > maxit) { done = 1; break; }
      }
      sIt = it; sSkip = skipped; sBestN = bestn; sK = k; sDone = done;
    }
    __syncthreads();
    if (sDone) break;
  }
  // final inliers of the best model; the candidate fails below min_inliers
  if (tid == 0) sFinal = 0;
  __syncthreads();
  const bool have = sBestD >= 0;
  double Ri[9], ti[3];
  if (have) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) Ri[3 * r + c] = sBest[3 * c + r];
#pragma unroll
    for (int r = 0; r < 3; ++r) ti[r] = -(Ri[3 * r] * sBest[9] + Ri[3 * r + 1] * sBest[10] + Ri[3 * r + 2] * sBest[11]);
    int cnt = 0;
    for (int i = tid; i < n; i += kAbsThreads) cnt += abs_score(Ri, ti, S.f(i), S.p(i), S.sg[i]) < th ? 1 : 0;
    atomicAdd(&sFinal, cnt);
  }
  __syncthreads();
  const int nin = sFinal;
  const bool ok = have && nin > 0 && nin >= B.min_inliers;
  for (int i = tid; i < n; i += kAbsThreads) B.inlier[o0 + i] = ok && abs_score(Ri, ti, S.f(i), S.p(i), S.sg[i]) < th ? 1 : 0;
  if (tid == 0) {
    B.inliers[b] = ok ? nin : 0;
    if (B.iterations) B.iterations[b] = sIt;
    if (B.best_draw) B.best_draw[b] = sBestD;
    if (ok) {
      double* T = B.T + 7 * (size_t)b;
      rot_to_quat(sBest, T);
      T[4] = sBest[9]; T[5] = sBest[10]; T[6] = sBest[11];
    }
  }
}

// test entry point: P3P on correspondences 0..2 of every quadruple, all solutions (ascending v), and the one the 4th picks
__global__ __launch_bounds__(64) void k_p3p(int num, const double* F, const double* Pw, double* T, int* nsol, int* chosen) {
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (e >= num) return;
  V3 f[3], P[3];
  for (int k = 0; k < 3; ++k) { f[k] = ld3(F + 12 * (size_t)e + 3 * k); P[k] = ld3(Pw + 12 * (size_t)e + 3 * k); }
  const V3 f4 = ld3(F + 12 * (size_t)e + 9), P4 = ld3(Pw + 12 * (size_t)e + 9);
  double best = 1e6;
  int bi = -1;
  const int ns = p3p_solve(f, P, [&](int i, const M3& R, V3 t) {
    double* o = T + 28 * (size_t)e + 7 * i;
    rot_to_quat(R.m, o);
    o[4] = t.x; o[5] = t.y; o[6] = t.z;
    const double sc = pick_score(R, t, f4, P4);
    if (sc < best) { best = sc; bi = i; }
  });
  nsol[e] = ns;
  chosen[e] = bi;
}

}  // namespace

static size_t abspose_lds_bytes(int max_n) {
  const int cap = max_n < kAbsStageCap ? max_n : kAbsStageCap;
  return sizeof(double) * (12 * (size_t)kAbsThreads + 12 + 7 * (size_t)(cap > 0 ? cap : 0));
}

void launch_abspose(int num, const int* ptr, const double* f, const double* P, const double* sig, const unsigned long long* seed, double* T,
                    unsigned char* inlier, int* inliers, int* iterations, int* best_draw, int min_inliers, int max_iterations, double probability,
                    double threshold, int max_n, hipStream_t st) {
  if (num <= 0) return;
  const int cap = max_n < kAbsStageCap ? max_n : kAbsStageCap;
  const size_t lds = abspose_lds_bytes(max_n);
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_abspose), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  AbsBatch B{num, ptr, f, P, sig, seed, T, inlier, inliers, iterations, best_draw, min_inliers, max_iterations, probability, threshold};
  hipLaunchKernelGGL(k_abspose, dim3(num), dim3(kAbsThreads), lds, st, B, cap);
}

void launch_p3p(int num, const double* F, const double* P, double* T, int* nsol, int* chosen, hipStream_t st) {
  if (num <= 0) return;
  hipLaunchKernelGGL(k_p3p, dim3((num + 63) / 64), dim3(64), 0, st, num, F, P, T, nsol, chosen);
}

}  // namespace covgpu
