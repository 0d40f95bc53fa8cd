// k_fivept.hip — batched five-point relative-pose RANSAC of COVINS-G's loop verification: RelNonCentralPosSolver::computePose
// (RelNonCentralPosSolver.cpp:343-377), an opengv RANSAC over 2D-2D matches with the five-point minimal solver, scored by the
// reprojection of the triangulated point in both frames.
//
// One workgroup of 256 threads runs one job: its bearings are staged into LDS as SoA, then per pass of 16 draws (a) a group of 16
// lanes takes one draw and solves the five-point problem on its slots 0..4, (b) the four waves score the pass's hypotheses, lanes
// over the correspondences, counting with a ballot, (c) thread 0 replays opengv's sequential loop over the pass in draw order, and
// the workgroup decides uniformly whether another pass is needed. The result is the sequential loop's. FP64 throughout.
//
// The minimal solver of a group: an orthonormal basis of the null space of the 5x9 epipolar matrix (Gauss-Jordan with full
// pivoting, Gram-Schmidt; lane 0), E = xX + yY + zZ + W, the ten cubics det E = 0, 2EE^TE - tr(EE^T)E = 0 as a 10x20 system over
// the monomials in Nister's order (lanes 0..9 build and hold one row each in registers), Gauss-Jordan with partial pivoting
// (the pivot row is broadcast inside the group), Nister's 3x3 polynomial matrix in z and its determinant of degree 10, the real
// roots by bracketing (the roots of each derivative bracket those of the one below; lane i bisects bracket i), then lane i takes
// root i: x, y from the polynomial matrix, three Gauss-Newton steps on the ten cubics at E itself. Solutions that lie close in z merge in
// the polynomial, so the elimination runs three times, with z, x and y hidden, and the distinct E are collected; lane i then takes
// solution i: its four poses in closed form and their selection sums over the 8 correspondences of the draw. Every loop has a
// compile-time bound and every branch around a barrier is uniform, so degenerate input costs what any input costs and ends as a
// failed draw.
#include "common.hpp"
#include "dev_math.hpp"

#include <cfloat>
#include <climits>

namespace covgpu {
using namespace covdev;

namespace {

constexpr int kFpThreads = 256;       // threads per workgroup
constexpr int kFpLanes = 16;          // lanes per hypothesis
constexpr int kFpHyp = kFpThreads / kFpLanes;   // hypotheses per pass
constexpr int kFpSample = 8;          // correspondences per draw: 5 for the solver, 3 more pick the pose
constexpr int kFpStageCap = 1024;     // correspondences staged into LDS (48 B each); larger jobs read global memory
constexpr int kFpMaxIterations = 100000;
constexpr int kFpBisect = 64;         // halvings per bracket, in the ordered bit patterns of its ends: down to neighbouring doubles
constexpr int kFpPolish = 3;          // Gauss-Newton steps per root
constexpr double kFpRankTol = 1e-12;  // a pivot of the 5x9 elimination below this fraction of the largest entry: rank-deficient sample
constexpr int kFpRounds = 3;          // eliminations per draw: z, x, y hidden in turn
constexpr double kFpDedup = 1e-6;     // two E that agree to this in every entry (up to sign) are one solution
constexpr double kFpCubicGate = 1e-9; // an E (||E||_F = sqrt 2) whose cubics exceed this after the polish is not a solution

struct FpBatch {
  int num;
  const int* ptr;
  const double *f1, *f2;              // [C][3]
  const unsigned long long* seed;     // [num]
  double* T;                          // [num][7]
  unsigned char* inlier;              // [C]
  int *inliers, *status, *iterations, *best_draw;
  int min_inliers, max_iterations;
  double probability, threshold, sigma;
};

// LDS work area of one group of 16 lanes
struct FpWork {
  double F[kFpSample][6];             // the draw: f1 | f2 per slot
  double Q[5][9];                     // epipolar rows
  double N[4][9];                     // null-space basis X Y Z W (E row-major)
  double EEt[6][10];                  // E E^T, upper triangle, as quadratic polynomials
  double B[10][10];                   // right half of the reduced 10x20 system
  double C[3][13];                    // Nister's polynomial matrix: per row x's cubic, y's cubic, the quartic; ascending powers
  double Pp[3][11];                   // the three terms of its determinant
  double D[11][11];                   // D[m][j]: coefficient of z^j in p^(m) / m!
  double R[2][12];                    // roots of the previous / this derivative
  double Acc[10][9];                  // the solutions found so far
  double H[12];                       // the draw's model: R (row-major) | t
  int idx[kFpSample], opos[kFpSample], oval[kFpSample], cols[9];
  int ok;
};

COV_DEV unsigned long long fp_splitmix64(unsigned long long x) {
  unsigned long long z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// the 8 distinct indices of draw d into W.idx: partial Fisher-Yates over [0, n), slot k swaps position k with
// k + splitmix64(seed + 8d + k) mod (n - k). Positions below k are never read again, so only the displaced values are remembered.
COV_DEV void fp_draw(FpWork& W, unsigned long long seed, unsigned long long d, int n) {
  int no = 0;
  for (int k = 0; k < kFpSample; ++k) {
    const unsigned long long x = fp_splitmix64(seed + (unsigned long long)kFpSample * d + (unsigned long long)k);
    const int j = k + (int)(x % (unsigned long long)(n - k));
    int vk = k, vj = j;
    for (int o = 0; o < kFpSample; ++o) {
      if (o < no && W.opos[o] == k) vk = W.oval[o];
      if (o < no && W.opos[o] == j) vj = W.oval[o];
    }
    bool put = false;                                   // a(j) = old a(k)
    for (int o = 0; o < kFpSample; ++o) if (o < no && W.opos[o] == j) { W.oval[o] = vk; put = true; }
    if (!put) { W.opos[no] = j; W.oval[no] = vk; ++no; }
    W.idx[k] = vj;
  }
}

// triangulate2 and the two reprojections of a correspondence under T_12 = [R | t]
COV_DEV void fp_reproject(const double* R, V3 t, V3 f1, V3 f2, V3& r1, V3& r2) {
  const V3 g = v3(R[0] * f2.x + R[1] * f2.y + R[2] * f2.z, R[3] * f2.x + R[4] * f2.y + R[5] * f2.z, R[6] * f2.x + R[7] * f2.y + R[8] * f2.z);
  const double b0 = dot(t, f1), b1 = dot(t, g);
  const double a00 = dot(f1, f1), a01 = -dot(f1, g), a11 = -dot(g, g);   // A = [[a00, a01], [-a01, a11]]
  const double det = a00 * a11 + a01 * a01;
  const double l0 = (a11 * b0 - a01 * b1) / det, l1 = (a01 * b0 + a00 * b1) / det;
  const V3 p = (f1 * l0 + t + g * l1) * 0.5;
  const V3 q = v3(R[0] * p.x + R[3] * p.y + R[6] * p.z, R[1] * p.x + R[4] * p.y + R[7] * p.z, R[2] * p.x + R[5] * p.y + R[8] * p.z) -
               v3(R[0] * t.x + R[3] * t.y + R[6] * t.z, R[1] * t.x + R[4] * t.y + R[7] * t.z, R[2] * t.x + R[5] * t.y + R[8] * t.z);
  r1 = p * (1.0 / sqrt(dot(p, p)));
  r2 = q * (1.0 / sqrt(dot(q, q)));
}

COV_DEV double fp_score(const double* R, V3 t, V3 f1, V3 f2, double sigma) {
  V3 r1, r2;
  fp_reproject(R, t, f1, f2, r1, r2);
  const V3 e1 = r1 - f1, e2 = r2 - f2;
  return 0.5 * dot(e1, e1) / sigma + 0.5 * dot(e2, e2) / sigma;
}

COV_DEV void fp_rot_to_quat(const double* R, double* q) {  // Hamilton x y z w, w >= 0
  const double tr = R[0] + R[4] + R[8];
  double x, y, z, w;
  if (tr > 0) { const double s = 0.5 / sqrt(tr + 1.0); w = 0.25 / s; x = (R[7] - R[5]) * s; y = (R[2] - R[6]) * s; z = (R[3] - R[1]) * s; }
  else if (R[0] > R[4] && R[0] > R[8]) { const double s = 2.0 * sqrt(1.0 + R[0] - R[4] - R[8]); w = (R[7] - R[5]) / s; x = 0.25 * s; y = (R[1] + R[3]) / s; z = (R[2] + R[6]) / s; }
  else if (R[4] > R[8]) { const double s = 2.0 * sqrt(1.0 + R[4] - R[0] - R[8]); w = (R[2] - R[6]) / s; x = (R[1] + R[3]) / s; y = 0.25 * s; z = (R[5] + R[7]) / s; }
  else { const double s = 2.0 * sqrt(1.0 + R[8] - R[0] - R[4]); w = (R[3] - R[1]) / s; x = (R[2] + R[6]) / s; y = (R[5] + R[7]) / s; z = 0.25 * s; }
  const double sg = w < 0 ? -1.0 : 1.0, in = sg / sqrt(x * x + y * y + z * z + w * w);
  q[0] = x * in; q[1] = y * in; q[2] = z * in; q[3] = w * in;
}

// ---- polynomials in (x, y, z): linear over {x y z 1}, quadratic over {x2 xy xz x y2 yz y z2 z 1}, cubic over Nister's order
// x3 y3 x2y xy2 x2z x2 y2z y2 xyz xy | xz2 xz x yz2 yz y z3 z2 z 1. The loops are unrolled, so every index below is a constant.
COV_DEV void fp_lin(const FpWork& W, int e, double p[4]) {
#pragma unroll
  for (int a = 0; a < 4; ++a) p[a] = W.N[a][e];
}
COV_DEV void fp_mul11(double acc[10], const double a[4], const double b[4], double s) {
  constexpr int m2[4][4] = {{0, 1, 2, 3}, {1, 4, 5, 6}, {2, 5, 7, 8}, {3, 6, 8, 9}};
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[m2[i][j]] += s * a[i] * b[j];
}
COV_DEV void fp_mul21(double acc[20], const double p[10], const double e[4]) {
  constexpr int m3[10][4] = {{0, 2, 4, 5}, {2, 3, 8, 9}, {4, 8, 10, 11}, {5, 9, 11, 12}, {3, 1, 6, 7},
                             {8, 6, 13, 14}, {9, 7, 14, 15}, {10, 13, 16, 17}, {11, 14, 17, 18}, {12, 15, 18, 19}};
#pragma unroll
  for (int i = 0; i < 10; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[m3[i][j]] += p[i] * e[j];
}

// doubles to unsigned integers in the same order (the bit pattern, negative values reflected): halving a bracket in this key reaches
// neighbouring doubles in 64 steps whatever the magnitudes (a Cauchy bound of 1e17 is common), where the arithmetic mean would not
COV_DEV unsigned long long fp_key(double x) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(x);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
COV_DEV double fp_unkey(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k));
}

COV_DEV void fp_mm(const double* A, const double* B, double* C) {    // C = A B, 3x3 row-major
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}
COV_DEV void fp_mmt(const double* A, const double* B, double* C) {   // C = A B^T
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) C[3 * i + j] = A[3 * i] * B[3 * j] + A[3 * i + 1] * B[3 * j + 1] + A[3 * i + 2] * B[3 * j + 2];
}

// orthonormal basis of the null space of the draw's 5x9 epipolar matrix into W.N (one lane). False: rank-deficient or non-finite.
COV_DEV bool fp_nullspace(FpWork& W) {
  double scale = 0.0;
  bool fin = true;
  for (int r = 0; r < 5; ++r)
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        const double v = W.F[r][i] * W.F[r][3 + j];
        W.Q[r][3 * i + j] = v;
        fin = fin && isfinite(v);
        scale = fmax(scale, fabs(v));
      }
  if (!fin || !(scale > 0.0)) return false;
  for (int i = 0; i < 9; ++i) W.cols[i] = i;
  for (int c = 0; c < 5; ++c) {
    double best = -1.0;
    int br = c, bk = c;
    for (int r = c; r < 5; ++r)
      for (int k = c; k < 9; ++k) {
        const double v = fabs(W.Q[r][k]);
        if (v > best) { best = v; br = r; bk = k; }
      }
    if (!(best > kFpRankTol * scale)) return false;
    for (int k = 0; k < 9; ++k) { const double a = W.Q[c][k]; W.Q[c][k] = W.Q[br][k]; W.Q[br][k] = a; }
    for (int r = 0; r < 5; ++r) { const double a = W.Q[r][c]; W.Q[r][c] = W.Q[r][bk]; W.Q[r][bk] = a; }
    { const int a = W.cols[c]; W.cols[c] = W.cols[bk]; W.cols[bk] = a; }
    const double inv = 1.0 / W.Q[c][c];
    for (int k = 0; k < 9; ++k) W.Q[c][k] *= inv;
    for (int r = 0; r < 5; ++r) {
      if (r == c) continue;
      const double f = W.Q[r][c];
      for (int k = 0; k < 9; ++k) W.Q[r][k] -= f * W.Q[c][k];
    }
  }
  for (int m = 0; m < 4; ++m) {
    for (int i = 0; i < 9; ++i) W.N[m][i] = 0.0;
    W.N[m][W.cols[5 + m]] = 1.0;
    for (int c = 0; c < 5; ++c) W.N[m][W.cols[c]] = -W.Q[c][5 + m];
  }
  for (int m = 0; m < 4; ++m) {                          // modified Gram-Schmidt, twice
    for (int pass = 0; pass < 2; ++pass)
      for (int k = 0; k < m; ++k) {
        double d = 0.0;
        for (int i = 0; i < 9; ++i) d += W.N[m][i] * W.N[k][i];
        for (int i = 0; i < 9; ++i) W.N[m][i] -= d * W.N[k][i];
      }
    double s = 0.0;
    for (int i = 0; i < 9; ++i) s += W.N[m][i] * W.N[m][i];
    const double in = 1.0 / sqrt(s);
    for (int i = 0; i < 9; ++i) W.N[m][i] *= in;
  }
  return true;
}

// What lane l of a group holds after fp_solve: its root's E (||E||_F = sqrt 2) if `valid`, the best of its four poses, and (the same
// on all lanes of the group) the lane whose pose wins the draw, -1: failed draw.
struct FpLane {
  bool valid;
  double E[9];
  double sum;        // smallest selection sum of this lane's poses, +inf: none
  double R[9];
  V3 t;
  int win;
};

// The five-point problem of the draw in W.F, by the 16 lanes of a group. Called by every thread of the workgroup (it holds barriers).
COV_DEV void fp_solve(FpWork& W, int l, int lane, FpLane& out) {
  if (l == 0) W.ok = fp_nullspace(W) ? 1 : 0;
  __syncthreads();
  const bool sample_ok = W.ok != 0;
  double (*Cand)[9] = reinterpret_cast<double (*)[9]>(&W.D[0][0]);   // the round's candidates; D is free once the roots are found
  const int gshift = lane & 48;
  int nacc = 0;
  // Solutions that lie close in the hidden variable merge in its polynomial, so the elimination runs three times, with z, x and y
  // hidden (the basis vectors X Y Z rotated), and a candidate joins W.Acc unless it repeats a solution.
  for (int round = 0; round < kFpRounds; ++round) {
  bool ok = sample_ok;
  // E E^T as quadratic polynomials: lanes 0..5 take the upper triangle (0,0) (0,1) (0,2) (1,1) (1,2) (2,2)
  if (l < 6) {
    const int i = l < 3 ? 0 : (l < 5 ? 1 : 2), j = l < 3 ? l : (l < 5 ? l - 2 : 2);
    double acc[10];
#pragma unroll
    for (int m = 0; m < 10; ++m) acc[m] = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      double a[4], b[4];
      fp_lin(W, 3 * i + k, a); fp_lin(W, 3 * j + k, b);
      fp_mul11(acc, a, b, 1.0);
    }
#pragma unroll
    for (int m = 0; m < 10; ++m) W.EEt[l][m] = acc[m];
  }
  __syncthreads();
  // the ten cubics: lane 3i + j holds entry (i, j) of (E E^T - tr(E E^T) / 2) E, lane 9 holds det E
  double row[20];
#pragma unroll
  for (int m = 0; m < 20; ++m) row[m] = 0.0;
  if (l < 9) {
    const int i = l / 3, j = l % 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int lo = i < k ? i : k, hi = i < k ? k : i;
      const int e = lo == 0 ? hi : (lo == 1 ? 2 + hi : 5);
      double lam[10], ev[4];
#pragma unroll
      for (int m = 0; m < 10; ++m) lam[m] = W.EEt[e][m] - (i == k ? 0.5 * (W.EEt[0][m] + W.EEt[3][m] + W.EEt[5][m]) : 0.0);
      fp_lin(W, 3 * k + j, ev);
      fp_mul21(row, lam, ev);
    }
  } else if (l == 9) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int j = (i + 1) % 3, k = (i + 2) % 3;
      double a[4], b[4], c[10];
#pragma unroll
      for (int m = 0; m < 10; ++m) c[m] = 0.0;
      fp_lin(W, 3 + j, a); fp_lin(W, 6 + k, b); fp_mul11(c, a, b, 1.0);
      fp_lin(W, 3 + k, a); fp_lin(W, 6 + j, b); fp_mul11(c, a, b, -1.0);
      fp_lin(W, i, a);
      fp_mul21(row, c, a);
    }
  }
  // Gauss-Jordan on the left 10 columns, partial pivoting; lane r holds row r, the pivot row is broadcast inside the group
#pragma unroll
  for (int c = 0; c < 10; ++c) {
    double bv = (l >= c && l < 10) ? fabs(row[c]) : -1.0;
    if (!(bv == bv)) bv = -1.0;
    int bi = l;
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1) {
      const double ov = __shfl_xor(bv, off, kFpLanes);
      const int oi = __shfl_xor(bi, off, kFpLanes);
      if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    ok = ok && bv > 0.0;
    const double pc = __shfl(row[c], bi, kFpLanes), cc = __shfl(row[c], c, kFpLanes);
    if (l == bi) row[c] = cc;
    if (l == c) row[c] = pc;
    const double f = row[c], inv = 1.0 / pc;
#pragma unroll
    for (int k = c + 1; k < 20; ++k) {
      const double pk = __shfl(row[k], bi, kFpLanes), ck = __shfl(row[k], c, kFpLanes);
      if (l == bi) row[k] = ck;
      const double pn = pk * inv;
      row[k] = l == c ? pn : row[k] - f * pn;
    }
    row[c] = l == c ? 1.0 : 0.0;
  }
  if (l < 10) {
#pragma unroll
    for (int k = 0; k < 10; ++k) W.B[l][k] = row[10 + k];
  }
  __syncthreads();
  // Nister: <x2z> - z <x2>, <y2z> - z <y2>, <xyz> - z <xy> give C(z) [x y 1]^T = 0
  if (l < 3) {
    const double *e = W.B[4 + 2 * l], *f = W.B[5 + 2 * l];
    double* C = W.C[l];
    C[0] = e[2]; C[1] = e[1] - f[2]; C[2] = e[0] - f[1]; C[3] = -f[0];
    C[4] = e[5]; C[5] = e[4] - f[5]; C[6] = e[3] - f[4]; C[7] = -f[3];
    C[8] = e[9]; C[9] = e[8] - f[9]; C[10] = e[7] - f[8]; C[11] = e[6] - f[7]; C[12] = -f[6];
  }
  __syncthreads();
  // det C(z), expanded along the quartics: lane r takes the term of row r
  if (l < 3) {
    const int r1 = l == 0 ? 1 : 0, r2 = l == 2 ? 1 : 2;
    double ax[4], ay[4], bx[4], by[4], q[5], mn[7], pp[11];
#pragma unroll
    for (int m = 0; m < 4; ++m) { ax[m] = W.C[r1][m]; ay[m] = W.C[r1][4 + m]; bx[m] = W.C[r2][m]; by[m] = W.C[r2][4 + m]; }
#pragma unroll
    for (int m = 0; m < 5; ++m) q[m] = W.C[l][8 + m];
#pragma unroll
    for (int m = 0; m < 7; ++m) mn[m] = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) mn[i + j] += ax[i] * by[j] - ay[i] * bx[j];
#pragma unroll
    for (int m = 0; m < 11; ++m) pp[m] = 0.0;
    const double sg = l == 1 ? -1.0 : 1.0;
#pragma unroll
    for (int i = 0; i < 7; ++i)
#pragma unroll
      for (int j = 0; j < 5; ++j) pp[i + j] += sg * mn[i] * q[j];
#pragma unroll
    for (int m = 0; m < 11; ++m) W.Pp[l][m] = pp[m];
  }
  __syncthreads();
  if (l < 11) W.D[0][l] = W.Pp[0][l] + W.Pp[1][l] + W.Pp[2][l];
  __syncthreads();
  if (l < 11) {                                          // p^(m) / m!: coefficient j is C(j + m, m) a[j + m]
    double bin = 1.0;
    for (int m = 1; m <= 10; ++m) {
      if (l + m > 10) break;
      bin = bin * (double)(l + m) / (double)m;
      W.D[m][l] = W.D[0][l + m] * bin;
    }
  }
  double bound;                                          // Cauchy; the derivatives' roots lie in the hull of the roots
  {
    double mx = 0.0;
#pragma unroll
    for (int j = 0; j < 10; ++j) mx = fmax(mx, fabs(W.D[0][j]));
    bound = 1.0 + mx / fabs(W.D[0][10]);
    bool fin = isfinite(bound);
#pragma unroll
    for (int j = 0; j < 11; ++j) fin = fin && isfinite(W.D[0][j]);
    ok = ok && fin;
  }
  __syncthreads();
  // real roots: level d brackets the roots of the derivative of degree d by those of degree d - 1; lane i bisects bracket i
  int nr = 0, cur = 0;
  for (int d = 1; d <= 10; ++d) {
    const int m = 10 - d;
    double cf[11];
#pragma unroll
    for (int j = 0; j < 11; ++j) cf[j] = j <= d ? W.D[m][j] : 0.0;
    auto ev = [&](double z) {
      double a = cf[10];
#pragma unroll
      for (int j = 9; j >= 0; --j) a = a * z + cf[j];
      return a;
    };
    bool has = false;
    double root = 0.0;
    if (ok && l <= nr) {
      double lo = l == 0 ? -bound : W.R[cur][l - 1], hi = l == nr ? bound : W.R[cur][l];
      const double flo = ev(lo), fhi = ev(hi);
      const bool neg = flo < 0.0;
      has = neg != (fhi < 0.0);
      unsigned long long klo = fp_key(lo), khi = fp_key(hi);
      for (int it = 0; it < kFpBisect; ++it) {
        const unsigned long long kmid = klo + ((khi - klo) >> 1);
        if ((ev(fp_unkey(kmid)) < 0.0) == neg) klo = kmid; else khi = kmid;
      }
      root = fp_unkey(klo);
    }
    const unsigned gm = (unsigned)((__ballot(has) >> gshift) & 0xFFFFull);
    if (has) W.R[cur ^ 1][__popc(gm & ((1u << l) - 1u))] = root;
    nr = __popc(gm);
    cur ^= 1;
    __syncthreads();
  }
  // lane i takes root i
  bool cand = false;
  double E[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) E[i] = 0.0;
  if (ok && l < nr) {
    double x, y, z = W.R[cur][l];
    {
      V3 cz[3];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const double* C = W.C[r];
        cz[r] = v3(((C[3] * z + C[2]) * z + C[1]) * z + C[0], ((C[7] * z + C[6]) * z + C[5]) * z + C[4],
                   (((C[12] * z + C[11]) * z + C[10]) * z + C[9]) * z + C[8]);
      }
      V3 v = cross(cz[0], cz[1]);
      const V3 v1 = cross(cz[0], cz[2]), v2 = cross(cz[1], cz[2]);
      if (fabs(v1.z) > fabs(v.z)) v = v1;
      if (fabs(v2.z) > fabs(v.z)) v = v2;
      x = v.x / v.z; y = v.y / v.z;
    }
    for (int it = 0; it < kFpPolish; ++it) {             // Gauss-Newton on the ten cubics at E itself: what the elimination lost does not stay
      double Ev[9], G[9], Pm[9], res[10], J[3][10];
#pragma unroll
      for (int i = 0; i < 9; ++i) Ev[i] = x * W.N[0][i] + y * W.N[1][i] + z * W.N[2][i] + W.N[3][i];
      fp_mmt(Ev, Ev, G);
      fp_mm(G, Ev, Pm);
      const double tr = G[0] + G[4] + G[8];
      const V3 r0 = v3(Ev[0], Ev[1], Ev[2]), r1 = v3(Ev[3], Ev[4], Ev[5]), r2 = v3(Ev[6], Ev[7], Ev[8]);
      const V3 k0 = cross(r1, r2), k1 = cross(r2, r0), k2 = cross(r0, r1);
      const double cof[9] = {k0.x, k0.y, k0.z, k1.x, k1.y, k1.z, k2.x, k2.y, k2.z};
#pragma unroll
      for (int i = 0; i < 9; ++i) res[i] = 2.0 * Pm[i] - tr * Ev[i];
      res[9] = dot(r0, k0);
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        double dE[9], K[9], S[9], A1[9], A2[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) dE[i] = W.N[a][i];
        fp_mmt(dE, Ev, K);
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
          for (int j = 0; j < 3; ++j) S[3 * i + j] = K[3 * i + j] + K[3 * j + i];
        fp_mm(S, Ev, A1);
        fp_mm(G, dE, A2);
        const double dtr = 2.0 * (K[0] + K[4] + K[8]);
        double dd = 0.0;
#pragma unroll
        for (int i = 0; i < 9; ++i) { J[a][i] = 2.0 * (A1[i] + A2[i]) - dtr * Ev[i] - tr * dE[i]; dd += cof[i] * dE[i]; }
        J[a][9] = dd;
      }
      double hxx = 0, hxy = 0, hxz = 0, hyy = 0, hyz = 0, hzz = 0, gx = 0, gy = 0, gz = 0;
#pragma unroll
      for (int r = 0; r < 10; ++r) {
        hxx += J[0][r] * J[0][r]; hxy += J[0][r] * J[1][r]; hxz += J[0][r] * J[2][r];
        hyy += J[1][r] * J[1][r]; hyz += J[1][r] * J[2][r]; hzz += J[2][r] * J[2][r];
        gx += J[0][r] * res[r]; gy += J[1][r] * res[r]; gz += J[2][r] * res[r];
      }
      const double c00 = hyy * hzz - hyz * hyz, c01 = hxz * hyz - hxy * hzz, c02 = hxy * hyz - hxz * hyy;
      const double c11 = hxx * hzz - hxz * hxz, c12 = hxy * hxz - hxx * hyz, c22 = hxx * hyy - hxy * hxy;
      const double det = hxx * c00 + hxy * c01 + hxz * c02;
      const double sx = (c00 * gx + c01 * gy + c02 * gz) / det, sy = (c01 * gx + c11 * gy + c12 * gz) / det, sz = (c02 * gx + c12 * gy + c22 * gz) / det;
      if (isfinite(sx) && isfinite(sy) && isfinite(sz)) { x -= sx; y -= sy; z -= sz; }
    }
    double nf = 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) { E[i] = x * W.N[0][i] + y * W.N[1][i] + z * W.N[2][i] + W.N[3][i]; nf += E[i] * E[i]; }
    const double sc = sqrt(2.0 / nf);
#pragma unroll
    for (int i = 0; i < 9; ++i) E[i] *= sc;
    // the ten cubics at E
    const V3 r0 = v3(E[0], E[1], E[2]), r1 = v3(E[3], E[4], E[5]), r2 = v3(E[6], E[7], E[8]);
    double res = fabs(dot(r0, cross(r1, r2)));
    {
      const double g00 = dot(r0, r0), g01 = dot(r0, r1), g02 = dot(r0, r2), g11 = dot(r1, r1), g12 = dot(r1, r2), g22 = dot(r2, r2);
      const double ht = 0.5 * (g00 + g11 + g22);
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        res = fmax(res, fabs(2.0 * ((g00 - ht) * E[j] + g01 * E[3 + j] + g02 * E[6 + j])));
        res = fmax(res, fabs(2.0 * (g01 * E[j] + (g11 - ht) * E[3 + j] + g12 * E[6 + j])));
        res = fmax(res, fabs(2.0 * (g02 * E[j] + g12 * E[3 + j] + (g22 - ht) * E[6 + j])));
      }
    }
    cand = isfinite(sc) && res <= kFpCubicGate;
#pragma unroll
    for (int i = 0; i < 9; ++i) cand = cand && isfinite(E[i]);
  }
  if (l < 10) {
#pragma unroll
    for (int i = 0; i < 9; ++i) Cand[l][i] = E[i];
  }
  const unsigned cm = (unsigned)((__ballot(cand) >> gshift) & 0xFFFFull);
  __syncthreads();
  // a candidate joins unless it repeats (up to sign) a solution, or an earlier candidate of this round that itself joins: lane q's
  // verdict is final once the lanes below it are through, so the lanes are taken in order
  auto repeats = [&](const double* F) {
    double dm = 0.0, dp = 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) { dm = fmax(dm, fabs(E[i] - F[i])); dp = fmax(dp, fabs(E[i] + F[i])); }
    return fmin(dm, dp) <= kFpDedup;
  };
  for (int q = 0; q < 10; ++q)
    if (cand && q < nacc && repeats(W.Acc[q])) cand = false;
  for (int q = 0; q < 10; ++q) {
    const int joins = __shfl((int)cand, q, kFpLanes);
    if (joins && cand && l > q && repeats(Cand[q])) cand = false;
  }
  const unsigned am = (unsigned)((__ballot(cand) >> gshift) & 0xFFFFull);
  const int slot = nacc + __popc(am & ((1u << l) - 1u));
  if (cand && slot < 10) {
#pragma unroll
    for (int i = 0; i < 9; ++i) W.Acc[slot][i] = E[i];
  }
  nacc = min(10, nacc + __popc(am));
  if (l < 9) { const double a = W.N[0][l]; W.N[0][l] = W.N[1][l]; W.N[1][l] = W.N[2][l]; W.N[2][l] = a; }
  __syncthreads();
  }
  // lane i takes solution i: its poses, t the left null direction (largest cross product of two columns), R = cof(E) -+ [t]x E
  out.valid = l < nacc;
  out.sum = INFINITY;
  out.t = v3(0, 0, 0);
#pragma unroll
  for (int i = 0; i < 9; ++i) { out.E[i] = 0.0; out.R[i] = 0.0; }
  if (out.valid) {
    double E[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) { E[i] = W.Acc[l][i]; out.E[i] = E[i]; }
    const V3 r0 = v3(E[0], E[1], E[2]), r1 = v3(E[3], E[4], E[5]), r2 = v3(E[6], E[7], E[8]);
    const V3 k0 = cross(r1, r2), k1 = cross(r2, r0), k2 = cross(r0, r1);      // rows of cof(E)
    const V3 c0 = v3(E[0], E[3], E[6]), c1 = v3(E[1], E[4], E[7]), c2 = v3(E[2], E[5], E[8]);
    V3 tv = cross(c0, c1);
    const V3 t1 = cross(c0, c2), t2 = cross(c1, c2);
    if (dot(t1, t1) > dot(tv, tv)) tv = t1;
    if (dot(t2, t2) > dot(tv, tv)) tv = t2;
    tv = tv * (1.0 / sqrt(dot(tv, tv)));
    const V3 e0 = cross(tv, c0), e1 = cross(tv, c1), e2 = cross(tv, c2);   // columns of [t]x E
    const double cof[9] = {k0.x, k0.y, k0.z, k1.x, k1.y, k1.z, k2.x, k2.y, k2.z};
    const double tE[9] = {e0.x, e1.x, e2.x, e0.y, e1.y, e2.y, e0.z, e1.z, e2.z};
    for (int p = 0; p < 4; ++p) {                       // (Ra, t) (Ra, -t) (Rb, t) (Rb, -t)
      const double sr = p < 2 ? -1.0 : 1.0, st = (p & 1) ? -1.0 : 1.0;
      double R[9];
#pragma unroll
      for (int i = 0; i < 9; ++i) R[i] = cof[i] + sr * tE[i];
      const V3 tt = tv * st;
      double sum = 0.0;
      for (int k = 0; k < kFpSample; ++k) {
        const V3 f1 = v3(W.F[k][0], W.F[k][1], W.F[k][2]), f2 = v3(W.F[k][3], W.F[k][4], W.F[k][5]);
        V3 q1, q2;
        fp_reproject(R, tt, f1, f2, q1, q2);
        sum += (1.0 - dot(f1, q1)) + (1.0 - dot(f2, q2));
      }
      if (isfinite(sum) && sum < out.sum) {
        out.sum = sum; out.t = tt;
#pragma unroll
        for (int i = 0; i < 9; ++i) out.R[i] = R[i];
      }
    }
  }
  // the draw's pose: the smallest sum, the first root on a tie
  double bs = out.sum;
  int bl = l;
#pragma unroll
  for (int off = 8; off >= 1; off >>= 1) {
    const double os = __shfl_xor(bs, off, kFpLanes);
    const int ol = __shfl_xor(bl, off, kFpLanes);
    if (os < bs || (os == bs && ol < bl)) { bs = os; bl = ol; }
  }
  out.win = bs < INFINITY ? bl : -1;
}

// correspondence i of a job: from the LDS stage (SoA, stride 1) or from global memory ([C][3], stride 3)
struct FpSrc {
  const double *ax, *ay, *az, *bx, *by, *bz;
  int s3;
  COV_DEV V3 f1(int i) const { return v3(ax[s3 * i], ay[s3 * i], az[s3 * i]); }
  COV_DEV V3 f2(int i) const { return v3(bx[s3 * i], by[s3 * i], bz[s3 * i]); }
};

__global__ __launch_bounds__(kFpThreads) void k_fivept(FpBatch B, int cap) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  FpWork* sW = reinterpret_cast<FpWork*>(sm);        // [16]
  double* sBest = reinterpret_cast<double*>(sW + kFpHyp);   // [12]
  double* sStage = sBest + 12;                       // [6][cap]
  __shared__ int sCnt[kFpHyp];                       // inlier count per hypothesis of the pass, -1: failed draw
  __shared__ int sIt, sSkip, sBestN, sBestD, sDone, sFinal;
  __shared__ double sK;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = tid / kFpLanes, l = tid % kFpLanes;
  const int o0 = B.ptr[b], n = B.ptr[b + 1] - o0;
  if (n < kFpSample) {                               // no sample can be drawn, no model
    for (int i = tid; i < n; i += kFpThreads) B.inlier[o0 + i] = 0;
    if (tid == 0) {
      B.inliers[b] = 0; B.status[b] = 1;
      if (B.iterations) B.iterations[b] = 0;
      if (B.best_draw) B.best_draw[b] = -1;
    }
    return;
  }
  FpSrc S;
  if (n <= cap) {
    for (int i = tid; i < n; i += kFpThreads) {
      const size_t c = (size_t)(o0 + i);
      sStage[i] = B.f1[3 * c]; sStage[cap + i] = B.f1[3 * c + 1]; sStage[2 * cap + i] = B.f1[3 * c + 2];
      sStage[3 * cap + i] = B.f2[3 * c]; sStage[4 * cap + i] = B.f2[3 * c + 1]; sStage[5 * cap + i] = B.f2[3 * c + 2];
    }
    S = FpSrc{sStage, sStage + cap, sStage + 2 * cap, sStage + 3 * cap, sStage + 4 * cap, sStage + 5 * cap, 1};
  } else {
    const double *a = B.f1 + 3 * (size_t)o0, *c = B.f2 + 3 * (size_t)o0;
    S = FpSrc{a, a + 1, a + 2, c, c + 1, c + 2, 3};
  }
  if (tid == 0) { sIt = 0; sSkip = 0; sBestN = INT_MIN; sBestD = -1; sDone = 0; sK = 1.0; }
  __syncthreads();
  const unsigned long long seed = B.seed[b];
  const double th = B.threshold, sigma = B.sigma;
  const int maxit = B.max_iterations, max_skip = 10 * maxit;
  FpWork& W = sW[g];
  for (int base = 0; ; base += kFpHyp) {
    // (a) one draw and one five-point problem per group
    if (l == 0) fp_draw(W, seed, (unsigned long long)(base + g), n);
    __syncthreads();
    if (l < kFpSample) {
      const V3 a = S.f1(W.idx[l]), c = S.f2(W.idx[l]);
      W.F[l][0] = a.x; W.F[l][1] = a.y; W.F[l][2] = a.z; W.F[l][3] = c.x; W.F[l][4] = c.y; W.F[l][5] = c.z;
    }
    __syncthreads();
    {
      FpLane h;
      fp_solve(W, l, lane, h);
      if (l == h.win) {
#pragma unroll
        for (int i = 0; i < 9; ++i) W.H[i] = h.R[i];
        W.H[9] = h.t.x; W.H[10] = h.t.y; W.H[11] = h.t.z;
      }
      if (l == 0) sCnt[g] = h.win >= 0 ? 0 : -1;
    }
    __syncthreads();
    // (b) inlier counts: wave w scores hypotheses w, w + 4, ...; lanes over the correspondences
    for (int hh = wave; hh < kFpHyp; hh += kFpThreads / 64) {
      if (sCnt[hh] < 0) continue;                    // wave-uniform (LDS broadcast)
      double R[9];
#pragma unroll
      for (int i = 0; i < 9; ++i) R[i] = sW[hh].H[i];
      const V3 t = v3(sW[hh].H[9], sW[hh].H[10], sW[hh].H[11]);
      int cnt = 0;
      for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane, ii = i < n ? i : 0;
        const bool in = i < n && fp_score(R, t, S.f1(ii), S.f2(ii), sigma) < th;
        cnt += __popcll(__ballot(in));
      }
      if (lane == 0) sCnt[hh] = cnt;
    }
    __syncthreads();
    // (c) opengv's loop over the pass, in draw order
    if (tid == 0) {
      int it = sIt, skipped = sSkip, bestn = sBestN, done = 0;
      double k = sK;
      for (int j = 0; j < kFpHyp; ++j) {
        if (!(it < k && skipped < max_skip)) { done = 1; break; }
        const int c = sCnt[j];
        if (c < 0) { ++skipped; continue; }
        if (c > bestn) {
          bestn = c; sBestD = base + j;
          for (int q = 0; q < 12; ++q) sBest[q] = sW[j].H[q];
          const double w = (double)bestn / (double)n;
          double pno = 1.0 - pow(w, (double)kFpSample);
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
  // final inliers of the best model; found iff at least min_inliers and fewer than max_iterations iterations
  if (tid == 0) sFinal = 0;
  __syncthreads();
  const bool have = sBestD >= 0;
  double R[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = have ? sBest[i] : 0.0;
  const V3 t = have ? v3(sBest[9], sBest[10], sBest[11]) : v3(0, 0, 0);
  if (have) {
    int cnt = 0;
    for (int i = tid; i < n; i += kFpThreads) cnt += fp_score(R, t, S.f1(i), S.f2(i), sigma) < th ? 1 : 0;
    atomicAdd(&sFinal, cnt);
  }
  __syncthreads();
  const int nin = sFinal;
  const int status = !have ? 2 : (nin < B.min_inliers ? 3 : (sIt >= maxit ? 4 : 0));
  for (int i = tid; i < n; i += kFpThreads) B.inlier[o0 + i] = status == 0 && fp_score(R, t, S.f1(i), S.f2(i), sigma) < th ? 1 : 0;
  if (tid == 0) {
    B.inliers[b] = nin; B.status[b] = status;
    if (B.iterations) B.iterations[b] = sIt;
    if (B.best_draw) B.best_draw[b] = sBestD;
    if (status == 0) {
      double* T = B.T + 7 * (size_t)b;
      fp_rot_to_quat(R, T);
      T[4] = t.x; T[5] = t.y; T[6] = t.z;
    }
  }
}

// test entry point: the five-point problem of every 8-tuple on its slots 0..4, all solutions, and the pose the 8 points pick
__global__ __launch_bounds__(kFpThreads) void k_fivept_solve(int num, const double* F1, const double* F2, double* E, int* nsol, double* T, int* chosen) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  FpWork* sW = reinterpret_cast<FpWork*>(sm);
  const int tid = threadIdx.x, lane = tid & 63, g = tid / kFpLanes, l = tid % kFpLanes;
  const int e = blockIdx.x * kFpHyp + g, ee = e < num ? e : num - 1;
  FpWork& W = sW[g];
  if (l < kFpSample) {
    const double *a = F1 + 24 * (size_t)ee + 3 * l, *c = F2 + 24 * (size_t)ee + 3 * l;
    W.F[l][0] = a[0]; W.F[l][1] = a[1]; W.F[l][2] = a[2]; W.F[l][3] = c[0]; W.F[l][4] = c[1]; W.F[l][5] = c[2];
  }
  __syncthreads();
  FpLane h;
  fp_solve(W, l, lane, h);
  const unsigned gm = (unsigned)((__ballot(h.valid) >> (lane & 48)) & 0xFFFFull);
  if (e >= num) return;
  if (h.valid) {
    double big = 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) if (fabs(h.E[i]) > fabs(big)) big = h.E[i];
    const double sg = big < 0.0 ? -1.0 : 1.0;
    double* o = E + 90 * (size_t)e + 9 * __popc(gm & ((1u << l) - 1u));
#pragma unroll
    for (int i = 0; i < 9; ++i) o[i] = sg * h.E[i];
  }
  if (l == 0) {
    nsol[e] = __popc(gm);
    chosen[e] = h.win >= 0 ? __popc(gm & ((1u << h.win) - 1u)) : -1;
  }
  if (l == h.win) {
    double* o = T + 7 * (size_t)e;
    fp_rot_to_quat(h.R, o);
    o[4] = h.t.x; o[5] = h.t.y; o[6] = h.t.z;
  }
}

}  // namespace

static size_t fivept_lds_bytes(int cap) { return sizeof(FpWork) * kFpHyp + sizeof(double) * (12 + 6 * (size_t)(cap > 0 ? cap : 0)); }

void fivept_limits(int out[4]) { out[0] = kFpStageCap; out[1] = kFpHyp; out[2] = kFpSample; out[3] = kFpMaxIterations; }

hipError_t launch_fivept(int num, const int* ptr, const double* f1, const double* f2, const unsigned long long* seed, double* T, unsigned char* inlier,
                   int* inliers, int* status, int* iterations, int* best_draw, int min_inliers, int max_iterations, double probability,
                   double threshold, double sigma, int max_n, hipStream_t st) {
  if (num <= 0) return hipSuccess;
  const int cap = max_n < kFpStageCap ? max_n : kFpStageCap;
  const size_t lds = fivept_lds_bytes(cap);
  if (const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_fivept), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) return e;
  FpBatch B{num, ptr, f1, f2, seed, T, inlier, inliers, status, iterations, best_draw, min_inliers, max_iterations, probability, threshold, sigma};
  hipLaunchKernelGGL(k_fivept, dim3(num), dim3(kFpThreads), lds, st, B, cap);
  return hipGetLastError();
}

hipError_t launch_fivept_solve(int num, const double* f1, const double* f2, double* E, int* nsol, double* T, int* chosen, hipStream_t st) {
  if (num <= 0) return hipSuccess;
  const size_t lds = fivept_lds_bytes(0);
  if (const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_fivept_solve), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) return e;
  hipLaunchKernelGGL(k_fivept_solve, dim3((num + kFpHyp - 1) / kFpHyp), dim3(kFpThreads), lds, st, num, f1, f2, E, nsol, T, chosen);
  return hipGetLastError();
}

}  // namespace covgpu
