// k_ncrelpose.hip — the back half of COVINS-G's loop verification, batched: the non-central 17-point RANSAC over all cells' matches, the
// non-linear polish of its model and the sampled 6x6 covariance of the loop edge (RelNonCentralPosSolver.cpp:149-301).
//
// One workgroup of 256 threads runs one job from the first draw to the covariance, in one launch. Its rays (g1, o1, g2, o2 per
// correspondence, in the two viewpoints' frames) are staged into LDS as SoA; a job longer than the cap computes them from global memory
// with the same arithmetic. A pass makes 8 draws, one per group of 32 lanes: (a) the group builds the N x 18 generalised epipolar system
// of its draw in LDS, column-major, one lane per column, reduces it to its triangular factor by Householder reflections (the reflector
// of a step is broadcast through LDS) and takes the singular values and the right singular vector of the smallest by one-sided Jacobi on
// the 18 x 18 factor, the columns of [R; V] in the registers of 18 lanes, partners exchanged by shuffles in a round-robin order: one
// method for N = 17 (a zero row is appended) and for the least-squares solves of N = 4 cells, and none that squares the condition number;
// lane 0 then takes the pose out of the null vector. (b) The four waves score the pass's models over the correspondences, counting with a
// ballot. (c) Thread 0 replays the sequential loop over the pass in draw order. The polish (Levenberg-Marquardt over 6 parameters, all
// threads over the inliers, sums reduced in a fixed order) and the covariance passes run on the same staged rays. FP64 throughout. Every
// loop has a compile-time bound and every branch around a barrier is uniform.
#include "common.hpp"
#include "dev_math.hpp"
#include "ncrelpose.hpp"

#include <cfloat>
#include <climits>

namespace covgpu {
using namespace covdev;

namespace {

constexpr int kNcThreads = 256;
constexpr int kNcLanes = 32;                        // lanes per draw
constexpr int kNcHyp = kNcThreads / kNcLanes;       // draws per pass
constexpr int kNcSample = 17;
constexpr int kNcCols = 18;                         // unknowns: vec E | vec R~
constexpr int kNcMaxRows = 64;                      // rows of a linear solve: 4 per cell, 16 cells
constexpr int kNcMaxCells = 16;
constexpr int kNcCovSample = 4;                     // correspondences per cell in a covariance draw
constexpr int kNcMaxCovRows = 256;
constexpr int kNcStageCap = 512;                    // correspondences staged into LDS (96 B each)
constexpr int kNcMaxIterations = 100000;
constexpr int kNcSweeps = 16;                       // Jacobi sweeps over the 18 x 18 factor
constexpr int kNcPolar = 12;                        // scaled Newton steps to the nearest rotation
constexpr int kNcLmIters = 40;                      // Levenberg-Marquardt steps of the polish, accepted or not
constexpr double kNcRankTol = 1e-12;
constexpr double kNcLmStep = 1e-6;                  // central differences
constexpr double kNcLmTol = 1e-12;                  // the polish ends at a step below this in every parameter
constexpr int kNcRed = 28;                          // 21 of J^T J, 6 of J^T r, the cost
constexpr unsigned long long kNcCovSalt = 0x17C0F17C0F17C0F1ull;

struct NcBatch {
  int num, cells;
  const int *ptr, *cell;                            // [num+1], [num][cells+1] relative to the job
  const double *f1, *f2;                            // [C][3]
  const int *cam1, *cam2;                           // [C] into the job's cameras
  const int* cam_ptr;                               // [num+1]
  const double* cam;                                // [M][12]: R_c row-major | o_c
  const double *Tq, *Tc;                            // [num][7]
  const unsigned long long* seed;
  double *T, *Tr, *Ts, *cov;
  unsigned char* inlier;
  int* list;                                        // [C] scratch: the ascending inlier list of every job
  int *inliers, *status, *iterations, *best_draw, *cov_rows, *cov_draws;
  int min_inliers, max_iterations, cov_iters, cov_max_iters;
  double probability, threshold, th_cov, cov_thres;
};

struct NcWork {                                     // LDS work area of one group of 32 lanes
  double A[kNcCols][kNcMaxRows + 1];                // the system, column-major (the odd stride spreads the lanes over the banks)
  double v[2][kNcMaxRows];                          // the reflector of this / the previous step
  double beta[2];
  double x[kNcCols];                                // the null vector
  double sv[3];                                     // sigma_1, sigma_17, sigma_18
  double H[12];                                     // the draw's model: R row-major | t
  int idx[kNcMaxRows];
  int ok;
};

struct NcRay { V3 g1, o1, g2, o2; };

COV_DEV unsigned long long nc_splitmix64(unsigned long long x) {
  unsigned long long z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// `cnt` (<= 17) distinct indices of [0, n) into out: partial Fisher-Yates, slot k swaps position k with k + splitmix64(key + k) mod (n - k).
// Only the displaced values are remembered (k_fivept.hip's fp_draw).
COV_DEV void nc_draw(int* out, unsigned long long key, int cnt, int n) {
  int opos[kNcSample], oval[kNcSample];
  int no = 0;
  for (int k = 0; k < kNcSample; ++k) {
    if (k >= cnt) break;
    const unsigned long long x = nc_splitmix64(key + (unsigned long long)k);
    const int j = k + (int)(x % (unsigned long long)(n - k));
    int vk = k, vj = j;
    for (int o = 0; o < kNcSample; ++o) {
      if (o < no && opos[o] == k) vk = oval[o];
      if (o < no && opos[o] == j) vj = oval[o];
    }
    bool put = false;
    for (int o = 0; o < kNcSample; ++o) if (o < no && opos[o] == j) { oval[o] = vk; put = true; }
    if (!put) { opos[no] = j; oval[no] = vk; ++no; }
    out[k] = vj;
  }
}

// the two rays of a correspondence in their viewpoints: g = R_c f, origin o_c. Written with explicit fma so that the staged and the
// global-memory path round alike.
COV_DEV V3 nc_rot(const double* R, V3 f) {
  return v3(fma(R[0], f.x, fma(R[1], f.y, R[2] * f.z)), fma(R[3], f.x, fma(R[4], f.y, R[5] * f.z)), fma(R[6], f.x, fma(R[7], f.y, R[8] * f.z)));
}
COV_DEV NcRay nc_make_ray(const double* f1, const double* f2, const double* c1, const double* c2) {
  NcRay r;
  r.g1 = nc_rot(c1, ld3(f1)); r.o1 = ld3(c1 + 9);
  r.g2 = nc_rot(c2, ld3(f2)); r.o2 = ld3(c2 + 9);
  return r;
}

struct NcSrc {
  const double* st;                                 // [12][cap] or unused
  int cap, staged;
  const double *f1, *f2, *cam;                      // of the job
  const int *c1, *c2;
  COV_DEV NcRay ray(int i) const {
    if (staged) {
      NcRay r;
      r.g1 = v3(st[i], st[cap + i], st[2 * cap + i]); r.o1 = v3(st[3 * cap + i], st[4 * cap + i], st[5 * cap + i]);
      r.g2 = v3(st[6 * cap + i], st[7 * cap + i], st[8 * cap + i]); r.o2 = v3(st[9 * cap + i], st[10 * cap + i], st[11 * cap + i]);
      return r;
    }
    return nc_make_ray(f1 + 3 * (size_t)i, f2 + 3 * (size_t)i, cam + 12 * (size_t)c1[i], cam + 12 * (size_t)c2[i]);
  }
};

// row of the generalised epipolar system: [g1 (x) g2 , g1 (x) m2 + m1 (x) g2], m = o x g   (⚠ seventeenpt)
COV_DEV void nc_row(const NcRay& r, double row[kNcCols]) {
  const V3 m1 = cross(r.o1, r.g1), m2 = cross(r.o2, r.g2);
  const double a[3] = {r.g1.x, r.g1.y, r.g1.z}, b[3] = {r.g2.x, r.g2.y, r.g2.z};
  const double ma[3] = {m1.x, m1.y, m1.z}, mb[3] = {m2.x, m2.y, m2.z};
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) { row[3 * i + j] = a[i] * b[j]; row[9 + 3 * i + j] = a[i] * mb[j] + ma[i] * b[j]; }
}

COV_DEV void nc_rot_to_quat(const double* R, double* q) {  // Hamilton x y z w, w >= 0
  const double tr = R[0] + R[4] + R[8];
  double x, y, z, w;
  if (tr > 0) { const double s = 0.5 / sqrt(tr + 1.0); w = 0.25 / s; x = (R[7] - R[5]) * s; y = (R[2] - R[6]) * s; z = (R[3] - R[1]) * s; }
  else if (R[0] > R[4] && R[0] > R[8]) { const double s = 2.0 * sqrt(1.0 + R[0] - R[4] - R[8]); w = (R[7] - R[5]) / s; x = 0.25 * s; y = (R[1] + R[3]) / s; z = (R[2] + R[6]) / s; }
  else if (R[4] > R[8]) { const double s = 2.0 * sqrt(1.0 + R[4] - R[0] - R[8]); w = (R[2] - R[6]) / s; x = (R[1] + R[3]) / s; y = 0.25 * s; z = (R[5] + R[7]) / s; }
  else { const double s = 2.0 * sqrt(1.0 + R[8] - R[0] - R[4]); w = (R[3] - R[1]) / s; x = (R[2] + R[6]) / s; y = (R[5] + R[7]) / s; z = 0.25 * s; }
  const double sg = w < 0 ? -1.0 : 1.0, in = sg / sqrt(x * x + y * y + z * z + w * w);
  q[0] = x * in; q[1] = y * in; q[2] = z * in; q[3] = w * in;
}

COV_DEV double nc_det3(const double* X) {
  return X[0] * (X[4] * X[8] - X[5] * X[7]) - X[1] * (X[3] * X[8] - X[5] * X[6]) + X[2] * (X[3] * X[7] - X[4] * X[6]);
}
COV_DEV void nc_cof3(const double* X, double* Cf) {
  Cf[0] = X[4] * X[8] - X[5] * X[7]; Cf[1] = X[5] * X[6] - X[3] * X[8]; Cf[2] = X[3] * X[7] - X[4] * X[6];
  Cf[3] = X[2] * X[7] - X[1] * X[8]; Cf[4] = X[0] * X[8] - X[2] * X[6]; Cf[5] = X[1] * X[6] - X[0] * X[7];
  Cf[6] = X[1] * X[5] - X[2] * X[4]; Cf[7] = X[2] * X[3] - X[0] * X[5]; Cf[8] = X[0] * X[4] - X[1] * X[3];
}

// the pose of a null vector x = (vec E, vec R~), row-major, E = [t]x R up to the common scale   (⚠ seventeenpt): the sign that makes
// det R~ > 0, R the nearest rotation (the orthogonal polar factor, by Newton's iteration with Frobenius scaling), s the mean singular
// value of R~ = tr(R^T R~) / 3, t the vee of the skew part of (E / s) R^T. False: det R~ is 0 or something is not finite.
COV_DEV bool nc_pose(const double* x, double* H) {
  double E[9], Rt[9], X[9];
  double det = nc_det3(x + 9);
  if (!(det != 0.0) || !isfinite(det)) return false;
  const double sg = det < 0.0 ? -1.0 : 1.0;
#pragma unroll
  for (int i = 0; i < 9; ++i) { E[i] = sg * x[i]; Rt[i] = sg * x[9 + i]; X[i] = Rt[i]; }
  for (int it = 0; it < kNcPolar; ++it) {
    double Cf[9];
    nc_cof3(X, Cf);
    const double d = nc_det3(X);
    double nx = 0.0, ni = 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) { Cf[i] /= d; nx += X[i] * X[i]; ni += Cf[i] * Cf[i]; }   // Cf = X^-T
    const double gam = sqrt(sqrt(ni / nx));
#pragma unroll
    for (int i = 0; i < 9; ++i) X[i] = 0.5 * (gam * X[i] + Cf[i] / gam);
  }
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < 9; ++i) s += X[i] * Rt[i];
  s /= 3.0;
  double M[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) M[3 * i + j] = (E[3 * i] * X[3 * j] + E[3 * i + 1] * X[3 * j + 1] + E[3 * i + 2] * X[3 * j + 2]) / s;
  bool fin = true;
#pragma unroll
  for (int i = 0; i < 9; ++i) { H[i] = X[i]; fin = fin && isfinite(X[i]); }
  H[9] = 0.5 * (M[7] - M[5]); H[10] = 0.5 * (M[2] - M[6]); H[11] = 0.5 * (M[3] - M[1]);
  return fin && isfinite(H[9]) && isfinite(H[10]) && isfinite(H[11]);
}

// The linear solve of the system in W.A (`rows` >= 18 rows, zero rows appended to a 17-row system) by the 32 lanes of a group: W.H and
// W.ok. Called by every thread of the workgroup with the same `rows` (it holds barriers).
COV_DEV void nc_solve(NcWork& W, int l, int rows) {
  double fro = 0.0;
  if (l < kNcCols)
    for (int i = 0; i < rows; ++i) { const double a = W.A[l][i]; fro += a * a; }
#pragma unroll
  for (int off = kNcLanes / 2; off >= 1; off >>= 1) fro += __shfl_xor(fro, off, kNcLanes);
  bool ok = isfinite(fro) && fro > 0.0;
  // Householder: lane k makes the reflector of step k from its own column, the lanes right of it apply it to theirs
  for (int k = 0; k < kNcCols; ++k) {
    double* v = W.v[k & 1];
    if (l == k) {
      const double alpha = W.A[k][k];
      double sig = 0.0;
      for (int i = k + 1; i < rows; ++i) { const double a = W.A[k][i]; sig += a * a; v[i] = a; }
      const double nrm = sqrt(alpha * alpha + sig);
      const double v0 = alpha + (alpha < 0.0 ? -nrm : nrm);
      v[k] = v0;
      const double vv = v0 * v0 + sig;
      W.beta[k & 1] = vv > 0.0 ? 2.0 / vv : 0.0;
      W.A[k][k] = alpha < 0.0 ? nrm : -nrm;
    }
    __syncthreads();
    if (l > k && l < kNcCols) {
      const double beta = W.beta[k & 1];
      double w = 0.0;
      for (int i = k; i < rows; ++i) w += v[i] * W.A[l][i];
      w *= beta;
      for (int i = k; i < rows; ++i) W.A[l][i] -= w * v[i];
    }
  }
  // one-sided Jacobi on the triangular factor: lane j holds column j of [R; V]; 17 rounds of 9 disjoint pairs make a sweep
  double Rc[kNcCols], Vc[kNcCols];
#pragma unroll
  for (int i = 0; i < kNcCols; ++i) {
    Rc[i] = (l < kNcCols && i <= l) ? W.A[l < kNcCols ? l : 0][i] : 0.0;
    Vc[i] = i == l ? 1.0 : 0.0;
  }
#pragma unroll 1
  for (int sweep = 0; sweep < kNcSweeps; ++sweep) {
#pragma unroll 1
    for (int r = 0; r < kNcCols - 1; ++r) {
      int p = l;
      if (l < kNcCols - 1) { p = (2 * r - l + (kNcCols - 1)) % (kNcCols - 1); if (p == l) p = kNcCols - 1; }
      else if (l == kNcCols - 1) p = r;
      double oR[kNcCols], oV[kNcCols];
      double aa = 0.0, bb = 0.0, ab = 0.0;
#pragma unroll
      for (int i = 0; i < kNcCols; ++i) {
        oR[i] = __shfl(Rc[i], p, kNcLanes);
        oV[i] = __shfl(Vc[i], p, kNcLanes);
        aa += Rc[i] * Rc[i]; bb += oR[i] * oR[i]; ab += Rc[i] * oR[i];
      }
      const bool lo = l < p;
      const double alpha = lo ? aa : bb, bet = lo ? bb : aa;
      const bool rot = p != l && fabs(ab) > 1.1e-16 * sqrt(aa * bb);
      const double zeta = (bet - alpha) / (2.0 * ab);
      const double t = (zeta < 0.0 ? -1.0 : 1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
      const double c = 1.0 / sqrt(1.0 + t * t), s = lo ? -c * t : c * t;
      if (rot && isfinite(c) && isfinite(s)) {
#pragma unroll
        for (int i = 0; i < kNcCols; ++i) { Rc[i] = c * Rc[i] + s * oR[i]; Vc[i] = c * Vc[i] + s * oV[i]; }
      }
    }
  }
  double n2 = 0.0;
#pragma unroll
  for (int i = 0; i < kNcCols; ++i) n2 += Rc[i] * Rc[i];
  const bool mine = l < kNcCols;
  if (!(n2 == n2)) { n2 = 0.0; ok = false; }
  double mn = mine ? n2 : INFINITY, mx = mine ? n2 : -INFINITY;
  int ml = l;
#pragma unroll
  for (int off = kNcLanes / 2; off >= 1; off >>= 1) {
    const double om = __shfl_xor(mn, off, kNcLanes), ox = __shfl_xor(mx, off, kNcLanes);
    const int ol = __shfl_xor(ml, off, kNcLanes);
    if (om < mn || (om == mn && ol < ml)) { mn = om; ml = ol; }
    mx = fmax(mx, ox);
  }
  double m2 = (mine && l != ml) ? n2 : INFINITY;
#pragma unroll
  for (int off = kNcLanes / 2; off >= 1; off >>= 1) m2 = fmin(m2, __shfl_xor(m2, off, kNcLanes));
  const unsigned long long okm = __ballot(ok);      // a NaN column on any lane of the group fails the draw
  const int gsh = (threadIdx.x & 63) & ~(kNcLanes - 1);
  ok = ((okm >> gsh) & 0xFFFFFFFFull) == 0xFFFFFFFFull;
  ok = ok && isfinite(mx) && m2 > kNcRankTol * kNcRankTol * mx;
  if (l == ml) {
#pragma unroll
    for (int i = 0; i < kNcCols; ++i) W.x[i] = Vc[i];
  }
  if (l == 0) { W.sv[0] = sqrt(mx); W.sv[1] = sqrt(m2); W.sv[2] = sqrt(mn); }
  __syncthreads();
  if (l == 0) W.ok = ok && nc_pose(W.x, W.H) ? 1 : 0;
  __syncthreads();
}

// triangulate2 on general rays under T_12 = [R | t]: ray 1 (o1, g1), ray 2 (R o2 + t, R g2), P the midpoint of their closest points; u1, u2
// the directions from the two origins to P, g the rotated g2   (⚠ getSelectedDistancesToModel)
COV_DEV void nc_reproject(const double* R, V3 t, const NcRay& r, V3& u1, V3& u2, V3& g) {
  g = v3(R[0] * r.g2.x + R[1] * r.g2.y + R[2] * r.g2.z, R[3] * r.g2.x + R[4] * r.g2.y + R[5] * r.g2.z, R[6] * r.g2.x + R[7] * r.g2.y + R[8] * r.g2.z);
  const V3 o = v3(R[0] * r.o2.x + R[1] * r.o2.y + R[2] * r.o2.z, R[3] * r.o2.x + R[4] * r.o2.y + R[5] * r.o2.z, R[6] * r.o2.x + R[7] * r.o2.y + R[8] * r.o2.z) + t;
  const V3 b = o - r.o1;
  const double b0 = dot(b, r.g1), b1 = dot(b, g);
  const double a00 = dot(r.g1, r.g1), a01 = -dot(r.g1, g), a11 = -dot(g, g);
  const double det = a00 * a11 + a01 * a01;
  const double l0 = (a11 * b0 - a01 * b1) / det, l1 = (a01 * b0 + a00 * b1) / det;
  const V3 P = (r.o1 + r.g1 * l0 + o + g * l1) * 0.5;
  const V3 d1 = P - r.o1, d2 = P - o;
  u1 = d1 * (1.0 / sqrt(dot(d1, d1)));
  u2 = d2 * (1.0 / sqrt(dot(d2, d2)));
}
COV_DEV double nc_score(const double* R, V3 t, const NcRay& r) {
  V3 u1, u2, g;
  nc_reproject(R, t, r, u1, u2, g);
  return (1.0 - dot(r.g1, u1)) + (1.0 - dot(g, u2));
}
// the six residuals of the polish   (⚠ optimize_nonlinear)
COV_DEV void nc_resid(const double* H, const NcRay& r, double e[6]) {
  V3 u1, u2, g;
  nc_reproject(H, v3(H[9], H[10], H[11]), r, u1, u2, g);
  e[0] = u1.x - r.g1.x; e[1] = u1.y - r.g1.y; e[2] = u1.z - r.g1.z;
  e[3] = u2.x - g.x; e[4] = u2.y - g.y; e[5] = u2.z - g.z;
}

// H (+) delta: R <- R Exp(delta[0..2]), t <- t + delta[3..5]
COV_DEV void nc_retract(const double* H, const double* d, double* out) {
  const M3 Ex = qrot(qexp(v3(d[0], d[1], d[2])));
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) out[3 * i + j] = H[3 * i] * Ex.m[j] + H[3 * i + 1] * Ex.m[3 + j] + H[3 * i + 2] * Ex.m[6 + j];
  out[9] = H[9] + d[3]; out[10] = H[10] + d[4]; out[11] = H[11] + d[5];
}

// [q | t] of the composition a b and of the inverse
COV_DEV void nc_compose(const double* a, const double* b, double* o) {
  const Q4 qa = qnormalize(ldq(a)), qb = qnormalize(ldq(b));
  const Q4 q = qnormalize(qmul(qa, qb));
  const V3 t = mul(qrot(qa), ld3(b + 4)) + ld3(a + 4);
  o[0] = q.x; o[1] = q.y; o[2] = q.z; o[3] = q.w; o[4] = t.x; o[5] = t.y; o[6] = t.z;
}
COV_DEV void nc_inverse(const double* a, double* o) {
  const Q4 qa = qnormalize(ldq(a));
  const V3 t = -mulT(qrot(qa), ld3(a + 4));
  o[0] = -qa.x; o[1] = -qa.y; o[2] = -qa.z; o[3] = qa.w; o[4] = t.x; o[5] = t.y; o[6] = t.z;
}
COV_DEV void nc_model_to_T(const double* H, double* T) {
  nc_rot_to_quat(H, T);
  T[4] = H[9]; T[5] = H[10]; T[6] = H[11];
}
// T_s1s2 = T_sc(Q) T_c1c2 T_sc(C)^-1   (RelNonCentralPosSolver.cpp:178-183 with the world poses cancelled)
COV_DEV void nc_sensor_pose(const double* Tq, const double* Tc, const double* H, double* Ts) {
  double T12[7], Tci[7], a[7];
  nc_model_to_T(H, T12);
  nc_inverse(Tc, Tci);
  nc_compose(Tq, T12, a);
  nc_compose(a, Tci, Ts);
  if (Ts[3] < 0.0) { Ts[0] = -Ts[0]; Ts[1] = -Ts[1]; Ts[2] = -Ts[2]; Ts[3] = -Ts[3]; }
}
// ⚠ robopt Minus: 2 vec(q_iter (x) q_ref^-1), the sign with w >= 0
COV_DEV V3 nc_minus(const double* qi, const double* qr) {
  Q4 d = qmul(ldq(qi), qconj(ldq(qr)));
  const double s = d.w < 0.0 ? -2.0 : 2.0;
  return v3(s * d.x, s * d.y, s * d.z);
}

// sums the kNcRed partial values of every thread in a fixed order: lanes by xor shuffles, then the four waves in turn; the totals are in
// red[0..kNcRed) after the barrier
COV_DEV void nc_reduce(const double* part, int cnt, double* sRed, double* red, int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  for (int q = 0; q < kNcRed; ++q) {
    if (q >= cnt) break;
    const double s = wave_sum(part[q]);
    if (lane == 0) sRed[wave * kNcRed + q] = s;
  }
  __syncthreads();
  if (tid < cnt) red[tid] = ((sRed[tid] + sRed[kNcRed + tid]) + sRed[2 * kNcRed + tid]) + sRed[3 * kNcRed + tid];
  __syncthreads();
}

__global__ __launch_bounds__(kNcThreads) void k_ncrelpose(NcBatch B, int cap) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  NcWork* sW = reinterpret_cast<NcWork*>(sm);                 // [8]
  double* sBest = reinterpret_cast<double*>(sW + kNcHyp);     // [12] the RANSAC model
  double* sPol = sBest + 12;                                   // [12] the polished model
  double* sCand = sPol + 12;                                   // [12] the step under test
  double* sPert = sCand + 12;                                  // [12][12] the model moved by +-h along each parameter
  double* sRed = sPert + 144;                                  // [4][28]
  double* sTot = sRed + 4 * kNcRed;                            // [28]
  double* sRows = sTot + kNcRed;                               // [256][6]
  double* sStage = sRows + 6 * kNcMaxCovRows;                  // [12][cap]
  __shared__ int sCnt[kNcHyp];
  __shared__ int sCell[kNcMaxCells + 1], sCellIn[kNcMaxCells + 1];
  __shared__ int sIt, sSkip, sBestN, sBestD, sDone, sFinal, sNrows, sNdraws;
  __shared__ double sK, sLambda, sCost, sTs[7];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = tid / kNcLanes, l = tid % kNcLanes;
  const int o0 = B.ptr[b], n = B.ptr[b + 1] - o0, cells = B.cells;
  if (n < kNcSample) {
    for (int i = tid; i < n; i += kNcThreads) B.inlier[o0 + i] = 0;
    if (tid == 0) { B.inliers[b] = 0; B.status[b] = 1; B.iterations[b] = 0; B.best_draw[b] = -1; B.cov_rows[b] = 0; B.cov_draws[b] = 0; }
    return;
  }
  NcSrc S;
  S.st = sStage; S.cap = cap; S.staged = n <= cap ? 1 : 0;
  S.f1 = B.f1 + 3 * (size_t)o0; S.f2 = B.f2 + 3 * (size_t)o0; S.cam = B.cam + 12 * (size_t)B.cam_ptr[b];
  S.c1 = B.cam1 + o0; S.c2 = B.cam2 + o0;
  if (S.staged) {
    for (int i = tid; i < n; i += kNcThreads) {
      const NcRay r = nc_make_ray(S.f1 + 3 * (size_t)i, S.f2 + 3 * (size_t)i, S.cam + 12 * (size_t)S.c1[i], S.cam + 12 * (size_t)S.c2[i]);
      sStage[i] = r.g1.x; sStage[cap + i] = r.g1.y; sStage[2 * cap + i] = r.g1.z;
      sStage[3 * cap + i] = r.o1.x; sStage[4 * cap + i] = r.o1.y; sStage[5 * cap + i] = r.o1.z;
      sStage[6 * cap + i] = r.g2.x; sStage[7 * cap + i] = r.g2.y; sStage[8 * cap + i] = r.g2.z;
      sStage[9 * cap + i] = r.o2.x; sStage[10 * cap + i] = r.o2.y; sStage[11 * cap + i] = r.o2.z;
    }
  }
  if (tid <= cells) sCell[tid] = B.cell[(size_t)b * (cells + 1) + tid];
  if (tid == 0) { sIt = 0; sSkip = 0; sBestN = INT_MIN; sBestD = -1; sDone = 0; sK = 1.0; }
  __syncthreads();
  const unsigned long long seed = B.seed[b];
  const int maxit = B.max_iterations, max_skip = 10 * maxit;
  NcWork& W = sW[g];

  // ---- the 17-point RANSAC
  for (int base = 0; ; base += kNcHyp) {
    if (l == 0) nc_draw(W.idx, seed + (unsigned long long)kNcSample * (unsigned long long)(base + g), kNcSample, n);
    __syncthreads();
    if (l < kNcCols) {                                         // 17 rows and the zero row
      double row[kNcCols];
#pragma unroll
      for (int j = 0; j < kNcCols; ++j) row[j] = 0.0;
      if (l < kNcSample) nc_row(S.ray(W.idx[l]), row);
#pragma unroll
      for (int j = 0; j < kNcCols; ++j) W.A[j][l] = row[j];
    }
    __syncthreads();
    nc_solve(W, l, kNcCols);
    if (l == 0) sCnt[g] = W.ok ? 0 : -1;
    __syncthreads();
    for (int hh = wave; hh < kNcHyp; hh += kNcThreads / 64) {
      if (sCnt[hh] < 0) continue;                              // wave-uniform
      double R[9];
#pragma unroll
      for (int i = 0; i < 9; ++i) R[i] = sW[hh].H[i];
      const V3 t = v3(sW[hh].H[9], sW[hh].H[10], sW[hh].H[11]);
      int cnt = 0;
      for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane, ii = i < n ? i : 0;
        const bool in = i < n && nc_score(R, t, S.ray(ii)) < B.threshold;
        cnt += __popcll(__ballot(in));
      }
      if (lane == 0) sCnt[hh] = cnt;
    }
    __syncthreads();
    if (tid == 0) {                                            // the sequential loop over the pass, in draw order (§4.10)
      int it = sIt, skipped = sSkip, bestn = sBestN, done = 0;
      double k = sK;
      for (int j = 0; j < kNcHyp; ++j) {
        if (!(it < k && skipped < max_skip)) { done = 1; break; }
        const int c = sCnt[j];
        if (c < 0) { ++skipped; continue; }
        if (c > bestn) {
          bestn = c; sBestD = base + j;
          for (int q = 0; q < 12; ++q) sBest[q] = sW[j].H[q];
          const double w = (double)bestn / (double)n;
          double pno = 1.0 - pow(w, (double)kNcSample);
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
  const bool have = sBestD >= 0;
  if (!have) {
    for (int i = tid; i < n; i += kNcThreads) B.inlier[o0 + i] = 0;
    if (tid == 0) { B.inliers[b] = 0; B.status[b] = 2; B.iterations[b] = sIt; B.best_draw[b] = -1; B.cov_rows[b] = 0; B.cov_draws[b] = 0; }
    return;
  }
  // ---- the inliers of the unpolished model: the mask, and the ascending list cell by cell (wave 0)
  if (wave == 0) {
    double R[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = sBest[i];
    const V3 t = v3(sBest[9], sBest[10], sBest[11]);
    int tot = 0;
    for (int c = 0; c < kNcMaxCells; ++c) {
      if (c >= cells) break;
      if (lane == 0) sCellIn[c] = tot;
      const int c0 = sCell[c], c1 = sCell[c + 1];
      for (int i0 = c0; i0 < c1; i0 += 64) {
        const int i = i0 + lane, ii = i < c1 ? i : c0;
        const bool in = i < c1 && nc_score(R, t, S.ray(ii)) < B.threshold;
        const unsigned long long m = __ballot(in);
        if (i < c1) B.inlier[o0 + i] = in ? 1 : 0;
        if (in) B.list[o0 + tot + __popcll(m & ((1ull << lane) - 1ull))] = i;
        tot += __popcll(m);
      }
    }
    if (lane == 0) { sCellIn[cells] = tot; sFinal = tot; }
  }
  __syncthreads();
  const int nin = sFinal;
  const int* list = B.list + o0;
  if (tid == 0) {
    B.inliers[b] = nin; B.iterations[b] = sIt; B.best_draw[b] = sBestD; B.cov_rows[b] = 0; B.cov_draws[b] = 0;
    nc_model_to_T(sBest, B.Tr + 7 * (size_t)b);
  }
  if (nin < B.min_inliers) {
    if (tid == 0) B.status[b] = 3;
    return;
  }

  // ---- the polish: Levenberg-Marquardt on the inliers from the RANSAC model
  if (tid < 12) sPol[tid] = sBest[tid];
  if (tid == 0) { sLambda = 1e-3; sDone = 0; }
  __syncthreads();
  for (int it = 0; it < kNcLmIters; ++it) {
    if (tid < 12) {                                            // thread 2p moves parameter p by +h, thread 2p + 1 by -h
      double d[6] = {0, 0, 0, 0, 0, 0};
      d[tid >> 1] = (tid & 1) ? -kNcLmStep : kNcLmStep;
      nc_retract(sPol, d, sPert + 12 * tid);
    }
    __syncthreads();
    double part[kNcRed];
#pragma unroll
    for (int q = 0; q < kNcRed; ++q) part[q] = 0.0;
    for (int k = tid; k < nin; k += kNcThreads) {
      const NcRay r = S.ray(list[k]);
      double e[6], J[6][6];
      nc_resid(sPol, r, e);
#pragma unroll
      for (int p = 0; p < 6; ++p) {
        double ep[6], em[6];
        nc_resid(sPert + 24 * p, r, ep);
        nc_resid(sPert + 24 * p + 12, r, em);
#pragma unroll
        for (int q = 0; q < 6; ++q) J[q][p] = (ep[q] - em[q]) * (0.5 / kNcLmStep);
      }
      int m = 0;
#pragma unroll
      for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) {
          double s = 0.0;
#pragma unroll
          for (int q = 0; q < 6; ++q) s += J[q][i] * J[q][j];
          part[m++] += s;
        }
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < 6; ++q) s += J[q][i] * e[q];
        part[21 + i] += s;
      }
#pragma unroll
      for (int q = 0; q < 6; ++q) part[27] += e[q] * e[q];
    }
    nc_reduce(part, kNcRed, sRed, sTot, tid);
    if (tid == 0) {                                            // (J^T J + lambda diag) delta = -J^T r by Cholesky
      double Hm[6][6], d[6];
      int m = 0;
      for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) { Hm[i][j] = sTot[m]; Hm[j][i] = sTot[m]; ++m; }
      for (int i = 0; i < 6; ++i) Hm[i][i] += sLambda * Hm[i][i];
      bool pd = true;
      for (int j = 0; j < 6; ++j) {
        double s = Hm[j][j];
        for (int k = 0; k < j; ++k) s -= Hm[j][k] * Hm[j][k];
        if (!(s > 0.0)) { pd = false; s = 1.0; }
        const double dj = sqrt(s);
        Hm[j][j] = dj;
        for (int i = j + 1; i < 6; ++i) {
          double u = Hm[i][j];
          for (int k = 0; k < j; ++k) u -= Hm[i][k] * Hm[j][k];
          Hm[i][j] = u / dj;
        }
      }
      for (int i = 0; i < 6; ++i) { double s = -sTot[21 + i]; for (int k = 0; k < i; ++k) s -= Hm[i][k] * d[k]; d[i] = s / Hm[i][i]; }
      for (int i = 5; i >= 0; --i) { double s = d[i]; for (int k = i + 1; k < 6; ++k) s -= Hm[k][i] * d[k]; d[i] = s / Hm[i][i]; }
      double big = 0.0;
      for (int i = 0; i < 6; ++i) { pd = pd && isfinite(d[i]); big = fmax(big, fabs(d[i])); }
      if (!pd) for (int i = 0; i < 6; ++i) d[i] = 0.0;
      nc_retract(sPol, d, sCand);
      sCost = sTot[27];
      sFinal = pd ? 1 : 0;                                     // the step exists
      sDone = (pd && big < kNcLmTol) || sLambda >= 1e12 ? 1 : 0;
    }
    __syncthreads();
    double c1 = 0.0;
    for (int k = tid; k < nin; k += kNcThreads) {
      double e[6];
      nc_resid(sCand, S.ray(list[k]), e);
#pragma unroll
      for (int q = 0; q < 6; ++q) c1 += e[q] * e[q];
    }
    nc_reduce(&c1, 1, sRed, sTot, tid);
    const bool take = sFinal && sTot[0] < sCost;               // uniform
    if (take && tid < 12) sPol[tid] = sCand[tid];
    if (tid == 0) sLambda = take ? fmax(sLambda * 0.1, 1e-15) : sLambda * 10.0;
    __syncthreads();
    if (sDone) break;
  }
  if (tid == 0) {
    nc_model_to_T(sPol, B.T + 7 * (size_t)b);
    nc_sensor_pose(B.Tq + 7 * (size_t)b, B.Tc + 7 * (size_t)b, sPol, sTs);
    for (int q = 0; q < 7; ++q) B.Ts[7 * (size_t)b + q] = sTs[q];
    sNrows = 0; sNdraws = 0; sDone = 0;
  }
  __syncthreads();

  // ---- the sampled covariance (RelNonCentralPosSolver.cpp:187-292)
  bool thin = false;
  for (int c = 0; c < kNcMaxCells; ++c) if (c < cells && sCellIn[c + 1] - sCellIn[c] < 2 * kNcCovSample) thin = true;
  if (thin) {
    if (tid == 0) B.status[b] = 4;
    return;
  }
  const unsigned long long cseed = nc_splitmix64(seed ^ kNcCovSalt);
  const int N = kNcCovSample * cells, rows = N < kNcCols ? kNcCols : N;
  for (int base = 0; ; base += kNcHyp) {
    const int e = base + g;
    if (l < cells) {                                           // lane j draws cell j's four from its ascending inlier list
      int pick[kNcCovSample];
      const int c0 = sCellIn[l], m = sCellIn[l + 1] - c0;
      nc_draw(pick, cseed + ((unsigned long long)e * (unsigned long long)cells + (unsigned long long)l) * kNcCovSample, kNcCovSample, m);
      for (int k = 0; k < kNcCovSample; ++k) W.idx[kNcCovSample * l + k] = list[c0 + pick[k]];
    }
    __syncthreads();
    for (int r = l; r < rows; r += kNcLanes) {
      double row[kNcCols];
#pragma unroll
      for (int j = 0; j < kNcCols; ++j) row[j] = 0.0;
      if (r < N) nc_row(S.ray(W.idx[r]), row);
#pragma unroll
      for (int j = 0; j < kNcCols; ++j) W.A[j][r] = row[j];
    }
    __syncthreads();
    nc_solve(W, l, rows);
    if (l == 0) sCnt[g] = W.ok ? 0 : -1;
    __syncthreads();
    for (int hh = wave; hh < kNcHyp; hh += kNcThreads / 64) {
      if (sCnt[hh] < 0) continue;
      double R[9];
#pragma unroll
      for (int i = 0; i < 9; ++i) R[i] = sW[hh].H[i];
      const V3 t = v3(sW[hh].H[9], sW[hh].H[10], sW[hh].H[11]);
      int cnt = 0;
      for (int k0 = 0; k0 < nin; k0 += 64) {
        const int k = k0 + lane, kk = k < nin ? k : 0;
        const bool in = k < nin && nc_score(R, t, S.ray(list[kk])) < B.th_cov;
        cnt += __popcll(__ballot(in));
      }
      if (lane == 0) sCnt[hh] = cnt;
    }
    __syncthreads();
    if (tid == 0) {
      int nrows = sNrows, done = 0;
      for (int j = 0; j < kNcHyp; ++j) {
        if (nrows >= B.cov_iters || base + j > B.cov_max_iters) { done = 1; break; }
        sNdraws = base + j + 1;
        const int c = sCnt[j];
        if (c >= 0 && (double)((float)c / (float)nin) > 0.8) {
          double Tt[7];
          nc_sensor_pose(B.Tq + 7 * (size_t)b, B.Tc + 7 * (size_t)b, sW[j].H, Tt);
          const V3 dth = nc_minus(Tt, sTs);
          double* m = sRows + 6 * nrows;
          m[0] = dth.x; m[1] = dth.y; m[2] = dth.z; m[3] = Tt[4]; m[4] = Tt[5]; m[5] = Tt[6];
          ++nrows;
        }
      }
      if (nrows >= B.cov_iters) done = 1;
      sNrows = nrows; sDone = done;
    }
    __syncthreads();
    if (sDone) break;
  }
  const int nrows = sNrows;
  if (tid == 0) { B.cov_rows[b] = nrows; B.cov_draws[b] = sNdraws; }
  if (nrows < B.cov_iters) {
    if (tid == 0) B.status[b] = 5;
    return;
  }
  if (tid < 36) {                                              // about x = (0, 0, 0, t_ref), not the sample mean (:287-292)
    const int i = tid / 6, j = tid % 6;
    const double xi = i < 3 ? 0.0 : sTs[4 + i - 3], xj = j < 3 ? 0.0 : sTs[4 + j - 3];
    double s = 0.0;
    for (int r = 0; r < nrows; ++r) s += (sRows[6 * r + i] - xi) * (sRows[6 * r + j] - xj);
    s /= (double)(nrows - 1);
    B.cov[36 * (size_t)b + tid] = s;
    sPert[tid] = s;
  }
  __syncthreads();
  if (tid == 0) {
    const double tr = ((((sPert[0] + sPert[7]) + sPert[14]) + sPert[21]) + sPert[28]) + sPert[35];
    B.status[b] = tr < B.cov_thres ? 0 : 6;
  }
}

// test entry point: the linear solve alone on N-tuples of ray pairs
__global__ __launch_bounds__(kNcThreads) void k_ncrelpose_solve(int num, int N, const double* ray1, const double* ray2, double* T, int* okout, double* sv) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  NcWork* sW = reinterpret_cast<NcWork*>(sm);
  const int tid = threadIdx.x, g = tid / kNcLanes, l = tid % kNcLanes;
  const int e = blockIdx.x * kNcHyp + g, ee = e < num ? e : num - 1;
  NcWork& W = sW[g];
  const int rows = N < kNcCols ? kNcCols : N;
  for (int r = l; r < rows; r += kNcLanes) {
    double row[kNcCols];
#pragma unroll
    for (int j = 0; j < kNcCols; ++j) row[j] = 0.0;
    if (r < N) {
      const double *a = ray1 + 6 * ((size_t)ee * N + r), *c = ray2 + 6 * ((size_t)ee * N + r);
      NcRay ry;
      ry.g1 = ld3(a); ry.o1 = ld3(a + 3); ry.g2 = ld3(c); ry.o2 = ld3(c + 3);
      nc_row(ry, row);
    }
#pragma unroll
    for (int j = 0; j < kNcCols; ++j) W.A[j][r] = row[j];
  }
  __syncthreads();
  nc_solve(W, l, rows);
  if (e < num && l == 0) {
    okout[e] = W.ok;
    for (int q = 0; q < 3; ++q) sv[3 * (size_t)e + q] = W.sv[q];
    if (W.ok) nc_model_to_T(W.H, T + 7 * (size_t)e);
  }
}

}  // namespace

static size_t ncrelpose_lds_bytes(int cap, bool solve_only) {
  size_t d = sizeof(NcWork) * kNcHyp;
  if (!solve_only) d += sizeof(double) * (12 + 12 + 12 + 144 + 4 * kNcRed + kNcRed + 6 * kNcMaxCovRows + 12 * (size_t)(cap > 0 ? cap : 0));
  return d;
}

void ncrelpose_limits(int out[8]) {
  out[0] = kNcStageCap; out[1] = kNcHyp; out[2] = kNcSample; out[3] = kNcMaxIterations; out[4] = kNcMaxCells; out[5] = kNcMaxCovRows;
  out[6] = kNcMaxRows; out[7] = kNcLmIters;
}

hipError_t launch_ncrelpose(const NcRelposeArgs& a, hipStream_t st) {
  if (a.num <= 0) return hipSuccess;
  int cap = a.stage_cap > 0 && a.stage_cap < kNcStageCap ? a.stage_cap : kNcStageCap;
  if (a.max_n < cap) cap = a.max_n > 0 ? a.max_n : 1;
  const size_t lds = ncrelpose_lds_bytes(cap, false);
  if (const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_ncrelpose), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) return e;
  NcBatch B{a.num, a.cells, a.ptr, a.cell, a.f1, a.f2, a.cam1, a.cam2, a.cam_ptr, a.cam, a.Tq, a.Tc, a.seed, a.T, a.Tr, a.Ts, a.cov, a.inlier, a.list,
            a.inliers, a.status, a.iterations, a.best_draw, a.cov_rows, a.cov_draws, a.min_inliers, a.max_iterations, a.cov_iters, a.cov_max_iters,
            a.probability, a.threshold, a.th_cov, a.cov_thres};
  hipLaunchKernelGGL(k_ncrelpose, dim3(a.num), dim3(kNcThreads), lds, st, B, cap);
  return hipGetLastError();
}

hipError_t launch_ncrelpose_solve(int num, int N, const double* ray1, const double* ray2, double* T, int* ok, double* sv, hipStream_t st) {
  if (num <= 0) return hipSuccess;
  const size_t lds = ncrelpose_lds_bytes(0, true);
  if (const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_ncrelpose_solve), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) return e;
  hipLaunchKernelGGL(k_ncrelpose_solve, dim3((num + kNcHyp - 1) / kNcHyp), dim3(kNcThreads), lds, st, num, N, ray1, ray2, T, ok, sv);
  return hipGetLastError();
}

}  // namespace covgpu
