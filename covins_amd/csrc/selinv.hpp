// selinv.hpp — what the top-down sweep of the selected inverse (k_selinv.hip) and its host side (selinv.hip) share: the per-call tables.
#pragma once
#include "common.hpp"
#include "selinv_check.hpp"

namespace covgpu {

// One front. Sigma's square and the temporaries W = L_OO^-1 / T = L_BO W live in two scratch buffers laid out like nd_M: the same element
// offset and leading dimension, own rows first, border rows from nI on (W over L_OO, T over L_BO).
struct SelFront {
  long long moff, linv, pmoff;   // element offset of the front | of its block inverses in nd_Linv | of its ancestor's front (-1: a root)
  int ld, nI, own, st;           // leading dimension | padded interior order of its level (where the border rows start) | own | border unknowns
  int nbo, pld;                  // 16-row blocks of its own unknowns | the ancestor's leading dimension
  int gmap, pad;                 // first entry of its border rows' map (border scalar -> row of the ancestor's square)
};
// One workgroup of a step: x = front, y = kind (0 gather | 1 W | 2 T | 3 Sigma_BO | 4 Sigma_OO | 5 the whole front in the vector form),
// z = 16-row block (kind 1: group of four 16-column chunks), w = panel of 128 own columns
struct SelArgs {
  const double *M, *Linv;
  double *S, *X;
  const SelFront* fr; const int* gmap; const int4* items;
};
void launch_selinv_gather(const SelArgs& a, int item0, int count, hipStream_t st);
void launch_selinv_step(const SelArgs& a, int item0, int count, int kind, hipStream_t st);
void launch_selinv_read(const double* S, const long long* src, double* out, long long n, hipStream_t st);

}  // namespace covgpu
