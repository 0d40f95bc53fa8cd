// leaf_front.hpp — the one-launch leaf form of the panel factorisation (k_panel.hip: k_potrf_leaf): which fronts it takes, and where the
// 16-row blocks of its working set lie in a front. Plain integer arithmetic shared by the host tables (nd_tables.hip) and the kernel; no HIP call,
// so a stand-alone host program can include it as it is.
//
// The form factors a front's own columns and leaves its Schur complement in ONE workgroup whose working set is the whole front: logical 16-blocks
// 0 .. nbo-1 are the front's own blocks (nbo = ceil(own / 16)), the border blocks follow them at once. In memory the border starts behind the
// level's padded interior (NdLevel::nI), so logical row r >= 16 nbo lies `nI - 16 nbo` rows further down.
#pragma once

#if defined(__HIPCC__)
#define COV_LEAF_HD __host__ __device__ __forceinline__
#else
#define COV_LEAF_HD inline
#endif

namespace covgpu {

constexpr int kLeafBlock = 16;          // block edge of the panel kernel (PB)
constexpr int kLeafRows = 256;          // rows of its working set (PROWS)
constexpr int kLeafMaxFronts = 384;     // levels of more fronts take the four-wave form (launch_potrf_panel: kSmallMin)

COV_LEAF_HD int leaf_blocks(int order) { return (order + kLeafBlock - 1) / kLeafBlock; }
// a front of `own` own and `st` border unknowns fits the form: every own column in the first eight blocks, the whole front in sixteen
COV_LEAF_HD bool leaf_front_fits(int own, int st) {
  return own >= 1 && st >= 0 && own <= kLeafRows / 2 && st <= kLeafRows / 2 && own + st <= kLeafRows &&
         leaf_blocks(own) + leaf_blocks(st) <= kLeafRows / kLeafBlock;
}
// rows between a border row's logical and physical position, for a front of nbo own blocks in a level of padded interior order nI
COV_LEAF_HD int leaf_border_shift(int nbo, int nI) { return nI - kLeafBlock * nbo; }
// physical row (= column) of logical row r: own rows stay, border rows (r >= nown = 16 nbo) move by the shift
COV_LEAF_HD int leaf_phys_row(int r, int nown, int bshift) { return r >= nown ? r + bshift : r; }

// A level is taken by the form when it has 1 .. kLeafMaxFronts fronts, every front fits, and every own variable of every front is a speed-bias
// block (odd variable index: DevProblem's numbering, 2 pos + 1): only then is everything the fronts hold final before the pose system is.
// own_dim / st_dim: [n] scalar sizes; own_ptr / own_var: CSR of the fronts' own variables.
inline bool leaf_level_eligible(int n, const int* own_dim, const int* st_dim, const int* own_ptr, const int* own_var) {
  if (n < 1 || n > kLeafMaxFronts) return false;
  for (int k = 0; k < n; ++k) {
    if (!leaf_front_fits(own_dim[k], st_dim[k])) return false;
    for (int q = own_ptr[k]; q < own_ptr[k + 1]; ++q) if ((own_var[q] & 1) == 0) return false;
  }
  return true;
}

}  // namespace covgpu
