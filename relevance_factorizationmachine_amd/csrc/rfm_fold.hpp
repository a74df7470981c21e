// What the two fold-in launches share (rfm_mf_fold_in in rfm_mf.hip, rfm_fm_fold_in in
// rfm_fm_fold.hip): the grouped examples of the new rows as the kernels see
// them, an example on its way to a lane group, the argument checks both entries open with, and the
// part of the launch shape both geometry entries report.  The kernels themselves are different
// algorithms and stay in their files.
#pragma once

#include "rfm_common.h"

namespace rfm {

constexpr int kFoldPerCu = 8;  // workgroups per CU of the capped grid, as the other MF launches

// the leading members of MfFoldArgs and FmFoldArgs
struct FoldExamples {
  const int64_t* row_ptr;  // [n_new + 1]: examples of new row r are row_ptr[r] .. row_ptr[r + 1]
  const int32_t* ids;      // fixed-side row of every example, in the row's own order
  const double* ry;        // label / propensity of every example
  const int32_t* order;    // [n_new]: new rows by descending example count
  int64_t n_new;
};

// An example on its way: fixed row, weight, and whether the lane group has it.  A group past its
// examples gets {0, 0.0, false}: row 0 of the fixed side, a valid address.  Each kernel spells that
// predicated read itself (fold_fetch_id, fold_fetch_ex).  One shared function was built and measured
// (profiles/n17/fold_in_timing_parent_vs_this.txt): inlined, it leaves the compiler one of two forms
// of the address x.ids + e0 + e, MF's chain is 2 % slower at k = 32 with the one and FM's launch 3 %
// slower at k = 400 with the other.
struct FoldEx {
  int32_t j;
  double ry;
  bool live;
};

// the checks both entries make first, in this order; the entry checks its own pointers next
inline FoldExamples fold_checked(const rfm_ctx* ctx, const int64_t* d_row_ptr, const int32_t* d_ids,
                                 const double* d_ry, const int32_t* d_order, int64_t n_new, int64_t n_fixed,
                                 int32_t n_factors, int32_t n_passes, Shape* shape) {
  RFM_REQUIRE(ctx, "null ctx");
  RFM_REQUIRE(n_new >= 0 && n_new < (int64_t(1) << 31), "n_new=%lld out of range", (long long)n_new);
  RFM_REQUIRE(n_fixed >= 0 && n_fixed < (int64_t(1) << 31), "n_fixed=%lld out of range", (long long)n_fixed);
  RFM_REQUIRE(n_passes >= 0, "negative n_passes");
  *shape = shape_for(n_factors);
  return FoldExamples{d_row_ptr, d_ids, d_ry, d_order, n_new};
}

// out[0..3] of both geometry entries: lanes per row, adjacent factors a lane owns per chunk, chunks
// per lane, lane groups per workgroup of `block` threads
inline void fold_shape_out(const Shape& s, int block, int32_t* out) {
  out[0] = s.lpr;
  out[1] = s.vec;
  out[2] = s.nc;
  out[3] = block / s.lpr;
}

}  // namespace rfm
