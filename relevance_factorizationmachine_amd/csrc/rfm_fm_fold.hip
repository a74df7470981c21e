// FM fold-in on gfx950 (rfm_fm_fold_in, fm_fold_kernel): the one-hot id column of
// a user or item that arrived after the fit is trained against the fixed other side by the
// reference's batch-sum step (src/fm.py:80-88, 135-187) restricted to that column, on the dense
// operands of the catalogue layer (rfm_fm_side_sums): the new row's own feature sums g_r, l_r and
// the fixed side F, fL.
//
//  * ONE WORKGROUP PER NEW ROW (grid-stride over the order array).  Within a pass the examples of a
//    row are independent -- every error is taken before the update -- so the GPB = 256 / LPR lane
//    groups of the factor count's shape class take examples grp, grp + GPB, ... of the row.
//  * A lane group keeps its own copy of nu_r, omega_r and g_r and its partial sums of err * h and
//    err in registers.  The row F[j_e] is loaded once and serves both dot products and the sum.
//    The id / weight of the example two trips ahead and the row of the next trip are in flight
//    while a trip computes.
//  * Every lane group makes the same number of trips (the row's example count is uniform over the
//    workgroup), so the cross-lane sums and the barriers run converged; a group past the row's
//    last example reads row 0 of the fixed side and adds nothing.
//  * End of pass: the partial sums go to LDS (at most GPB x LPR x VEC x NC = 4 096 doubles, 32 KB,
//    plus GPB sums of err), one barrier, then EVERY group adds the partials in group order
//    0 .. GPB-1 and applies the update to its own copy: the copies stay identical bit for bit, and
//    nothing depends on timing.  A second barrier frees the LDS for the next pass or row.
//  * No atomics, plain loads and plain vector stores only.
// The example layout and the entry's first checks are MF fold-in's too: rfm_fold.hpp.
#include <algorithm>

#include "rfm_common.h"
#include "rfm_device_utils.hpp"
#include "rfm_fold.hpp"

namespace rfm {

constexpr int kFmFoldBlock = 256;

struct FmFoldArgs : FoldExamples {
  const double* g;   // [n_new][kpad]: the new rows' feature sums
  const double* l;   // [n_new]
  const double* F;   // [n_fixed][kpad]: the fixed side (B, LI for new users; A, LU for new items)
  const double* fL;  // [n_fixed]
  const double* c;   // *w0
  int32_t k, kpad;
  double lr;
  int32_t n_passes;
  double* w_new;  // [n_new] in / out
  double* V_new;  // [n_new][k] in / out
  double* A_new;  // [n_new][kpad] out
  double* L_new;  // [n_new] out
};

// factors f = (ch * LPR + l) * VEC + v of a row of `k` factors; zeros past k
template <int LPR, int VEC, int NC>
__device__ __forceinline__ void fold_load(Pack<VEC> (&dst)[NC], const double* row, int k, int l) {
#pragma unroll
  for (int ch = 0; ch < NC; ++ch) {
    const int f = (ch * LPR + l) * VEC;
    if (f < k) {
      dst[ch].load(row + f);
    } else {
#pragma unroll
      for (int v = 0; v < VEC; ++v) dst[ch].v[v] = 0.0;
    }
  }
}

template <int LPR, int VEC, int NC>
__device__ __forceinline__ void fold_store(const Pack<VEC> (&src)[NC], double* row, int k, int l) {
#pragma unroll
  for (int ch = 0; ch < NC; ++ch) {
    const int f = (ch * LPR + l) * VEC;
    if (f < k) src[ch].store(row + f);
  }
}

__device__ __forceinline__ FoldEx fold_fetch_ex(const FmFoldArgs& a, int64_t e0, int64_t n, int64_t e) {
  FoldEx x;
  x.live = e < n;
  x.j = 0;  // past the row's examples: row 0 of the fixed side, a valid address
  x.ry = 0.0;
  if (x.live) {
    x.j = a.ids[e0 + e];
    x.ry = a.ry[e0 + e];
  }
  return x;
}

template <int LPR, int VEC, int NC>
__global__ __launch_bounds__(kFmFoldBlock) void fm_fold_kernel(FmFoldArgs a) {
  constexpr int GPB = kFmFoldBlock / LPR;
  constexpr int SLOTS = LPR * VEC * NC;  // factors a lane group holds (>= kpad)
  __shared__ __attribute__((aligned(16))) double s_sum[GPB * SLOTS];  // [grp][ch][l][v]
  __shared__ double s_err[GPB];
  const int l = threadIdx.x % LPR;
  const int grp = threadIdx.x / LPR;
  const int k = a.k, kpad = a.kpad;
  const double c = *a.c;
  for (int64_t at = blockIdx.x; at < a.n_new; at += gridDim.x) {
    const int64_t r = a.order[at];
    const int64_t e0 = a.row_ptr[r];
    const int64_t n = a.row_ptr[r + 1] - e0;
    Pack<VEC> g[NC], nu[NC];
    fold_load<LPR, VEC, NC>(g, a.g + r * kpad, k, l);
    fold_load<LPR, VEC, NC>(nu, a.V_new + r * k, k, l);
    double omega = a.w_new[r];
    const double base = c + a.l[r];
    const int64_t trips = (n + GPB - 1) / GPB;  // the same for every lane group
    const int live_groups = n < GPB ? int(n) : GPB;
    for (int p = 0; p < a.n_passes && n > 0; ++p) {
      Pack<VEC> sum[NC];
#pragma unroll
      for (int ch = 0; ch < NC; ++ch) {
#pragma unroll
        for (int v = 0; v < VEC; ++v) sum[ch].v[v] = 0.0;
      }
      double sum_err = 0.0;
      FoldEx cur = fold_fetch_ex(a, e0, n, grp);
      Pack<VEC> row[NC];
      fold_load<LPR, VEC, NC>(row, a.F + int64_t(cur.j) * kpad, k, l);
      double fl = a.fL[cur.j];
      FoldEx nxt = fold_fetch_ex(a, e0, n, int64_t(grp) + GPB);
      for (int64_t t = 0; t < trips; ++t) {
        // the next trip's row and the id of the trip after it leave before this trip computes
        Pack<VEC> row_nxt[NC];
        fold_load<LPR, VEC, NC>(row_nxt, a.F + int64_t(nxt.j) * kpad, k, l);
        const double fl_nxt = a.fL[nxt.j];
        const FoldEx far = fold_fetch_ex(a, e0, n, (t + 2) * GPB + grp);
        // z = c + l_r + fL[j] + g.F[j] + omega + nu.h, h = g + F[j]: one sum over the factors
        double dot = 0.0;
#pragma unroll
        for (int ch = 0; ch < NC; ++ch) {
#pragma unroll
          for (int v = 0; v < VEC; ++v)
            dot += g[ch].v[v] * row[ch].v[v] + nu[ch].v[v] * (g[ch].v[v] + row[ch].v[v]);
        }
        dot = group_sum<LPR>(dot);
        const double err = cur.ry - sigmoid_clipped(base + fl + omega + dot);
#pragma unroll
        for (int ch = 0; ch < NC; ++ch) {
#pragma unroll
          for (int v = 0; v < VEC; ++v) {
            const double s_new = sum[ch].v[v] + err * (g[ch].v[v] + row[ch].v[v]);
            sum[ch].v[v] = cur.live ? s_new : sum[ch].v[v];
          }
        }
        sum_err = cur.live ? sum_err + err : sum_err;
        cur = nxt;
        nxt = far;
        fl = fl_nxt;
#pragma unroll
        for (int ch = 0; ch < NC; ++ch) row[ch] = row_nxt[ch];
      }
      // the groups' partial sums, added by every group in group order
#pragma unroll
      for (int ch = 0; ch < NC; ++ch) sum[ch].store(&s_sum[((grp * NC + ch) * LPR + l) * VEC]);
      if (l == 0) s_err[grp] = sum_err;
      __syncthreads();
      Pack<VEC> tot[NC];
#pragma unroll
      for (int ch = 0; ch < NC; ++ch) tot[ch].load(&s_sum[(ch * LPR + l) * VEC]);
      double tot_err = s_err[0];
      for (int q = 1; q < live_groups; ++q) {
#pragma unroll
        for (int ch = 0; ch < NC; ++ch) {
          Pack<VEC> part;
          part.load(&s_sum[((q * NC + ch) * LPR + l) * VEC]);
#pragma unroll
          for (int v = 0; v < VEC; ++v) tot[ch].v[v] += part.v[v];
        }
        tot_err += s_err[q];
      }
#pragma unroll
      for (int ch = 0; ch < NC; ++ch) {
#pragma unroll
        for (int v = 0; v < VEC; ++v) nu[ch].v[v] += a.lr * tot[ch].v[v];
      }
      omega += a.lr * tot_err;
      __syncthreads();  // (the next pass, or the next row, writes the same LDS)
    }
    // the served operands of the grown row: A = g + nu (zeros past k), L = l + omega + g . nu
    double gnu = 0.0;
    Pack<VEC> served[NC];
#pragma unroll
    for (int ch = 0; ch < NC; ++ch) {
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        served[ch].v[v] = g[ch].v[v] + nu[ch].v[v];
        gnu += g[ch].v[v] * nu[ch].v[v];
      }
    }
    gnu = group_sum<LPR>(gnu);
    if (grp == 0) {
      fold_store<LPR, VEC, NC>(served, a.A_new + r * kpad, kpad, l);
      if (l == 0) a.L_new[r] = a.l[r] + omega + gnu;
      if (n > 0 && a.n_passes > 0) {  // (else the column keeps its bits)
        fold_store<LPR, VEC, NC>(nu, a.V_new + r * k, k, l);
        if (l == 0) a.w_new[r] = omega;
      }
    }
  }
}

}  // namespace rfm

using namespace rfm;

extern "C" {

int32_t rfm_fm_fold_geometry(const rfm_ctx* ctx, int64_t n_new, int32_t n_factors, int32_t* h_out5) {
  return guarded([&] {
    RFM_REQUIRE(h_out5, "null pointer");
    RFM_REQUIRE(n_new >= 0 && n_new < (int64_t(1) << 31), "n_new=%lld out of range", (long long)n_new);
    const Shape s = shape_for(n_factors);
    const rfm_ctx assumed{};  // (the CU count of an MI355X)
    fold_shape_out(s, kFmFoldBlock, h_out5);
    h_out5[4] = capped_grid(ctx ? ctx : &assumed, n_new, 1, kFoldPerCu, 0);
  });
}

int32_t rfm_fm_fold_in(rfm_ctx* ctx, const int64_t* d_row_ptr, const int32_t* d_ids, const double* d_ry,
                       const int32_t* d_order, int64_t n_new, const double* d_g, const double* d_l,
                       const double* d_F, const double* d_fL, int64_t n_fixed, const double* d_c,
                       int32_t n_factors, double lr, int32_t n_passes, double* d_w_new, double* d_V_new,
                       double* d_A_new, double* d_L_new) {
  return guarded([&] {
    Shape s;
    const FoldExamples x = fold_checked(ctx, d_row_ptr, d_ids, d_ry, d_order, n_new, n_fixed, n_factors, n_passes, &s);
    RFM_REQUIRE(d_row_ptr && d_ids && d_ry && d_order && d_g && d_l && d_F && d_fL && d_c && d_w_new && d_V_new &&
                    d_A_new && d_L_new,
                "null pointer");
    if (n_new == 0) return;
    // (a lane group past the row's examples reads row 0 of the fixed side)
    RFM_REQUIRE(n_fixed >= 1, "a fixed side without rows");
    RFM_HIP_CHECK(hipSetDevice(ctx->device));
    FmFoldArgs a{x};
    a.g = d_g;
    a.l = d_l;
    a.F = d_F;
    a.fL = d_fL;
    a.c = d_c;
    a.k = n_factors;
    a.kpad = (n_factors + 3) / 4 * 4;
    a.lr = lr;
    a.n_passes = n_passes;
    a.w_new = d_w_new;
    a.V_new = d_V_new;
    a.A_new = d_A_new;
    a.L_new = d_L_new;
    const int grid = capped_grid(ctx, n_new, 1, kFoldPerCu, 0);
#define RFM_CALL_FM_FOLD(L, Vv, N) \
  hipLaunchKernelGGL((fm_fold_kernel<L, Vv, N>), dim3(grid), dim3(kFmFoldBlock), 0, ctx->stream, a)
    RFM_FOR_SHAPE(s, RFM_CALL_FM_FOLD);
#undef RFM_CALL_FM_FOLD
    RFM_HIP_CHECK(hipGetLastError());
  });
}

}  // extern "C"
