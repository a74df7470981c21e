// Diversified re-ranking: k of a list's candidates chosen one after the other by
// Maximal Marginal Relevance.  The picks of a list are sequential, the lists are parallel: one
// workgroup per list, the candidates' base value, largest similarity so far and item id in LDS, the
// chosen item's row staged in LDS, every remaining candidate's row read once per step.  The
// arithmetic is the one include/rfm_diverse.h states, operation by operation; the whole file is
// compiled without contraction, so that a product and the sum it enters stay two roundings.
#include <cmath>

#include "rfm_common.h"

#pragma clang fp contract(off)

namespace rfm {
namespace {

constexpr int kDivBlock = 256;                 // 4 wavefronts
constexpr int kDivWaves = kDivBlock / 64;
constexpr int kDivMaxDepth = 1024;             // candidates of a list
constexpr int kDivMaxK = 64;                   // picks of a list: recommend.MAX_K
constexpr int kDivUnroll = 4;                  // candidates a wavefront has in flight
// s_base, s_m, s_row (doubles), s_item (ints), the four wavefronts' picks
constexpr int64_t kDivLdsBytes = int64_t(2 * kDivMaxDepth + RFM_MAX_FACTORS) * 8 + kDivMaxDepth * 4 + kDivWaves * 16;
constexpr int kDivPerCu = 5;                   // workgroups of a CU: 5 x 28.7 KB of its 160 KB
static_assert(kDivPerCu * kDivLdsBytes <= (160 << 10), "the grid's workgroups of a CU do not fit its LDS");

struct DiverseArgs {
  const int32_t* cand_items;
  const double* cand_scores;
  int64_t n_lists, ld_c;
  const double* R;
  int64_t n_items, ld_R;
  const double* penalty;
  double lambda;
  int depth, n_factors, k;
  int32_t* out_items;
  double* out_scores;
  double* out_values;
  int32_t* out_pos;
};

// a step's candidate for the pick: pos < 0 is none
struct Pick {
  double v;
  int item, pos;
};

// The order of the rfm_pair_* entries (value descending, then item id descending; rfm_pairs.hip's
// better(), repeated here so that its translation unit stays as it is), then the lower position.
__device__ inline bool pick_wins(const Pick& a, const Pick& b) {
  if (a.pos < 0) return false;
  if (b.pos < 0) return true;
  return a.v > b.v || (a.v == b.v && (a.item > b.item || (a.item == b.item && a.pos < b.pos)));
}

__global__ __launch_bounds__(kDivBlock) void diverse_select_kernel(DiverseArgs a) {
  __shared__ double s_base[kDivMaxDepth];
  __shared__ double s_m[kDivMaxDepth];
  __shared__ double s_row[RFM_MAX_FACTORS];
  __shared__ int s_item[kDivMaxDepth];  // -1: chosen, or never eligible
  __shared__ double s_pick_v[kDivWaves];
  __shared__ int s_pick_item[kDivWaves], s_pick_pos[kDivWaves];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const double rest = 1.0 - a.lambda;
  for (int64_t list = blockIdx.x; list < a.n_lists; list += gridDim.x) {
    __syncthreads();  // (the list before this one is done with the LDS)
    const int32_t* __restrict__ ci = a.cand_items + list * a.ld_c;
    const double* __restrict__ cs = a.cand_scores + list * a.ld_c;
    for (int c = tid; c < a.depth; c += kDivBlock) {
      const int item = ci[c];
      const double p = cs[c];
      const bool ok = item >= 0 && int64_t(item) < a.n_items && p == p;
      double base = a.lambda * p;
      if (ok && a.penalty) base = base - a.penalty[item];
      s_base[c] = base;
      s_m[c] = -INFINITY;
      s_item[c] = ok ? item : -1;
    }
    // (step 0's value pass reads what its own thread wrote above: no barrier before it)
    int32_t* __restrict__ o_items = a.out_items + list * a.k;
    double* __restrict__ o_scores = a.out_scores + list * a.k;
    double* __restrict__ o_values = a.out_values + list * a.k;
    int32_t* __restrict__ o_pos = a.out_pos + list * a.k;
    int filled = 0;
    for (int t = 0; t < a.k; ++t) {
      // the value pass: every thread's best eligible candidate, positions ascending
      Pick best{0.0, -1, -1};
      for (int c = tid; c < a.depth; c += kDivBlock) {
        const int item = s_item[c];
        double v = s_base[c];
        if (t > 0) {
          const double w = rest * s_m[c];
          v = v - w;
        }
        const Pick cand{v, item, (item >= 0 && v == v) ? c : -1};
        if (pick_wins(cand, best)) best = cand;
      }
      for (int m = 32; m >= 1; m >>= 1) {
        const Pick o{__shfl_xor(best.v, m, 64), __shfl_xor(best.item, m, 64), __shfl_xor(best.pos, m, 64)};
        if (pick_wins(o, best)) best = o;
      }
      if (lane == 0) {
        s_pick_v[wave] = best.v;
        s_pick_item[wave] = best.item;
        s_pick_pos[wave] = best.pos;
      }
      __syncthreads();
      best = Pick{s_pick_v[0], s_pick_item[0], s_pick_pos[0]};
      for (int w = 1; w < kDivWaves; ++w) {
        const Pick o{s_pick_v[w], s_pick_item[w], s_pick_pos[w]};
        if (pick_wins(o, best)) best = o;
      }
      if (best.pos < 0) break;  // (every thread holds the same pick)
      filled = t + 1;
      if (tid == 0) {
        o_items[t] = best.item;
        o_scores[t] = cs[best.pos];
        o_values[t] = best.v;
        o_pos[t] = best.pos;
        s_item[best.pos] = -1;
      }
      if (filled == a.k) break;
      // the chosen row, then every remaining candidate's similarity to it
      const double* __restrict__ rj = a.R + int64_t(best.item) * a.ld_R;
      for (int f = tid; f < a.n_factors; f += kDivBlock) s_row[f] = rj[f];
      __syncthreads();
      for (int c0 = wave; c0 < a.depth; c0 += kDivWaves * kDivUnroll) {
        int item[kDivUnroll];
        const double* __restrict__ row[kDivUnroll];
        double s[kDivUnroll];
        bool any = false;
#pragma unroll
        for (int u = 0; u < kDivUnroll; ++u) {
          const int c = c0 + u * kDivWaves;
          item[u] = __builtin_amdgcn_readfirstlane(c < a.depth ? s_item[c] : -1);
          any = any || item[u] >= 0;
          row[u] = a.R + int64_t(item[u] >= 0 ? item[u] : 0) * a.ld_R;  // (row 0: read and not used)
          s[u] = 0.0;
        }
        if (!any) continue;
        for (int f = lane; f < a.n_factors; f += 64) {
          const double y = s_row[f];
#pragma unroll
          for (int u = 0; u < kDivUnroll; ++u) {
            const double x = row[u][f];
            const double xy = x * y;
            s[u] = s[u] + xy;
          }
        }
#pragma unroll
        for (int u = 0; u < kDivUnroll; ++u) {
          for (int m = 32; m >= 1; m >>= 1) s[u] = s[u] + __shfl_xor(s[u], m, 64);
          if (lane == 0 && item[u] >= 0) {
            const int c = c0 + u * kDivWaves;
            const double sim = s[u] == s[u] ? s[u] : 0.0;
            const double m = s_m[c];
            s_m[c] = sim > m ? sim : m;
          }
        }
      }
      __syncthreads();
    }
    for (int r = filled + tid; r < a.k; r += kDivBlock) {
      o_items[r] = -1;
      o_scores[r] = NAN;
      o_values[r] = NAN;
      o_pos[r] = -1;
    }
  }
}

void check_shape(int64_t n_lists, int32_t depth, int32_t n_factors, int64_t ld_R, int32_t k) {
  RFM_REQUIRE(n_lists >= 0 && n_lists < (int64_t(1) << 40), "n_lists=%lld", (long long)n_lists);
  RFM_REQUIRE(depth >= 1 && depth <= kDivMaxDepth, "depth=%d outside 1..%d", depth, kDivMaxDepth);
  RFM_REQUIRE(n_factors >= 1 && n_factors <= RFM_MAX_FACTORS, "n_factors=%d unsupported (1..%d)", n_factors,
              RFM_MAX_FACTORS);
  RFM_REQUIRE(ld_R >= n_factors && ld_R < (int64_t(1) << 20), "ld_R=%lld for %d factors", (long long)ld_R, n_factors);
  RFM_REQUIRE(k >= 1 && k <= kDivMaxK, "k=%d outside 1..%d", k, kDivMaxK);
}

int64_t diverse_grid(const rfm_ctx* ctx, int64_t n_lists) {
  const int64_t n_cu = ctx ? ctx->n_cu : 256;
  return std::max<int64_t>(1, std::min<int64_t>(n_lists, n_cu * kDivPerCu));
}

}  // namespace
}  // namespace rfm

using namespace rfm;

extern "C" {

int32_t rfm_diverse_select(rfm_ctx* ctx, const int32_t* d_cand_items, const double* d_cand_scores, int64_t n_lists,
                           int32_t depth, int64_t ld_c, const double* d_R, int64_t n_items, int32_t n_factors,
                           int64_t ld_R, const double* d_penalty, double trade_off, int32_t k, int32_t* d_out_items,
                           double* d_out_scores, double* d_out_values, int32_t* d_out_pos) {
  return guarded([&] {
    RFM_REQUIRE(ctx && d_cand_items && d_cand_scores && d_R && d_out_items && d_out_scores && d_out_values && d_out_pos,
                "null pointer");
    check_shape(n_lists, depth, n_factors, ld_R, k);
    RFM_REQUIRE(ld_c >= depth && ld_c < (int64_t(1) << 31), "ld_c=%lld for depth %d", (long long)ld_c, depth);
    RFM_REQUIRE(n_items >= 1 && n_items < (int64_t(1) << 31), "n_items=%lld: none, or too many for int32 item ids",
                (long long)n_items);
    RFM_REQUIRE(trade_off >= 0.0 && trade_off <= 1.0, "trade_off=%g outside [0, 1]", trade_off);  // (false for a NaN)
    if (n_lists == 0) return;
    RFM_HIP_CHECK(hipSetDevice(ctx->device));
    const DiverseArgs a{d_cand_items, d_cand_scores, n_lists, ld_c, d_R, n_items, ld_R, d_penalty, trade_off,
                        depth, n_factors, k, d_out_items, d_out_scores, d_out_values, d_out_pos};
    hipLaunchKernelGGL(diverse_select_kernel, dim3((unsigned)diverse_grid(ctx, n_lists)), dim3(kDivBlock), 0,
                       ctx->stream, a);
    RFM_HIP_CHECK(hipGetLastError());
  });
}

int32_t rfm_diverse_geometry(const rfm_ctx* ctx, int64_t n_lists, int32_t depth, int32_t n_factors, int64_t ld_R,
                             int32_t k, int64_t* h_out6) {
  return guarded([&] {
    RFM_REQUIRE(h_out6, "null pointer");
    check_shape(n_lists, depth, n_factors, ld_R, k);
    const int64_t grid = diverse_grid(ctx, n_lists);
    h_out6[0] = 0;
    h_out6[1] = n_lists ? grid : 0;
    h_out6[2] = (n_lists + grid - 1) / grid;
    h_out6[3] = (depth + kDivBlock - 1) / kDivBlock;
    h_out6[4] = kDivLdsBytes;
    h_out6[5] = (n_factors + 63) / 64;
  });
}

}  // extern "C"
