// Logistic-MF kernels for gfx950 and their C-ABI launchers.
//
// Layout in HBM: P[n_users][k], Q[n_items][k] row-major f64 (the reference's
// NumPy layout), b_u[n_users], b_i[n_items]; the (user, item) pairs of the log
// are two int32 arrays.  A pair is handled by LPR consecutive lanes (same
// factor-to-lane map as the FM kernels): k=128 -> 64 lanes x 16 bytes.
//
// Training keeps the reference's strictly sequential per-example semantics
// (src/mf.py:97-108) through the level schedule of rfm_mf_schedule: examples
// of one level touch disjoint rows of P, Q, b_u, b_i.  Levels with many
// examples get a grid-wide launch each; runs of small levels are executed by
// ONE workgroup that walks the levels with a barrier in between, so a batch
// whose popular item forms a long chain costs one launch, not one per level.
//
// The schedule comes in two forms: the plain form (an order of batch positions,
// rfm_mf_sgd_levels; rfm_mf_sgd_hogwild is its wide kernel on the whole batch)
// and the record form the fits use (level-ordered MfEx records, an item cache
// and a read-ahead ring in the sequential kernel, rfm_mf_sgd_levels_ex).  Both
// run the same example update (mf_load_row, mf_update, mf_store_row), the same
// host walk over the level pointers (mf_walk_levels) and fill the model's
// fields of their argument blocks in one place (set_model).
//
// Several models on one schedule (rfm_mf_sgd_levels_many, rfm_mf_predict_many / _loss_many): models
// fitted on one log with one batch size share the schedule, so the record form's kernels and the
// scoring kernels exist a second time with a model dimension.  Their bodies are the single-model
// kernels' (mf_seq_ex_body, mf_wide_ex_body, mf_predict_body, mf_loss_finish_body), run on an
// argument block the workgroup fills from its model's row of a device table (rfm_mf_model).
//
// Fold-in (rfm_mf_fold_in, mf_fold_kernel) trains new rows of one side against the fixed
// other side by the same update restricted to that side: independent chains, one lane group
// per new row, no schedule.  What it shares with FM fold-in is in rfm_fold.hpp.
#include <algorithm>
#include <cmath>
#include <cstddef>

#include "rfm_common.h"
#include "rfm_device_utils.hpp"
#include "rfm_fold.hpp"
#include "rfm_rule.hpp"

namespace rfm {

constexpr int kMfBlock = 256;
constexpr int kSeqBlock = 1024;  // threads of the sequential workgroup
struct MfPredArgs {
  const int32_t* users;
  const int32_t* items;
  const int32_t* row_ids;  // nullable
  int64_t n_rows;
  const double* P;
  const double* Q;
  const double* bu;
  const double* bi;
  double b;
  int32_t k;
  const double* y;
  const double* pscore;
  double* out_pred;      // nullable
  double* loss_partial;  // nullable
  double eps;
};

// (the body of mf_predict_kernel and of mf_predict_many_kernel: blockIdx.x / gridDim.x walk the rows)
template <int LPR, int VEC, int NC>
__device__ __forceinline__ void mf_predict_body(const MfPredArgs& a) {
  constexpr int GPB = kMfBlock / LPR;
  __shared__ double lds[kMfBlock];
  const int tid = threadIdx.x;
  const int l = tid % LPR;
  const int g = tid / LPR;
  const int k = a.k;
  double loss_acc = 0.0;
  for (int64_t base = int64_t(blockIdx.x) * GPB; base < a.n_rows;
       base += int64_t(gridDim.x) * GPB) {
    const int64_t t = base + g;
    const bool valid = t < a.n_rows;
    int64_t r = 0;
    int32_t u = 0, i = 0;
    if (valid) {
      r = a.row_ids ? int64_t(a.row_ids[t]) : t;
      u = a.users[r];
      i = a.items[r];
    }
    double dot = 0.0;
    if (valid) {
      const double* pu = a.P + int64_t(u) * k;
      const double* qi = a.Q + int64_t(i) * k;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int f = (c * LPR + l) * VEC;
        if (f < k) {
          Pack<VEC> pp, pq;
          pp.load(pu + f);
          pq.load(qi + f);
#pragma unroll
          for (int v = 0; v < VEC; ++v) dot += pp.v[v] * pq.v[v];
        }
      }
    }
    dot = group_sum<LPR>(dot);
    if (valid && l == 0) {
      const double pred = sigmoid_clipped(dot + a.bu[u] + a.bi[i] + a.b);
      if (a.out_pred) a.out_pred[t] = pred;
      if (a.loss_partial) {
        const double rr = a.y[r] / a.pscore[r];
        loss_acc += rr * log(pred + a.eps) + (1.0 - rr) * log(1.0 - pred + a.eps);
      }
    }
  }
  if (a.loss_partial) {
    lds[tid] = loss_acc;
    __syncthreads();
#pragma unroll
    for (int s = kMfBlock / 2; s > 0; s >>= 1) {
      if (tid < s) lds[tid] += lds[tid + s];
      __syncthreads();
    }
    if (tid == 0) a.loss_partial[blockIdx.x] = lds[0];
  }
}

template <int LPR, int VEC, int NC>
__global__ __launch_bounds__(kMfBlock) void mf_predict_kernel(MfPredArgs a) {
  mf_predict_body<LPR, VEC, NC>(a);
}

__device__ __forceinline__ void mf_loss_finish_body(const double* partial, int n_partial,
                                                    int64_t n_rows, double* out) {
  __shared__ double lds[kMfBlock];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n_partial; i += kMfBlock) acc += partial[i];
  lds[threadIdx.x] = acc;
  __syncthreads();
#pragma unroll
  for (int s = kMfBlock / 2; s > 0; s >>= 1) {
    if (int(threadIdx.x) < s) lds[threadIdx.x] += lds[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = -lds[0] / double(n_rows);
}

__global__ __launch_bounds__(kMfBlock) void mf_loss_finish_kernel(const double* partial,
                                                                 int n_partial, int64_t n_rows,
                                                                 double* out) {
  mf_loss_finish_body(partial, n_partial, n_rows, out);
}

// ---- several models on one log (rfm_mf_predict_many, rfm_mf_predict_loss_many): blockIdx.y is
// the model, blockIdx.x walks the rows as in the single-model launch, so a model's scores and the
// order of its partial sums are those of rfm_mf_predict / rfm_mf_predict_loss
struct MfPredManyArgs {
  const int32_t* users;
  const int32_t* items;
  const int32_t* row_ids;  // nullable
  int64_t n_rows;
  const rfm_mf_model* models;
  const rfm_mf_labels* labels;  // nullable (scores only)
  int32_t k;
  double eps;
  double* const* out_base;  // nullable: model m's scores go to out_base[m] + out_offset
  int64_t out_offset;
  double* loss_partial;  // nullable: [model][block]
};

template <int LPR, int VEC, int NC>
__global__ __launch_bounds__(kMfBlock) void mf_predict_many_kernel(MfPredManyArgs m) {
  const rfm_mf_model mod = m.models[blockIdx.y];
  MfPredArgs a;
  a.users = m.users;
  a.items = m.items;
  a.row_ids = m.row_ids;
  a.n_rows = m.n_rows;
  a.P = mod.P;
  a.Q = mod.Q;
  a.bu = mod.bu;
  a.bi = mod.bi;
  a.b = mod.b;
  a.k = m.k;
  a.y = m.labels ? m.labels[blockIdx.y].y : nullptr;
  a.pscore = m.labels ? m.labels[blockIdx.y].pscore : nullptr;
  a.out_pred = m.out_base ? m.out_base[blockIdx.y] + m.out_offset : nullptr;
  a.loss_partial = m.loss_partial ? m.loss_partial + int64_t(blockIdx.y) * gridDim.x : nullptr;
  a.eps = m.eps;
  mf_predict_body<LPR, VEC, NC>(a);
}

__global__ __launch_bounds__(kMfBlock) void mf_loss_finish_many_kernel(const double* partial,
                                                                      int n_partial, int64_t n_rows,
                                                                      double* out, int64_t out_stride) {
  mf_loss_finish_body(partial + int64_t(blockIdx.x) * n_partial, n_partial, n_rows,
                      out + int64_t(blockIdx.x) * out_stride);
}

// THE UPDATE RULE of the record form's kernels (mf_update and the bodies that call it), a type
// parameter O.  SgdRule (rfm_rule.hpp): theta -= lr * g, the text every site had before there was
// a choice; its instantiations are that code.  MfAdaGradRule (rfm_mf_sgd_levels_opt): every element
// of P, Q, b_u, b_i has an accumulator G of its own and takes adagrad_element's step, with g the
// element's gradient as the SGD text forms it, the four updates of an example in the reference's
// order.
struct MfAdaGradRule {
  static constexpr bool kAda = true;
  double* acc_P;   // [n_users][k]
  double* acc_Q;   // [n_items][k]
  double* acc_bu;  // [n_users]
  double* acc_bi;  // [n_items]
  double eps;
};

// the accumulators of one example's two rows and two biases in registers (nothing under SgdRule)
template <int VEC, int NC, bool ADA>
struct MfAccRegs {};
template <int VEC, int NC>
struct MfAccRegs<VEC, NC, true> {
  Pack<VEC> gp[NC], gq[NC];
  double gbu, gbi;
};

// the arithmetic of one example on rows already in registers (src/mf.py:99-108,
// 172-216): returns the residual, rows and biases are updated in place (acc: their accumulators,
// MfAdaGradRule only, needed after the residual)
template <int LPR, int VEC, int NC, class O = SgdRule>
__device__ inline void mf_update(Pack<VEC> (&pp)[NC], Pack<VEC> (&pq)[NC], double& bu,
                                 double& bi, double ry, double b, double lr, double reg, int k,
                                 int l, const O& o = O{},
                                 MfAccRegs<VEC, NC, O::kAda>* acc = nullptr) {
  double dot = 0.0;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int f = (c * LPR + l) * VEC;
    if (f < k) {
#pragma unroll
      for (int v = 0; v < VEC; ++v) dot += pp[c].v[v] * pq[c].v[v];
    }
  }
  dot = group_sum<LPR>(dot);
  const double err = ry - sigmoid_clipped(dot + bu + bi + b);
  if constexpr (O::kAda) {
    // (the four updates are independent but for the item row reading the new user row: the user's
    // two first, then the item's two, gives the bits of the reference's order)
#pragma unroll
    for (int c = 0; c < NC; ++c) {
#pragma unroll
      for (int v = 0; v < VEC; ++v)
        pp[c].v[v] = adagrad_element(pp[c].v[v], -err * pq[c].v[v] + reg * pp[c].v[v], lr, o.eps,
                                        &acc->gp[c].v[v]);
    }
    bu = adagrad_element(bu, -err + reg * bu, lr, o.eps, &acc->gbu);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
#pragma unroll
      for (int v = 0; v < VEC; ++v)
        // the item row sees the user row this example has just updated (src/mf.py:193)
        pq[c].v[v] = adagrad_element(pq[c].v[v], -err * pp[c].v[v] + reg * pq[c].v[v], lr, o.eps,
                                        &acc->gq[c].v[v]);
    }
    bi = adagrad_element(bi, -err + reg * bi, lr, o.eps, &acc->gbi);
  } else {
#pragma unroll
    for (int c = 0; c < NC; ++c) {
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        const double p_new = pp[c].v[v] - lr * (-err * pq[c].v[v] + reg * pp[c].v[v]);
        // the item row sees the user row this example has just updated (src/mf.py:193)
        const double q_new = pq[c].v[v] - lr * (-err * p_new + reg * pq[c].v[v]);
        pp[c].v[v] = p_new;
        pq[c].v[v] = q_new;
      }
    }
    bu = bu - lr * (-err + reg * bu);
    bi = bi - lr * (-err + reg * bi);
  }
}

template <int LPR, int VEC, int NC>
__device__ inline void mf_load_row(Pack<VEC> (&dst)[NC], const double* row, int k, int l) {
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int f = (c * LPR + l) * VEC;
    dst[c].load(row + (f < k ? f : 0));
  }
}

// an accumulator row (memory or LDS): a chunk past k is not read -- its lanes compute on zeros and
// store nothing -- so every chunk's address is the row's plus a constant and none is kept in
// registers of its own (mf_load_row's clamped addresses are: two registers a chunk and row)
template <int LPR, int VEC, int NC>
__device__ inline void mf_load_acc_row(Pack<VEC> (&dst)[NC], const double* row, int k, int l) {
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int f = (c * LPR + l) * VEC;
#pragma unroll
    for (int v = 0; v < VEC; ++v) dst[c].v[v] = 0.0;
    if (f < k) dst[c].load(row + f);
  }
}

template <int LPR, int VEC, int NC>
__device__ inline void mf_store_row(const Pack<VEC> (&src)[NC], double* row, int k, int l) {
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int f = (c * LPR + l) * VEC;
    if (f < k) src[c].store(row + f);
  }
}

struct MfSgdArgs {
  const int32_t* users;
  const int32_t* items;
  const double* y;
  const double* pscore;
  const int32_t* pos_rows;   // batch position -> training row
  const int32_t* order;      // batch positions grouped by level (null: identity)
  const int32_t* level_ptr;  // device copy (sequential kernel only)
  int32_t lo, hi;            // wide kernel: order[lo, hi); seq kernel: levels [lo, hi)
  double* P;
  double* Q;
  double* bu;
  double* bi;
  double b;
  int32_t k;
  double lr, reg;
};

// one example of the plain form, LPR lanes
template <int LPR, int VEC, int NC>
__device__ inline void mf_example(const MfSgdArgs& a, int32_t s, int l) {
  const int k = a.k;
  const int64_t r = a.pos_rows[s];
  const int32_t u = a.users[r], i = a.items[r];
  Pack<VEC> pp[NC], pq[NC];
  mf_load_row<LPR, VEC, NC>(pp, a.P + int64_t(u) * k, k, l);
  mf_load_row<LPR, VEC, NC>(pq, a.Q + int64_t(i) * k, k, l);
  double bu = a.bu[u], bi = a.bi[i];
  mf_update<LPR, VEC, NC>(pp, pq, bu, bi, a.y[r] / a.pscore[r], a.b, a.lr, a.reg, k, l);
  mf_store_row<LPR, VEC, NC>(pp, a.P + int64_t(u) * k, k, l);
  mf_store_row<LPR, VEC, NC>(pq, a.Q + int64_t(i) * k, k, l);
  if (l == 0) {
    a.bu[u] = bu;
    a.bi[i] = bi;
  }
}

// one level, many workgroups
template <int LPR, int VEC, int NC>
__global__ __launch_bounds__(kMfBlock) void mf_sgd_wide_kernel(MfSgdArgs a) {
  constexpr int GPB = kMfBlock / LPR;
  const int l = threadIdx.x % LPR;
  const int g = threadIdx.x / LPR;
  for (int64_t idx = int64_t(a.lo) + int64_t(blockIdx.x) * GPB + g; idx < a.hi;
       idx += int64_t(gridDim.x) * GPB)
    mf_example<LPR, VEC, NC>(a, a.order ? a.order[idx] : int32_t(idx), l);
}

// levels [lo, hi) by one workgroup, barrier between levels
template <int LPR, int VEC, int NC>
__global__ __launch_bounds__(kSeqBlock) void mf_sgd_seq_kernel(MfSgdArgs a) {
  constexpr int GPB = kSeqBlock / LPR;
  const int l = threadIdx.x % LPR;
  const int g = threadIdx.x / LPR;
  for (int lev = a.lo; lev < a.hi; ++lev) {
    const int32_t b0 = a.level_ptr[lev], b1 = a.level_ptr[lev + 1];
    for (int32_t idx = b0 + g; idx < b1; idx += GPB) mf_example<LPR, VEC, NC>(a, a.order[idx], l);
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// level-ordered example records: the fast form of the same schedule
// ---------------------------------------------------------------------------
struct MfEx {       // one example of a batch, stored in level order, 24 B
  int32_t u, i;     // user, item
  int32_t cslot;    // >= 0: LDS cache slot of the item row in the sequential kernel;
                    // -1: the item occurs once in the batch; -2: repeated but not cached
  int32_t gap;      // levels between this example and the previous writer of its user row
                    // (RFM_MF_NO_WRITER if none in the batch): the row is final that far ahead
  double ry;        // label / propensity
};

struct MfExArgs {
  const MfEx* ex;            // [batch], grouped by level
  const int32_t* level_ptr;  // device copy (sequential kernel only)
  int32_t lo, hi;            // wide kernel: ex[lo, hi); seq kernel: levels [lo, hi)
  int32_t rec_lo, rec_hi;    // seq kernel: level_ptr[lo], level_ptr[hi]
  const int32_t* cache_items;  // items whose rows the sequential kernel keeps in LDS
  int32_t n_cached;
  double* P;
  double* Q;
  double* bu;
  double* bi;
  double b;
  int32_t k;
  double lr, reg;
};

// where a record's label / propensity comes from: the record itself (one model), or the model's
// own vector over the training log through the record's row (several models on one schedule)
struct RyOfRecord {
  static constexpr bool kInRecord = true;
  __device__ __forceinline__ double operator()(int32_t, double ry) const { return ry; }
};
struct RyOfModel {
  static constexpr bool kInRecord = false;
  const double* ry;         // [rows of the training log]
  const int32_t* ex_rows;   // [batch] training-log row of each record, level order
  __device__ __forceinline__ double operator()(int32_t rec, double) const { return ry[ex_rows[rec]]; }
};

// one level, many workgroups (examples of a level touch disjoint rows); blockIdx.x / gridDim.x
// walk the level
template <int LPR, int VEC, int NC, class Ry, class O = SgdRule>
__device__ __forceinline__ void mf_wide_ex_body(const MfExArgs& a, Ry ry_of, const O& o = O{}) {
  constexpr int GPB = kMfBlock / LPR;
  const int l = threadIdx.x % LPR;
  const int g = threadIdx.x / LPR;
  const int k = a.k;
  for (int64_t idx = int64_t(a.lo) + int64_t(blockIdx.x) * GPB + g; idx < a.hi;
       idx += int64_t(gridDim.x) * GPB) {
    const MfEx e = a.ex[idx];
    Pack<VEC> pp[NC], pq[NC];
    mf_load_row<LPR, VEC, NC>(pp, a.P + int64_t(e.u) * k, k, l);
    mf_load_row<LPR, VEC, NC>(pq, a.Q + int64_t(e.i) * k, k, l);
    double bu = a.bu[e.u], bi = a.bi[e.i];
    if constexpr (O::kAda) {
      // the two accumulator rows and the two bias accumulators beside the parameter rows
      MfAccRegs<VEC, NC, true> acc;
      mf_load_acc_row<LPR, VEC, NC>(acc.gp, o.acc_P + int64_t(e.u) * k, k, l);
      mf_load_acc_row<LPR, VEC, NC>(acc.gq, o.acc_Q + int64_t(e.i) * k, k, l);
      acc.gbu = o.acc_bu[e.u];
      acc.gbi = o.acc_bi[e.i];
      mf_update<LPR, VEC, NC, O>(pp, pq, bu, bi, ry_of(int32_t(idx), e.ry), a.b, a.lr, a.reg, k, l, o, &acc);
      mf_store_row<LPR, VEC, NC>(acc.gp, o.acc_P + int64_t(e.u) * k, k, l);
      mf_store_row<LPR, VEC, NC>(acc.gq, o.acc_Q + int64_t(e.i) * k, k, l);
      if (l == 0) {
        o.acc_bu[e.u] = acc.gbu;
        o.acc_bi[e.i] = acc.gbi;
      }
    } else {
      mf_update<LPR, VEC, NC>(pp, pq, bu, bi, ry_of(int32_t(idx), e.ry), a.b, a.lr, a.reg, k, l);
    }
    mf_store_row<LPR, VEC, NC>(pp, a.P + int64_t(e.u) * k, k, l);
    mf_store_row<LPR, VEC, NC>(pq, a.Q + int64_t(e.i) * k, k, l);
    if (l == 0) {
      a.bu[e.u] = bu;
      a.bi[e.i] = bi;
    }
  }
}

template <int LPR, int VEC, int NC, class O = SgdRule>
__global__ __launch_bounds__(kMfBlock) void mf_sgd_wide_ex_kernel(ArgsUnder<MfExArgs, O> a) {
  mf_wide_ex_body<LPR, VEC, NC, RyOfRecord, O>(a, RyOfRecord{}, rule_of(a));
}

// Several models on one schedule (rfm_mf_sgd_levels_many): the records, level pointers and cached
// items are shared, the parameters, lr, reg, b and the label / propensity vector are the model's.
// A workgroup builds its own MfExArgs from its model's row of the table and runs the bodies above.
struct MfManyArgs {
  const MfEx* ex;
  const int32_t* ex_rows;    // [batch] training-log row of each record
  const int32_t* level_ptr;
  int32_t lo, hi;
  int32_t rec_lo, rec_hi;
  const int32_t* cache_items;
  int32_t n_cached;
  const rfm_mf_model* models;
  int32_t k;
};

__device__ __forceinline__ MfExArgs mf_model_args(const MfManyArgs& m, const rfm_mf_model& mod) {
  MfExArgs a;
  a.ex = m.ex;
  a.level_ptr = m.level_ptr;
  a.lo = m.lo;
  a.hi = m.hi;
  a.rec_lo = m.rec_lo;
  a.rec_hi = m.rec_hi;
  a.cache_items = m.cache_items;
  a.n_cached = m.n_cached;
  a.P = mod.P;
  a.Q = mod.Q;
  a.bu = mod.bu;
  a.bi = mod.bi;
  a.b = mod.b;
  a.k = m.k;
  a.lr = mod.lr;
  a.reg = mod.reg;
  return a;
}

// one level of every model: blockIdx.y is the model
template <int LPR, int VEC, int NC>
__global__ __launch_bounds__(kMfBlock) void mf_sgd_wide_many_kernel(MfManyArgs m) {
  const rfm_mf_model mod = m.models[blockIdx.y];
  mf_wide_ex_body<LPR, VEC, NC>(mf_model_args(m, mod), RyOfModel{mod.ry, m.ex_rows});
}

// ---------------------------------------------------------------------------
// The chain of small levels (the path through a popular item is hundreds of levels
// long), by ONE workgroup with a barrier between levels.  Nothing on the
// level-to-level path waits for an index load:
//  * the chunk's level pointers and example records are copied to LDS first;
//  * the rows (and biases) of the items that occur more than once in the batch
//    live in LDS for the whole launch;
//  * a lane group knows the example it runs kMfAhead levels ahead and loads the
//    user row / bias (when final by then: MfEx.gap) and the row of an item that
//    occurs only once into a register slot of a ring of kMfAhead slots.  The ring
//    is unrolled with fixed slots and its loads are unconditional (unused ones read
//    row 0).
// What remains per level (about 0.7 us) is the dependent arithmetic of one example --
// dot product, lane-group reduction, exp, division, the two row updates -- issued by a
// single wavefront; a one-wavefront variant without barriers, with an LDS ring that
// forwards rows between levels, measured no faster and was dropped.
// ---------------------------------------------------------------------------
constexpr int kMfAhead = RFM_MF_READ_AHEAD;
static_assert(kMfAhead == 4, "the level loop below is unrolled for four slots");
constexpr int kSeqMaxLevels = 1024;  // per launch: level pointers, 4 KiB of LDS
constexpr int kSeqMaxRecs = 1024;    // per launch: example records, 24 KiB of LDS
constexpr int kSeqMaxCacheBytes = 32 << 10;  // (96 KiB measured no faster at k = 16 ... 400: more rows to copy in and write back per launch)

template <int VEC, int NC>
struct MfSlot {
  MfEx e;
  bool has;       // this lane group has an example at the slot's level
  bool got_user;  // pp / bu hold the user row (final)
  bool got_item;  // pq / bi hold the item row (an item that occurs once in the batch)
  Pack<VEC> pp[NC], pq[NC];
  double bu, bi;
};

struct MfSeqLds {
  const int32_t* lptr;  // [n_lev + 1], relative to the chunk's first record
  const MfEx* exs;      // [n_rec]
  double* qcache;       // [n_cached][k+2]: item row, item bias, pad (MfAdaGradRule: [n_cached][2][k+2],
                        // the same of the item's accumulators behind it)
  int32_t n_lev;
};

// doubles of one cached item in LDS under rule O
template <class O>
__device__ __forceinline__ int mf_cache_width(int k) {
  return O::kAda ? 2 * (k + 2) : k + 2;
}

// what lane group g runs at chunk level t, and its rows if they may be read now: the
// user row is final when its previous writer lies more than `ahead` levels back
template <int LPR, int VEC, int NC, bool PF>
__device__ __forceinline__ void mf_slot_fetch(const MfExArgs& a, const MfSeqLds& m, int t, int g,
                                              int l, int ahead, MfSlot<VEC, NC>& s) {
  int32_t idx = 0;
  bool has = false;
  if (t < m.n_lev) {
    idx = m.lptr[t] + g;
    has = idx < m.lptr[t + 1];
  }
  s.e = m.exs[has ? idx : 0];
  s.has = has;
  s.got_user = PF && has && s.e.gap > ahead;
  s.got_item = PF && has && s.e.cslot == -1;
  // a wavefront none of whose lane groups has an example at that level issues nothing
  // (the condition is uniform in the wavefront, so the loads of an active one stay
  // unconditional and together)
  if (PF && __ballot(has) != 0ull) {
    const int k = a.k;
    const int32_t u = s.got_user ? s.e.u : 0;
    const int32_t it = s.got_item ? s.e.i : 0;
    mf_load_row<LPR, VEC, NC>(s.pp, a.P + int64_t(u) * k, k, l);
    s.bu = a.bu[u];
    mf_load_row<LPR, VEC, NC>(s.pq, a.Q + int64_t(it) * k, k, l);
    s.bi = a.bi[it];
  }
}

// (MfAdaGradRule: the accumulators are not in the ring.  They are requested here, behind whatever
// parameter rows are still to be read, and are needed only after the residual, so their latency
// lies beside the dot product, the lane-group sum and the sigmoid; an accumulator row has the
// writer of its parameter row, so it is final here as that row is.)
template <int LPR, int VEC, int NC, class O = SgdRule>
__device__ __forceinline__ void mf_slot_run(const MfExArgs& a, const MfSeqLds& m, int l,
                                            MfSlot<VEC, NC>& s, const O& o = O{}) {
  if (!s.has) return;
  const int k = a.k;
  const MfEx e = s.e;
  if (!s.got_user) {  // written within the last kMfAhead levels: read it now
    mf_load_row<LPR, VEC, NC>(s.pp, a.P + int64_t(e.u) * k, k, l);
    s.bu = a.bu[e.u];
  }
  if (e.cslot < 0 && !s.got_item) {  // item row through memory
    mf_load_row<LPR, VEC, NC>(s.pq, a.Q + int64_t(e.i) * k, k, l);
    s.bi = a.bi[e.i];
  }
  double* crow = m.qcache + (e.cslot >= 0 ? e.cslot : 0) * mf_cache_width<O>(k);
  if (e.cslot >= 0) {
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int f = (c * LPR + l) * VEC;
      s.pq[c].load(crow + (f < k ? f : 0));
    }
    s.bi = crow[k];
  }
  if constexpr (O::kAda) {
    MfAccRegs<VEC, NC, true> acc;
    double* grow = crow + (k + 2);  // a cached item's accumulators
    mf_load_acc_row<LPR, VEC, NC>(acc.gp, o.acc_P + int64_t(e.u) * k, k, l);
    acc.gbu = o.acc_bu[e.u];
    if (e.cslot >= 0) {
      mf_load_acc_row<LPR, VEC, NC>(acc.gq, grow, k, l);
      acc.gbi = grow[k];
    } else {
      mf_load_acc_row<LPR, VEC, NC>(acc.gq, o.acc_Q + int64_t(e.i) * k, k, l);
      acc.gbi = o.acc_bi[e.i];
    }
    mf_update<LPR, VEC, NC, O>(s.pp, s.pq, s.bu, s.bi, e.ry, a.b, a.lr, a.reg, k, l, o, &acc);
    mf_store_row<LPR, VEC, NC>(acc.gp, o.acc_P + int64_t(e.u) * k, k, l);
    if (l == 0) o.acc_bu[e.u] = acc.gbu;
    if (e.cslot >= 0) {
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int f = (c * LPR + l) * VEC;
        if (f < k) acc.gq[c].store(grow + f);
      }
      if (l == 0) grow[k] = acc.gbi;
    } else {
      mf_store_row<LPR, VEC, NC>(acc.gq, o.acc_Q + int64_t(e.i) * k, k, l);
      if (l == 0) o.acc_bi[e.i] = acc.gbi;
    }
  } else {
    mf_update<LPR, VEC, NC>(s.pp, s.pq, s.bu, s.bi, e.ry, a.b, a.lr, a.reg, k, l);
  }
  mf_store_row<LPR, VEC, NC>(s.pp, a.P + int64_t(e.u) * k, k, l);
  if (l == 0) a.bu[e.u] = s.bu;
  if (e.cslot >= 0) {
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int f = (c * LPR + l) * VEC;
      if (f < k) s.pq[c].store(crow + f);
    }
    if (l == 0) crow[k] = s.bi;
  } else {
    mf_store_row<LPR, VEC, NC>(s.pq, a.Q + int64_t(e.i) * k, k, l);
    if (l == 0) a.bi[e.i] = s.bi;
  }
}

// levels [lo, hi) (at most kSeqMaxLevels, kSeqMaxRecs examples, each level of at most
// kSeqBlock/LPR examples); a.rec_lo / a.rec_hi = level_ptr[lo] / level_ptr[hi]
// (BLOCK: 1024 threads for one chunk of factors per lane; 512 for two to four chunks -- the
// reference's published k = 300 / 400 -- whose ring of four slots needs 128 + VGPRs: eight lane
// groups then, and more than four chunks run without the ring)
constexpr int seq_block(int nc) { return nc > 1 ? 512 : kSeqBlock; }

// Slots of the read-ahead ring under MfAdaGradRule, by shape class.  The accumulators of the running
// example (as many registers as its two rows and biases) and the root and quotient come on top of
// the ring, and no instantiation may spill (profiles/n23/register_counts.txt): at one chunk of two
// factors per lane the 1024-thread workgroup has 128 registers a lane and SgdRule's ring of four
// takes 116 of them, so two slots; at four chunks three slots.
constexpr int mf_ada_ring(int vec, int nc) {
  return nc > 4 ? 0 : nc == 4 ? 3 : (vec == 2 && nc == 1) ? 2 : kMfAhead;
}
// Threads of the sequential workgroup under a rule.  The level limit (seq_block(nc) / LPR examples)
// is the schedule's and does not depend on the rule; at sixteen chunks a lane the four rows of an
// AdaGrad example and the residual's constants do not fit the 256 registers of a 512-thread
// workgroup, so that class runs 256 threads and a lane group takes its level in two passes.
template <class O>
constexpr int mf_seq_threads(int nc) {
  return O::kAda && nc > 8 ? 256 : seq_block(nc);
}

template <int LPR, int VEC, int NC, class Ry, class O = SgdRule>
__device__ __forceinline__ void mf_seq_ex_body(const MfExArgs& a, Ry ry_of, const O& o = O{}) {
  extern __shared__ double seq_lds[];
  constexpr int kSeqBlock = mf_seq_threads<O>(NC);  // (shadows the one-chunk constant inside this kernel)
  // rows wider than four chunks per lane leave no registers for a ring of them
  constexpr bool PF = NC <= 4;
  const int l = threadIdx.x % LPR;
  const int g = threadIdx.x / LPR;
  const int k = a.k;
  const int cw = mf_cache_width<O>(k);
  const int n_lev = a.hi - a.lo;
  const int n_rec = a.rec_hi - a.rec_lo;
  int32_t* lptr = reinterpret_cast<int32_t*>(seq_lds);
  MfEx* exs = reinterpret_cast<MfEx*>(seq_lds + (n_lev + 2) / 2);
  double* qcache = reinterpret_cast<double*>(exs + n_rec);
  for (int i = threadIdx.x; i <= n_lev; i += kSeqBlock) lptr[i] = a.level_ptr[a.lo + i] - a.rec_lo;
  {
    const double* src = reinterpret_cast<const double*>(a.ex + a.rec_lo);
    double* dst = reinterpret_cast<double*>(exs);
    // (a record is three doubles, the third its label / propensity: where that comes from the
    // model's vector, it is fetched first -- two dependent loads -- and the copy leaves it alone)
    static_assert(sizeof(MfEx) == 24 && offsetof(MfEx, ry) == 16, "MfEx layout");
    if (!Ry::kInRecord)
      for (int r = threadIdx.x; r < n_rec; r += kSeqBlock) dst[3 * r + 2] = ry_of(a.rec_lo + r, 0.0);
    for (int i = threadIdx.x; i < n_rec * 3; i += kSeqBlock)
      if (Ry::kInRecord || i % 3 != 2) dst[i] = src[i];
  }
  for (int i = threadIdx.x; i < a.n_cached * cw; i += kSeqBlock) {
    const int c = i / cw, f = i % cw;
    const int32_t item = a.cache_items[c];
    if constexpr (O::kAda) {
      // the item's row, bias and pad, then the same of its accumulators
      const int h = f / (k + 2), ff = f % (k + 2);
      const double* rows = h ? o.acc_Q : a.Q;
      const double* bias = h ? o.acc_bi : a.bi;
      qcache[i] = ff < k ? rows[int64_t(item) * k + ff] : (ff == k ? bias[item] : 0.0);
    } else {
      qcache[i] = f < k ? a.Q[int64_t(item) * k + f] : (f == k ? a.bi[item] : 0.0);
    }
  }
  __syncthreads();
  const MfSeqLds m{lptr, exs, qcache, n_lev};

  MfSlot<VEC, NC> s0, s1, s2, s3;
  if constexpr (O::kAda) {
    // the same walk with a ring of as many slots as the class's registers hold beside the
    // accumulators (mf_ada_ring): the rows of level t + D are read while level t is still running,
    // final if the previous writer lies more than D levels back; D = 0 reads every row where it is used
    constexpr int D = mf_ada_ring(VEC, NC);
    if constexpr (D > 0) {
      MfSlot<VEC, NC> s[D];
#pragma unroll
      for (int d = 0; d < D; ++d) mf_slot_fetch<LPR, VEC, NC, true>(a, m, d, g, l, d, s[d]);
      for (int t = 0; t < n_lev; t += D) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
          if (t + d >= n_lev) break;
          mf_slot_run<LPR, VEC, NC, O>(a, m, l, s[d], o);
          mf_slot_fetch<LPR, VEC, NC, true>(a, m, t + d + D, g, l, D, s[d]);
          __syncthreads();
        }
      }
    } else {
      // (a level holds up to seq_block(NC) / LPR examples whatever the workgroup's size)
      MfSlot<VEC, NC> s;
      for (int t = 0; t < n_lev; ++t) {
        for (int gg = g; gg < seq_block(NC) / LPR; gg += kSeqBlock / LPR) {
          mf_slot_fetch<LPR, VEC, NC, false>(a, m, t, gg, l, 0, s);
          mf_slot_run<LPR, VEC, NC, O>(a, m, l, s, o);
        }
        __syncthreads();
      }
    }
  } else {
    // every level before lo has run, so the first level's rows are final; a row of one
    // of the next levels is final if its previous writer lies before this launch
    mf_slot_fetch<LPR, VEC, NC, PF>(a, m, 0, g, l, 0, s0);
    mf_slot_fetch<LPR, VEC, NC, PF>(a, m, 1, g, l, 1, s1);
    mf_slot_fetch<LPR, VEC, NC, PF>(a, m, 2, g, l, 2, s2);
    mf_slot_fetch<LPR, VEC, NC, PF>(a, m, 3, g, l, 3, s3);
    for (int t = 0; t < n_lev; t += kMfAhead) {
      // the rows of level t+4 are read while level t is still running: final if the
      // previous writer lies before level t, i.e. more than four levels back
      mf_slot_run<LPR, VEC, NC, O>(a, m, l, s0, o);
      mf_slot_fetch<LPR, VEC, NC, PF>(a, m, t + 4, g, l, kMfAhead, s0);
      __syncthreads();
      if (t + 1 >= n_lev) break;
      mf_slot_run<LPR, VEC, NC, O>(a, m, l, s1, o);
      mf_slot_fetch<LPR, VEC, NC, PF>(a, m, t + 5, g, l, kMfAhead, s1);
      __syncthreads();
      if (t + 2 >= n_lev) break;
      mf_slot_run<LPR, VEC, NC, O>(a, m, l, s2, o);
      mf_slot_fetch<LPR, VEC, NC, PF>(a, m, t + 6, g, l, kMfAhead, s2);
      __syncthreads();
      if (t + 3 >= n_lev) break;
      mf_slot_run<LPR, VEC, NC, O>(a, m, l, s3, o);
      mf_slot_fetch<LPR, VEC, NC, PF>(a, m, t + 7, g, l, kMfAhead, s3);
      __syncthreads();
    }
  }
  __syncthreads();
  // write the cached item rows back
  for (int i = threadIdx.x; i < a.n_cached * cw; i += kSeqBlock) {
    const int c = i / cw, f = i % cw;
    const int32_t item = a.cache_items[c];
    if constexpr (O::kAda) {
      const int h = f / (k + 2), ff = f % (k + 2);
      double* rows = h ? o.acc_Q : a.Q;
      double* bias = h ? o.acc_bi : a.bi;
      if (ff < k)
        rows[int64_t(item) * k + ff] = qcache[i];
      else if (ff == k)
        bias[item] = qcache[i];
    } else {
      if (f < k)
        a.Q[int64_t(item) * k + f] = qcache[i];
      else if (f == k)
        a.bi[item] = qcache[i];
    }
  }
}

template <int LPR, int VEC, int NC, class O = SgdRule>
__global__ __launch_bounds__(mf_seq_threads<O>(NC)) void mf_sgd_seq_ex_kernel(ArgsUnder<MfExArgs, O> a) {
  mf_seq_ex_body<LPR, VEC, NC, RyOfRecord, O>(a, RyOfRecord{}, rule_of(a));
}

// the chain of every model, ONE sequential workgroup each: blockIdx.x is the model
template <int LPR, int VEC, int NC>
__global__ __launch_bounds__(seq_block(NC)) void mf_sgd_seq_many_kernel(MfManyArgs m) {
  const rfm_mf_model mod = m.models[blockIdx.x];
  mf_seq_ex_body<LPR, VEC, NC>(mf_model_args(m, mod), RyOfModel{mod.ry, m.ex_rows});
}

// the sequential kernels with their dynamic-LDS limit raised where the item cache needs it
template <int L, int Vv, int N, class O = SgdRule>
static void launch_seq_ex(rfm_ctx* ctx, const ArgsUnder<MfExArgs, O>& a, int threads, size_t lds) {
  const auto kern = &mf_sgd_seq_ex_kernel<L, Vv, N, O>;
  static LdsLimits allowed;
  allow_dynamic_lds(ctx, reinterpret_cast<const void*>(kern), lds, allowed);
  hipLaunchKernelGGL(kern, dim3(1), dim3(threads), lds, ctx->stream, a);
}
template <int L, int Vv, int N>
static void launch_seq_many(rfm_ctx* ctx, const MfManyArgs& m, int n_models, int threads, size_t lds) {
  const auto kern = &mf_sgd_seq_many_kernel<L, Vv, N>;
  static LdsLimits allowed;
  allow_dynamic_lds(ctx, reinterpret_cast<const void*>(kern), lds, allowed);
  hipLaunchKernelGGL(kern, dim3(n_models), dim3(threads), lds, ctx->stream, m);
}

// the model's fields of a kernel argument block (MfPredArgs, MfSgdArgs, MfExArgs)
template <class Args>
static void set_model(Args& a, decltype(Args::P) P, decltype(Args::P) Q, decltype(Args::P) bu,
                      decltype(Args::P) bi, double b, int32_t k) {
  RFM_REQUIRE(P && Q && bu && bi, "null pointer");
  a.P = P;
  a.Q = Q;
  a.bu = bu;
  a.bi = bi;
  a.b = b;
  a.k = k;
}
template <class Args>
static void set_model(Args& a, double* P, double* Q, double* bu, double* bi, double b, int32_t k,
                      double lr, double reg) {
  set_model(a, P, Q, bu, bi, b, k);
  a.lr = lr;
  a.reg = reg;
}

// rfm_mf_predict (scores of any number of rows) and, with want_loss, rfm_mf_predict_loss (the
// loss of at least one row; the scores only where d_out_pred is given)
static int32_t mf_predict(rfm_ctx* ctx, const int32_t* d_users, const int32_t* d_items,
                          const double* d_y, const double* d_pscore, const int32_t* d_row_ids,
                          int64_t n_rows, const double* d_P, const double* d_Q,
                          const double* d_bu, const double* d_bi, double b, int32_t n_factors,
                          double eps, double* d_out_pred, double* d_out_loss, bool want_loss) {
  return guarded([&] {
    RFM_REQUIRE(ctx, "null ctx");
    RFM_REQUIRE(n_rows >= (want_loss ? 1 : 0), "n_rows=%lld out of range", (long long)n_rows);
    if (n_rows == 0) return;
    RFM_REQUIRE(d_users && d_items && (want_loss ? d_y && d_pscore && d_out_loss : d_out_pred != nullptr),
                "null pointer");
    MfPredArgs a{};
    set_model(a, d_P, d_Q, d_bu, d_bi, b, n_factors);
    a.users = d_users;
    a.items = d_items;
    a.row_ids = d_row_ids;
    a.n_rows = n_rows;
    a.y = d_y;
    a.pscore = d_pscore;
    a.eps = eps;
    a.out_pred = d_out_pred;
    const Shape s = shape_for(a.k);
    const int grid = capped_grid(ctx, n_rows, kMfBlock / s.lpr, 8, 1);
    if (want_loss) {
      ctx->loss_partials.ensure(size_t(ctx->n_cu) * 8 * sizeof(double));
      a.loss_partial = ctx->loss_partials.as<double>();
    }
#define RFM_CALL_MFP(L, Vv, N) \
  hipLaunchKernelGGL((mf_predict_kernel<L, Vv, N>), dim3(grid), dim3(kMfBlock), 0, ctx->stream, a)
    RFM_FOR_SHAPE(s, RFM_CALL_MFP);
#undef RFM_CALL_MFP
    if (want_loss)
      hipLaunchKernelGGL(mf_loss_finish_kernel, dim3(1), dim3(kMfBlock), 0, ctx->stream,
                         a.loss_partial, grid, n_rows, d_out_loss);
    RFM_HIP_CHECK(hipGetLastError());
  });
}

// rfm_mf_predict_many and, with want_loss, rfm_mf_predict_loss_many: the grid of mf_predict over
// the rows, times the models
static int32_t mf_predict_many(rfm_ctx* ctx, const int32_t* d_users, const int32_t* d_items,
                               const rfm_mf_labels* d_labels, const int32_t* d_row_ids, int64_t n_rows,
                               const rfm_mf_model* d_models, int32_t n_models, int32_t n_factors,
                               double eps, double* const* d_out_base, int64_t out_offset,
                               double* d_out_loss, int64_t loss_stride, bool want_loss) {
  return guarded([&] {
    RFM_REQUIRE(ctx, "null ctx");
    RFM_REQUIRE(n_models >= 1 && n_models <= RFM_MF_MAX_MODELS, "n_models=%d out of range (1..%d)",
                n_models, RFM_MF_MAX_MODELS);
    RFM_REQUIRE(n_rows >= (want_loss ? 1 : 0), "n_rows=%lld out of range", (long long)n_rows);
    const Shape s = shape_for(n_factors);
    if (n_rows == 0) return;
    RFM_REQUIRE(d_users && d_items && d_models &&
                    (want_loss ? d_labels && d_out_loss : d_out_base != nullptr),
                "null pointer");
    RFM_REQUIRE(out_offset >= 0 && (!want_loss || loss_stride >= 1), "bad output offsets");
    MfPredManyArgs a{};
    a.users = d_users;
    a.items = d_items;
    a.row_ids = d_row_ids;
    a.n_rows = n_rows;
    a.models = d_models;
    a.labels = want_loss ? d_labels : nullptr;
    a.k = n_factors;
    a.eps = eps;
    a.out_base = d_out_base;
    a.out_offset = out_offset;
    const int grid = capped_grid(ctx, n_rows, kMfBlock / s.lpr, 8, 1);
    if (want_loss) {
      ctx->loss_partials.ensure(size_t(n_models) * size_t(ctx->n_cu) * 8 * sizeof(double));
      a.loss_partial = ctx->loss_partials.as<double>();
    }
#define RFM_CALL_MFPM(L, Vv, N)                                                                   \
  hipLaunchKernelGGL((mf_predict_many_kernel<L, Vv, N>), dim3(grid, n_models), dim3(kMfBlock), 0, \
                     ctx->stream, a)
    RFM_FOR_SHAPE(s, RFM_CALL_MFPM);
#undef RFM_CALL_MFPM
    if (want_loss)
      hipLaunchKernelGGL(mf_loss_finish_many_kernel, dim3(n_models), dim3(kMfBlock), 0, ctx->stream,
                         a.loss_partial, grid, n_rows, d_out_loss, loss_stride);
    RFM_HIP_CHECK(hipGetLastError());
  });
}

// the plain form's wide kernel on a.order[a.lo, a.hi) (a null order: batch positions lo .. hi)
static void launch_wide(rfm_ctx* ctx, const Shape& s, const MfSgdArgs& a) {
  const int grid = capped_grid(ctx, int64_t(a.hi) - a.lo, kMfBlock / s.lpr, 8, 0);
#define RFM_CALL_WIDE(L, Vv, N) \
  hipLaunchKernelGGL((mf_sgd_wide_kernel<L, Vv, N>), dim3(grid), dim3(kMfBlock), 0, ctx->stream, a)
  RFM_FOR_SHAPE(s, RFM_CALL_WIDE);
#undef RFM_CALL_WIDE
}

// The launches of one batch from its level pointers: a level of more than seq_cap examples (more
// than the sequential workgroup takes) is one grid-wide launch, wide(rec_lo, rec_hi); a run of
// smaller levels is one sequential launch, seq(lev_lo, lev_hi), that ends before a wide level,
// after max_levels levels and before the level that would take it past max_recs examples (the
// two LDS tables of the record form's kernel; the plain form has neither: kNoLimit).
constexpr int kNoLimit = INT32_MAX;

template <class Wide, class Seq>
static void mf_walk_levels(const int32_t* h_level_ptr, int n_levels, int seq_cap, int max_levels,
                           int max_recs, Wide wide, Seq seq) {
  const auto count = [&](int lev) {
    const int cnt = h_level_ptr[lev + 1] - h_level_ptr[lev];
    RFM_REQUIRE(cnt >= 0, "level_ptr not monotone");
    return cnt;
  };
  int lev = 0;
  while (lev < n_levels) {
    if (count(lev) > seq_cap) {
      wide(h_level_ptr[lev], h_level_ptr[lev + 1]);
      ++lev;
      continue;
    }
    int end = lev;
    while (end < n_levels && end - lev < max_levels && count(end) <= seq_cap &&
           h_level_ptr[end + 1] - h_level_ptr[lev] <= max_recs)
      ++end;
    seq(lev, end);
    lev = end;
  }
}

// ---------------------------------------------------------------------------
// Fold-in (rfm_mf_fold_in): new rows of one side trained against the fixed other side by
// the same per-example update restricted to that side (src/mf.py:99-108, 172-216).  New rows
// are independent of each other and each is one sequential chain, so there is no level
// schedule: ONE LANE GROUP PER NEW ROW, the row and its bias in registers for all of its
// examples and passes, written once at the end; no barrier, atomic or LDS hand-off.
//  * A step is one example of one pass; a chain of n examples and p passes has n * p steps and
//    step s reads example s % n, so the rings below run across a pass boundary unchanged.
//  * The chain is latency-bound, so a lane group reads ahead through two rings of kFoldAhead
//    register slots: the id and weight of the step 2 * kFoldAhead ahead, and -- from the id that
//    arrived one turn of the ring earlier -- the fixed row and bias of the step kFoldAhead ahead.
//    No step waits for an index load and then a row load in sequence.
//  * Lane groups of one wavefront have chains of different length (the host orders the rows by
//    descending length, so neighbours are close).  The wavefront walks to its longest chain with
//    a wave-uniform trip count, so the cross-lane sums run converged; a group past its own chain
//    is predicated off: its loads read row 0 of the fixed side, its update is not applied.
// ---------------------------------------------------------------------------
constexpr int kFoldAhead = RFM_MF_FOLD_READ_AHEAD;

struct MfFoldArgs : FoldExamples {  // (a row's examples in chain order)
  const double* F;   // the fixed side: Q, b_i for new users; P, b_u for new items
  const double* fb;
  double b;
  int32_t k;
  double lr, reg;
  int32_t n_passes;
  double* rows;  // [n_new][k] in / out
  double* bias;  // [n_new] in / out
};

struct FoldChain {
  int64_t e0, n, total;  // first example, examples, steps = n * n_passes
  int64_t step, e;       // the next step whose id is fetched, and its example
};

template <int VEC, int NC>
struct FoldSlot {
  FoldEx far;  // the step 2 * kFoldAhead ahead: id and weight on their way
  // the step kFoldAhead ahead: the fixed row and bias on their way
  Pack<VEC> q[NC];
  double fb, ry;
  bool live;  // the lane group has that step (its chain is not over)
};

template <int VEC, int NC>
__device__ __forceinline__ void fold_fetch_id(const MfFoldArgs& a, FoldChain& ch, FoldSlot<VEC, NC>& s) {
  s.far.live = ch.step < ch.total;
  s.far.j = 0;  // past the chain: row 0, a valid address
  s.far.ry = 0.0;
  if (s.far.live) {
    s.far.j = a.ids[ch.e0 + ch.e];
    s.far.ry = a.ry[ch.e0 + ch.e];
  }
  ++ch.step;
  if (++ch.e == ch.n) ch.e = 0;  // the next pass
}

template <int LPR, int VEC, int NC>
__device__ __forceinline__ void fold_fetch_row(const MfFoldArgs& a, int l, FoldSlot<VEC, NC>& s) {
  s.live = s.far.live;
  s.ry = s.far.ry;
  mf_load_row<LPR, VEC, NC>(s.q, a.F + int64_t(s.far.j) * a.k, a.k, l);
  s.fb = a.fb[s.far.j];
}

// one step on the row in registers; every lane of the wavefront takes part in the sum.  A chunk
// past k holds what mf_load_row put there (row[0 .. VEC), not zeros) and is updated along with the
// rest: it stays out of the dot product and mf_store_row never writes it.
template <int LPR, int VEC, int NC>
__device__ __forceinline__ void fold_step(const MfFoldArgs& a, int l, const FoldSlot<VEC, NC>& s,
                                          Pack<VEC> (&x)[NC], double& c) {
  double dot = 0.0;
#pragma unroll
  for (int ch = 0; ch < NC; ++ch) {
    const int f = (ch * LPR + l) * VEC;
    if (f < a.k) {
#pragma unroll
      for (int v = 0; v < VEC; ++v) dot += x[ch].v[v] * s.q[ch].v[v];
    }
  }
  dot = group_sum<LPR>(dot);
  const double err = s.ry - sigmoid_clipped(dot + c + s.fb + a.b);
#pragma unroll
  for (int ch = 0; ch < NC; ++ch) {
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      const double x_new = x[ch].v[v] - a.lr * (-err * s.q[ch].v[v] + a.reg * x[ch].v[v]);
      x[ch].v[v] = s.live ? x_new : x[ch].v[v];
    }
  }
  const double c_new = c - a.lr * (-err + a.reg * c);
  c = s.live ? c_new : c;
}

// the largest value among the 64 lanes, as a scalar
__device__ inline int64_t wave_max(int64_t v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const int64_t o = __shfl_xor(static_cast<long long>(v), m, 64);
    v = o > v ? o : v;
  }
  const uint32_t lo = __builtin_amdgcn_readfirstlane(int(uint32_t(v)));
  const uint32_t hi = __builtin_amdgcn_readfirstlane(int(uint32_t(uint64_t(v) >> 32)));
  return int64_t((uint64_t(hi) << 32) | lo);
}

template <int LPR, int VEC, int NC>
__global__ __launch_bounds__(kMfBlock) void mf_fold_kernel(MfFoldArgs a) {
  constexpr int GPB = kMfBlock / LPR;
  const int l = threadIdx.x % LPR;
  const int g = threadIdx.x / LPR;
  const int k = a.k;
  for (int64_t base = int64_t(blockIdx.x) * GPB; base < a.n_new; base += int64_t(gridDim.x) * GPB) {
    const bool valid = base + g < a.n_new;
    // a lane group without a row walks along on row 0 with a chain of no examples
    const int64_t r = valid ? int64_t(a.order[base + g]) : 0;
    FoldChain ch;
    ch.e0 = a.row_ptr[r];
    ch.n = valid ? a.row_ptr[r + 1] - ch.e0 : 0;
    ch.total = ch.n * a.n_passes;
    ch.step = ch.e = 0;
    const int64_t steps = wave_max(ch.total);
    Pack<VEC> x[NC];
    mf_load_row<LPR, VEC, NC>(x, a.rows + r * k, k, l);
    double c = a.bias[r];
    FoldSlot<VEC, NC> s[kFoldAhead];
#pragma unroll
    for (int d = 0; d < kFoldAhead; ++d) fold_fetch_id(a, ch, s[d]);
#pragma unroll
    for (int d = 0; d < kFoldAhead; ++d) {
      fold_fetch_row<LPR>(a, l, s[d]);
      fold_fetch_id(a, ch, s[d]);
    }
    for (int64_t t = 0; t < steps; t += kFoldAhead) {
#pragma unroll
      for (int d = 0; d < kFoldAhead; ++d) {
        if (t + d >= steps) break;
        fold_step<LPR>(a, l, s[d], x, c);
        fold_fetch_row<LPR>(a, l, s[d]);
        fold_fetch_id(a, ch, s[d]);
      }
    }
    if (valid) {
      mf_store_row<LPR, VEC, NC>(x, a.rows + r * k, k, l);
      if (l == 0) a.bias[r] = c;
    }
  }
}

}  // namespace rfm

using namespace rfm;

// Replica merge of the user-partitioned MF mode: every rank runs the
// exact sequential SGD on the examples of ITS users against its own replica of Q / b_i;
// after the batch the replicas' changes are added up.
//   delta: out = cur - sync                 (what this rank's examples changed)
//   merge: sync += total; cur = sync        (total = all ranks' deltas, all-reduced)
__global__ __launch_bounds__(256) void mf_delta_kernel(const double* cur, const double* sync,
                                                      double* out, int64_t n) {
  for (int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x; i < n; i += int64_t(gridDim.x) * 256)
    out[i] = cur[i] - sync[i];
}
__global__ __launch_bounds__(256) void mf_merge_kernel(double* cur, double* sync,
                                                      const double* total, int64_t n) {
  for (int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x; i < n; i += int64_t(gridDim.x) * 256) {
    const double v = sync[i] + total[i];
    sync[i] = v;
    cur[i] = v;
  }
}

extern "C" {

int32_t rfm_mf_predict(rfm_ctx* ctx, const int32_t* d_users, const int32_t* d_items,
                       const int32_t* d_row_ids, int64_t n_rows, const double* d_P,
                       const double* d_Q, const double* d_bu, const double* d_bi, double b,
                       int32_t n_factors, double* d_out_pred) {
  return mf_predict(ctx, d_users, d_items, nullptr, nullptr, d_row_ids, n_rows, d_P, d_Q, d_bu, d_bi,
                    b, n_factors, 0.0, d_out_pred, nullptr, false);
}

int32_t rfm_mf_predict_loss(rfm_ctx* ctx, const int32_t* d_users, const int32_t* d_items,
                            const double* d_y, const double* d_pscore,
                            const int32_t* d_row_ids, int64_t n_rows, const double* d_P,
                            const double* d_Q, const double* d_bu, const double* d_bi,
                            double b, int32_t n_factors, double eps, double* d_out_pred,
                            double* d_out_loss) {
  return mf_predict(ctx, d_users, d_items, d_y, d_pscore, d_row_ids, n_rows, d_P, d_Q, d_bu, d_bi, b,
                    n_factors, eps, d_out_pred, d_out_loss, true);
}

int32_t rfm_mf_sgd_levels(rfm_ctx* ctx, const int32_t* d_users, const int32_t* d_items,
                          const double* d_y, const double* d_pscore,
                          const int32_t* d_pos_rows, const int32_t* d_order,
                          const int32_t* h_level_ptr, const int32_t* d_level_ptr,
                          int32_t n_levels, double* d_P, double* d_Q, double* d_bu,
                          double* d_bi, double b, int32_t n_factors, double lr, double reg) {
  return guarded([&] {
    RFM_REQUIRE(ctx && d_users && d_items && d_y && d_pscore && d_pos_rows && d_order &&
                    h_level_ptr && d_level_ptr,
                "null pointer");
    RFM_REQUIRE(n_levels >= 0, "negative n_levels");
    const Shape s = shape_for(n_factors);
    MfSgdArgs a{};
    set_model(a, d_P, d_Q, d_bu, d_bi, b, n_factors, lr, reg);
    a.users = d_users;
    a.items = d_items;
    a.y = d_y;
    a.pscore = d_pscore;
    a.pos_rows = d_pos_rows;
    a.order = d_order;
    a.level_ptr = d_level_ptr;
    // a level is "small" when two passes of the sequential workgroup cover it
    mf_walk_levels(
        h_level_ptr, n_levels, 2 * (kSeqBlock / s.lpr), kNoLimit, kNoLimit,
        [&](int32_t rec_lo, int32_t rec_hi) {
          a.lo = rec_lo;
          a.hi = rec_hi;
          launch_wide(ctx, s, a);
        },
        [&](int32_t lev_lo, int32_t lev_hi) {
          a.lo = lev_lo;
          a.hi = lev_hi;
#define RFM_CALL_SEQ(L, Vv, N) \
  hipLaunchKernelGGL((mf_sgd_seq_kernel<L, Vv, N>), dim3(1), dim3(kSeqBlock), 0, ctx->stream, a)
          RFM_FOR_SHAPE(s, RFM_CALL_SEQ);
#undef RFM_CALL_SEQ
        });
    RFM_HIP_CHECK(hipGetLastError());
  });
}

int32_t rfm_mf_cache_capacity(int32_t n_factors, int32_t* h_out) {
  return guarded([&] {
    RFM_REQUIRE(h_out && n_factors >= 1, "bad arguments");
    *h_out = int32_t(std::min<int64_t>(1024, int64_t(kSeqMaxCacheBytes) / (int64_t(n_factors + 2) * 8)));
  });
}

}  // extern "C"

// rfm_mf_sgd_levels_ex (SgdRule) and rfm_mf_sgd_levels_opt under either rule: one schedule, one
// launch plan; an item cached under MfAdaGradRule takes twice the LDS (its accumulators)
template <class O>
static int32_t mf_levels_ex(rfm_ctx* ctx, const void* d_ex, const int32_t* h_level_ptr,
                            const int32_t* d_level_ptr, int32_t n_levels,
                            const int32_t* d_cache_items, int32_t n_cached, double* d_P,
                            double* d_Q, double* d_bu, double* d_bi, double b,
                            int32_t n_factors, double lr, double reg, const O& o) {
  return guarded([&] {
    RFM_REQUIRE(ctx && d_ex && h_level_ptr && d_level_ptr, "null pointer");
    RFM_REQUIRE(n_levels >= 0 && n_cached >= 0 && (n_cached == 0 || d_cache_items),
                "bad schedule");
    const Shape s = shape_for(n_factors);
    const size_t row_bytes = size_t(n_cached) * size_t(n_factors + 2) * sizeof(double);
    RFM_REQUIRE(row_bytes <= size_t(kSeqMaxCacheBytes),
                "item cache of %d rows exceeds %d bytes of LDS", n_cached, kSeqMaxCacheBytes);
    const size_t cache_bytes = row_bytes * (O::kAda ? 2 : 1);
    auto a = args_under(MfExArgs{}, o);
    set_model(a, d_P, d_Q, d_bu, d_bi, b, n_factors, lr, reg);
    a.ex = static_cast<const MfEx*>(d_ex);
    a.level_ptr = d_level_ptr;
    a.cache_items = d_cache_items;
    a.n_cached = n_cached;
    // a level is "small" when the sequential workgroup covers it in one pass; a launch takes a
    // run of them that fits the kernel's LDS tables
    const int seq_threads = seq_block(s.nc);
    mf_walk_levels(
        h_level_ptr, n_levels, seq_threads / s.lpr, kSeqMaxLevels, kSeqMaxRecs,
        [&](int32_t rec_lo, int32_t rec_hi) {
          a.lo = rec_lo;
          a.hi = rec_hi;
          const int grid = capped_grid(ctx, rec_hi - rec_lo, kMfBlock / s.lpr, 8, 0);
#define RFM_CALL_WIDE_EX(L, Vv, N)                                                            \
  hipLaunchKernelGGL((mf_sgd_wide_ex_kernel<L, Vv, N, O>), dim3(grid), dim3(kMfBlock), 0,     \
                     ctx->stream, a)
          RFM_FOR_SHAPE(s, RFM_CALL_WIDE_EX);
#undef RFM_CALL_WIDE_EX
        },
        [&](int32_t lev_lo, int32_t lev_hi) {
          a.lo = lev_lo;
          a.hi = lev_hi;
          a.rec_lo = h_level_ptr[lev_lo];
          a.rec_hi = h_level_ptr[lev_hi];
          const size_t lds = size_t((lev_hi - lev_lo + 2) / 2) * 8 +
                             size_t(a.rec_hi - a.rec_lo) * sizeof(MfEx) + cache_bytes;
#define RFM_CALL_SEQ_EX(L, Vv, N) launch_seq_ex<L, Vv, N, O>(ctx, a, mf_seq_threads<O>(N), lds)
          RFM_FOR_SHAPE(s, RFM_CALL_SEQ_EX);
#undef RFM_CALL_SEQ_EX
        });
    RFM_HIP_CHECK(hipGetLastError());
  });
}

extern "C" {

int32_t rfm_mf_sgd_levels_ex(rfm_ctx* ctx, const void* d_ex, const int32_t* h_level_ptr,
                             const int32_t* d_level_ptr, int32_t n_levels,
                             const int32_t* d_cache_items, int32_t n_cached, double* d_P,
                             double* d_Q, double* d_bu, double* d_bi, double b,
                             int32_t n_factors, double lr, double reg) {
  return mf_levels_ex(ctx, d_ex, h_level_ptr, d_level_ptr, n_levels, d_cache_items, n_cached, d_P, d_Q,
                      d_bu, d_bi, b, n_factors, lr, reg, SgdRule{});
}

int32_t rfm_mf_sgd_levels_opt(rfm_ctx* ctx, const void* d_ex, const int32_t* h_level_ptr,
                              const int32_t* d_level_ptr, int32_t n_levels,
                              const int32_t* d_cache_items, int32_t n_cached, double* d_P,
                              double* d_Q, double* d_bu, double* d_bi, double b,
                              int32_t n_factors, double lr, double reg, int32_t kind,
                              double* d_acc_P, double* d_acc_Q, double* d_acc_bu, double* d_acc_bi,
                              double eps) {
  bool ada = false;
  const int32_t rc = guarded([&] { ada = require_rule(kind, d_acc_P && d_acc_Q && d_acc_bu && d_acc_bi, eps); });
  if (rc != RFM_OK) return rc;
  if (!ada)
    return rfm_mf_sgd_levels_ex(ctx, d_ex, h_level_ptr, d_level_ptr, n_levels, d_cache_items, n_cached,
                                d_P, d_Q, d_bu, d_bi, b, n_factors, lr, reg);
  return mf_levels_ex(ctx, d_ex, h_level_ptr, d_level_ptr, n_levels, d_cache_items, n_cached, d_P, d_Q,
                      d_bu, d_bi, b, n_factors, lr, reg,
                      MfAdaGradRule{d_acc_P, d_acc_Q, d_acc_bu, d_acc_bi, eps});
}

int32_t rfm_mf_opt_geometry(const rfm_ctx*, int32_t kind, int32_t n_factors, int32_t* h_out7) {
  return guarded([&] {
    RFM_REQUIRE(h_out7, "null pointer");
    RFM_REQUIRE(kind == RFM_MF_OPT_SGD || kind == RFM_MF_OPT_ADAGRAD,
                "optimizer kind %d is neither SGD nor AdaGrad", kind);
    const Shape s = shape_for(n_factors);
    const bool ada = kind == RFM_MF_OPT_ADAGRAD;
    h_out7[0] = s.lpr;
    h_out7[1] = s.vec;
    h_out7[2] = s.nc;
    h_out7[3] = ada ? mf_seq_threads<MfAdaGradRule>(s.nc) : seq_block(s.nc);
    h_out7[4] = 0;  // the accumulators are read where they are used, in every class
    h_out7[5] = (n_factors + 2) * int32_t(sizeof(double)) * (ada ? 2 : 1);
    h_out7[6] = ada ? mf_ada_ring(s.vec, s.nc) : (s.nc <= 4 ? kMfAhead : 0);
  });
}

int32_t rfm_mf_sgd_levels_many(rfm_ctx* ctx, const void* d_ex, const int32_t* d_ex_rows,
                               const int32_t* h_level_ptr, const int32_t* d_level_ptr,
                               int32_t n_levels, const int32_t* d_cache_items, int32_t n_cached,
                               const rfm_mf_model* d_models, int32_t n_models, int32_t n_factors) {
  return guarded([&] {
    RFM_REQUIRE(ctx && d_ex && d_ex_rows && h_level_ptr && d_level_ptr && d_models, "null pointer");
    RFM_REQUIRE(n_models >= 1 && n_models <= RFM_MF_MAX_MODELS, "n_models=%d out of range (1..%d)",
                n_models, RFM_MF_MAX_MODELS);
    RFM_REQUIRE(n_levels >= 0 && n_cached >= 0 && (n_cached == 0 || d_cache_items),
                "bad schedule");
    const Shape s = shape_for(n_factors);
    const size_t cache_bytes = size_t(n_cached) * size_t(n_factors + 2) * sizeof(double);
    RFM_REQUIRE(cache_bytes <= size_t(kSeqMaxCacheBytes),
                "item cache of %d rows exceeds %d bytes of LDS", n_cached, kSeqMaxCacheBytes);
    MfManyArgs m{};
    m.ex = static_cast<const MfEx*>(d_ex);
    m.ex_rows = d_ex_rows;
    m.level_ptr = d_level_ptr;
    m.cache_items = d_cache_items;
    m.n_cached = n_cached;
    m.models = d_models;
    m.k = n_factors;
    // the launch plan of rfm_mf_sgd_levels_ex, each launch with a model dimension
    const int seq_threads = seq_block(s.nc);
    mf_walk_levels(
        h_level_ptr, n_levels, seq_threads / s.lpr, kSeqMaxLevels, kSeqMaxRecs,
        [&](int32_t rec_lo, int32_t rec_hi) {
          m.lo = rec_lo;
          m.hi = rec_hi;
          const int grid = capped_grid(ctx, rec_hi - rec_lo, kMfBlock / s.lpr, 8, 0);
#define RFM_CALL_WIDE_MANY(L, Vv, N)                                                              \
  hipLaunchKernelGGL((mf_sgd_wide_many_kernel<L, Vv, N>), dim3(grid, n_models), dim3(kMfBlock), 0, \
                     ctx->stream, m)
          RFM_FOR_SHAPE(s, RFM_CALL_WIDE_MANY);
#undef RFM_CALL_WIDE_MANY
        },
        [&](int32_t lev_lo, int32_t lev_hi) {
          m.lo = lev_lo;
          m.hi = lev_hi;
          m.rec_lo = h_level_ptr[lev_lo];
          m.rec_hi = h_level_ptr[lev_hi];
          const size_t lds = size_t((lev_hi - lev_lo + 2) / 2) * 8 +
                             size_t(m.rec_hi - m.rec_lo) * sizeof(MfEx) + cache_bytes;
#define RFM_CALL_SEQ_MANY(L, Vv, N) launch_seq_many<L, Vv, N>(ctx, m, n_models, seq_threads, lds)
          RFM_FOR_SHAPE(s, RFM_CALL_SEQ_MANY);
#undef RFM_CALL_SEQ_MANY
        });
    RFM_HIP_CHECK(hipGetLastError());
  });
}

int32_t rfm_mf_predict_many(rfm_ctx* ctx, const int32_t* d_users, const int32_t* d_items,
                            const int32_t* d_row_ids, int64_t n_rows, const rfm_mf_model* d_models,
                            int32_t n_models, int32_t n_factors, double* const* d_out_base,
                            int64_t out_offset) {
  return mf_predict_many(ctx, d_users, d_items, nullptr, d_row_ids, n_rows, d_models, n_models,
                         n_factors, 0.0, d_out_base, out_offset, nullptr, 0, false);
}

int32_t rfm_mf_predict_loss_many(rfm_ctx* ctx, const int32_t* d_users, const int32_t* d_items,
                                 const rfm_mf_labels* d_labels, const int32_t* d_row_ids,
                                 int64_t n_rows, const rfm_mf_model* d_models, int32_t n_models,
                                 int32_t n_factors, double eps, double* const* d_out_base,
                                 int64_t out_offset, double* d_out_loss, int64_t loss_stride) {
  return mf_predict_many(ctx, d_users, d_items, d_labels, d_row_ids, n_rows, d_models, n_models,
                         n_factors, eps, d_out_base, out_offset, d_out_loss, loss_stride, true);
}

int32_t rfm_mf_many_geometry(const rfm_ctx* ctx, int32_t n_models, int32_t n_factors, int64_t n_recs,
                             int32_t* h_out7) {
  return guarded([&] {
    RFM_REQUIRE(h_out7, "null pointer");
    RFM_REQUIRE(n_models >= 1 && n_models <= RFM_MF_MAX_MODELS, "n_models=%d out of range (1..%d)",
                n_models, RFM_MF_MAX_MODELS);
    RFM_REQUIRE(n_recs >= 0 && n_recs < (int64_t(1) << 31), "n_recs=%lld out of range", (long long)n_recs);
    const Shape s = shape_for(n_factors);
    const rfm_ctx assumed{};  // (the CU count of an MI355X)
    const rfm_ctx* c = ctx ? ctx : &assumed;
    h_out7[0] = seq_block(s.nc);
    h_out7[1] = s.lpr;
    h_out7[2] = n_models;
    h_out7[3] = capped_grid(c, n_recs, kMfBlock / s.lpr, 8, 0);
    h_out7[4] = n_models;
    h_out7[5] = capped_grid(c, n_recs, kMfBlock / s.lpr, 8, 1);
    h_out7[6] = n_models;
  });
}

int32_t rfm_mf_sgd_hogwild(rfm_ctx* ctx, const int32_t* d_users, const int32_t* d_items,
                           const double* d_y, const double* d_pscore,
                           const int32_t* d_pos_rows, int64_t batch, double* d_P, double* d_Q,
                           double* d_bu, double* d_bi, double b, int32_t n_factors, double lr,
                           double reg) {
  return guarded([&] {
    RFM_REQUIRE(ctx && d_users && d_items && d_y && d_pscore && d_pos_rows, "null pointer");
    RFM_REQUIRE(batch >= 0 && batch < (int64_t(1) << 31), "batch out of range");
    MfSgdArgs a{};
    set_model(a, d_P, d_Q, d_bu, d_bi, b, n_factors, lr, reg);
    if (batch == 0) return;
    a.users = d_users;
    a.items = d_items;
    a.y = d_y;
    a.pscore = d_pscore;
    a.pos_rows = d_pos_rows;
    a.order = nullptr;  // batch order, all examples at once
    a.lo = 0;
    a.hi = int32_t(batch);
    launch_wide(ctx, shape_for(n_factors), a);
    RFM_HIP_CHECK(hipGetLastError());
  });
}

int32_t rfm_mf_fold_geometry(const rfm_ctx* ctx, int64_t n_new, int32_t n_factors, int32_t* h_out6) {
  return guarded([&] {
    RFM_REQUIRE(h_out6, "null pointer");
    RFM_REQUIRE(n_new >= 0 && n_new < (int64_t(1) << 31), "n_new=%lld out of range", (long long)n_new);
    const Shape s = shape_for(n_factors);
    const rfm_ctx assumed{};  // (the CU count of an MI355X)
    fold_shape_out(s, kMfBlock, h_out6);
    h_out6[4] = capped_grid(ctx ? ctx : &assumed, n_new, kMfBlock / s.lpr, kFoldPerCu, 0);
    h_out6[5] = kFoldAhead;
  });
}

int32_t rfm_mf_fold_in(rfm_ctx* ctx, const int64_t* d_row_ptr, const int32_t* d_ids, const double* d_ry,
                       const int32_t* d_order, int64_t n_new, const double* d_F, const double* d_fb,
                       int64_t n_fixed, double b, int32_t n_factors, double lr, double reg,
                       int32_t n_passes, double* d_rows, double* d_bias) {
  return guarded([&] {
    Shape s;
    const FoldExamples x = fold_checked(ctx, d_row_ptr, d_ids, d_ry, d_order, n_new, n_fixed, n_factors, n_passes, &s);
    RFM_REQUIRE(d_row_ptr && d_ids && d_ry && d_order && d_F && d_fb && d_rows && d_bias, "null pointer");
    if (n_new == 0 || n_passes == 0) return;
    // (a lane group past its chain reads row 0 of the fixed side)
    RFM_REQUIRE(n_fixed >= 1, "a fixed side without rows");
    MfFoldArgs a{x};
    a.F = d_F;
    a.fb = d_fb;
    a.b = b;
    a.k = n_factors;
    a.lr = lr;
    a.reg = reg;
    a.n_passes = n_passes;
    a.rows = d_rows;
    a.bias = d_bias;
    const int grid = capped_grid(ctx, n_new, kMfBlock / s.lpr, kFoldPerCu, 0);
#define RFM_CALL_FOLD(L, Vv, N) \
  hipLaunchKernelGGL((mf_fold_kernel<L, Vv, N>), dim3(grid), dim3(kMfBlock), 0, ctx->stream, a)
    RFM_FOR_SHAPE(s, RFM_CALL_FOLD);
#undef RFM_CALL_FOLD
    RFM_HIP_CHECK(hipGetLastError());
  });
}

int32_t rfm_mf_delta(rfm_ctx* ctx, const double* d_cur, const double* d_sync, double* d_out,
                     int64_t count) {
  return guarded([&] {
    RFM_REQUIRE(ctx && count >= 0, "bad argument");
    if (count == 0) return;
    RFM_REQUIRE(d_cur && d_sync && d_out, "null pointer");
    const int grid = capped_grid(ctx, count, 256, 16, 0);
    hipLaunchKernelGGL(mf_delta_kernel, dim3(grid), dim3(256), 0, ctx->stream, d_cur, d_sync, d_out,
                       count);
    RFM_HIP_CHECK(hipGetLastError());
  });
}

int32_t rfm_mf_merge(rfm_ctx* ctx, double* d_cur, double* d_sync, const double* d_total,
                     int64_t count) {
  return guarded([&] {
    RFM_REQUIRE(ctx && count >= 0, "bad argument");
    if (count == 0) return;
    RFM_REQUIRE(d_cur && d_sync && d_total, "null pointer");
    const int grid = capped_grid(ctx, count, 256, 16, 0);
    hipLaunchKernelGGL(mf_merge_kernel, dim3(grid), dim3(256), 0, ctx->stream, d_cur, d_sync,
                       d_total, count);
    RFM_HIP_CHECK(hipGetLastError());
  });
}

}  // extern "C"
