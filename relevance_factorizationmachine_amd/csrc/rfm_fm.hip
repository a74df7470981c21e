// FM path of librfm_hip.so: launch side and C-ABI entry points of the forward, the training
// step, its dense and touched-row gradient forms, and the fit() loop.  The kernels are in
// rfm_fm_kernels.hpp / rfm_fm_rows.hpp, the training plan is built by rfm_fm_plan.hip
// (layout: rfm_fm_plan.h, rfm_fm_records.h; DESIGN.md sections 3 and 4).
//
// One training step (rfm_fm_step) is two launches on one stream:
//   1. fm_forward_kernel   rows of the batch in parallel: q_t = V^T x_t, logit, residual;
//                          writes Q, leaves {t, residual} marks + bitmap bits at the slots of
//                          the row's sparse-class entries and adds the hot entries'
//                          err_t x_tj [q_t, 1, x_tj] into the workgroup's LDS sums.
//   2. fm_consume_kernel   one task (a fixed number of 64-slot bitmap words) per lane group:
//                          lists the marked slots; the workgroup's marks are dealt evenly to
//                          its groups, each accumulates err_t x_tj [Q[t,:], 1, x_tj] of its
//                          part IN SLOT ORDER, updates the columns inside the part in place
//                          and combines columns that run over several parts of the workgroup
//                          in LDS; trailing workgroups reduce the hot columns' slabs and w0.
//  (3. fm_finalize_kernel  only for columns longer than a whole workgroup's tasks.)
// The only global float atomics are the no-return f64 adds to w[col] and w0 by the value's only
// writer of the step.  Sparse-class sums have a fixed order (bitwise reproducible);
// hot-class sums inside one workgroup are LDS atomics, so their last bits may vary from run
// to run (hot_min_count < 0 turns the class off).
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <memory>
#include <numeric>
#include <string>
#include <thread>

#include "rfm_common.h"
#include "rfm_fm_kernels.hpp"
#include "rfm_fm_plan.h"
#include "rfm_fm_rows.hpp"
#include "rfm_fm_sliced.hpp"

static_assert(RFM_MAX_FACTORS <= 1024, "fm_finalize_kernel's LDS totals hold 1024+2 values");

namespace rfm {

// The one decision of a forward launch (FwdForm).  What the rows and the factor count decide -- a
// plan-level question -- of `n_rows` rows through the plan's records or the caller's CSR arrays:
// 1024-thread workgroups whose lane groups keep several rows in flight once the batch fills the
// chip with them (one per CU: as few hot-sum slabs as possible), 256-thread / one-row ones otherwise ...
FwdForm forward_form(const rfm_ctx* ctx, int64_t n_rows, int k, bool records) {
  constexpr int per_cu = kBigBlock >= 1024 ? 1 : 2;
  FwdForm f{};
  f.shape = shape_for(k);
  f.lanes = f.shape.lpr;
  // (the plain forward -- the caller's CSR arrays: predict, validation loss -- takes the same two
  // shapes with its own number of rows per lane group)
  f.kind = records ? FwdKind::kRecords : FwdKind::kCsr;
  const int64_t rows_big = int64_t(kBigBlock / f.lanes) * forward_rows(kBigBlock, f.shape.nc, f.kind);
  // (measured on config 3: the many-rows shape wins from about a third of a chip of such
  // workgroups: 16 384 rows 26 vs 30 us, 8 192 rows 21 vs 20 us)
  const bool big = (n_rows + rows_big - 1) / rows_big * 2 >= int64_t(ctx->n_cu) * per_cu;
  f.block = big ? kBigBlock : kSmallBlock;
  f.rows = forward_rows(f.block, f.shape.nc, f.kind);
  f.trip = f.block / f.lanes * f.rows;
  f.grid = std::min(capped_grid(ctx, n_rows, f.trip, big ? per_cu : 8, 1), kMaxFwdGrid);
  return f;
}

// ... and what the arguments add: the kind, the kernel and its LDS
FwdForm forward_form(const rfm_ctx* ctx, const FwdArgs& a) {
  const bool recs = a.ent != nullptr || a.ell != nullptr;  // the plan's records
  FwdForm f = forward_form(ctx, a.n_rows, a.k, recs);
  const bool big = f.block == kBigBlock, riders = a.n_rows_x > 0;
  f.fixed = recs && a.hot_fixed && a.n_hot > 0;
  RFM_REQUIRE(!f.fixed || forward_form_exists(f.shape.lpr, f.shape.nc, f.block, FwdKind::kBlocksFixed),
              big ? "fixed-order hot sums are not built for this factor count at this batch"
                  : "fixed-order hot sums are not built for this factor count");
  RFM_REQUIRE(!riders || (recs && !big && !f.fixed), "this step cannot score extra rows");
  if (!recs) {
    f.kind = a.indptr2 ? FwdKind::kCsrPair : FwdKind::kCsr;
  } else if (a.ell) {
    // (a plan made for many-rows batches keeps only the padded row blocks: a step of fewer rows
    // on it reads those too)
    f.kind = f.fixed ? FwdKind::kBlocksFixed : riders ? FwdKind::kBlocksRiders : FwdKind::kBlocks;
  } else {
    RFM_REQUIRE(a.ent && a.rows, "the plan holds no row records");
    f.kind = f.fixed ? FwdKind::kRecordsFixed : riders ? FwdKind::kRecordsRiders : FwdKind::kRecords;
  }
  // the step's forward on padded row blocks, many-rows shape, arrival-order hot sums, k = 20 .. 32
  // in fours: 8 lanes x 4 factors per row, one row per lane group (the plan, the trip and the LDS
  // are those of 16 lanes)
  f.lanes8 = big && f.kind == FwdKind::kBlocks && forward_lanes8(a.k) && a.out_Q && a.slot_mark &&
             !a.loss_partial && a.ell_stride == int64_t(16 * sizeof(Entry));
  if (f.lanes8) {
    f.lanes = 8;
    f.rows = 1;
  }
  f.lds = forward_lds_bytes(f, a.n_hot, a.k);
  return f;
}

int forward_grid(const rfm_ctx* ctx, int64_t rows, int n_factors) {
  return forward_form(ctx, rows, n_factors, true).grid;
}

bool forward_many_rows(const rfm_ctx* ctx, int64_t rows, int n_factors) {
  return forward_form(ctx, rows, n_factors, true).block == kBigBlock;
}

bool forward_fixed_order_ok(const rfm_ctx* ctx, int64_t max_batch, int n_factors) {
  const FwdForm f = forward_form(ctx, max_batch, n_factors, true);  // (steps of fewer rows: the one-row shape)
  return forward_form_exists(f.shape.lpr, f.shape.nc, kSmallBlock, FwdKind::kBlocksFixed) &&
         forward_form_exists(f.shape.lpr, f.shape.nc, f.block, FwdKind::kBlocksFixed);
}

// one kernel: raises its dynamic-LDS limit when a launch needs more than the default
template <auto KERN>
void launch_forward_kernel(rfm_ctx* ctx, const FwdArgs& a, const FwdForm& f) {
  static LdsLimits allowed;
  allow_dynamic_lds(ctx, reinterpret_cast<const void*>(KERN), f.lds, allowed);
  hipLaunchKernelGGL(KERN, dim3(f.grid), dim3(f.block), f.lds, ctx->stream, a);
}

template <int L, int Vv, int N, int BLOCK, FwdKind K>
void launch_forward_as(rfm_ctx* ctx, const FwdArgs& a, const FwdForm& f) {
  if constexpr (forward_form_exists(L, N, BLOCK, K))
    launch_forward_kernel<&fm_forward_kernel<L, Vv, N, BLOCK, K>>(ctx, a, f);
  else
    RFM_REQUIRE(false, "forward kernel: form %d is not built at %d threads", int(K), BLOCK);
}

// the instantiation of a shape and block that f.kind names
template <int L, int Vv, int N, int BLOCK>
void launch_forward_kind(rfm_ctx* ctx, const FwdArgs& a, const FwdForm& f) {
#define RFM_KIND(K) case FwdKind::K: return launch_forward_as<L, Vv, N, BLOCK, FwdKind::K>(ctx, a, f)
  switch (f.kind) {
    RFM_KIND(kCsr); RFM_KIND(kCsrPair); RFM_KIND(kRecords); RFM_KIND(kBlocks);
    RFM_KIND(kRecordsFixed); RFM_KIND(kBlocksFixed); RFM_KIND(kRecordsRiders); RFM_KIND(kBlocksRiders);
  }
#undef RFM_KIND
}

// launches what `f` says (forward_form of a; a step with riding rows has added their workgroups)
void launch_forward(rfm_ctx* ctx, const FwdArgs& a, const FwdForm& f) {
  if (a.n_rows <= 0) return;
  RFM_REQUIRE(f.lds <= (160u << 10), "forward kernel: %zu bytes of LDS", f.lds);
  RFM_REQUIRE(!f.fixed || a.hot_rounds >= 1, "hot_rounds unset");
#define RFM_CALL_FWD(L, Vv, N)                                                \
  (f.block == kBigBlock ? launch_forward_kind<L, Vv, N, kBigBlock>(ctx, a, f) \
                        : launch_forward_kind<L, Vv, N, kSmallBlock>(ctx, a, f))
  if (f.lanes8)
    launch_forward_kernel<&fm_forward_lanes8_kernel<kBigBlock>>(ctx, a, f);
  else
    RFM_FOR_SHAPE(f.shape, RFM_CALL_FWD);
#undef RFM_CALL_FWD
  RFM_HIP_CHECK(hipGetLastError());
}

void launch_forward(rfm_ctx* ctx, const FwdArgs& a) {
  if (a.n_rows <= 0) return;
  launch_forward(ctx, a, forward_form(ctx, a));
}

// forward with loss whose partials go to `partial_row` (kMaxFwdGrid doubles) and are
// finished later, many launches at once; returns the number of partials written
int forward_loss_deferred(rfm_ctx* ctx, FwdArgs a, double* partial_row) {
  RFM_REQUIRE(a.n_rows > 0, "loss of zero rows");
  a.loss_partial = partial_row;
  const FwdForm f = forward_form(ctx, a);
  RFM_REQUIRE(f.grid <= kMaxFwdGrid, "forward grid %d exceeds %d", f.grid, kMaxFwdGrid);
  launch_forward(ctx, a, f);
  return f.grid;
}

// The two loss forwards of a fit() iteration in ONE launch (FwdKind::kCsrPair): rows a.row_ids[0 .. n_rows_a)
// of the training log (loss partials -> row_a) and every row of the validation log (-> row_b).  Returns the partials
// per row, or -1 when the rows together do not take the many-rows shape (the caller launches the two separately).
int forward_loss_pair_deferred(rfm_ctx* ctx, FwdArgs a, double* row_a, double* row_b) {
  RFM_REQUIRE(a.indptr2, "merged loss forward: no second log");
  a.loss_partial = row_a;
  a.loss_partial2 = row_b;
  const FwdForm f = forward_form(ctx, a);
  if (f.block != kBigBlock || f.grid > kMaxFwdGrid) return -1;
  launch_forward(ctx, a, f);
  return f.grid;
}

// forward with loss: partials in ctx scratch, finished into d_out_loss
void forward_loss(rfm_ctx* ctx, FwdArgs a, double* d_out_loss) {
  ctx->loss_partials.ensure(size_t(std::max(kMaxFwdGrid, ctx->n_cu * 8)) * sizeof(double));
  const int parts = forward_loss_deferred(ctx, a, ctx->loss_partials.as<double>());
  hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(kBlock), 0, ctx->stream,
                     ctx->loss_partials.as<double>(), parts, a.n_rows, d_out_loss);
  RFM_HIP_CHECK(hipGetLastError());
}

// Sliced loss forward (rfm_fm_sliced.hpp) over `rows` rows: workgroups per slice (one
// workgroup per CU, a multiple of the XCDs a slice is dealt to), rows per workgroup and per
// staged chunk, LDS.  ok = false: the plan has no slices, or the rows are too few to pay for
// every workgroup's copy of the cached columns (RFM_SLICED_MIN_ROWS, default 4 096;
// RFM_SLICED_LOSS=0: never).  `form_rows` (>= 0) takes that decision for another number of rows
// than the launch's: a shard of a log then scores its rows in the form the whole log would.
struct SlicedGeom {
  bool ok = false;
  int grid = 0, rows_per_wg = 0;
  size_t lds = 0;
};
SlicedGeom sliced_geom(const rfm_ctx* ctx, const rfm_fm_plan* plan, int64_t rows, int64_t form_rows = -1) {
  SlicedGeom g;
  if (plan->sl_ns <= 0 || env_int("RFM_SLICED_LOSS", 1) == 0) return g;
  if ((form_rows >= 0 ? form_rows : rows) < std::max(1, env_int("RFM_SLICED_MIN_ROWS", 4096))) return g;
  if (rows >= (int64_t(1) << 31) - 1) return g;  // (the kernel numbers a log's rows in 31 bits)
  const int xs = 8 / plan->sl_ns;
  int wps = std::max(xs, ctx->n_cu / plan->sl_ns / xs * xs);
  // (few rows: fewer, fuller workgroups -- each fills its own copy of the cached columns)
  const int64_t min_rows = kSlWaves * 4;
  while (wps > xs && rows / wps < min_rows) wps -= xs;
  g.rows_per_wg = int(std::min<int64_t>((rows + wps - 1) / wps, INT32_MAX));
  g.lds = sliced_lds_bytes(plan->sl_n_cached, plan->sl_sw);
  if (g.lds > size_t(kSlicedLds)) return g;
  g.grid = 8 * (wps / xs);
  g.ok = true;
  return g;
}

// the arguments of a sliced forward that the plan and the parameters give (the caller adds its logs)
SlicedArgs plan_sliced_args(const rfm_fm_plan* plan, const double* w0, const double* w, const double* V,
                            double* zpart) {
  SlicedArgs a{};
  a.tr_a = plan->sl_train.as<SlEnt>();
  a.pad = plan->sl_pad.as<SlEnt>();
  a.w0 = w0;
  a.w = w;
  a.V = V;
  a.k = plan->k;
  a.ns = plan->sl_ns;
  a.sw = plan->sl_sw;
  a.n_cached = plan->sl_n_cached;
  a.cached_cols = plan->sl_cols.as<int32_t>();
  a.cached_rank = plan->sl_rank.as<int32_t>();
  a.ml_log2 = plan->sl_ml_log2;
  a.zpart = zpart;
  return a;
}

void launch_sliced(rfm_ctx* ctx, const SlicedGeom& g, SlicedArgs a) {
  a.rows_per_wg = g.rows_per_wg;
  static LdsLimits allowed;
  allow_dynamic_lds(ctx, reinterpret_cast<const void*>(&fm_logit_slices_kernel), g.lds, allowed);
  hipLaunchKernelGGL(fm_logit_slices_kernel, dim3(g.grid), dim3(kSlBlock), g.lds, ctx->stream, a);
  RFM_HIP_CHECK(hipGetLastError());
}

}  // namespace rfm

using namespace rfm;

namespace {

void check_step_args(const rfm_fm_plan* plan, const void* indptr, const void* indices,
                     const void* values, const void* y, const void* p, const void* ids,
                     int64_t batch) {
  RFM_REQUIRE(plan, "null plan");
  // the step reads the plan's own records of the log; the caller's arrays are
  // only checked for presence (they are what the plan was built from)
  RFM_REQUIRE(indptr && indices && values && y && p && ids, "null pointer");
  RFM_REQUIRE(batch >= 1 && batch <= plan->max_batch, "batch=%lld outside 1..max_batch=%lld",
              (long long)batch, (long long)plan->max_batch);
}

// RFM_CHECK_IDS=1 (debugging aid; synchronises): the ids of every one of the n_iters
// batches must be rows of the plan's log and distinct within their batch
void validate_ids(rfm_ctx* ctx, rfm_fm_plan* plan, const int32_t* d_ids, int64_t batch,
                  int64_t n_iters) {
  if (env_int("RFM_CHECK_IDS", 0) == 0 || batch <= 0 || n_iters <= 0) return;
  if (!plan->ids_seen.p || plan->ids_stamp > INT32_MAX - n_iters - 2) {
    plan->ids_seen.ensure(size_t(plan->n_rows) * 4);
    plan->ids_flags.ensure(8);
    RFM_HIP_CHECK(hipMemsetAsync(plan->ids_seen.p, 0, plan->ids_seen.bytes, ctx->stream));
    plan->ids_stamp = 0;
  }
  RFM_HIP_CHECK(hipMemsetAsync(plan->ids_flags.p, 0, 8, ctx->stream));
  const int64_t total = batch * n_iters;
  const int grid = capped_grid(ctx, total, kBlock, 8, 0);
  hipLaunchKernelGGL(ids_check_kernel, dim3(grid), dim3(kBlock), 0, ctx->stream, d_ids, batch,
                     n_iters, plan->n_rows, plan->ids_seen.as<int32_t>(), plan->ids_stamp + 1,
                     plan->ids_flags.as<int32_t>());
  plan->ids_stamp += int32_t(n_iters);
  int32_t flags[2] = {0, 0};
  RFM_HIP_CHECK(hipMemcpyAsync(flags, plan->ids_flags.p, 8, hipMemcpyDeviceToHost, ctx->stream));
  RFM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  RFM_REQUIRE(!flags[0], "a row id lies outside the plan's log (0..%lld)", (long long)plan->n_rows - 1);
  RFM_REQUIRE(!flags[1], "a row id occurs twice in one batch: the ids of a step must be distinct");
}

// rows of the plan's log that a step's forward launch scores on the side (fm_forward_kernel, the ...Riders kinds)
struct XtraRows {
  const int32_t* ids;  // rows ids[0 .. n) of the plan's log ...
  int64_t n;
  double* out_pred;
  const RowRec* rows_y;  // ... and every row of another log given as records (n_y = 0: none)
  const Entry* ent_y;
  int64_t n_y;
  double* out_pred_y;
};

// a forward of rows ids[0 .. n) of the plan's log, through the plan's records
FwdArgs plan_fwd_args(const rfm_fm_plan* plan, const int32_t* ids, int64_t n, const double* w0,
                      const double* w, const double* V) {
  FwdArgs f{};
  f.ent = plan->ent.as<Entry>();
  f.rows = plan->rows.as<RowRec>();
  f.ell = plan->ell.as<char>();
  f.ell_stride = plan->ell_stride;
  f.ell_yp = plan->ell_yp.as<double2>();
  f.row_ids = ids;
  f.n_rows = n;
  f.w0 = w0;
  f.w = w;
  f.V = V;
  f.k = plan->k;
  return f;
}

// ... of a step: it leaves Q rows, marks, hot sums and residual sums (the caller adds the slot bitmap)
FwdArgs step_fwd_args(const rfm_fm_plan* plan, const int32_t* ids, int64_t n, const double* w0,
                      const double* w, const double* V) {
  FwdArgs f = plan_fwd_args(plan, ids, n, w0, w, V);
  f.out_Q = plan->Q.as<double>();
  f.slot_mark = plan->slot_t.as<SlotMark>();
  f.n_hot = plan->n_hot;
  f.hot_rounds = plan->hot_rounds;
  f.hot_fixed = plan->hot_fixed ? 1 : 0;
  f.hot_slab = plan->hot_slab.as<double>();
  f.err_partial = plan->err_partial.as<double>();
  return f;
}

// the step's forward launch: its own workgroups (returned: one hot-sum slab each), then those that
// score the extra rows riding along
int launch_step_forward(rfm_ctx* ctx, FwdArgs f, const XtraRows* xtra) {
  if (xtra && xtra->n > 0) {
    f.row_ids_x = xtra->ids;
    f.n_rows_x = xtra->n;
    f.out_pred_x = xtra->out_pred;
  }
  const FwdForm own = forward_form(ctx, f);  // (fails for riding rows on a step that cannot score them)
  FwdForm launch = own;
  if (f.n_rows_x > 0) {
    const FwdForm gx = forward_form(ctx, xtra->n, f.k, true);
    RFM_REQUIRE(gx.block == kSmallBlock, "extra rows: unexpected geometry");
    f.grid_main = own.grid;
    f.grid_x = gx.grid;
    launch.grid += gx.grid;
    if (xtra->n_y > 0) {
      const FwdForm gy = forward_form(ctx, xtra->n_y, f.k, true);
      RFM_REQUIRE(gy.block == kSmallBlock && f.ent && f.rows, "extra log: unexpected geometry / plan form");
      f.rows_y = xtra->rows_y;
      f.ent_y = xtra->ent_y;
      f.n_rows_y = xtra->n_y;
      f.out_pred_y = xtra->out_pred_y;
      launch.grid += gy.grid;
    }
  }
  ctx->prof_mark();
  launch_forward(ctx, f, launch);
  ctx->prof_mark();
  return own.grid;
}

// the step's consume launch (fm_consume_kernel): the slot-ordered sums and the updates under
// the rule o
template <class O>
void launch_consume(rfm_ctx* ctx, ConsArgs c, const Shape& s, const O& o) {
  const int grid = c.nb_tasks + c.n_hot + 1;  // tasks, then the hot columns, then w0
  const size_t lds = consume_lds_bytes(s.lpr, c.c.k);
  if (s.nc > 1) {
    // one workgroup per (four tasks, chunk of 64 lanes x vec factors)
    const int n_chunks = fm_chunks(c.c.k, s.vec);
    c.n_chunks = n_chunks;
    // chunks dealt to XCDs (see the kernel): every chunk gets at least 8 / n_chunks XCDs
    c.xcd_chunks = n_chunks <= 8 ? 1 : 0;
    const int per_chunk = 8 / n_chunks;  // (the fewest XCDs a chunk gets)
    const dim3 g2 = c.xcd_chunks ? dim3(8 * ((grid + per_chunk - 1) / per_chunk)) : dim3(grid, n_chunks);
    const auto a = args_under(c, o);
    if (s.vec == 2)
      hipLaunchKernelGGL((fm_consume_kernel<64, 2, true, O>), g2, dim3(kBlock), lds, ctx->stream, a);
    else
      hipLaunchKernelGGL((fm_consume_kernel<64, 1, true, O>), g2, dim3(kBlock), lds, ctx->stream, a);
  } else {
    const auto a = args_under(c, o);
#define RFM_CALL_CONS(L, Vv, N) \
  hipLaunchKernelGGL((fm_consume_kernel<L, Vv, false, O>), dim3(grid), dim3(kBlock), lds, ctx->stream, a)
    RFM_FOR_SINGLE_CHUNK_SHAPE(s, RFM_CALL_CONS);
#undef RFM_CALL_CONS
  }
  RFM_HIP_CHECK(hipGetLastError());
}

// the finalize launch of the columns cut into several tasks
template <class O>
void launch_finalize(rfm_ctx* ctx, const FinArgs& fa, const Shape& s, const O& o) {
  const int gpb = kBlock / s.lpr;
  const int nb_short = (fa.n_split_short + gpb - 1) / gpb;
  const int grid = nb_short + fa.n_split_long;
  const auto a = args_under(fa, o);
  if (s.nc > 1) {
    const dim3 g2(grid, fm_chunks(fa.c.k, s.vec));
    if (s.vec == 2)
      hipLaunchKernelGGL((fm_finalize_chunk_kernel<2, O>), g2, dim3(kBlock), 0, ctx->stream, a, nb_short);
    else
      hipLaunchKernelGGL((fm_finalize_chunk_kernel<1, O>), g2, dim3(kBlock), 0, ctx->stream, a, nb_short);
  } else {
#define RFM_CALL_FIN(L, Vv, N) \
  hipLaunchKernelGGL((fm_finalize_kernel<L, Vv, O>), dim3(grid), dim3(kBlock), 0, ctx->stream, a, nb_short)
    RFM_FOR_SINGLE_CHUNK_SHAPE(s, RFM_CALL_FIN);
#undef RFM_CALL_FIN
  }
  RFM_HIP_CHECK(hipGetLastError());
}

// launches 2 and 3 of a step under the rule o: the consume launch, then the partial rows of the
// columns cut into several tasks (none on most plans)
template <class O>
void launch_updates(rfm_ctx* ctx, const rfm_fm_plan* plan, const ConsArgs& c, const Shape& s, const O& o) {
  launch_consume(ctx, c, s, o);
  ctx->prof_mark();
  if (plan->n_split_short + plan->n_split_long > 0) {
    FinArgs fa{};
    fa.c = c.c;
    fa.split = plan->split.as<SplitCol>();
    fa.n_split_short = plan->n_split_short;
    fa.n_split_long = plan->n_split_long;
    launch_finalize(ctx, fa, s, o);
  }
  ctx->prof_mark();
}

// the launches of one step; grad == nullptr -> update in place
void enqueue_step(rfm_ctx* ctx, rfm_fm_plan* plan, const int32_t* d_row_ids, int64_t batch, double* d_w0,
                  double* d_w, double* d_V, double lr, double* d_grad, int32_t* d_touch = nullptr,
                  int32_t touch_id = 0, const XtraRows* xtra = nullptr) {
  const int k = plan->k;
  const Shape s = shape_for(k);
  FwdArgs f = step_fwd_args(plan, d_row_ids, batch, d_w0, d_w, d_V);
  // more than one chunk per lane: the slot bitmap alternates between two buffers by step
  // parity (see fm_consume_kernel, CH form)
  const bool chunked = s.nc > 1;
  const int64_t parity = chunked ? ((plan->step + 1) & 1) : 0;
  unsigned long long* bits = plan->slot_bits.as<unsigned long long>() + parity * plan->bits_words;
  unsigned long long* bits_other =
      plan->slot_bits.as<unsigned long long>() + (1 - parity) * plan->bits_words;
  f.slot_bits = bits;
  const int n_slabs = launch_step_forward(ctx, f, xtra);

  if (d_grad && !d_touch) {  // dense gradient: every element is written
    const size_t bytes = (size_t(plan->n_features) * (k + 1) + 1) * sizeof(double);
    RFM_HIP_CHECK(hipMemsetAsync(d_grad, 0, bytes, ctx->stream));
  }
  ColArgs col{};  // what both launches need to finish a column
  col.V = d_V;
  col.w = d_w;
  col.k = k;
  col.n = plan->n_features;
  col.lr = lr;
  col.grad = d_grad;
  col.touch = d_touch;
  col.touch_id = touch_id;
  col.parts = plan->parts.as<double>();
  col.stamp = double(++plan->step);
  ConsArgs c{};
  c.c = col;
  c.tasks = plan->tasks.as<TaskRec>();
  c.task_words = plan->task_words;
  c.pool = consume_pools(plan->task_words, plan->max_batch, plan->n_rows) ? 1 : 0;
  c.slot_bits = bits;
  c.slot_bits_other = bits_other;
  c.slot_mark = plan->slot_t.as<SlotMark>();
  c.slots = plan->slots.as<SlotRec>();
  c.Q = plan->Q.as<double>();
  c.w0 = d_w0;
  c.nb_tasks = plan->n_task_blocks;  // one task per lane group
  c.n_hot = plan->n_hot;
  c.hot_cols = plan->hot_cols.as<int32_t>();
  c.hot_slab = plan->hot_slab.as<double>();
  c.n_slabs = n_slabs;
  c.err_partial = plan->err_partial.as<double>();
  // the rule of the plan (rfm_fm_plan_set_optimizer); gradient mode forms g alone, under any rule
  if (!d_grad && plan->opt_kind == RFM_FM_OPT_ADAGRAD)
    launch_updates(ctx, plan, c, s, AdaGradRule{plan->opt_acc_V, plan->opt_acc_w, plan->opt_acc_w0, plan->opt_eps});
  else
    launch_updates(ctx, plan, c, s, SgdRule{});
}

FwdArgs forward_args(const int64_t* d_indptr, const int32_t* d_indices, const double* d_values,
                     const int32_t* d_row_ids, int64_t n_rows, const double* d_w0,
                     const double* d_w, const double* d_V, int32_t k) {
  FwdArgs f{};
  f.indptr = d_indptr;
  f.indices = d_indices;
  f.values = d_values;
  f.row_ids = d_row_ids;
  f.n_rows = n_rows;
  f.w0 = d_w0;
  f.w = d_w;
  f.V = d_V;
  f.k = k;
  return f;
}

// The loss partials of a run of iterations of a fit() loop (rfm_fm_train, rfm_fm_fit_dp): one row
// of kMaxFwdGrid per-workgroup partials per iteration and loss in plan->loss_rows, finished by one
// launch per run and loss (fixed order inside an iteration, as loss_finish_kernel does it).  A run
// closed with `hold` is finished after the next step instead (finish_pending).
constexpr int64_t kRun = 128;  // iterations of a run at most
struct LossRun {
  double* train_rows;
  double* val_rows;
  int train_parts = 0, val_parts = 0;  // partials per row
  int64_t first = 0;                   // the open run's first iteration
  int64_t pending_first = -1, pending_count = 0;

  LossRun(rfm_fm_plan* plan, bool any) {
    if (any) plan->loss_rows.ensure(size_t(2 * kRun) * size_t(kMaxFwdGrid) * sizeof(double));
    train_rows = plan->loss_rows.as<double>();
    val_rows = train_rows + kRun * kMaxFwdGrid;
  }
  int64_t slot(int64_t it) const { return it - first; }
  double* train_row(int64_t it) const { return train_rows + slot(it) * kMaxFwdGrid; }
  double* val_row(int64_t it) const { return val_rows + slot(it) * kMaxFwdGrid; }

  // after iteration `it`: a run that has reached run_len iterations is finished (or held)
  template <class Finish>
  void close(int64_t it, int64_t run_len, bool hold, Finish&& finish) {
    if (it - first + 1 != run_len) return;
    if (hold) {
      pending_first = first;
      pending_count = run_len;
    } else {
      finish(first, run_len);
    }
    first = it + 1;
  }
  template <class Finish>
  void finish_pending(Finish&& finish) {
    if (pending_count <= 0) return;
    finish(pending_first, pending_count);
    pending_count = 0;
  }
  template <class Finish>
  void finish_open(int64_t n_iters, Finish&& finish) {
    if (n_iters > first) finish(first, n_iters - first);
  }

  // iterations first .. first + count into the means of n_* rows (rfm_fm_train) or into sums (a
  // rank's part, rfm_fm_fit_dp); a null output: that loss is not asked for
  void finish_means(rfm_ctx* ctx, int64_t first, int64_t count, int64_t n_train, double* out_train,
                    int64_t n_val, double* out_val) const {
    if (out_train)
      hipLaunchKernelGGL(loss_finish_many_kernel, dim3(int(count)), dim3(kBlock), 0, ctx->stream,
                         train_rows, int64_t(kMaxFwdGrid), train_parts, n_train, out_train + first);
    if (out_val)
      hipLaunchKernelGGL(loss_finish_many_kernel, dim3(int(count)), dim3(kBlock), 0, ctx->stream,
                         val_rows, int64_t(kMaxFwdGrid), val_parts, n_val, out_val + first);
    RFM_HIP_CHECK(hipGetLastError());
  }
  void finish_sums(rfm_ctx* ctx, int64_t first, int64_t count, double* sums_train, double* sums_val) const {
    if (sums_train)
      hipLaunchKernelGGL(loss_sum_many_kernel, dim3(int(count)), dim3(kBlock), 0, ctx->stream, train_rows,
                         int64_t(kMaxFwdGrid), train_parts, sums_train + first);
    if (sums_val)
      hipLaunchKernelGGL(loss_sum_many_kernel, dim3(int(count)), dim3(kBlock), 0, ctx->stream, val_rows,
                         int64_t(kMaxFwdGrid), val_parts, sums_val + first);
    RFM_HIP_CHECK(hipGetLastError());
  }
};

// scores of the rows of a CSR through the plan, in the form `form_rows` rows would take (-1: n_rows)
void plan_forward(rfm_ctx* ctx, rfm_fm_plan* plan, const int64_t* d_indptr, const int32_t* d_indices,
                  const double* d_values, int64_t n_rows, const double* d_w0, const double* d_w,
                  const double* d_V, double* d_out_pred, int64_t form_rows = -1);

}  // namespace

#include "rfm_fm_dp.hpp"

extern "C" {

int32_t rfm_fm_forward(rfm_ctx* ctx, const int64_t* d_indptr, const int32_t* d_indices,
                       const double* d_values, const int32_t* d_row_ids, int64_t n_rows,
                       const double* d_w0, const double* d_w, const double* d_V,
                       int64_t n_features, int32_t n_factors, double* d_out_pred) {
  return guarded([&] {
    RFM_REQUIRE(ctx, "null ctx");
    RFM_REQUIRE(n_rows >= 0 && n_rows < (int64_t(1) << 31) && n_features >= 1, "bad shape");
    if (n_rows == 0) return;  // nothing to score (empty inputs carry null pointers)
    RFM_REQUIRE(d_indptr && d_w0 && d_w && d_V && d_out_pred, "null pointer");
    RFM_REQUIRE(d_indices && d_values, "null CSR arrays");
    FwdArgs f = forward_args(d_indptr, d_indices, d_values, d_row_ids, n_rows, d_w0, d_w, d_V,
                             n_factors);
    f.out_pred = d_out_pred;
    launch_forward(ctx, f);
  });
}

int32_t rfm_ips_logloss(rfm_ctx* ctx, const double* d_y, const double* d_pred,
                        const double* d_pscore, const int32_t* d_row_ids, int64_t n_rows,
                        double eps, double* d_out_loss) {
  return guarded([&] {
    RFM_REQUIRE(ctx && d_y && d_pred && d_pscore && d_out_loss, "null pointer");
    RFM_REQUIRE(n_rows >= 1, "loss of zero rows");
    const int grid = capped_grid(ctx, n_rows, kBlock, 8, 0);
    ctx->loss_partials.ensure(size_t(std::max(kMaxFwdGrid, ctx->n_cu * 8)) * sizeof(double));
    hipLaunchKernelGGL(logloss_kernel, dim3(grid), dim3(kBlock), 0, ctx->stream, d_y, d_pred,
                       d_pscore, d_row_ids, n_rows, eps, ctx->loss_partials.as<double>());
    hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(kBlock), 0, ctx->stream,
                       ctx->loss_partials.as<double>(), grid, n_rows, d_out_loss);
    RFM_HIP_CHECK(hipGetLastError());
  });
}

int32_t rfm_fm_forward_loss(rfm_ctx* ctx, const int64_t* d_indptr, const int32_t* d_indices,
                            const double* d_values, const double* d_y, const double* d_pscore,
                            const int32_t* d_row_ids, int64_t n_rows, const double* d_w0,
                            const double* d_w, const double* d_V, int64_t n_features,
                            int32_t n_factors, double eps, double* d_out_pred,
                            double* d_out_loss) {
  return guarded([&] {
    RFM_REQUIRE(ctx && d_indptr && d_indices && d_values && d_y && d_pscore && d_w0 && d_w &&
                    d_V && d_out_loss,
                "null pointer");
    RFM_REQUIRE(n_rows >= 1 && n_rows < (int64_t(1) << 31) && n_features >= 1, "bad shape");
    FwdArgs f = forward_args(d_indptr, d_indices, d_values, d_row_ids, n_rows, d_w0, d_w, d_V,
                             n_factors);
    f.y = d_y;
    f.pscore = d_pscore;
    f.eps = eps;
    f.out_pred = d_out_pred;
    forward_loss(ctx, f, d_out_loss);
  });
}

int32_t rfm_fm_step(rfm_ctx* ctx, rfm_fm_plan* plan, const int64_t* d_indptr,
                    const int32_t* d_indices, const double* d_values, const double* d_y,
                    const double* d_pscore, const int32_t* d_row_ids, int64_t batch,
                    double* d_w0, double* d_w, double* d_V, double lr) {
  return guarded([&] {
    RFM_REQUIRE(ctx && d_w0 && d_w && d_V, "null pointer");
    check_step_args(plan, d_indptr, d_indices, d_values, d_y, d_pscore, d_row_ids, batch);
    validate_ids(ctx, plan, d_row_ids, batch, 1);
    enqueue_step(ctx, plan, d_row_ids, batch, d_w0, d_w, d_V, lr, nullptr);
  });
}

int32_t rfm_fm_grad(rfm_ctx* ctx, rfm_fm_plan* plan, const int64_t* d_indptr,
                    const int32_t* d_indices, const double* d_values, const double* d_y,
                    const double* d_pscore, const int32_t* d_row_ids, int64_t batch,
                    const double* d_w0, const double* d_w, const double* d_V, double* d_grad) {
  return guarded([&] {
    RFM_REQUIRE(ctx && d_w0 && d_w && d_V && d_grad, "null pointer");
    check_step_args(plan, d_indptr, d_indices, d_values, d_y, d_pscore, d_row_ids, batch);
    validate_ids(ctx, plan, d_row_ids, batch, 1);
    enqueue_step(ctx, plan, d_row_ids, batch, const_cast<double*>(d_w0), const_cast<double*>(d_w),
                 const_cast<double*>(d_V), 0.0, d_grad);
  });
}

int32_t rfm_fm_apply(rfm_ctx* ctx, double* d_w0, double* d_w, double* d_V,
                     const double* d_grad, int64_t n_features, int32_t n_factors, double lr) {
  return guarded([&] {
    RFM_REQUIRE(ctx && d_w0 && d_w && d_V && d_grad, "null pointer");
    RFM_REQUIRE(n_features >= 1 && n_factors >= 1, "bad shape");
    const int64_t nk = n_features * int64_t(n_factors);
    const int64_t total = nk + n_features + 1;
    const int grid = capped_grid(ctx, total, kBlock, 16, 0);
    hipLaunchKernelGGL(fm_apply_kernel, dim3(grid), dim3(kBlock), 0, ctx->stream, d_V, d_w, d_w0,
                       d_grad, nk, n_features, lr);
    RFM_HIP_CHECK(hipGetLastError());
  });
}

// ---------------------------------------------------------------------------
// touched-row gradients and their exchange (SURVEY.md 8e option 1)
// ---------------------------------------------------------------------------
int32_t rfm_fm_grad_rows(rfm_ctx* ctx, rfm_fm_plan* plan, const int32_t* d_row_ids, int64_t batch,
                         const double* d_w0, const double* d_w, const double* d_V, double* d_rows,
                         int64_t cap_rows, int32_t* d_n_rows, double* d_gw0,
                         const int32_t* d_range_lo, int32_t n_ranges, int32_t* d_range_bounds) {
  return guarded([&] {
    RFM_REQUIRE(ctx && plan && d_w0 && d_w && d_V && d_rows && d_n_rows && d_gw0, "null pointer");
    RFM_REQUIRE(batch >= 0 && batch <= plan->max_batch, "batch=%lld outside 0..max_batch=%lld",
                (long long)batch, (long long)plan->max_batch);
    RFM_REQUIRE(batch == 0 || d_row_ids, "null row ids");
    RFM_REQUIRE(cap_rows >= 0, "negative capacity");
    RFM_REQUIRE(n_ranges >= 0 && n_ranges <= kMaxRanges, "n_ranges=%d outside 0..%d", n_ranges,
                kMaxRanges);
    RFM_REQUIRE(n_ranges == 0 || (d_range_lo && d_range_bounds), "null range arrays");
    const int32_t id = next_touch_ids(ctx, plan, 1);
    validate_ids(ctx, plan, d_row_ids, batch, 1);
    enqueue_grad_rows(ctx, plan, id, d_row_ids, batch, d_w0, d_w, d_V, d_rows, cap_rows, d_n_rows,
                      d_gw0, d_range_lo, n_ranges, d_range_bounds);
  });
}

int32_t rfm_fm_apply_rows(rfm_ctx* ctx, const double* d_rows, const int32_t* d_n_rows,
                          int64_t cap_rows, const double* d_gw0, double* d_w0, double* d_w,
                          double* d_V, int64_t n_features, int32_t n_factors, double lr) {
  return guarded([&] {
    RFM_REQUIRE(ctx && d_rows && d_n_rows && d_w0 && d_w && d_V, "null pointer");
    RFM_REQUIRE(n_features >= 1 && n_factors >= 1 && cap_rows >= 0, "bad shape");
    const int grid = capped_grid(ctx, cap_rows, kBlock / kWave, 8, 1);
    hipLaunchKernelGGL(rows_apply_kernel, dim3(grid), dim3(kBlock), 0, ctx->stream, d_rows,
                       d_n_rows, cap_rows, d_gw0, d_w0, d_w, d_V, n_features, int(n_factors), lr);
    RFM_HIP_CHECK(hipGetLastError());
  });
}

int32_t rfm_fm_reduce_rows(rfm_ctx* ctx, const double* d_rows, const int32_t* d_seg_ptr,
                           int32_t n_segments, int64_t total_rows, const double* d_w,
                           const double* d_V, int64_t n_features, int32_t n_factors, double lr,
                           double* d_out_rows) {
  return guarded([&] {
    RFM_REQUIRE(ctx && d_seg_ptr && d_w && d_V, "null pointer");
    RFM_REQUIRE(n_segments >= 1 && n_segments <= kWave, "n_segments=%d outside 1..%d", n_segments,
                kWave);
    RFM_REQUIRE(n_features >= 1 && n_factors >= 1 && total_rows >= 0, "bad shape");
    if (total_rows == 0) return;
    RFM_REQUIRE(d_rows && d_out_rows, "null record lists");
    const int grid = capped_grid(ctx, total_rows, kBlock / kWave, 8, 0);
    hipLaunchKernelGGL(rows_reduce_kernel, dim3(grid), dim3(kBlock), 0, ctx->stream, d_rows,
                       d_seg_ptr, int(n_segments), d_w, d_V, n_features, int(n_factors), lr,
                       d_out_rows);
    RFM_HIP_CHECK(hipGetLastError());
  });
}

int32_t rfm_fm_set_rows(rfm_ctx* ctx, const double* d_rows, int64_t n_rows,
                        const double* d_gw0_parts, int32_t n_parts, int64_t part_stride,
                        double* d_w0, double* d_w, double* d_V, int64_t n_features,
                        int32_t n_factors, double lr) {
  return guarded([&] {
    RFM_REQUIRE(ctx && d_w0 && d_w && d_V, "null pointer");
    RFM_REQUIRE(n_features >= 1 && n_factors >= 1 && n_rows >= 0 && n_parts >= 0, "bad shape");
    RFM_REQUIRE(n_rows == 0 || d_rows, "null record list");
    RFM_REQUIRE(n_parts == 0 || d_gw0_parts, "null g_w0 partials");
    if (n_rows == 0 && n_parts == 0) return;
    const int grid = capped_grid(ctx, n_rows, kBlock / kWave, 8, 1);
    hipLaunchKernelGGL(rows_set_kernel, dim3(grid), dim3(kBlock), 0, ctx->stream, d_rows, n_rows,
                       n_parts ? d_gw0_parts : nullptr, int(n_parts), part_stride, d_w0, d_w, d_V,
                       n_features, int(n_factors), lr);
    RFM_HIP_CHECK(hipGetLastError());
  });
}

}  // extern "C"

namespace {

// scores of the rows of a CSR through the plan (rfm_fm_plan_forward): the sliced forward where
// the plan has one and the rows (form_rows, when given) are enough for it, else the plain one.  A
// row's score does not depend on the other rows of the launch, only on the form.
void plan_forward(rfm_ctx* ctx, rfm_fm_plan* plan, const int64_t* d_indptr, const int32_t* d_indices,
                  const double* d_values, int64_t n_rows, const double* d_w0, const double* d_w,
                  const double* d_V, double* d_out_pred, int64_t form_rows) {
  if (n_rows == 0) return;
  const SlicedGeom sliced = sliced_geom(ctx, plan, n_rows, form_rows);
  if (!sliced.ok) {  // the plain forward (rfm_fm_forward)
    FwdArgs f = forward_args(d_indptr, d_indices, d_values, nullptr, n_rows, d_w0, d_w, d_V, plan->k);
    f.out_pred = d_out_pred;
    launch_forward(ctx, f);
    return;
  }
  rfm_fm_plan::SlLog& log = plan->sl_log[1];
  if (!log.holds(d_indptr, d_indices, d_values, n_rows)) {
    log.rows = -1;
    sliced_translate(ctx, plan, d_indptr, d_indices, d_values, n_rows, log.tr);
  }
  plan->sl_zf.ensure(size_t(plan->sl_ns) * size_t(n_rows) * 8);
  SlicedArgs f = plan_sliced_args(plan, d_w0, d_w, d_V, plan->sl_zf.as<double>());
  f.tr_b = log.tr.as<SlEnt>();
  f.indptr_b = d_indptr;
  f.indices_b = d_indices;
  f.values_b = d_values;
  f.n_b = n_rows;
  launch_sliced(ctx, sliced, f);
  const int grid = capped_grid(ctx, n_rows, kBlock, 8, 0);
  hipLaunchKernelGGL(scores_from_slices_kernel, dim3(grid), dim3(kBlock), 0, ctx->stream,
                     plan->sl_zf.as<double>(), plan->sl_ns, n_rows, d_out_pred);
  RFM_HIP_CHECK(hipGetLastError());
}

// what a fit() loop with a ValEvaluator does after every iteration (utils/search_params.py:96-111,
// utils/evaluate.py:160-207): score the evaluation log, take its IPS-DCG@k (rfm_val_dcg)
struct EvalHook {
  const int64_t* indptr;
  const int32_t* indices;
  const double* values;
  int64_t n_rows;
  const int32_t* seg_ptr;
  const int32_t* rows;
  const double* labels;
  const double* pscores;
  int32_t n_segments, k;
  double* scores;        // [n_slots][scores_stride]; iteration i of the call -> slot slot_first + i
  int64_t scores_stride;
  double* user_scratch;  // [n_slots][user_stride]
  int64_t user_stride;
  int64_t slot_first;
  double* dcg_out;       // [n_iters][2]
};

// the arguments of one rfm_fm_train / rfm_fm_train_eval call
struct FitCall {
  rfm_ctx* ctx;
  rfm_fm_plan* plan;
  const int64_t* indptr;  // the training log
  const int32_t* indices;
  const double *values, *y, *pscore;
  const int32_t* ids;  // [n_iters][batch]
  int64_t batch, n_iters;
  double *w0, *w, *V;
  double lr;
  const int64_t* val_indptr;  // the validation log
  const int32_t* val_indices;
  const double *val_values, *val_y, *val_pscore;
  int64_t n_val;
  double eps;
  double *out_train_loss, *out_val_loss;  // [n_iters] each, or null: not asked for
  const EvalHook* hook;                   // or null
  // rfm_fm_train_part: the iterations of the longer call this one is a piece of (0: n_iters).
  // The loss forms are chosen for that length, so a fit's losses do not depend on the cut.
  int64_t form_iters = 0;
};

// How a call computes its loss forwards: one decision for the whole call (the partials of a run
// are finished together).
struct LossForms {
  int64_t n_a = 0, n_b = 0;   // rows of an iteration's train / validation loss (0: not asked for)
  SlicedGeom sliced;          // sliced by factors: partial logits, ONE launch per iteration
  bool merge_call = false;    // both losses in ONE fm_forward_kernel launch (FwdKind::kCsrPair)
  bool scores_only = false;   // plain forwards that leave scores; the run's logarithms come later
  bool ride = false;          // the train rows ride in the next step's forward launch (the ...Riders kinds)
  bool ride_val = false;      // ... and so do the validation rows
  int zns = 0;                // partial logits per row in plan->sl_z (0: it holds scores)
  int64_t z_per_iter = 0;     // doubles of plan->sl_z per iteration
  int64_t run_len = kRun;     // iterations of a run
  bool deferred() const { return sliced.ok || scores_only; }
};

LossForms loss_forms(const FitCall& c) {
  rfm_ctx* ctx = c.ctx;
  const rfm_fm_plan* plan = c.plan;
  const Shape s = shape_for(plan->k);
  LossForms f;
  f.n_a = c.out_train_loss ? c.batch : 0;
  f.n_b = c.out_val_loss ? c.n_val : 0;
  // factor counts of several chunks per lane: the loss forwards sliced by factors, ONE launch
  // per iteration that leaves partial logits; the scores and logarithms of a whole run of
  // iterations are then computed together (rfm_fm_sliced.hpp)
  f.sliced = sliced_geom(ctx, plan, f.n_a + f.n_b);
  // Both losses asked for: ONE launch over the batch's rows of the training log and the
  // validation log.  Only for factor counts of several chunks per lane: there it saves a launch
  // (k = 400, B = 2 000: 0.098 -> 0.090 ms per iteration of fit()); at one chunk per lane the
  // batch's rows are faster through the plan's padded row blocks than through the CSR arrays
  // (config 3: 104.7 vs 111.6 us per iteration at B = 65 536).  RFM_MERGE_LOSS=0 / 2: never / always.
  const int merge_mode = env_int("RFM_MERGE_LOSS", 1);
  f.merge_call = !f.sliced.ok && merge_mode != 0 && (merge_mode == 2 || s.nc > 1) && c.out_train_loss &&
                 c.out_val_loss && forward_form(ctx, c.batch + c.n_val, plan->k, false).block == kBigBlock;
  // The plain loss forwards (neither sliced nor merged) leave their rows' SCORES and take no
  // logarithms: the two logs of a row's term are ~200 dependent f64 instructions, and a whole
  // run of iterations' terms are computed by one launch instead (RFM_DEFER_LOSS=0: in the
  // forward, staged through LDS).
  // (a call of a few iterations -- a fit() with a host evaluator trains one per call -- would only
  // add the run's launches)
  f.scores_only = !f.sliced.ok && !f.merge_call && f.n_a + f.n_b > 0 &&
                  (c.form_iters > 0 ? c.form_iters : c.n_iters) >= 4 &&
                  env_int("RFM_DEFER_LOSS", 1) != 0;
  // Small batches: the train-loss forward of iteration it - 1 reads the parameters that step
  // it's forward reads -- it RIDES in that launch (extra workgroups that only score the previous
  // batch's rows; fm_forward_kernel's ...Riders kinds), and only the last iteration's is a launch of
  // its own.  A run's logarithms then wait for the next step's launch.  The step must take the
  // one-row forward shape and arrival-order hot sums.  (RFM_RIDE_LOSS=0: never.)
  f.ride = f.scores_only && c.out_train_loss && forward_form(ctx, c.batch, plan->k, true).block == kSmallBlock &&
           !(plan->hot_fixed && plan->n_hot > 0) && env_int("RFM_RIDE_LOSS", 1) != 0;
  // ... and so may the validation rows (the same parameters again), when the caller has registered
  // the log (rfm_fm_plan_register_log keeps it as records), it takes the one-row shape too -- as
  // records in a step's launch and as the caller's arrays in the last iteration's own -- and the
  // plan holds plain records (RFM_RIDE_VAL=0: never)
  const rfm_fm_plan::SlLog& vlog = plan->sl_log[0];
  f.ride_val = f.ride && c.out_val_loss && vlog.records &&
               vlog.holds(c.val_indptr, c.val_indices, c.val_values, c.n_val) && plan->ent.p && !plan->ell.p &&
               forward_form(ctx, c.n_val, plan->k, true).block == kSmallBlock &&
               forward_form(ctx, c.n_val, plan->k, false).block == kSmallBlock && env_int("RFM_RIDE_VAL", 1) != 0;
  f.zns = f.sliced.ok ? plan->sl_ns : 0;
  f.z_per_iter = int64_t(std::max(f.zns, 1)) * (f.n_a + f.n_b);
  if (f.deferred()) {
    f.run_len = std::max<int64_t>(1, std::min<int64_t>(kRun, (int64_t(256) << 20) / (f.z_per_iter * 8)));
    f.run_len = std::min(f.run_len, c.n_iters);
  }
  return f;
}

// step `it`, with iteration it - 1's loss rows riding in its forward launch (LossForms::ride)
void fit_step(const FitCall& c, const LossForms& f, const LossRun& run, int64_t it) {
  const int32_t* ids = c.ids + it * c.batch;
  XtraRows prev{};
  if (f.ride && it > 0) {
    const int64_t prev_slot = run.pending_count > 0 ? run.pending_count - 1 : run.slot(it) - 1;
    double* zs = c.plan->sl_z.as<double>() + prev_slot * f.z_per_iter;
    const rfm_fm_plan::SlLog& vlog = c.plan->sl_log[0];
    prev = f.ride_val ? XtraRows{ids - c.batch, c.batch, zs, vlog.rows_rec.as<RowRec>(), vlog.ent_rec.as<Entry>(),
                                 c.n_val, zs + f.n_a}
                      : XtraRows{ids - c.batch, c.batch, zs, nullptr, nullptr, 0, nullptr};
  }
  enqueue_step(c.ctx, c.plan, ids, c.batch, c.w0, c.w, c.V, c.lr, nullptr, nullptr, 0,
               prev.n > 0 ? &prev : nullptr);
}

// the loss forwards of iteration `it` after its step: into the run's slot of the iteration
void fit_loss_forwards(const FitCall& c, const LossForms& f, LossRun& run, int64_t it) {
  const int32_t* ids = c.ids + it * c.batch;
  double* z = f.deferred() ? c.plan->sl_z.as<double>() + run.slot(it) * f.z_per_iter : nullptr;
  if (f.sliced.ok) {
    SlicedArgs a = plan_sliced_args(c.plan, c.w0, c.w, c.V, z);
    a.tr_b = c.plan->sl_log[0].tr.as<SlEnt>();
    a.indptr_a = c.indptr;
    a.indices_a = c.indices;
    a.values_a = c.values;
    a.row_ids = ids;
    a.n_a = f.n_a;
    a.indptr_b = c.val_indptr;
    a.indices_b = c.val_indices;
    a.values_b = c.val_values;
    a.n_b = f.n_b;
    launch_sliced(c.ctx, f.sliced, a);
    return;
  }
  if (f.merge_call) {
    FwdArgs a = forward_args(c.indptr, c.indices, c.values, ids, c.batch + c.n_val, c.w0, c.w, c.V, c.plan->k);
    a.n_rows_a = c.batch;
    a.y = c.y;
    a.pscore = c.pscore;
    a.indptr2 = c.val_indptr;
    a.indices2 = c.val_indices;
    a.values2 = c.val_values;
    a.y2 = c.val_y;
    a.pscore2 = c.val_pscore;
    a.eps = c.eps;
    const int parts = forward_loss_pair_deferred(c.ctx, a, run.train_row(it), run.val_row(it));
    RFM_REQUIRE(parts > 0, "merged loss forward: unexpected geometry");
    run.train_parts = run.val_parts = parts;
    return;
  }
  const bool last = it + 1 == c.n_iters;  // (riding rows of the last iteration have no next step)
  if (c.out_train_loss && (!f.ride || last)) {
    // same batch, new parameters (src/fm.py:90-96), through the plan's records
    FwdArgs a = plan_fwd_args(c.plan, ids, c.batch, c.w0, c.w, c.V);
    a.eps = c.eps;
    if (f.scores_only) {
      a.out_pred = z;
      launch_forward(c.ctx, a);
    } else {
      run.train_parts = forward_loss_deferred(c.ctx, a, run.train_row(it));
    }
  }
  if (c.out_val_loss && (!f.ride_val || last)) {
    FwdArgs a = forward_args(c.val_indptr, c.val_indices, c.val_values, nullptr, c.n_val, c.w0, c.w, c.V,
                             c.plan->k);
    a.eps = c.eps;
    if (f.scores_only) {
      a.out_pred = z + f.n_a;
      launch_forward(c.ctx, a);
    } else {
      a.y = c.val_y;
      a.pscore = c.val_pscore;
      run.val_parts = forward_loss_deferred(c.ctx, a, run.val_row(it));
    }
  }
}

// the evaluator's scores and their IPS-DCG@k, iteration `it`'s parameters
void fit_eval(const FitCall& c, int64_t it) {
  const EvalHook* h = c.hook;
  double* sc = h->scores + (h->slot_first + it) * h->scores_stride;
  plan_forward(c.ctx, c.plan, h->indptr, h->indices, h->values, h->n_rows, c.w0, c.w, c.V, sc);
  const int32_t rc = rfm_val_dcg(c.ctx, sc, h->seg_ptr, h->rows, h->labels, h->pscores, h->n_segments, h->k,
                                 h->user_scratch + (h->slot_first + it) * h->user_stride, h->dcg_out + 2 * it);
  if (rc != RFM_OK) throw Error(rc, "the evaluator's DCG failed (see above)");
}

// iterations first .. first + count of a run -> the call's mean losses; deferred forms take the
// logarithms of the run's scores / partial logits first
void fit_finish(const FitCall& c, const LossForms& f, LossRun& run, int64_t first, int64_t count) {
  if (f.deferred()) {
    const auto shares = [](int64_t rows) { return int(std::min<int64_t>(64, (rows + kBlock - 1) / kBlock)); };
    const double* z = c.plan->sl_z.as<double>();
    if (f.n_a > 0) {
      run.train_parts = shares(f.n_a);
      hipLaunchKernelGGL(loss_from_slices_kernel, dim3(run.train_parts, int(count)), dim3(kBlock), 0,
                         c.ctx->stream, z, f.z_per_iter, f.zns, f.n_a + f.n_b, int64_t(0), f.n_a,
                         c.ids + first * c.batch, c.batch, c.y, c.pscore, c.eps, run.train_rows,
                         int64_t(kMaxFwdGrid));
    }
    if (f.n_b > 0) {
      run.val_parts = shares(f.n_b);
      hipLaunchKernelGGL(loss_from_slices_kernel, dim3(run.val_parts, int(count)), dim3(kBlock), 0,
                         c.ctx->stream, z, f.z_per_iter, f.zns, f.n_a + f.n_b, f.n_a, f.n_b,
                         static_cast<const int32_t*>(nullptr), int64_t(0), c.val_y, c.val_pscore, c.eps,
                         run.val_rows, int64_t(kMaxFwdGrid));
    }
  }
  run.finish_means(c.ctx, first, count, c.batch, c.out_train_loss, c.n_val, c.out_val_loss);
}

// rfm_fm_train: per iteration the step (with riding loss rows), the loss forwards, the evaluator
// hook; the losses of a run of iterations are finished together
void train_loop(const FitCall& c) {
  RFM_REQUIRE(c.ctx && c.w0 && c.w && c.V, "null pointer");
  RFM_REQUIRE(c.n_iters >= 0, "negative n_iters");
  if (c.n_iters == 0) return;
  check_step_args(c.plan, c.indptr, c.indices, c.values, c.y, c.pscore, c.ids, c.batch);
  validate_ids(c.ctx, c.plan, c.ids, c.batch, c.n_iters);
  if (c.out_val_loss)
    RFM_REQUIRE(c.val_indptr && c.val_indices && c.val_values && c.val_y && c.val_pscore && c.n_val >= 1,
                "validation arrays missing");
  LossRun run(c.plan, c.out_train_loss || c.out_val_loss);
  const LossForms f = loss_forms(c);
  if (f.deferred()) {
    c.plan->sl_z.ensure(size_t(f.run_len) * size_t(f.z_per_iter) * 8);
    // (the validation log is only known here: translated once per call)
    // (... unless the caller has registered these arrays: rfm_fm_plan_register_log, slot 0)
    rfm_fm_plan::SlLog& vlog = c.plan->sl_log[0];
    if (f.sliced.ok && f.n_b > 0 && !vlog.holds(c.val_indptr, c.val_indices, c.val_values, f.n_b)) {
      vlog.rows = -1;  // (the slot is about to hold another log)
      sliced_translate(c.ctx, c.plan, c.val_indptr, c.val_indices, c.val_values, f.n_b, vlog.tr);
    }
  }
  const auto finish = [&](int64_t first, int64_t count) { fit_finish(c, f, run, first, count); };
  for (int64_t it = 0; it < c.n_iters; ++it) {
    fit_step(c, f, run, it);
    run.finish_pending(finish);  // (before this iteration's forwards reuse the run's first slots)
    fit_loss_forwards(c, f, run, it);
    if (c.hook) fit_eval(c, it);
    // (riding train rows: a run's last scores arrive with the next step)
    run.close(it, f.run_len, f.ride && it + 1 < c.n_iters, finish);
  }
  run.finish_open(c.n_iters, finish);
}

}  // namespace

extern "C" {

int32_t rfm_fm_plan_forward(rfm_ctx* ctx, rfm_fm_plan* plan, const int64_t* d_indptr,
                            const int32_t* d_indices, const double* d_values, int64_t n_rows,
                            const double* d_w0, const double* d_w, const double* d_V,
                            double* d_out_pred) {
  return guarded([&] {
    RFM_REQUIRE(ctx && plan && d_indptr && d_w0 && d_w && d_V && d_out_pred, "null pointer");
    RFM_REQUIRE(n_rows >= 0, "negative n_rows");
    plan_forward(ctx, plan, d_indptr, d_indices, d_values, n_rows, d_w0, d_w, d_V, d_out_pred);
  });
}

int32_t rfm_fm_train(rfm_ctx* ctx, rfm_fm_plan* plan, const int64_t* d_indptr,
                     const int32_t* d_indices, const double* d_values, const double* d_y,
                     const double* d_pscore, const int32_t* d_ids, int64_t batch,
                     int64_t n_iters, double* d_w0, double* d_w, double* d_V, double lr,
                     const int64_t* d_val_indptr, const int32_t* d_val_indices,
                     const double* d_val_values, const double* d_val_y,
                     const double* d_val_pscore, int64_t n_val, double eps,
                     double* d_out_train_loss, double* d_out_val_loss) {
  return guarded([&] {
    train_loop(FitCall{ctx, plan, d_indptr, d_indices, d_values, d_y, d_pscore, d_ids, batch, n_iters, d_w0,
                       d_w, d_V, lr, d_val_indptr, d_val_indices, d_val_values, d_val_y, d_val_pscore, n_val,
                       eps, d_out_train_loss, d_out_val_loss, nullptr});
  });
}

int32_t rfm_fm_forward_geometry(const rfm_ctx* ctx, int64_t n_rows, int32_t n_factors, int32_t records,
                                int32_t* h_out4) {
  return guarded([&] {
    RFM_REQUIRE(ctx && h_out4, "null pointer");
    RFM_REQUIRE(n_rows >= 1 && n_rows < (int64_t(1) << 31), "bad shape");
    const FwdForm f = forward_form(ctx, n_rows, n_factors, records != 0);
    h_out4[0] = f.block;
    h_out4[1] = f.grid;
    h_out4[2] = f.trip;
    h_out4[3] = f.lanes;
  });
}

int32_t rfm_fm_step_form(const rfm_ctx* ctx, const rfm_fm_plan* plan, int64_t batch, int64_t n_riding_rows,
                         int32_t* h_out8) {
  return guarded([&] {
    RFM_REQUIRE(ctx && plan && h_out8, "null pointer");
    RFM_REQUIRE(batch >= 1 && batch <= plan->max_batch, "batch=%lld outside 1..max_batch=%lld",
                (long long)batch, (long long)plan->max_batch);
    RFM_REQUIRE(n_riding_rows >= 0, "negative n_riding_rows");
    FwdArgs a = step_fwd_args(plan, nullptr, batch, nullptr, nullptr, nullptr);
    a.n_rows_x = n_riding_rows;
    const FwdForm f = forward_form(ctx, a);
    const int32_t out[8] = {f.block, f.grid, f.trip, f.lanes, int32_t(f.kind), f.lanes8, int32_t(f.lds), f.fixed};
    std::copy(out, out + 8, h_out8);
  });
}

int32_t rfm_fm_sliced_geometry(const rfm_ctx* ctx, const rfm_fm_plan* plan, int64_t n_rows, int64_t form_rows,
                               int32_t* h_out4) {
  return guarded([&] {
    RFM_REQUIRE(ctx && plan && h_out4, "null pointer");
    RFM_REQUIRE(n_rows >= 1 && form_rows >= -1, "bad shape");
    const SlicedGeom g = sliced_geom(ctx, plan, n_rows, form_rows);
    h_out4[0] = g.ok ? 1 : 0;
    h_out4[1] = g.grid;
    h_out4[2] = g.rows_per_wg;
    h_out4[3] = int32_t(g.lds);
  });
}

int32_t rfm_fm_train_forms(const rfm_ctx* ctx, const rfm_fm_plan* plan, int64_t batch, int64_t n_iters,
                           int64_t call_iters, const int64_t* d_val_indptr, const int32_t* d_val_indices,
                           const double* d_val_values, int64_t n_val, int32_t want_train, int32_t want_val,
                           int32_t* h_out8) {
  return guarded([&] {
    RFM_REQUIRE(ctx && plan && h_out8, "null pointer");
    RFM_REQUIRE(batch >= 1 && batch <= plan->max_batch, "batch=%lld outside 1..max_batch=%lld",
                (long long)batch, (long long)plan->max_batch);
    RFM_REQUIRE(n_iters >= 1 && (call_iters == 0 || call_iters >= n_iters), "bad iteration counts");
    RFM_REQUIRE(!want_val || n_val >= 1, "validation arrays missing");
    // (loss_forms only asks whether a loss is wanted: the outputs are never written through)
    static double wanted;
    FitCall c{};
    c.ctx = const_cast<rfm_ctx*>(ctx);
    c.plan = const_cast<rfm_fm_plan*>(plan);
    c.batch = batch;
    c.n_iters = n_iters;
    c.val_indptr = d_val_indptr;
    c.val_indices = d_val_indices;
    c.val_values = d_val_values;
    c.n_val = n_val;
    c.out_train_loss = want_train ? &wanted : nullptr;
    c.out_val_loss = want_val ? &wanted : nullptr;
    c.form_iters = call_iters;
    const LossForms f = loss_forms(c);
    // threads per workgroup of the launch that scores the rows of each loss (fit_loss_forwards,
    // fit_step): the sliced kernel's, the merged launch's, the step's own forward for riding rows
    // (whose last iteration is a launch of its own: loss_forms lets rows ride only where that
    // launch takes the one-row shape too, so the answer holds for both)
    const auto block_of = [&](int64_t rows, bool recs, bool rides) {
      if (f.sliced.ok) return kSlBlock;
      if (f.merge_call) return kBigBlock;
      if (rides) return kSmallBlock;
      return forward_form(ctx, rows, plan->k, recs).block;
    };
    h_out8[0] = f.sliced.ok ? 1 : 0;
    h_out8[1] = f.merge_call ? 1 : 0;
    h_out8[2] = f.scores_only ? 1 : 0;
    h_out8[3] = f.ride ? 1 : 0;
    h_out8[4] = f.ride_val ? 1 : 0;
    h_out8[5] = int32_t(f.run_len);
    h_out8[6] = want_train ? block_of(batch, true, f.ride) : 0;
    h_out8[7] = want_val ? block_of(n_val, false, f.ride_val) : 0;
  });
}

int32_t rfm_fm_train_part(rfm_ctx* ctx, rfm_fm_plan* plan, const int64_t* d_indptr,
                          const int32_t* d_indices, const double* d_values, const double* d_y,
                          const double* d_pscore, const int32_t* d_ids, int64_t batch,
                          int64_t n_iters, double* d_w0, double* d_w, double* d_V, double lr,
                          const int64_t* d_val_indptr, const int32_t* d_val_indices,
                          const double* d_val_values, const double* d_val_y,
                          const double* d_val_pscore, int64_t n_val, double eps,
                          double* d_out_train_loss, double* d_out_val_loss, int64_t call_iters) {
  return guarded([&] {
    RFM_REQUIRE(call_iters >= n_iters, "call_iters=%lld is less than n_iters=%lld", (long long)call_iters,
                (long long)n_iters);
    train_loop(FitCall{ctx, plan, d_indptr, d_indices, d_values, d_y, d_pscore, d_ids, batch, n_iters, d_w0,
                       d_w, d_V, lr, d_val_indptr, d_val_indices, d_val_values, d_val_y, d_val_pscore, n_val,
                       eps, d_out_train_loss, d_out_val_loss, nullptr, call_iters});
  });
}

int32_t rfm_fm_train_eval(rfm_ctx* ctx, rfm_fm_plan* plan, const int64_t* d_indptr,
                          const int32_t* d_indices, const double* d_values, const double* d_y,
                          const double* d_pscore, const int32_t* d_ids, int64_t batch,
                          int64_t n_iters, double* d_w0, double* d_w, double* d_V, double lr,
                          const int64_t* d_val_indptr, const int32_t* d_val_indices,
                          const double* d_val_values, const double* d_val_y,
                          const double* d_val_pscore, int64_t n_val, double eps,
                          double* d_out_train_loss, double* d_out_val_loss,
                          const int64_t* d_ev_indptr, const int32_t* d_ev_indices,
                          const double* d_ev_values, int64_t n_ev, const int32_t* d_seg_ptr,
                          const int32_t* d_rows, const double* d_labels, const double* d_ev_pscores,
                          int32_t n_segments, int32_t k, double* d_scores, int64_t scores_stride,
                          double* d_user_scratch, int64_t user_stride, int64_t slot_first,
                          double* d_dcg_out) {
  return guarded([&] {
    RFM_REQUIRE(d_ev_indptr && d_seg_ptr && d_rows && d_labels && d_scores && d_user_scratch && d_dcg_out,
                "null pointer (evaluation)");
    RFM_REQUIRE(n_ev >= 1 && scores_stride >= n_ev && user_stride >= 3 * int64_t(n_segments) && slot_first >= 0,
                "bad evaluation shape");
    const EvalHook hook{d_ev_indptr, d_ev_indices, d_ev_values, n_ev, d_seg_ptr, d_rows, d_labels,
                        d_ev_pscores, n_segments, k, d_scores, scores_stride, d_user_scratch, user_stride,
                        slot_first, d_dcg_out};
    train_loop(FitCall{ctx, plan, d_indptr, d_indices, d_values, d_y, d_pscore, d_ids, batch, n_iters, d_w0,
                       d_w, d_V, lr, d_val_indptr, d_val_indices, d_val_values, d_val_y, d_val_pscore, n_val,
                       eps, d_out_train_loss, d_out_val_loss, &hook});
  });
}

}  // extern "C"
