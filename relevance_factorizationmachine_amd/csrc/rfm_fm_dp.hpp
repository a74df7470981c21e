// The data-parallel fit() loop of one rank (rfm_fm_fit_dp).  Included by
// rfm_fm.hip (it enqueues that file's launches).  The reference has no multi-process mode;
// what is reproduced is src/fm.py:71-102 with the batch's rows dealt to the ranks:
//   dense        gradient of the shard -> all-reduce(sum) of [G_V | g_w | g_w0] -> apply
//   touched rows gradient records of the shard -> owners (all-to-all) -> rank-ordered sum +
//                update by the owner -> updated rows to everybody (all-to-all) -> store
// and the two losses as per-rank sums combined once per call.  Nothing inside the loop
// synchronises with the host or allocates: every transfer size of the call is derived from
// the row ids before the loop (plan_transfers).
#pragma once

namespace rfm {
namespace {

// contiguous shard of `total` items for `rank` (the first total % world ranks take one more)
inline void shard_of(int64_t total, int world, int rank, int64_t& lo, int64_t& hi) {
  const int64_t q = total / world, m = total % world;
  lo = rank * q + std::min<int64_t>(rank, m);
  hi = lo + q + (rank < m ? 1 : 0);
}

struct DpExchange {
  rfm_ctx* ctx;
  const rfm_transport* cb;
  int world, rank;
  static void ok(int32_t rc, const char* what) {
    if (rc != 0) fail(RFM_ERR_INTERNAL, "transport %s failed (%d)", what, rc);
  }
  void all_gather(const void* d_send, void* d_recv, int64_t bytes) {
    if (cb)
      ok(cb->all_gather(cb->user, d_send, d_recv, bytes), "all_gather");
    else
      comm_all_gather(ctx, d_send, d_recv, bytes);
  }
  void all_reduce_sum(double* d_buf, int64_t count) {
    if (cb)
      ok(cb->all_reduce_sum(cb->user, d_buf, count), "all_reduce_sum");
    else
      comm_all_reduce_sum(ctx, d_buf, count);
  }
  void all_to_all(const void* d_send, const int64_t* soff, const int64_t* sbytes, void* d_recv,
                  const int64_t* roff, const int64_t* rbytes) {
    if (cb)
      ok(cb->all_to_all(cb->user, d_send, soff, sbytes, d_recv, roff, rbytes), "all_to_all");
    else
      comm_all_to_all(ctx, rank, d_send, soff, sbytes, d_recv, roff, rbytes);
  }
};

// table / stamps of the touched-row gradients, allocated on first use; returns the next stamp
// (`ids` of them are reserved: the caller uses id .. id + ids - 1)
int32_t next_touch_ids(rfm_ctx* ctx, rfm_fm_plan* plan, int64_t ids) {
  const int64_t n = plan->n_features;
  const int k = plan->k;
  RFM_REQUIRE(ids >= 1 && ids < INT32_MAX / 2, "too many iterations in one call");
  if (!plan->row_table.p) {
    plan->row_table.alloc((size_t(n) * size_t(k + 1) + 1) * sizeof(double));
    plan->touch.alloc(size_t(n) * 4);
    plan->chunk_cnt.alloc(size_t((n + kTouchChunk - 1) / kTouchChunk) * 4);
    plan->touch_seq = 0;
  }
  if (plan->touch_seq == 0 || int64_t(plan->touch_seq) + ids >= INT32_MAX) {
    RFM_HIP_CHECK(hipMemsetAsync(plan->touch.p, 0, plan->touch.bytes, ctx->stream));
    plan->touch_seq = 0;
  }
  const int32_t first = plan->touch_seq + 1;
  plan->touch_seq += int32_t(ids);
  return first;
}

// the launches of rfm_fm_grad_rows: gradient of `batch` rows into the plan's table, stamped
// with `id`, then the stamped columns as records (count -> list -> fill)
void enqueue_grad_rows(rfm_ctx* ctx, rfm_fm_plan* plan, int32_t id, const int32_t* d_row_ids,
                       int64_t batch, const double* d_w0, const double* d_w, const double* d_V,
                       double* d_rows, int64_t cap_rows, int32_t* d_n_rows, double* d_gw0,
                       const int32_t* d_range_lo, int32_t n_ranges, int32_t* d_range_bounds) {
  const int64_t n = plan->n_features;
  const int k = plan->k;
  double* table = plan->row_table.as<double>();
  int32_t* touch = plan->touch.as<int32_t>();
  if (batch > 0) {
    enqueue_step(ctx, plan, d_row_ids, batch, const_cast<double*>(d_w0), const_cast<double*>(d_w),
                 const_cast<double*>(d_V), 0.0, table, touch, id);
  } else {  // an empty shard touches nothing
    RFM_HIP_CHECK(hipMemsetAsync(table + n * (k + 1), 0, sizeof(double), ctx->stream));
  }
  const int n_chunks = int((n + kTouchChunk - 1) / kTouchChunk);
  int32_t* chunk = plan->chunk_cnt.as<int32_t>();
  hipLaunchKernelGGL(touch_count_kernel, dim3(n_chunks), dim3(kBlock), 0, ctx->stream, touch, id, n,
                     chunk);
  hipLaunchKernelGGL(touch_list_kernel, dim3(n_chunks), dim3(kBlock), 0, ctx->stream, touch, id, n,
                     k, chunk, n_chunks, table, d_rows, cap_rows, d_n_rows, d_gw0,
                     n_ranges ? d_range_lo : nullptr, int(n_ranges), d_range_bounds);
  if (cap_rows > 0) {
    const int grid = capped_grid(ctx, std::min<int64_t>(cap_rows, n), kBlock / kWave, 8, 1);
    hipLaunchKernelGGL(rows_fill_kernel, dim3(grid), dim3(kBlock), 0, ctx->stream, table, d_rows,
                       d_n_rows, cap_rows, n, k);
  }
  RFM_HIP_CHECK(hipGetLastError());
}

// small device scratch of rfm_fm_fit_dp (plan->dp_small): [0] record count | [1..2] error flag |
// [8 .. 8+64) a step's real bounds | then the shard's g_w0
struct DpSmall {
  int32_t *n_rows, *flag, *chk;
  double* gw0;
  explicit DpSmall(rfm_fm_plan* plan) {
    plan->dp_small.ensure(8 * 4 + 64 * 4 + 16);
    n_rows = plan->dp_small.as<int32_t>();
    flag = n_rows + 1;
    chk = n_rows + 8;
    gw0 = reinterpret_cast<double*>(plan->dp_small.as<char>() + 8 * 4 + 64 * 4);
  }
  // (synchronises) the flag bounds_check_kernel raises when the records do not match the plan
  void check(hipStream_t st) const {
    int32_t h[2] = {0, 0};
    RFM_HIP_CHECK(hipMemcpyAsync(h, flag, 8, hipMemcpyDeviceToHost, st));
    RFM_HIP_CHECK(hipStreamSynchronize(st));
    if (h[0] != 0)
      fail(RFM_ERR_INTERNAL,
           "iteration %d: the gradient records do not match the transfer plan derived from the row ids",
           h[0] - 1);
  }
};

// Sizes of every transfer of a call of `n_iters` iterations, from the row ids alone.
struct TransferPlan {
  int world = 1, rank = 0;
  int64_t n_iters = 0;
  std::vector<int32_t> bounds;  // [world][n_iters][world + 1]: rank s's record list cut by owner
  std::vector<int32_t> seg;     // [n_iters][world + 1]: what this rank receives, by source
  std::vector<int64_t> out_off; // [n_iters][world + 1]: the updated rows, by owner
  int64_t cap_rows = 0, cap_recv = 0, cap_all = 0;
  std::vector<int64_t> soff, sbytes, roff, rbytes;  // [world]: one all-to-all's offsets and sizes
  const int32_t* of(int s, int64_t it) const { return bounds.data() + (size_t(s) * n_iters + it) * (world + 1); }
};

void plan_transfers(rfm_ctx* ctx, rfm_fm_plan* plan, DpExchange& ex, const int32_t* d_ids,
                    int64_t global_batch, int64_t lo, int64_t hi, int64_t n_iters,
                    TransferPlan& tp) {
  const int W = ex.world, nb = W + 1;
  const int64_t n = plan->n_features;
  const Shape shp = shape_for(plan->k);
  tp.world = W;
  tp.rank = ex.rank;
  tp.n_iters = n_iters;
  std::vector<int32_t> range_lo(static_cast<size_t>(W));
  for (int r = 0; r < W; ++r) range_lo[size_t(r)] = int32_t(n * r / W);
  plan->dp_range_lo.ensure(size_t(W) * 4);
  RFM_HIP_CHECK(hipMemcpyAsync(plan->dp_range_lo.p, range_lo.data(), size_t(W) * 4,
                               hipMemcpyHostToDevice, ctx->stream));
  plan->dp_bounds.ensure(size_t(n_iters) * nb * 4);
  plan->dp_all_bounds.ensure(size_t(W) * size_t(n_iters) * nb * 4);
  int32_t* d_n_rows = DpSmall(plan).n_rows;
  const int32_t id0 = next_touch_ids(ctx, plan, n_iters);
  const int n_chunks = int((n + kTouchChunk - 1) / kTouchChunk);
  const int64_t batch = hi - lo;
  for (int64_t it = 0; it < n_iters; ++it) {
    const int32_t id = id0 + int32_t(it);
    if (batch > 0) {
      const int64_t items = plan->ell.p ? batch * shp.lpr : batch * kWave;
      const int grid = capped_grid(ctx, items, kBlock, 16, 1);
      hipLaunchKernelGGL(rows_mark_kernel, dim3(grid), dim3(kBlock), 0, ctx->stream,
                         plan->ent.as<Entry>(), plan->rows.as<RowRec>(), plan->ell.as<char>(),
                         plan->ell_stride, shp.lpr, d_ids + it * global_batch + lo, batch,
                         plan->touch.as<int32_t>(), id, plan->hot_cols.as<int32_t>(), plan->n_hot);
    }
    hipLaunchKernelGGL(touch_count_kernel, dim3(n_chunks), dim3(kBlock), 0, ctx->stream,
                       plan->touch.as<int32_t>(), id, n, plan->chunk_cnt.as<int32_t>());
    hipLaunchKernelGGL(touch_list_kernel, dim3(n_chunks), dim3(kBlock), 0, ctx->stream,
                       plan->touch.as<int32_t>(), id, n, plan->k, plan->chunk_cnt.as<int32_t>(),
                       n_chunks, plan->row_table.as<double>(), static_cast<double*>(nullptr),
                       int64_t(0), d_n_rows, static_cast<double*>(nullptr),
                       plan->dp_range_lo.as<int32_t>(), W, plan->dp_bounds.as<int32_t>() + it * nb);
  }
  RFM_HIP_CHECK(hipGetLastError());
  // every rank's bounds to every rank: the one exchange whose result the host reads
  ex.all_gather(plan->dp_bounds.p, plan->dp_all_bounds.p, n_iters * nb * 4);
  tp.bounds.resize(size_t(W) * size_t(n_iters) * nb);
  RFM_HIP_CHECK(hipMemcpyAsync(tp.bounds.data(), plan->dp_all_bounds.p, tp.bounds.size() * 4,
                               hipMemcpyDeviceToHost, ctx->stream));
  RFM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  // the record that carries a rank's g_w0 (column n) closes its list: owned by the last rank
  for (int s = 0; s < W; ++s)
    for (int64_t it = 0; it < n_iters; ++it) tp.bounds[(size_t(s) * n_iters + it) * nb + W] += 1;
  for (auto* v : {&tp.soff, &tp.sbytes, &tp.roff, &tp.rbytes}) v->assign(size_t(W), 0);
  tp.seg.assign(size_t(n_iters) * nb, 0);
  tp.out_off.assign(size_t(n_iters) * nb, 0);
  for (int64_t it = 0; it < n_iters; ++it) {
    int32_t* seg = tp.seg.data() + it * nb;
    int64_t* off = tp.out_off.data() + it * nb;
    for (int s = 0; s < W; ++s) {
      const int32_t* b = tp.of(s, it);
      for (int r = 0; r < W; ++r) RFM_REQUIRE(b[r + 1] >= b[r] && b[0] == 0, "corrupt bounds");
      seg[s + 1] = seg[s] + (b[ex.rank + 1] - b[ex.rank]);
    }
    for (int r = 0; r < W; ++r) {
      int64_t cnt = 0;
      for (int s = 0; s < W; ++s) cnt += tp.of(s, it)[r + 1] - tp.of(s, it)[r];
      off[r + 1] = off[r] + cnt;
    }
    tp.cap_rows = std::max<int64_t>(tp.cap_rows, tp.of(ex.rank, it)[W]);
    tp.cap_recv = std::max<int64_t>(tp.cap_recv, seg[W]);
    tp.cap_all = std::max<int64_t>(tp.cap_all, off[W]);
  }
  // on the device: this rank's planned bounds (what bounds_check_kernel compares with) and the
  // segment pointers of rfm_fm_reduce_rows, for all iterations
  plan->dp_seg.ensure(size_t(n_iters) * nb * 4);
  RFM_HIP_CHECK(hipMemcpyAsync(plan->dp_bounds.p, tp.of(ex.rank, 0), size_t(n_iters) * nb * 4,
                               hipMemcpyHostToDevice, ctx->stream));
  RFM_HIP_CHECK(hipMemcpyAsync(plan->dp_seg.p, tp.seg.data(), size_t(n_iters) * nb * 4,
                               hipMemcpyHostToDevice, ctx->stream));
  const size_t wb = size_t(plan->k + 2) * 8;
  plan->dp_rows.ensure(size_t(std::max<int64_t>(tp.cap_rows, 1)) * wb);
  plan->dp_recv.ensure(size_t(std::max<int64_t>(tp.cap_recv, 1)) * wb);
  plan->dp_all.ensure(size_t(std::max<int64_t>(tp.cap_all, 1)) * wb);
  // (the host vectors uploaded above outlive the copies: tp is the caller's, range_lo was
  // consumed before the synchronisation)
}

// the collectives of a call: the caller's transport, else the ctx's communicator, else one rank
DpExchange dp_exchange(rfm_ctx* ctx, const rfm_transport* transport) {
  DpExchange ex{ctx, transport, 1, 0};
  if (transport) {
    RFM_REQUIRE(transport->all_gather && transport->all_reduce_sum && transport->all_to_all,
                "transport lacks a function");
    ex.world = transport->n_ranks;
    ex.rank = transport->rank;
  } else if (ctx->comm) {
    ex.world = ctx->comm_ranks;
    ex.rank = ctx->comm_rank;
  }
  RFM_REQUIRE(ex.world >= 1 && ex.world <= kMaxRanges - 1 && ex.rank >= 0 && ex.rank < ex.world,
              "bad rank %d of %d", ex.rank, ex.world);
  return ex;
}

// iteration `it` of the dense exchange: gradient of the shard -> all-reduce(sum) -> apply
void exchange_dense(rfm_ctx* ctx, rfm_fm_plan* plan, DpExchange& ex, const int32_t* ids, int64_t batch,
                    double* d_w0, double* d_w, double* d_V, double lr) {
  const int64_t n = plan->n_features;
  const int64_t count = n * int64_t(plan->k + 1) + 1;
  double* grad = plan->dp_grad.as<double>();
  if (batch > 0)
    enqueue_step(ctx, plan, ids, batch, d_w0, d_w, d_V, 0.0, grad);
  else
    RFM_HIP_CHECK(hipMemsetAsync(grad, 0, size_t(count) * 8, ctx->stream));
  ex.all_reduce_sum(grad, count);
  hipLaunchKernelGGL(fm_apply_kernel, dim3(capped_grid(ctx, count, kBlock, 16, 0)), dim3(kBlock), 0, ctx->stream,
                     d_V, d_w, d_w0, grad, n * int64_t(plan->k), n, lr);
}

// the ranks' loss sums [train (n_iters) | val (n_iters)] -> the mean losses, the same on every rank
// (a null output: not asked for)
void dp_losses(rfm_ctx* ctx, DpExchange& ex, bool exchange_on, double* sums, int64_t n_iters, int64_t n_train,
               double* out_train, int64_t n_val, double* out_val) {
  if (exchange_on && (out_train || out_val)) ex.all_reduce_sum(sums, 2 * n_iters);
  const int sgrid = int((n_iters + kBlock - 1) / kBlock);
  if (out_train)
    hipLaunchKernelGGL(loss_scale_kernel, dim3(sgrid), dim3(kBlock), 0, ctx->stream, sums, n_iters,
                       double(n_train), out_train);
  if (out_val)
    hipLaunchKernelGGL(loss_scale_kernel, dim3(sgrid), dim3(kBlock), 0, ctx->stream, sums + n_iters, n_iters,
                       double(n_val), out_val);
  RFM_HIP_CHECK(hipGetLastError());
}

// iteration `it` of the touched-rows exchange: the shard's gradient records to their owners, the
// owners' ordered sums and updates, every owner's updated rows to everybody
void exchange_rows(rfm_ctx* ctx, rfm_fm_plan* plan, DpExchange& ex, TransferPlan& tp, const DpSmall& small,
                   int64_t it, int32_t id, const int32_t* ids, int64_t batch, double* d_w0, double* d_w,
                   double* d_V, double lr) {
  const int W = ex.world, nb = W + 1;
  const int64_t n = plan->n_features;
  const int k = plan->k;
  const int64_t wb = int64_t(k + 2) * 8;
  hipStream_t st = ctx->stream;
  const int32_t* mine = tp.of(ex.rank, it);
  const int32_t* seg = tp.seg.data() + it * nb;
  const int64_t* off = tp.out_off.data() + it * nb;
  double* rows = plan->dp_rows.as<double>();
  enqueue_grad_rows(ctx, plan, id, ids, batch, d_w0, d_w, d_V, rows, tp.cap_rows, small.n_rows, small.gw0,
                    plan->dp_range_lo.as<int32_t>(), W, small.chk);
  hipLaunchKernelGGL(rows_append_w0_kernel, dim3(1), dim3(kWave), 0, st, rows, small.n_rows, tp.cap_rows,
                     small.gw0, n, k);
  hipLaunchKernelGGL(bounds_check_kernel, dim3(1), dim3(kWave * 2), 0, st, small.chk,
                     plan->dp_bounds.as<int32_t>() + it * nb, W, tp.cap_rows, int32_t(it), small.flag);
  // records to their owners
  for (int p = 0; p < W; ++p) {
    tp.soff[size_t(p)] = int64_t(mine[p]) * wb;
    tp.sbytes[size_t(p)] = int64_t(mine[p + 1] - mine[p]) * wb;
    tp.roff[size_t(p)] = int64_t(seg[p]) * wb;
    tp.rbytes[size_t(p)] = int64_t(seg[p + 1] - seg[p]) * wb;
  }
  ex.all_to_all(rows, tp.soff.data(), tp.sbytes.data(), plan->dp_recv.p, tp.roff.data(), tp.rbytes.data());
  // the owner's ordered sums and updated rows, written where they sit in the list of all
  double* all = plan->dp_all.as<double>();
  if (seg[W] > 0)
    hipLaunchKernelGGL(rows_reduce_kernel, dim3(capped_grid(ctx, seg[W], kBlock / kWave, 8, 0)), dim3(kBlock),
                       0, st, plan->dp_recv.as<double>(), plan->dp_seg.as<int32_t>() + it * nb, W, d_w, d_V, n,
                       k, lr, all + off[ex.rank] * (k + 2), d_w0);
  // every owner's updated rows to everybody
  for (int p = 0; p < W; ++p) {
    tp.soff[size_t(p)] = off[ex.rank] * wb;
    tp.sbytes[size_t(p)] = (off[ex.rank + 1] - off[ex.rank]) * wb;
    tp.roff[size_t(p)] = off[p] * wb;
    tp.rbytes[size_t(p)] = (off[p + 1] - off[p]) * wb;
  }
  ex.all_to_all(all, tp.soff.data(), tp.sbytes.data(), all, tp.roff.data(), tp.rbytes.data());
  if (off[W] > 0)
    hipLaunchKernelGGL(rows_set_kernel, dim3(capped_grid(ctx, off[W], kBlock / kWave, 8, 1)), dim3(kBlock), 0,
                       st, all, off[W], static_cast<const double*>(nullptr), 0, int64_t(1), d_w0, d_w, d_V, n,
                       k, lr, true);
}

// the evaluator of rfm_fm_fit_dp_eval: this rank's shard of the evaluation log (the rows of its
// user groups, in grouped order) and where its per-iteration results go
struct DpEval {
  const int64_t* indptr;
  const int32_t* indices;
  const double* values;
  int64_t n_rows;        // rows of the shard
  int64_t n_rows_total;  // rows of the whole log (they choose the forward's form)
  const int32_t* seg_ptr;
  const int32_t* rows;
  const double* labels;
  const double* pscores;
  int32_t n_local, k;    // user groups of the shard, ranking depth
  double* scores;        // [slots][scores_stride]: iteration i of the call -> slot slot_first + i
  int64_t scores_stride;
  double* user_scratch;  // [slots][user_stride]: [vals | counted | order-dependent], pad apart
  int64_t user_stride;
  int64_t slot_first;
  const int32_t* h_group_lo;  // [n_ranks + 1]: first user group of every rank
  int32_t pad;                // max_local_segments
  int32_t n_segments;         // user groups of the whole log
  double* full_out;           // [n_iters][3 n_segments]
  double* dcg_out;            // [n_iters][2]
};

// iteration `it`: the shard's scores with the new parameters and its per-user values
void dp_eval_iteration(rfm_ctx* ctx, rfm_fm_plan* plan, const DpEval& e, int64_t it, const double* d_w0,
                       const double* d_w, const double* d_V) {
  double* sc = e.scores + (e.slot_first + it) * e.scores_stride;
  double* slot = e.user_scratch + (e.slot_first + it) * e.user_stride;
  plan_forward(ctx, plan, e.indptr, e.indices, e.values, e.n_rows, d_w0, d_w, d_V, sc, e.n_rows_total);
  enqueue_val_dcg_users(ctx, sc, e.seg_ptr, e.rows, e.labels, e.pscores, e.n_local, e.k, slot, slot + e.pad,
                        slot + 2 * int64_t(e.pad));
}

// after the call's iterations: every rank's per-user tables to every rank (ONE all-gather of
// n_iters x user_stride doubles per rank), merged into the whole log's table, and its means
void dp_eval_finish(rfm_ctx* ctx, rfm_fm_plan* plan, DpExchange& ex, bool exchange_on, const DpEval& e,
                    int64_t n_iters) {
  const int64_t bytes = n_iters * e.user_stride * 8;
  const double* mine = e.user_scratch + e.slot_first * e.user_stride;
  const double* all = mine;
  const int W = exchange_on ? ex.world : 1;
  if (exchange_on) {
    plan->dp_ev_all.ensure(size_t(ex.world) * size_t(bytes));
    ex.all_gather(mine, plan->dp_ev_all.p, bytes);
    all = plan->dp_ev_all.as<double>();
  }
  plan->dp_ev_lo.ensure(size_t(ex.world + 1) * 4);
  RFM_HIP_CHECK(hipMemcpyAsync(plan->dp_ev_lo.p, e.h_group_lo, size_t(ex.world + 1) * 4, hipMemcpyHostToDevice,
                               ctx->stream));
  enqueue_val_dcg_merge(ctx, all, W, n_iters, e.user_stride, e.pad, plan->dp_ev_lo.as<int32_t>(), e.n_segments,
                        e.full_out);
  enqueue_val_dcg_means(ctx, e.full_out, n_iters, e.n_segments, e.dcg_out);
}

// rfm_fm_fit_dp, and with `ev` the evaluator of rfm_fm_fit_dp_eval after every update
void fit_dp(rfm_ctx* ctx, rfm_fm_plan* plan, const rfm_transport* transport, int32_t exchange,
            const int32_t* d_ids, int64_t global_batch, int64_t n_iters, double* d_w0, double* d_w, double* d_V,
            double lr, const int64_t* d_val_indptr, const int32_t* d_val_indices, const double* d_val_values,
            const double* d_val_y, const double* d_val_pscore, int64_t n_val, double eps,
            double* d_out_train_loss, double* d_out_val_loss, const DpEval* ev) {
  RFM_REQUIRE(ctx && plan && d_w0 && d_w && d_V, "null pointer");
  RFM_REQUIRE(exchange == 0 || exchange == 1, "exchange=%d (0 dense, 1 touched rows)", exchange);
  RFM_REQUIRE(n_iters >= 0 && global_batch >= 1 && n_val >= 0, "bad shape");
  RFM_REQUIRE(plan->opt_kind == RFM_FM_OPT_SGD,
              "the data-parallel fit applies summed gradients with the SGD rule; the plan's rule is kind %d",
              plan->opt_kind);
  if (n_iters == 0) return;
  RFM_REQUIRE(d_ids, "null row ids");
  DpExchange ex = dp_exchange(ctx, transport);
  if (ev) {
    const int32_t* lo = ev->h_group_lo;
    RFM_REQUIRE(lo, "null group bounds");
    RFM_REQUIRE(lo[0] == 0 && lo[ex.world] == ev->n_segments, "group bounds do not cover the %d user groups",
                ev->n_segments);
    for (int r = 0; r < ex.world; ++r)
      RFM_REQUIRE(lo[r + 1] >= lo[r] && lo[r + 1] - lo[r] <= ev->pad, "group bounds of rank %d", r);
    RFM_REQUIRE(lo[ex.rank + 1] - lo[ex.rank] == ev->n_local, "rank %d holds %d user groups, bounds say %d",
                ex.rank, ev->n_local, lo[ex.rank + 1] - lo[ex.rank]);
  }
  int64_t lo, hi, vlo, vhi;
  shard_of(global_batch, ex.world, ex.rank, lo, hi);
  shard_of(n_val, ex.world, ex.rank, vlo, vhi);
  const int64_t batch = hi - lo, n_my_val = vhi - vlo;
  RFM_REQUIRE(batch <= plan->max_batch, "shard of %lld rows exceeds the plan's max_batch %lld",
              (long long)batch, (long long)plan->max_batch);
  const bool want_val = d_out_val_loss && n_val > 0;
  if (want_val)
    RFM_REQUIRE(d_val_indptr && d_val_indices && d_val_values && d_val_y && d_val_pscore,
                "validation arrays missing");
  for (int64_t it = 0; it < n_iters && batch > 0; ++it)
    validate_ids(ctx, plan, d_ids + it * global_batch + lo, batch, 1);
  const int64_t count = plan->n_features * int64_t(plan->k + 1) + 1;
  hipStream_t st = ctx->stream;

  // per-iteration loss SUMS of this rank: [train (n_iters) | val (n_iters)]
  plan->dp_sums.ensure(size_t(2 * n_iters) * 8);
  RFM_HIP_CHECK(hipMemsetAsync(plan->dp_sums.p, 0, size_t(2 * n_iters) * 8, st));
  double* sums_train = plan->dp_sums.as<double>();
  double* sums_val = sums_train + n_iters;
  LossRun run(plan, d_out_train_loss || want_val);
  const bool train_here = d_out_train_loss && batch > 0, val_here = want_val && n_my_val > 0;
  const auto finish = [&](int64_t first, int64_t cnt) {
    run.finish_sums(ctx, first, cnt, train_here ? sums_train : nullptr, val_here ? sums_val : nullptr);
  };
  if (ev)  // (the padding of the per-user tables travels too: defined bytes)
    RFM_HIP_CHECK(hipMemsetAsync(ev->user_scratch + ev->slot_first * ev->user_stride, 0,
                                 size_t(n_iters * ev->user_stride) * 8, st));

  TransferPlan tp;
  // (RFM_DP_FORCE_EXCHANGE=1: a single rank goes through the exchange too -- every collective
  // with itself -- so that the whole multi-rank loop, RCCL calls included, can be run and
  // checked on one GPU)
  const bool exchange_on = ex.world > 1 || env_int("RFM_DP_FORCE_EXCHANGE", 0) != 0;
  const bool rows_mode = exchange == 1 && exchange_on;
  int32_t id0 = 0;
  if (rows_mode) {
    plan_transfers(ctx, plan, ex, d_ids, global_batch, lo, hi, n_iters, tp);
    id0 = next_touch_ids(ctx, plan, n_iters);
  } else if (exchange_on) {
    plan->dp_grad.ensure(size_t(count) * 8);
  }
  const DpSmall small(plan);
  RFM_HIP_CHECK(hipMemsetAsync(small.flag, 0, 8, st));

  for (int64_t it = 0; it < n_iters; ++it) {
    const int32_t* ids = d_ids + it * global_batch + lo;
    if (!exchange_on) {
      enqueue_step(ctx, plan, ids, batch, d_w0, d_w, d_V, lr, nullptr);
    } else if (!rows_mode) {
      exchange_dense(ctx, plan, ex, ids, batch, d_w0, d_w, d_V, lr);
    } else {
      exchange_rows(ctx, plan, ex, tp, small, it, id0 + int32_t(it), ids, batch, d_w0, d_w, d_V, lr);
    }
    RFM_HIP_CHECK(hipGetLastError());
    if (train_here) {
      // the shard's part of the train loss: same batch, new parameters (src/fm.py:90-96)
      FwdArgs f = plan_fwd_args(plan, ids, batch, d_w0, d_w, d_V);
      f.eps = eps;
      run.train_parts = forward_loss_deferred(ctx, f, run.train_row(it));
    }
    if (val_here) {
      FwdArgs f = forward_args(d_val_indptr + vlo, d_val_indices, d_val_values, nullptr, n_my_val,
                               d_w0, d_w, d_V, plan->k);
      f.y = d_val_y + vlo;
      f.pscore = d_val_pscore + vlo;
      f.eps = eps;
      run.val_parts = forward_loss_deferred(ctx, f, run.val_row(it));
    }
    if (ev) dp_eval_iteration(ctx, plan, *ev, it, d_w0, d_w, d_V);
    run.close(it, kRun, false, finish);
  }
  run.finish_open(n_iters, finish);
  dp_losses(ctx, ex, exchange_on, sums_train, n_iters, global_batch, d_out_train_loss, n_val,
            want_val ? d_out_val_loss : nullptr);
  if (ev) dp_eval_finish(ctx, plan, ex, exchange_on, *ev, n_iters);
  small.check(st);
}

}  // namespace
}  // namespace rfm

extern "C" int32_t rfm_fm_fit_dp(rfm_ctx* ctx, rfm_fm_plan* plan, const rfm_transport* transport,
                                 int32_t exchange, const int32_t* d_ids, int64_t global_batch,
                                 int64_t n_iters, double* d_w0, double* d_w, double* d_V,
                                 double lr, const int64_t* d_val_indptr,
                                 const int32_t* d_val_indices, const double* d_val_values,
                                 const double* d_val_y, const double* d_val_pscore, int64_t n_val,
                                 double eps, double* d_out_train_loss, double* d_out_val_loss) {
  return rfm::guarded([&] {
    rfm::fit_dp(ctx, plan, transport, exchange, d_ids, global_batch, n_iters, d_w0, d_w, d_V, lr, d_val_indptr,
                d_val_indices, d_val_values, d_val_y, d_val_pscore, n_val, eps, d_out_train_loss, d_out_val_loss,
                nullptr);
  });
}

extern "C" int32_t rfm_fm_fit_dp_eval(
    rfm_ctx* ctx, rfm_fm_plan* plan, const rfm_transport* transport, int32_t exchange, const int32_t* d_ids,
    int64_t global_batch, int64_t n_iters, double* d_w0, double* d_w, double* d_V, double lr,
    const int64_t* d_val_indptr, const int32_t* d_val_indices, const double* d_val_values, const double* d_val_y,
    const double* d_val_pscore, int64_t n_val, double eps, double* d_out_train_loss, double* d_out_val_loss,
    const int64_t* d_ev_indptr, const int32_t* d_ev_indices, const double* d_ev_values, int64_t n_ev,
    int64_t n_ev_total, const int32_t* d_seg_ptr, const int32_t* d_rows, const double* d_labels,
    const double* d_ev_pscores, int32_t n_local_segments, int32_t k, double* d_scores, int64_t scores_stride,
    double* d_user_scratch, int64_t user_stride, int64_t slot_first, const int32_t* h_group_lo,
    int32_t max_local_segments, int32_t n_segments, double* d_full_out, double* d_dcg_out) {
  using namespace rfm;
  return guarded([&] {
    RFM_REQUIRE(k >= 1, "k=%d (ranking positions) must be >= 1", k);
    RFM_REQUIRE(n_segments >= 0 && n_local_segments >= 0 && max_local_segments >= n_local_segments &&
                    n_local_segments <= n_segments,
                "bad user groups: %d of %d, padded to %d", n_local_segments, n_segments, max_local_segments);
    RFM_REQUIRE(n_ev >= 0 && n_ev_total >= n_ev && slot_first >= 0 && scores_stride >= n_ev &&
                    user_stride >= std::max<int64_t>(1, 3 * int64_t(max_local_segments)),
                "bad evaluation shape");
    RFM_REQUIRE(d_user_scratch && d_full_out && d_dcg_out, "null pointer (evaluation)");
    if (n_ev > 0) RFM_REQUIRE(d_ev_indptr && d_scores, "null pointer (evaluation log)");
    if (n_local_segments > 0) RFM_REQUIRE(n_ev > 0 && d_seg_ptr && d_labels, "null pointer (user groups)");
    const DpEval ev{d_ev_indptr, d_ev_indices, d_ev_values, n_ev, n_ev_total, d_seg_ptr, d_rows, d_labels,
                    d_ev_pscores, n_local_segments, k, d_scores, scores_stride, d_user_scratch, user_stride,
                    slot_first, h_group_lo, max_local_segments, n_segments, d_full_out, d_dcg_out};
    fit_dp(ctx, plan, transport, exchange, d_ids, global_batch, n_iters, d_w0, d_w, d_V, lr, d_val_indptr,
           d_val_indices, d_val_values, d_val_y, d_val_pscore, n_val, eps, d_out_train_loss, d_out_val_loss, &ev);
  });
}
