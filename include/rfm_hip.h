/*
 * rfm_hip.h -- C ABI of librfm_hip.so, the MI355X (gfx950) implementation of the
 * FM / MF mini-batch SGD path of tatsuki1107/Relevance-FactorizationMachine.
 *
 * The reference has no FFI of its own (it is pure Python); the boundary it
 * offers is the Python class surface of src/base.py, src/fm.py, src/mf.py and
 * utils/optimizer.py.  Each entry point below names the reference code
 * (file:line, relative to the reference root) whose arithmetic it replaces.
 * The Python mirror of that surface (relevance_factorizationmachine_amd/fm.py,
 * mf.py) calls these through ctypes; INTEGRATION.md shows the binding.
 *
 * Conventions
 *  - every call returns int32: RFM_OK or an RFM_ERR_* class; the message is
 *    fetched with rfm_last_error() (thread-local).  No C++ exception crosses.
 *  - pointers named d_* are DEVICE pointers owned by the caller (torch tensors
 *    in the Python mirror); h_* are HOST pointers.  The library allocates only
 *    ctx-/plan-owned scratch and frees it in the matching destroy call.
 *  - calls that take a ctx are asynchronous on the ctx's HIP stream; use
 *    rfm_sync() (or synchronise the stream yourself) before reading results.
 *  - a CSR row names a column at most once (SciPy sums duplicate entries before
 *    it squares them, src/fm.py:127; the Python mirror canonicalises its inputs the
 *    same way); the order of a row's entries is free, explicit zeros are fine.
 *  - all parameters and activations are float64 (the reference computes in
 *    NumPy float64); CSR column indices and row ids are int32, CSR row
 *    pointers int64, labels are passed as float64 {0,1}.
 *  - one ctx per (host thread, device); no global mutable state.
 */
#ifndef RFM_HIP_H
#define RFM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RFM_VERSION 100 /* 0.1.0 */

enum {
  RFM_OK = 0,
  RFM_ERR_BAD_ARG = 1, /* caller error: shapes, null pointers, unsupported k */
  RFM_ERR_HIP = 2,     /* a HIP runtime call or kernel launch failed */
  RFM_ERR_NO_DEVICE = 3,
  RFM_ERR_INTERNAL = 4
};

/* limits of this build */
#define RFM_MAX_FACTORS 1024
/* levels the sequential MF kernel reads an example's rows ahead of its own level */
#define RFM_MF_READ_AHEAD 4
/* rfm_mf_schedule_ex: gap of an example whose user row no earlier example of the batch writes */
#define RFM_MF_NO_WRITER (1 << 30)
/* steps rfm_mf_fold_in reads a chain's fixed rows ahead (and its ids twice as far); measured:
 * profiles/n13/ */
#define RFM_MF_FOLD_READ_AHEAD 4

typedef struct rfm_ctx rfm_ctx;
typedef struct rfm_fm_plan rfm_fm_plan;

/* ---- diagnostics ------------------------------------------------------- */
int32_t rfm_version(void);
/* copies the calling thread's last error message (NUL-terminated) */
int32_t rfm_last_error(char* buf, size_t n);

/* ---- context ----------------------------------------------------------- */
/* hip_stream: a hipStream_t to run on (NULL = the device's default stream). */
int32_t rfm_create(int32_t device, void* hip_stream, rfm_ctx** out);
int32_t rfm_destroy(rfm_ctx* ctx);
int32_t rfm_sync(rfm_ctx* ctx);
/* Synchronous copies ordered after the work on the ctx stream (for a host-staged
 * rfm_transport, which is handed raw device pointers). */
int32_t rfm_copy_to_host(rfm_ctx* ctx, void* h_dst, const void* d_src, int64_t bytes);
int32_t rfm_copy_to_device(rfm_ctx* ctx, void* d_dst, const void* h_src, int64_t bytes);

/* ---- per-kernel timing (HIP events on the ctx stream) ---------------------
 * Between rfm_profile_begin and rfm_profile_end every FM training step records
 * events around its launches.  rfm_profile_end synchronises and returns, per
 * phase, the summed milliseconds and the number of launches:
 *   phase 0 forward (+residual, Q, marks)   phase 1 column gradient/update
 *   phase 2 finalize (long columns, w0)     phase 3 whole step
 * h_ms[4], h_count[4]. */
int32_t rfm_profile_begin(rfm_ctx* ctx);
int32_t rfm_profile_end(rfm_ctx* ctx, double* h_ms, int64_t* h_count);

/* ---- mini-batch selection (host) ---------------------------------------
 * Replaces sklearn.utils.resample(X, y, p, replace=False, n_samples=B,
 * random_state=epoch) as called at src/fm.py:72-79 and src/mf.py:88-95:
 * legacy MT19937 seeded with the iteration number, Fisher-Yates shuffle of
 * arange(n_rows) with NumPy's masked-rejection interval draw, first B ids.
 * h_out_ids[(e - epoch_begin) * batch_size + t], bit-identical to NumPy.
 * RFM_ERR_BAD_ARG when batch_size > n_rows (the reference raises ValueError). */
int32_t rfm_sample_batches(int64_t n_rows, int64_t batch_size, int64_t epoch_begin,
                           int64_t n_epochs, int32_t* h_out_ids, int32_t n_threads);

/* ---- mini-batch selection (device) -------------------------------------
 * rfm_sample_batches on the GPU: d_out_ids[(e - epoch_begin) * batch_size + t], bit-identical
 * to the host sampler, enqueued on hip_stream (NULL = the ctx's stream).  The swap partners of
 * the shuffle are drawn by one wavefront per epoch; the first batch_size entries are then
 * resolved in parallel from them (rfm_sample.hip).  Epochs run in groups that share
 * d_workspace; the results do not depend on its size.  Argument checks and messages are those
 * of rfm_sample_batches; RFM_ERR_BAD_ARG also when the workspace is short of one epoch's.
 * rfm_sample_batches_device_workspace: the bytes `epochs_in_flight` epochs at once need
 * (12 n_rows + 8 batch_size per epoch; host only). */
int32_t rfm_sample_batches_device_workspace(int64_t n_rows, int64_t batch_size,
                                            int64_t epochs_in_flight, int64_t* h_bytes);
int32_t rfm_sample_batches_device(rfm_ctx* ctx, void* hip_stream, int64_t n_rows,
                                  int64_t batch_size, int64_t epoch_begin, int64_t n_epochs,
                                  int32_t* d_out_ids, void* d_workspace, int64_t workspace_bytes);

/* ---- content fingerprint of a host buffer (host) -------------------------
 * Not on the reference's path: the reference reads its inputs on every fit()
 * (src/fm.py:72-79 gathers from train["features"] each iteration); this library keeps device
 * copies of a split between fits and re-uploads when this 64-bit hash of ALL bytes of the
 * host array differs.  Independent of n_threads. */
int32_t rfm_hash_bytes(const void* h_data, int64_t n_bytes, int32_t n_threads, uint64_t* h_out);

/* ---- FM: forward / scores ----------------------------------------------
 * Replaces FactorizationMachines.predict (src/fm.py:114-133) with _sigmoid
 * (src/base.py:63-66): out[t] = sigmoid(clip(w0 + sum_i w_i x_ti
 *   + 0.5 * sum_f[(sum_i v_if x_ti)^2 - sum_i v_if^2 x_ti^2], +-700))
 * for row r = d_row_ids ? d_row_ids[t] : t of the CSR matrix.  d_indices and
 * d_values must be readable for at least one element even if the matrix has
 * no entries (rows without entries score sigmoid(w0)). */
int32_t rfm_fm_forward(rfm_ctx* ctx, const int64_t* d_indptr, const int32_t* d_indices,
                       const double* d_values, const int32_t* d_row_ids, int64_t n_rows,
                       const double* d_w0, const double* d_w, const double* d_V,
                       int64_t n_features, int32_t n_factors, double* d_out_pred);

/* Replaces _cross_entropy_loss (src/base.py:37-61):
 * *d_out = -(1/n) * sum_t[(y/p) log(pred_t + eps) + (1 - y/p) log(1 - pred_t + eps)]
 * with y, p taken at row d_row_ids[t] (or t) and pred at t.  Deterministic
 * two-pass reduction. */
int32_t rfm_ips_logloss(rfm_ctx* ctx, const double* d_y, const double* d_pred,
                        const double* d_pscore, const int32_t* d_row_ids, int64_t n_rows,
                        double eps, double* d_out_loss);

/* Fused forward + loss of the rows (src/fm.py:90-102): scores never leave the
 * chip.  d_out_pred may be NULL. */
int32_t rfm_fm_forward_loss(rfm_ctx* ctx, const int64_t* d_indptr, const int32_t* d_indices,
                            const double* d_values, const double* d_y, const double* d_pscore,
                            const int32_t* d_row_ids, int64_t n_rows, const double* d_w0,
                            const double* d_w, const double* d_V, int64_t n_features,
                            int32_t n_factors, double eps, double* d_out_pred,
                            double* d_out_loss);

/* ---- FM: training plan --------------------------------------------------
 * One-time (per fit) device layout of the training log (train["features"],
 * ["labels"], ["pscores"] of src/fm.py:55-79) for the gradient without global
 * atomics: row records, entry records and a column-major view (entries sorted
 * by column, row order kept inside a column), built ON THE DEVICE and stored in
 * plan-owned device memory.  rfm_fm_plan_create takes the caller's HOST arrays
 * (and uploads a transient copy); rfm_fm_plan_create_device takes the DEVICE copy
 * of the log the caller already holds (same dtypes as everywhere: indptr int64,
 * indices int32, values / labels / propensities float64).  Both reject an indptr
 * that is not monotone, a column index outside 0..n_features-1 and a row that
 * names a column twice (RFM_ERR_BAD_ARG).
 * max_batch bounds the batch size of later steps (max_batch * n_factors < 2^31).
 * hot_min_count: a column
 * whose expected number of entries per batch (its training frequency *
 * max_batch / n_rows) reaches this value is accumulated on chip by the forward
 * workgroups instead of through its column list (0 = library default).  The on-chip
 * sums of the default form are LDS float atomics: their last bits depend on arrival
 * order.  -1 = no such columns: every sum of a step has a fixed order (bitwise
 * reproducible results).  -2 = the default columns, summed in a fixed order as well
 * (each column's rows of a forward workgroup in row order, the workgroups in block
 * order): bitwise reproducible at a fraction of -1's cost; where the factor count has
 * no such kernel (several chunks of factors per lane: more than 128 factors, or an odd
 * count above 64; or, at batches of the many-rows shape, fewer than 16 lanes per row: an
 * even count up to 16, an odd one up to 8) it means -1. */
int32_t rfm_fm_plan_create(rfm_ctx* ctx, const int64_t* h_indptr, const int32_t* h_indices,
                           const double* h_values, const double* h_y, const double* h_pscore,
                           int64_t n_rows, int64_t n_features, int32_t n_factors,
                           int64_t max_batch, int32_t hot_min_count, rfm_fm_plan** out);
int32_t rfm_fm_plan_create_device(rfm_ctx* ctx, const int64_t* d_indptr, const int32_t* d_indices,
                                  const double* d_values, const double* d_y,
                                  const double* d_pscore, int64_t n_rows, int64_t n_features,
                                  int32_t n_factors, int64_t max_batch, int32_t hot_min_count,
                                  rfm_fm_plan** out);
int32_t rfm_fm_plan_destroy(rfm_fm_plan* plan);
/* h_out8[0]=tasks of the gradient launch, [1]=columns longer than a workgroup's
 * tasks (split), [2]=hot columns, [3]=nnz, [4]=device bytes owned by the plan,
 * [5]=forward workgroups of a max_batch step (= hot-sum slabs per step), [6]=slots
 * of the sparse class (padded to whole tasks), [7]=64-slot bitmap words per task */
int32_t rfm_fm_plan_info(const rfm_fm_plan* plan, int64_t* h_out8);
/* how the plan keeps the log for the forward: h_out4[0]=1 if as padded row blocks (every
 * row fits one round of a lane group and max_batch asks for the many-rows shape), else 0 =
 * row + entry records; [1]=bytes of a row block (0 if none); [2]=lanes per row of this
 * factor count; [3]=entries of the longest row */
int32_t rfm_fm_plan_layout(const rfm_fm_plan* plan, int32_t* h_out4);
/* the sliced loss forwards of rfm_fm_train (even factor counts above 128): h_out4[0]=slices of
 * the factors (0: this plan has none), [1]=factors per slice, [2]=columns whose slice a workgroup
 * keeps in LDS, [3]=records per row of the translated logs */
int32_t rfm_fm_plan_sliced(const rfm_fm_plan* plan, int32_t* h_out4);
/* Optional: a log that coming calls on this plan will name (device CSR arrays): slot 0 = the
 * validation log of rfm_fm_train, slot 1 = the log rfm_fm_plan_forward scores.  A plan with sliced
 * loss forwards keeps the log's translated form, and calls that pass the SAME three pointers and row
 * count skip the per-call translation (a fit() that trains one iteration per call and scores an
 * evaluation log after each).  The caller promises that the arrays do not change until it registers
 * the slot again (n_rows = 0: nothing); any other arrays are translated per call. */
int32_t rfm_fm_plan_register_log(rfm_ctx* ctx, rfm_fm_plan* plan, int32_t slot, const int64_t* d_indptr,
                                 const int32_t* d_indices, const double* d_values, int64_t n_rows);
/* rfm_fm_forward through the plan: scores of the rows of a CSR with the plan's column count, by the
 * sliced forward (rfm_fm_train's loss forward, even factor counts above 128) when the plan has one
 * and the rows are enough for it, else by the plain forward -- the same scores up to the order of
 * the sums.  Replaces src/fm.py:114-133 inside a fit() that scores an evaluation log every
 * iteration (utils/search_params.py:96-111). */
int32_t rfm_fm_plan_forward(rfm_ctx* ctx, rfm_fm_plan* plan, const int64_t* d_indptr,
                            const int32_t* d_indices, const double* d_values, int64_t n_rows,
                            const double* d_w0, const double* d_w, const double* d_V,
                            double* d_out_pred);
/* the hot columns (ascending), h_out[0 .. info[2]); capacity = room in h_out */
int32_t rfm_fm_plan_hot_columns(const rfm_fm_plan* plan, int32_t* h_out, int32_t capacity);
/* the columns whose slice a sliced forward's workgroup keeps in LDS, in their LDS order (most
 * frequent first, ties ascending), h_out[0 .. sliced[2]); capacity = room in h_out */
int32_t rfm_fm_plan_sliced_columns(const rfm_fm_plan* plan, int32_t* h_out, int32_t capacity);

/* ---- FM: one training step ----------------------------------------------
 * Replaces lines src/fm.py:80-88 with _update_w0/_update_w/_update_V
 * (src/fm.py:135-187) and SGD.update (utils/optimizer.py:56-64) for the batch
 * rows d_row_ids[0..batch): residual e = y/p - predict(old params); batch-SUM
 * gradients (no 1/|B|); w0, w, V updated in place with lr.  The CSR / label /
 * propensity arrays are the device copy of the log the plan was built from
 * (the step reads the plan's own records of it).
 * PRECONDITION of every call that takes the row ids of a step (rfm_fm_step,
 * rfm_fm_grad, rfm_fm_grad_rows, rfm_fm_train, rfm_fm_fit_dp): the ids of one
 * step lie in 0 .. n_rows-1 of the plan's log and are DISTINCT -- what
 * resample(replace=False) yields (src/fm.py:72-79).  A row's batch position is
 * recorded with a plain store, so a repeated id would silently lose one of its
 * contributions, and an id outside the log would index the records out of
 * bounds.  The calls do not check this by default; with the environment
 * variable RFM_CHECK_IDS=1 they validate the ids on the device first (this
 * synchronises the stream) and return RFM_ERR_BAD_ARG.
 * d_w0 / d_w / d_V: ordinary device memory (hipMalloc -- what a torch device tensor is): every
 * element has ONE writer per step, which adds to w0 / w[col] with a hardware f64 atomic add that
 * returns nothing (no wait for the old value); fine-grained / host-mapped memory is not supported. */
int32_t rfm_fm_step(rfm_ctx* ctx, rfm_fm_plan* plan, const int64_t* d_indptr,
                    const int32_t* d_indices, const double* d_values, const double* d_y,
                    const double* d_pscore, const int32_t* d_row_ids, int64_t batch,
                    double* d_w0, double* d_w, double* d_V, double lr);

/* Same gradients, not applied: d_grad = [G_V (n*k) | g_w (n) | g_w0 (1)] for
 * the given rows (a rank's shard of the batch).  Every element of d_grad is
 * written.  For the data-parallel path: all-reduce d_grad, then rfm_fm_apply. */
int32_t rfm_fm_grad(rfm_ctx* ctx, rfm_fm_plan* plan, const int64_t* d_indptr,
                    const int32_t* d_indices, const double* d_values, const double* d_y,
                    const double* d_pscore, const int32_t* d_row_ids, int64_t batch,
                    const double* d_w0, const double* d_w, const double* d_V, double* d_grad);
/* theta -= lr * grad over the same [V | w | w0] layout (utils/optimizer.py:56-64). */
int32_t rfm_fm_apply(rfm_ctx* ctx, double* d_w0, double* d_w, double* d_V,
                     const double* d_grad, int64_t n_features, int32_t n_factors, double lr);

/* ---- FM: touched-row gradients -----------------------------
 * The reference writes only the rows of V whose gradient is non-zero
 * (src/fm.py:183-187): the columns the batch touches.  rfm_fm_grad_rows computes
 * the same batch-SUM gradients as rfm_fm_grad for rows d_row_ids[0..batch) (a
 * rank's shard; batch may be 0) but returns them as a list of RECORDS, ascending
 * by column, of n_factors + 2 doubles each:
 *     [column (exact in a double), G_V[column, 0..k), g_w[column]]
 * d_rows has room for cap_rows records; *d_n_rows receives the true number (a
 * caller that sees *d_n_rows > cap_rows got only the first cap_rows), *d_gw0
 * the shard's g_w0.  Optional owner ranges for the exchange: d_range_lo[n_ranges]
 * (ascending first columns, n_ranges <= 64) -> d_range_bounds[n_ranges + 1]:
 * position in the list of the first record with column >= range_lo[i], and the
 * total.  Range starts may repeat (more ranks than columns: n_features * r / n_ranks
 * gives the same first column to several ranks; their bounds are then equal).
 * Nothing of size n_features is cleared or moved per call: the kernels
 * stamp the columns they write, and a count / scan / gather over the stamps
 * builds the list. */
int32_t rfm_fm_grad_rows(rfm_ctx* ctx, rfm_fm_plan* plan, const int32_t* d_row_ids, int64_t batch,
                         const double* d_w0, const double* d_w, const double* d_V, double* d_rows,
                         int64_t cap_rows, int32_t* d_n_rows, double* d_gw0,
                         const int32_t* d_range_lo, int32_t n_ranges, int32_t* d_range_bounds);
/* theta -= lr * g for the records of such a list (utils/optimizer.py:56-64 with a
 * row index): V[column,:] -= lr * G_V row, w[column] -= lr * g_w; w0 -= lr * *d_gw0
 * when d_gw0 is given.  The count is read on the device (min(*d_n_rows, cap_rows)). */
int32_t rfm_fm_apply_rows(rfm_ctx* ctx, const double* d_rows, const int32_t* d_n_rows,
                          int64_t cap_rows, const double* d_gw0, double* d_w0, double* d_w,
                          double* d_V, int64_t n_features, int32_t n_factors, double lr);
/* Owner side of the exchange.  d_rows holds n_segments lists back to back, segment
 * s = records d_seg_ptr[s] .. d_seg_ptr[s+1] (what rank s sent; ascending by column;
 * total_rows = d_seg_ptr[n_segments], passed on the host too to size the launch).
 * Records of one column are added in segment (= rank) order, the row is updated from
 * the owner's d_V / d_w (read only), and d_out_rows -- same number of records -- holds
 * [column, V_new[column,:], w_new[column]] at the position of the column's first
 * record and column = -1 at the positions of its other records. */
int32_t rfm_fm_reduce_rows(rfm_ctx* ctx, const double* d_rows, const int32_t* d_seg_ptr,
                           int32_t n_segments, int64_t total_rows, const double* d_w,
                           const double* d_V, int64_t n_features, int32_t n_factors, double lr,
                           double* d_out_rows);
/* Store updated rows ([column, V_new row, w_new]; column < 0 = skip; columns distinct)
 * into a replica, and w0 -= lr * (d_gw0_parts[0] + d_gw0_parts[part_stride] + ...,
 * n_parts terms in that order) when n_parts > 0. */
int32_t rfm_fm_set_rows(rfm_ctx* ctx, const double* d_rows, int64_t n_rows,
                        const double* d_gw0_parts, int32_t n_parts, int64_t part_stride,
                        double* d_w0, double* d_w, double* d_V, int64_t n_features,
                        int32_t n_factors, double lr);

/* ---- FM: the fit() loop --------------------------------------------------
 * Replaces the body of FactorizationMachines.fit (src/fm.py:71-102) for
 * iterations [0, n_iters): step on batch d_ids[it*batch ...], then the train
 * loss of the SAME batch with the new parameters, then the validation loss.
 * d_out_train_loss / d_out_val_loss receive one value per iteration (either
 * may be NULL to skip that forward).  Everything is enqueued on the ctx
 * stream; nothing synchronises.  For even factor counts above 128 (every published run of the
 * reference) the two loss forwards are ONE launch sliced by factors that keeps the log's frequent
 * columns in LDS, once the batch and the validation log together have RFM_SLICED_MIN_ROWS rows
 * (default 4 096; RFM_SLICED_LOSS=0: never) -- same losses up to the order of the sums.  The
 * other loss forwards leave their rows' scores and one launch per run of iterations takes the
 * logarithms (RFM_DEFER_LOSS=0: inside the forward); at small batches the train-loss rows of an
 * iteration are scored inside the NEXT iteration's forward launch (RFM_RIDE_LOSS=0: apart), and so
 * are the rows of a small validation log registered with rfm_fm_plan_register_log (RFM_RIDE_VAL=0). */
int32_t rfm_fm_train(rfm_ctx* ctx, rfm_fm_plan* plan, const int64_t* d_indptr,
                     const int32_t* d_indices, const double* d_values, const double* d_y,
                     const double* d_pscore, const int32_t* d_ids, int64_t batch,
                     int64_t n_iters, double* d_w0, double* d_w, double* d_V, double lr,
                     const int64_t* d_val_indptr, const int32_t* d_val_indices,
                     const double* d_val_values, const double* d_val_y,
                     const double* d_val_pscore, int64_t n_val, double eps,
                     double* d_out_train_loss, double* d_out_val_loss);
/* rfm_fm_train for a piece of a longer call (src/fm.py:71-102, cut where the caller has something
 * to enqueue between two iterations -- the catalogue metrics of DESIGN.md 8 N8): n_iters
 * iterations of a call that would have had call_iters >= n_iters of them.  rfm_fm_train chooses
 * the form of its loss forwards by the length of the call (a call of fewer than 4 iterations takes
 * the logarithms inside the forward), and the forms differ in the order of their sums; here the
 * form is the one a call of call_iters iterations takes, so the pieces of a call leave the losses
 * that call leaves, bit for bit where the fit is reproducible at all.  Everything else is
 * rfm_fm_train's. */
int32_t rfm_fm_train_part(rfm_ctx* ctx, rfm_fm_plan* plan, const int64_t* d_indptr,
                          const int32_t* d_indices, const double* d_values, const double* d_y,
                          const double* d_pscore, const int32_t* d_ids, int64_t batch,
                          int64_t n_iters, double* d_w0, double* d_w, double* d_V, double lr,
                          const int64_t* d_val_indptr, const int32_t* d_val_indices,
                          const double* d_val_values, const double* d_val_y,
                          const double* d_val_pscore, int64_t n_val, double eps,
                          double* d_out_train_loss, double* d_out_val_loss, int64_t call_iters);
/* The launch shape of a forward of n_rows rows at n_factors factors (nothing is launched):
 * h_out4[0]=threads per workgroup (1024: the many-rows shape, lane groups with several rows in
 * flight; 256: one row per lane group), [1]=workgroups, [2]=rows of a workgroup's trip (lane
 * groups * rows in flight), [3]=lanes per row.  records != 0: a forward through a plan's records
 * (the training step, the train-loss forward); 0: through the caller's CSR arrays (rfm_fm_forward,
 * rfm_fm_forward_loss, the validation-loss forward). */
int32_t rfm_fm_forward_geometry(const rfm_ctx* ctx, int64_t n_rows, int32_t n_factors, int32_t records,
                                int32_t* h_out4);
/* The forward launch of a step of `batch` rows on this plan (rfm_fm_step, the steps of rfm_fm_train),
 * with n_riding_rows rows of another batch riding in it (0: none); nothing is launched.
 * h_out8[0]=threads per workgroup, [1]=workgroups that score the batch's rows (riding rows add
 * theirs), [2]=rows of a workgroup's trip, [3]=lanes per row of the kernel that runs (8 for the
 * 8-lane kernel of k = 20, 24, 28, 32, where rfm_fm_forward_geometry reports the plan's 16),
 * [4]=the form, RFM_FWD_*, [5]=1 the 8-lane kernel, [6]=bytes of LDS per workgroup, [7]=1 the
 * hot-class sums in a fixed order.  Fails where the step would: riding rows on a step of the
 * many-rows shape or with fixed-order hot sums. */
enum {
  RFM_FWD_CSR = 0,         /* the caller's CSR arrays (never a step) */
  RFM_FWD_CSR_PAIR = 1,    /* ... of two logs in one launch (never a step) */
  RFM_FWD_RECORDS = 2,     /* the plan's row and entry records */
  RFM_FWD_BLOCKS = 3,      /* the plan's padded row blocks */
  RFM_FWD_RECORDS_FIXED = 4, /* records / blocks, hot-class sums in a fixed order */
  RFM_FWD_BLOCKS_FIXED = 5,
  RFM_FWD_RECORDS_RIDERS = 6, /* records / blocks, with riding rows */
  RFM_FWD_BLOCKS_RIDERS = 7
};
int32_t rfm_fm_step_form(const rfm_ctx* ctx, const rfm_fm_plan* plan, int64_t batch, int64_t n_riding_rows,
                         int32_t* h_out8);
/* The launch of a sliced forward of n_rows rows through this plan (rfm_fm_plan_forward; the loss
 * forwards of rfm_fm_train with n_rows = batch + n_val), form_rows >= 0: the decision between the
 * sliced and the plain form taken for that many rows instead (a shard of a log), -1: for n_rows.
 * Nothing is launched; the environment switches are read as the call reads them.  h_out4[0]=1 if
 * the sliced form is taken (0: the plan has no slices, the rows are too few, RFM_SLICED_LOSS=0; the
 * call then takes the plain forward and [1..3] say nothing), [1]=workgroups, [2]=rows per workgroup
 * (a wavefront takes every 16th of them, in blocks of 64), [3]=bytes of LDS per workgroup. */
int32_t rfm_fm_sliced_geometry(const rfm_ctx* ctx, const rfm_fm_plan* plan, int64_t n_rows, int64_t form_rows,
                               int32_t* h_out4);
/* The forms of the loss forwards that rfm_fm_train (call_iters = 0) or rfm_fm_train_part would
 * take with this plan, batch, n_iters, call_iters and validation log, want_train / want_val saying
 * which of d_out_train_loss / d_out_val_loss is given (nothing is launched; the environment
 * switches are read as the call reads them): h_out8[0]=1 sliced by factors, [1]=1 both losses in
 * one merged launch, [2]=1 the forwards leave scores and a run's logarithms come later, [3]=1 the
 * train rows ride in the next step's forward launch, [4]=1 so do the validation rows, [5]=iterations
 * of a run, [6]=threads per workgroup of the launch that scores the train-loss rows (0: not asked
 * for), [7]=... the validation-loss rows.  Riding rows: [6] / [7] are the step's forward launch
 * they ride in (256 threads); the rows of the call's LAST iteration, which has no next step, are
 * scored by a launch of their own, of the one-row shape as well. */
int32_t rfm_fm_train_forms(const rfm_ctx* ctx, const rfm_fm_plan* plan, int64_t batch, int64_t n_iters,
                           int64_t call_iters, const int64_t* d_val_indptr, const int32_t* d_val_indices,
                           const double* d_val_values, int64_t n_val, int32_t want_train, int32_t want_val,
                           int32_t* h_out8);
/* rfm_fm_train with the evaluator hook of the reference's search loop inside
 * (utils/search_params.py:96-111: fit(..., evaluator=ValEvaluator) -- after every iteration the
 * scores of the evaluation log, src/fm.py:104-110, and their IPS-DCG@k, utils/evaluate.py:160-207):
 * iteration i of the call leaves the scores of the n_ev rows of the evaluation CSR in
 * d_scores + (slot_first + i) * scores_stride (through rfm_fm_plan_forward), the per-group values
 * of rfm_val_dcg in d_user_scratch + (slot_first + i) * user_stride (>= 3 * n_segments doubles) and
 * its two results in d_dcg_out[2 i], [2 i + 1].  d_seg_ptr / d_rows / d_labels / d_ev_pscores /
 * n_segments / k: as rfm_val_dcg.  One enqueue for the whole run of iterations; nothing synchronises. */
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
                          double* d_dcg_out);

/* ---- FM: the data-parallel fit() loop ------------------------
 * The reference has no multi-process mode; this is the body of FactorizationMachines.fit
 * (src/fm.py:71-102) for one rank of n_ranks replicas: per iteration the rank computes the
 * batch-SUM gradient of ITS contiguous shard of the global batch d_ids[it*global_batch ..)
 * (rank r takes rows [r*q + min(r, m), ...) with q, m = divmod(global_batch, n_ranks): the
 * first m ranks one row more), the shards' gradients are combined, every replica applies
 * the same update, then the train loss of the same global batch with the new parameters
 * (src/fm.py:90-96; every rank its shard) and the validation loss (src/fm.py:98-102; the
 * validation rows cut the same way) are formed as sums, combined over the ranks and
 * written -- the same value on every rank -- to d_out_train_loss / d_out_val_loss
 * (n_iters doubles each, either may be NULL).
 *   exchange 0 (dense, what the north star names): all-reduce(sum) of [G_V | g_w | g_w0],
 *     n_features*(n_factors+1)+1 doubles per iteration, then rfm_fm_apply.
 *   exchange 1 (touched rows, feature-range ownership): rank r owns the columns
 *     [n_features*r/n_ranks, n_features*(r+1)/n_ranks); per iteration the gradient records
 *     of rfm_fm_grad_rows (+ one record for g_w0, owned by the last rank) go to the owners,
 *     an owner adds the records of a column in RANK ORDER, updates its row and sends the
 *     updated rows to everybody (rfm_fm_reduce_rows / rfm_fm_set_rows): each row is
 *     computed once and copied, the replicas stay bit-identical.  Which columns a shard
 *     touches depends on the row ids only, so the sizes of every transfer of the whole
 *     call are derived BEFORE the loop (one count pass per iteration, one all-gather of the
 *     counts, one host synchronisation per call); inside the loop nothing synchronises and
 *     nothing is allocated.
 * Transport: `transport` == NULL -> RCCL on the communicator of rfm_comm_init (n_ranks and the
 * rank are its; no communicator = one rank, nothing is exchanged), everything on the ctx
 * stream.  Otherwise the caller's functions move the (device) buffers -- e.g. staged through
 * the host over another fabric, or ranks that share one GPU in a test; each must be ordered
 * after the work already enqueued on the ctx stream and complete before it returns (or
 * be enqueued on that stream).  Offsets and sizes are bytes; entry p of an array belongs to
 * peer p (the rank's own entry included: a local copy).  Return 0 for success.
 * The call ends with one synchronisation (it reads back an error flag: a transfer plan that
 * does not match what the gradient kernels produced is RFM_ERR_INTERNAL, never a silent
 * truncation). */
typedef struct rfm_transport {
  void* user;
  int32_t n_ranks, rank;
  int32_t (*all_gather)(void* user, const void* d_send, void* d_recv, int64_t bytes_per_rank);
  int32_t (*all_reduce_sum)(void* user, double* d_buf, int64_t count);
  int32_t (*all_to_all)(void* user, const void* d_send, const int64_t* h_send_off,
                        const int64_t* h_send_bytes, void* d_recv, const int64_t* h_recv_off,
                        const int64_t* h_recv_bytes);
} rfm_transport;
int32_t rfm_fm_fit_dp(rfm_ctx* ctx, rfm_fm_plan* plan, const rfm_transport* transport,
                      int32_t exchange, const int32_t* d_ids, int64_t global_batch,
                      int64_t n_iters, double* d_w0, double* d_w, double* d_V, double lr,
                      const int64_t* d_val_indptr, const int32_t* d_val_indices,
                      const double* d_val_values, const double* d_val_y,
                      const double* d_val_pscore, int64_t n_val, double eps,
                      double* d_out_train_loss, double* d_out_val_loss);
/* rfm_fm_fit_dp with the evaluator of the reference's search loop inside (utils/search_params.py:
 * 96-111: fit(..., evaluator=ValEvaluator), scored after every iteration, src/fm.py:104-110, as
 * IPS-DCG@k, utils/evaluate.py:160-207) -- the data-parallel form of rfm_fm_train_eval.  The
 * evaluation log's user groups (ascending user, as rfm_val_dcg) are cut into n_ranks contiguous
 * ranges: rank r owns groups h_group_lo[r] .. h_group_lo[r + 1] - 1 (h_group_lo: n_ranks + 1 ints
 * on the HOST, h_group_lo[n_ranks] = n_segments; a rank may own none) and holds only their rows,
 * in grouped order, as the CSR d_ev_* of n_ev rows; d_seg_ptr / d_rows / d_labels / d_ev_pscores /
 * n_local_segments / k describe them as rfm_val_dcg's arguments do.  After the update of
 * iteration i the rank scores its rows (through rfm_fm_plan_forward, in the form -- sliced or
 * plain -- that the whole log's n_ev_total rows take, so every score is bitwise the whole log's)
 * into d_scores + (slot_first + i) * scores_stride and leaves its groups' per-user values in
 * d_user_scratch + (slot_first + i) * user_stride as [vals | counted | order-dependent], each part
 * max_local_segments apart (user_stride >= 3 * max_local_segments, the same on every rank, as is
 * max_local_segments >= every rank's group count).  After the loop, next to the loss all-reduce,
 * ONE all-gather moves the n_iters * user_stride doubles of every rank to every rank; they are
 * merged into d_full_out[i][3 * n_segments] -- the table one rfm_val_dcg over the whole log
 * would leave -- and its mean and order-dependent count go to d_dcg_out[2 i], [2 i + 1], bit for
 * bit what rfm_val_dcg gives, the same on every rank.  Nothing inside the loop synchronises.
 * With transport == NULL the all-gather is RCCL's (one process per GPU; not run on hardware with
 * more than one rank). */
int32_t rfm_fm_fit_dp_eval(rfm_ctx* ctx, rfm_fm_plan* plan, const rfm_transport* transport,
                           int32_t exchange, const int32_t* d_ids, int64_t global_batch,
                           int64_t n_iters, double* d_w0, double* d_w, double* d_V, double lr,
                           const int64_t* d_val_indptr, const int32_t* d_val_indices,
                           const double* d_val_values, const double* d_val_y,
                           const double* d_val_pscore, int64_t n_val, double eps,
                           double* d_out_train_loss, double* d_out_val_loss,
                           const int64_t* d_ev_indptr, const int32_t* d_ev_indices,
                           const double* d_ev_values, int64_t n_ev, int64_t n_ev_total,
                           const int32_t* d_seg_ptr, const int32_t* d_rows, const double* d_labels,
                           const double* d_ev_pscores, int32_t n_local_segments, int32_t k,
                           double* d_scores, int64_t scores_stride, double* d_user_scratch,
                           int64_t user_stride, int64_t slot_first, const int32_t* h_group_lo,
                           int32_t max_local_segments, int32_t n_segments, double* d_full_out,
                           double* d_dcg_out);

/* kinds of rfm_fm_plan_set_optimizer */
#define RFM_FM_OPT_SGD 0
#define RFM_FM_OPT_ADAGRAD 1

/* ---- FM: the optimiser seam ---------------------------------------------------------
 * The reference builds w0, w and V as SGD(params, lr) objects behind BaseOptimizer.update(grad,
 * index) (utils/optimizer.py, src/fm.py:48-50); another rule there is another subclass.  Here the
 * rule is fused into the gradient launch, so it is a property of the plan whose steps run it.
 *
 * kind = RFM_FM_OPT_SGD (a new plan's rule): theta -= lr * g.  The accumulator arguments and eps
 * are ignored and nothing is kept of them.
 *
 * kind = RFM_FM_OPT_ADAGRAD: every element of w0, w and V has an accumulator G of its own in
 * d_acc_w0[1], d_acc_w[n_features], d_acc_V[n_features][n_factors] (float64, the caller's device
 * memory, read and written by every step, kept alive by the caller while the rule is set).  With g
 * the element's batch-SUM gradient, bit for bit what rfm_fm_grad writes for it,
 *   G_new     = G + g * g                            (the product rounded, then the sum)
 *   theta_new = theta - (lr * g) / (sqrt(G_new) + eps)
 * in IEEE basic operations, all three gradients from the residual before the update
 * (src/fm.py:80-88).  g = 0 is a no-op, so which columns a step visits cannot be seen in the
 * result; a column no batch row holds keeps the bits of its parameters and accumulators.
 *
 * The rule is taken by rfm_fm_step, rfm_fm_train, rfm_fm_train_part and rfm_fm_train_eval.
 * rfm_fm_grad and rfm_fm_grad_rows form g alone under any rule.  rfm_fm_fit_dp and
 * rfm_fm_fit_dp_eval apply gradients that were summed over ranks with the SGD rule and return
 * RFM_ERR_BAD_ARG on a plan whose rule is another.
 * RFM_ERR_BAD_ARG: a kind outside the two, AdaGrad with a null accumulator or eps <= 0 (or NaN);
 * the plan's rule is then unchanged. */
int32_t rfm_fm_plan_set_optimizer(rfm_fm_plan* plan, int32_t kind, double* d_acc_w0, double* d_acc_w,
                                  double* d_acc_V, double eps);
/* h_out[0] = the plan's kind */
int32_t rfm_fm_plan_optimizer(const rfm_fm_plan* plan, int32_t* h_out);

/* ---- MF ------------------------------------------------------------------
 * Replaces LogisticMatrixFactorization.predict/_predict_pair
 * (src/mf.py:136-170): out[t] = sigmoid(clip(P_u . Q_i + b_u + b_i + b)). */
int32_t rfm_mf_predict(rfm_ctx* ctx, const int32_t* d_users, const int32_t* d_items,
                       const int32_t* d_row_ids, int64_t n_rows, const double* d_P,
                       const double* d_Q, const double* d_bu, const double* d_bi, double b,
                       int32_t n_factors, double* d_out_pred);
int32_t rfm_mf_predict_loss(rfm_ctx* ctx, const int32_t* d_users, const int32_t* d_items,
                            const double* d_y, const double* d_pscore,
                            const int32_t* d_row_ids, int64_t n_rows, const double* d_P,
                            const double* d_Q, const double* d_bu, const double* d_bi,
                            double b, int32_t n_factors, double eps, double* d_out_pred,
                            double* d_out_loss);

/* Order-preserving schedule of one batch (host): the reference updates the
 * batch strictly sequentially (src/mf.py:97-108).  Example s must run after
 * the latest earlier example sharing its user or its item; level(s) = 1 +
 * max(level of those).  Examples of one level touch disjoint rows, so running
 * the levels in order reproduces the sequential result exactly.
 * h_users/h_items: ids of the batch in batch order.  h_order[batch] receives
 * the batch positions grouped by level (ascending position inside a level),
 * h_level_ptr[n_levels+1] (capacity batch+1) the group boundaries;
 * *h_n_levels the number of levels. */
int32_t rfm_mf_schedule(const int32_t* h_users, const int32_t* h_items, int64_t batch,
                        int32_t n_users, int32_t n_items, int32_t* h_order,
                        int32_t* h_level_ptr, int32_t* h_n_levels);

/* Replaces the inner loop src/mf.py:97-108 with _update_P/_Q/_b_u/_b_i
 * (src/mf.py:172-216): for each level in order, for each example of the level
 * (independent): err = y/p - predict; P_u -= lr(-err Q_i + reg P_u); Q_i -=
 * lr(-err P_u(new) + reg Q_i); b_u, b_i likewise.  d_order/h_level_ptr from
 * rfm_mf_schedule (level_ptr both on the host, to size the launches, and on
 * the device); d_pos_rows[s] is the training row of batch position s. */
int32_t rfm_mf_sgd_levels(rfm_ctx* ctx, const int32_t* d_users, const int32_t* d_items,
                          const double* d_y, const double* d_pscore,
                          const int32_t* d_pos_rows, const int32_t* d_order,
                          const int32_t* h_level_ptr, const int32_t* d_level_ptr,
                          int32_t n_levels, double* d_P,
                          double* d_Q, double* d_bu, double* d_bi, double b,
                          int32_t n_factors, double lr, double reg);

/* The same schedule in the form the fast kernels read: the batch's examples as
 * 24-byte records {int32 user, int32 item, int32 cache_slot, int32 gap, double
 * label/propensity} grouped by level (ascending batch position inside a level).
 * h_users/h_items/h_y/h_pscore are the batch in batch order.  Up to cache_cap items
 * that occur more than once in the batch (most frequent first) are listed in
 * h_cache_items: the sequential kernel keeps their rows in LDS (cache_slot >= 0;
 * -1 = the item occurs once, -2 = repeated without a slot); gap = levels between the
 * example and the previous writer of its user row (RFM_MF_NO_WRITER if none), i.e.
 * how far ahead of its level the row is final and may be read.  The cached rows must
 * fit the kernel's LDS: cache_cap <= rfm_mf_cache_capacity(n_factors) (32 KiB of rows, at most 1024).  Capacities: h_ex batch records, h_level_ptr batch+1,
 * h_cache_items cache_cap. */
/* Item rows (with their bias) the sequential kernel may keep in LDS for one batch: the largest
 * cache_cap rfm_mf_schedule_ex / rfm_mf_sgd_levels_ex accept for this factor count. */
int32_t rfm_mf_cache_capacity(int32_t n_factors, int32_t* h_out);
int32_t rfm_mf_schedule_ex(const int32_t* h_users, const int32_t* h_items, const double* h_y,
                           const double* h_pscore, int64_t batch, int32_t n_users,
                           int32_t n_items, int32_t cache_cap, void* h_ex,
                           int32_t* h_level_ptr, int32_t* h_n_levels, int32_t* h_cache_items,
                           int32_t* h_n_cached);
/* rfm_mf_sgd_levels on those records (d_ex = device copy of h_ex, d_cache_items of
 * h_cache_items; n_cached rows of n_factors+2 doubles must fit 32 KiB of LDS).
 * Pinned by tests/test_gpu_mf_step.py: level sizes may grow as well as shrink (small and
 * large levels alternate in any order); every factor count 1..RFM_MAX_FACTORS is served;
 * one call may take several launches, and the cached rows are consistent in memory between
 * them (written back at the end of a launch, loaded again at the start of the next), so a
 * level launched grid-wide in between reads and writes them through memory. */
int32_t rfm_mf_sgd_levels_ex(rfm_ctx* ctx, const void* d_ex, const int32_t* h_level_ptr,
                             const int32_t* d_level_ptr, int32_t n_levels,
                             const int32_t* d_cache_items, int32_t n_cached, double* d_P,
                             double* d_Q, double* d_bu, double* d_bi, double b,
                             int32_t n_factors, double lr, double reg);

/* models of one rfm_mf_sgd_levels_many / rfm_mf_predict_many call */
#define RFM_MF_MAX_MODELS 1024

/* ---- MF: several models on one schedule --------------------------------------------
 * Models that are fitted on the same (user, item) log with the same batch_size draw the same
 * batch ids in every iteration (resample(..., random_state=epoch), src/mf.py:88-95, does not
 * depend on the model) and so share the level schedule; they differ in their parameters, lr,
 * reg, b and in label / propensity.  The schedule is derived once and the device runs it for
 * every model: one sequential workgroup per model, wide levels on a grid with a model
 * dimension.  Each model's result has the bits of its own rfm_mf_sgd_levels_ex.
 *
 * rfm_mf_schedule_rows is rfm_mf_schedule_ex for such a shared schedule: h_rows[batch] (the
 * training-log row of each batch position) in place of h_y / h_pscore; the same records, level
 * pointers, cached items and counts, every record's label / propensity a quiet NaN, and
 * h_ex_rows[batch] = the training-log row of each record, in level order. */
int32_t rfm_mf_schedule_rows(const int32_t* h_users, const int32_t* h_items, const int32_t* h_rows,
                             int64_t batch, int32_t n_users, int32_t n_items, int32_t cache_cap,
                             void* h_ex, int32_t* h_ex_rows, int32_t* h_level_ptr,
                             int32_t* h_n_levels, int32_t* h_cache_items, int32_t* h_n_cached);

/* One model of a many-model call, in device memory.  A table of these is built once per fit: no
 * launch rewrites it, and what changes per iteration travels by value. */
typedef struct rfm_mf_model {      /* 64 bytes */
  double *P, *Q, *bu, *bi;
  const double* ry;                /* [rows of the training log] label / propensity, divided on the host */
  double b, lr, reg;
} rfm_mf_model;
/* Labels and propensities of a scored log, per model (rfm_mf_predict_loss_many divides on the
 * device, as rfm_mf_predict_loss does). */
typedef struct rfm_mf_labels {     /* 16 bytes */
  const double *y, *pscore;
} rfm_mf_labels;

/* Replaces the inner loop src/mf.py:97-108 with _update_P/_Q/_b_u/_b_i (src/mf.py:172-216) of
 * n_models fits at once: rfm_mf_sgd_levels_ex on the records of rfm_mf_schedule_rows for every
 * model of d_models[n_models], model m reading label / propensity d_models[m].ry[d_ex_rows[rec]].
 * The launches are those of rfm_mf_sgd_levels_ex for the same level pointers; a run of small
 * levels is one launch of n_models sequential workgroups, a wide level one launch whose grid has
 * the model as its second dimension.  The models' arrays must not overlap.
 * 1 <= n_models <= RFM_MF_MAX_MODELS. */
int32_t rfm_mf_sgd_levels_many(rfm_ctx* ctx, const void* d_ex, const int32_t* d_ex_rows,
                               const int32_t* h_level_ptr, const int32_t* d_level_ptr,
                               int32_t n_levels, const int32_t* d_cache_items, int32_t n_cached,
                               const rfm_mf_model* d_models, int32_t n_models, int32_t n_factors);
/* Replaces LogisticMatrixFactorization.predict (src/mf.py:136-170) and the loss of
 * src/base.py:37-61 for n_models models on one log: rfm_mf_predict / rfm_mf_predict_loss with a
 * model dimension.  The rows are walked by the grid of the single-model call and the partial sums
 * are added in its order, so each model's scores and loss have the bits of its own call.  Model
 * m's scores go to d_out_base[m] + out_offset (d_out_base: a device table of n_models pointers,
 * built once; NULL in rfm_mf_predict_loss_many: no scores), its loss to
 * d_out_loss[m * loss_stride]; d_labels[m] names its labels and propensities of the scored log. */
int32_t rfm_mf_predict_many(rfm_ctx* ctx, const int32_t* d_users, const int32_t* d_items,
                            const int32_t* d_row_ids, int64_t n_rows, const rfm_mf_model* d_models,
                            int32_t n_models, int32_t n_factors, double* const* d_out_base,
                            int64_t out_offset);
int32_t rfm_mf_predict_loss_many(rfm_ctx* ctx, const int32_t* d_users, const int32_t* d_items,
                                 const rfm_mf_labels* d_labels, const int32_t* d_row_ids,
                                 int64_t n_rows, const rfm_mf_model* d_models, int32_t n_models,
                                 int32_t n_factors, double eps, double* const* d_out_base,
                                 int64_t out_offset, double* d_out_loss, int64_t loss_stride);
/* The launch shapes of the three calls above (host only, nothing is launched): h_out7[0]=threads
 * of the sequential workgroup, [1]=lanes per row, [2]=sequential workgroups (one per model),
 * [3], [4]=grid x and y of a wide level of n_recs records, [5], [6]=grid x and y of a prediction
 * over n_recs rows.  ctx == NULL: the grids on a device of 256 CUs (an MI355X). */
int32_t rfm_mf_many_geometry(const rfm_ctx* ctx, int32_t n_models, int32_t n_factors, int64_t n_recs,
                             int32_t* h_out7);

/* kinds of rfm_mf_sgd_levels_opt: the numbering of RFM_FM_OPT_* */
#define RFM_MF_OPT_SGD RFM_FM_OPT_SGD
#define RFM_MF_OPT_ADAGRAD RFM_FM_OPT_ADAGRAD

/* ---- MF: the optimiser seam ---------------------------------------------------------
 * The reference builds P, Q, b_u and b_i as SGD(params, lr) objects behind
 * BaseOptimizer.update(grad, index) (utils/optimizer.py, src/mf.py:45-62); another rule there is
 * another subclass.  Here the rule is fused into the level kernels, so it is an argument of the
 * call that runs a batch.
 *
 * rfm_mf_sgd_levels_opt is rfm_mf_sgd_levels_ex (same records, level pointers, cached items and
 * rfm_mf_cache_capacity, same launches for the same level pointers) under the rule `kind`.
 *
 * kind = RFM_MF_OPT_SGD: exactly the launches and the bits of rfm_mf_sgd_levels_ex; the
 * accumulator arguments and eps are never read.
 *
 * kind = RFM_MF_OPT_ADAGRAD: every element of P, Q, b_u, b_i has an accumulator G of its own in
 * d_acc_P[n_users][n_factors], d_acc_Q[n_items][n_factors], d_acc_bu[n_users], d_acc_bi[n_items]
 * (float64, the caller's device memory, in / out).  Examples run in the strict batch order of the
 * level schedule.  For one example (u, i), err is formed once, before any of its updates, and then
 *   g = -err Q_i + reg P_u;       G_P[u] += g g;  P_u -= (lr g) / (sqrt(G_P[u]) + eps)
 *   g = -err P_u(new) + reg Q_i;  G_Q[i], Q_i likewise (the item row sees the updated user row)
 *   g = -err + reg b_u[u];        G_bu[u], b_u[u] likewise
 *   g = -err + reg b_i[i];        G_bi[i], b_i[i] likewise
 * element by element, G + g g as the product rounded, then the sum; root and quotient correctly
 * rounded.  A user or item outside the batch keeps the bits of its parameters and accumulators.
 * A cached item keeps its accumulator row and bias accumulator in LDS beside its parameter row
 * (twice the LDS per cached item); both are written back at the end of a launch.
 *
 * RFM_ERR_BAD_ARG: a kind outside the two, AdaGrad with a null accumulator or eps <= 0 (or NaN),
 * and whatever rfm_mf_sgd_levels_ex rejects; nothing is launched then. */
int32_t rfm_mf_sgd_levels_opt(rfm_ctx* ctx, const void* d_ex, const int32_t* h_level_ptr,
                              const int32_t* d_level_ptr, int32_t n_levels,
                              const int32_t* d_cache_items, int32_t n_cached, double* d_P,
                              double* d_Q, double* d_bu, double* d_bi, double b,
                              int32_t n_factors, double lr, double reg, int32_t kind,
                              double* d_acc_P, double* d_acc_Q, double* d_acc_bu, double* d_acc_bi,
                              double eps);

/* Host-only: what rfm_mf_sgd_levels_opt launches for `kind` and `n_factors` (ctx may be NULL).
 * h_out7 = {lanes per row, factors per lane and chunk, chunks per lane, threads of the sequential
 * workgroup, levels ahead of their use at which the accumulators are read (0: where they are
 * used), LDS bytes per cached item, levels ahead at which the parameter rows are read (the slots
 * of the read-ahead ring; 0: where they are used)}.  The largest level the sequential workgroup
 * takes does not depend on the kind. */
int32_t rfm_mf_opt_geometry(const rfm_ctx* ctx, int32_t kind, int32_t n_factors, int32_t* h_out7);

/* ---- MF fold-in: new rows of one side against the fixed other side ----------------
 * The per-example update of src/mf.py:99-108 with _update_P / _update_b_u (src/mf.py:172-216)
 * restricted to ONE side: new row r has factors x_r = d_rows[r][0..k) and bias c_r = d_bias[r]
 * (in / out; the caller's initial values, zeros for a cold start).  Its examples are
 * e = d_row_ptr[r] .. d_row_ptr[r+1]-1 in that order; example e names row d_ids[e] of the fixed
 * side d_F [n_fixed][k], d_fb [n_fixed] (Q, b_i for new users; P, b_u for new items -- the same
 * rule with the sides exchanged) and carries d_ry[e] = label / propensity.  n_passes passes are
 * made over the row's examples, each in order:
 *   err = ry_e - sigmoid(clip(x_r . F[j] + c_r + fb[j] + b));
 *   x_r -= lr (-err F[j] + reg x_r);  c_r -= lr (-err + reg c_r)   (err from before the row update)
 * Nothing of the fixed side is written; a row without examples keeps its bits.  For new users,
 * one pass and all item ids of the call distinct this is what the reference's sequential batch
 * does to those user rows.  One lane group per new row, one launch for any n_new; d_order
 * [n_new] hands the rows to the lane groups: the rows by descending example count (stable), so
 * that the lane groups of a wavefront have chains of similar length and the longest start first.
 * The ids are not checked on the device: every d_ids[e] must lie in 0 .. n_fixed-1, d_order must
 * be a permutation of 0 .. n_new-1.  n_new == 0 or n_passes == 0: no launch. */
int32_t rfm_mf_fold_in(rfm_ctx* ctx, const int64_t* d_row_ptr, const int32_t* d_ids, const double* d_ry,
                       const int32_t* d_order, int64_t n_new, const double* d_F, const double* d_fb,
                       int64_t n_fixed, double b, int32_t n_factors, double lr, double reg,
                       int32_t n_passes, double* d_rows, double* d_bias);
/* The launch shape of rfm_mf_fold_in for n_new rows at n_factors factors (host only, nothing is
 * launched): h_out6[0]=lanes per row, [1]=adjacent factors a lane owns per chunk, [2]=chunks per
 * lane, [3]=new rows per workgroup, [4]=workgroups, [5]=read-ahead depth in steps
 * (RFM_MF_FOLD_READ_AHEAD).  ctx == NULL: the grid on a device of 256 CUs (an MI355X). */
int32_t rfm_mf_fold_geometry(const rfm_ctx* ctx, int64_t n_new, int32_t n_factors, int32_t* h_out6);

/* ---- FM fold-in: the id column of new rows of one side against the fixed other side ----
 * The reference's loaders give every user and item a one-hot id column next to its feature columns;
 * a user or item that arrived after the fit has none.  New row r of one side has
 *   - its FEATURE SUMS, fixed: g_r = d_g[r][0..k), l_r = d_l[r], the A and L that rfm_fm_side_sums
 *     gives for its feature entries (no id entry stored);
 *   - its NEW ID COLUMN (entry 1), trained: weight w_r = d_w_new[r], factor row v_r = d_V_new[r][0..k)
 *     (in / out; the caller's initial values, zeros for a cold start);
 *   - its examples e = d_row_ptr[r] .. d_row_ptr[r+1]-1, each naming row j_e = d_ids[e] of the fixed
 *     side d_F [n_fixed][kpad], d_fL [n_fixed] (B, LI of the operands for a new user; A, LU for a new
 *     item) and carrying ry_e = d_ry[e] = label / propensity;  c = *d_c (w0), read on the device.
 * One pass is the reference's batch-sum step (src/fm.py:80-88, 135-187) on the batch of all of r's
 * examples, restricted to the new column:
 *     h_e   = g_r + F[j_e]
 *     z_e   = c + l_r + fL[j_e] + g_r.F[j_e] + w_r + v_r.h_e
 *     err_e = ry_e - sigmoid(clip(z_e, +-700))
 *     w_r  += lr * sum_e err_e;   v_r += lr * sum_e err_e h_e      (every err_e from before the update)
 * n_passes passes are made; there is no regularisation (the reference's FM has none).  On the model
 * grown by the new columns (stored last) one step of the reference on the batch of ALL examples of
 * the call does to the new columns of w and V exactly one pass of this rule.  After the last pass
 * the served operands of the row are written as well: d_A_new[r] = g_r + v_r (zero-padded to kpad),
 * d_L_new[r] = l_r + w_r + g_r.v_r, so that c + L_new[r] + fL[j] + A_new[r].F[j] is the FM logit of
 * the grown row.  A row without examples, or n_passes == 0, keeps the bits of w_r, v_r; A_new and
 * L_new are still written.  Nothing of the model or of the fixed side is written.
 * One workgroup per new row, its lane groups over the row's examples, partial sums added in a fixed
 * order: no atomics, the same inputs give the same bits, and p passes in one call equal p calls of
 * one pass bit for bit.  One launch for any n_new, no host wait; d_order [n_new] hands the rows to
 * the workgroups: the rows by descending example count (stable).  The ids are not checked on the
 * device (RFM_CHECK_IDS is not consulted: the check kernels belong to the pair entries): every
 * d_ids[e] must lie in 0 .. n_fixed-1, d_order must be a permutation of 0 .. n_new-1.
 * n_new == 0: no launch. */
int32_t rfm_fm_fold_in(rfm_ctx* ctx, const int64_t* d_row_ptr, const int32_t* d_ids, const double* d_ry,
                       const int32_t* d_order, int64_t n_new, const double* d_g, const double* d_l,
                       const double* d_F, const double* d_fL, int64_t n_fixed, const double* d_c,
                       int32_t n_factors, double lr, int32_t n_passes, double* d_w_new, double* d_V_new,
                       double* d_A_new, double* d_L_new);
/* The launch shape of rfm_fm_fold_in for n_new rows at n_factors factors (host only, nothing is
 * launched): h_out5[0]=lanes per example, [1]=adjacent factors a lane owns per chunk, [2]=chunks per
 * lane, [3]=lane groups per workgroup (examples of a row in flight), [4]=workgroups (one new row
 * each per grid-stride turn).  ctx == NULL: the grid on a device of 256 CUs (an MI355X). */
int32_t rfm_fm_fold_geometry(const rfm_ctx* ctx, int64_t n_new, int32_t n_factors, int32_t* h_out5);

/* ---- fold-in: the examples of a log in device memory, grouped by new row -----------
 * What fold.fold_examples does on the host, for a log that already lies in HBM: the n examples
 * (new-row id, other id, label, propensity) grouped by new row with a stable sort (a row's examples
 * keep their input order), label / propensity as an IEEE double quotient, and the new rows by
 * descending example count, ties in row order.  Everything is enqueued on the context's stream and
 * nothing waits for the device; rfm_mf_fold_in / rfm_fm_fold_in may be enqueued right behind.
 *
 * d_new, d_other: the FIRST element of each id column; consecutive examples lie id_stride elements
 * apart (2 for the columns of an (N, 2) array, 1 for separate arrays); id_bytes: 4 (int32) or 8
 * (int64).  d_labels, d_pscores: float64 [n].  Inputs are never written.
 *
 * Outputs, as the two fold-in entries take them: d_row_ptr int64 [n_new + 1]; d_ids int32 [n] (the
 * other column in grouped order); d_ry float64 [n]; d_order int32 [n_new]; d_status int32 [4]:
 * [0] = examples whose new-row id lies outside 0..n_new-1, [1] = examples whose other id lies outside
 * 0..n_fixed-1, [2] = the index of the first example counted in either, -1 if there is none,
 * [3] = 0 (spare).  Such an example is left out of every output: d_row_ptr[n_new] is the number of
 * examples kept, and only that many elements of d_ids / d_ry are written -- a fold launch behind this
 * call stays in bounds whatever the log holds.
 *
 * n_new == 0: the status and d_row_ptr[0] are zeroed, nothing else happens.  n == 0: d_row_ptr is
 * zeroed and d_order is 0..n_new-1 (the stable order of equal counts), one launch.
 * d_workspace: rfm_fold_group_workspace(n, n_new) bytes, 16-byte aligned, the caller's until the
 * stream has passed this call.  n, n_new < 2^31; anything else is RFM_ERR_BAD_ARG. */
int32_t rfm_fold_group(rfm_ctx* ctx, const void* d_new, const void* d_other, int64_t id_stride,
                       int32_t id_bytes, const double* d_labels, const double* d_pscores, int64_t n,
                       int64_t n_new, int64_t n_fixed, void* d_workspace, int64_t workspace_bytes,
                       int64_t* d_row_ptr, int32_t* d_ids, double* d_ry, int32_t* d_order,
                       int32_t* d_status);
/* Bytes of workspace of rfm_fold_group for n examples and n_new rows (host only). */
int32_t rfm_fold_group_workspace(int64_t n, int64_t n_new, int64_t* h_bytes);
/* The launch shape of one grouping of n keys into n_bins bins (host only, nothing is launched);
 * rfm_fold_group makes two: (n, n_new) for the examples and (n_new, n + 1) for the row order.
 * h_out8[0] = the longest bin that is ordered in LDS (the cap; a longer bin is rebuilt by a walk over
 * all keys), [1] = lanes per workgroup of the per-bin launches, [2] = workgroups of the per-bin launch
 * (a wavefront per bin and turn), [3] = the longest bin a wavefront orders (longer ones up to the cap
 * take a workgroup), [4] = workgroups of that workgroup-per-bin launch (0: not launched, no bin can be
 * that long), [5] = workgroups of the walk (0: not launched), [6] = lanes per workgroup of the walk,
 * [7] = workgroups of the per-key launches (count, place, gather).  ctx == NULL: the grids on a device
 * of 256 CUs (an MI355X). */
int32_t rfm_fold_group_geometry(const rfm_ctx* ctx, int64_t n, int64_t n_bins, int32_t* h_out8);

/* ---- MF across GPUs: user-range partition ------------------
 * NOT the reference's semantics (its batch is strictly sequential, src/mf.py:97-108;
 * exact mode = one GPU or independent replicas).  Throughput mode: rank r runs the exact
 * sequential SGD (rfm_mf_sgd_levels_ex) over the batch's examples whose USER lies in its
 * range, in batch order, on its own replica of Q / b_i; P / b_u rows are only ever
 * written by their owner.  After the batch each rank forms what its examples changed,
 * rfm_mf_delta: d_out = d_cur - d_sync, the deltas are all-reduced (sum), and
 * rfm_mf_merge: d_sync += d_total, d_cur = d_sync brings every replica to the same
 * values.  With one rank nothing is exchanged and the result is the reference's. */
int32_t rfm_mf_delta(rfm_ctx* ctx, const double* d_cur, const double* d_sync, double* d_out,
                     int64_t count);
int32_t rfm_mf_merge(rfm_ctx* ctx, double* d_cur, double* d_sync, const double* d_total,
                     int64_t count);

/* ---- multi-GPU exchange (RCCL over xGMI) ----------------------------------
 * The data-parallel FM step all-reduces the dense gradient buffer of rfm_fm_grad
 * (SURVEY.md 8e).  The Python mirror does that through torch.distributed (backend
 * "nccl" is RCCL); these entry points are the same collective for callers
 * without torch: rank 0 draws an id (128 bytes) and hands it to the other ranks
 * by any means, every rank calls rfm_comm_init on its own ctx (one process per
 * GPU), then rfm_allreduce_sum sums d_buf[0..count) in place over all ranks on
 * the ctx stream.  librccl.so is loaded on first use. */
int32_t rfm_comm_unique_id(uint8_t* h_out128);
int32_t rfm_comm_init(rfm_ctx* ctx, int32_t n_ranks, int32_t rank, const uint8_t* h_id128);
int32_t rfm_allreduce_sum(rfm_ctx* ctx, double* d_buf, int64_t count);
int32_t rfm_comm_destroy(rfm_ctx* ctx);

/* HOGWILD-style variant of the same batch (NOT the reference's semantics): all
 * examples of the batch are updated concurrently without ordering, so examples
 * sharing a user or an item race.  Throughput mode for very large batches; its
 * results match the reference only at the loss / ranking level, not 1e-5 on the
 * parameters.  d_pos_rows[s] is the training row of batch position s. */
int32_t rfm_mf_sgd_hogwild(rfm_ctx* ctx, const int32_t* d_users, const int32_t* d_items,
                           const double* d_y, const double* d_pscore,
                           const int32_t* d_pos_rows, int64_t batch, double* d_P, double* d_Q,
                           double* d_bu, double* d_bi, double b, int32_t n_factors, double lr,
                           double reg);

/* ---- per-iteration validation metric ---------------------
 * IPS-DCG@k of ValEvaluator.evaluate (utils/evaluate.py:183-207 with
 * utils/metrics.py:53-80), the value src/fm.py:104-110 and src/mf.py:126-132
 * append to val_metrics every iteration.  The frame's rows are grouped by user
 * (groups in ascending user order, rows of a group in frame order -- what
 * DataFrame.groupby("user").agg(list) yields): group g holds positions
 * d_seg_ptr[g] .. d_seg_ptr[g+1]; d_labels / d_pscores are indexed by position,
 * the score of position j is d_scores[d_rows[j]] (d_rows == NULL: d_scores[j]).
 * Per group: rows ranked by descending score, groups whose labels sum to zero are
 * left out, value = y0/p0 + sum_{r=1..k-1} y_r / (p_r * log2(r+1)); d_out[0] = mean
 * over the groups that count (nan if none).  Equal scores rank the later position
 * first, i.e. argsort(kind="stable")[::-1]; NumPy's default sort, which the
 * reference calls, is not stable and orders ties differently from CPU to CPU, so
 * d_out[1] = number of counted groups whose value depends on that order (a tie
 * reaching into the first k ranks between rows of different label or propensity,
 * or a NaN score, which is never ranked here).  With d_out[1] == 0 the value is the
 * reference's; otherwise the caller decides (the Python mirror redoes exactly those
 * groups on the host with NumPy's own sort, from the per-group flags below).  d_pscores == NULL means all ones
 * (the Naive estimator's ones_pscore column; also calc_dcg_at_k of
 * utils/metrics.py:83-107).  d_user_scratch: 3*n_segments doubles; after the call
 * [0, n) holds the per-group values, [n, 2n) 1.0 / 0.0 for counted / left out and
 * [2n, 3n) 1.0 for the order-dependent groups. */
int32_t rfm_val_dcg(rfm_ctx* ctx, const double* d_scores, const int32_t* d_seg_ptr,
                    const int32_t* d_rows, const double* d_labels, const double* d_pscores,
                    int32_t n_segments, int32_t k, double* d_user_scratch, double* d_out);

/* ---- test-set metrics -------------------------------------
 * The ranking half of TestEvaluator.evaluate (utils/evaluate.py:80-127): per user
 * group (same grouping arrays as rfm_val_dcg; d_items = item id per position, may
 * be NULL) the positions of the k best-scored rows, d_out_pos[g*k + r] = position
 * of rank r or -1 past the group's rows, same tie rule (later position first).
 * d_out_flags[g]: bit 0 = the group has a positive label (the others are left out
 * of every metric, evaluate.py:99-100); bit 1 = the first k ranks depend on how
 * equal scores are ordered (a tie between rows of different label, propensity or
 * item inside the first k ranks or across rank k, or a NaN score) -- the Python
 * mirror ranks exactly those groups again with NumPy's own sort.  DCG@K, Recall,
 * MAP, mean exposure, CatalogCoverage and Gini (utils/metrics.py:9-166) are sums
 * over these n_segments x k positions. */
int32_t rfm_topk_users(rfm_ctx* ctx, const double* d_scores, const int32_t* d_seg_ptr,
                       const int32_t* d_rows, const double* d_labels, const double* d_pscores,
                       const int32_t* d_items, int32_t n_segments, int32_t k, int32_t* d_out_pos,
                       int32_t* d_out_flags);

/* ---- CSR assembly -------------------------------------------
 * The step before the training path: the FM design matrix of the reference's loaders
 * -- one-hot user (+) one-hot item (+) per-interaction columns (+) the user's feature row
 * (+) the item's feature row, hstack'ed (utils/dataloader/kuairec/_feature.py:54-84,
 * 201-207; coat/_preparer.py:154-168) -- and the row selections made from it
 * (features[indices]: kuairec/_preparer.py:117-136, loader.py:104-115).  Output row r
 * is the concatenation, in segment order, of
 *   kind 0: the single entry (col_offset + d_ids[r], 1.0)          -- a one-hot of an id
 *   kind 1: row d_ids[r] (d_ids == NULL: row r) of a CSR block, its columns shifted by
 *           col_offset                            -- a feature table gathered by id
 * n_block_rows = rows of the block (kind 1) / size of the one-hot (kind 0); an id outside
 * it is RFM_ERR_BAD_ARG.  Blocks use the ABI's dtypes (indptr int64, indices int32,
 * values float64); stored zeros are kept as they are.  Call rfm_csr_assemble_count (fills
 * d_out_indptr[n_rows + 1], returns the number of entries on the host -- it synchronises),
 * allocate indices / values, then rfm_csr_assemble_fill. */
typedef struct rfm_csr_segment {
  int32_t kind;
  const int32_t* d_ids;
  const int64_t* d_indptr;
  const int32_t* d_indices;
  const double* d_values;
  int64_t col_offset;
  int64_t n_block_rows;
} rfm_csr_segment;
int32_t rfm_csr_assemble_count(rfm_ctx* ctx, const rfm_csr_segment* h_segments, int32_t n_segments,
                               int64_t n_rows, int64_t* d_out_indptr, int64_t* h_out_nnz);
int32_t rfm_csr_assemble_fill(rfm_ctx* ctx, const rfm_csr_segment* h_segments, int32_t n_segments,
                              int64_t n_rows, const int64_t* d_indptr, int32_t* d_out_indices,
                              double* d_out_values);

/* ---- catalogue scoring and top-K -----------------------------
 * Every (user, item) pair of a trained model without the design matrix of the pairs.  The FM
 * rows the reference's loaders build are "the user's entries + the item's entries" on disjoint
 * columns, x(u,i) = xu(u) + xi(i); with a_u = sum_j xu_j V[j,:], b_i = sum_j xi_j V[j,:] and, per
 * side, L(x) = w.x + 0.5 sum_f((sum_j x_j V[j,f])^2 - sum_j x_j^2 V[j,f]^2), the logit of
 * FactorizationMachines.predict (src/fm.py:114-133) is exactly
 *     logit(u,i) = w0 + L(xu) + L(xi) + a_u . b_i,
 * and LogisticMatrixFactorization._predict_pair (src/mf.py:136-170) has the same shape with
 * a = P, b = Q, L = b_u, b_i and the constant b.
 *
 * rfm_fm_side_sums: A[n_rows][kpad] and L[n_rows] of a CSR side matrix (one row per user, or
 * per item; dtypes as everywhere), kpad = n_factors rounded up to a multiple of 4, the padding
 * zero-filled.  Entries are summed in stored order and the factors in a fixed order: bitwise
 * reproducible.  A column index outside 0..n_features-1 is never read; with RFM_CHECK_IDS=1 it
 * is RFM_ERR_BAD_ARG (this synchronises), otherwise the entry is skipped. */
int32_t rfm_fm_side_sums(rfm_ctx* ctx, const int64_t* d_indptr, const int32_t* d_indices,
                         const double* d_values, int64_t n_rows, const double* d_w, const double* d_V,
                         int64_t n_features, int32_t n_factors, double* d_A, double* d_L);
/* d_out[s][i] = sigmoid(clip(*d_c + LU[u] + LI[i] + A[u,:].B[i,:], +-700)) (src/base.py:63-66; a
 * NaN logit stays NaN) for every item i and selected user s, u = d_user_ids ? d_user_ids[s] : s
 * (any order, repeats allowed; NULL needs n_sel_users == n_users).  A is [n_users][kpad], B is
 * [n_items][kpad] with kpad as above (MF: P and Q themselves when n_factors % 4 == 0); the
 * product runs on the f64 matrix core in 64 x 64 tiles.  *d_c is FM's w0 / MF's b, read on the
 * device.  A user id outside 0..n_users-1 scores NaN (RFM_CHECK_IDS=1: RFM_ERR_BAD_ARG). */
int32_t rfm_pair_scores(rfm_ctx* ctx, const double* d_A, const double* d_LU, int64_t n_users,
                        const int32_t* d_user_ids, int64_t n_sel_users, const double* d_B,
                        const double* d_LI, int64_t n_items, int32_t n_factors, const double* d_c,
                        double* d_out);
/* The k best items of every selected user, 1 <= k <= 64 (else RFM_ERR_BAD_ARG), under the TOTAL
 * order (logit descending, then item index descending): np.argsort(logit, kind="stable")[::-1][:k],
 * the tie rule of rfm_val_dcg / rfm_topk_users.  Ranking is by the logit, never by the
 * probability (which saturates to exactly 0.0 / 1.0).  A NaN logit is never ranked.
 * d_out_items[s][r] = item of rank r, d_out_scores[s][r] = its sigmoid(logit); fewer than k
 * rankable items pads with item -1 / score NaN.  Optional exclusion lists, CSR by USER ID
 * (d_excl_indptr[n_users + 1], strictly ascending item ids; NULL = none): a listed item is never
 * returned to that user.  The items are split over workgroups that keep partial lists in
 * d_workspace (rfm_pair_topk_workspace bytes; host only, a function of the three sizes), merged by
 * a second launch; because the order is total the result does not depend on the split, and no
 * float atomic is used: the same inputs give the same bits.  RFM_CHECK_IDS=1 validates the user
 * ids and the exclusion lists first (RFM_ERR_BAD_ARG; this synchronises). */
int32_t rfm_pair_topk_workspace(int64_t n_sel_users, int64_t n_items, int32_t k, int64_t* h_bytes);
int32_t rfm_pair_topk(rfm_ctx* ctx, const double* d_A, const double* d_LU, int64_t n_users,
                      const int32_t* d_user_ids, int64_t n_sel_users, const double* d_B,
                      const double* d_LI, int64_t n_items, int32_t n_factors, const double* d_c,
                      const int64_t* d_excl_indptr, const int32_t* d_excl_items, int32_t k,
                      void* d_workspace, int32_t* d_out_items, double* d_out_scores);
#include "rfm_neighbours.h"
/* Ranks against the whole catalogue: where given (user, item) pairs land in the
 * order rfm_pair_topk ranks by.  The first eleven arguments, the user ids, the exclusion lists and
 * RFM_CHECK_IDS are rfm_pair_topk's.  The CANDIDATES of selected user s are the items whose logit
 * is not NaN and that the user's exclusion list does not name; j is BETTER than i when
 * logit(j) > logit(i), or they are equal and j > i.  The TARGETS of selected user s are
 * d_tgt_items[d_tgt_indptr[s] .. d_tgt_indptr[s + 1]) (CSR by SELECTED user, not by user id;
 * d_tgt_indptr[0] = 0, item ids ascending, repeats allowed; n_targets = d_tgt_indptr[n_sel_users] is
 * read back from the device, which synchronises).  Per target t = (s, i):
 *     d_out_ranks[t]  = number of candidates j != i of s that are better than i (0-based), i.e. the
 *                       position of i in np.argsort(logit[s], kind="stable")[::-1] once the NaNs and
 *                       the excluded items are taken out; -1 if the target's own logit is NaN (NaN
 *                       item row, user id or item id outside its table);
 *     d_out_scores[t] = sigmoid(clip(logit, +-700)), NaN where the rank is -1;
 * and d_out_candidates[s] = the number of candidates of s.  A target that the exclusion list names
 * is still ranked, against the candidates (it is not one of them).  The logit is the pair tile's,
 * bit for bit: the rank of rfm_pair_topk's r-th item is r, and its score has the same bytes.  Two
 * passes over the product: the first stores the targets' logits in d_workspace
 * (rfm_pair_ranks_workspace bytes; host only), the second counts, per tile, the logits better
 * than each target.  Counts are integers added with integer atomics and no float atomic is used:
 * the result does not depend on the split of the items over workgroups, and the same inputs give
 * the same bits.  n_targets == 0 is legal (d_tgt_items, d_workspace, d_out_ranks, d_out_scores may
 * be NULL) and still fills d_out_candidates.  RFM_CHECK_IDS=1 validates user ids, exclusion lists
 * and target lists (ids inside 0..n_items-1, ascending) first: RFM_ERR_BAD_ARG. */
int32_t rfm_pair_ranks_workspace(int64_t n_sel_users, int64_t n_items, int64_t n_targets, int64_t* h_bytes);
int32_t rfm_pair_ranks(rfm_ctx* ctx, const double* d_A, const double* d_LU, int64_t n_users,
                       const int32_t* d_user_ids, int64_t n_sel_users, const double* d_B,
                       const double* d_LI, int64_t n_items, int32_t n_factors, const double* d_c,
                       const int64_t* d_excl_indptr, const int32_t* d_excl_items,
                       const int64_t* d_tgt_indptr, const int32_t* d_tgt_items, void* d_workspace,
                       int32_t* d_out_ranks, double* d_out_scores, int32_t* d_out_candidates);
/* rfm_pair_ranks with the number of targets given by the host: n_targets must be
 * d_tgt_indptr[n_sel_users].  Nothing is read back and nothing synchronises (unless RFM_CHECK_IDS=1),
 * so the call can be enqueued between the iterations of a fit; every other argument, the launches
 * and the results, byte for byte, are rfm_pair_ranks' (the ranks utils/metrics.py:9-107 are taken
 * from when the whole catalogue is ranked). */
int32_t rfm_pair_ranks_n(rfm_ctx* ctx, const double* d_A, const double* d_LU, int64_t n_users,
                         const int32_t* d_user_ids, int64_t n_sel_users, const double* d_B,
                         const double* d_LI, int64_t n_items, int32_t n_factors, const double* d_c,
                         const int64_t* d_excl_indptr, const int32_t* d_excl_items,
                         const int64_t* d_tgt_indptr, const int32_t* d_tgt_items, int64_t n_targets,
                         void* d_workspace, int32_t* d_out_ranks, double* d_out_scores,
                         int32_t* d_out_candidates);
/* Catalogue metrics from ranks, on the device: the reference's calc_dcg_at_k,
 * calc_recall_at_k and calc_average_precision_at_k (utils/metrics.py:9-107; the IPS form of the
 * DCG: calc_ips_of_dcg_at_k, utils/metrics.py:53-80) as they come out for the 0/1 vector of a
 * user's candidates in ranked order, plus MRR and AUC, from the ranks of the user's positives.
 * The targets are grouped as rfm_pair_ranks takes them (d_tgt_indptr[n_sel_users + 1], n_targets =
 * its last entry, given by the host); d_ranks[n_targets] is rfm_pair_ranks' output (-1 = unranked:
 * left out), d_candidates[n_sel_users] its candidate counts, d_weights[n_targets] an optional weight
 * per target (NULL = ones; 1 / propensity for the IPS estimate).  The targets of a user must be
 * distinct items, so that the ranks are.  h_K[n_K]: depths >= 1 on the host, 1 <= n_K <= 16.  Per
 * selected user with ranked positives r_1 < ... < r_P, weights v_j and C candidates:
 *     DCG@K    = sum_{r_j < K} v_j g(r_j),  g(0) = 1, g(r) = 1 / log2(r + 1)
 *     Recall@K = #{r_j < K} / P
 *     MAP@K    = sum_{r_j < K} j / (r_j + 1)
 *     MRR      = 1 / (r_1 + 1)
 *     AUC      = 1 - sum_j (r_j - (j - 1)) / (P (C - P)),  NaN when C <= P.
 * d_out[3 n_K + 2] = DCG@K[0..] | Recall@K[0..] | MAP@K[0..] | MRR | AUC: the mean of each column
 * over the users with at least one ranked positive, the AUC over those of them with C > P; NaN for a
 * column without a user.  d_out_counts[3] = users counted, users counted for the AUC, unranked
 * positives.  One wavefront per user orders the ranks by counting and adds a user's terms in
 * ascending rank order; the means are a second launch with a fixed order; no float atomic: the same
 * inputs give the same bits.  Nothing synchronises.  d_workspace: rfm_rank_metrics_workspace bytes
 * (host only).  An indptr that leaves 0..n_targets is clamped, never followed outside the arrays;
 * RFM_CHECK_IDS=1 makes it RFM_ERR_BAD_ARG (this synchronises). */
int32_t rfm_rank_metrics_workspace(int64_t n_sel_users, int64_t n_targets, int32_t n_K, int64_t* h_bytes);
int32_t rfm_rank_metrics(rfm_ctx* ctx, const int64_t* d_tgt_indptr, int64_t n_sel_users, int64_t n_targets,
                         const int32_t* d_ranks, const int32_t* d_candidates, const double* d_weights,
                         const int64_t* h_K, int32_t n_K, void* d_workspace, double* d_out,
                         int64_t* d_out_counts);
/* A user's ranking of the catalogue to any depth: the items at positions
 * 0 .. depth-1 of the order rfm_pair_topk and rfm_pair_ranks use, depth >= 1 and not bounded by 64 --
 * a candidate list for a re-ranker, a user's full ordering (depth >= n_items), and the lists the
 * reference's mean exposure, catalogue coverage and Gini are taken from (utils/metrics.py:110-166,
 * utils/evaluate.py:93-125) when the catalogue is what is ranked.  The first eleven arguments, the
 * user ids, the exclusion lists and RFM_CHECK_IDS are rfm_pair_topk's; candidates and BETTER are
 * rfm_pair_ranks'.  Per selected user s:
 *     d_out_items[s][r]  = the candidate at position r, -1 past the user's last candidate;
 *     d_out_scores[s][r] = sigmoid(clip(logit, +-700)) of that item, NaN where the item is -1;
 *     d_out_n_ranked[s]  = the number of candidates of s (rfm_pair_ranks' d_out_candidates).
 * +-inf logits are ordinary candidates; a user id outside the table gives an all-NaN row (items -1,
 * n_ranked 0).  The logit is the pair tile's, bit for bit, so the first min(depth, 64) columns are
 * rfm_pair_topk's bytes and rfm_pair_ranks of the r-th returned item is r.  Two stages per block of
 * users: the tile stores the block's raw logits [users][n_items] in d_workspace, then one workgroup
 * per user keeps the best min(depth, 4096) (rounded up to a power of two) in LDS while it streams
 * the row, sorting and merging a staging area of the same size (bitonic); deeper lists go in pages
 * of 4096 ranks, each page ranking what comes strictly after the last entry of the page before.
 * The caller chooses workspace_bytes: the users are worked through in blocks of as many rows as fit
 * (a multiple of 64).  rfm_pair_order_workspace (host only) gives the least size -- one block of 64
 * users, less is RFM_ERR_BAD_ARG -- and the size that takes every selected user in one block.  The
 * order is total and no float atomic is used: the result does not depend on the block cut, the
 * pages or timing, and the same inputs give the same bits. */
int32_t rfm_pair_order_workspace(int64_t n_sel_users, int64_t n_items, int64_t depth, int64_t* h_min_bytes,
                                 int64_t* h_preferred_bytes);
int32_t rfm_pair_order(rfm_ctx* ctx, const double* d_A, const double* d_LU, int64_t n_users,
                       const int32_t* d_user_ids, int64_t n_sel_users, const double* d_B,
                       const double* d_LI, int64_t n_items, int32_t n_factors, const double* d_c,
                       const int64_t* d_excl_indptr, const int32_t* d_excl_items, int64_t depth,
                       void* d_workspace, int64_t workspace_bytes, int32_t* d_out_items,
                       double* d_out_scores, int32_t* d_out_n_ranked);
/* The launches the rfm_pair_* entries make for these sizes (host only, no context; nothing is
 * launched; computed by the functions the launches are sized by).  rfm_pair_geometry, n_sel_users
 * >= 1: h_out8[0]=kpad, [1]=chunks of 32 factors a tile goes through, [2]=factors per MFMA k-slot
 * in the last chunk, (kpad - 32 ([1] - 1)) / 4 in 1..8, [3]=user tiles, [4]=item tiles (of 64),
 * and for the entries whose workgroups walk a split of the item tiles (rfm_pair_topk,
 * rfm_pair_ranks): [5]=splits, [6]=tiles per split, [7]=tiles of the last split.
 * rfm_pair_order_geometry: h_out4[0]=entries of the ranking kernel's list in LDS (a power of two,
 * 256..4096), [1]=items of a pass over the row, [2]=the staged count above which a flush (sort and
 * merge of the staging area) precedes a pass, [0] - [1]; the remainder is flushed after the last
 * pass, [3]=pages (launches of the ranking kernel per block of users). */
int32_t rfm_pair_geometry(int64_t n_sel_users, int64_t n_items, int32_t n_factors, int64_t* h_out8);
int32_t rfm_pair_order_geometry(int64_t n_items, int64_t depth, int64_t* h_out4);
#include "rfm_audience.h"
#include "rfm_diverse.h"

#ifdef __cplusplus
}
#endif
#endif /* RFM_HIP_H */
