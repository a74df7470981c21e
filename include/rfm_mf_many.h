/* Several MF models on one schedule: a part of the C ABI of librfm_hip.so.  Included by rfm_hip.h,
 * which declares rfm_ctx and the single-model entry points these extend; do not include it alone.
 * Bound from _lib.MF_MANY_SIGNATURES (tests/test_mf_many_host.py compares the two, argument by
 * argument). */
#ifndef RFM_MF_MANY_H
#define RFM_MF_MANY_H

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

#endif /* RFM_MF_MANY_H */
