/* Fold-in examples grouped on the device: a part of the C ABI of librfm_hip.so.  Included by
 * rfm_hip.h, which declares rfm_ctx and the two fold-in entries these feed; do not include it alone.
 * Bound from _lib.FOLD_GROUP_SIGNATURES (tests/test_fold_group_host.py compares the two, argument by
 * argument). */
#ifndef RFM_FOLD_GROUP_H
#define RFM_FOLD_GROUP_H

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

#endif /* RFM_FOLD_GROUP_H */
