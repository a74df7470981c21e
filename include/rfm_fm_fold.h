/* FM fold-in: the part of the C ABI of librfm_hip.so that trains the id column of users and items
 * which arrive after the fit.  Included by rfm_hip.h, which supplies rfm_ctx, the
 * status codes and the extern "C" block; the ctypes binding is _lib.FOLD_SIGNATURES, and
 * tests/test_fm_fold_host.py holds the two equal argument by argument. */
#ifndef RFM_FM_FOLD_H
#define RFM_FM_FOLD_H
#ifndef RFM_HIP_H
#error "include rfm_hip.h, which includes this file"
#endif

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

#endif /* RFM_FM_FOLD_H */
