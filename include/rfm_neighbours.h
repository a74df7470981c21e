/* Nearest neighbours in factor space: a part of the C ABI of librfm_hip.so.  Included by rfm_hip.h
 * (inside its extern "C"), which declares rfm_ctx and the rfm_pair_* entries that this extends; do
 * not include it alone.  It stands in a file of its own because tests/test_host_abi.py pins
 * rfm_hip.h and _lib.SIGNATURES at a fixed count of entries.  Bound from _lib.NEIGHBOUR_SIGNATURES
 * (tests/test_neighbours_host.py compares the two, argument by argument). */
#ifndef RFM_NEIGHBOURS_H
#define RFM_NEIGHBOURS_H

/* ---- nearest neighbours in factor space ----------------------
 * Which items are like this item, which users like this user: the rows of one of the two tables
 * of the catalogue entries -- b_i / Q, a_u / P; where they come from: src/fm.py:114-133, src/mf.py:136-170 -- compared
 * with each other by cosine or dot product.  The reference has no counterpart of either entry.
 *
 * rfm_pair_topk_raw: rfm_pair_topk's arguments, launches and workspace (rfm_pair_topk_workspace).
 * The one difference: d_out_values[s][r] is the logit itself, *d_c + LU[u] + LI[i] + A[u,:].B[i,:],
 * not its sigmoid; an empty slot is item -1 / value NaN.  The items are rfm_pair_topk's, bit for
 * bit, for the same operands.  With LU = LI = 0 and *d_c = 0 the value is the dot product of the two
 * operand rows.
 *
 * rfm_rows_normalise: d_out[r][f] = d_M[r * ld_in + f] / ||row r||_2 for f < n_factors, +0.0 for
 * n_factors <= f < kpad, d_norm[r] = the norm; ld_in >= n_factors (MF's P, Q: n_factors; side sums:
 * kpad), else RFM_ERR_BAD_ARG, as is d_out == d_M.  The arithmetic is fixed; every step is one IEEE
 * operation in round-to-nearest, nothing is contracted into an fma:
 *   - one wavefront per row; lane l of 64 starts from +0.0 and adds x_f * x_f for f = l, l + 64,
 *     l + 128, ... < n_factors in ascending order, the product rounded, then the sum;
 *   - the 64 sums t_0 .. t_63 go through the xor tree of the side sums: for m = 32, 16, 8, 4, 2, 1
 *     every lane takes t_l := t_l + t_(l xor m); after the last step all lanes hold the same s;
 *   - norm = sqrt(s), correctly rounded;
 *   - d_out[r][f] = x_f / norm, a division, never a product with a reciprocal.
 * A row whose norm is zero, NaN or infinite -- an empty FM side row, squares that underflow to
 * zero or overflow; nothing is rescaled against that -- gets NaN in every f < n_factors (its
 * padding stays zero, d_norm holds the norm as computed).  Through the pair entries such a row has
 * NaN logits: as a candidate it is never ranked, as a query its list is empty.  The same inputs
 * give the same bits; no LDS, no atomic. */
int32_t rfm_pair_topk_raw(rfm_ctx* ctx, const double* d_A, const double* d_LU, int64_t n_users,
                          const int32_t* d_user_ids, int64_t n_sel_users, const double* d_B,
                          const double* d_LI, int64_t n_items, int32_t n_factors, const double* d_c,
                          const int64_t* d_excl_indptr, const int32_t* d_excl_items, int32_t k,
                          void* d_workspace, int32_t* d_out_items, double* d_out_values);
int32_t rfm_rows_normalise(rfm_ctx* ctx, const double* d_M, int64_t n_rows, int32_t n_factors,
                           int64_t ld_in, double* d_out, double* d_norm);

#endif /* RFM_NEIGHBOURS_H */
