/* The item -> users direction of the catalogue entries: a part of the C ABI of librfm_hip.so.
 * Included by rfm_hip.h (inside its extern "C"), which declares rfm_ctx and the rfm_pair_* entries
 * that these are the twins of; do not include it alone.  It stands in a file of its own because
 * tests/test_host_abi.py pins rfm_hip.h and _lib.SIGNATURES at a fixed count of entries.  Bound from
 * _lib.AUDIENCE_SIGNATURES (tests/test_audience_host.py compares the two, argument by argument). */
#ifndef RFM_AUDIENCE_H
#define RFM_AUDIENCE_H

/* ---- for this item, which users? ------------------------------
 * rfm_pair_topk, rfm_pair_ranks_n and rfm_pair_order answer "for this user, which items?".  The
 * three entries below answer the opposite question with the same kernels in a second compile-time
 * form: the rows of the tile (the queries) are items, its columns (the candidates) users.  The
 * reference has no counterpart of either direction beyond predict() (src/fm.py:114-133,
 * src/mf.py:136-170).
 *
 * THE SAME BYTES.  The logit of (item i, user u) is
 *     ((*d_c + LU[u]) + LI[i]) + A[u,:].B[i,:],
 * the user's side term first, exactly as the forward entries form the logit of (u, i); the factors
 * are taken in the same order and every product commutes.  So one pair has one logit, bit for bit,
 * through rfm_pair_scores, _topk, _topk_raw, _ranks, _order and the three entries here.  Calling a
 * forward entry with the two tables exchanged does NOT give that: it adds LI[i] first, which rounds
 * differently for about a third of all pairs.
 *
 * ARGUMENTS.  Each entry takes the argument list of its forward twin, and the operand arguments
 * keep their meaning: d_A, d_LU, n_users are the user side, d_B, d_LI, n_items the item side.  What
 * changes sides:
 *   - d_item_ids [n_sel_items] (null: every item, and then n_sel_items == n_items) select the
 *     QUERIES, in any order, repeats allowed; an id outside 0 .. n_items-1 gives NaN logits and an
 *     empty list (RFM_CHECK_IDS=1: RFM_ERR_BAD_ARG);
 *   - d_excl_indptr [n_items + 1], d_excl_users: PER ITEM lists of user ids, strictly ascending,
 *     the users never to return for that item (both null: none).  They are the transpose of the
 *     lists the forward entries take;
 *   - the outputs hold USER ids.  n_users must fit int32 ids as n_items must in the twins.
 * The order is the twins' total order on the candidate: logit descending, then USER index
 * descending.  A NaN logit is never ranked.  No float atomic is used and every sum has a fixed
 * order: the same inputs give the same bits.  Argument checks and RFM_CHECK_IDS behave as in the
 * twins (whose messages name the rows of the tile "users" and its columns "items").
 *
 * GEOMETRY AND WORKSPACES.  The launches are those of the twins for the exchanged counts, so no
 * query of its own is needed: rfm_pair_geometry(n_sel_items, n_users, n_factors) and
 * rfm_pair_order_geometry(n_users, depth) report them, and the workspaces are sized by
 * rfm_pair_topk_workspace(n_sel_items, n_users, k), rfm_pair_ranks_workspace(n_sel_items, n_users,
 * n_targets) and rfm_pair_order_workspace(n_sel_items, n_users, depth).
 *
 * rfm_pair_topk_by_item: twin of rfm_pair_topk.  d_out_users [n_sel_items][k], d_out_values the
 * sigmoid of the logit, or with raw != 0 the logit itself as rfm_pair_topk_raw returns it; fewer
 * than k rankable users pads with user -1 / value NaN.
 *
 * rfm_pair_ranks_by_item: twin of rfm_pair_ranks_n (the host gives n_targets, nothing is read back,
 * nothing synchronises unless RFM_CHECK_IDS=1).  The targets of selected item s are the users
 * d_tgt_users[d_tgt_indptr[s] .. d_tgt_indptr[s+1]), ascending; d_out_ranks[t] = the number of the
 * item's candidates (users with a logit that is not NaN and that the item's list does not name)
 * that are better than target t, -1 for a NaN logit; d_out_scores[t] = sigmoid(logit);
 * d_out_candidates[s] = the item's candidate count.  A target that its item's list names is
 * treated as rfm_pair_ranks treats an excluded target: it is no candidate, and its rank counts the
 * candidates in front of it.
 *
 * rfm_pair_order_by_item: twin of rfm_pair_order.  d_out_users, d_out_scores [n_sel_items][depth],
 * d_out_n_ranked [n_sel_items]: each item's ranking of the users down to depth, any depth >= 1. */
int32_t rfm_pair_topk_by_item(rfm_ctx* ctx, const double* d_A, const double* d_LU, int64_t n_users,
                              const int32_t* d_item_ids, int64_t n_sel_items, const double* d_B,
                              const double* d_LI, int64_t n_items, int32_t n_factors, const double* d_c,
                              const int64_t* d_excl_indptr, const int32_t* d_excl_users, int32_t k,
                              int32_t raw, void* d_workspace, int32_t* d_out_users, double* d_out_values);
int32_t rfm_pair_ranks_by_item(rfm_ctx* ctx, const double* d_A, const double* d_LU, int64_t n_users,
                               const int32_t* d_item_ids, int64_t n_sel_items, const double* d_B,
                               const double* d_LI, int64_t n_items, int32_t n_factors, const double* d_c,
                               const int64_t* d_excl_indptr, const int32_t* d_excl_users,
                               const int64_t* d_tgt_indptr, const int32_t* d_tgt_users, int64_t n_targets,
                               void* d_workspace, int32_t* d_out_ranks, double* d_out_scores,
                               int32_t* d_out_candidates);
int32_t rfm_pair_order_by_item(rfm_ctx* ctx, const double* d_A, const double* d_LU, int64_t n_users,
                               const int32_t* d_item_ids, int64_t n_sel_items, const double* d_B,
                               const double* d_LI, int64_t n_items, int32_t n_factors, const double* d_c,
                               const int64_t* d_excl_indptr, const int32_t* d_excl_users, int64_t depth,
                               void* d_workspace, int64_t workspace_bytes, int32_t* d_out_users,
                               double* d_out_scores, int32_t* d_out_n_ranked);

#endif /* RFM_AUDIENCE_H */
