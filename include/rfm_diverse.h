/* Diversified re-ranking of catalogue candidates: a part of the C ABI of librfm_hip.so.  Included by
 * rfm_hip.h (inside its extern "C"), which declares rfm_ctx and the rfm_pair_* entries whose outputs
 * these take; do not include it alone.  It stands in a file of its own because
 * tests/test_host_abi.py pins rfm_hip.h and _lib.SIGNATURES at a fixed count of entries.  Bound from
 * _lib.DIVERSE_SIGNATURES (tests/test_diverse_host.py compares the two, argument by argument). */
#ifndef RFM_DIVERSE_H
#define RFM_DIVERSE_H

/* ---- greedy MMR selection among a list's candidates ----------
 * rfm_pair_order leaves every user's `depth` most relevant items and their scores in device
 * memory; rfm_rows_normalise gives the item rows whose dot products are cosines.  This entry chooses
 * k of a list's candidates one after the other by Maximal Marginal Relevance: each pick trades its
 * relevance against its similarity to what the list already holds, less an optional per-item
 * penalty.  The reference has no counterpart (it measures coverage, utils/metrics.py:110-166, and
 * changes it by training alone).
 *
 * rfm_diverse_select: one launch on the context's stream, no workspace, no host wait.
 *   d_cand_items  int32 [n_lists][ld_c], d_cand_scores f64 [n_lists][ld_c]: the first `depth`
 *                 (1..1024) entries of a row are the list's candidates p_c, ld_c >= depth;
 *   d_R           f64 [n_items][ld_R]: the item rows, n_factors (1..RFM_MAX_FACTORS) <= ld_R;
 *   d_penalty     f64 [n_items] or null;  trade_off = lambda in [0, 1];  k in 1..64;
 *   d_out_items   int32 [n_lists][k], d_out_scores f64 [n_lists][k] (the candidate's score, its
 *                 bytes as given), d_out_values f64 [n_lists][k] (the MMR value at the step it was
 *                 chosen), d_out_pos int32 [n_lists][k] (its position in the candidate list).
 * An argument out of range is RFM_ERR_BAD_ARG before any launch; n_lists == 0 launches nothing.
 *
 * THE ARITHMETIC IS FIXED.  Every step is one IEEE operation in round-to-nearest, nothing is
 * contracted into an fma:
 *   - sim(c, j), the dot product of the rows R[item_c], R[item_j] over f < n_factors: lane l of 64
 *     starts from +0.0 and adds x_f * y_f for f = l, l + 64, l + 128, ... < n_factors in ascending
 *     order, the product rounded, then the sum; the 64 sums t_0 .. t_63 go through the xor tree of
 *     rfm_rows_normalise: for m = 32, 16, 8, 4, 2, 1 every lane takes t_l := t_l + t_(l xor m).
 *     A NaN similarity counts as +0.0 (a row without a direction: an FM item without entries, an
 *     Inf * 0);
 *   - m_c, the maximum over the items chosen so far of sim(c, j): it starts from -inf and every
 *     pick j updates it by m_c := s > m_c ? s : m_c;
 *   - base_c = lambda * p_c, then base_c := base_c - penalty[item_c] where a penalty is given;
 *   - step 0 takes v_c = base_c; step t >= 1 takes v_c = base_c - (1 - lambda) * m_c, with
 *     1 - lambda one double subtraction, the product rounded, then the difference.
 * A candidate is ELIGIBLE at a step when it is not yet chosen, its item id lies in 0 .. n_items-1,
 * its score is not NaN and v_c is not NaN.  The step takes the best eligible candidate under the
 * total order of the rfm_pair_* entries: value descending, then item id descending; among repeats
 * of one id the lower position goes first.  With no eligible candidate left the rest of the row is
 * item -1, score NaN, value NaN, pos -1.  The same inputs give the same bits; no atomic.
 *
 * THE KERNEL.  One workgroup of 256 threads per list, the lists strided over a capped grid.  base,
 * m and the item id of every candidate sit in LDS (an id of -1 once chosen or never eligible), the
 * chosen row is staged in LDS, and each of the four wavefronts takes every fourth candidate of a
 * step, four at a time: it reads the candidate's row once per step.  The step's argmax goes
 * through lane exchanges inside a wavefront and through LDS across the four.  There is one form.
 *
 * rfm_diverse_geometry (host only, nothing is launched): h_out6[0]=form (0: the streaming form
 * above, the only one), [1]=workgroups, [2]=passes over the grid (lists of the busiest workgroup),
 * [3]=candidates per thread of the value pass, [4]=LDS bytes of a workgroup, [5]=trips of a lane's
 * factor loop, ceil(n_factors / 64).  ctx == NULL: the grid on a device of 256 CUs (an MI355X). */
int32_t rfm_diverse_select(rfm_ctx* ctx, const int32_t* d_cand_items, const double* d_cand_scores,
                           int64_t n_lists, int32_t depth, int64_t ld_c, const double* d_R, int64_t n_items,
                           int32_t n_factors, int64_t ld_R, const double* d_penalty, double trade_off,
                           int32_t k, int32_t* d_out_items, double* d_out_scores, double* d_out_values,
                           int32_t* d_out_pos);
int32_t rfm_diverse_geometry(const rfm_ctx* ctx, int64_t n_lists, int32_t depth, int32_t n_factors,
                             int64_t ld_R, int32_t k, int64_t* h_out6);

#endif /* RFM_DIVERSE_H */
