/* The update rule of the exact MF batch step: a part of the C ABI of librfm_hip.so.  Included by
 * rfm_hip.h, which declares rfm_ctx and rfm_mf_sgd_levels_ex that this extends; do not include it
 * alone.  Bound from _lib.MF_OPT_SIGNATURES (tests/test_mf_adagrad_host.py compares the two,
 * argument by argument). */
#ifndef RFM_MF_OPT_H
#define RFM_MF_OPT_H

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

#endif /* RFM_MF_OPT_H */
