/* The update rule of an FM plan's steps: a part of the C ABI of librfm_hip.so.  Included by
 * rfm_hip.h, which declares rfm_fm_plan and the step entry points this extends; do not include it
 * alone.  Bound from _lib.FM_OPT_SIGNATURES (tests/test_adagrad_host.py compares the two, argument
 * by argument). */
#ifndef RFM_FM_OPT_H
#define RFM_FM_OPT_H

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

#endif /* RFM_FM_OPT_H */
