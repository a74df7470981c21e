// The update rule of a fused step, as the FM gradient launch (rfm_fm_kernels.hpp) and the record
// form's MF kernels (rfm_mf.hip) take it: a type parameter O of the kernel, the rule's operands
// behind the kernel's argument block, and the one check of what a caller may ask for.
#pragma once

#include <type_traits>

#include "rfm_common.h"

namespace rfm {

// SgdRule: theta -= lr * g as each update site spells it, the text the sites had before there was
// a choice; its instantiations are that code and their argument block is the plain one.  A rule
// with kAda (AdaGradRule of the FM side, MfAdaGradRule: their accumulator fields differ) gives
// every element an accumulator G of its own (same shape, float64) and, with g the element's
// gradient,
//   G_new = G + g * g             (the product rounded, then the sum)
//   theta_new = theta - (lr * g) / (sqrt(G_new) + eps)
// in IEEE basic operations.
struct SgdRule {
  static constexpr bool kAda = false;
};

// one element under an AdaGrad rule; *G: its accumulator as it was read, then as it is to be written
__device__ inline double adagrad_element(double theta, double g, double lr, double eps, double* G) {
#pragma clang fp contract(off)
  const double gg = g * g;
  const double gn = *G + gg;
  *G = gn;
  return theta - (lr * g) / (sqrt(gn) + eps);
}

// the argument block of a kernel under a rule: SgdRule's is Args itself
template <class Args, class O>
struct WithRule : Args {
  O o;
};
template <class Args, class O>
using ArgsUnder = std::conditional_t<O::kAda, WithRule<Args, O>, Args>;

template <class Args>
__device__ inline SgdRule rule_of(const Args&) {
  return SgdRule{};
}
template <class Args, class O>
__device__ inline const O& rule_of(const WithRule<Args, O>& a) {
  return a.o;
}

// host: the block a launch under rule o passes
template <class Args, class O>
inline ArgsUnder<Args, O> args_under(const Args& a, const O& o) {
  ArgsUnder<Args, O> out{};
  static_cast<Args&>(out) = a;
  if constexpr (O::kAda) out.o = o;
  return out;
}

// host: what rfm_fm_plan_set_optimizer and rfm_mf_sgd_levels_opt accept, in this order; true for
// AdaGrad.  accs: every accumulator of the rule is there.
inline bool require_rule(int32_t kind, bool accs, double eps) {
  RFM_REQUIRE(kind == RFM_FM_OPT_SGD || kind == RFM_FM_OPT_ADAGRAD,
              "optimizer kind %d is neither SGD nor AdaGrad", kind);
  if (kind == RFM_FM_OPT_SGD) return false;
  RFM_REQUIRE(accs, "AdaGrad with a null accumulator");
  RFM_REQUIRE(eps > 0.0, "AdaGrad eps=%g must be > 0", eps);  // (false for a NaN)
  return true;
}

}  // namespace rfm
