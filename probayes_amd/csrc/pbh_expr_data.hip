// pbh_expr_data.hip -- PBH_TARGET_EXPR with loop regions: mh_kernel<D, RNG, kTargetExprData,
// 0> for d = 1..16 and the four RNG modes and pbh_eval_expr_data's kernel; a unit of
// its own because each of the two takes minutes to compile.
#include "pbh_expr_impl.h"

namespace pbh {

hipError_t launch_mh_expr_data(const KArgs &a, hipStream_t s) {
  return launch_mh_expr_form<true>(a, s);
}
hipError_t launch_eval_expr_data(const KArgs &a, int64_t n, const double *x, double *out) {
  return launch_eval_expr_form<true>(a, n, x, out);
}

}  // namespace pbh
