// pbh_expr.hip -- PBH_TARGET_EXPR without loop regions: mh_kernel<D, RNG, PBH_TARGET_EXPR, 0>
// for d = 1..16 and the four RNG modes, pbh_eval_expr's kernel, the exported launchers.
#include "pbh_expr_impl.h"

namespace pbh {

hipError_t launch_mh_expr(const KArgs &a, hipStream_t s) {
  return a.edata ? launch_mh_expr_data(a, s) : launch_mh_expr_form<false>(a, s);
}
hipError_t launch_eval_expr(const KArgs &a, int64_t n, const double *x, double *out) {
  return a.edata ? launch_eval_expr_data(a, n, x, out)
                 : launch_eval_expr_form<false>(a, n, x, out);
}

}  // namespace pbh
