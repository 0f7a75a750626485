// pbh_expr.hip -- the kernels of PBH_TARGET_EXPR: mh_kernel<D, RNG,
// PBH_TARGET_EXPR, 0> for d = 1..16 and the four RNG modes (the general MH
// kernel with every proposal form, whose density is the interpreter
// expr_density), and pbh_eval_expr's kernel.
#include "pbh_kernels_impl.h"

namespace pbh {

namespace {

// pbh_eval_expr: the program at n points x [d][n] (a.d variables)
__global__ __launch_bounds__(kBlock) void expr_eval_kernel(KArgs a, int64_t n, const double *xs,
                                                           double *out) {
  const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t cc = c < n ? c : 0;
  double x[PBH_EXPR_MAX_DIM];
#pragma unroll
  for (int k = 0; k < PBH_EXPR_MAX_DIM; ++k) x[k] = k < a.d ? xs[k * n + cc] : 0.;
  const double v = expr_density<PBH_EXPR_MAX_DIM>(a, x);
  if (c < n) out[c] = v;
}

}  // namespace

hipError_t launch_mh_expr(const KArgs &a, hipStream_t s) {
  switch (a.d) {
#define PBH_CASE(D)                                  \
  case D:                                            \
    launch_mh_spec<D, PBH_TARGET_EXPR, 0>(a, s, 0);  \
    return hipGetLastError();
    PBH_CASE(1) PBH_CASE(2) PBH_CASE(3) PBH_CASE(4) PBH_CASE(5) PBH_CASE(6)
    PBH_CASE(7) PBH_CASE(8) PBH_CASE(9) PBH_CASE(10) PBH_CASE(11) PBH_CASE(12)
    PBH_CASE(13) PBH_CASE(14) PBH_CASE(15) PBH_CASE(16)
#undef PBH_CASE
    default:
      return hipErrorInvalidValue;
  }
}

hipError_t launch_eval_expr(const KArgs &a, int64_t n, const double *x, double *out) {
  const dim3 grid((unsigned)((n + kBlock - 1) / kBlock)), block(kBlock);
  hipLaunchKernelGGL(expr_eval_kernel, grid, block, 0, 0, a, n, x, out);
  hipError_t err = hipGetLastError();
  if (err == hipSuccess) err = hipDeviceSynchronize();
  return err;
}

}  // namespace pbh
