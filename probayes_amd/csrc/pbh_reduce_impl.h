// pbh_reduce_impl.h -- the two fixed-order sums the cross-chain reductions
// share (pbh_rhat.hip: the final reduction and the wide superchains;
// pbh_cov.hip: the shift and the finish): a thread's strided share of a sum
// with kBatch loads in flight, and the workgroup's tree in LDS.  No atomics:
// the same bits every call.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pbh {
namespace {

constexpr int kBatch = 16;          // loads in flight per thread of the cross-chain sums

// Sums part[0..T) into part[0] by a fixed tree; every thread of the workgroup
// calls it, and all read the total.
template <int T>
__device__ __forceinline__ double tree_sum(double *part, double mine) {
  __syncthreads();   // the previous total has been read
  part[threadIdx.x] = mine;
  __syncthreads();
#pragma unroll
  for (int w = T / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
    __syncthreads();
  }
  return part[0];
}

// Thread t's share of sum_j term(load(j)) over j = t, t + T, ... < L, added in
// that order.  kBatch values are loaded before any is used -- the loads are
// independent, so they are in flight together (a thread of the final
// reduction has 128 elements at 65 536 chains: one load per round trip made
// that kernel 0.11 ms).  A batch that reaches past L loads element L - 1
// again and adds +0 in its place.
template <int T, class Load, class Term>
__device__ __forceinline__ double strided_sum(int64_t L, Load load, Term term) {
  double acc = 0.;
  for (int64_t j = threadIdx.x; j < L; j += (int64_t)kBatch * T) {
    double x[kBatch];
#pragma unroll
    for (int i = 0; i < kBatch; ++i) {
      const int64_t at = j + (int64_t)i * T;
      x[i] = load(at < L ? at : L - 1);
    }
#pragma unroll
    for (int i = 0; i < kBatch; ++i) acc += j + (int64_t)i * T < L ? term(x[i]) : 0.;
  }
  return acc;
}

}  // namespace
}  // namespace pbh
