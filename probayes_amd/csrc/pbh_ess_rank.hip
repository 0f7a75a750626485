// pbh_ess_rank.hip -- the autocovariance of a recorded series averaged over
// its split chains, on gfx950: what the bulk- and the tail-ESS across chains
// (Vehtari et al. 2021) are estimated from, without the trace leaving the
// device.  probayes_amd/diag.py split_chain_acov is the host definition; the
// estimator itself (multi_chain_ess) is O(h) and runs on the host
// (pbh_trace_host.cpp).
//
// One dim and one variant at a time.  The series is [record][chain], the chain
// fastest, `stride` doubles between records: the trace at a dim, or the normal
// scores of a dim as a one-dim trace.  The C = 2 n split chains are the first
// h = count / 2 records of every chain and the last h.  The biased
// autocovariance of a split chain is linear in its power spectrum, so the
// spectra are summed over the split chains and ONE inverse transform gives
// the sum of their autocovariance sums:
//
//   spectrum  ess_spectrum_kernel.  The ceil(n / 2) chain pairs of the dim are
//             cut into `groups` runs of `run` consecutive pairs, a workgroup
//             each.  Per pair and half: chains 2 p and 2 p + 1 are the real and
//             the imaginary part (adjacent doubles of every record: one
//             16-byte load per lane where the address allows, and the pairs of
//             a run, one after the other, read the same cache lines; the last
//             chain of an odd n stands alone), each element through the
//             variant's transform (identity, or x <= thr as 0. / 1.), each part
//             centred by its first record plus the mean of its differences
//             from it (fp64, a fixed order: per thread ascending, then
//             block_sum's tree; a constant chain is centred to exact zeros),
//             zero-padded to 4 096 points and transformed (pbh_fft_impl.h).
//             Nothing is unpacked: |Z_k|^2 is added to 16 per-thread
//             accumulators, the only registers alive across the loop, and the
//             real part of the inverse transform of sum |Z_k|^2 is the sum of
//             the two parts' autocovariance sums.  The workgroup writes its
//             4 096 sums to a row of its own: no floating-point atomics.
//             With means wanted (the indicator variants) the two means go to
//             mean_first / mean_second [n].
//   finish    ess_finish_kernel, one workgroup: the partial rows added in
//             ascending workgroup order, the inverse transform, A[t] = Re /
//             (4 096 h C) for t < h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pbh_kernels.h"
#include "pbh_trace_host.h"   // EssLayout, kEssPoints

namespace pbh {
namespace {

#include "pbh_fft_impl.h"

static_assert(kFftN == kEssPoints, "a partial row is one transform");

struct EssSeries {
  const double *base;   // record 0 of the window, chain 0
  int64_t n, stride;    // chains; doubles between records
  int64_t h, second;    // records of a half; the second half's first record
  const double *thr;    // null: the values; else *thr is the indicator's threshold
};

__device__ __forceinline__ double ess_element(double x, bool ind, double thr) {
  // (a NaN threshold: the dim holds a NaN, and so does every element)
  return !ind ? x : thr != thr ? thr : x <= thr ? 1. : 0.;
}

// grid (groups).  part [groups][kFftN]; mean_first, mean_second [n] or null.
__global__ __launch_bounds__(kFftT) __attribute__((amdgpu_waves_per_eu(2, 2)))
void ess_spectrum_kernel(EssSeries a, int64_t pairs, int64_t run, double *__restrict__ part,
                         double *__restrict__ mean_first, double *__restrict__ mean_second) {
  __shared__ double sb[kFftN + kFftN / 16];
  __shared__ double red[8];
  const int j = (int)threadIdx.x;
  const bool ind = a.thr != nullptr;
  const double thr = ind ? *a.thr : 0.;
  const int h = (int)a.h;
  const FftTw tw = fft_twiddles();
  double acc[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.;
  const int64_t p0 = (int64_t)blockIdx.x * run;
  const int64_t p1 = p0 + run < pairs ? p0 + run : pairs;
  // (one pair and half per iteration, not unrolled: only acc stays live)
#pragma nounroll
  for (int64_t it = 2 * p0; it < 2 * p1; ++it) {
    const int64_t c0 = it & ~(int64_t)1;   // chain 2 p
    const bool half = it & 1;
    const bool has_b = c0 + 1 < a.n;
    const double *src = a.base + (half ? a.second * a.stride : 0) + c0;
    // chains c0, c0 + 1 of a record: one 16-byte load when every record's
    // address is 16-byte aligned
    const bool wide = has_b && !(a.stride & 1) && (reinterpret_cast<uintptr_t>(src) & 15) == 0;
    const double k0 = ess_element(src[0], ind, thr);
    const double k1 = has_b ? ess_element(src[1], ind, thr) : 0.;
    // ---- load (t = j + 256 q, q < 8: h <= 2048) shifted by the first record ----
    cdbl v[16];
    double sa = 0., sc = 0.;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int t = j + q * kFftT;
      double xa = k0, xb = k1;
      if (t < h) {
        const double *p = src + (int64_t)t * a.stride;
        if (wide) {
          const double2 x = *reinterpret_cast<const double2 *>(p);
          xa = ess_element(x.x, ind, thr);
          xb = ess_element(x.y, ind, thr);
        } else {
          xa = ess_element(p[0], ind, thr);
          if (has_b) xb = ess_element(p[1], ind, thr);
        }
      }
      // (past the half: k - k, +0 or the NaN of a non-finite first record)
      v[q] = cdbl{xa - k0, xb - k1};
      sa += v[q].re;
      sc += v[q].im;
    }
    const double ma = block_sum(sa, red) / (double)h;
    const double mb = block_sum(sc, red + 4) / (double)h;
    if (j == 0 && mean_first) {
      double *m = half ? mean_second : mean_first;
      m[c0] = k0 + ma;
      if (has_b) m[c0 + 1] = k1 + mb;
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const bool in = q < 8 && j + q * kFftT < h;
      v[q] = in ? cdbl{v[q].re - ma, v[q].im - mb} : cdbl{0., 0.};
    }
    // ---- forward transform (points 2048 .. 4095 zero).  The twiddle bases
    // are made opaque per iteration: their powers are loop-invariant, and
    // hoisted out of the loop the two passes' 30 complex powers stayed live
    // across it (spilled VGPRs) ----
    cdbl w16 = tw.w16, w256 = tw.w256;
    asm volatile("" : "+v"(w16.re), "+v"(w16.im), "+v"(w256.re), "+v"(w256.im));
    fft_compute<-1, 1, true>(v, cdbl{1., 0.});
    fft_exchange<1>(sb, v);
    fft_compute<-1, 16>(v, w16);
    fft_exchange<16>(sb, v);
    fft_compute<-1, 256>(v, w256);
    // ---- v[i] = Z at bin fft_out<256>(i) ----
#pragma unroll
    for (int i = 0; i < 16; ++i)
      acc[i] += __builtin_fma(v[i].re, v[i].re, v[i].im * v[i].im);
  }
  double *row = part + (int64_t)blockIdx.x * kFftN;
#pragma unroll
  for (int i = 0; i < 16; ++i) row[fft_out<256>(i)] = acc[i];
}

// One workgroup.  acov [h].
__global__ __launch_bounds__(kFftT) void ess_finish_kernel(const double *__restrict__ part,
                                                           int64_t groups, int64_t h,
                                                           double scale,
                                                           double *__restrict__ acov) {
  __shared__ double sb[kFftN + kFftN / 16];
  const int j = (int)threadIdx.x;
  const FftTw tw = fft_twiddles();
  cdbl v[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) v[r] = cdbl{0., 0.};
  // the first pass's points x[j + 256 r]: the rows in ascending order
  for (int64_t g = 0; g < groups; ++g) {
    const double *row = part + g * kFftN + j;
    double x[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) x[r] = row[r * kFftT];
#pragma unroll
    for (int r = 0; r < 16; ++r) v[r].re += x[r];
  }
  fft_compute<1, 1>(v, cdbl{1., 0.});
  fft_exchange<1>(sb, v);
  fft_compute<1, 16>(v, conj(tw.w16));
  fft_exchange<16>(sb, v);
  fft_compute<1, 256>(v, conj(tw.w256));
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int lag = fft_out<256>(i);
    if (lag < h) acov[lag] = v[i].re / scale;
  }
}

}  // namespace

hipError_t launch_ess_spectrum(const double *base, int64_t n, int64_t stride, int64_t count,
                               const double *thr, const EssLayout &l, double *part,
                               double *mean_first, double *mean_second, hipStream_t s) {
  if (n < 1 || stride < n || count < 4 || l.h != count / 2 || l.h > kFftN / 2 ||
      l.pairs != n / 2 + n % 2 || l.run < 1 || l.groups < 1 || l.groups > kEssMaxGroups ||
      l.groups * l.run < l.pairs || (l.groups - 1) * l.run >= l.pairs ||
      (mean_first == nullptr) != (mean_second == nullptr))
    return hipErrorInvalidValue;
  const EssSeries a{base, n, stride, l.h, count - l.h, thr};
  hipLaunchKernelGGL(ess_spectrum_kernel, dim3((unsigned)l.groups), dim3(kFftT), 0, s, a, l.pairs,
                     l.run, part, mean_first, mean_second);
  return hipGetLastError();
}

hipError_t launch_ess_finish(const double *part, int64_t n, const EssLayout &l, double *acov,
                             hipStream_t s) {
  if (n < 1 || l.h < 2 || l.h > kFftN / 2 || l.groups < 1 || l.groups > kEssMaxGroups)
    return hipErrorInvalidValue;
  const double scale = (double)kFftN * (double)l.h * (double)(2 * n);
  hipLaunchKernelGGL(ess_finish_kernel, dim3(1), dim3(kFftT), 0, s, part, l.groups, l.h, scale,
                     acov);
  return hipGetLastError();
}

}  // namespace pbh
