// pbh_rhat.hip -- cross-chain convergence of a recorded trace on gfx950:
// split-R-hat (Gelman et al., BDA3; Vehtari et al. 2021 without rank
// normalisation) and nested R-hat (Margossian et al. 2024), per dim, without
// the trace leaving the device.  probayes_amd/diag.py is the host definition.
//
// Both statistics need nothing of a chain but the mean and the variance of its
// first half, its second half and the whole window, so the work is two stages:
//
//   per chain   rhat_chain_kernel, the only pass over the trace ([record][dim]
//               [chain], the chain fastest).  Thread (k, c) walks its column as
//               trace_stats_kernel does: a wave reads 512 contiguous bytes per
//               record.  Sums of x - K and of (x - K)^2 in record order, K the
//               window's first record: sums of raw squares cancel when the
//               mean is large against the spread, the shifted ones do not, and
//               the shift costs no traffic.  mean = K + S / n, var = (Q - S S /
//               n) / (n - 1).  A chain that stays at K gives S = Q = 0 and
//               variance 0 exactly.  Eight records are loaded before any is
//               used, so eight loads per lane are in flight; K is loaded and
//               waited for before the loops (record 0 contributes x - K = 0 and
//               is not read again), so no load issued ahead of a loop is
//               pending inside it.  stats[6][d][n]: mean, variance of the first
//               half, of the second half, of the window.
//   cross chain over the small stats arrays, two passes each (the mean first,
//               then the squared deviations from it; never sum m^2 - (sum m)^2
//               / n), every element assigned to a fixed thread and the partial
//               sums combined by a fixed tree in LDS (pbh_reduce_impl.h): no
//               atomics, the same bits every call.
//               rhat_group_thread_kernel / rhat_group_block_kernel reduce each
//               superchain of `group` consecutive chains to (mu_k, B_k + W_k):
//               a thread per superchain up to kThreadGroup chains, a workgroup
//               per superchain above (256 threads, 1 024 beyond kGroupWide
//               chains), so neither 65 536 superchains of one chain nor two
//               of 32 768 run on one lane.
//               rhat_final_kernel, one workgroup per (dim, statistic): the
//               variance (ddof 1) of the L means and the mean of the L
//               variances, then sqrt(((h - 1) / h W + V) / W) over the 2 n half
//               chains or sqrt(1 + V / W) over the superchains.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pbh_kernels.h"
#include "pbh_reduce_impl.h"

namespace pbh {
namespace {

constexpr int kUnroll = 8;          // records in flight per lane
constexpr int kThreadGroup = 32;    // superchains of at most this many chains: one thread each
constexpr int kGroupT = 256;        // workgroup of a superchain of up to kGroupWide chains,
constexpr int kGroupWide = 2048;    // kFinalT threads above
constexpr int kFinalT = 1024;       // workgroup of the final reduction

// Adds records p[0], p[stride], ... (nrec of them) shifted by K to (s, q) and
// to the window's (sw, qw), in record order.
__device__ __forceinline__ void accumulate(const double *__restrict__ p, int64_t stride,
                                           int64_t nrec, double K, double &s, double &q,
                                           double &sw, double &qw) {
  int64_t r = 0;
  for (; r + kUnroll <= nrec; r += kUnroll, p += kUnroll * stride) {
    double x[kUnroll];
#pragma unroll
    for (int j = 0; j < kUnroll; ++j) x[j] = p[j * stride];
#pragma unroll
    for (int j = 0; j < kUnroll; ++j) {
      const double v = x[j] - K, v2 = v * v;
      s += v;
      q += v2;
      sw += v;
      qw += v2;
    }
  }
  for (; r < nrec; ++r, p += stride) {
    const double v = *p - K, v2 = v * v;
    s += v;
    q += v2;
    sw += v;
    qw += v2;
  }
}

__device__ __forceinline__ double shifted_var(double s, double q, double n) {
  return (q - s * s / n) / (n - 1.);
}

__global__ __launch_bounds__(256) void rhat_chain_kernel(const double *__restrict__ tx,
                                                         int64_t n, int32_t d, int64_t first,
                                                         int64_t count,
                                                         double *__restrict__ stats) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t k = i / n, c = i - k * n;
  if (k >= d) return;
  const int64_t stride = (int64_t)d * n, h = count / 2;
  const double *p = tx + (first * d + k) * n + c;
  const double K = *p;
  // x - K of record 0: +0, or NaN when K is not finite -- as the sums want it
  const double v0 = K - K;
  double s1 = v0, q1 = v0 * v0, sw = s1, qw = q1, s2 = 0., q2 = 0.;
  accumulate(p + stride, stride, h - 1, K, s1, q1, sw, qw);   // (count >= 2: h >= 1)
  if (count - 2 * h == 1) {   // the middle record of an odd count: the window's only
    const double v = p[h * stride] - K;
    sw += v;
    qw += v * v;
  }
  accumulate(p + (count - h) * stride, stride, h, K, s2, q2, sw, qw);
  const double nh = (double)h, nw = (double)count;
  const int64_t row = (int64_t)d * n, at = k * n + c;
  stats[0 * row + at] = K + s1 / nh;
  stats[1 * row + at] = shifted_var(s1, q1, nh);
  stats[2 * row + at] = K + s2 / nh;
  stats[3 * row + at] = shifted_var(s2, q2, nh);
  stats[4 * row + at] = K + sw / nw;
  stats[5 * row + at] = shifted_var(sw, qw, nw);
}

// Superchains of m <= kThreadGroup chains: thread (k, g) reduces superchain g
// of dim k.  mean / var: the window's rows of stats, [d][n]; mu, bw: [d][K].
__global__ __launch_bounds__(256) void rhat_group_thread_kernel(
    const double *__restrict__ mean, const double *__restrict__ var, int64_t n, int32_t d,
    int64_t m, double *__restrict__ mu, double *__restrict__ bw) {
  const int64_t K = n / m;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t k = i / K, g = i - k * K;
  if (k >= d) return;
  const double *pm = mean + k * n + g * m, *pv = var + k * n + g * m;
  double sm = 0., sv = 0.;
  for (int64_t c = 0; c < m; ++c) {
    sm += pm[c];
    sv += pv[c];
  }
  const double mk = sm / (double)m;
  double dev = 0.;
  for (int64_t c = 0; c < m; ++c) {
    const double e = pm[c] - mk;
    dev += e * e;
  }
  const double b = m > 1 ? dev / (double)(m - 1) : 0.;
  mu[k * K + g] = mk;
  bw[k * K + g] = b + sv / (double)m;
}

// Larger superchains: workgroup (g, k) of T threads reduces superchain g of
// dim k; thread t takes the chains t, t + T, ... of it.
template <int T>
__global__ __launch_bounds__(T) void rhat_group_block_kernel(
    const double *__restrict__ mean, const double *__restrict__ var, int64_t n, int64_t m,
    double *__restrict__ mu, double *__restrict__ bw) {
  __shared__ double part[T];
  const int64_t K = n / m, g = blockIdx.x, k = blockIdx.y;
  const double *pm = mean + k * n + g * m, *pv = var + k * n + g * m;
  const auto same = [](double v) { return v; };
  const double sm = strided_sum<T>(m, [&](int64_t c) { return pm[c]; }, same);
  const double sv = strided_sum<T>(m, [&](int64_t c) { return pv[c]; }, same);
  const double mk = tree_sum<T>(part, sm) / (double)m;
  const double wk = tree_sum<T>(part, sv) / (double)m;
  const double dev = strided_sum<T>(m, [&](int64_t c) { return pm[c]; }, [&](double v) {
    const double e = v - mk;
    return e * e;
  });
  const double b = tree_sum<T>(part, dev) / (double)(m - 1);   // (m > kThreadGroup)
  if (threadIdx.x == 0) {
    mu[k * K + g] = mk;
    bw[k * K + g] = b + wk;
  }
}

// One statistic's final reduction: L = segs * len values each of means and of
// variances per dim, element j < len at m0 / v0 [k * pitch + j], the others at
// m1 / v1 [k * pitch + j - len].
struct RhatFinal {
  const double *m0, *m1, *v0, *v1;
  int64_t len, pitch;
  int32_t segs;
  int32_t nested;    // sqrt(1 + V / W), else sqrt((scale W + V) / W)
  double scale;      // (h - 1) / h
  double *out;       // [d]
};

__global__ __launch_bounds__(kFinalT) void rhat_final_kernel(RhatFinal a, RhatFinal b) {
  __shared__ double part[kFinalT];
  const RhatFinal &f = blockIdx.y == 0 ? a : b;
  const int64_t k = blockIdx.x, len = f.len, L = f.segs * len;
  const double *m0 = f.m0 + k * f.pitch, *v0 = f.v0 + k * f.pitch;
  const double *m1 = f.m1 + k * f.pitch, *v1 = f.v1 + k * f.pitch;
  const auto same = [](double v) { return v; };
  const auto mean_at = [&](int64_t j) { return j < len ? m0[j] : m1[j - len]; };
  const double sm = strided_sum<kFinalT>(L, mean_at, same);
  const double sv = strided_sum<kFinalT>(
      L, [&](int64_t j) { return j < len ? v0[j] : v1[j - len]; }, same);
  const double mbar = tree_sum<kFinalT>(part, sm) / (double)L;
  const double W = tree_sum<kFinalT>(part, sv) / (double)L;
  const double dev = strided_sum<kFinalT>(L, mean_at, [&](double v) {
    const double e = v - mbar;
    return e * e;
  });
  const double V = tree_sum<kFinalT>(part, dev) / (double)(L - 1);
  if (threadIdx.x == 0)
    f.out[k] = f.nested ? sqrt(1. + V / W) : sqrt((f.scale * W + V) / W);
}

}  // namespace

hipError_t launch_rhat_chain(const double *tx, int64_t n, int32_t d, int64_t first,
                             int64_t count, double *stats, hipStream_t s) {
  const int64_t m = (int64_t)d * n;
  hipLaunchKernelGGL(rhat_chain_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s,
                     tx, n, d, first, count, stats);
  return hipGetLastError();
}

hipError_t launch_rhat_cross(const double *stats, int64_t n, int32_t d, int64_t count,
                             int64_t group, double *sc, double *split_out,
                             double *nested_out, hipStream_t s) {
  const int64_t row = (int64_t)d * n, h = count / 2;
  RhatFinal f[2];
  int nf = 0;
  if (split_out) {
    f[nf++] = RhatFinal{stats, stats + 2 * row, stats + row, stats + 3 * row, n, n, 2, 0,
                        (double)(h - 1) / (double)h, split_out};
  }
  if (nested_out) {
    const int64_t K = n / group;
    double *mu = sc, *bw = sc + (int64_t)d * K;
    const double *mean = stats + 4 * row, *var = stats + 5 * row;
    if (group <= kThreadGroup) {
      const int64_t t = (int64_t)d * K;
      hipLaunchKernelGGL(rhat_group_thread_kernel, dim3((unsigned)((t + 255) / 256)),
                         dim3(256), 0, s, mean, var, n, d, group, mu, bw);
    } else if (group <= kGroupWide) {
      hipLaunchKernelGGL(rhat_group_block_kernel<kGroupT>, dim3((unsigned)K, (unsigned)d),
                         dim3(kGroupT), 0, s, mean, var, n, group, mu, bw);
    } else {
      hipLaunchKernelGGL(rhat_group_block_kernel<kFinalT>, dim3((unsigned)K, (unsigned)d),
                         dim3(kFinalT), 0, s, mean, var, n, group, mu, bw);
    }
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    f[nf++] = RhatFinal{mu, mu, bw, bw, K, K, 1, 1, 0., nested_out};
  }
  if (nf == 0) return hipSuccess;
  hipLaunchKernelGGL(rhat_final_kernel, dim3((unsigned)d, (unsigned)nf), dim3(kFinalT), 0, s,
                     f[0], f[nf - 1]);
  return hipGetLastError();
}

}  // namespace pbh
