// pbh_quantile.hip -- summary.sorted(key).quantile(q)[key] of a recorded
// trace on gfx950 (pd.py:408-493; probayes_amd/pd.py PD.sorted +
// _quantile_batched), per chain and per dim, without the trace leaving the
// device.
//
// The trace is [record][dim][chain] with the chain fastest, so the series of
// one (chain, dim) is strided by d n doubles and a row of consecutive chains
// of one dim is contiguous.  A workgroup of kTile waves takes kTile
// consecutive chains of one dim:
//   load   every thread reads (chain j = tid % kTile, record tid / kTile +
//          64 i): a wave's load instruction covers 8 records x one 64-byte
//          row segment.  Each series goes to LDS as P = max(64, next power of
//          two >= T) pairs (monotone uint64 image of the key, uint16 record
//          index); positions >= T hold the sentinel (all ones, index >= T).
//   sort   wave w sorts series w by a bitonic network on (image, index):
//          ascending, ties by record index (so the order is total and the
//          padding stays behind every record), NaN keys last as np.argsort
//          puts them, -0.0 with +0.0.  Up to three stages of a merge run in
//          registers per pass over the series (sort_pass).  Only this wave
//          touches the series, so the passes are separated by a fence, not
//          a workgroup barrier.
//   scan   the weights in sorted order -- 1.0, or the recorded v.prob
//          rescaled to linear as trace_expect_kernel does -- gathered by the
//          sorted indices 64 at a time; an inclusive wave scan plus the
//          running carry gives cumsum(p), written over the key images (the
//          values are read back from the trace through the sorted indices).
//          Unit weights give exact integers in any association.
//   divide cumprob = cum / max(tiny, cum[T-1]), elementwise, in place.
//   count  per quantile #{cumprob <= q} by wave ballots over the divided
//          values (the host's own comparison), kept in lane j for q[j].
//   answer lane j < nq evaluates _quantile_batched's arithmetic for q[j] in
//          fp64 (this unit is built without contraction) and stores
//          out[j][dim][chain].
// No atomics; the result is a pure function of the trace.
//
// LDS: kTile P (8 + 2) bytes, dynamic: 160 KiB at P = 2 048 (one workgroup
// of 8 waves per CU), 80 KiB at P = 1 024 (two), ...  kTile = 8 is the widest
// tile the 2 048-record limit admits, and it makes the row segments 64 bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pbh_device.h"   // key_image
#include "pbh_kernels.h"

namespace pbh {
namespace {

constexpr int kTile = 8;                 // chains (= waves) per workgroup
constexpr int kThreads = 64 * kTile;
constexpr int kMaxP = 2048;              // PBH_QUANTILE_MAX_RECORDS
constexpr double kTiny = 2.2250738585072014e-308;     // NEARLY_POSITIVE_ZERO
constexpr double kNpi = 1.7976931348623158e+308;      // NEARLY_POSITIVE_INF

// LDS traffic of one wave between two dependent phases: the wave's DS
// operations complete in order; the fence keeps the compiler from moving
// them across and waits for the outstanding ones.
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

// pscales.rescale(prob, pscale, 'lin') of one recorded prob
__device__ __forceinline__ double lin_prob(double l, int32_t lin, double log_npi) {
  return lin ? l : (l <= log_npi ? exp(l) : kNpi);
}

// np.interp(x, [c0, c1], [v0, v1]) as pd.py's _interp2 writes it out
__device__ __forceinline__ double interp2(double x, double c0, double c1, double v0,
                                          double v1) {
  const double slope = (v1 - v0) / (c1 - c0);
  double mid = slope * (x - c0) + v0;
  const double alt = slope * (x - c1) + v1;
  if (mid != mid) mid = (alt != alt && v0 == v1) ? v0 : alt;
  double out = x == c0 ? v0 : mid;
  out = x >= c1 ? v1 : out;
  return x < c0 ? v0 : out;
}

// R consecutive stages (strides j2, j2 / 2, .. j2 >> (R - 1)) of the bitonic
// merge of size k2 on series (K, I) of P elements: the 2^R elements that
// these stages connect are loaded once, exchanged in registers and stored
// once (2^R independent LDS reads in flight per lane instead of one
// dependent read-compare-write per stage).  All of them lie in one k2 block,
// so they share the direction.
template <int R>
__device__ __forceinline__ void sort_pass(uint64_t *K, uint16_t *I, int P, int k2, int j2,
                                          int lane) {
  constexpr int E = 1 << R;
  const int jl = j2 >> (R - 1);   // the smallest stride
  for (int g = lane; g < (P >> R); g += 64) {
    const int base = ((g & ~(jl - 1)) << R) | (g & (jl - 1));
    const bool up = (base & k2) == 0;
    uint64_t k[E];
    uint32_t ix[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
      k[e] = K[base + e * jl];
      ix[e] = I[base + e * jl];
    }
#pragma unroll
    for (int s = R - 1; s >= 0; --s) {
#pragma unroll
      for (int e = 0; e < E; ++e) {
        if (e & (1 << s)) continue;
        const int f = e | (1 << s);
        const bool gt = k[e] > k[f] || (k[e] == k[f] && ix[e] > ix[f]);
        const bool sw = gt == up;
        const uint64_t ke = sw ? k[f] : k[e], kf = sw ? k[e] : k[f];
        const uint32_t ie = sw ? ix[f] : ix[e], jf = sw ? ix[e] : ix[f];
        k[e] = ke; k[f] = kf;
        ix[e] = ie; ix[f] = jf;
      }
    }
#pragma unroll
    for (int e = 0; e < E; ++e) {
      K[base + e * jl] = k[e];
      I[base + e * jl] = (uint16_t)ix[e];
    }
  }
}

__global__ __launch_bounds__(kThreads) void trace_quantile_kernel(
    const double *__restrict__ tx, const double *__restrict__ tlp, int64_t n, int32_t d,
    int64_t first, int32_t T, int32_t P, int32_t nq, const double *__restrict__ qv,
    int32_t weighted, int32_t lin, double log_npi, double *__restrict__ out) {
  extern __shared__ __align__(16) unsigned char s_mem[];
  uint64_t *s_key = reinterpret_cast<uint64_t *>(s_mem);                 // [kTile][P]
  uint16_t *s_idx = reinterpret_cast<uint16_t *>(s_mem + (size_t)kTile * P * 8);
  const int tid = threadIdx.x;
  const int64_t c0 = (int64_t)blockIdx.x * kTile;
  const int k = blockIdx.y;
  const int64_t stride = (int64_t)d * n;
  {
    const int j = tid % kTile;
    const bool live = c0 + j < n;
    const double *col = tx + (first * d + k) * n + c0 + j;
    for (int r = tid / kTile; r < P; r += kThreads / kTile) {
      uint64_t key = ~0ull;
      if (live && r < T) key = key_image(col[r * stride]);
      s_key[j * P + r] = key;
      s_idx[j * P + r] = (uint16_t)r;
    }
  }
  __syncthreads();
  const int w = tid >> 6, lane = tid & 63;
  const int64_t c = c0 + w;
  if (c >= n) return;
  uint64_t *K = s_key + w * P;
  uint16_t *I = s_idx + w * P;
  double *C = reinterpret_cast<double *>(K);

  // the merge of size k2 has log2(k2) stages (strides k2/2 .. 1): up to three
  // at a time in registers
  for (int k2 = 2, m = 1; k2 <= P; k2 <<= 1, ++m) {
    for (int left = m; left > 0;) {
      const int j2 = 1 << (left - 1);
      if (left >= 3) {
        sort_pass<3>(K, I, P, k2, j2, lane);
        left -= 3;
      } else if (left == 2) {
        sort_pass<2>(K, I, P, k2, j2, lane);
        left = 0;
      } else {
        sort_pass<1>(K, I, P, k2, j2, lane);
        left = 0;
      }
      wave_sync();
    }
  }

  const double *xs = tx + (first * d + k) * n + c;
  const double *ls = tlp + first * n + c;
  // cum = cumsum(p) in sorted order, over the key images
  double carry = 0.;
  for (int b = 0; b < P; b += 64) {
    const int i = b + lane;
    double p = 0.;
    // (sorted positions < T hold records < T; the clamp only keeps a read
    // inside the trace whatever else goes wrong)
    if (i < T)
      p = weighted ? lin_prob(ls[(int64_t)min((int)I[i], T - 1) * n], lin, log_npi) : 1.0;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const double up = __shfl_up(p, o);
      if (lane >= o) p = up + p;
    }
    const double cum = carry + p;
    carry = __shfl(cum, 63);
    C[i] = cum;
  }
  wave_sync();
  const double total = C[T - 1];
  wave_sync();
  const double den = total != total ? total : (total > kTiny ? total : kTiny);
  for (int i = lane; i < T; i += 64) C[i] = C[i] / den;
  wave_sync();

  int32_t mine = 0;
  for (int j = 0; j < nq; ++j) {
    const double q = qv[j];
    int32_t cnt = 0;
    for (int b = 0; b < T; b += 64) {
      const int i = b + lane;
      cnt += __popcll(__ballot(i < T && C[i] <= q));
    }
    if (lane == j) mine = cnt;
  }
  if (lane < nq) {
    const double q = qv[lane];
    const int i0 = mine > 0 ? mine - 1 : 0;
    const int r0 = min((int)I[i0], T - 1);
    const double v0 = xs[r0 * stride];
    double res = v0;
    if (i0 != T - 1) {
      const int r1 = min((int)I[i0 + 1], T - 1);
      const double v1 = xs[r1 * stride];
      const double p0 = weighted ? lin_prob(ls[(int64_t)r0 * n], lin, log_npi) : 1.0;
      const double p1 = weighted ? lin_prob(ls[(int64_t)r1 * n], lin, log_npi) : 1.0;
      const double m = (1. - q) < q ? 1. - q : q;
      if (fabs(p1 - p0) < m)
        res = interp2(q, C[i0], C[i0 + 1], v0, v1);
      else
        res = (p0 * v0 + p1 * v1) / (p0 + p1);
    }
    out[((int64_t)lane * d + k) * n + c] = res;
  }
}

}  // namespace

hipError_t launch_trace_quantile(const double *tx, const double *tlp, int64_t n,
                                 int32_t d, int64_t first, int32_t count, int32_t nq,
                                 const double *q, int32_t weighted, int32_t lin,
                                 double log_npi, double *out, hipStream_t s) {
  if (count < 1 || count > kMaxP || nq < 1 || nq > 64 || n < 1 || d < 1)
    return hipErrorInvalidValue;
  int32_t P = 64;
  while (P < count) P <<= 1;
  const size_t lds = (size_t)kTile * P * (sizeof(uint64_t) + sizeof(uint16_t));
  hipError_t err = hipFuncSetAttribute(
      reinterpret_cast<const void *>(trace_quantile_kernel),
      hipFuncAttributeMaxDynamicSharedMemorySize, kTile * kMaxP * 10);
  if (err != hipSuccess) return err;
  const dim3 grid((unsigned)((n + kTile - 1) / kTile), (unsigned)d);
  hipLaunchKernelGGL(trace_quantile_kernel, grid, dim3(kThreads), lds, s, tx, tlp, n, d,
                     first, count, P, nq, q, weighted, lin, log_npi, out);
  return hipGetLastError();
}

}  // namespace pbh
