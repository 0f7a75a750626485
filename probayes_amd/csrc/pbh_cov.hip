// pbh_cov.hip -- the posterior covariance of a recorded trace on gfx950, pooled
// over every chain and record of a window, without the trace leaving the
// device.  probayes_amd/diag.py pooled_cov is the host definition;
// pbh_trace_host.h has the layout and the last step (cov_finish).
//
// With v = x - K: S_a = sum v_a and P_ab = sum v_a v_b (a <= b) over the
// window, then mean = K + S / M and cov_ab = (P_ab - S_a S_b / M) / (M - 1) on
// the host.  Sums of raw products cancel when the mean is large against the
// spread; the shifted ones do not as long as K lies among the draws, and the
// mean over chains of the window's first record does by construction.  Three
// stages on the engine's stream, no atomics, every order fixed -- two calls
// give the same bits:
//
//   cov_shift_kernel    K [d], a workgroup per dim: the strided sum and the
//                       LDS tree of pbh_reduce_impl.h over the first record.
//   cov_partial_kernel  the only pass over the trace ([record][dim][chain],
//                       the chain fastest).  A workgroup owns 256 consecutive
//                       chains, one tile job and one slice of consecutive
//                       records; a lane owns one chain and keeps its sums in
//                       registers: every accumulator index is a compile-time
//                       constant, nothing is a runtime-indexed private array.
//                       Up to 16 dims the job is the whole triangle (WA = d, 16
//                       + 136 doubles at d = 16); above, blockIdx.y runs over
//                       the two diagonal tiles of 16 dims (the kernel of d = 16)
//                       and the 8 x 8 rectangles between them (64 doubles; with
//                       16 x 8 the compiler no longer issued a record's loads
//                       together and the pass ran at a sixth of the bandwidth).
//                       A tile that reaches past d reads dim d - 1 in the
//                       missing dims' place and its results are not stored: no
//                       branch per element.  A lane walks its records as
//                       rhat_chain_kernel does: kUnroll records' loads issued
//                       before the first is used; K is read through scalar loads
//                       and used (K - K, the sums' start) before the loop, so
//                       nothing issued ahead of the loop is pending inside it.
//                       The products are accumulated with an explicit fused
//                       multiply-add -- the definition is met by tolerance, not
//                       bit for bit, and without it the instruction count per
//                       record doubles.  The lanes' sums are combined in LDS, 16
//                       accumulators at a time: 16 threads per accumulator add
//                       16 lanes each in lane order, then one thread adds the 16
//                       results in order.  One partial row per (chain block,
//                       slice): part [row][d + d (d + 1) / 2].
//   cov_finish_kernel   a workgroup per column: the rows in index order by the
//                       same strided sum and tree -> res [cols].  Every slice of
//                       every chain block used the same K, so the rows add.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pbh_kernels.h"
#include "pbh_reduce_impl.h"
#include "pbh_trace_host.h"

namespace pbh {
namespace {

constexpr int kShiftT = 1024;    // workgroup of the shift
constexpr int kFinishT = 256;    // workgroup of a column of the finish
constexpr int kChunk = 16;       // accumulators combined per round in LDS
constexpr int kFoldLanes = kCovLanes / kChunk;   // lanes a thread adds in a round

static_assert(kCovLanes == kChunk * kFoldLanes && kFoldLanes == 16, "the combine's shape");

struct CovArgs {
  const double *tx;                  // the trace [record][d][n]
  int64_t n, first, count, slice_len, slices, cols;
  int32_t d;
  const double *K;                   // [d]
  double *part;                      // [rows][cols]
};

__global__ __launch_bounds__(kShiftT) void cov_shift_kernel(const double *__restrict__ tx,
                                                            int64_t n, int32_t d, int64_t first,
                                                            double *__restrict__ K) {
  __shared__ double part[kShiftT];
  const int64_t k = blockIdx.x;
  const double *p = tx + (first * d + k) * n;
  const double s = strided_sum<kShiftT>(
      n, [&](int64_t c) { return p[c]; }, [](double v) { return v; });
  const double total = tree_sum<kShiftT>(part, s);
  if (threadIdx.x == 0) K[k] = total / (double)n;
}

// The sums of a tile job.  WB == 0: the diagonal tile of WA dims from a0, S
// [WA] then the triangle row by row.  WB > 0: the rectangle of the WA dims
// from a0 by the WB dims from b0 >= a0 + WA.
template <int WA, int WB>
struct CovTile {
  static constexpr int kDims = WA + WB;
  static constexpr int kAcc = WB == 0 ? WA + WA * (WA + 1) / 2 : WA * WB;
  // records in flight per lane: about 48 doubles of loads, 2 .. 8 records
  static constexpr int kUnroll = 48 / kDims < 2 ? 2 : 48 / kDims > 8 ? 8 : 48 / kDims;
  static constexpr int tri(int i, int j) { return WA + i * WA - i * (i - 1) / 2 + (j - i); }

  static __device__ __forceinline__ void fold(const double (&v)[kDims], double (&acc)[kAcc]) {
    if constexpr (WB == 0) {
#pragma unroll
      for (int i = 0; i < WA; ++i) acc[i] += v[i];
#pragma unroll
      for (int i = 0; i < WA; ++i)
#pragma unroll
        for (int j = i; j < WA; ++j) acc[tri(i, j)] = __builtin_fma(v[i], v[j], acc[tri(i, j)]);
    } else {
#pragma unroll
      for (int i = 0; i < WA; ++i)
#pragma unroll
        for (int j = 0; j < WB; ++j)
          acc[i * WB + j] = __builtin_fma(v[i], v[WA + j], acc[i * WB + j]);
    }
  }

  // The column of accumulator `at` in a partial row, or -1 where the tile
  // reaches past d.
  static __device__ __forceinline__ int64_t column(int at, int a0, int b0, int d) {
    if constexpr (WB == 0) {
      if (at < WA) return a0 + at < d ? a0 + at : -1;
      int i = 0, rem = at - WA;
      while (rem >= WA - i) {
        rem -= WA - i;
        ++i;
      }
      const int a = a0 + i, b = a + rem;
      return b < d ? d + cov_tri(a, b, d) : -1;
    } else {
      const int a = a0 + at / WB, b = b0 + at % WB;
      return a < d && b < d ? d + cov_tri(a, b, d) : -1;
    }
  }
};

template <int WA, int WB>
__global__ __launch_bounds__(kCovLanes) void cov_partial_kernel(CovArgs p) {
  using Tile = CovTile<WA, WB>;
  constexpr int kDims = Tile::kDims, kAcc = Tile::kAcc, kUnroll = Tile::kUnroll;
  __shared__ double s_lane[kChunk * kCovLanes];
  __shared__ double s_fold[kChunk * kFoldLanes];
  const int d = p.d;
  // blockIdx.y: the diagonal tile, or the rectangle -- its rows' place in the
  // first tile, the fastest, and its columns' behind it
  constexpr int kRowTiles = kCovTile / WA;
  const int a0 = WB == 0 ? (int)blockIdx.y * kCovTile : ((int)blockIdx.y % kRowTiles) * WA;
  const int b0 = WB == 0 ? 0 : kCovTile + ((int)blockIdx.y / kRowTiles) * WB;
  const int64_t c = (int64_t)blockIdx.x * kCovLanes + threadIdx.x;
  const bool live = c < p.n;
  const int64_t cc = live ? c : p.n - 1;
  const int64_t r0 = (int64_t)blockIdx.z * p.slice_len;
  const int64_t r1 = r0 + p.slice_len < p.count ? r0 + p.slice_len : p.count;

  int64_t off[kDims];   // wave-uniform: where the tile's dims lie in a record
  double K[kDims];
#pragma unroll
  for (int i = 0; i < kDims; ++i) {
    const int k = (i < WA ? a0 + i : b0 + i - WA);
    const int kk = k < d ? k : d - 1;
    off[i] = (int64_t)kk * p.n;
    K[i] = p.K[kk];
  }
  double acc[kAcc];
  if constexpr (WB == 0) {
    // x - K of no record: +0, or NaN when K is not finite -- as the sums want it
#pragma unroll
    for (int i = 0; i < WA; ++i) acc[i] = K[i] - K[i];
#pragma unroll
    for (int i = 0; i < WA; ++i)
#pragma unroll
      for (int j = i; j < WA; ++j) acc[Tile::tri(i, j)] = acc[i] * acc[j];
  } else {
    double z[kDims];
#pragma unroll
    for (int i = 0; i < kDims; ++i) z[i] = K[i] - K[i];
#pragma unroll
    for (int i = 0; i < WA; ++i)
#pragma unroll
      for (int j = 0; j < WB; ++j) acc[i * WB + j] = z[i] * z[WA + j];
  }

  const int64_t stride = (int64_t)d * p.n;
  const double *q = p.tx + (p.first + r0) * stride + cc;
  int64_t r = r0;
  for (; r + kUnroll <= r1; r += kUnroll, q += kUnroll * stride) {
    double x[kUnroll][kDims];
#pragma unroll
    for (int j = 0; j < kUnroll; ++j)
#pragma unroll
      for (int i = 0; i < kDims; ++i) x[j][i] = q[j * stride + off[i]];
#pragma unroll
    for (int j = 0; j < kUnroll; ++j) {
      double v[kDims];
#pragma unroll
      for (int i = 0; i < kDims; ++i) v[i] = x[j][i] - K[i];
      Tile::fold(v, acc);
    }
  }
  for (; r < r1; ++r, q += stride) {
    double v[kDims];
#pragma unroll
    for (int i = 0; i < kDims; ++i) v[i] = q[off[i]] - K[i];
    Tile::fold(v, acc);
  }

  // the lanes' sums in a fixed order: per round of kChunk accumulators, thread
  // (a, l) adds lanes l, l + 16, .. of accumulator a, then thread a the 16
  // results
  double *row = p.part + ((int64_t)blockIdx.x * p.slices + blockIdx.z) * p.cols;
  const int fa = threadIdx.x / kFoldLanes, fl = threadIdx.x % kFoldLanes;
#pragma unroll
  for (int c0 = 0; c0 < kAcc; c0 += kChunk) {
    __syncthreads();   // the previous round has been read
#pragma unroll
    for (int i = 0; i < kChunk; ++i)
      s_lane[i * kCovLanes + threadIdx.x] = c0 + i < kAcc && live ? acc[c0 + i < kAcc ? c0 + i : 0] : 0.;
    __syncthreads();
    double s = s_lane[fa * kCovLanes + fl];
#pragma unroll
    for (int j = 1; j < kFoldLanes; ++j) s += s_lane[fa * kCovLanes + fl + j * kFoldLanes];
    s_fold[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x < kChunk && c0 + (int)threadIdx.x < kAcc) {
      double t = s_fold[threadIdx.x * kFoldLanes];
#pragma unroll
      for (int j = 1; j < kFoldLanes; ++j) t += s_fold[threadIdx.x * kFoldLanes + j];
      const int64_t col = Tile::column(c0 + (int)threadIdx.x, a0, b0, d);
      if (col >= 0) row[col] = t;
    }
  }
}

__global__ __launch_bounds__(kFinishT) void cov_finish_kernel(const double *__restrict__ part,
                                                              int64_t rows, int64_t cols,
                                                              double *__restrict__ res) {
  __shared__ double tree[kFinishT];
  const int64_t col = blockIdx.x;
  const double s = strided_sum<kFinishT>(
      rows, [&](int64_t r) { return part[r * cols + col]; }, [](double v) { return v; });
  const double total = tree_sum<kFinishT>(tree, s);
  if (threadIdx.x == 0) res[col] = total;
}

template <int WA, int WB>
void launch_partial(const CovArgs &a, int64_t chain_blocks, int tiles, hipStream_t s) {
  hipLaunchKernelGGL((cov_partial_kernel<WA, WB>),
                     dim3((unsigned)chain_blocks, (unsigned)tiles, (unsigned)a.slices),
                     dim3(kCovLanes), 0, s, a);
}

}  // namespace

hipError_t launch_cov(const double *tx, int64_t n, int32_t d, int64_t first, int64_t count,
                      unsigned char *scratch, const CovLayout &l, hipStream_t s) {
  double *K = reinterpret_cast<double *>(scratch + l.K);
  double *part = reinterpret_cast<double *>(scratch + l.part);
  double *res = reinterpret_cast<double *>(scratch + l.res);
  hipLaunchKernelGGL(cov_shift_kernel, dim3((unsigned)d), dim3(kShiftT), 0, s, tx, n, d, first, K);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return err;
  const CovArgs a{tx, n, first, count, l.slice_len, l.slices, l.cols, d, K, part};
  switch (d <= kCovTile ? d : 0) {
#define PBH_COV_D(D) case D: launch_partial<D, 0>(a, l.chain_blocks, 1, s); break;
    PBH_COV_D(1) PBH_COV_D(2) PBH_COV_D(3) PBH_COV_D(4) PBH_COV_D(5) PBH_COV_D(6)
    PBH_COV_D(7) PBH_COV_D(8) PBH_COV_D(9) PBH_COV_D(10) PBH_COV_D(11) PBH_COV_D(12)
    PBH_COV_D(13) PBH_COV_D(14) PBH_COV_D(15) PBH_COV_D(16)
#undef PBH_COV_D
    default:
      launch_partial<kCovTile, 0>(a, l.chain_blocks, 2, s);
      err = hipGetLastError();
      if (err != hipSuccess) return err;
      launch_partial<kCovHalf, kCovHalf>(a, l.chain_blocks, (int)l.pairs - 2, s);
  }
  err = hipGetLastError();
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(cov_finish_kernel, dim3((unsigned)l.cols), dim3(kFinishT), 0, s, part,
                     l.rows, l.cols, res);
  return hipGetLastError();
}

}  // namespace pbh
