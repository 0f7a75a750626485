// pbh_hist.hip -- the posterior histograms of a recorded trace on gfx950, pooled
// over every chain and record of a window, without the trace leaving the
// device: per dim the counts in the bins of the caller's edges (np.histogram),
// and per pair of dims the counts in the grid of the two dims' bins
// (np.histogram2d).  probayes_amd/diag.py hist_bin, pooled_hist and
// pooled_hist2d are the host definition; pbh_hist_bin.h has the lookup, which
// the CPU tests run as it stands here; pbh_trace_host.h has the layouts.
//
// The only state is integer counts: the result does not depend on the order of
// the adds and equals NumPy's bit for bit.  No floating-point atomics.
//
//   hist_count_kernel    grid (chain blocks, dim groups, record slices).  A
//                        workgroup owns 256 consecutive chains, one dim group
//                        and one slice of consecutive records.  It stages the
//                        group's lookup tables in LDS and clears the group's
//                        uint32 counters there (per dim the bins, then below,
//                        above, NaN), then takes the group's dims one after the
//                        other: a lane owns a chain and walks the dim's records
//                        of the slice ([record][dim][chain], the chain fastest:
//                        a wave reads 512 contiguous bytes), eight records'
//                        loads issued before the first is used, as
//                        cov_partial_kernel walks.  The lookup of a dim is fixed
//                        before its walk by a wave-uniform switch: the guess, or
//                        the search at the dim's depth, a template parameter, so
//                        the loop holds straight-line code.  Per value one
//                        ds_add: the lanes of a wave on the first active lane's
//                        counter add once for them all, as select_count_kernel's
//                        add does -- a posterior that sits in a few bins and
//                        chains that never move put a whole wave on one counter.
//                        A slice is short enough that a counter cannot wrap
//                        (kHistMaxSlice).  Padding lanes of a ragged last block
//                        read the last chain and count nothing.  At the end the
//                        non-zero counters go to the global uint64 counts by
//                        64-bit atomic adds.
//   hist2d_count_kernel  grid (chain blocks, pairs, record slices).  The two
//                        dims' tables and the B_a x B_b uint32 cells sit in LDS;
//                        the cell of a draw is i_a B_b + i_b, a draw with either
//                        bin negative is dropped.  Four records' two loads in
//                        flight; the lookups go through hist_bin_any's uniform
//                        switch, whose cases are the same straight-line
//                        functions.  The add and the flush are the same.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pbh_hist_bin.h"
#include "pbh_kernels.h"
#include "pbh_trace_host.h"

namespace pbh {
namespace {

constexpr int kUnroll = 8;     // records in flight per lane, one dim
constexpr int kUnroll2 = 4;    // records in flight per lane, a pair of dims
constexpr uint32_t kNone = ~0u;

struct HistArgs {
  const double *tx;                  // the trace [record][d][n]
  int64_t n, first, count, slice_len;
  int32_t d;
  const double *tables;              // the groups' tables one after the other
  unsigned long long *counts;        // the groups' counters one after the other
  int32_t group_first[kHistMaxDims + 1];
  int32_t tab_off[kHistMaxDims], tab_len[kHistMaxDims], ctr_off[kHistMaxDims],
      ctr_len[kHistMaxDims];                                                   // per group
  int32_t dim[kHistMaxDims], bins[kHistMaxDims], mode[kHistMaxDims], tab[kHistMaxDims],
      ctr[kHistMaxDims];                                                       // per listed dim
  double e0[kHistMaxDims], eB[kHistMaxDims], s[kHistMaxDims];
};

struct Hist2dArgs {
  const double *tx;
  int64_t n, first, count, slice_len;
  int32_t d;
  const double *tables;              // the tables of the dims with edges
  const int64_t *pairs;              // [pair][4]: a, b, where its cells start, 0
  unsigned long long *counts;
  int32_t bins[kHistMaxDims], mode[kHistMaxDims], tab_off[kHistMaxDims];   // per dim
  double e0[kHistMaxDims], eB[kHistMaxDims], s[kHistMaxDims];
};

// Adds one to the LDS counter `at`.  The lanes on the first active lane's
// counter add once for all of them; the others add singly.
__device__ __forceinline__ void add_one(uint32_t *ctr, uint32_t at) {
  if (at == kNone) return;
  const uint32_t at0 = __builtin_amdgcn_readfirstlane(at);
  const uint64_t same = __ballot(at == at0);
  uint32_t by = 1u;
  if (at == at0) {
    if (__ffsll((unsigned long long)same) - 1 != (int)__lane_id()) return;
    by = (uint32_t)__popcll(same);
  }
  atomicAdd(&ctr[at], by);
}

// the counter of a bin among a dim's bins + 3: below, above and NaN behind the bins
__device__ __forceinline__ uint32_t counter_of(int32_t bin, int32_t bins) {
  return (uint32_t)(bin >= 0 ? bin : bins - 1 - bin);
}

struct DimWalk {
  const double *q;     // the lane's chain at the slice's first record of the dim
  int64_t stride, records;
  const double *t;     // the dim's table (LDS)
  uint32_t *ctr;       // the dim's counters (LDS)
  int32_t bins;
  double e0, eB, s;
  bool live;
};

template <int MODE>
__device__ __forceinline__ uint32_t lookup(const DimWalk &w, double x) {
  int32_t bin;
  if constexpr (MODE == kHistGuess)
    bin = hist_bin_guess(w.t, w.bins, w.e0, w.eB, w.s, x);
  else
    bin = hist_bin_search<MODE>(w.t, w.e0, w.eB, x);
  return w.live ? counter_of(bin, w.bins) : kNone;
}

template <int MODE>
__device__ __forceinline__ void walk_dim(const DimWalk &w) {
  const double *q = w.q;
  int64_t r = 0;
  for (; r + kUnroll <= w.records; r += kUnroll, q += kUnroll * w.stride) {
    double x[kUnroll];
#pragma unroll
    for (int j = 0; j < kUnroll; ++j) x[j] = q[j * w.stride];
    // four lookups side by side before their adds
#pragma unroll
    for (int h = 0; h < kUnroll; h += 4) {
      uint32_t at[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) at[j] = lookup<MODE>(w, x[h + j]);
#pragma unroll
      for (int j = 0; j < 4; ++j) add_one(w.ctr, at[j]);
    }
  }
  for (; r < w.records; ++r, q += w.stride) add_one(w.ctr, lookup<MODE>(w, *q));
}

__global__ __launch_bounds__(kHistLanes) void hist_count_kernel(HistArgs p) {
  extern __shared__ __align__(16) unsigned char s_mem[];
  const int g = blockIdx.y, tid = threadIdx.x;
  const int32_t tab_len = p.tab_len[g], ctr_len = p.ctr_len[g];
  double *s_tab = reinterpret_cast<double *>(s_mem);
  uint32_t *s_ctr = reinterpret_cast<uint32_t *>(s_mem + (size_t)tab_len * 8);
  const double *tab = p.tables + p.tab_off[g];
  for (int i = tid; i < tab_len; i += kHistLanes) s_tab[i] = tab[i];
  for (int i = tid; i < ctr_len; i += kHistLanes) s_ctr[i] = 0u;
  __syncthreads();

  const int64_t c = (int64_t)blockIdx.x * kHistLanes + tid;
  const bool live = c < p.n;
  const int64_t cc = live ? c : p.n - 1;
  const int64_t r0 = (int64_t)blockIdx.z * p.slice_len;
  const int64_t r1 = r0 + p.slice_len < p.count ? r0 + p.slice_len : p.count;
  const int64_t stride = (int64_t)p.d * p.n;

  for (int j = p.group_first[g]; j < p.group_first[g + 1]; ++j) {
    DimWalk w;
    w.q = p.tx + ((p.first + r0) * p.d + p.dim[j]) * p.n + cc;
    w.stride = stride;
    w.records = r1 > r0 ? r1 - r0 : 0;
    w.t = s_tab + p.tab[j];
    w.ctr = s_ctr + p.ctr[j];
    w.bins = p.bins[j];
    w.e0 = p.e0[j];
    w.eB = p.eB[j];
    w.s = p.s[j];
    w.live = live;
    switch (p.mode[j]) {
#define PBH_HIST_DEPTH(D) case D: walk_dim<D>(w); break;
      PBH_HIST_DEPTH(0) PBH_HIST_DEPTH(1) PBH_HIST_DEPTH(2) PBH_HIST_DEPTH(3) PBH_HIST_DEPTH(4)
      PBH_HIST_DEPTH(5) PBH_HIST_DEPTH(6) PBH_HIST_DEPTH(7) PBH_HIST_DEPTH(8) PBH_HIST_DEPTH(9)
      PBH_HIST_DEPTH(10) PBH_HIST_DEPTH(11) PBH_HIST_DEPTH(12)
#undef PBH_HIST_DEPTH
      default: walk_dim<kHistGuess>(w);
    }
  }

  __syncthreads();
  unsigned long long *out = p.counts + p.ctr_off[g];
  for (int i = tid; i < ctr_len; i += kHistLanes) {
    const uint32_t v = s_ctr[i];
    if (v) atomicAdd(&out[i], (unsigned long long)v);
  }
}

__global__ __launch_bounds__(kHistLanes) void hist2d_count_kernel(Hist2dArgs p) {
  extern __shared__ __align__(16) unsigned char s_mem[];
  const int tid = threadIdx.x;
  const int64_t *pair = p.pairs + (int64_t)blockIdx.y * 4;
  const int a = (int)pair[0], b = (int)pair[1];
  const int32_t Ba = p.bins[a], Bb = p.bins[b], cells = Ba * Bb;
  const int32_t len_a = (int32_t)hist_table_len(Ba), len_b = (int32_t)hist_table_len(Bb);
  double *s_ta = reinterpret_cast<double *>(s_mem), *s_tb = s_ta + len_a;
  uint32_t *s_ctr = reinterpret_cast<uint32_t *>(s_tb + len_b);
  const double *ta = p.tables + p.tab_off[a], *tb = p.tables + p.tab_off[b];
  for (int i = tid; i < len_a; i += kHistLanes) s_ta[i] = ta[i];
  for (int i = tid; i < len_b; i += kHistLanes) s_tb[i] = tb[i];
  for (int i = tid; i < cells; i += kHistLanes) s_ctr[i] = 0u;
  __syncthreads();

  const int64_t c = (int64_t)blockIdx.x * kHistLanes + tid;
  const bool live = c < p.n;
  const int64_t cc = live ? c : p.n - 1;
  const int64_t r0 = (int64_t)blockIdx.z * p.slice_len;
  const int64_t r1 = r0 + p.slice_len < p.count ? r0 + p.slice_len : p.count;
  const int64_t stride = (int64_t)p.d * p.n;
  const int mode_a = p.mode[a], mode_b = p.mode[b];
  const double a0 = p.e0[a], aB = p.eB[a], as = p.s[a];
  const double b0 = p.e0[b], bB = p.eB[b], bs = p.s[b];
  const auto cell = [&](double xa, double xb) {
    const int32_t ia = hist_bin_any(mode_a, s_ta, Ba, a0, aB, as, xa);
    const int32_t ib = hist_bin_any(mode_b, s_tb, Bb, b0, bB, bs, xb);
    return live && ia >= 0 && ib >= 0 ? (uint32_t)(ia * Bb + ib) : kNone;
  };

  const double *qa = p.tx + ((p.first + r0) * p.d + a) * p.n + cc;
  const double *qb = p.tx + ((p.first + r0) * p.d + b) * p.n + cc;
  int64_t r = r0;
  for (; r + kUnroll2 <= r1; r += kUnroll2, qa += kUnroll2 * stride, qb += kUnroll2 * stride) {
    double xa[kUnroll2], xb[kUnroll2];
#pragma unroll
    for (int j = 0; j < kUnroll2; ++j) {
      xa[j] = qa[j * stride];
      xb[j] = qb[j * stride];
    }
    uint32_t at[kUnroll2];
#pragma unroll
    for (int j = 0; j < kUnroll2; ++j) at[j] = cell(xa[j], xb[j]);
#pragma unroll
    for (int j = 0; j < kUnroll2; ++j) add_one(s_ctr, at[j]);
  }
  for (; r < r1; ++r, qa += stride, qb += stride) add_one(s_ctr, cell(*qa, *qb));

  __syncthreads();
  unsigned long long *out = p.counts + pair[2];
  for (int i = tid; i < cells; i += kHistLanes) {
    const uint32_t v = s_ctr[i];
    if (v) atomicAdd(&out[i], (unsigned long long)v);
  }
}

// a workgroup's dynamic LDS above the 64 KiB a kernel gets unasked
template <class Kernel>
hipError_t allow_lds(Kernel kernel, int64_t bytes) {
  if (bytes <= 64 * 1024) return hipSuccess;
  return hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

}  // namespace

hipError_t launch_hist(const double *tx, int64_t n, int32_t d, int64_t first, int64_t count,
                       unsigned char *scratch, const HistLayout &l, const HistDimPlan *plan,
                       hipStream_t s) {
  HistArgs a{};
  a.tx = tx;
  a.n = n;
  a.first = first;
  a.count = count;
  a.slice_len = l.slice_len;
  a.d = d;
  a.tables = reinterpret_cast<const double *>(scratch + l.tables);
  a.counts = reinterpret_cast<unsigned long long *>(scratch + l.counts);
  for (int g = 0; g <= l.groups; ++g) a.group_first[g] = l.group_first[g];
  for (int g = 0; g < l.groups; ++g) {
    a.tab_off[g] = l.tab_off[g];
    a.tab_len[g] = l.tab_len[g];
    a.ctr_off[g] = l.ctr_off[g];
    a.ctr_len[g] = l.ctr_len[g];
  }
  for (int j = 0; j < l.dims; ++j) {
    const HistDimPlan &p = plan[l.dim[j]];
    a.dim[j] = l.dim[j];
    a.bins[j] = p.bins;
    a.mode[j] = p.mode;
    a.tab[j] = l.tab[j];
    a.ctr[j] = l.ctr[j];
    a.e0[j] = p.e0;
    a.eB[j] = p.eB;
    a.s[j] = p.s;
  }
  hipError_t err = hipMemsetAsync(a.counts, 0, (size_t)l.n_ctr * 8, s);
  if (err != hipSuccess) return err;
  err = allow_lds(hist_count_kernel, l.lds_bytes);
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(hist_count_kernel,
                     dim3((unsigned)l.chain_blocks, (unsigned)l.groups, (unsigned)l.slices),
                     dim3(kHistLanes), (size_t)l.lds_bytes, s, a);
  return hipGetLastError();
}

hipError_t launch_hist2d(const double *tx, int64_t n, int32_t d, int64_t first, int64_t count,
                         unsigned char *scratch, const Hist2dLayout &l, const HistDimPlan *plan,
                         hipStream_t s) {
  Hist2dArgs a{};
  a.tx = tx;
  a.n = n;
  a.first = first;
  a.count = count;
  a.slice_len = l.slice_len;
  a.d = d;
  a.tables = reinterpret_cast<const double *>(scratch + l.tables);
  a.pairs = reinterpret_cast<const int64_t *>(scratch + l.pairs);
  a.counts = reinterpret_cast<unsigned long long *>(scratch + l.counts);
  for (int k = 0; k < d; ++k) {
    a.bins[k] = plan[k].bins;
    a.mode[k] = plan[k].mode;
    a.tab_off[k] = l.tab_off[k];
    a.e0[k] = plan[k].e0;
    a.eB[k] = plan[k].eB;
    a.s[k] = plan[k].s;
  }
  hipError_t err = hipMemsetAsync(a.counts, 0, (size_t)l.n_ctr * 8, s);
  if (err != hipSuccess) return err;
  err = allow_lds(hist2d_count_kernel, l.lds_bytes);
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(hist2d_count_kernel,
                     dim3((unsigned)l.chain_blocks, (unsigned)l.n_pairs, (unsigned)l.slices),
                     dim3(kHistLanes), (size_t)l.lds_bytes, s, a);
  return hipGetLastError();
}

}  // namespace pbh
