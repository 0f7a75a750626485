// pbh_select.hip -- order statistics of a recorded trace pooled over chains
// and records, per dim, on gfx950: the two values each pooled quantile is
// interpolated between (probayes_amd/diag.py pooled_quantile is the host
// definition), without sorting and without the trace leaving the device.
//
// A most-significant-digit radix select over key_image, the monotone 64-bit
// image of a double.  The host names the wanted ranks, sorted and distinct
// (the targets, at most kSelectMaxTargets, the same for every dim); per (dim,
// target) the device keeps the key prefix fixed so far and the rank that
// remains among the keys under that prefix.  The digits are 11, 11, 11, 11,
// 10, 10 bits wide: six passes, each one streaming read of the window and two
// launches, with no host round trip in between.
//
//   count  select_count_kernel.  Targets are sorted by rank, so their keys
//          and prefixes ascend with the target index: the distinct prefixes
//          of a dim (its groups) are runs of consecutive targets and come
//          sorted.  Prefixes of one length are equal or disjoint, so a key
//          falls under at most one: a binary search over the groups staged in
//          LDS on the key's high bits (in the first pass the one empty prefix
//          matches every key and nothing is searched).  The search's depth is
//          a template parameter fixed by the number of targets, at most 8, so
//          that it is straight-line code; as a run-time loop it made the
//          kernel issue-bound.  A match adds one to (group, next
//          digit).
//          The first kLdsGroups groups are counted in LDS (uint32, privatised
//          per workgroup, flushed once with 64-bit global atomics, zeros
//          skipped).  That covers the dense passes: the first, where every
//          key matches, and the second, where the exponent digit of the first
//          has left whole binades under one prefix.  Groups beyond those go to
//          global memory directly.  Either way a wave whose lanes hit the
//          counter of its first active lane adds once for them all: on tied
//          data every lane is on one counter in every pass.
//          The window is walked as one index e = record * n + chain over the M
//          = count * n elements of a dim, consecutive lanes on consecutive
//          chains (a wave reads 512 contiguous bytes but where a record
//          ends), (record, chain) advanced without a division, eight loads in
//          flight per lane.
//   pick   select_pick_kernel, one workgroup per dim.  Group by group: an
//          inclusive scan of the histogram, then every target of the group
//          takes the digit at which the running count first exceeds its
//          rank, appends it to its prefix and subtracts the count below it.
//          The histogram is cleared as it is read.  Then the groups of the
//          next pass are formed from the new prefixes.  After the last pass
//          the prefix is the key, and its inverse image the order statistic.
//
// The only state is integer counts: the result does not depend on the order
// of the atomics, and equals sorting on the host bit for bit.  NaN has the
// largest image, so a dim holds a NaN exactly when its largest element is one:
// the caller makes rank M - 1 a target.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pbh_device.h"   // key_image, key_value
#include "pbh_kernels.h"

namespace pbh {
namespace {

constexpr int kT = kSelectMaxTargets;
constexpr int kBins = 2048;          // of the widest digit
constexpr int kLdsGroups = 16;       // groups counted in LDS (8 KiB each)
constexpr int kCountT = 1024;        // workgroup of the count kernel
constexpr int kPickT = 1024;         // workgroup of the pick kernel: two bins per thread
constexpr int kUnroll = 8;           // loads in flight per lane
constexpr int kMaxSteps = 8;         // of the search: 2^8 > kT
constexpr int kPasses = 6;
constexpr int kWidth[kPasses] = {11, 11, 11, 11, 10, 10};

// The engine's scratch, in 8-byte words: per (dim, target) the prefix, the
// remaining rank and the group; per (dim, group) the group's prefix; per dim
// the number of groups; the histograms [d][nt][kBins]; the order statistics
// [d][nt].
struct Layout {
  int64_t prefix, rank, group, gprefix, ngroups, hist, stats, words;
};

__host__ __device__ inline Layout layout(int32_t d, int32_t nt) {
  Layout l;
  const int64_t per = (int64_t)d * kT;
  l.prefix = 0;
  l.rank = per;
  l.group = 2 * per;
  l.gprefix = 3 * per;
  l.ngroups = 4 * per;
  l.hist = 4 * per + d;
  l.stats = l.hist + (int64_t)d * nt * kBins;
  l.words = l.stats + (int64_t)d * nt;
  return l;
}

struct Counters {
  const uint64_t *gp;   // gp[1 + g]: the dim's group prefixes, sorted (LDS); see below
  uint32_t *lds;        // [gl][kBins]
  uint64_t *hist;       // the dim's [nt][kBins]
  int32_t gl;           // groups counted in LDS
  int32_t done, shift;  // bits fixed before this pass; the digit's position
  uint32_t mask;
};

constexpr uint32_t kNone = ~0u;

// The counter of a value: group * kBins + digit, or kNone under no group's
// prefix.  STEPS < 0: the first pass, one group with the empty prefix.
// Otherwise a search of STEPS steps, fixed by the number of targets so that
// it is straight-line code and the searches of a round's elements interleave:
// gp[1 .. ng] are the prefixes, gp[ng + 1 .. 2^STEPS - 1] and gp[0] all ones,
// above every prefix of fewer than 64 bits: pos, the number of prefixes <=
// hi, needs no bound check, and gp[pos] == hi is the match (gp[0] never).
template <int STEPS>
__device__ __forceinline__ uint32_t counter_of(const Counters &c, double v) {
  const uint64_t key = key_image(v);
  const uint32_t digit = (uint32_t)(key >> c.shift) & c.mask;
  if constexpr (STEPS < 0) {
    return digit;
  } else {
    const uint64_t hi = key >> (64 - c.done);   // (done >= 11 after the first pass)
    uint32_t pos = 0;
#pragma unroll
    for (int s = STEPS - 1; s >= 0; --s) {
      const uint32_t j = pos + (1u << s);
      if (c.gp[j] <= hi) pos = j;
    }
    return c.gp[pos] == hi ? (pos - 1u) * kBins + digit : kNone;
  }
}

// Adds one to counter `at`.  The lanes on the first active lane's counter add
// once for all of them (tied data puts a whole wave on one counter); the
// others add singly.
__device__ __forceinline__ void add_one(const Counters &c, uint32_t at) {
  if (at == kNone) return;
  const uint32_t at0 = __builtin_amdgcn_readfirstlane(at);
  const uint64_t same = __ballot(at == at0);
  uint32_t by = 1u;
  if (at == at0) {
    if (__ffsll((unsigned long long)same) - 1 != (int)__lane_id()) return;
    by = (uint32_t)__popcll(same);
  }
  if (at < (uint32_t)c.gl * kBins)
    atomicAdd(&c.lds[at], by);
  else
    atomicAdd((unsigned long long *)&c.hist[at], (unsigned long long)by);
}

// grid (bx, d).  step = bx * kCountT elements between a thread's elements:
// step_rec = step / n records and step_col = step % n chains.
template <int STEPS>
__global__ __launch_bounds__(kCountT) void select_count_kernel(
    const double *__restrict__ tx, int64_t n, int32_t d, int64_t first, int64_t M,
    int64_t step_rec, int64_t step_col, uint64_t *sc, int32_t nt, int32_t glds,
    int32_t done, int32_t bits) {
  extern __shared__ __align__(16) unsigned char s_mem[];
  __shared__ uint64_t s_gp[1 << kMaxSteps];
  uint32_t *s_hist = reinterpret_cast<uint32_t *>(s_mem);
  const int k = blockIdx.y, tid = threadIdx.x;
  const Layout l = layout(d, nt);
  int32_t ng = (int32_t)sc[l.ngroups + k];
  ng = ng < 1 ? 1 : (ng > nt ? nt : ng);   // (1 <= ng <= nt <= kT whatever the scratch holds)
  const int32_t gl = ng < glds ? ng : glds;
  for (int i = tid; i < (1 << kMaxSteps); i += kCountT)
    s_gp[i] = i >= 1 && i <= ng ? sc[l.gprefix + (int64_t)k * kT + i - 1] : ~0ull;
  for (int i = tid; i < gl * kBins; i += kCountT) s_hist[i] = 0u;
  __syncthreads();

  Counters c;
  c.gp = s_gp;
  c.lds = s_hist;
  c.hist = sc + l.hist + (int64_t)k * nt * kBins;
  c.gl = gl;
  c.done = done;
  c.shift = 64 - done - bits;
  c.mask = (1u << bits) - 1u;

  const int64_t dn = (int64_t)d * n;
  const int64_t step = step_rec * n + step_col;
  const int64_t jump = step_rec * dn + step_col, wrap = dn - n;
  int64_t e = (int64_t)blockIdx.x * kCountT + tid;
  int64_t col = e % n;
  const double *p = tx + (first * d + k) * n + (e / n) * dn + col;
  // (e < M keeps p inside the window: p addresses element e of dim k)
  for (; e + (kUnroll - 1) * step < M; e += kUnroll * step) {
    double x[kUnroll];
#pragma unroll
    for (int j = 0; j < kUnroll; ++j) {
      x[j] = *p;
      col += step_col;
      p += jump;
      if (col >= n) {
        col -= n;
        p += wrap;
      }
    }
    // four searches side by side before their adds
#pragma unroll
    for (int h = 0; h < kUnroll; h += 4) {
      uint32_t at[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) at[j] = counter_of<STEPS>(c, x[h + j]);
#pragma unroll
      for (int j = 0; j < 4; ++j) add_one(c, at[j]);
    }
  }
  for (; e < M; e += step) {
    const double x = *p;
    col += step_col;
    p += jump;
    if (col >= n) {
      col -= n;
      p += wrap;
    }
    add_one(c, counter_of<STEPS>(c, x));
  }
  __syncthreads();
  for (int i = tid; i < gl * kBins; i += kCountT) {
    const uint32_t v = s_hist[i];
    if (v) atomicAdd((unsigned long long *)&c.hist[i], (unsigned long long)v);
  }
}

// Inclusive scan of two values per thread over the workgroup: returns the
// running count up to and including b.
__device__ __forceinline__ uint64_t scan_pair(uint64_t *s_wave, uint64_t a, uint64_t b) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint64_t v = a + b;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint64_t up = __shfl_up((unsigned long long)v, o);
    if (lane >= o) v += up;
  }
  __syncthreads();   // the previous totals have been read
  if (lane == 63) s_wave[w] = v;
  __syncthreads();
  uint64_t below = 0;
  for (int i = 0; i < w; ++i) below += s_wave[i];
  return below + v;
}

__global__ __launch_bounds__(kPickT) void select_pick_kernel(uint64_t *sc,
                                                             int32_t d, int32_t nt, int32_t bits,
                                                             int32_t last) {
  __shared__ uint64_t s_cum[kBins];
  __shared__ uint64_t s_wave[kPickT / 64];
  __shared__ uint64_t s_prefix[kT];
  const int k = blockIdx.x, tid = threadIdx.x;
  const Layout l = layout(d, nt);
  const int32_t bins = 1 << bits;
  int32_t ng = (int32_t)sc[l.ngroups + k];
  ng = ng < 1 ? 1 : (ng > nt ? nt : ng);
  const bool mine = tid < nt;
  const int64_t at = (int64_t)k * kT + tid;
  uint64_t prefix = 0, rank = 0;
  int32_t group = -1;
  if (mine) {
    prefix = sc[l.prefix + at];
    rank = sc[l.rank + at];
    group = (int32_t)sc[l.group + at];
  }
  uint64_t *hist = sc + l.hist + (int64_t)k * nt * kBins;
  const bool live = 2 * tid < bins;
  uint64_t a = 0, b = 0;
  if (live) {
    a = hist[2 * tid];
    b = hist[2 * tid + 1];
  }
  for (int32_t g = 0; g < ng; ++g) {
    const uint64_t a0 = a, b0 = b;
    if (live) {
      hist[(int64_t)g * kBins + 2 * tid] = 0;
      hist[(int64_t)g * kBins + 2 * tid + 1] = 0;
      if (g + 1 < ng) {   // the next group's bins, on their way during the scan
        a = hist[(int64_t)(g + 1) * kBins + 2 * tid];
        b = hist[(int64_t)(g + 1) * kBins + 2 * tid + 1];
      }
    }
    // (its barriers also separate the previous group's reads of s_cum from
    // the writes below)
    const uint64_t upto = scan_pair(s_wave, a0, b0);
    if (live) {
      s_cum[2 * tid] = upto - b0;
      s_cum[2 * tid + 1] = upto;
    }
    __syncthreads();
    if (mine && group == g) {
      // the first digit whose running count exceeds the rank (the last bin
      // if none does, which a consistent histogram rules out)
      int32_t lo = 0, hi = bins - 1;
      while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (s_cum[mid] > rank) hi = mid; else lo = mid + 1;
      }
      const uint64_t below = lo ? s_cum[lo - 1] : 0ull;
      rank = rank >= below ? rank - below : 0ull;
      prefix = (prefix << bits) | (uint64_t)lo;
    }
  }
  // the groups of the next pass: runs of equal prefixes
  if (mine) s_prefix[tid] = prefix;
  __syncthreads();
  if (mine) {
    int32_t heads = 0;
    for (int i = 1; i <= tid; ++i) heads += s_prefix[i] != s_prefix[i - 1];
    const bool head = tid == 0 || s_prefix[tid] != s_prefix[tid - 1];
    sc[l.prefix + at] = prefix;
    sc[l.rank + at] = rank;
    sc[l.group + at] = (uint64_t)heads;
    if (head) sc[l.gprefix + (int64_t)k * kT + heads] = prefix;
    if (tid == nt - 1) sc[l.ngroups + k] = (uint64_t)(heads + 1);
    if (last)
      sc[l.stats + (int64_t)k * nt + tid] = __builtin_bit_cast(uint64_t, key_value(prefix));
  }
}

}  // namespace

int64_t select_scratch_words(int32_t d, int32_t nt) { return layout(d, nt).words; }

int64_t select_stats_offset(int32_t d, int32_t nt) { return layout(d, nt).stats; }

int32_t select_passes() { return kPasses; }

hipError_t launch_select_init(uint64_t *sc, int32_t d, int32_t nt, const uint64_t *ranks,
                              uint64_t *host, hipStream_t s) {
  if (d < 1 || nt < 1 || nt > kT) return hipErrorInvalidValue;
  const Layout l = layout(d, nt);
  // every target under the one empty prefix, group 0
  for (int64_t i = 0; i < l.hist; ++i) host[i] = 0;
  for (int32_t k = 0; k < d; ++k) {
    for (int32_t t = 0; t < nt; ++t) host[l.rank + (int64_t)k * kT + t] = ranks[t];
    host[l.ngroups + k] = 1;
  }
  hipError_t err = hipMemcpyAsync(sc, host, l.hist * sizeof(uint64_t), hipMemcpyHostToDevice, s);
  if (err != hipSuccess) return err;
  return hipMemsetAsync(sc + l.hist, 0, (size_t)(l.stats - l.hist) * sizeof(uint64_t), s);
}

hipError_t launch_select_pass(const double *tx, int64_t n, int32_t d, int64_t first,
                              int64_t count, uint64_t *sc, int32_t nt, int32_t pass,
                              hipStream_t s) {
  if (n < 1 || d < 1 || count < 1 || nt < 1 || nt > kT || pass < 0 || pass >= kPasses)
    return hipErrorInvalidValue;
  int32_t done = 0;
  for (int32_t i = 0; i < pass; ++i) done += kWidth[i];
  const int32_t bits = kWidth[pass];
  const int64_t M = count * n;
  // about two workgroups per CU over all dims, a thread at least one unrolled
  // round, and fewer than 2^31 elements per workgroup (the LDS counts)
  int64_t bx = (M + (int64_t)kCountT * kUnroll - 1) / ((int64_t)kCountT * kUnroll);
  const int64_t most = 512 / d > 1 ? 512 / d : 1;
  if (bx > most) bx = most;
  const int64_t least = (M >> 31) + 1;
  if (bx < least) bx = least;
  const int64_t step = bx * kCountT;
  const int32_t glds = pass == 0 ? 1 : (nt < kLdsGroups ? nt : kLdsGroups);
  const size_t lds = (size_t)glds * kBins * sizeof(uint32_t);
  // the search's steps: 2^steps > nt >= the number of groups
  int32_t steps = 1;
  while ((1 << steps) <= nt) ++steps;
  const auto launch = [&](auto kernel) {
    hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                                         hipFuncAttributeMaxDynamicSharedMemorySize,
                                         kLdsGroups * kBins * (int)sizeof(uint32_t));
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(kernel, dim3((unsigned)bx, (unsigned)d), dim3(kCountT), lds, s, tx, n, d,
                       first, M, step / n, step % n, sc, nt, glds, done, bits);
    return hipGetLastError();
  };
  hipError_t err = hipErrorInvalidValue;
  if (pass == 0) err = launch(select_count_kernel<-1>);
  else if (steps == 1) err = launch(select_count_kernel<1>);
  else if (steps == 2) err = launch(select_count_kernel<2>);
  else if (steps == 3) err = launch(select_count_kernel<3>);
  else if (steps == 4) err = launch(select_count_kernel<4>);
  else if (steps == 5) err = launch(select_count_kernel<5>);
  else if (steps == 6) err = launch(select_count_kernel<6>);
  else if (steps == 7) err = launch(select_count_kernel<7>);
  else if (steps == 8) err = launch(select_count_kernel<8>);
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(select_pick_kernel, dim3((unsigned)d), dim3(kPickT), 0, s, sc, d, nt, bits,
                     pass == kPasses - 1 ? 1 : 0);
  return hipGetLastError();
}

}  // namespace pbh
