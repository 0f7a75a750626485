// pbh_pointwise_tail.hip -- pbh_trace_pointwise_tail on gfx950: per observation
// j, the k smallest of the terms T[s, j] a pointwise program gives over the
// draws of a trace window, and the log-sum-exp of -T over the other draws
// (diag.pointwise_tail is the host definition).  It is what Pareto-smoothed
// importance sampling needs of the [draws][observations] matrix, which is never
// formed: every pass recomputes the terms with pointwise_kernel's grid and walk
// (pbh_pointwise_impl.h) and keeps integers only.
//
// A most-significant-digit radix select on key_image(T[s, j]), one select per
// observation, the host in the loop (pbh_trace_host.h tail_pick, tail_finish):
//
//   tail_count_kernel   per term whose key's high `done` bits equal its
//       observation's prefix, one is added to (observation, next digit) in an
//       LDS histogram of uint32, privatised per workgroup and flushed once to
//       the global uint64 histogram [npad][1 024] with 64-bit integer atomics,
//       zeros skipped.  The lanes of a wave that hit the counter of its first
//       active lane add once for all of them (chains that never move put a
//       whole wave on one counter).
//   tail_gather_kernel  one more walk.  A term whose key prefix is <= its
//       observation's is appended to that observation's candidate list: the
//       wave's appending lanes take their places with one atomic add to the
//       list's cursor.  Every other term is folded as lse_push(., -t) into the
//       lane's pair; the lanes merge as pointwise_kernel's do
//       (pointwise_merge_lanes) into one partial row per workgroup, which the
//       host merges in index order.  With all 64 bits fixed the prefix is the
//       cut's key: keys below it are appended, keys above it folded, keys equal
//       to it neither -- the host knows their count.  A place at or past the
//       list's capacity is not written.
//
// Digits: 10 bits (six passes) and the 4 that remain (the seventh).  LDS per
// workgroup: the interpreter's slots 32 KB and body temporaries 64 KB, and in
// the count kernel the histogram 8 observations x 1 024 bins x 4 bytes = 32 KB:
// 128 KB of the 160 KB (an 11-bit digit's 64 KB would not fit); the gather
// kernel takes the 96 KB of pointwise_kernel.
//
// Only integer atomics: the histograms do not depend on their order, and the
// order in which a list was filled is lost in the host's sort, so two calls
// give the same bits.  -ffp-contract=off, and the unit goes through the E64
// pass, as pbh_pointwise.hip does.
#include "pbh_device.h"   // key_image
#include "pbh_kernels.h"
#include "pbh_pointwise_impl.h"

namespace pbh {
namespace {

static_assert(kW * kTailBins * 4 + (kExprSlots + kExprTemps * kW) * kBlock * 8 <= 160 * 1024,
              "slots, temporaries and the histogram fit the LDS");

struct TailArgs {
  int32_t tile0, n_obs;      // the batch's first tile; observations of the program
  int32_t done, bits;        // bits fixed so far; the width of the digit counted
  int64_t capacity;          // of a candidate list
  const uint64_t *prefix;    // [npad] of the batch, right-aligned
  uint64_t *hist;            // [npad][kTailBins]
  unsigned long long *cursor;   // [npad]
  uint64_t *list;            // [npad][capacity]
};

constexpr uint32_t kNone = ~0u;

// Adds one to the LDS counter `at` (pbh_select.hip add_one): the lanes on the
// first active lane's counter add once for all of them.
__device__ __forceinline__ void add_one(uint32_t *hist, uint32_t at) {
  if (at == kNone) return;
  const uint32_t at0 = __builtin_amdgcn_readfirstlane(at);
  const uint64_t same = __ballot(at == at0);
  uint32_t by = 1u;
  if (at == at0) {
    if (__ffsll((unsigned long long)same) - 1 != (int)__lane_id()) return;
    by = (uint32_t)__popcll(same);
  }
  atomicAdd(&hist[at], by);
}

// the high `done` bits of a key, right-aligned (0 of them: 0)
__device__ __forceinline__ uint64_t key_prefix(uint64_t key, int32_t done) {
  return done ? key >> (64 - done) : 0ull;
}

__global__ __launch_bounds__(kBlock) void tail_count_kernel(KArgs a, PointwiseArgs p, TailArgs q) {
  __shared__ double s_slot[kExprSlots * kBlock];
  __shared__ double s_temp[kExprTemps * kW * kBlock];
  __shared__ uint32_t s_hist[kW * kTailBins];
  const PointwiseGroup g = pointwise_group(p, q.tile0 + (int)blockIdx.x);
  const int jb = blockIdx.x * kW;   // the tile's first observation in the batch
  for (int i = threadIdx.x; i < kW * kTailBins; i += kBlock) s_hist[i] = 0u;
  uint64_t pfx[kW];
#pragma unroll
  for (int i = 0; i < kW; ++i) pfx[i] = q.prefix[jb + i];
  __syncthreads();
  const int shift = 64 - q.done - q.bits;
  const uint32_t mask = (1u << q.bits) - 1u;

  pointwise_walk(a, p, g, s_slot + threadIdx.x, s_temp + threadIdx.x,
                 [&](int64_t, const double (&t)[kW]) {
    if (!g.live) return;
#pragma unroll
    for (int i = 0; i < kW; ++i) {
      if (g.j0 + i >= q.n_obs) continue;   // (the last tile's padding)
      const uint64_t key = key_image(t[i]);
      const uint32_t digit = (uint32_t)(key >> shift) & mask;
      add_one(s_hist, key_prefix(key, q.done) == pfx[i] ? i * kTailBins + digit : kNone);
    }
  });

  __syncthreads();
  uint64_t *hist = q.hist + (int64_t)jb * kTailBins;
  for (int i = threadIdx.x; i < kW * kTailBins; i += kBlock) {
    const uint32_t v = s_hist[i];
    if (v) atomicAdd((unsigned long long *)&hist[i], (unsigned long long)v);
  }
}

__global__ __launch_bounds__(kBlock) void tail_gather_kernel(KArgs a, PointwiseArgs p,
                                                             TailArgs q) {
  __shared__ double s_slot[kExprSlots * kBlock];
  __shared__ double s_temp[kExprTemps * kW * kBlock];
  const PointwiseGroup g = pointwise_group(p, q.tile0 + (int)blockIdx.x);
  const int jb = blockIdx.x * kW;
  uint64_t pfx[kW];
#pragma unroll
  for (int i = 0; i < kW; ++i) pfx[i] = q.prefix[jb + i];
  const bool fixed = q.done == 64;
  const int lane = (int)__lane_id();

  LsePair lse[kW];
  Moments mom[kW];
#pragma unroll
  for (int i = 0; i < kW; ++i) {
    lse[i] = lse_identity();
    mom[i] = moments_identity();   // (none kept: the merge's identity throughout)
  }
  pointwise_walk(a, p, g, s_slot + threadIdx.x, s_temp + threadIdx.x,
                 [&](int64_t, const double (&t)[kW]) {
#pragma unroll
    for (int i = 0; i < kW; ++i) {
      if (g.j0 + i >= q.n_obs) continue;   // (uniform: every lane takes every ballot)
      const uint64_t key = key_image(t[i]);
      const uint64_t hi = fixed ? key : key_prefix(key, q.done);
      const bool app = g.live && (fixed ? hi < pfx[i] : hi <= pfx[i]);
      const bool fold = g.live && hi > pfx[i];
      const LsePair pushed = lse_push(lse[i], -t[i]);
      if (fold) lse[i] = pushed;
      const uint64_t takers = __ballot(app);
      if (takers) {
        const int leader = __ffsll((unsigned long long)takers) - 1;
        unsigned long long base = 0;
        if (lane == leader)
          base = atomicAdd(&q.cursor[jb + i], (unsigned long long)__popcll(takers));
        base = __shfl(base, leader);
        const unsigned long long at = base + __popcll(takers & ((1ull << lane) - 1ull));
        if (app && at < (unsigned long long)q.capacity)
          q.list[(int64_t)(jb + i) * q.capacity + (int64_t)at] = key;
      }
    }
  });

  LsePair fl;
  Moments fm;
  int o, t;
  pointwise_merge_lanes(lse, mom, g.live, s_slot, s_temp, &fl, &fm, &o, &t);
  if (t == 0) {
    const int64_t row = g.block * p.slices + g.slice, plane = p.rows * p.npad;
    double *out = p.part + row * p.npad + jb + o;
    out[0 * plane] = fl.m;
    out[1 * plane] = fl.s;
  }
}

void bind(const TailLaunch &t, int32_t done, int32_t bits, KArgs *a, PointwiseArgs *p,
          TailArgs *q) {
  const PointwiseLayout &l = *t.pl;
  *a = KArgs{};
  a->d = t.d;
  expr_bind(*a, t.prog, *t.el);
  *p = PointwiseArgs{};
  p->tx = t.tx;
  p->n = t.n;
  p->first = t.first;
  p->count = t.count;
  p->slice_len = l.slice_len;
  p->slices = l.slices;
  p->rows = l.rows;
  p->npad = l.npad;
  p->d = t.d;
  p->loop_pc = t.loop_pc;
  p->body_len = t.el->n_code - t.loop_pc - 2;
  p->part = reinterpret_cast<double *>(t.scratch + l.part);
  uint64_t *sel = reinterpret_cast<uint64_t *>(t.scratch + l.select);
  *q = TailArgs{};
  q->tile0 = t.tile0;
  q->n_obs = t.n_obs;
  q->done = done;
  q->bits = bits;
  q->capacity = t.capacity;
  q->prefix = sel + t.tl->prefix;
  q->hist = sel + t.tl->hist;
  q->cursor = reinterpret_cast<unsigned long long *>(sel + t.tl->cursor);
  q->list = sel + t.tl->list;
}

dim3 grid_of(const PointwiseLayout &l) {
  return dim3((unsigned)l.tiles, (unsigned)l.chain_blocks, (unsigned)l.slices);
}

}  // namespace

hipError_t launch_tail_count(const TailLaunch &t, int32_t done, hipStream_t s) {
  KArgs a;
  PointwiseArgs p;
  TailArgs q;
  bind(t, done, tail_digit_bits(done), &a, &p, &q);
  hipError_t err = hipMemsetAsync(q.hist, 0, (size_t)t.tl->npad * kTailBins * 8, s);
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(tail_count_kernel, grid_of(*t.pl), dim3(kBlock), 0, s, a, p, q);
  return hipGetLastError();
}

hipError_t launch_tail_gather(const TailLaunch &t, int32_t done, hipStream_t s) {
  KArgs a;
  PointwiseArgs p;
  TailArgs q;
  bind(t, done, 0, &a, &p, &q);
  hipError_t err = hipMemsetAsync(q.cursor, 0, (size_t)t.tl->npad * 8, s);
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(tail_gather_kernel, grid_of(*t.pl), dim3(kBlock), 0, s, a, p, q);
  return hipGetLastError();
}

}  // namespace pbh
