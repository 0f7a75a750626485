// pbh_rank.hip -- the ranks of a recorded trace pooled over chains and records,
// per dim, and their normal scores, on gfx950: what the rank-normalised and
// the folded split-R-hat (Vehtari et al. 2021) are reduced from, without the
// trace leaving the device.  probayes_amd/diag.py average_ranks / normal_scores
// / rank_rhat are the host definition.
//
// One dim and one variant (plain, folded about the pooled median) at a time,
// over the M = count * n elements of the window, element e = record * n +
// chain.  M < 2^32: the sort carries e as a 32-bit payload.
//
//   keys    rank_keys_kernel walks the window as select_count_kernel does
//           (consecutive lanes on consecutive chains, (record, chain) advanced
//           without a division, four loads in flight per lane) and writes
//           key_image(x), or key_image(fabs(x - med)) with med the dim's pooled
//           median read from device memory.  8 B read, 8 B written per element.
//   sort    a least-significant-digit radix sort of (key, e) by eight 8-bit
//           digits between two key and two index buffers.  A tile is 2 048
//           consecutive elements, one workgroup of four waves; wave w owns the
//           tile's elements [512 w, 512 w + 512) in eight rounds of 64.  Per
//           pass:
//             rank_hist_kernel     the tile's count per digit -> hist [tile]
//                                  [digit] (8 B read per element).  LDS atomics
//                                  on counts only: a count does not depend on
//                                  the order of its increments.
//             rank_chunk_kernel    the tiles are cut into at most 256 chunks of
//                                  chunk_tiles consecutive tiles; thread = digit
//                                  sums its column over the chunk's tiles.
//             rank_offsets_kernel  one workgroup: the 256 digit totals, their
//                                  exclusive scan (the digit's first position),
//                                  and per digit the running sum over the
//                                  chunks -> chunk [chunk][digit], a position.
//                                  If one digit holds all M elements the pass
//                                  would move nothing: it marks the pass
//                                  skipped, and the two kernels after it return
//                                  at once.
//             rank_tiles_kernel    per chunk, thread = digit: the running sum
//                                  over the chunk's tiles, in place -> hist
//                                  [tile][digit] is the position of the tile's
//                                  first element of the digit.
//             rank_scatter_kernel  the tile's elements to their positions (12 B
//                                  read, 12 B written per element; the first
//                                  pass that runs reads no index: it is e).
//                                  In a round the lanes of a wave on one digit
//                                  are found by one __ballot per digit bit; a
//                                  lane's place among them is the popcount of
//                                  the lower ones.  The wave's count per digit
//                                  is formed first, the digits and within a
//                                  digit the waves are scanned in order, then
//                                  each round adds its lanes in lane order:
//                                  that is the element's slot in the tile's
//                                  sorted order, and the tile is put in that
//                                  order in LDS.  From there consecutive lanes
//                                  store consecutive slots, which within a
//                                  digit are consecutive positions: the
//                                  stores run as long as the tile's share of
//                                  a digit.  Element order is kept within a
//                                  tile, tiles are in order by the scan, so
//                                  every pass is stable.  No atomic decides a
//                                  position.
//           Which buffer holds the data before pass p follows from the skip
//           marks of the passes before it (their parity), read on the device:
//           the host makes no round trip during the sort.  A pass that runs
//           moves 32 B per element (8 + 12 + 12; 28 B for the first), a skipped
//           one 8 B; the tables are 5 KiB of traffic per tile on top, 2.5 B per
//           element.
//   scores  rank_score_kernel: the thread of sorted position p finds the run
//           [lo, hi) of keys equal to its own (pbh_rank_impl.h equal_run), r =
//           (lo + hi + 1) / 2, z = AS241 of (r - 3/8) / (M + 1/4), and writes z
//           (and r, when ranks are wanted) at its element's index, under index
//           < M.  12 B read (the neighbours come from cache), 8 or 16 B written
//           per element, in partial lines.  If the largest key is the NaN
//           image, every rank and score is NaN.
//
// The scores of a dim are a [count][n] buffer: launch_rhat_chain and
// launch_rhat_cross (pbh_rhat.hip) reduce it as a one-dim trace, in their
// fixed order.  The sort's state is integer counts and positions, so two
// calls give the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pbh_device.h"   // key_image
#include "pbh_kernels.h"
#include "pbh_rank_impl.h"
#include "pbh_trace_host.h"   // RankLayout, kRankTile, kRankBins

namespace pbh {
namespace {

constexpr int kPasses = 8;          // 8-bit digits of a 64-bit key
constexpr int kBins = (int)kRankBins;
constexpr int kTileT = 256;         // workgroup of a tile: thread = digit in the tables
constexpr int kWaves = kTileT / 64;
constexpr int kRounds = (int)kRankTile / kTileT;   // rounds of 64 per wave, loads per thread
constexpr int kKeysT = 1024;        // workgroup of the key kernel
constexpr int kKeysUnroll = 4;      // loads in flight per lane
constexpr int kScoreT = 256;

static_assert(kTileT == kBins, "a tile's thread is a digit in the table kernels");
static_assert(kRounds * kTileT == kRankTile, "whole rounds");

// grid (bx).  step = bx * kKeysT elements between a thread's elements: step_rec
// = step / n records and step_col = step % n chains.
__global__ __launch_bounds__(kKeysT) void rank_keys_kernel(
    const double *__restrict__ tx, int64_t n, int32_t d, int32_t k, int64_t first, int64_t M,
    int64_t step_rec, int64_t step_col, const double *__restrict__ med,
    uint64_t *__restrict__ keys) {
  const bool fold = med != nullptr;
  const double m = fold ? med[k] : 0.;
  const int64_t dn = (int64_t)d * n;
  const int64_t step = step_rec * n + step_col;
  const int64_t jump = step_rec * dn + step_col, wrap = dn - n;
  int64_t e = (int64_t)blockIdx.x * kKeysT + threadIdx.x;
  int64_t col = e % n;
  const double *p = tx + (first * d + k) * n + (e / n) * dn + col;
  // (e < M keeps p inside the window: p addresses element e of dim k)
  for (; e + (kKeysUnroll - 1) * step < M; e += kKeysUnroll * step) {
    double x[kKeysUnroll];
#pragma unroll
    for (int j = 0; j < kKeysUnroll; ++j) {
      x[j] = *p;
      col += step_col;
      p += jump;
      if (col >= n) {
        col -= n;
        p += wrap;
      }
    }
#pragma unroll
    for (int j = 0; j < kKeysUnroll; ++j)
      keys[e + j * step] = key_image(fold ? fabs(x[j] - m) : x[j]);
  }
  for (; e < M; e += step) {
    const double x = *p;
    col += step_col;
    p += jump;
    if (col >= n) {
      col -= n;
      p += wrap;
    }
    keys[e] = key_image(fold ? fabs(x - m) : x);
  }
}

// The passes before `pass` that ran (state[i] != 0: pass i was skipped).  Its
// parity names the buffer that holds the data; zero: no index written yet.
__device__ __forceinline__ int passes_run(const uint32_t *state, int pass) {
  int c = 0;
  for (int i = 0; i < pass; ++i) c += state[i] == 0u;
  return c;
}

struct SortBuffers {
  uint64_t *key[2];
  uint32_t *idx[2];
  uint32_t *state;   // [kPasses]
  uint32_t *chunk;   // [chunks][kBins]
  uint32_t *hist;    // [tiles][kBins]
};

// The lanes of the wave whose element is valid and on this lane's digit: one
// __ballot per digit bit.
__device__ __forceinline__ uint64_t same_digit(uint32_t digit, bool valid) {
  uint64_t mask = __ballot(valid);
#pragma unroll
  for (int bit = 0; bit < 8; ++bit) {
    const bool set = (digit >> bit) & 1u;
    const uint64_t with = __ballot(valid && set);
    mask &= set ? with : ~with;
  }
  return mask;
}

// grid (tiles).
__global__ __launch_bounds__(kTileT) void rank_hist_kernel(SortBuffers b, int64_t M, int pass) {
  __shared__ uint32_t s_h[kBins];
  const int tid = threadIdx.x;
  const uint64_t *src = b.key[passes_run(b.state, pass) & 1];
  s_h[tid] = 0u;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * kRankTile;
  uint64_t key[kRounds];
#pragma unroll
  for (int j = 0; j < kRounds; ++j) {
    const int64_t e = base + j * kTileT + tid;
    key[j] = e < M ? src[e] : 0ull;
  }
#pragma unroll
  for (int j = 0; j < kRounds; ++j) {
    const int64_t e = base + j * kTileT + tid;
    // an element past M counts nowhere; the lanes on the first lane's digit add
    // once for them all (tied data puts a whole wave on one counter).  Measured
    // slower: one add per digit present, the lanes matched by
    // ballots as the scatter kernel does; four tiles to a workgroup.
    const uint32_t digit = e < M ? (uint32_t)(key[j] >> (8 * pass)) & 255u : ~0u;
    const uint32_t d0 = __builtin_amdgcn_readfirstlane(digit);
    const uint64_t same = __ballot(digit == d0);
    if (digit != ~0u) {
      if (digit != d0)
        atomicAdd(&s_h[digit], 1u);
      else if (__ffsll((unsigned long long)same) - 1 == (int)__lane_id())
        atomicAdd(&s_h[digit], (uint32_t)__popcll(same));
    }
  }
  __syncthreads();
  b.hist[(int64_t)blockIdx.x * kBins + tid] = s_h[tid];
}

// grid (chunks): chunk[c][digit] = the chunk's count of the digit.
__global__ __launch_bounds__(kTileT) void rank_chunk_kernel(SortBuffers b, int64_t tiles,
                                                            int64_t chunk_tiles) {
  const int tid = threadIdx.x;
  const int64_t t0 = (int64_t)blockIdx.x * chunk_tiles;
  const int64_t t1 = t0 + chunk_tiles < tiles ? t0 + chunk_tiles : tiles;
  uint32_t sum = 0u;
#pragma unroll 8
  for (int64_t t = t0; t < t1; ++t) sum += b.hist[t * kBins + tid];
  b.chunk[(int64_t)blockIdx.x * kBins + tid] = sum;
}

// One workgroup: chunk[c][digit] becomes the position of the chunk's first
// element of the digit, and state[pass] whether one digit holds everything.
__global__ __launch_bounds__(kTileT) void rank_offsets_kernel(SortBuffers b, int64_t chunks,
                                                              int64_t M, int pass) {
  __shared__ uint32_t s_wave[kWaves];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  uint32_t total = 0u;
#pragma unroll 8
  for (int64_t c = 0; c < chunks; ++c) total += b.chunk[c * kBins + tid];
  const int all = __syncthreads_or((int64_t)total == M);
  if (tid == 0) b.state[pass] = all ? 1u : 0u;
  if (all) return;
  // the exclusive scan of the totals over the digits
  uint32_t v = total;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t up = __shfl_up(v, o);
    if (lane >= o) v += up;
  }
  if (lane == 63) s_wave[w] = v;
  __syncthreads();
  uint32_t run = v - total;
  for (int i = 0; i < w; ++i) run += s_wave[i];
  for (int64_t c = 0; c < chunks; ++c) {
    const uint32_t here = b.chunk[c * kBins + tid];
    b.chunk[c * kBins + tid] = run;
    run += here;
  }
}

// grid (chunks): hist[t][digit] becomes the position of tile t's first element
// of the digit.
__global__ __launch_bounds__(kTileT) void rank_tiles_kernel(SortBuffers b, int64_t tiles,
                                                            int64_t chunk_tiles, int pass) {
  if (b.state[pass]) return;
  const int tid = threadIdx.x;
  const int64_t t0 = (int64_t)blockIdx.x * chunk_tiles;
  const int64_t t1 = t0 + chunk_tiles < tiles ? t0 + chunk_tiles : tiles;
  uint32_t run = b.chunk[(int64_t)blockIdx.x * kBins + tid];
  for (int64_t t = t0; t < t1; ++t) {
    const uint32_t here = b.hist[t * kBins + tid];
    b.hist[t * kBins + tid] = run;
    run += here;
  }
}

// grid (tiles).
__global__ __launch_bounds__(kTileT) void rank_scatter_kernel(SortBuffers b, int64_t M,
                                                              int pass) {
  __shared__ uint64_t s_key[kRankTile];       // the tile in its sorted order
  __shared__ uint32_t s_idx[kRankTile];
  __shared__ uint32_t s_pos[kWaves][kBins];   // the wave's next slot of a digit
  __shared__ uint32_t s_shift[kBins];         // a digit's position minus its first slot
  __shared__ uint32_t s_wave[kWaves];
  if (b.state[pass]) return;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int ran = passes_run(b.state, pass);
  const uint64_t *src = b.key[ran & 1];
  const uint32_t *src_idx = b.idx[ran & 1];
  uint64_t *dst = b.key[(ran & 1) ^ 1];
  uint32_t *dst_idx = b.idx[(ran & 1) ^ 1];
#pragma unroll
  for (int i = 0; i < kWaves; ++i) s_pos[i][tid] = 0u;
  __syncthreads();
  const int64_t tile0 = (int64_t)blockIdx.x * kRankTile;
  const int64_t base = tile0 + w * (kRounds * 64) + lane;
  const uint64_t below = (1ull << lane) - 1ull;
  uint64_t key[kRounds];
  uint32_t idx[kRounds];
#pragma unroll
  for (int j = 0; j < kRounds; ++j) {
    const int64_t e = base + j * 64;
    key[j] = e < M ? src[e] : 0ull;
    idx[j] = e < M ? (ran ? src_idx[e] : (uint32_t)e) : 0u;
  }
  // Per round the lanes of the wave on this lane's digit: how many are below
  // it (its place among them) and how many there are, kept for the second
  // sweep.  The wave's count per digit: the lowest lane of each digit adds for
  // its lanes (distinct digits, distinct words; rounds in program order).
  uint32_t place[kRounds];   // lanes below | lanes on the digit << 8
#pragma unroll
  for (int j = 0; j < kRounds; ++j) {
    const bool valid = base + j * 64 < M;
    const uint32_t digit = (uint32_t)(key[j] >> (8 * pass)) & 255u;
    const uint64_t mask = same_digit(digit, valid);
    const uint32_t lower = (uint32_t)__popcll(mask & below), all = (uint32_t)__popcll(mask);
    place[j] = lower | (all << 8);
    if (valid && lower == 0u) s_pos[w][digit] += all;
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  // thread = digit: the digit's first slot in the tile's sorted order (the
  // exclusive scan of the tile's counts over the digits), then the waves in
  // order; and what turns a slot of the digit into its position
  uint32_t count = 0u;
#pragma unroll
  for (int i = 0; i < kWaves; ++i) count += s_pos[i][tid];
  uint32_t v = count;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t up = __shfl_up(v, o);
    if (lane >= o) v += up;
  }
  if (lane == 63) s_wave[w] = v;
  __syncthreads();
  uint32_t run = v - count;
  for (int i = 0; i < w; ++i) run += s_wave[i];
  s_shift[tid] = b.hist[(int64_t)blockIdx.x * kBins + tid] - run;   // (modulo 2^32)
#pragma unroll
  for (int i = 0; i < kWaves; ++i) {
    const uint32_t here = s_pos[i][tid];
    s_pos[i][tid] = run;
    run += here;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kRounds; ++j) {
    const bool valid = base + j * 64 < M;
    const uint32_t digit = (uint32_t)(key[j] >> (8 * pass)) & 255u;
    const uint32_t lower = place[j] & 255u;
    const uint32_t slot = s_pos[w][digit] + lower;
    __builtin_amdgcn_wave_barrier();   // every lane has read before the digit's slot moves
    if (valid && lower == 0u) s_pos[w][digit] += place[j] >> 8;
    __builtin_amdgcn_wave_barrier();
    if (valid && slot < (uint32_t)kRankTile) {
      s_key[slot] = key[j];
      s_idx[slot] = idx[j];
    }
  }
  __syncthreads();
  // consecutive lanes take consecutive slots: within a digit consecutive
  // positions, so the stores of a digit's run in the tile are contiguous
  const int64_t held = M - tile0 < kRankTile ? M - tile0 : kRankTile;
#pragma unroll
  for (int j = 0; j < kRounds; ++j) {
    const int slot = j * kTileT + tid;
    if (slot < held) {
      const uint64_t k = s_key[slot];
      const uint32_t at = (uint32_t)slot + s_shift[(uint32_t)(k >> (8 * pass)) & 255u];
      if ((int64_t)at < M) {   // (a consistent table keeps every position below M)
        dst[at] = k;
        dst_idx[at] = s_idx[slot];
      }
    }
  }
}

// grid (ceil(M / kScoreT)).
__global__ __launch_bounds__(kScoreT) void rank_score_kernel(SortBuffers b, int64_t M,
                                                             double *__restrict__ z,
                                                             double *__restrict__ r) {
  const int64_t p = (int64_t)blockIdx.x * kScoreT + threadIdx.x;
  if (p >= M) return;
  const int ran = passes_run(b.state, kPasses);
  const uint64_t *keys = b.key[ran & 1];
  const int64_t e = ran ? (int64_t)b.idx[ran & 1][p] : p;
  double rank, score;
  if (keys[M - 1] == ~0ull) {   // the largest key is the NaN image
    rank = score = __builtin_nan("");
  } else {
    int64_t lo, hi;
    equal_run(keys, M, p, &lo, &hi);
    rank = average_rank(lo, hi);
    score = normal_score(rank, (double)M);
  }
  if (e < M) {
    z[e] = score;
    if (r) r[e] = rank;
  }
}

}  // namespace

hipError_t launch_rank_dim(const double *tx, int64_t n, int32_t d, int32_t k, int64_t first,
                           int64_t count, const double *med, unsigned char *scratch,
                           const RankLayout &l, bool want_ranks, hipStream_t s) {
  if (n < 1 || d < 1 || k < 0 || k >= d || count < 1 || l.M != n * count || l.tiles < 1 ||
      l.chunk_tiles < 1 || l.chunks < 1 || l.chunks > kRankMaxChunks ||
      l.chunks * l.chunk_tiles < l.tiles || l.tiles * kRankTile < l.M)
    return hipErrorInvalidValue;
  const int64_t M = l.M;
  SortBuffers b;
  b.key[0] = reinterpret_cast<uint64_t *>(scratch + l.key[0]);
  b.key[1] = reinterpret_cast<uint64_t *>(scratch + l.key[1]);
  b.idx[0] = reinterpret_cast<uint32_t *>(scratch + l.idx[0]);
  b.idx[1] = reinterpret_cast<uint32_t *>(scratch + l.idx[1]);
  b.state = reinterpret_cast<uint32_t *>(scratch + l.state);
  b.chunk = reinterpret_cast<uint32_t *>(scratch + l.chunk);
  b.hist = reinterpret_cast<uint32_t *>(scratch + l.hist);
  double *z = reinterpret_cast<double *>(scratch + l.z);
  double *r = want_ranks ? reinterpret_cast<double *>(scratch + l.r) : nullptr;

  // a thread takes up to kKeysUnroll elements, a grid's width apart: one
  // unrolled round, or (the last threads, where the round would pass M) singly
  const int64_t bx = (M + (int64_t)kKeysT * kKeysUnroll - 1) / ((int64_t)kKeysT * kKeysUnroll);
  const int64_t step = bx * kKeysT;
  hipLaunchKernelGGL(rank_keys_kernel, dim3((unsigned)bx), dim3(kKeysT), 0, s, tx, n, d, k, first,
                     M, step / n, step % n, med, b.key[0]);
  hipError_t err = hipGetLastError();
  const dim3 tiles((unsigned)l.tiles), chunks((unsigned)l.chunks), wg(kTileT);
  for (int pass = 0; err == hipSuccess && pass < kPasses; ++pass) {
    hipLaunchKernelGGL(rank_hist_kernel, tiles, wg, 0, s, b, M, pass);
    hipLaunchKernelGGL(rank_chunk_kernel, chunks, wg, 0, s, b, l.tiles, l.chunk_tiles);
    hipLaunchKernelGGL(rank_offsets_kernel, dim3(1), wg, 0, s, b, l.chunks, M, pass);
    hipLaunchKernelGGL(rank_tiles_kernel, chunks, wg, 0, s, b, l.tiles, l.chunk_tiles, pass);
    hipLaunchKernelGGL(rank_scatter_kernel, tiles, wg, 0, s, b, M, pass);
    err = hipGetLastError();
  }
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(rank_score_kernel, dim3((unsigned)((M + kScoreT - 1) / kScoreT)),
                     dim3(kScoreT), 0, s, b, M, z, r);
  return hipGetLastError();
}

}  // namespace pbh
