// pbh_trace_host.h -- the host arithmetic of the trace reductions: the window
// check every trace entry point makes, the checks of a quantile list, and the
// host steps of the pooled quantile around the device's radix select, and the
// geometry and scratch layout of the pooled sort (pbh_rank.hip), and the layout
// and the estimator of the ESS across chains (pbh_ess_rank.hip), the layout and
// the merges of the pointwise reduction (pbh_pointwise.hip), and the pick and
// the finish of its tail select (pbh_pointwise_tail.hip), the layout and the
// last step of the pooled covariance (pbh_cov.hip), and the checks, the choice
// of lookup and the layouts of the pooled histograms (pbh_hist.hip).  No HIP: a host
// compiler alone builds it (tests/trace_host_main.cpp, the one program the CPU
// tests drive it through).  Built with -ffp-contract=off: the interpolation and
// the estimator must round as NumPy's do.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "pbh_hist_bin.h"
#include "pbh_pointwise_merge.h"

namespace pbh {

// Whether records [first, first + count) lie inside [0, rec) with count >=
// min_count (rec >= 0): no sum is formed, so no argument overflows.
bool trace_window_ok(int64_t rec, int64_t first, int64_t count, int64_t min_count);
// first + count for the message of a refused window, saturated at the ends of
// int64 where the sum leaves it.
int64_t trace_window_end(int64_t first, int64_t count);

// What is wrong with the quantiles q[0..nq) (nq in 1..PBH_QUANTILE_MAX_Q,
// every q[j] in [0, 1]; a NaN is not), or empty.
std::string quantile_list_error(int32_t nq, const double *q);

// The pooled quantiles q[0..nq) of M values, as diag.pooled_quantile places
// them: vi = (M - 1) q, lo = floor(vi), hi = min(lo + 1, M - 1), frac = vi - lo.
// ranks: the order statistics the device selects -- every lo and hi and M - 1
// (the largest element: a NaN if the dim holds one), sorted and distinct.
struct PooledPlan {
  std::vector<int64_t> lo, hi;
  std::vector<double> frac;
  std::vector<uint64_t> ranks;
};
PooledPlan pooled_plan(int64_t M, int32_t nq, const double *q);
// stats [d][nt], the values at p.ranks per dim -> out [nq][d], and with
// order_stats [nq][2][d] the two values each quantile is interpolated
// between.  A dim whose largest element is a NaN gives NaN for every q.
void pooled_interpolate(const PooledPlan &p, int64_t d, const double *stats, double *out,
                        double *order_stats);

// The geometry and the scratch of the pooled sort behind the rank-normalised
// R-hat (pbh_rank.hip), which runs one dim and one variant at a time over M =
// n count elements.  A tile is what one workgroup sorts by a digit; the
// [tile][digit] table of a pass is scanned in `chunks` (at most
// kRankMaxChunks) runs of chunk_tiles consecutive tiles.  The offsets are in
// bytes from the start of the reduction scratch, each a multiple of 256, the
// regions disjoint and in this order: the select's own scratch (the median),
// med [d], res [2][d], the eight passes' skip flags, chunk [chunks][256] and
// hist [tiles][256] (uint32), stats [6][n], the two key buffers (uint64 [M]),
// the two index buffers (uint32 [M]), z [M] and, with want_ranks, r [M]
// (doubles).
constexpr int64_t kRankTile = 2048;
constexpr int64_t kRankBins = 256;
constexpr int64_t kRankMaxChunks = 256;
struct RankLayout {
  int64_t M, tiles, chunk_tiles, chunks;
  int64_t select, med, res, state, chunk, hist, stats, key[2], idx[2], z, r, bytes;
};
// False when M = n count does not fit the 32-bit index the sort carries (M >=
// 2^32, or the product leaves int64) or an argument is out of range (n, count
// < 1, d < 1, select_words < 0); `out` is then untouched.
bool rank_layout(int64_t n, int64_t count, int32_t d, int64_t select_words, bool want_ranks,
                 RankLayout *out);

// The bulk- and tail-ESS across chains (pbh_ess_rank.hip), one dim and one
// variant (bulk, tail_lower, tail_upper, basic) at a time.  The ceil(n / 2)
// chain pairs of a dim are cut into `groups` (at most kEssMaxGroups) runs of
// `run` consecutive pairs, a workgroup and a partial row of kEssPoints power
// sums each.  The scratch behind `base` bytes (RankLayout.bytes when the bulk
// variant sorts, else 0), each offset a multiple of 256, the regions disjoint
// and in this order: the select's own scratch (the tail's two quantiles), thr
// [2][d], part [groups][kEssPoints], acov [4][d][h], means [4][2][d][n] (first
// halves, second halves) and stats [6][d][n] (the values' rows of
// launch_rhat_chain).
constexpr int64_t kEssPoints = 4096;
constexpr int64_t kEssMaxGroups = 512;
struct EssLayout {
  int64_t h, pairs, run, groups;
  int64_t select, thr, part, acov, means, stats, bytes;
};
// False when an argument is out of range (n < 1, count < 4, count / 2 >
// PBH_ESS_RANK_MAX_HALF, d < 1, base < 0 or no multiple of 256, select_words <
// 0); `out` is then untouched.
bool ess_layout(int64_t n, int64_t count, int32_t d, int64_t base, int64_t select_words,
                EssLayout *out);

// The effective sample size of C split chains of h records from their means m
// [C] and mean autocovariance A [h]: diag.multi_chain_ess in exactly its
// operation order (the variance of the means, rho, Geyer's pairs, the scan,
// the running minimum, tau), so the two give the same bits.  C >= 2, h >= 2.
// k_star (may be null): where the scan stopped.
double multi_chain_ess(const double *m, const double *A, int64_t C, int64_t h,
                       int64_t *k_star = nullptr);

// The pointwise reduction (pbh_pointwise.hip): the statistics over the draws
// of a window of every observation's term.  A workgroup owns one block of
// kPointwiseLanes chains, one tile of kPointwiseTile observations and one slice
// of slice_len consecutive records (the last slice may be shorter); the record
// slices are there to fill the device when chains and tiles are few: as many as
// bring the grid to kPointwiseGroups workgroups, at most one per record.  Each
// workgroup leaves one partial row, row = chain block * slices + slice, of npad
// = 8 tiles observations.  The scratch, each offset a multiple of 256, the
// regions disjoint and in this order: the select's own scratch (none today),
// prog (the program's block as expr_pack lays it out, prog_doubles doubles),
// part [6][rows][npad] (the maximum, the sum; the count, the shift, the mean
// less the shift, M2) and res [3][npad] (lse, mean, var).
constexpr int64_t kPointwiseGroups = 1024;
struct PointwiseLayout {
  int64_t chain_blocks, tiles, npad, slices, slice_len, rows;
  int64_t select, prog, part, res, bytes;
};
// False when an argument is out of range (n, count < 1, n_obs outside 1 ..
// PBH_EXPR_MAX_OBS, select_words < 0, prog_doubles < 1), n count leaves int64,
// or the chain blocks exceed a grid's 65 535; `out` is then untouched.
bool pointwise_layout(int64_t n, int64_t count, int32_t n_obs, int64_t select_words,
                      int64_t prog_doubles, PointwiseLayout *out);
// A workgroup's combination of its lanes' partials of one observation, lse and
// mom [kPointwiseLanes], in the device's order (pbh_pointwise_merge.h).
void pointwise_combine(const LsePair *lse, const Moments *mom, LsePair *lse_out,
                       Moments *mom_out);
// The finish: `rows` partial rows of one observation merged in index order,
// then lse, mean and the variance at ddof 1 (any of the three may be null).
void pointwise_finish(const LsePair *lse, const Moments *mom, int64_t rows, double *lse_out,
                      double *mean_out, double *var_out);

// The tail of the pointwise terms (pbh_pointwise_tail.hip): per observation the
// k smallest terms over the S = n count draws of a window and the log-sum-exp
// of minus the others, by a most-significant-digit radix select on tail_key,
// the monotone 64-bit image of a double (pbh_device.h key_image: negative
// values reversed below the positive ones, either zero one image, every NaN
// the largest).  The digits are kTailDigit = 10 bits wide, the seventh the 4
// bits that remain.  The device counts and gathers; the host picks and
// finishes:
//   tail_pick    after a count pass over the keys under the observation's
//       prefix: the digit at which the running count first exceeds the
//       remaining rank is appended to the prefix.
//   tail_settled whether the keys at or under the prefix -- below + under of
//       them -- fit a candidate list of `capacity`; the passes stop when every
//       observation is settled or all 64 bits are fixed.
//   tail_finish  the candidates the device gathered (keys whose prefix is <=
//       the observation's; with all 64 bits fixed only the keys below the cut,
//       the `under` keys equal to it being neither gathered nor folded),
//       sorted; the first k are the tail, filled up with the cut; what remains
//       is pushed in ascending order into a log-sum-exp pair of the negated
//       values (remaining ties as one pair (-v, count)) and merged with the
//       device's partial rows in index order.
constexpr int kTailDigit = 10, kTailBins = 1 << kTailDigit;
inline int tail_digit_bits(int done) { return 64 - done < kTailDigit ? 64 - done : kTailDigit; }
uint64_t tail_key(double v);
double tail_key_value(uint64_t key);   // +0.0 for either zero, one quiet NaN for every NaN
// prefix: the `done` bits fixed so far, right-aligned; rank: the rank that
// remains among the `under` keys under the prefix; below: the keys whose
// prefix is smaller.  Start: (0, k - 1, 0, S).
struct TailState {
  uint64_t prefix, rank, below, under;
};
// hist [1 << bits]: the counts of the next digit among the keys under s.prefix
// (their sum is s.under, rank < under).
void tail_pick(const uint64_t *hist, int bits, TailState *s);
inline bool tail_settled(const TailState &s, int64_t capacity) {
  return s.below + s.under <= (uint64_t)capacity;
}
// How many candidates the device gathers for s after `done` bits.
inline uint64_t tail_candidates(const TailState &s, int done) {
  return done == 64 ? s.below : s.below + s.under;
}
// keys [n_keys]: the gathered candidates in any order (sorted in place), n_keys
// = tail_candidates(s, done) >= k, or with done == 64 >= k - s.under.  rows
// [n_rows]: the device's partial pairs of the other terms, negated.  tail [k]
// and rest_lse may be null.
void tail_finish(uint64_t *keys, int64_t n_keys, int64_t k, int done, const TailState &s,
                 const LsePair *rows, int64_t n_rows, double *tail, double *rest_lse);

// The select's scratch of one batch of `tiles` observation tiles, in 8-byte
// words from the start of the reduction scratch (pointwise_layout's select
// region): prefix [npad], cursor [npad], hist [npad][kTailBins], list [npad]
// [capacity], npad = 8 tiles.  The lists are held to kTailListBytes whatever
// n_obs is: tail_batch_tiles is how many tiles a batch may hold, at least 1 --
// capacity <= kTailMaxCapacity = kTailListBytes / 64 makes one tile fit.
constexpr int64_t kTailListBytes = (int64_t)256 << 20;
constexpr int64_t kTailMaxCapacity = kTailListBytes / (8 * kPointwiseTile);
struct TailLayout {
  int64_t npad, prefix, cursor, hist, list, words;
};
int64_t tail_batch_tiles(int64_t capacity);
TailLayout tail_layout(int64_t tiles, int64_t capacity);
// max(2 k, 65 536)
int64_t tail_default_capacity(int64_t k);

// The pooled covariance (pbh_cov.hip): the sums S_a of v_a and P_ab (a <= b) of
// v_a v_b over every chain and record of a window, v = x - K, K the mean over
// chains of the window's first record.  The dims go in tiles of at most
// kCovTile: up to kCovTile dims one tile holds S and the whole triangle; above,
// `pairs` tile jobs -- the two diagonal tiles of kCovTile dims (S and the
// tile's triangle) and the rectangles of kCovHalf x kCovHalf dims between
// them -- each read their dims of the window once.  A workgroup owns one block of kCovLanes
// chains, one tile job and one slice of slice_len consecutive records (the
// last slice may be shorter); the record slices fill the device when chains
// are few, as pointwise_layout's do: as many as bring the grid to
// kPointwiseGroups workgroups, at most one per record.  The workgroups of a
// (chain block, slice) fill one partial row, row = chain block * slices +
// slice, of cols = d + d (d + 1) / 2 doubles: S [d], then P's upper triangle
// row by row (cov_tri).  The scratch, each offset a multiple of 256, the
// regions disjoint and in this order: K [d], part [rows][cols], res [cols].
constexpr int kCovLanes = 256, kCovTile = 16, kCovHalf = 8;
struct CovLayout {
  int64_t pairs, chain_blocks, slices, slice_len, rows, cols;
  int64_t K, part, res, bytes;
};
// where P_ab, a <= b < d, lies in the packed triangle
constexpr int64_t cov_tri(int64_t a, int64_t b, int64_t d) {
  return a * d - a * (a - 1) / 2 + (b - a);
}
// False when an argument is out of range (n, count < 1, d outside 1 ..
// PBH_MAX_DIM), n count leaves int64, or the chain blocks exceed a grid's 2^31
// - 1; `out` is then untouched.
bool cov_layout(int64_t n, int64_t count, int32_t d, CovLayout *out);
// The last step, from the merged sums over M draws: mean [d] = K + S / M, cov
// [d][d] = (P_ab - S_a S_b / M) / (M - 1) for a <= b and mirrored, corr [d][d]
// = cov_ab / sqrt(cov_aa cov_bb), the diagonal included (1, or NaN for a dim
// that never moves) -- diag.pooled_cov_finish in exactly its operation order,
// so the two give the same bits.  P: the packed triangle.  Any of the three
// results may be null.
void cov_finish(const double *K, const double *S, const double *P, int64_t M, int32_t d,
                double *mean, double *cov, double *corr);

// The pooled histograms (pbh_hist.hip): per dim the counts of the draws of a
// window in the bins of strictly increasing finite edges, and per pair of dims
// the counts in the grid of the two dims' bins; pbh_hist_bin.h has the lookup.
// n_bins [d]: B_k, 0 for a dim that is skipped; edges: the dims' B_k + 1 edges
// one after the other.
constexpr int kHistLanes = 256, kHistMaxDims = 32;   // (PBH_MAX_DIM)
// what one workgroup's LDS holds of a dim group (two workgroups per CU of 160 KiB)
constexpr int64_t kHistLdsBudget = 64 * 1024;
// the records of a slice: a workgroup's uint32 counter takes at most kHistLanes
// x kHistMaxSlice < 2^32 elements
constexpr int64_t kHistMaxSlice = ((int64_t)1 << 24) - 1;
// What is wrong with the edges, naming the dim and the index, or empty: an
// n_bins[k] outside 0 .. PBH_HIST_MAX_BINS, every n_bins[k] 0, an edge that is
// not finite, edges that do not strictly increase.
std::string hist_check_edges(int32_t d, const int32_t *n_bins, const double *edges);
// Whether the guess path of pbh_hist_bin.h is right for every double with these
// edges e [bins + 1] (checked: strictly increasing, finite): s = bins / (e[bins] -
// e[0]) is finite and above 0, and hist_guess lies within one of i at e[i] and
// at the double just below e[i + 1], for every bin i.
bool hist_guess_ok(const double *e, int32_t bins);
// A dim's lookup: mode kHistGuess or the search's depth; s is read by the guess
// alone.  bins == 0: a skipped dim, all 0.
struct HistDimPlan {
  int32_t bins, mode;
  double e0, eB, s;
};
HistDimPlan hist_dim_plan(const double *e, int32_t bins);
// The dim's table t [hist_table_len(bins)] for its mode (pbh_hist_bin.h).
void hist_fill_table(const double *e, const HistDimPlan &p, double *t);

// hist_layout: the listed dims (n_bins[k] > 0) in ascending order go in dim
// groups of consecutive listed dims.  A listed dim takes lds(k) = 8
// hist_table_len(B_k) + 4 (B_k + 3) bytes, rounded up to 8: its table and its
// uint32 counters (the bins, then below, above, NaN).  A dim with lds(k) above
// half of kHistLdsBudget is a group of its own; the others fill a group while
// the sum stays within the budget.  A workgroup owns one block of kHistLanes
// chains, one dim group and one slice of slice_len <= kHistMaxSlice consecutive
// records (the last may be shorter): as many slices as bring the grid to
// kPointwiseGroups workgroups, at most one per record, as cov_layout forms
// them.  A group's LDS: its dims' tables one after the other, then their
// counters one after the other; tab[j] / ctr[j] are where listed dim j's lie
// among the group's, tab_off[g] / ctr_off[g] where the group's lie among all
// (the same order in the scratch), tab_len[g] / ctr_len[g] how many.  The
// scratch, each offset a multiple of 256, the regions disjoint and in this
// order: tables (n_tab doubles), counts (n_ctr uint64).
struct HistLayout {
  int32_t dims, groups;
  int32_t dim[kHistMaxDims], tab[kHistMaxDims], ctr[kHistMaxDims];                // per listed dim
  int32_t group_first[kHistMaxDims + 1];                                           // listed dims
  int32_t tab_off[kHistMaxDims], tab_len[kHistMaxDims], ctr_off[kHistMaxDims],     // per group
      ctr_len[kHistMaxDims];
  int64_t lds_bytes;   // of the largest group
  int64_t chain_blocks, slices, slice_len, n_tab, n_ctr;
  int64_t tables, counts, bytes;
};
// False when an argument is out of range (n, count < 1, d outside 1 ..
// kHistMaxDims, an n_bins[k] outside 0 .. PBH_HIST_MAX_BINS, no dim listed), n
// count leaves int64, the chain blocks exceed 2^31 - 1 or the slices a grid's
// 65 535; `out` is then untouched.
bool hist_layout(int64_t n, int64_t count, int32_t d, const int32_t *n_bins, HistLayout *out);

// hist2d_layout: a workgroup owns one block of kHistLanes chains, one pair and
// one slice of records, formed as above with the pairs in the groups' place.
// Its LDS: the table of dim a, the table of dim b, the B_a B_b uint32 cells.
// tab_off[k]: where dim k's table lies among the tables of the dims that have
// edges (all of them, in ascending order), -1 without edges; out[p]: where the
// pair's cells lie among the counts.  The scratch, each offset a multiple of
// 256, the regions disjoint and in this order: tables (n_tab doubles), pairs
// (n_pairs records of 4 int64: a, b, out, 0), counts (n_ctr uint64).
struct Hist2dLayout {
  int32_t n_pairs;
  int32_t tab_off[kHistMaxDims];
  std::vector<int64_t> out;
  int64_t lds_bytes;   // of the largest pair
  int64_t chain_blocks, slices, slice_len, n_tab, n_ctr;
  int64_t tables, pairs, counts, bytes;
};
// What is wrong with the pairs [n_pairs][2], naming the pair, or empty: n_pairs
// outside 1 .. 65 535, a dim outside [0, d), a dim without edges, B_a B_b above
// PBH_HIST2D_MAX_CELLS.  a == b is allowed.
std::string hist2d_check_pairs(int32_t d, const int32_t *n_bins, int32_t n_pairs,
                               const int32_t *pairs);
// False when an argument is out of range (as hist_layout's, and the pairs as
// hist2d_check_pairs has them); `out` is then untouched.
bool hist2d_layout(int64_t n, int64_t count, int32_t d, const int32_t *n_bins, int32_t n_pairs,
                   const int32_t *pairs, Hist2dLayout *out);

}  // namespace pbh
