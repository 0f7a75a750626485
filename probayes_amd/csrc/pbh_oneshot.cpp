// pbh_oneshot.cpp -- the entry points of include/pbhip.h that take no engine:
// each allocates its device buffers, uploads, launches, downloads and frees
// within the call.  No kernel lives here: the launches are pbh_kernels.h's.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pbh_engine_state.h"
#include "pbh_expr_host.h"
#include "pbh_device.h"

using pbh::KArgs;
using pbh::check_ptr;
using pbh::fail;

// PBH_EXPR_DATA_WIDE=0: the bodies one observation at a time (the comparison
// form; the default decodes a body word once per block of 8 observations)
int32_t pbh::expr_data_wide() {
  const char *v = std::getenv("PBH_EXPR_DATA_WIDE");
  return (v && v[0] == '0') ? 0 : 1;
}

namespace {

// One call's device work.  The buffers are all allocated before the first
// step; rc keeps the first failed dalloc (none is tried after it), err the
// first failed step (up, down, or `if (c.go()) c.err = ...`: none runs after
// it, or after a failed dalloc).  Everything is freed on scope exit.
struct Call {
  const char *fn;
  int rc = PBH_OK;
  hipError_t err = hipSuccess;
  std::vector<void *> held;
  explicit Call(const char *name) : fn(name) {}
  Call(const Call &) = delete;
  ~Call() {
    for (void *&p : held) pbh::dfree(p);
  }
  template <class T>
  T *alloc(size_t count) {
    T *p = nullptr;
    if (!rc && !(rc = pbh::dalloc(p, count))) held.push_back(p);
    return p;
  }
  bool go() const { return !rc && err == hipSuccess; }
  template <class T>
  void up(T *dst, const T *src, size_t count) {
    if (go()) err = hipMemcpy(dst, src, count * sizeof(T), hipMemcpyHostToDevice);
  }
  template <class T>
  void down(T *dst, const T *src, size_t count) {
    if (go()) err = hipMemcpy(dst, src, count * sizeof(T), hipMemcpyDeviceToHost);
  }
  // the call's status: the dalloc code first, then "<function>: <hip string>"
  int status() const {
    if (rc) return rc;
    if (err != hipSuccess) return fail(PBH_ERR_HIP, "%s: %s", fn, hipGetErrorString(err));
    return PBH_OK;
  }
};

// A private stream and two events for a call that times its kernel (made
// after the call's buffers, gone before them).
struct Timed {
  hipStream_t st = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  double total = 0.;   // ms over the timed launches
  explicit Timed(Call &c) {
    if (c.go()) c.err = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
    if (c.go()) c.err = hipEventCreate(&e0);
    if (c.go()) c.err = hipEventCreate(&e1);
  }
  Timed(const Timed &) = delete;
  ~Timed() {
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (st) (void)hipStreamDestroy(st);
  }
  // Launches r = first .. reps, each prep(st) and then launch(st) between the
  // events; r = 0 is an untimed warm-up (the code object loads lazily on the
  // first launch), r >= 1 add to total.
  template <class Prep, class Launch>
  void run(Call &c, int first, int reps, Prep prep, Launch launch) {
    for (int r = first; r <= reps && c.go(); ++r) {
      c.err = prep(st);
      if (c.go()) c.err = hipEventRecord(e0, st);
      if (c.go()) c.err = launch(st);
      if (c.go()) c.err = hipEventRecord(e1, st);
      if (c.go()) c.err = hipEventSynchronize(e1);
      float ms = 0.f;
      if (c.go()) c.err = hipEventElapsedTime(&ms, e0, e1);
      if (r > 0) total += ms;
    }
  }
};

int eval_expr_impl(const char *fn, int device, const pbh::ExprProgram &p, int64_t n,
                   const double *x, double *out) {
  if (check_ptr(x, "x") || check_ptr(out, "out")) return PBH_ERR_ARG;
  if (n <= 0) return fail(PBH_ERR_ARG, "n must be positive");
  int pc = -1;
  if (const char *why = pbh::expr_check(p, &pc))
    return fail(PBH_ERR_ARG, "expression program: %s (code word %d)", why, pc);
  HIP_TRY(hipSetDevice(device));
  std::vector<double> blk;
  const pbh::ExprLayout lay = pbh::expr_pack(blk, p);
  const int32_t d = p.d;
  std::vector<double> xt((size_t)d * n);
  pbh::rows_to_dim_major(x, xt.data(), n, d);
  Call c(fn);
  double *dblk = c.alloc<double>(blk.size());
  double *dx = c.alloc<double>(xt.size());
  double *dout = c.alloc<double>(n);
  c.up(dblk, blk.data(), blk.size());
  c.up(dx, xt.data(), xt.size());
  if (c.go()) {
    KArgs k{};
    k.d = d;
    k.target = PBH_TARGET_EXPR;
    pbh::expr_bind(k, dblk, lay);
    k.ewide = pbh::expr_data_wide();
    c.err = pbh::launch_eval_expr(k, n, dx, dout);
  }
  c.down(out, dout, n);
  return c.status();
}

// numpy's pairwise sum of a contiguous float64 array (the 8-accumulator
// leaf of <= 128 terms, split at n/2 rounded down to a multiple of 8).
double np_pairwise_host(const double *a, int64_t n) {
  if (n < 8) {
    double r = 0.;
    for (int64_t i = 0; i < n; ++i) r += a[i];
    return r;
  }
  if (n <= 128) {
    double r[8];
    for (int j = 0; j < 8; ++j) r[j] = a[j];
    int64_t i = 8;
    for (; i < n - (n % 8); i += 8)
      for (int j = 0; j < 8; ++j) r[j] += a[i + j];
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += a[i];
    return res;
  }
  int64_t n2 = n / 2;
  n2 -= n2 % 8;
  return np_pairwise_host(a, n2) + np_pairwise_host(a + n2, n - n2);
}

}  // namespace

extern "C" {

int pbh_check_accept(int device, int64_t n, const double *lp,
                     const double *lpp, const uint32_t *t0, const uint32_t *t1,
                     int32_t lin, uint8_t *out) {
  if (check_ptr(lp, "lp") || check_ptr(lpp, "lpp") || check_ptr(t0, "t0") ||
      check_ptr(t1, "t1") || check_ptr(out, "out"))
    return PBH_ERR_ARG;
  if (n <= 0) return fail(PBH_ERR_ARG, "n must be positive");
  HIP_TRY(hipSetDevice(device));
  Call c("pbh_check_accept");
  double *dlp = c.alloc<double>(n), *dlpp = c.alloc<double>(n);
  uint32_t *d0 = c.alloc<uint32_t>(n), *d1 = c.alloc<uint32_t>(n);
  uint8_t *dout = c.alloc<uint8_t>(n);
  c.up(dlp, lp, n);
  c.up(dlpp, lpp, n);
  c.up(d0, t0, n);
  c.up(d1, t1, n);
  if (c.go())
    c.err = pbh::launch_check_accept(n, dlp, dlpp, d0, d1, lin,
                                     std::log(1.7976931348623158e+308), dout);
  c.down(out, dout, n);
  return c.status();
}

int pbh_eval_expr(int device, int32_t d, const int32_t *code, int32_t n_code,
                  const double *consts, int32_t n_consts, int32_t depth, int64_t n,
                  const double *x, double *out) {
  return eval_expr_impl("pbh_eval_expr", device,
                        {d, code, n_code, consts, n_consts, depth, nullptr, 0, 0}, n, x, out);
}

int pbh_eval_expr_data(int device, int32_t d, const int32_t *code, int32_t n_code,
                       const double *consts, int32_t n_consts, int32_t depth,
                       const double *data, int32_t n_cols, int32_t n_obs, int64_t n,
                       const double *x, double *out) {
  if (check_ptr(data, "data")) return PBH_ERR_ARG;
  return eval_expr_impl("pbh_eval_expr_data", device,
                        {d, code, n_code, consts, n_consts, depth, data, n_cols, n_obs}, n, x,
                        out);
}

int pbh_bool_perm_freq(int device, int64_t rows, int32_t cols,
                       const uint8_t *bool2d, int64_t *counts, int32_t reps,
                       double *kernel_ms) {
  if (check_ptr(counts, "counts")) return PBH_ERR_ARG;
  if (cols < 1 || cols > pbh::bool_perm_max_cols())
    return fail(PBH_ERR_ARG, "cols must be in 1..%d, got %d",
                pbh::bool_perm_max_cols(), cols);
  if (rows < 0) return fail(PBH_ERR_ARG, "rows must be >= 0");
  if (rows > 0 && !bool2d) return fail(PBH_ERR_ARG, "bool2d must not be NULL");
  if (reps < 1) return fail(PBH_ERR_ARG, "reps must be >= 1");
  const int64_t nbins = (int64_t)1 << cols;
  if (kernel_ms) *kernel_ms = 0.;
  if (rows == 0) {
    std::memset(counts, 0, nbins * sizeof(int64_t));
    return PBH_OK;
  }
  HIP_TRY(hipSetDevice(device));
  int n_cu = 0;
  HIP_TRY(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device));
  using u64 = unsigned long long;
  Call c("pbh_bool_perm_freq");
  uint8_t *din = c.alloc<uint8_t>(rows * cols);
  u64 *dcnt = c.alloc<u64>(nbins);
  u64 *dscr = c.alloc<u64>(pbh::bool_perm_scratch_words(n_cu));
  Timed tm(c);
  c.up(din, bool2d, (size_t)(rows * cols));
  tm.run(c, 0, reps,
         [&](hipStream_t st) { return hipMemsetAsync(dcnt, 0, nbins * sizeof(u64), st); },
         [&](hipStream_t st) {
           return pbh::launch_bool_perm_freq(din, rows, cols, dcnt, dscr, n_cu, st);
         });
  c.down(reinterpret_cast<u64 *>(counts), dcnt, nbins);
  if (c.go() && kernel_ms) *kernel_ms = tm.total / reps;
  return c.status();
}

int pbh_check_normals64(int device, int64_t n, const uint32_t *words,
                        double *fast, double *ref) {
  if (check_ptr(words, "words") || check_ptr(fast, "fast") || check_ptr(ref, "ref"))
    return PBH_ERR_ARG;
  if (n <= 0) return fail(PBH_ERR_ARG, "n must be positive");
  HIP_TRY(hipSetDevice(device));
  std::vector<double> tab(pbh::kBm64Doubles);
  pbh::bm64_tables(tab.data());
  Call c("pbh_check_normals64");
  uint32_t *dw = c.alloc<uint32_t>(3 * n);
  double *df = c.alloc<double>(2 * n), *dr = c.alloc<double>(2 * n);
  double *dt = c.alloc<double>(tab.size());
  c.up(dw, words, 3 * n);
  c.up(dt, tab.data(), tab.size());
  if (c.go()) c.err = pbh::launch_check_normals64(n, dw, dt, df, dr);
  c.down(fast, df, 2 * n);
  c.down(ref, dr, 2 * n);
  return c.status();
}

int pbh_bm64_tables(double *out) {
  if (check_ptr(out, "out")) return PBH_ERR_ARG;
  pbh::bm64_tables(out);
  return PBH_OK;
}

int pbh_check_normals(int device, int64_t n, const uint32_t *words,
                      double *fast, double *ref) {
  if (check_ptr(words, "words") || check_ptr(fast, "fast") || check_ptr(ref, "ref"))
    return PBH_ERR_ARG;
  if (n <= 0) return fail(PBH_ERR_ARG, "n must be positive");
  HIP_TRY(hipSetDevice(device));
  Call c("pbh_check_normals");
  uint32_t *dw = c.alloc<uint32_t>(4 * n);
  double *df = c.alloc<double>(2 * n), *dr = c.alloc<double>(2 * n);
  c.up(dw, words, 4 * n);
  if (c.go()) c.err = pbh::launch_check_normals(n, dw, df, dr);
  c.down(fast, df, 2 * n);
  c.down(ref, dr, 2 * n);
  return c.status();
}

int pbh_linreg_gibbs(int device, int64_t n_obs, const double *x_obs,
                     const double *y_obs, const double *hyper,
                     const double *vsets, int64_t n_chains,
                     int64_t chain_offset, int64_t n_steps, int64_t step0,
                     const double *init, int32_t rng_mode, uint64_t seed,
                     const double *rand, double *trace_x, double *trace_lp,
                     double *final_x, double *final_lp, int32_t reps,
                     double *kernel_ms) {
  if (check_ptr(x_obs, "x_obs") || check_ptr(y_obs, "y_obs") ||
      check_ptr(hyper, "hyper") || check_ptr(init, "init"))
    return PBH_ERR_ARG;
  if (n_obs < 1 || n_obs > pbh::linreg_max_obs())
    return fail(PBH_ERR_ARG, "n_obs must be in 1..%lld, got %lld",
                (long long)pbh::linreg_max_obs(), (long long)n_obs);
  if (n_chains < 1 || n_steps < 0 || step0 < 0 || chain_offset < 0)
    return fail(PBH_ERR_ARG, "n_chains must be >= 1 and n_steps, step0, "
                "chain_offset >= 0");
  if (rng_mode != PBH_RNG_REPLAY && rng_mode != PBH_RNG_PHILOX &&
      rng_mode != PBH_RNG_PHILOX_F64)
    return fail(PBH_ERR_UNSUPPORTED, "pbh_linreg_gibbs: rng_mode %d", rng_mode);
  if (rng_mode == PBH_RNG_REPLAY && n_steps > 0 && !rand)
    return fail(PBH_ERR_ARG, "REPLAY needs rand [n_steps][n_chains]");
  if (reps < 1) return fail(PBH_ERR_ARG, "reps must be >= 1");
  if (hyper[1] == 0. || hyper[3] == 0.)
    return fail(PBH_ERR_ARG, "prior sigmas must be non-zero");
  const double alpha_post = hyper[4] + 0.5 * (double)n_obs;
  if (!(alpha_post >= 1.))
    return fail(PBH_ERR_ARG, "y_sigma_alpha + n_obs/2 must be >= 1");
  pbh::LinregArgs h{};
  std::vector<double> sq(n_obs);
  // centred statistics for the FAST form, two passes in long double
  long double mx = 0.L, my = 0.L;
  for (int64_t j = 0; j < n_obs; ++j) {
    sq[j] = x_obs[j] * x_obs[j];
    mx += x_obs[j];
    my += y_obs[j];
  }
  mx /= (long double)n_obs;
  my /= (long double)n_obs;
  long double cxx = 0.L, cxy = 0.L, cyy = 0.L;
  for (int64_t j = 0; j < n_obs; ++j) {
    const long double dx = x_obs[j] - mx, dy = y_obs[j] - my;
    cxx += dx * dx;
    cxy += dx * dy;
    cyy += dy * dy;
  }
  h.hyper[0] = 1. / (hyper[1] * hyper[1]); h.hyper[1] = hyper[0];
  h.hyper[2] = 1. / (hyper[3] * hyper[3]); h.hyper[3] = hyper[2];
  h.hyper[4] = alpha_post; h.hyper[5] = hyper[5];
  h.hyper[6] = np_pairwise_host(sq.data(), n_obs);
  for (int k = 0; k < 3; ++k) {
    if (vsets) {
      if (!(vsets[2 * k] < vsets[2 * k + 1]))
        return fail(PBH_ERR_ARG, "vsets[%d] must have lo < hi", k);
      h.hyper[7 + k] = -std::log(vsets[2 * k + 1] - vsets[2 * k]);
      h.bounds[2 * k] = vsets[2 * k];
      h.bounds[2 * k + 1] = vsets[2 * k + 1];
    } else {            // joint=False: no prior terms (lp + 0.0 == lp)
      h.hyper[7 + k] = 0.;
      h.bounds[2 * k] = -HUGE_VAL;
      h.bounds[2 * k + 1] = HUGE_VAL;
    }
  }
  h.hyper[10] = std::log(std::sqrt(2. * M_PI));
  h.stats[0] = (double)mx; h.stats[1] = (double)my; h.stats[2] = (double)cxx;
  h.stats[3] = (double)cxy; h.stats[4] = (double)cyy;
  h.n_obs = n_obs; h.n = n_chains; h.chain_offset = chain_offset;
  h.n_steps = n_steps; h.step0 = step0; h.seed = seed; h.mode = rng_mode;
  if (kernel_ms) *kernel_ms = 0.;
  HIP_TRY(hipSetDevice(device));
  const int64_t T = n_steps, N = n_chains;
  Call c("pbh_linreg_gibbs");
  double *dxo = c.alloc<double>(n_obs), *dyo = c.alloc<double>(n_obs);
  double *dinit = c.alloc<double>(3 * N), *dstate = c.alloc<double>(3 * N);
  double *dlp = c.alloc<double>(N);
  double *drand = rng_mode == PBH_RNG_REPLAY && T > 0 ? c.alloc<double>(T * N) : nullptr;
  double *dtx = T > 0 && trace_x ? c.alloc<double>(T * 3 * N) : nullptr;
  double *dtp = T > 0 && trace_lp ? c.alloc<double>(T * N) : nullptr;
  Timed tm(c);
  c.up(dxo, x_obs, n_obs);
  c.up(dyo, y_obs, n_obs);
  c.up(dinit, init, 3 * N);
  if (drand) c.up(drand, rand, T * N);
  h.x_obs = dxo; h.y_obs = dyo; h.state = dstate; h.lp_state = dlp;
  h.rand = drand; h.tx = dtx; h.tp = dtp;
  // the warm-up launch is made only when timing several repetitions (a
  // single run is the sampler's own)
  if (T > 0)
    tm.run(c, reps > 1 ? 0 : 1, reps,
           [&](hipStream_t st) {
             return hipMemcpyAsync(dstate, dinit, 3 * N * 8, hipMemcpyDeviceToDevice, st);
           },
           [&](hipStream_t st) { return pbh::launch_linreg_gibbs(h, st); });
  if (trace_x && T > 0) c.down(trace_x, dtx, T * 3 * N);
  if (trace_lp && T > 0) c.down(trace_lp, dtp, T * N);
  if (final_x) c.down(final_x, T > 0 ? dstate : dinit, 3 * N);
  if (final_lp && T > 0) c.down(final_lp, dlp, N);
  if (c.go() && kernel_ms) *kernel_ms = tm.total / reps;
  return c.status();
}

}  // extern "C"
