// pbh_engine_state.h -- what the units behind the C-ABI of include/pbhip.h
// share (pbh_engine.hip, pbh_trace.cpp, pbh_oneshot.cpp): the engine's state,
// the error plumbing, device memory through the resource cache, the two
// waits, and the host transposes between the caller's chain rows and the
// device's dim-major arrays.  Internal: nothing here is part of the ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <chrono>
#include <vector>

#include "../../include/pbhip.h"
#include "pbh_kernels.h"

struct pbh_engine {
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  unsigned ev_flags = 0;   // the events' hipEventCreateWithFlags flags
  // model / proposal / gibbs (device constant blocks)
  bool has_model = false, has_prop = false, has_gibbs = false;
  int d = 0;
  pbh::KArgs k{};
  double *dmodel = nullptr, *dprop = nullptr, *dgibbs = nullptr;
  std::vector<int32_t> draw_order;  // GAUSS: dim receiving the j-th draw
  // chains
  int64_t n = 0, off = 0;
  double *x = nullptr, *lp = nullptr;
  bool has_pred = false;
  int64_t g = 0;  // chain-steps done since pbh_init_chains
  // randomness
  int32_t rng = PBH_RNG_PHILOX;
  uint64_t seed = 0;
  double *rep = nullptr;
  int64_t rep_steps = 0, rep_g0 = 0;
  size_t rep_alloc = 0;          // doubles allocated at rep (device streams reuse it)
  uint32_t *xo = nullptr;      // xoshiro128** states [4][2][n]
  bool xo_seeded = false;
  // legacy NumPy RandomState per chain (pbh_legacy_seed)
  uint32_t *mt_key = nullptr;
  bool mt_k4 = true;           // mt_key layout: Mt4's [16][20][n][32] (chunked blocks),
                               // or the double-buffered [2][624][n] (Mt3)
  bool legacy_k4 = true;       // PBH_LEGACY_K4=0: the double-buffered state at any chain count
  bool legacy_fused = true;    // PBH_LEGACY_FUSED=0: pbh_legacy_run as generation + run
  bool legacy_wp = true;       // PBH_LEGACY_WP=0: the chain-per-lane generator for MH streams
  bool legacy_ahead = true;    // PBH_LEGACY_AHEAD=0: no twist-ahead pass before fused launches
  bool mt_odd = false;         // a stream may sit at an odd word (randint drew single words)
  bool rec_thr = false;        // pbh_set_record_threshold: keep pbh_legacy_run's thresholds
  double *thr = nullptr;       // [thr_steps][n] thresholds of the last pbh_legacy_run
  double *ess_tot = nullptr;   // pbh_trace_ess_total's per-dim sums (PBH_MAX_DIM)
  size_t thr_alloc = 0;
  int64_t thr_steps = 0;
  int32_t *mt_pos = nullptr, *mt_has = nullptr, *mt_order = nullptr;
  double *mt_gauss = nullptr;
  bool mt_stale = false;       // pbh_restore ran: the streams wait for
                               // pbh_set_legacy_state (the checkpoint's)
  // trace
  int64_t cap = 0;
  int32_t thin = 1, debug = 0;
  int64_t rec_base = 0;
  double *tx = nullptr, *tlp = nullptr, *tpx = nullptr, *tpp = nullptr,
         *ts = nullptr;
  uint64_t *tacc = nullptr;
  // moments (pbh_set_collect)
  int32_t collect = PBH_COLLECT_MOMENTS;
  double *msum = nullptr, *msq = nullptr;
  int64_t *nacc = nullptr;
  int64_t mom_steps = 0;
  // production fp64 normal tables (bm64, pbh_device.h), read into LDS
  double *bm64 = nullptr;
  double *lgtab = nullptr;     // legacy_log_table (device legacy streams)
  double *ess = nullptr;     // [d][n] per-chain ESS (pbh_trace_ess), NaN before
  int32_t *ess_list = nullptr;   // the 2 048-point ESS form's fallback list
  size_t ess_list_len = 0;
  double *stage = nullptr;       // pinned staging of doubles: the ESS copy-out, and
  size_t stage_len = 0;          // the selected quantiles the rank reductions upload
  // The one scratch of the trace reductions (expectation, quantile, R-hat,
  // pooled quantile), grown on demand and kept between calls.  Each call
  // writes all it reads and has copied its result out when it returns, so
  // the next one may find anything here.
  unsigned char *scratch = nullptr;
  size_t scratch_bytes = 0;
  bool spin_sync = true;     // poll <= 2 ms, then block; PBH_SYNC=block: block
  bool sync_event = false;   // PBH_SYNC=event: poll the last run's end event
  // timing events as marker packets around the launches (default), or
  // PBH_EVENT_MARKERS=0: on the first / last dispatch packet
  // (hipExtLaunchKernel: 2 us less GPU time, 3-4 us more host enqueue and
  // ~7 us more wall per short launch, measured: profiles/r02j_events.jsonl)
  bool gmm_full = true;      // PBH_GMM_FULL=0: no steady-state quad kernel
  bool pair_full = true;     // PBH_PAIR_FULL=0: no steady-state pair kernel
  int ess_fft = 2;           // PBH_ESS_FFT=1: the 4 096-point form only, 0: direct sums
  bool iid_full = true;      // PBH_IID_FULL=0: no steady-state iid kernel
  int fair = 11;             // PBH_FAIR=k: wave priorities alternate every 2^k x 10 ns (0: off)
  int pair_wg = 512;         // PBH_PAIR_WG=256: FULL pair kernel in 4-wave workgroups
                             // (512: one table copy per CU, 20-step launches ~5 % faster)
  // Launches of <= 64 steps (the driver's 20-step shape): the alternation
  // clock starts at each wave's loop entry and hands over once, half-way
  // (2^10 ticks = 10.24 us for 20 steps) -- the
  // free-running clock put the one hand-over anywhere in the launch or nowhere
  // (profiles/r04f_phase.jsonl: the last wave ends 26.4-29.2 us into a k11
  // launch, 26.5-26.6 us with the launch-relative clock)
  int fair_short = 10;       // PBH_FAIR_SHORT=k
  int fair_rel = 0;          // PBH_FAIR_REL=1: long launches use the relative clock too
  bool event_markers = true;
  bool pair_enabled = true;  // PBH_NO_PAIR=1 disables the lane-pair kernel
  bool gibbs_mfma = true;    // PBH_GIBBS_MFMA=0 keeps the VALU quadratic form
  bool gibbs_fast = true;    // PBH_GIBBS_FAST=0 keeps the ndtri kernel for Philox
  int gibbs_lanes = 0;       // PBH_GIBBS_LANES: lanes per chain of that kernel
  int gmm_lanes = 4;         // PBH_GMM_LANES: lanes per chain of the GMM kernel
  // MVN target on the host (for the production Gibbs tables)
  std::vector<double> mvn_mean, mvn_U;
  double mvn_const = 0.;
  // production Gibbs: persisted g = P'(x - mu'), Q per chain
  double *gq = nullptr;
  // production ufun logs carried as chain state ([d][n], KArgs.lx)
  double *lx = nullptr;
  bool lx_valid = false;
  bool gq_valid = false;
  // timing of the last pbh_run
  bool timed = false;
  int64_t last_launches = 0;
  // resident sampling server (PBH_SERVER=1; pbh_server_*): the FULL pair
  // kernel launched once, each eligible pbh_run a command in pinned host
  // memory; srv_timed: the last run was a command (timed by its stamps)
  bool srv_enabled = false;
  bool srv_active = false;
  bool srv_timed = false;
  uint32_t srv_seq = 0, srv_pending = 0;
  int32_t srv_wgs = 0;
  int64_t srv_idle_ms = 1000;      // PBH_SERVER_IDLE_MS: the kernel's idle exit
  pbh::SrvCmd *srv_cmd = nullptr;  // pinned, fine-grained
  pbh::SrvDone *srv_done = nullptr;
  pbh::SrvCmd *srv_mail = nullptr;   // the device mailbox the workgroups poll
  int32_t srv_done_len = 0;
  // the command protocol (KArgs.srv_mode): 1 direct (the default) --
  // srv_mail is fine-grained device memory the host writes through srv_wmail
  // (its host mapping) and every workgroup polls; 0 relay -- workgroup 0
  // polls the pinned host block srv_cmd and copies each command into
  // srv_mail.  Direct needs a host mapping whose stores the device sees: the
  // first launch probes it (srv_probed) and falls back to the relay.
  int32_t srv_mode = 1;
  bool srv_probed = false;
  bool srv_mail_fine = false;        // srv_mail came from the fine-grained pool
  pbh::SrvCmd *srv_wmail = nullptr;
  // srv_last: the last submit (or launch) -- never moved forward at a wait:
  // a command completes after its submit, and each workgroup's idle timer
  // starts at its completion, so idle measured from the submit is an upper
  // bound on the kernel's own
  std::chrono::steady_clock::time_point srv_last{};
  // a server command was lost (the kernel ended or hung before completing
  // it): the chain state may be partly advanced, so runs refuse until
  // pbh_init_chains / pbh_restore / pbh_set_chains replace it
  bool state_lost = false;
  int64_t srv_commands = 0, srv_launches = 0;
  // RCCL
  ncclComm_t comm = nullptr;
  int32_t rank = 0, world = 1;
  double *gather_send = nullptr, *gather_recv = nullptr, *scalar = nullptr;
};

namespace pbh {

// Sets the calling thread's pbh_last_error text and returns code.
int fail(int code, const char *fmt, ...);

inline int check_ptr(const void *p, const char *name) {
  return p ? PBH_OK : fail(PBH_ERR_ARG, "%s must not be NULL", name);
}

#define HIP_TRY(expr)                                                        \
  do {                                                                       \
    hipError_t _e = (expr);                                                  \
    if (_e != hipSuccess)                                                    \
      return pbh::fail(PBH_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e)); \
  } while (0)

// Device memory through the engine resource cache (pbh_engine.hip).  Every
// form first lets go of what *p holds and leaves it null: Free and Alloc to the
// runtime, Retire into the cache while it fits (a destroyed engine's buffer,
// its stream drained).  Alloc then takes `bytes` from the cache or the runtime.
enum class DMem { Alloc, Free, Retire };
int dmem(DMem op, void **p, size_t bytes = 0);

template <class T>
int dalloc(T *&p, size_t count) { return dmem(DMem::Alloc, (void **)&p, count * sizeof(T)); }
template <class T>
void dfree(T *&p) { (void)dmem(DMem::Free, (void **)&p); }
template <class T>
void dretire(T *&p) { (void)dmem(DMem::Retire, (void **)&p); }
// A buffer of at least `need` elements (len: what p holds), reallocated when
// it is smaller; what it held is not kept.
template <class T>
int dgrow(T *&p, size_t &len, size_t need) {
  if (len >= need) return PBH_OK;
  len = 0;
  if (const int rc = dalloc(p, need)) return rc;
  len = need;
  return PBH_OK;
}

// The caller's rows [n][d] (one chain or point after another) -> the device's
// dim-major [d][n], and back; on the host.
inline void rows_to_dim_major(const double *rows, double *dm, int64_t n, int64_t d) {
  for (int64_t c = 0; c < n; ++c)
    for (int64_t k = 0; k < d; ++k) dm[(size_t)k * n + c] = rows[(size_t)c * d + k];
}
inline void dim_major_to_rows(const double *dm, double *rows, int64_t n, int64_t d) {
  for (int64_t c = 0; c < n; ++c)
    for (int64_t k = 0; k < d; ++k) rows[(size_t)c * d + k] = dm[(size_t)k * n + c];
}

// PBH_EXPR_DATA_WIDE (pbh_oneshot.cpp): KArgs.ewide of pbh_set_model and of
// the one-shot expression evaluator; not among the library's exported names
__attribute__((visibility("hidden"))) int32_t expr_data_wide();

// Ends the resident sampling server (pbh_engine.hip).  Every entry point that
// touches the device state, the trace or the stream stops it first.
int srv_stop(pbh_engine *e);

#define SRV_STOP(e)                         \
  do {                                      \
    if ((e)->srv_active) {                  \
      const int srv_rc_ = pbh::srv_stop(e); \
      if (srv_rc_) return srv_rc_;          \
    }                                       \
  } while (0)

// The engine stream's completion, as pbh_sync waits for it: polled for up to
// 2 ms (PBH_SYNC, spin_sync), then a blocking wait.  A blocking
// hipStreamSynchronize wakes ~10-50 us after a short kernel ends.
inline hipError_t stream_wait(pbh_engine *e) {
  if (!e->spin_sync) return hipStreamSynchronize(e->stream);
  const auto t0 = std::chrono::steady_clock::now();
  hipError_t q;
  while ((q = hipStreamQuery(e->stream)) == hipErrorNotReady) {
    if (std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(2000))
      return hipStreamSynchronize(e->stream);
  }
  return q;
}

}  // namespace pbh
