/*
 * pbhip.h -- C-ABI of libpbhip.so, the MI355X (gfx950) batched
 * Metropolis-Hastings / CondCov-Gibbs engine behind probayes_amd.
 *
 * The reference (probayes 0.0.8) has no C/FFI layer: its boundary is the pure
 * Python SP API.  Each entry point below replaces one piece of the per-chain
 * Python call stack of SP.next (sp.py:221-258) for N chains at once; the
 * reference interface it stands in for is cited beside it.  Bindings: the
 * ctypes stub in probayes_amd/_lib.py (and INTEGRATION.md).
 *
 * Conventions
 *  - Every function returns int status: 0 = PBH_OK, < 0 = error; the message
 *    is in pbh_last_error() (thread-local).  No function throws or aborts.
 *  - Host buffers are caller-allocated; the engine owns every device buffer.
 *  - One engine per device, calls on one engine must not be concurrent.
 *    Multi-GPU = one process (or thread) per device + pbh_rccl_*.
 *  - Chain-major arrays on the host are [chain][dim]; device and trace arrays
 *    are dim-major with the chain index fastest ([step][dim][chain]).
 *  - All arithmetic is IEEE fp64 (constants.py:7 DEFAULT_FP_PRECISION = 64).
 */
#ifndef PBHIP_H
#define PBHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PBH_ABI_VERSION 7
/* Additions that leave every version-7 call and struct prefix as it was bump
 * the revision: 1 = pbh_model.expr_data / expr_n_obs / expr_n_cols (a caller
 * passes the whole struct, zero-initialised), pbh_eval_expr_data;
 * 2 = pbh_trace_quantile.  pbh_trace_rhat, pbh_trace_quantile_pooled,
 * pbh_trace_rhat_rank and pbh_trace_ess_rank were added within revision 2
 * without a bump: a caller finds them by looking the symbol up.             */
#define PBH_ABI_REVISION 2
#define PBH_MAX_DIM 32

#define PBH_OK 0
#define PBH_ERR_ARG (-1)
#define PBH_ERR_HIP (-2)
#define PBH_ERR_STATE (-3)
#define PBH_ERR_UNSUPPORTED (-4)
#define PBH_ERR_RCCL (-5)

/* Joint density forms the engine lowers. */
enum pbh_target_kind {
  PBH_TARGET_DIAG_GAUSS = 1,  /* sum_i norm.logpdf(x_i, mu_i, sigma_i)        */
  PBH_TARGET_NORM_IID = 2,    /* np.sum(norm.logpdf(obs, x[loc], x[scale]))   */
  PBH_TARGET_GMM = 3,         /* logsumexp_k(logw_k + sum_i logpdf(x_i,mu_ki,sd_k)) */
  PBH_TARGET_NORM_PDF = 4,    /* prod_i norm.pdf(x_i, loc_i, scale_i)          */
  PBH_TARGET_UNIFORM_PDF = 5, /* prod_i uniform.pdf(x_i, lo_i, scale_i)        */
  PBH_TARGET_MVN = 6,         /* multivariate_normal.pdf at the permuted x     */
  PBH_TARGET_EXPR = 7         /* a scalar expression of x as a program the
                                 kernels interpret (pbh_model.expr_*)          */
};
/* PBH_TARGET_EXPR: the program.  One instruction per code word, one result
 * per instruction; the previous instruction's result is the accumulator, and
 * an instruction with the store bit also writes its result to slot dst.
 *   word = op | dst << 6 | store << 10 | akind << 11 | aidx << 13
 *             | bkind << 21 | bidx << 23        (bit 31 clear)
 * Operand kinds: 0 slot, 1 variable x[idx], 2 constant, 3 accumulator.  The
 * density is the accumulator after the last instruction.  IEEE fp64; MAX /
 * MIN propagate NaN as np.maximum / np.minimum do; POW is pow(a, b).       */
/* Loop regions (a program with data, pbh_model.expr_data): all data columns
 * have one length n; a value that depends on one is summed over the n
 * observations by a non-nested region
 *   LOOP | len << 13,  len body words,  SUM | dst << 6 | store << 10 | 3 << 11
 * whose body runs once per observation j with an accumulator of its own, and
 * whose SUM word leaves the sum of the body's last value over j in the
 * accumulator (and in slot dst).  In a body a variable index >= 16 is data
 * column idx - 16 at observation j, a slot index >= 16 is body temporary
 * idx - 16 (PBH_EXPR_MAX_TEMPS of them), a slot index < 16 reads an outer
 * slot, and the store field names a body temporary.  The sum is NumPy's 1-D
 * pairwise sum in every RNG mode: sequential below 8 terms, eight
 * accumulators per block up to 128, halving (to a multiple of 8) above.      */
enum pbh_expr_op {
  PBH_EXPR_MOV = 0, PBH_EXPR_ADD = 1, PBH_EXPR_SUB = 2, PBH_EXPR_MUL = 3,
  PBH_EXPR_DIV = 4, PBH_EXPR_NEG = 5, PBH_EXPR_ABS = 6, PBH_EXPR_SQRT = 7,
  PBH_EXPR_EXP = 8, PBH_EXPR_LOG = 9, PBH_EXPR_LOG1P = 10, PBH_EXPR_EXPM1 = 11,
  PBH_EXPR_MAX = 12, PBH_EXPR_MIN = 13, PBH_EXPR_POW = 14, PBH_EXPR_N_OPS = 15,
  /* region markers, outside the elementwise opcodes 0..N_OPS-1 */
  PBH_EXPR_LOOP = 32, PBH_EXPR_SUM = 33
};
enum pbh_expr_operand {
  PBH_EXPR_SLOT = 0, PBH_EXPR_VAR = 1, PBH_EXPR_CONST = 2, PBH_EXPR_ACC = 3
};
#define PBH_EXPR_MAX_CODE 256
#define PBH_EXPR_MAX_CONSTS 128
#define PBH_EXPR_MAX_SLOTS 16
#define PBH_EXPR_MAX_DIM 16
#define PBH_EXPR_BODY_BASE 16   /* body: data column / temporary indices from here */
#define PBH_EXPR_MAX_COLS 8
#define PBH_EXPR_MAX_TEMPS 4
#define PBH_EXPR_MAX_OBS 65536
enum pbh_pscale { PBH_PSCALE_LOG = 0, PBH_PSCALE_LIN = 1 };
enum pbh_scores {
  PBH_SCORES_HASTINGS = 1, PBH_SCORES_METROPOLIS = 2, PBH_SCORES_GIBBS = 3
};
enum pbh_tran_kind { PBH_TRAN_CONST = 1, PBH_TRAN_GAUSS_PDF = 2 };
enum pbh_proposal_kind {
  PBH_PROP_GAUSS = 1,   /* callable Delta(norm.rvs(loc, scale)) per dim        */
  PBH_PROP_SPHERE = 2,  /* tuple delta, field.py:509-531                      */
  PBH_PROP_UNIFORM = 3, /* list delta, variable.py:625-633                    */
  PBH_PROP_GIBBS = 4,   /* CondCov conditional draw, cond_cov.py:42-65        */
  PBH_PROP_VARDELTA = 5 /* per-variable deltas (a Delta of containers, or a
                           bare scalar Field delta): field.py:266-306,
                           variable.py:600-640                                */
};
/* Per-variable delta modes of PBH_PROP_VARDELTA (Variable.eval_delta,
 * variable.py:618-633).  Replay streams hold, per variable, the raw uniform
 * (POLARITY, UNIFORM), the randint value (RANDINT) or nothing (FIXED).     */
enum pbh_var_delta {
  PBH_VAR_FIXED = 0,     /* bare scalar: x + delta                             */
  PBH_VAR_POLARITY = 1,  /* (delta,): +delta if uniform() > 0.5 else -delta    */
  PBH_VAR_UNIFORM = 2,   /* [delta]: uniform(-delta, delta)                    */
  PBH_VAR_RANDINT = 3    /* [delta] of an int variable: randint(-delta, delta),
                            bounds truncated toward zero as NumPy does         */
};
enum pbh_rng_mode {
  PBH_RNG_REPLAY = 0,    /* randoms read from a caller-supplied [T][R][N]
                            stream; reference arithmetic (parity mode)        */
  PBH_RNG_PHILOX = 1,    /* production: Philox-4x32-10 keyed by (seed, global
                            chain id); fp64 Box-Muller normals on 52-bit
                            uniforms (table-driven log / sqrt / sincos, a few
                            ulp from libm), fp64 chain arithmetic in the
                            production (FMA) forms                            */
  PBH_RNG_PHILOX_F64 = 2, /* Philox-4x32-10 with libm fp64 Box-Muller normals
                            and the reference arithmetic of REPLAY             */
  PBH_RNG_XOSHIRO = 3,   /* production: one xoshiro128** stream per chain (per
                            lane half), seeded by SplitMix64 of (seed, global
                            chain id); otherwise as PHILOX                    */
  PBH_RNG_PHILOX_FP32 = 4 /* comparison only (the round-1 production form):
                            as PHILOX but fp32 hardware Box-Muller normals on
                            24-bit uniforms (|z| <= 5.77) with exact sign
                            symmetry; lane-pair diagonal-Gauss kernel only   */
};
/* What pbh_run accumulates besides the trace (pbh_set_collect). */
enum pbh_collect {
  PBH_COLLECT_MOMENTS = 1   /* per-chain sum / sumsq / n_acc (pbh_get_moments) */
};

/* Joint density + acceptance (replaces RF.set_prob/set_tran + SP.set_scores:
 * rf.py:91,169; sp.py:57-100; prob.py:331-380; rf_utils.py:10-42).
 * All pointers are host pointers, copied into device memory by the call.   */
typedef struct pbh_model {
  int32_t dim;          /* d, 1..PBH_MAX_DIM                                  */
  int32_t target_kind;  /* enum pbh_target_kind                               */
  int32_t pscale;       /* enum pbh_pscale of the density (pscales.py:21-41)   */
  int32_t scores;       /* enum pbh_scores (sp_utils.py:87-91)                */
  /* target parameters (meaning per kind):
   *   DIAG_GAUSS : a = mu[d], b = sigma[d], c = log(sigma)[d], e = 1/sigma[d]
   *   NORM_IID   : a = obs[n], n = n_obs, i0 = loc dim, i1 = scale dim
   *   GMM        : a = logw[K], b = mu[K*d], c = sd[K], e = log(sd)[K], n = K
   *   NORM_PDF   : a = loc[d], b = scale[d]
   *   UNIFORM_PDF: a = lo[d], b = scale[d]
   *   MVN        : a = mean[d], b = whitening U[d*d] row-major (scipy
   *                CovViaPSD._LP), c = {rank*log(2pi) + log_pdet}; the density
   *                is taken at x[perm] with prob.py:354-357's fixed perm
   *   EXPR       : none of them; the expr_* fields at the end of the struct */
  const double *a, *b, *c, *e;
  const int32_t *perm;
  int64_t n;
  int32_t i0, i1;
  /* joint=True uniform root prior (rv_utils.py:8-47); has_prior = 0/1 */
  int32_t has_prior;
  const double *prior_lo, *prior_hi;
  const int32_t *prior_lo_incl, *prior_hi_incl;
  double prior_logp;
  /* per-dim change of variable: 1 = (log, exp) ufun (variable.py:693-697) */
  const int32_t *ufun;
  /* transition q(x'|x) (rf.py:169-239, 490-538) */
  int32_t tran_kind;    /* enum pbh_tran_kind                                 */
  int32_t tran_sym;     /* 1 = symmetric (r = None), 0 = tuple tran           */
  double tran_value;    /* CONST: value of q                                  */
  double tran_scale;    /* GAUSS_PDF: sigma                                   */
  const double *tran_offset;  /* GAUSS_PDF: loc offset per dim               */
  const int32_t *tran_order;  /* GAUSS_PDF: multiplication order of dims     */
  /* PBH_TARGET_EXPR (dim <= PBH_EXPR_MAX_DIM): the program, checked by
   * pbh_set_model before any launch -- every opcode, every variable /
   * constant / slot index, that a slot or the accumulator is read only after
   * it was written, and the limits above; PBH_ERR_ARG otherwise.            */
  const int32_t *expr_code;   /* expr_n_code words, 1..PBH_EXPR_MAX_CODE      */
  int32_t expr_n_code;
  const double *expr_consts;  /* expr_n_consts values, 0..PBH_EXPR_MAX_CONSTS */
  int32_t expr_n_consts;
  int32_t expr_depth;         /* slots the program writes, 0..PBH_EXPR_MAX_SLOTS */
  /* a program with loop regions: expr_data[expr_n_cols][expr_n_obs], copied
   * to the device with the program (NULL / 0 / 0: a program without regions).
   * Checked with the program: region bounds, no nesting, column and temporary
   * indices, a temporary read only after the body wrote it, the accumulator
   * not read by a body's first word, no outer slot written inside a body,
   * 1 <= expr_n_cols <= PBH_EXPR_MAX_COLS, 1 <= expr_n_obs <= PBH_EXPR_MAX_OBS. */
  const double *expr_data;
  int32_t expr_n_obs;
  int32_t expr_n_cols;
} pbh_model;

/* Proposal (replaces RF.set_delta / Field.eval_delta / apply_delta:
 * field.py:220-317, 469-552; variable.py:600-739).                         */
typedef struct pbh_proposal {
  int32_t kind;             /* enum pbh_proposal_kind (not GIBBS)            */
  const double *loc;        /* GAUSS: loc[d]                                  */
  const double *scale;      /* GAUSS: scale[d]                                */
  const int32_t *order;     /* GAUSS: dim receiving the j-th draw             */
  double delta;             /* SPHERE: delta (already * rss if scale=True)    */
  const double *lengths;    /* SPHERE: per-dim multiplier (lengths or 1)      */
  const double *delta_vec;  /* UNIFORM: delta[d]                              */
  /* Optional covariance-matrix random walk (any kind): the base delta is
   * multiplied by tfun[d*d] (row-major), i.e. delta' = tfun . delta, as
   * RF.eval_delta does with the Cholesky factor that RF.set_tran(ndarray)
   * installs (rf.py:210-220, 340-354).  NULL = no tfun.                    */
  const double *tfun;
  /* VARDELTA: var_mode[d] (enum pbh_var_delta); the steps are delta_vec[d] */
  const int32_t *var_mode;
  /* Optional, any MH kind.  var_int[d] = 1: an int variable, whose proposed
   * value is truncated toward zero (revtype, variable.py:697).  NULL = none. */
  const int32_t *var_int;
  /* Optional, any MH kind: bound=True (variable.py:700-739), per dim
   * bound_on[d]; limits bound_lo[d] <= bound_hi[d] (the vset limits) and
   * which are exclusive (bound_xlo[d], bound_xhi[d]).  With both limits
   * closed the proposal is clamped; an exclusive side it crosses returns the
   * predecessor value (both exclusive: anything outside (lo, hi); one
   * exclusive: strictly beyond it), the other side is clamped.  NULL = none. */
  const int32_t *bound_on;
  const double *bound_lo, *bound_hi;
  const int32_t *bound_xlo, *bound_xhi;
} pbh_proposal;

/* CondCov Gibbs tables (replaces CondCov.__init__ + RF.eval_tfun cycling:
 * cond_cov.py:22-39, rf.py:446-458).  Precomputed on the host like the
 * reference does (np.linalg.inv, norm.cdf).                                  */
typedef struct pbh_gibbs {
  const double *mean;   /* mu[d]                                             */
  const double *coef;   /* coef[d*(d-1)]: row i = Sigma_{i,-i} Sigma_{-i,-i}^-1 */
  const double *stdv;   /* conditional sd[d]                                 */
  const double *cdf;    /* cdf limits [d*2] (lo, hi)                         */
  int32_t tsteps;       /* coordinates per SP step (rf.py:446-452)            */
} pbh_gibbs;

typedef struct pbh_engine pbh_engine;

/* ---- engine lifetime ---------------------------------------------------- */
const char *pbh_last_error(void);
int pbh_abi_version(void);
int pbh_abi_revision(void);   /* PBH_ABI_REVISION */
int pbh_device_count(int *count);
int pbh_create(int device, pbh_engine **out);
/* Destroys the engine.  Its device buffers, stream and events (drained) stay
 * in a process-wide cache for the next engine of the same device (one
 * engine per SP.sampler call); PBH_CACHE_MB bounds the cached buffers
 * (default 32 768, 0: no cache).                                            */
int pbh_destroy(pbh_engine *eng);
/* Frees every cached buffer and stream (an allocation that fails does this
 * itself and retries).                                                       */
int pbh_cache_release(void);
/* Cached (idle) bytes, and allocations served from / missed in the cache.  */
int pbh_cache_info(int64_t *idle_bytes, int64_t *hits, int64_t *misses);

/* ---- model ------------------------------------------------------------- */
int pbh_set_model(pbh_engine *eng, const pbh_model *model);
int pbh_set_proposal(pbh_engine *eng, const pbh_proposal *prop);
int pbh_set_gibbs(pbh_engine *eng, const pbh_gibbs *gibbs);

/* ---- chains and randomness (SP.sampler(init, ...): sp.py:261-278) ------- */
/* Allocates chain state for chains [chain_offset, chain_offset + n) and copies
 * init [n][d]; the first pbh_run step proposes from init and auto-accepts
 * (sp_utils.py:24-25, App. A-3).                                            */
int pbh_init_chains(pbh_engine *eng, int64_t n_chains, int64_t chain_offset,
                    const double *init);
/* Global step index of the first pbh_run step (default 0): the phase of the
 * CondCov coordinate cycle, which the reference keeps per RF across samplers
 * (RF.__cond_mod, rf.py:446-452), and the Philox step counter.  Only right
 * after pbh_init_chains.                                                     */
int pbh_set_step(pbh_engine *eng, int64_t step);
int pbh_set_rng(pbh_engine *eng, int32_t mode, uint64_t seed);
/* Checkpoint / resume: everything a chain needs to continue
 * exactly -- state x [N][d] and its prob lp [N], the global step index
 * (Philox counter, CondCov cycle phase), whether step 1 is behind (the
 * auto-accept, sp.py:231-232), and for XOSHIRO the per-chain generator
 * state [8][N] (NULL otherwise).  pbh_restore goes after pbh_init_chains
 * (same N) and pbh_set_rng; it detaches a trace buffer and replay rows
 * (pbh_alloc_trace again); a run from the restored engine continues the
 * checkpointed one step for step.  The production Gibbs
 * kernel's persisted g, Q are recomputed from x (v.prob then agrees to its
 * refresh tolerance, 1e-9).                                                 */
int pbh_get_checkpoint(pbh_engine *eng, double *x, double *lp, int64_t *step,
                       int32_t *has_pred, uint32_t *xo);
int pbh_restore(pbh_engine *eng, const double *x, const double *lp,
                int64_t step, int32_t has_pred, const uint32_t *xo);
/* The device legacy streams' state for a checkpoint (pbh_legacy_seed):
 * key [words][N] with words per chain from pbh_legacy_state_words (1248
 * double-buffered, 640 for the default chunked layout: the
 * current block, moved into buffer 0 by the get; the words are the device
 * layout, opaque to the caller and valid only for an engine seeded with the
 * same layout), the read position pos [N]
 * (packed with the layout's buffer indices), the cached-gauss flag
 * has [N] and value gauss [N] (NumPy's RandomState has_gauss / gauss).
 * After pbh_restore on an engine with legacy streams, pbh_legacy_replay
 * refuses until pbh_set_legacy_state restores the checkpoint's state.       */
int pbh_legacy_state_words(pbh_engine *eng, int64_t *words_per_chain);
int pbh_get_legacy_state(pbh_engine *eng, uint32_t *key, int32_t *pos,
                         int32_t *has, double *gauss);
int pbh_set_legacy_state(pbh_engine *eng, const uint32_t *key,
                         const int32_t *pos, const int32_t *has,
                         const double *gauss);
/* Replaces the chains' state (x [N][d], lp [N]), the global step and the
 * step-1 flag at any point; every generator state (xoshiro, legacy streams)
 * continues where it is.  The trace buffer and the replay rows are
 * detached: pbh_alloc_trace / pbh_upload_replay / pbh_legacy_replay again
 * before pbh_run.  Used by the SP facade's incremental samplers (SP.reset,
 * sp.py:113-128) to restart chains at init or to rewind to the last step
 * handed out.                                                               */
int pbh_set_chains(pbh_engine *eng, const double *x, const double *lp,
                   int64_t step, int32_t has_pred);
/* The carried logs of the ufun dims (production modes: the log of a ufun
 * dim is chain state, the accepted proposal's log x + delta, variable.py:
 * 693-697 without the round trip through exp): lx [N][d] row-major (the
 * non-ufun columns unused); valid = 0 when they are not maintained (another
 * RNG mode, or a fresh / restored state: then ln x at the next launch).  A
 * checkpoint of a production ufun model carries them so that a restored
 * engine continues the run bit for bit.                                    */
int pbh_get_chain_logs(pbh_engine *eng, double *lx, int32_t *valid);
int pbh_set_chain_logs(pbh_engine *eng, const double *lx);
/* Replay stream [n_steps][R][n_chains] (R = d + 1 for MH, 1 for Gibbs),
 * consumed from the next pbh_run step on.                                   */
int pbh_upload_replay(pbh_engine *eng, int64_t n_steps, const double *rand);
int pbh_stream_width(pbh_engine *eng, int32_t *r);
/* The same streams generated on the device: one NumPy legacy RandomState per
 * chain (MT19937 seeded as RandomState(seeds[c]), random_sample, polar
 * legacy gauss with its cached deviate), drawn in the reference's per-step
 * order.  pbh_legacy_seed seeds the engine's chains;
 * each pbh_legacy_replay fills the replay stream with the next n_steps rows
 * of every chain's generator (continuing where the last call stopped) for
 * the runs from the current step on.  pbh_get_replay copies steps [first,
 * first + n_steps) of the current stream back: draw < 0 gives every draw in
 * the pbh_upload_replay layout [n][R][N], draw = j only draw j, [n][N].   */
int pbh_legacy_seed(pbh_engine *eng, const uint32_t *seeds);
int pbh_legacy_replay(pbh_engine *eng, int64_t n_steps);
/* Sizes the replay stream buffer for n_steps rows without drawing (the
 * buffer only grows; a later generation or upload of at most that many rows
 * allocates nothing).  Rows already in the buffer are dropped when it grows:
 * reserve before filling it.                                               */
int pbh_reserve_replay(pbh_engine *eng, int64_t n_steps);
int pbh_get_replay(pbh_engine *eng, int64_t first, int64_t n_steps,
                   int32_t draw, double *out);
/* pbh_legacy_replay(n) followed by pbh_run(n), in one kernel per launch:
 * each step's draws are generated into the step's registers and never
 * written to HBM.  The chains, trace, moments and legacy generator state are
 * those of generation + run chunk by chunk (steps_per_launch as pbh_run);
 * forms the fused kernel does not cover (Gibbs, per-variable deltas, a
 * permuted draw order, a d without an instantiation) run that way.  REPLAY
 * RNG, after pbh_legacy_seed.  No replay rows are held afterwards.  Replaces
 * the reference's per-step np.random draws + SP.next (sp.py:221-258).      */
int pbh_legacy_run(pbh_engine *eng, int64_t n_steps, int32_t steps_per_launch);
/* on != 0: pbh_legacy_run also keeps each step's MH threshold t (the
 * reference's metropolis_thresh draw, sp_utils.py:30-31, which SP.next
 * returns as opqrstuv.t, sp.py:249-258) on the device; pbh_get_thresholds
 * copies steps [first, first + n_steps) of the last pbh_legacy_run as
 * [n_steps][n_chains].  (The fused kernel stores them as it draws them.)   */
int pbh_set_record_threshold(pbh_engine *eng, int32_t on);
int pbh_get_thresholds(pbh_engine *eng, int64_t first, int64_t n_steps, double *out);
/* The next n_steps draws of every chain's device RandomState (after
 * pbh_legacy_seed) into out [n_steps][n_chains], the chain's generator
 * continuing: kind PBH_DRAWS_LINREG draws what the gibbs_linreg example's
 * cond_reg consumes at global step step0 + t (examples/mcmc/gibbs_linreg.py:
 * 38-47): standard_gamma(param) when (step0 + t) % 3 == 2, else the legacy
 * gauss (NumPy's legacy_standard_gamma: Marsaglia-Tsang over the polar gauss
 * and random_sample, the shape < 1 and shape == 1 branches included);
 * PBH_DRAWS_GAUSS the legacy gauss every step.                             */
enum pbh_draws { PBH_DRAWS_GAUSS = 0, PBH_DRAWS_LINREG = 1 };
int pbh_legacy_draws(pbh_engine *eng, int64_t n_steps, int64_t step0, int32_t kind,
                     double param, double *out);

/* ---- running (SP.walk / sample_generator: sp.py:281-295, sp_utils.py:8-16) */
/* Device trace ring for the next runs: every thin-th step is recorded.
 * debug = 1 also records proposals p_x, p_p and the score s; OR-ed with
 * PBH_TRACE_NOFILL the records are not zero-filled (the caller's next run
 * writes every one of them).                                                */
enum { PBH_TRACE_NOFILL = 0x100 };
int pbh_alloc_trace(pbh_engine *eng, int64_t capacity, int32_t thin,
                    int32_t debug);
/* Launches n_steps chain-steps on the engine stream (asynchronous);
 * steps_per_launch bounds one kernel's fused step loop (0 = all).          */
int pbh_run(pbh_engine *eng, int64_t n_steps, int32_t steps_per_launch);
int pbh_sync(pbh_engine *eng);
/* pbh_run + pbh_sync in one call (one host-to-library crossing: the
 * synchronous walk of sp.py:281-295 for a batch of steps).                  */
int pbh_run_wait(pbh_engine *eng, int64_t n_steps, int32_t steps_per_launch);
/* flags = OR of enum pbh_collect; default PBH_COLLECT_MOMENTS.  With 0 the
 * kernels keep no running moments (no per-launch read-modify-write of them);
 * pbh_trace_stats then reduces the recorded trace on the device instead.   */
int pbh_set_collect(pbh_engine *eng, int32_t flags);
/* Kernel-only time of the last pbh_run (HIP events on the engine stream;
 * for a resident-server command, its first workgroup's sight of the command
 * to its last workgroup's completion on the device's 100 MHz clock).       */
int pbh_last_run_ms(pbh_engine *eng, double *ms, int64_t *launches);
/* Resident sampling server (opt-in, PBH_SERVER=1 at pbh_create; the
 * walk/next loop of sp.py:221-295 kept resident on the device): a run that is
 * one steady-state lane-pair launch (the cfg2 form, production Philox, thin
 * 1, past step 1, every record inside the trace) becomes a command to a
 * kernel that stays resident with the chain state in registers; the kernel
 * leaves after PBH_SERVER_IDLE_MS (default 1000) without a command.  Every
 * other entry point stops it first; pbh_server_stop stops it explicitly
 * (chain state stored, stream idle); pbh_destroy stops it.  active = the
 * server kernel is running; commands / launches: totals of this engine.    */
int pbh_server_stop(pbh_engine *eng);
int pbh_server_info(pbh_engine *eng, int32_t *active, int64_t *commands,
                    int64_t *launches);
/* Diagnostic: the server's per-workgroup completion words of the last
 * command (seq, the 100 MHz stamps of its sight and completion); n = the
 * workgroup count, at most cap entries copied.                             */
int pbh_server_stamps(pbh_engine *eng, int32_t cap, uint32_t *seq, uint64_t *t0,
                      uint64_t *t1, int32_t *n);

/* ---- results (SP.__call__(samples) summary: sp.py:131-198) -------------- */
int pbh_get_state(pbh_engine *eng, double *x, double *logp);
int pbh_trace_len(pbh_engine *eng, int64_t *n_recorded);
/* Copies recorded steps [first, first + n) of the trace:
 * x [n][d][N], logp [n][N], acc [n][ceil(N/64)] accept bitmask words
 * (bit j of word w = chain 64 w + j).  Optional debug buffers may be NULL. */
int pbh_get_trace(pbh_engine *eng, int64_t first, int64_t n, double *x,
                  double *logp, uint64_t *acc, double *p_x, double *p_p,
                  double *s);
/* Per-chain running moments over every step since the last reset:
 * sum[d][N], sumsq[d][N] of the accepted state, n_acc[N] accepts.          */
int pbh_get_moments(pbh_engine *eng, double *sum, double *sumsq,
                    int64_t *n_acc, int64_t *n_steps);
int pbh_reset_moments(pbh_engine *eng);
/* Per-(chain, dim) effective sample size of trace records [first, first +
 * count) on the device: Geyer's initial positive sequence over the
 * autocorrelations of each centred series (the estimator behind cfg5's
 * ESS/s); the autocorrelations by FFT (two series per
 * 4 096-point transform, count <= 2 048; direct sums above that or with
 * PBH_ESS_FFT=0); ess [d][N] on the host (may be NULL).  The result also
 * stays in the engine for pbh_rccl_allgather_stats.                         */
int pbh_trace_ess(pbh_engine *eng, int64_t first, int64_t count, double *ess);
/* The sum over chains of pbh_trace_ess's per-chain ESS, per dim: total[d]
 * (cfg5's ESS is the min over dims of the summed per-chain
 * ESS), reduced on the device -- d doubles cross to the host, not d N.      */
int pbh_trace_ess_total(pbh_engine *eng, int64_t first, int64_t count, double *total);
/* The same per-chain statistics reduced on the device from trace records
 * [first, first + count) (PD summate + expectation over a recorded trace,
 * pd_utils.py:332-411, pd.py:373-407, without copying the trace to the
 * host).  The result replaces the engine's moment buffers (what
 * pbh_rccl_allgather_stats sends, n_steps = count); host pointers may be
 * NULL.                                                                     */
int pbh_trace_stats(pbh_engine *eng, int64_t first, int64_t count, double *sum,
                    double *sumsq, int64_t *n_acc);
/* PD.expectation of a summary over trace records [first, first + count) on
 * the device (pd.py:373-405): per chain and dim sum_t p_t v_t^e /
 * max(tiny, sum_t p_t), p_t = v.prob rescaled to linear (exp_logp of the
 * recorded log-prob under a log pscale), v^e = v when exponent is 0 (the
 * reference's `val ** exponent if exponent else val`), sums in record
 * order.  out [d][N] on the host.                                           */
int pbh_trace_expectation(pbh_engine *eng, int64_t first, int64_t count,
                          double exponent, double *out);
/* summary.sorted(key).quantile(q)[key] over trace records [first, first +
 * count) on the device (pd.py:408-493), for every chain and every key: each
 * dim k is sorted by itself (after sorted(key) only the sort key is
 * monotonic; the reference gives {size} for the others), ascending, ties by
 * record index, NaN last; out[j][k][c] is PD.quantile(q[j]) of chain c's
 * summary sorted by dim k, for key k.  weighted = 1: the weights are the
 * recorded v.prob rescaled to linear (as pbh_trace_expectation); weighted =
 * 0: unit weights, the plain empirical quantile -- PD(vals, prob = ones,
 * pscale = 'lin') on the host, which it equals bit for bit (with weights,
 * to the device's exp).  The arithmetic is the reference's: cumprob =
 * cumsum(p) / max(tiny, sum p), idx = max(0, #{cumprob <= q} - 1), the last
 * record's value at idx = count - 1, else np.interp between the records idx
 * and idx + 1 when |p1 - p0| < min(q, 1 - q), else their p-weighted mean.
 * 1 <= count <= PBH_QUANTILE_MAX_RECORDS (a series is sorted in LDS), 1 <=
 * nq <= PBH_QUANTILE_MAX_Q, every q[j] in [0, 1]; out [nq][d][N] on the
 * host.  Changes nothing in the engine: not the moments (unlike
 * pbh_trace_stats), the ESS, the trace, the chains or the generators.       */
#define PBH_QUANTILE_MAX_RECORDS 2048
#define PBH_QUANTILE_MAX_Q 64
int pbh_trace_quantile(pbh_engine *eng, int64_t first, int64_t count,
                       int32_t nq, const double *q, int32_t weighted,
                       double *out);
/* Cross-chain convergence over trace records [first, first + count) on the
 * device, per dim (added within revision 2: PBH_ABI_REVISION did not change
 * for it, so a caller that may meet an older revision-2 library finds out by
 * looking the symbol up).
 * split_rhat [d]: split-R-hat (Gelman et al., BDA3; Vehtari et al. 2021,
 * without rank normalisation).  h = count / 2; every chain gives the split
 * chains [first, first + h) and [first + count - h, first + count) (an odd
 * count drops the middle record).  Over the 2N split chains with mean m_j and
 * variance s2_j (ddof 1): W = mean_j s2_j, B/h = var_j m_j (ddof 1), R-hat =
 * sqrt(((h - 1) / h W + B/h) / W).  Needs count >= 4.
 * nested_rhat [d]: nested R-hat (Margossian et al. 2024).  Chain c belongs to
 * superchain c / group; the caller starts a superchain's chains at one point.
 * With per-chain mean m_c and variance s2_c (ddof 1) over the whole window,
 * per superchain mu_k = mean_c m_c, B_k = var_c m_c (ddof 1; 0 at group = 1),
 * W_k = mean_c s2_c: nR-hat = sqrt(1 + var_k mu_k / mean_k (B_k + W_k)), var_k
 * at ddof 1.  Needs count >= 2, group >= 1, N % group == 0, N / group >= 2;
 * group is read only when nested_rhat is given.
 * chain_stats [6][d][N]: mean and variance of the first half, of the second
 * half and of the whole window, per chain -- all either statistic needs, so
 * the rows of several ranks concatenated in chain order give the pooled
 * statistic on the host (probayes_amd/diag.py).  With count < 4 the half
 * variances are 0/0.
 * Each of the three may be NULL.  The values are the IEEE results of the
 * formulas with no special cases: all chains constant and equal give NaN,
 * constant but different +inf, and a NaN record propagates.  Sums run in a
 * fixed order: two calls on one trace give the same bits.  Changes nothing in
 * the engine: not the moments, the ESS, the trace, the chains or the
 * generators.                                                               */
int pbh_trace_rhat(pbh_engine *eng, int64_t first, int64_t count, int32_t group,
                   double *split_rhat, double *nested_rhat, double *chain_stats);
/* Quantiles of trace records [first, first + count) pooled over every chain
 * and record, per dim, on the device (added within revision 2 as
 * pbh_trace_rhat was: look the symbol up).  probayes_amd/diag.py
 * pooled_quantile is the definition.  Per dim, with s the M = N count values
 * sorted ascending: vi = (M - 1) q in fp64, lo = floor(vi), hi = min(lo + 1,
 * M - 1), g = vi - lo, a = s[lo], b = s[hi]; out[j][k] is b - (b - a)(1 - g)
 * if g >= 0.5, else a + (b - a) g -- np.quantile's default method, bit for
 * bit.  A dim that holds a NaN gives NaN for every q; there are no other
 * special cases (a = b = inf gives NaN); -0.0 counts as +0.0 and is returned
 * as +0.0.  order_stats [nq][2][d] (may be NULL): a and b themselves.
 * The order statistics are found by a radix select over the monotone 64-bit
 * image of the doubles in six streaming passes over the window, with integer
 * histograms as the only state: no record limit, the result equals sorting on
 * the host whatever the order of the atomics, and two calls give the same
 * bits.  1 <= count, 1 <= nq <= PBH_QUANTILE_MAX_Q, every q[j] in [0, 1]; out
 * [nq][d] on the host.  Changes nothing in the engine: not the moments, the
 * ESS, the trace, the chains or the generators.                             */
int pbh_trace_quantile_pooled(pbh_engine *eng, int64_t first, int64_t count,
                              int32_t nq, const double *q, double *out,
                              double *order_stats);

/* Rank-normalised and folded split-R-hat (Vehtari et al. 2021) over trace
 * records [first, first + count) on the device, per dim (added within
 * revision 2 as pbh_trace_rhat was: PBH_ABI_REVISION did not change for it,
 * look the symbol up).  probayes_amd/diag.py average_ranks / normal_scores /
 * rank_rhat are the definition.  Per dim, over the M = N count values pooled
 * over chains and records: the 1-based rank of each value, ties taking the
 * mean of their ranks, -0.0 and +0.0 one value; the normal score z = Phi^-1((r
 * - 3/8) / (M + 1/4)) by Wichura's AS241 (PPND16) in fp64; and split-R-hat of
 * the scores as pbh_trace_rhat forms it of the values.
 * bulk [d]: that, of the ranks of the values.  folded [d]: of the ranks of
 * |x - med|, med the dim's pooled median (pbh_trace_quantile_pooled at q =
 * 0.5, bit for bit).  The rank-normalised R-hat a caller reads is the larger
 * of the two.
 * ranks, folded_ranks [count][d][N]: the ranks themselves.
 * Each of the four may be NULL; a variant is computed only if one of its two
 * outputs is asked for, and with all four NULL the call returns PBH_ERR_ARG
 * (whatever else it was given).  A dim that holds a NaN -- after folding also
 * a NaN median or an inf - inf -- gives NaN for every rank and for both
 * statistics; there are no other special cases (constant chains give W = 0
 * and so inf or NaN, as pbh_trace_rhat does).
 * The ranks come from a least-significant-digit radix sort of (key, element
 * index) pairs over the monotone 64-bit image of the doubles, one dim and one
 * variant at a time, in the engine's reduction scratch (about 40 bytes per
 * element of a dim); every pass is stable and no atomic decides a position, so
 * the ranks equal sorting on the host and two calls give the same bits.
 * count >= 4; N count >= 2^32 is PBH_ERR_UNSUPPORTED (the element index is 32
 * bits).  Changes nothing in the engine: not the moments, the ESS, the trace,
 * the chains or the generators.                                             */
int pbh_trace_rhat_rank(pbh_engine *eng, int64_t first, int64_t count,
                        double *bulk, double *folded, double *ranks,
                        double *folded_ranks);

/* Bulk- and tail-ESS across chains (Vehtari et al. 2021) over trace records
 * [first, first + count) on the device, per dim (added within revision 2 as
 * pbh_trace_rhat_rank was: PBH_ABI_REVISION did not change for it, look the
 * symbol up).  probayes_amd/diag.py split_chain_acov / multi_chain_ess /
 * rank_ess are the definition.  Per dim and variant, over the C = 2 N split
 * chains of h = count / 2 records (first halves of the chains, then second
 * halves; an odd count drops the middle record): the biased autocovariance of
 * each split chain about its own mean, averaged over the split chains, A[t], t
 * < h; and Stan's estimator from A and the split chains' means (Geyer's
 * initial positive and monotone sequences over rho[t] = 1 - (A[0] h / (h - 1) -
 * A[t]) / (A[0] + var_j m_j), tau floored at 1 / log10(C h), ESS = C h / tau).
 * The variants are the series the estimator reads:
 * bulk [d]: the normal scores of the pooled ranks (pbh_trace_rhat_rank's).
 * tail_parts [2][d]: lower, then upper -- the indicators x <= q05 and x <= q95
 * as 0. / 1., q the dim's pooled quantiles (pbh_trace_quantile_pooled at 0.05
 * and 0.95, bit for bit).  tail [d]: the smaller of the two (a NaN propagates).
 * basic [d]: the values themselves.
 * mean_acov [4][d][h]: the A[t] of the variants, in the order bulk, tail_lower,
 * tail_upper, basic; rows of a variant that was not computed are left
 * untouched.
 * Each of the five may be NULL; bulk asks for the bulk variant, tail or
 * tail_parts for the two tail variants, basic for the basic one, mean_acov
 * alone for all four, and with all five NULL the call returns PBH_ERR_ARG
 * (whatever else it was given).  A dim that holds a NaN gives NaN everywhere;
 * there are no other special cases (all chains constant and equal give NaN,
 * constant chains that differ a finite value).
 * The autocovariance is linear in the power spectrum: a kernel sums |FFT|^2
 * of the centred, zero-padded split chains (4 096 points in fp64, two chains
 * to a complex transform) in a fixed order without floating-point atomics, one
 * inverse transform per dim and variant gives A, and the O(h) estimator runs
 * on the host; two calls give the same bits.  count >= 4; count / 2 >
 * PBH_ESS_RANK_MAX_HALF is PBH_ERR_UNSUPPORTED, and so is, for bulk, N count
 * >= 2^32 (the sort's element index).  Changes nothing in the engine: not the
 * moments, the per-chain ESS, the trace, the chains or the generators.       */
#define PBH_ESS_RANK_MAX_HALF 2048
int pbh_trace_ess_rank(pbh_engine *eng, int64_t first, int64_t count,
                       double *bulk, double *tail, double *tail_parts,
                       double *basic, double *mean_acov);

/* Pointwise log-likelihood over trace records [first, first + count) on the
 * device, per observation (added within revision 2 as pbh_trace_rhat was:
 * PBH_ABI_REVISION did not change for it, look the symbol up).  The program is
 * a PBH_TARGET_EXPR program over data [n_cols][n_obs] of the pointwise shape:
 * scalar words, one LOOP region, and that region's SUM as the last word
 * (probayes_amd/expr.py trace_pointwise makes one of a callable that returns
 * the unreduced vector of terms).  The body's last value at observation j and
 * draw s = (record, chain) is the term T[s, j] (expr.evaluate_pointwise); the
 * SUM is not formed.  Over the S = N count draws of the window, per
 * observation (probayes_amd/diag.py pointwise_stats is the definition):
 * lse [n_obs]: log sum_s exp T[s, j], shifted by the largest term -- -inf when
 * every term is -inf, +inf with a +inf term, NaN with a NaN term; lppd_j is
 * lse[j] - log S.
 * mean [n_obs], var [n_obs]: the mean and the sample variance (ddof 1) of T[.,
 * j]; the sum of var is WAIC's effective number of parameters.  A column that
 * holds an infinite term has that infinity (or NaN for both) as its mean and a
 * NaN variance.
 * Each of the three may be NULL.  The program has nothing to do with the
 * engine's model: it may be any target kind, its variables are the engine's
 * dims (a variable index >= dim, or dim > PBH_EXPR_MAX_DIM, is PBH_ERR_ARG),
 * and an engine whose own target is an expression program keeps it.  T is
 * never stored: a workgroup folds the terms of 256 chains, 8 observations and
 * a slice of the records into an online log-sum-exp pair and Welford's moments
 * per lane, merges its lanes in a fixed order, and a second kernel merges the
 * workgroups' rows in index order: no floating-point atomics, two calls give
 * the same bits.  count >= 1 and N count >= 2; a bad program or one that is
 * not of the pointwise shape is PBH_ERR_ARG, no trace PBH_ERR_STATE.  Changes
 * nothing in the engine: not the model, the moments, the ESS, the trace, the
 * chains or the generators.                                                 */
int pbh_trace_pointwise(pbh_engine *eng, int64_t first, int64_t count,
                        const int32_t *code, int32_t n_code,
                        const double *consts, int32_t n_consts, int32_t depth,
                        const double *data, int32_t n_cols, int32_t n_obs,
                        double *lse, double *mean, double *var);

/* The tail of the pointwise terms over trace records [first, first + count)
 * on the device, per observation: what Pareto-smoothed importance sampling
 * (PSIS-LOO: Vehtari, Gelman & Gabry 2017; Vehtari et al. 2024) needs of the
 * terms T[s, j] of pbh_trace_pointwise, which are never stored (added within
 * revision 2 as pbh_trace_pointwise was: look the symbol up).  The program and
 * data arguments are pbh_trace_pointwise's.  Over the S = N count draws
 * (probayes_amd/diag.py pointwise_tail is the definition):
 * tail [n_obs][k]: the k smallest terms of observation j, ascending -- the k
 * largest importance log-ratios -T -- either zero as +0.0 and NaN, the largest
 * in the order, last.
 * rest_lse [n_obs]: log sum exp(-T[s, j]) over the other S - k draws, with
 * pbh_trace_pointwise's conventions: -inf when every one of them is +inf, +inf
 * with a -inf term among them, NaN with a NaN.
 * passes (may be NULL): the count passes run, the most of any batch.
 * A most-significant-digit radix select on the monotone 64-bit image of a
 * double, one select per observation, 10 bits a pass, the terms recomputed in
 * every pass: the device counts the next digit under every observation's
 * prefix (integer atomics), the host picks the digit that holds rank k - 1;
 * once the keys at or below the prefix fit `capacity` per observation (0: max(2
 * k, 65 536), no more than S), or all 64 bits are fixed, one more pass appends
 * them to per-observation lists and folds minus every other term into an
 * online log-sum-exp, merged in pbh_trace_pointwise's fixed order.  The host
 * sorts each list: the first k are the tail, the others join the rest in
 * ascending order.  The order in which the lists were filled is lost in the
 * sort and no floating-point atomic is used: two calls give the same bits.
 * The observations are taken in batches, so that the lists hold at most 256
 * MiB whatever n_obs is.  1 <= k < N count; capacity >= k or 0, at most 4 194
 * 304; tail or rest_lse may be NULL, not both (PBH_ERR_ARG); other errors as
 * pbh_trace_pointwise.  Changes nothing in the engine.                       */
int pbh_trace_pointwise_tail(pbh_engine *eng, int64_t first, int64_t count,
                             const int32_t *code, int32_t n_code,
                             const double *consts, int32_t n_consts,
                             int32_t depth, const double *data, int32_t n_cols,
                             int32_t n_obs, int64_t k, int64_t capacity,
                             double *tail, double *rest_lse, int32_t *passes);

/* Posterior covariance over trace records [first, first + count) on the
 * device, pooled over every chain and record (added within revision 2 as
 * pbh_trace_rhat was: PBH_ABI_REVISION did not change for it, look the symbol
 * up).  probayes_amd/diag.py pooled_cov is the definition.  With M = N count
 * draws, K [d] the mean over chains of record `first` and v = x - K: S_a = sum
 * v_a and P_ab = sum v_a v_b over the window;
 * mean [d]: K + S / M.
 * cov [d][d]: (P_ab - S_a S_b / M) / (M - 1), computed for a <= b and
 * mirrored, so the matrix is symmetric in its bits.
 * corr [d][d]: cov_ab / sqrt(cov_aa cov_bb), the diagonal included.
 * The shift costs no traffic and lies among the draws, so S S / M cancels
 * against P only mildly wherever the posterior lies; sums of raw products lose
 * everything once the mean is large against the spread.
 * Each of the three may be NULL; with all three NULL the call returns
 * PBH_ERR_ARG (whatever else it was given).  The values are the IEEE results
 * of the formulas with no special cases: chains that are constant and equal
 * give cov exactly 0 and corr NaN (0 / 0), also on the diagonal, which is
 * exactly 1 otherwise; a NaN record propagates.  The products are accumulated
 * with a fused multiply-add, so the definition is met to rounding, not bit for
 * bit.  Sums run in a fixed order without atomics: two calls on one trace give
 * the same bits.  count >= 1 and N count >= 2.  Changes nothing in the engine:
 * not the moments, the ESS, the trace, the chains or the generators.         */
int pbh_trace_cov(pbh_engine *eng, int64_t first, int64_t count, double *mean,
                  double *cov, double *corr);

/* Posterior histograms over trace records [first, first + count) on the
 * device, pooled over every chain and record (added within revision 2 as
 * pbh_trace_cov was: PBH_ABI_REVISION did not change for them, look the
 * symbols up).  probayes_amd/diag.py hist_bin, pooled_hist and pooled_hist2d
 * are the definition.  A dim k with n_bins[k] = B > 0 has B + 1 strictly
 * increasing finite edges e[0 .. B]; n_bins[k] = 0 skips the dim.  The bin of
 * a value x:
 *   bin i holds e[i] <= x < e[i + 1];
 *   the last bin also holds x == e[B];
 *   x < e[0] is below, x > e[B] is above, a NaN is NaN: none of them is in a
 *   bin;
 *   plain comparisons: -0.0 and +0.0 are one value, -inf is below, +inf above.
 * That is the rule of np.histogram(a, edges), of np.histogram(a, B, range =
 * (lo, hi)) with edges = np.linspace(lo, hi, B + 1), and of np.histogram2d
 * with explicit edges; the counts equal NumPy's bit for bit: the only state is
 * integer counts, which no order of adds changes.
 * pbh_trace_hist: counts holds the listed dims' counts one after the other,
 * n_bins[k] each; outside [d][3] (may be NULL) holds below, above and NaN per
 * dim, 0 for a skipped dim, so that a dim's counts and its row of outside add
 * up to N count.
 * pbh_trace_hist2d: per pair (a, b) of dims, counts [B_a][B_b] holds the draws
 * with x_a in bin i of dim a and x_b in bin j of dim b; a draw with either
 * value outside its bins is dropped.  a == b is allowed.  The pairs' grids lie
 * one after the other.
 * PBH_ERR_ARG, the message naming the dim or the pair and the index: counts
 * NULL (whatever else was given), every n_bins[k] 0, an n_bins[k] below 0 or
 * above PBH_HIST_MAX_BINS, an edge that is not finite, edges that do not
 * strictly increase; for pairs n_pairs outside 1 .. 65 535, a dim outside [0,
 * d), a dim without edges, B_a B_b above PBH_HIST2D_MAX_CELLS.  count >= 1.
 * Two calls give the same counts.  Changes nothing in the engine: not the
 * moments, the ESS, the trace, the chains or the generators.                */
#define PBH_HIST_MAX_BINS 4096        /* per dim */
#define PBH_HIST2D_MAX_CELLS 16384    /* B_a * B_b of a pair: 64 KiB of uint32 */
int pbh_trace_hist(pbh_engine *eng, int64_t first, int64_t count,
                   const int32_t *n_bins, const double *edges, int64_t *counts,
                   int64_t *outside);
int pbh_trace_hist2d(pbh_engine *eng, int64_t first, int64_t count,
                     const int32_t *n_bins, const double *edges,
                     int32_t n_pairs, const int32_t *pairs, int64_t *counts);

/* ---- multi-GPU: one RCCL all-gather over xGMI --------- */
int pbh_rccl_unique_id(uint8_t id[128]);
int pbh_rccl_init(pbh_engine *eng, int32_t rank, int32_t world,
                  const uint8_t id[128]);
/* The largest N_local over the ranks (a collective: every rank calls it).  */
int pbh_rccl_max_chains(pbh_engine *eng, int64_t *n_max);
/* The one collective of the data path: gathers every
 * rank's per-chain statistics into out[world][3d+1][n_max] on the host,
 * rows sum[d], sumsq[d], n_acc, ess[d] (the moment buffers: in-kernel
 * moments or pbh_trace_stats; ess: pbh_trace_ess, NaN before), and every
 * rank's N_local into counts[world].  Ranks may hold different N_local (the
 * ragged contiguous blocks of dist.shard): rank r's columns >= counts[r] are
 * padding.  Every rank enters every collective whatever fails locally, and
 * all ranks then return the same error.                                     */
int pbh_rccl_allgather_stats(pbh_engine *eng, double *out, int64_t *counts);
/* Max-reduces one double over ranks (bench timing).                         */
int pbh_rccl_allreduce_max(pbh_engine *eng, double *value);
int pbh_rccl_destroy(pbh_engine *eng);

/* ---- likelihoods (likelihoods.py) --------------------------------------- */
/* bool_perm_freq (likelihoods.py:45-101): counts[2^cols] (C order: the first
 * column is the most significant index bit, each dimension ordered [False,
 * True]) of the boolean row patterns of bool2d [rows][cols] (one byte per
 * element, non-zero = True).  1 <= cols <= 26; rows = 0 gives zero counts.
 * Host buffers.  The kernel runs `reps` >= 1 times on device-resident input
 * after one untimed warm-up launch (counts of the last run are returned);
 * *kernel_ms (may be NULL) receives
 * the average kernel time from HIP events.                                  */
int pbh_bool_perm_freq(int device, int64_t rows, int32_t cols,
                       const uint8_t *bool2d, int64_t *counts, int32_t reps,
                       double *kernel_ms);

/* ---- user-conditional Gibbs: conjugate linear regression ---------------- */
/* Replaces the per-chain loop of SP.next -> RF.eval_tfun (rf.py:413-462)
 * over the user conditional cond_reg of examples/mcmc/gibbs_linreg.py:34-62
 * (paras = beta_0 & beta_1 & y_sigma, tsteps = 1, gibbs scores), with
 * v.prob = sum_j norm.logpdf(y_j, b0 + b1 x_j, y_sigma) + the joint uniform
 * root priors (rf.py:541-562, rv_utils.py:30-38).
 * hyper[6] = beta_0_mu, beta_0_sigma, beta_1_mu, beta_1_sigma,
 *            y_sigma_alpha, y_sigma_beta (cond_reg's keyword defaults);
 * vsets[6] = closed (lo, hi) of beta_0, beta_1, y_sigma (joint=True: each
 * adds -log(hi - lo) inside, NEARLY_NEGATIVE_INF outside); NULL = no prior
 * terms (joint=False).  Step k of the chain
 * (absolute k = step0 + t) updates parameter k mod 3 (the RF's __cond_mod).
 * init/final_x [3][n_chains]; rand [n_steps][n_chains] (REPLAY: the standard
 * gauss, or standard_gamma(alpha + n_obs/2) on y_sigma steps, in NumPy's
 * legacy order); trace_x [n_steps][3][n_chains], trace_lp [n_steps][n_chains]
 * (either may be NULL: then no device trace is kept).  rng_mode REPLAY /
 * PHILOX_F64 use the reference's arithmetic; PHILOX uses centred sufficient
 * statistics.  Host buffers; the chain runs `reps` >= 1 times from init on
 * device-resident inputs (reps > 1: after one untimed warm-up), *kernel_ms
 * (may be NULL) = the average kernel time.                                  */
int pbh_linreg_gibbs(int device, int64_t n_obs, const double *x_obs,
                     const double *y_obs, const double *hyper,
                     const double *vsets, int64_t n_chains,
                     int64_t chain_offset, int64_t n_steps, int64_t step0,
                     const double *init, int32_t rng_mode, uint64_t seed,
                     const double *rand, double *trace_x, double *trace_lp,
                     double *final_x, double *final_lp, int32_t reps,
                     double *kernel_ms);

/* ---- diagnostics -------------------------------------------------------- */
/* Evaluates the production-mode acceptance filter and the exact ratio form
 * (sp_utils.py:40-64) on device for n triples (lp, lp', t = u01(t0, t1)).
 * out[i]: bit 0 = exact decision s >= t, bit 1 = the filter decided without
 * the exact fallback, bit 2 = the filter's decision.                        */
int pbh_check_accept(int device, int64_t n, const double *lp,
                     const double *lpp, const uint32_t *t0, const uint32_t *t1,
                     int32_t lin, uint8_t *out);

/* Evaluates the production Gibbs kernel's fp64 Box-Muller (box_muller_fast:
 * the cheap log / sin / cos) and the libm form on n Philox-like blocks
 * words[n][4]; fast[n][2], ref[n][2] receive (z0, z1) of each.             */
int pbh_check_normals(int device, int64_t n, const uint32_t *words,
                      double *fast, double *ref);

/* The production fp64 normals (bm96_pair, PBH_RNG_PHILOX / XOSHIRO) on n
 * word triples words[n][3]: fast[n][2] = bm96_pair, ref[n][2] = the same u1
 * and angle through libm log / sqrt / sincos.  pbh_bm64_tables fills
 * out[4162] with the engine's tables ({-2 ln c_j, 1/c_j} x 1025, {sin, cos}
 * x 1024 over the full turn, 2^(i/64) x 64).                                */
int pbh_check_normals64(int device, int64_t n, const uint32_t *words,
                        double *fast, double *ref);
int pbh_bm64_tables(double *out);

/* Evaluates a PBH_TARGET_EXPR program (checked as pbh_set_model checks it)
 * at n points x[n][d] with the kernels' own device function; out[n].       */
int pbh_eval_expr(int device, int32_t d, const int32_t *code, int32_t n_code,
                  const double *consts, int32_t n_consts, int32_t depth,
                  int64_t n, const double *x, double *out);
/* The same for a program with loop regions over data[n_cols][n_obs], through
 * the interpreter of the data kernels.  PBH_EXPR_DATA_WIDE=0 in the
 * environment selects the one-observation-at-a-time body (same bits).       */
int pbh_eval_expr_data(int device, int32_t d, const int32_t *code, int32_t n_code,
                       const double *consts, int32_t n_consts, int32_t depth,
                       const double *data, int32_t n_cols, int32_t n_obs,
                       int64_t n, const double *x, double *out);

#ifdef __cplusplus
}
#endif
#endif /* PBHIP_H */
