"""The production kernels' Philox draw contracts, rebuilt in NumPy.

Every draw of the PBH_RNG_PHILOX / PBH_RNG_PHILOX_F64 kernels is a pure
function of (seed, chain id, absolute step), so the host can rebuild each
step's proposal randoms r and acceptance threshold t and a test can check the
recorded chains step by step (tests/test_gpu_philox_pin.py).  Everything is
vectorised over (step, chain); words are uint64 arrays masked to 32 bits.

Conventions read from the code (pbh_engine.hip, pbh_kernels_impl.h):

  * chain ids are chain_offset + c for the engine's chain c (KArgs.off);
  * the first step after Engine.init_chains is absolute step g = 0 (or the g
    given to Engine.set_step right after it) and has no predecessor: the
    proposal is accepted whatever the threshold (pbh_init_chains clears
    has_pred; every later step, in the same or a later launch, has one);
  * the key is (seed & 0xFFFFFFFF, seed >> 32);
  * counter words: (j, g & M32, chain & M32,
    (chain >> 32) ^ ((g >> 32) << 16)), j the block index of a role;
  * the lane-pair kernel (mh_pair_kernel, even d >= 4): lane half h owns the
    dims [h H, h H + H), H = d / 2, and draws them from blocks q + 16 h; half
    1 holds the threshold and decides (its lead, tail block 0x40 + 16);
  * the production Gibbs kernel (gibbs_fast_kernel, d <= 16, L = 1, 2 or 4
    lanes per chain, M = d / L): step g updates the coordinates [(g % nblk)
    tsteps, min(d, ... + tsteps)), nblk = ceil(d / tsteps); every draw of a
    coordinate cycle is keyed by the cycle's FIRST step gc = g - g % nblk,
    whichever launch or step consumes it.  Coordinate k = p M + ii takes
    component ii % 2 of the Box-Muller pair (box_muller(): u1 = 1 - u01(x, y),
    u2 = u01(z, w); the device's box_muller_tab approximates it) of block
    0x100 + 16 p + ii / 2 at (gc, chain).  A normal outside [ndtri(cdf_lo_k),
    ndtri(cdf_hi_k)] is replaced by ndtri(cdf_lo + (cdf_hi - cdf_lo) u), u =
    u01(w.x, w.y) of block 0x200 + k at (gc, chain);
  * the ndtri Gibbs kernel (gibbs_kernel: d > 16, PBH_GIBBS_FAST=0 or debug
    records): the j-th coordinate a step g updates takes u01(w.x, w.y) of
    block j at (g, chain), the step itself, not the cycle.

Draw functions return (r [T, d, N], thr [T, N], blocks) for the absolute steps
g0 .. g0 + T - 1 and chain ids chain_offset .. chain_offset + N - 1; blocks is
the list of (j, g-slot, role) Philox blocks consumed for one chain, g-slot
being the value in the counter's step words (g, or the step pair g >> 1).
"""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85

STEP_LEAD = 24        # kStepLead: step_draws' lead bits (mh_kernel, GMM kernels)
PAIR_LEAD = 16        # PairDraw::LB in PBH_RNG_PHILOX
UNIFORM_LEAD = 22     # the uniform draws' lead bits
TAIL_STEP = 0x40      # threshold tail block of the step_draws stream
TAIL_PAIR = 0x40 + 16  # ... of the lane-pair kernel (half 1 decides)
TAIL_UNIFORM = 0xFFFF  # ... of the uniform draws, and philox_f64's threshold
# the bits u01(a, b) keeps of its two words
U01_KEEP = (0xFFFFFFE0, 0xFFFFFFC0)


def _u64(v):
  return np.asarray(v, dtype=np.uint64)


def philox4x32_10(ctr, k0, k1):
  """Philox-4x32-10 (Salmon et al., SC'11; pbh_device.h philox4x32_10).
  ctr: four broadcastable arrays of 32-bit words; returns the four output
  words as uint64 arrays."""
  x, y, z, w = [_u64(c) & M32 for c in ctr]
  k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
  sh = np.uint64(32)
  for _ in range(10):
    p0, p1 = _M0 * x, _M1 * z          # 32 x 32 -> 64 bits: exact in uint64
    hi0, lo0 = p0 >> sh, p0 & M32
    hi1, lo1 = p1 >> sh, p1 & M32
    x, y, z, w = hi1 ^ y ^ np.uint64(k0), lo1, hi0 ^ w ^ np.uint64(k1), lo0
    k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
  return x, y, z, w


def ctr(j, g, chain):
  """pbh_kernels_impl.h ctr(j, g, chain) for non-negative 64-bit g, chain."""
  g, chain = _u64(g), _u64(chain)
  sh = np.uint64(32)
  w3 = ((chain >> sh) ^ (((g >> sh) & M32) << np.uint64(16))) & M32
  j = np.broadcast_to(_u64(j), np.broadcast(g, chain).shape)
  return j, g & M32, chain & M32, w3


def key(seed):
  seed = int(seed) & (2 ** 64 - 1)
  return seed & 0xFFFFFFFF, seed >> 32


def block(seed, j, g, chain):
  k0, k1 = key(seed)
  return philox4x32_10(ctr(j, g, chain), k0, k1)


def u01(a, b):
  """pbh_device.h u01: ((a >> 5) 2^26 + (b >> 6)) / 2^53."""
  a, b = np.asarray(a), np.asarray(b)
  return ((a >> 5).astype(np.float64) * 67108864.0 +
          (b >> 6).astype(np.float64)) / 9007199254740992.0


def bm96(a, b, c):
  """bm96_pair's construction (pbh_device.h): u1 = (k1 + 1/2) 2^-52 from
  b[31:12]:a, the full-turn angle (J + c 2^-32) 2 pi / 1024 with J = b[11:2].
  Returns (z0, z1, radius)."""
  a, b, c = _u64(a), _u64(b), _u64(c)
  k1 = ((b >> np.uint64(12)) << np.uint64(32)) | a
  u1 = (k1.astype(np.float64) + 0.5) * 2.0 ** -52
  j = ((b >> np.uint64(2)) & np.uint64(0x3FF)).astype(np.float64)
  ang = (j + c.astype(np.float64) * 2.0 ** -32) * (2 * np.pi / 1024)
  r = np.sqrt(-2.0 * np.log(u1))
  return r * np.cos(ang), r * np.sin(ang), r


def bm96_host(w):
  """bm96 of the rows of w [n, 3] -> ([n, 2] normals, [n] radii)."""
  z0, z1, r = bm96(w[:, 0], w[:, 1], w[:, 2])
  return np.stack([z0, z1], 1), r


def box_muller(blk):
  """pbh_device.h box_muller (the libm form of PBH_RNG_PHILOX_F64): u1 = 1 -
  u01(x, y), u2 = u01(z, w), r = sqrt(-2 log u1), (z0, z1) = r (cos, sin)(2
  pi u2).  The device calls sincospi(2 u2); here the angle is reduced to
  |f| <= 1/4 turn first (exactly), so that rounding pi f costs an ulp of the
  result, not of 2 pi."""
  x, y, z, w = blk
  u1 = 1.0 - u01(x, y)
  t = 2.0 * u01(z, w)                   # [0, 2) half turns, exact
  k = np.rint(t * 2.0)                  # quarter turns 0 .. 4
  f = t - k * 0.5                       # exact, |f| <= 1/4
  s, c = np.sin(np.pi * f), np.cos(np.pi * f)
  q = k.astype(np.int64) & 3
  cs = np.where(q == 0, c, np.where(q == 1, -s, np.where(q == 2, -c, s)))
  sn = np.where(q == 0, s, np.where(q == 1, c, np.where(q == 2, -s, -c)))
  r = np.sqrt(-2.0 * np.log(u1))
  return r * cs, r * sn


# ---------------------------------------------------------------------------
# layouts (the CPU tests read these)
# ---------------------------------------------------------------------------
def step_layout(d):
  """step_draws<D>: (words of the normal pairs, the lead's word, blocks)."""
  n_pairs = (d + 1) // 2
  n_words = 3 * n_pairs + 1
  return ([(3 * p, 3 * p + 1, 3 * p + 2) for p in range(n_pairs)], 3 * n_pairs,
          (n_words + 3) // 4)


def pair_layout(d):
  """PairDraw<H, PBH_RNG_PHILOX> of one lane half: H Box-Muller pairs (the
  two steps' 2 H normals), word 3 H holds both 16-bit leads."""
  h = d // 2
  n_words = 3 * h + 1
  return [(3 * q, 3 * q + 1, 3 * q + 2) for q in range(h)], 3 * h, (n_words + 3) // 4


def uniform_lead_fields(d):
  """The uniform draws' 22 lead bits as (word of block 0, mask, left shift
  into the lead; a negative shift is a right shift), most significant first."""
  f = [(0, 31, 17), (1, 63, 11)]
  if d >= 2:
    return f + [(2, 31, 6), (3, 63, 0)]
  return f + [(2, 0xFFE00000, -21)]


def _grid(g0, T, chain_offset, N):
  g = (np.uint64(int(g0)) + np.arange(T, dtype=np.uint64))[:, None]
  chain = (np.uint64(int(chain_offset)) + np.arange(N, dtype=np.uint64))[None, :]
  return g, chain


def _tail_thr(seed, j, g, chain, lead, lead_bits):
  """t = u01((lead << (32 - LB)) | (w.x >> LB), w.y) of block j."""
  w = block(seed, j, g, chain)
  t0 = ((lead << np.uint64(32 - lead_bits)) & M32) | (w[0] >> np.uint64(lead_bits))
  return u01(t0, w[1])


def _dedup(blocks):
  out, seen = [], set()
  for b in blocks:
    if b not in seen:
      seen.add(b)
      out.append(b)
  return out


# ---------------------------------------------------------------------------
# the draw contracts
# ---------------------------------------------------------------------------
def step_draws(seed, d, g0, T, chain_offset, N):
  """The step_draws stream (mh_kernel with a Gaussian proposal, the
  expression kernels, the GMM lanes / quad kernels): the words of blocks
  ctr(q, g, chain) in order; normal pair p takes words 3p .. 3p + 2; the next
  word's top 24 bits lead the threshold, block 0x40 gives its tail."""
  g, chain = _grid(g0, T, chain_offset, N)
  pairs, lead_word, nb = step_layout(d)
  w = []
  for q in range(nb):
    w.extend(block(seed, q, g, chain))
  r = np.empty((T, d, N))
  for p, (i0, i1, i2) in enumerate(pairs):
    z0, z1, _ = bm96(w[i0], w[i1], w[i2])
    r[:, 2 * p] = z0
    if 2 * p + 1 < d:
      r[:, 2 * p + 1] = z1
  lead = w[lead_word] >> np.uint64(32 - STEP_LEAD)
  thr = _tail_thr(seed, TAIL_STEP, g, chain, lead, STEP_LEAD)
  blocks = []
  for t in range(T):
    gt = int(g0) + t
    blocks += [(q, gt, 'normals/lead') for q in range(nb)]
    blocks.append((TAIL_STEP, gt, 'threshold tail'))
  return r, thr, _dedup(blocks)


def uniform_lead(w, d):
  lead = np.zeros_like(w[0])
  for word, mask, sh in uniform_lead_fields(d):
    v = w[word] & np.uint64(mask)
    lead = lead | (v << np.uint64(sh) if sh >= 0 else v >> np.uint64(-sh))
  return lead


def uniform_draws(seed, d, g0, T, chain_offset, N):
  """The production uniform draws (mh_kernel with uniform / sphere /
  vardelta proposals, mh_iid_full_kernel): blocks p give u01(x, y), u01(z,
  w); the 22-bit lead is the spare low bits of block 0 (w.z >> 21 at d = 1);
  block 0xFFFF gives the tail."""
  g, chain = _grid(g0, T, chain_offset, N)
  r = np.empty((T, d, N))
  nb = (d + 1) // 2
  lead = None
  for p in range(nb):
    w = block(seed, p, g, chain)
    r[:, 2 * p] = u01(w[0], w[1])
    if 2 * p + 1 < d:
      r[:, 2 * p + 1] = u01(w[2], w[3])
    if p == 0:
      lead = uniform_lead(w, d)
  thr = _tail_thr(seed, TAIL_UNIFORM, g, chain, lead, UNIFORM_LEAD)
  blocks = []
  for t in range(T):
    gt = int(g0) + t
    blocks += [(p, gt, 'uniforms/lead' if p == 0 else 'uniforms') for p in range(nb)]
    blocks.append((TAIL_UNIFORM, gt, 'threshold tail'))
  return r, thr, _dedup(blocks)


def pair_draws(seed, d, g0, T, chain_offset, N):
  """PairDraw (mh_pair_kernel, PBH_RNG_PHILOX): per step pair P = g >> 1 and
  lane half h the words of blocks q + 16 h at (P, chain); of the half's 2 H
  normals (pair q gives normals 2q, 2q + 1) 0 .. H-1 go to step 2P and H ..
  2H-1 to step 2P + 1; word 3 H holds the two steps' 16-bit leads (high half:
  step 2P).  Half 1's lead decides; tail: block 0x40 + 16 at (g, chain)."""
  assert d % 2 == 0 and d >= 4
  H = d // 2
  g, chain = _grid(g0, T, chain_offset, N)
  P = g >> np.uint64(1)
  odd = (g & np.uint64(1)).astype(bool)            # [T, 1]
  pairs, lead_word, nb = pair_layout(d)
  r = np.empty((T, d, N))
  lead = None
  for h in range(2):
    w = []
    for q in range(nb):
      w.extend(block(seed, q + 16 * h, P, chain))
    z = []
    for i0, i1, i2 in pairs:
      z0, z1, _ = bm96(w[i0], w[i1], w[i2])
      z += [z0, z1]
    for i in range(H):
      r[:, h * H + i] = np.where(odd, z[H + i], z[i])
    if h == 1:
      lw = w[lead_word]
      lead = np.where(odd, lw & np.uint64(0xFFFF), lw >> np.uint64(16))
  thr = _tail_thr(seed, TAIL_PAIR, g, chain, lead, PAIR_LEAD)
  blocks = []
  for t in range(T):
    gt = int(g0) + t
    for h in range(2):
      blocks += [(q + 16 * h, gt >> 1, 'pair normals/leads, half {}'.format(h))
                 for q in range(nb)]
    blocks.append((TAIL_PAIR, gt, 'threshold tail'))
  return r, thr, _dedup(blocks)


def f64_draws(seed, d, g0, T, chain_offset, N, kind='gauss', pair=False):
  """PBH_RNG_PHILOX_F64: the libm Box-Muller of blocks p (Gaussian
  proposals; the lane-pair kernel: half h's dims from blocks p + 16 h) or
  u01(x, y), u01(z, w) of blocks p (the other proposals); the threshold is
  u01(w.x, w.y) of block 0xFFFF."""
  g, chain = _grid(g0, T, chain_offset, N)
  r = np.empty((T, d, N))
  blocks_j = []
  if pair:
    assert kind == 'gauss' and d % 2 == 0 and d >= 4
    H = d // 2
    for h in range(2):
      for p in range((H + 1) // 2):
        z0, z1 = box_muller(block(seed, p + 16 * h, g, chain))
        r[:, h * H + 2 * p] = z0
        if 2 * p + 1 < H:
          r[:, h * H + 2 * p + 1] = z1
        blocks_j.append((p + 16 * h, 'normals, half {}'.format(h)))
  else:
    for p in range((d + 1) // 2):
      w = block(seed, p, g, chain)
      z0, z1 = box_muller(w) if kind == 'gauss' else (u01(w[0], w[1]), u01(w[2], w[3]))
      r[:, 2 * p] = z0
      if 2 * p + 1 < d:
        r[:, 2 * p + 1] = z1
      blocks_j.append((p, 'normals' if kind == 'gauss' else 'uniforms'))
  w = block(seed, TAIL_UNIFORM, g, chain)
  thr = u01(w[0], w[1])
  blocks = []
  for t in range(T):
    gt = int(g0) + t
    blocks += [(j, gt, role) for j, role in blocks_j]
    blocks.append((TAIL_UNIFORM, gt, 'threshold'))
  return r, thr, _dedup(blocks)


def streams(r, thr):
  """(r, thr) as the replay layout [T, d + 1, N] of oracle.run_mh."""
  return np.concatenate([r, thr[:, None, :]], axis=1)


# ---------------------------------------------------------------------------
# the CondCov Gibbs kernels
# ---------------------------------------------------------------------------
GIBBS_NORMALS = 0x100   # + 16 p + ii / 2: the Box-Muller pairs of part p
GIBBS_INVERT = 0x200    # + k: coordinate k's inversion uniform
GIBBS_MAX_D = 16        # gibbs_fast_form: d <= 16


def gibbs_layout(d, L):
  """gibbs_fast_kernel<d, L>: ([(block, pair component)] of every
  coordinate's normal, [inversion block] of every coordinate)."""
  assert L in (1, 2, 4) and d % L == 0
  M = d // L
  normals = [(GIBBS_NORMALS + 16 * (k // M) + (k % M) // 2, (k % M) % 2)
             for k in range(d)]
  return normals, [GIBBS_INVERT + k for k in range(d)]


def gibbs_lanes(d, env=None):
  """Lanes per chain as launch_gibbs_d chooses them: PBH_GIBBS_LANES when it
  is 1, 2 or 4 and divides d, else 1 for odd d, 2 for even d <= 12, and
  above that 4 where 4 divides d (2 where it does not)."""
  import os
  default = 1 if d % 2 else (2 if d <= 12 else (4 if d % 4 == 0 else 2))
  text = (os.environ if env is None else env).get('PBH_GIBBS_LANES')
  try:
    want = int(text) if text is not None else 0      # the engine reads it with atoi
  except ValueError:
    want = 0
  return want if want in (1, 2, 4) and d % want == 0 else default


def gibbs_lane_choices(d):
  """Every L the kernel can take at d."""
  return [L for L in (1, 2, 4) if d % L == 0]


def gibbs_cycle_starts(d, tsteps, g0, T):
  """(nblk, [gc of steps g0 .. g0 + T - 1])."""
  nblk = -(-d // tsteps)
  return nblk, [g - g % nblk for g in range(int(g0), int(g0) + T)]


def gibbs_fast_draws(seed, d, L, tsteps, g0, T, chain_offset, N):
  """gibbs_fast_kernel's draws for the steps g0 .. g0 + T - 1: z [T, d, N],
  the d Box-Muller normals of each step's coordinate cycle, and u_inv [T, d,
  N], the inversion uniforms of that cycle (steps of one cycle share both)."""
  _, gcs = gibbs_cycle_starts(d, tsteps, g0, T)
  uniq = sorted(set(gcs))
  at = {gc: i for i, gc in enumerate(uniq)}
  g = np.array(uniq, dtype=np.uint64)[:, None]
  chain = (np.uint64(int(chain_offset)) + np.arange(N, dtype=np.uint64))[None, :]
  normals, invert = gibbs_layout(d, L)
  z = np.empty((len(uniq), d, N))
  u = np.empty((len(uniq), d, N))
  pairs = {}
  for k in range(d):
    j, comp = normals[k]
    if j not in pairs:
      pairs[j] = box_muller(block(seed, j, g, chain))
    z[:, k] = pairs[j][comp]
    w = block(seed, invert[k], g, chain)
    u[:, k] = u01(w[0], w[1])
  idx = np.array([at[gc] for gc in gcs])
  return z[idx], u[idx]


def gibbs_uniform_streams(seed, d, tsteps, g0, T, chain_offset, N):
  """gibbs_kernel's Philox uniforms as the replay layout [T, tsteps, N] of
  oracle.run_gibbs: u01(w.x, w.y) of block j at (g, chain) for the j-th
  coordinate of step g (a short last block leaves its spare rows unread)."""
  g, chain = _grid(g0, T, chain_offset, N)
  out = np.empty((T, tsteps, N))
  for j in range(tsteps):
    w = block(seed, j, g, chain)
    out[:, j] = u01(w[0], w[1])
  return out


def gibbs_blocks(d, L, tsteps):
  """The three block sets a Gibbs run of this shape can touch: the normals',
  the inversion draws' and gibbs_kernel's 0 .. tsteps - 1."""
  normals, invert = gibbs_layout(d, L)
  return {j for j, _ in normals}, set(invert), set(range(tsteps))
