// pbh_philox.h -- Philox-4x32-10 pieces shared by device and host code: the
// counter layout, the round keys, and the factored first three rounds for
// several blocks of one (pair / step, chain).
//
// Plain C++: compiles for the host (no device builtin there; a three-input
// xor is two ^) and for the device, where the round function's xors are one
// v_bitop3_b32 each.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PBH_PHILOX_FN __host__ __device__ __forceinline__
#else
#define PBH_PHILOX_FN inline
#endif
#if defined(__clang__)
#define PBH_UNROLL _Pragma("unroll")
#else
#define PBH_UNROLL
#endif

namespace pbh {

struct u32x4 { uint32_t x, y, z, w; };

constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;

PBH_PHILOX_FN uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__builtin_amdgcn_bitop3_b32(a, b, c, 0x96);   // truth table of a ^ b ^ c
#else
  return a ^ b ^ c;
#endif
}

// The counter of block j at step (or step pair) g of a chain: g's high word
// shares the last counter word with the chain id's.
PBH_PHILOX_FN u32x4 philox_ctr(uint32_t j, int64_t g, int64_t chain) {
  return u32x4{j, (uint32_t)g, (uint32_t)chain,
               (uint32_t)((uint64_t)chain >> 32) ^
                   ((uint32_t)((uint64_t)g >> 32) << 16)};
}

// The ten round keys: k0[i] = seed_lo + i W0, k1[i] = seed_hi + i W1.
struct PhiloxKeys { uint32_t k0[10], k1[10]; };

// ---------------------------------------------------------------------------
// Rounds 1-3 factored over the NB blocks j0, j0 + 1, ..., j0 + NB - 1 of one
// (g, chain).  A round maps (x, y, z, w) to
//   (hi(M1 z) ^ y ^ k0, lo(M1 z), hi(M0 x) ^ w ^ k1, lo(M0 x)).
// From the counter (j, g_lo, c_lo, W), W = c_hi ^ (g_hi << 16):
//   round 1: x1 = [hi(M1 c_lo) ^ k0[0]] ^ g_lo        the same for every block
//            y1 = lo(M1 c_lo)                         fixed
//            z1 = hi(M0 j) ^ W ^ k1[0], w1 = lo(M0 j) fixed per block
//   round 2: x2 = hi(M1 z1) ^ y1 ^ k0[1], y2 = lo(M1 z1)   fixed per block
//            z2 = hi(M0 x1) ^ [w1 ^ k1[1]]
//            w2 = lo(M0 x1)                           one product for all blocks
//   round 3: x3 = hi(M1 z2) ^ [y2 ^ k0[2]], y3 = lo(M1 z2)
//            z3 = w2 ^ [hi(M0 x2) ^ k1[2]], w3 = lo(M0 x2)
// The bracketed words and w3 depend on (j, chain, g_hi, seed) alone: one
// shared word and four per block.  With them a new g_lo costs 1 + NB
// multiplies and 1 + 3 NB two-input xors for the NB blocks' rounds 1-3,
// against 6 NB and 6 NB three-input xors.  The words are the plain function's,
// bit for bit.
// ---------------------------------------------------------------------------
template <int NB>
struct PhiloxPrefix {
  uint32_t a;                            // hi(M1 c_lo) ^ k0[0]
  uint32_t b[NB], c[NB], d[NB], e[NB];   // w1 ^ k1[1], y2 ^ k0[2], hi(M0 x2) ^ k1[2], w3
};

template <int NB>
PBH_PHILOX_FN PhiloxPrefix<NB> philox_prefix(uint32_t j0, int64_t chain, uint32_t g_hi,
                                      uint32_t seed_lo, uint32_t seed_hi) {
  const u32x4 c0 = philox_ctr(j0, (int64_t)((uint64_t)g_hi << 32), chain);
  const uint64_t pc = (uint64_t)kPhiloxM1 * c0.z;
  const uint32_t y1 = (uint32_t)pc;
  PhiloxPrefix<NB> p;
  p.a = (uint32_t)(pc >> 32) ^ seed_lo;
PBH_UNROLL
  for (int q = 0; q < NB; ++q) {
    const uint64_t pj = (uint64_t)kPhiloxM0 * (j0 + (uint32_t)q);
    const uint32_t z1 = (uint32_t)(pj >> 32) ^ c0.w ^ seed_hi;
    const uint64_t pz = (uint64_t)kPhiloxM1 * z1;
    const uint32_t x2 = (uint32_t)(pz >> 32) ^ y1 ^ (seed_lo + kPhiloxW0);
    const uint64_t px = (uint64_t)kPhiloxM0 * x2;
    p.b[q] = (uint32_t)pj ^ (seed_hi + kPhiloxW1);
    p.c[q] = (uint32_t)pz ^ (seed_lo + 2u * kPhiloxW0);
    p.d[q] = (uint32_t)(px >> 32) ^ (seed_hi + 2u * kPhiloxW1);
    p.e[q] = (uint32_t)px;
  }
  return p;
}

// Blocks j0 + Q0 .. j0 + NB - 1 at g_lo, words 4 q .. 4 q + 3 of w in order
// (x, y, z, w); the words before block Q0 are set to 0.  Round keys 3..9 of k
// are read, keys 0..2 are inside the prefix.  Equal to
// philox4x32_10(philox_ctr(j0 + q, g, chain)) for the (chain, g_hi, seed) the
// prefix was built from.
template <int NB, int Q0 = 0>
PBH_PHILOX_FN void philox_prefix_blocks(uint32_t g_lo, const PhiloxPrefix<NB> &p,
                                 const PhiloxKeys &k, uint32_t (&w)[4 * NB]) {
  const uint32_t x1 = p.a ^ g_lo;
  const uint64_t p1 = (uint64_t)kPhiloxM0 * x1;
  const uint32_t hi1 = (uint32_t)(p1 >> 32), w2 = (uint32_t)p1;
PBH_UNROLL
  for (int q = 0; q < 4 * Q0; ++q) w[q] = 0u;
PBH_UNROLL
  for (int q = Q0; q < NB; ++q) {
    const uint32_t z2 = hi1 ^ p.b[q];
    const uint64_t p2 = (uint64_t)kPhiloxM1 * z2;
    u32x4 c{(uint32_t)(p2 >> 32) ^ p.c[q], (uint32_t)p2, w2 ^ p.d[q], p.e[q]};
PBH_UNROLL
    for (int i = 3; i < 10; ++i) {
      const uint64_t m0 = (uint64_t)kPhiloxM0 * c.x;
      const uint64_t m1 = (uint64_t)kPhiloxM1 * c.z;
      c = u32x4{xor3((uint32_t)(m1 >> 32), c.y, k.k0[i]), (uint32_t)m1,
                xor3((uint32_t)(m0 >> 32), c.w, k.k1[i]), (uint32_t)m0};
    }
    w[4 * q] = c.x;
    w[4 * q + 1] = c.y;
    w[4 * q + 2] = c.z;
    w[4 * q + 3] = c.w;
  }
}

}  // namespace pbh
