// Stand-alone check of pbh_philox.h's factored first rounds on the host:
// philox_prefix + philox_prefix_blocks against a ten-round Philox-4x32-10
// written here from the published definition (Salmon et al., SC'11), on random
// (seed, h, P, chain) and on the corners of P and chain.
//
// usage: philox_prefix_main <draws>; prints "ok <blocks compared>" or the
// first mismatch, exit status 0 / 1.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "pbh_philox.h"

namespace {

// the plain function: counter c, key (k0, k1), ten rounds
void philox_plain(const uint32_t (&c)[4], uint32_t k0, uint32_t k1, uint32_t (&out)[4]) {
  uint32_t x = c[0], y = c[1], z = c[2], w = c[3];
  for (int i = 0; i < 10; ++i) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * x, p1 = (uint64_t)0xCD9E8D57u * z;
    const uint32_t nx = (uint32_t)(p1 >> 32) ^ y ^ k0, nz = (uint32_t)(p0 >> 32) ^ w ^ k1;
    y = (uint32_t)p1;
    w = (uint32_t)p0;
    x = nx;
    z = nz;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = x;
  out[1] = y;
  out[2] = z;
  out[3] = w;
}

uint64_t rng_state = 0x243F6A8885A308D3ull;
uint64_t next64() {   // SplitMix64
  uint64_t x = (rng_state += 0x9E3779B97F4A7C15ull);
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

long long compared = 0;

// every block Q0 .. NB-1 of (seed, h, P, chain) against the plain function
template <int NB, int Q0>
bool check_from(uint64_t seed, uint32_t h, int64_t P, int64_t chain) {
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  pbh::PhiloxKeys rk;
  for (int i = 0; i < 10; ++i) {
    rk.k0[i] = k0 + (uint32_t)i * 0x9E3779B9u;
    rk.k1[i] = k1 + (uint32_t)i * 0xBB67AE85u;
  }
  // keys 0..2 belong to the prefix: the block function must not read them
  for (int i = 0; i < 3; ++i) rk.k0[i] = rk.k1[i] = 0xDEADBEEFu;
  const pbh::PhiloxPrefix<NB> pre = pbh::philox_prefix<NB>(
      16u * h, chain, (uint32_t)((uint64_t)P >> 32), k0, k1);
  uint32_t w[4 * NB];
  for (int q = 0; q < 4 * NB; ++q) w[q] = 0xA5A5A5A5u;
  pbh::philox_prefix_blocks<NB, Q0>((uint32_t)P, pre, rk, w);
  for (int q = 0; q < 4 * Q0; ++q)
    if (w[q] != 0u) {
      std::printf("word %d before block %d not cleared (NB %d)\n", q, Q0, NB);
      return false;
    }
  for (int q = Q0; q < NB; ++q) {
    // the counter of block j = q + 16 h at pair P of the chain
    const uint32_t c[4] = {(uint32_t)q + 16u * h, (uint32_t)P, (uint32_t)chain,
                           (uint32_t)((uint64_t)chain >> 32) ^
                               ((uint32_t)((uint64_t)P >> 32) << 16)};
    uint32_t want[4];
    philox_plain(c, k0, k1, want);
    const pbh::u32x4 cc = pbh::philox_ctr((uint32_t)q + 16u * h, P, chain);
    if (cc.x != c[0] || cc.y != c[1] || cc.z != c[2] || cc.w != c[3]) {
      std::printf("philox_ctr differs\n");
      return false;
    }
    for (int e = 0; e < 4; ++e)
      if (w[4 * q + e] != want[e]) {
        std::printf("mismatch NB %d Q0 %d block %d word %d: got %08x want %08x "
                    "(seed %016" PRIx64 " h %u P %016" PRIx64 " chain %016" PRIx64 ")\n",
                    NB, Q0, q, e, w[4 * q + e], want[e], seed, h, (uint64_t)P, (uint64_t)chain);
        return false;
      }
    ++compared;
  }
  return true;
}

// the first blocks in use: 0 (whole pairs) and the launch that starts on a
// pair's second step, block 3 (H / 2) / 4 with H = (4 NB - 1) / 3 rounded to
// the kernel's d (NB = 2, 4, 7 <-> d = 4, 10, 16: Q0 = 0, 1, 3); every other
// Q0 < NB is checked as well
template <int NB, int Q0 = 0>
bool check_all(uint64_t seed, uint32_t h, int64_t P, int64_t chain) {
  if (!check_from<NB, Q0>(seed, h, P, chain)) return false;
  if constexpr (Q0 + 1 < NB) return check_all<NB, Q0 + 1>(seed, h, P, chain);
  else return true;
}

bool check(uint64_t seed, uint32_t h, int64_t P, int64_t chain) {
  return check_all<2>(seed, h, P, chain) && check_all<4>(seed, h, P, chain) &&
         check_all<7>(seed, h, P, chain);
}

}  // namespace

int main(int argc, char **argv) {
  const long draws = argc > 1 ? std::atol(argv[1]) : 100000;
  // the published known-answer vector of Philox-4x32-10 (counter 0, key 0)
  {
    const uint32_t c[4] = {0u, 0u, 0u, 0u};
    uint32_t out[4];
    philox_plain(c, 0u, 0u, out);
    if (out[0] != 0x6627e8d5u || out[1] != 0xe169c58du || out[2] != 0xbc57ac4cu ||
        out[3] != 0x9b00dbd8u) {
      std::printf("the plain function misses the known answer\n");
      return 1;
    }
  }
  // corners: P_lo 0 and 0xFFFFFFFF with P_hi 0, 1 and large; chain_hi 0 / not
  const uint64_t p_lo[] = {0u, 0xFFFFFFFFu, 1u, 0x80000000u};
  const uint64_t p_hi[] = {0u, 1u, 0x7FFFu, 0xFFFFu};
  const uint64_t chains[] = {0u, 31u, 0xFFFFFFFFull, 0x100000000ull, 0x1234ABCD00000007ull,
                             0x7FFFFFFFFFFFFFFFull};
  for (uint64_t lo : p_lo)
    for (uint64_t hi : p_hi)
      for (uint64_t ch : chains)
        for (uint32_t h = 0; h < 2; ++h)
          if (!check(next64(), h, (int64_t)((hi << 32) | lo), (int64_t)ch)) return 1;
  for (long i = 0; i < draws; ++i) {
    const uint64_t seed = next64(), r = next64();
    const uint32_t h = (uint32_t)(r & 1u);
    // a third of the draws each: small, 2^32-straddling and full-width P / chain
    const int kind = (int)((r >> 1) % 3u);
    uint64_t P = next64() >> 1, chain = next64() >> 1;
    if (kind == 0) {
      P &= 0xFFFFFFFFull;
      chain &= 0xFFFFFFFFull;
    } else if (kind == 1) {
      P = 0x100000000ull - 64 + (P & 127u);
      chain = 0x100000000ull - 64 + (chain & 127u);
    }
    // one draw in eight at an end of P's low word
    if (((r >> 8) & 7u) == 0u) P = (P & ~0xFFFFFFFFull) | ((r & 4u) ? 0xFFFFFFFFull : 0ull);
    if (!check(seed, h, (int64_t)P, (int64_t)chain)) return 1;
  }
  std::printf("ok %lld\n", compared);
  return 0;
}
