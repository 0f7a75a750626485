// pbh_fft_impl.h -- the 4 096-point fp64 FFT of a workgroup of 256 threads in
// LDS, and its block-wide sum and minimum: device functions shared by the
// per-chain ESS kernels (pbh_dispatch.cpp, where the method is described) and
// the cross-chain ESS kernels (pbh_ess_rank.hip).  Included inside namespace
// pbh; everything is __forceinline__, so each unit keeps its own code.
#pragma once
constexpr int kFftN = 4096, kFftT = 256;   // points, threads
struct cdbl { double re, im; };
__device__ __forceinline__ int fsw(int e) { return e + (e >> 4); }
__device__ __forceinline__ cdbl cadd(cdbl a, cdbl b) { return {a.re + b.re, a.im + b.im}; }
__device__ __forceinline__ cdbl csub(cdbl a, cdbl b) { return {a.re - b.re, a.im - b.im}; }
__device__ __forceinline__ cdbl cmul(cdbl a, cdbl b) {
  return {__builtin_fma(a.re, b.re, -(a.im * b.im)), __builtin_fma(a.re, b.im, a.im * b.re)};
}
__device__ __forceinline__ cdbl conj(cdbl a) { return {a.re, -a.im}; }
// times SIGN i
template <int SIGN>
__device__ __forceinline__ cdbl cmuli(cdbl a) {
  return SIGN > 0 ? cdbl{-a.im, a.re} : cdbl{a.im, -a.re};
}
template <int SIGN>
__device__ __forceinline__ void dft4(cdbl &a0, cdbl &a1, cdbl &a2, cdbl &a3) {
  const cdbl t0 = cadd(a0, a2), t1 = csub(a0, a2), t2 = cadd(a1, a3);
  const cdbl t3 = cmuli<SIGN>(csub(a1, a3));
  a0 = cadd(t0, t2);
  a2 = csub(t0, t2);
  a1 = cadd(t1, t3);
  a3 = csub(t1, t3);
}
// 16-point DFT (exponent sign SIGN) of v; X[k1 + 4 k2] lands in v[4 k1 + k2]
template <int SIGN>
__device__ __forceinline__ void dft16(cdbl (&v)[16]) {
  constexpr double C1 = 0.92387953251128675613, S1 = 0.38268343236508977173;
  constexpr double C2 = 0.70710678118654752440;
#pragma unroll
  for (int n2 = 0; n2 < 4; ++n2) dft4<SIGN>(v[n2], v[4 + n2], v[8 + n2], v[12 + n2]);
  // v[4 k1 + n2] *= W16^(SIGN n2 k1)
  const cdbl w1{C1, SIGN * S1}, w2{C2, SIGN * C2}, w3{S1, SIGN * C1};
  const cdbl w6{-C2, SIGN * C2}, w9{-C1, -SIGN * S1};
  v[5] = cmul(v[5], w1);
  v[6] = cmul(v[6], w2);
  v[7] = cmul(v[7], w3);
  v[9] = cmul(v[9], w2);
  v[10] = cmuli<SIGN>(v[10]);
  v[11] = cmul(v[11], w6);
  v[13] = cmul(v[13], w3);
  v[14] = cmul(v[14], w6);
  v[15] = cmul(v[15], w9);
#pragma unroll
  for (int k1 = 0; k1 < 4; ++k1) dft4<SIGN>(v[4 * k1], v[4 * k1 + 1], v[4 * k1 + 2], v[4 * k1 + 3]);
}
// The arithmetic of one Stockham pass (sub-transform size NS -> 16 NS) on
// the thread's points v[r] = x[j + 256 r]: twiddle, 16-point DFT.  w = exp(SIGN
// 2 pi i m / (16 NS)), m = j % NS.  IN_HALF:
// v[8..15] are zero (the padded series) and are not multiplied.
template <int SIGN, int NS, bool IN_HALF = false>
__device__ __forceinline__ void fft_compute(cdbl (&v)[16], cdbl w) {
  if constexpr (NS > 1) {
    // w^(4 a + b) = w^(4 a) w^b: six powers live, each other one formed
    // just before its product (14 complex products in all)
    const cdbl p1 = w, p2 = cmul(w, w), p3 = cmul(p2, w), p4 = cmul(p2, p2);
    const cdbl p8 = cmul(p4, p4), p12 = cmul(p8, p4);
    const cdbl pb[4] = {cdbl{1., 0.}, p1, p2, p3}, pa[4] = {cdbl{1., 0.}, p4, p8, p12};
#pragma unroll
    for (int r = 1; r < 16; ++r) {
      if (IN_HALF && r >= 8) continue;
      const int a = r >> 2, b = r & 3;
      v[r] = cmul(v[r], a == 0 ? pb[b] : b == 0 ? pa[a] : cmul(pa[a], pb[b]));
    }
  }
  dft16<SIGN>(v);
}
// where a pass leaves output v[i] (i = 4 k1 + k2): base + (k1 + 4 k2) NS
template <int NS>
__device__ __forceinline__ int fft_out(int i) {
  const int j = (int)threadIdx.x;
  return (j / NS) * NS * 16 + (j % NS) + ((i >> 2) + 4 * (i & 3)) * NS;
}
// Move the pass outputs (fft_out<NS>) to the next pass's inputs
// (x[j + 256 r] in v[r]) through sb, real parts then imaginary parts.
template <int NS>
__device__ __forceinline__ void fft_exchange(double *sb, cdbl (&v)[16]) {
  const int j = (int)threadIdx.x;
  double t[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) sb[fsw(fft_out<NS>(i))] = v[i].re;
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 16; ++r) t[r] = sb[fsw(j + r * kFftT)];
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 16; ++i) sb[fsw(fft_out<NS>(i))] = v[i].im;
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 16; ++r) v[r] = cdbl{t[r], sb[fsw(j + r * kFftT)]};
  __syncthreads();
}
// the twiddle bases of passes 2 and 3 (NS = 16, 256) for SIGN = -1; the
// inverse transform's are their conjugates
struct FftTw { cdbl w16, w256; };
__device__ __forceinline__ FftTw fft_twiddles() {
  const int j = (int)threadIdx.x;
  FftTw t;
  double sn, cs;
  sincospi(-(double)(2 * (j % 16)) / 256.0, &sn, &cs);
  t.w16 = cdbl{cs, sn};
  sincospi(-(double)(2 * (j % 256)) / 4096.0, &sn, &cs);
  t.w256 = cdbl{cs, sn};
  return t;
}

// block-wide sum / min over the 256 threads (red: 8 scratch entries)
__device__ __forceinline__ double block_sum(double v, double *red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}
__device__ __forceinline__ int block_min(int v, int *red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  return min(min(red[0], red[1]), min(red[2], red[3]));
}
