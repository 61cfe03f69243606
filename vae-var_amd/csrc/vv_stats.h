// Device functions shared by the statistics kernels: the noise stream of vv_obs_synth / vv_normal_fill / vv_vae_sample
// (one definition, hence one set of bits) and the workgroup sum of the fixed chunk / lane / wave / channel tree of
// vv_errstats.hip and vv_vae.hip. Every function that multiplies then adds turns FP contraction off for itself, so the
// including file's mode does not matter.
#pragma once
#include <hip/hip_runtime.h>

namespace vv {

namespace {

// Philox4x32-10 with the key (seed & 0xffffffff, seed >> 32); counter word 3 is the draw number, word 2 the stream
// (1 the mask keys, 2 the noise), words 0..1 the cell or the group of four elements.
constexpr unsigned kPhM0 = 0xD2511F53u, kPhM1 = 0xCD9E8D57u, kPhW0 = 0x9E3779B9u, kPhW1 = 0xBB67AE85u;
constexpr unsigned kStreamMask = 1u, kStreamNoise = 2u;

__device__ __forceinline__ uint4 philox4x32_10(uint4 c, unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(kPhM0, c.x), lo0 = kPhM0 * c.x;
    const unsigned hi1 = __umulhi(kPhM1, c.z), lo1 = kPhM1 * c.z;
    c = make_uint4(hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0);
    k0 += kPhW0;
    k1 += kPhW1;
  }
  return c;
}

// Box-Muller on two words: u1 = ((wa >> 8) + 1) 2^-24 in (0, 1], 2 u2 = (wb >> 8) 2^-23 in [0, 2), both exact;
// every product rounds on its own
__device__ __forceinline__ void synth_pair(unsigned wa, unsigned wb, float& c, float& s) {
#pragma clang fp contract(off)
  const float u1 = (float)((wa >> 8) + 1u) * 0x1p-24f, a = (float)(wb >> 8) * 0x1p-23f;
  const float r = __fsqrt_rn(-2.0f * logf(u1));
  c = r * cospif(a);
  s = r * sinpif(a);
}
// eps of the four elements 4 g .. 4 g + 3: the one definition every kernel uses
__device__ __forceinline__ void synth_eps4(unsigned k0, unsigned k1, unsigned draw, unsigned long long g, float* ep) {
  const uint4 w = philox4x32_10(make_uint4((unsigned)g, (unsigned)(g >> 32), kStreamNoise, draw), k0, k1);
  synth_pair(w.x, w.y, ep[0], ep[1]);
  synth_pair(w.z, w.w, ep[2], ep[3]);
}

// the fixed tree inside a workgroup of 256: lanes by shuffles, then the four waves in order; every thread returns the
// workgroup's sum. red: four doubles of LDS
__device__ __forceinline__ double err_block_sum(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const double t = ((red[0] + red[1]) + red[2]) + red[3];
  __syncthreads();
  return t;
}

}  // namespace

}  // namespace vv
