// Device functions shared by the statistics kernels: the noise stream of vv_obs_synth / vv_normal_fill / vv_vae_sample
// (one definition, hence one set of bits), the chunk walk of vv_errstats.hip and vv_vae.hip with its four-cell
// accesses, and the workgroup sum of their fixed chunk / lane / wave / channel tree. Every function that multiplies
// then adds turns FP contraction off for itself, so the including file's mode does not matter.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "vv_kernels.h"  // kErrChunk

namespace vv {

namespace {

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Four consecutive cells in registers. VEC: the address is 16-byte aligned and all four are valid: one 16-byte access
// (two for double). Otherwise n = 1..4 of them are valid and move one by one; a load zeroes the rest
template <bool VEC>
__device__ __forceinline__ void load4(const float* p, int n, float* v) {
  if (VEC) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = e < n ? p[e] : 0.0f;
  }
}
template <bool VEC>
__device__ __forceinline__ void load4(const double* p, int n, double* v) {
  if (VEC) {
    const double2 lo = *reinterpret_cast<const double2*>(p), hi = *reinterpret_cast<const double2*>(p + 2);
    v[0] = lo.x, v[1] = lo.y, v[2] = hi.x, v[3] = hi.y;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = e < n ? p[e] : 0.0;
  }
}
template <bool VEC>
__device__ __forceinline__ void store4(float* p, int n, const float* v) {
  if (VEC) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (e < n) p[e] = v[e];
  }
}
template <bool VEC>
__device__ __forceinline__ void store4(double* p, int n, const double* v) {
  if (VEC) {
    *reinterpret_cast<double2*>(p) = make_double2(v[0], v[1]);
    *reinterpret_cast<double2*>(p + 2) = make_double2(v[2], v[3]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (e < n) p[e] = v[e];
  }
}

// The chunk layout: a plane of HW cells is cut into chunks of kErrChunk cells, one workgroup of 256 each; the grid is
// rows * nck workgroups and workgroup row * nck + k takes cells [k kErrChunk, (k + 1) kErrChunk) of plane `row`. A
// thread owns kErrItems groups of four consecutive cells, 256 groups apart, and visits them in ascending order
constexpr int kErrItems = kErrChunk / (256 * 4);

struct ChunkWalk {
  unsigned row, k;
  __device__ __forceinline__ explicit ChunkWalk(unsigned nck) : row(blockIdx.x / nck), k(blockIdx.x - row * nck) {}
  // a kernel that orders its workgroups otherwise (vv_obsstats.hip: chunk-major) names its plane and chunk itself
  __device__ __forceinline__ ChunkWalk(unsigned row_, unsigned k_) : row(row_), k(k_) {}
  // f(p0, n) for each of the thread's groups that begins inside the plane: p0 its first cell, n its valid cells (4 on
  // the 16-byte path, where HW is a multiple of four)
  template <bool VEC, class F>
  __device__ __forceinline__ void each(int HW, F&& f) const {
#pragma unroll
    for (int i = 0; i < kErrItems; ++i) {
      const long long p0 = (long long)k * kErrChunk + ((long long)i * 256 + threadIdx.x) * 4;
      if (p0 >= HW) break;
      f(p0, VEC || HW - p0 >= 4 ? 4 : (int)(HW - p0));
    }
  }
};

// launches the 16-byte (vec) or the element instantiation of a chunk kernel on rows * nck workgroups of 256
template <class A>
inline void chunk_launch(bool vec, void (*k16)(A), void (*k1)(A), unsigned rows, unsigned nck, hipStream_t s,
                         const A& a) {
  hipLaunchKernelGGL(vec ? k16 : k1, dim3(rows * nck), dim3(256), 0, s, a);
}

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
