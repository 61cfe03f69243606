// Departure statistics of an assimilation window on the device (include/vaevar.h vv_obs_stats): per
// time level t and observation channel c the fp64 sums, over the observed entries S = {p : Hmask[t][c][p] != 0}, of
// 1, h, d_b, d_a, d_b^2, d_a^2, d_a d_b, r and the J_o terms (h (d d)) / r, with d_b = yo - H(xb), d_a = yo - H(xa).
// These are the moments the consistency relations of Desroziers et al. (2005) are formed from.
//
// Decomposition: the (t, c) planes are walked in the chunk layout of vv_stats.h (ChunkWalk), one workgroup per plane
// and chunk of kErrChunk cells, chunk-major: the workgroups of all planes that share a chunk of pixels are neighbours
// in the grid, so with a level operator the level columns of a pixel, which every channel of a variable gathers again,
// are served by the cache. A thread reads its four consecutive Hmask cells (the only dense read) and, where h != 0,
// yo, R and the state: channel c itself for the identity or a surface channel, else the variable's n_in level column in
// registers and k_obs_augment's sum with row o of the operator; the loads of a group's observed cells are issued
// together (one 16-byte access each when all four are observed on the 16-byte path). Ten fp64 accumulators a thread,
// cells ascending; then lanes, waves (err_block_sum) and, in k_obs_stats_final, the chunks of a plane ascending. No
// atomics. A plane's sums see only its own entries and the pixel -> (chunk, wave, lane) map is the same for every
// plane, so a row's bits depend neither on T nor on the other channels.
#include <cmath>

#include "vv_kernels.h"
#include "vv_stats.h"  // ChunkWalk, load4, err_block_sum

namespace vv {

namespace {

// rows of a table (include/vaevar.h VV_OSTAT_*)
enum { OS_COUNT = 0, OS_H, OS_OB, OS_OA, OS_OB2, OS_OA2, OS_OAOB, OS_R, OS_JB, OS_JA };
static_assert(OS_JA + 1 == kObsStatN, "ten rows");

// the cells p[e] with bit e of m set; the others are not read and come back as 0. ALL: m == 15 and p is 16-byte
// aligned: one 16-byte access
template <bool ALL>
__device__ __forceinline__ void load4m(const float* p, unsigned m, float* v) {
  if (ALL) {
    load4<true>(p, 4, v);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (m >> e) & 1u ? p[e] : 0.0f;
  }
}

// (Op x)[c] at the cells p + e of the mask m: col points at channel c (identity, surface) or at level 0 of the
// variable's column. The operator sum is k_obs_augment's statement (vv_ops.hip): the column first, then y = 0 and
// y += P[o][j] * x[j] for j ascending under the file's default contraction, so the two round alike. The loads of the
// group's columns are issued together, whichever of its cells are observed
template <bool ALL>
__device__ __forceinline__ void obs_value(const float* col, const float* pr, int nin, bool op, int HW, long long p,
                                          unsigned m, float* y) {
  if (!op) {
    load4m<ALL>(col + p, m, y);
    return;
  }
  float xs[kObsMaxIn][4];
#pragma unroll
  for (int j = 0; j < kObsMaxIn; ++j) {
    if (j < nin) {
      load4m<ALL>(col + (size_t)j * HW + p, m, xs[j]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) xs[j][e] = 0.0f;
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float v = 0.0f;
#pragma unroll
    for (int j = 0; j < kObsMaxIn; ++j)
      if (j < nin) v += pr[j] * xs[j][e];
    y[e] = v;
  }
}

// one observed entry: every fp32 operation rounds on its own; the fp64 products of widened fp32 values are exact
__device__ __forceinline__ void stat_entry(float h, float yo, float r, float xb, float xa, bool has_a, double* s) {
#pragma clang fp contract(off)
  const float db = yo - xb;
  const double wb = (double)db;
  s[OS_COUNT] += 1.0;
  s[OS_H] += (double)h;
  s[OS_OB] += wb;
  s[OS_OB2] += wb * wb;
  s[OS_R] += (double)r;
  s[OS_JB] += (double)((h * (db * db)) / r);
  if (has_a) {
    const float da = yo - xa;
    const double wa = (double)da;
    s[OS_OA] += wa;
    s[OS_OA2] += wa * wa;
    s[OS_OAOB] += wa * wb;
    s[OS_JA] += (double)((h * (da * da)) / r);
  }
}

// grid: nck * T * Ca workgroups of 256, workgroup k * rows + row takes chunk k of plane row = t * Ca + c. VEC: HW is
// a multiple of four and every field is 16-byte aligned
template <bool VEC>
__global__ __launch_bounds__(256) void k_obs_stats(ObsStatsArgs a) {
  __shared__ double red[4];
  const unsigned rows = (unsigned)(a.T * a.Ca);
  const unsigned k = blockIdx.x / rows, row = blockIdx.x - k * rows;
  const ChunkWalk w(row, k);
  const unsigned t = row / (unsigned)a.Ca, c = row - t * (unsigned)a.Ca;
  const int HW = a.HW, nin = a.nin;
  const bool op = a.P != nullptr && c >= 4u, has_a = a.xa != nullptr;
  float pr[kObsMaxIn];
#pragma unroll
  for (int j = 0; j < kObsMaxIn; ++j) pr[j] = 0.0f;
  size_t xc = c;  // the state channel the plane reads, or level 0 of its column
  if (op) {
    const unsigned v = (c - 4u) / (unsigned)a.nout, o = (c - 4u) - v * (unsigned)a.nout;
    xc = 4u + (unsigned)nin * v;
#pragma unroll
    for (int j = 0; j < kObsMaxIn; ++j)
      if (j < nin) pr[j] = a.P[o * nin + j];
  }
  const size_t plane = (size_t)row * HW, col = ((size_t)t * a.C + xc) * HW;
  const float* Hm = a.Hm + plane;
  const float* yo = a.yo + plane;
  const float* R = a.R + plane;
  const float* xb = a.xb + col;
  const float* xa = has_a ? a.xa + col : nullptr;
  double s[kObsStatN];
#pragma unroll
  for (int i = 0; i < kObsStatN; ++i) s[i] = 0.0;
  w.each<VEC>(HW, [&](long long p0, int n) {
    float h[4];
    load4<VEC>(Hm + p0, n, h);  // cells past the plane come back as 0: unobserved
    unsigned m = 0u;  // the group's observed cells
#pragma unroll
    for (int e = 0; e < 4; ++e) m |= h[e] != 0.0f ? 1u << e : 0u;
    if (m == 0u) return;
    float y4[4], r4[4], b4[4], a4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (VEC && m == 15u) {
      load4m<true>(yo + p0, m, y4);
      load4m<true>(R + p0, m, r4);
      obs_value<true>(xb, pr, nin, op, HW, p0, m, b4);
      if (has_a) obs_value<true>(xa, pr, nin, op, HW, p0, m, a4);
    } else {
      load4m<false>(yo + p0, m, y4);
      load4m<false>(R + p0, m, r4);
      obs_value<false>(xb, pr, nin, op, HW, p0, m, b4);
      if (has_a) obs_value<false>(xa, pr, nin, op, HW, p0, m, a4);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if ((m >> e) & 1u) stat_entry(h[e], y4[e], r4[e], b4[e], a4[e], has_a, s);
  });
  double* out = a.partial + ((size_t)row * a.nck + k) * kObsStatN;
#pragma unroll
  for (int i = 0; i < kObsStatN; ++i) {
    const double tot = err_block_sum(s[i], red);
    if (threadIdx.x == 0) out[i] = tot;
  }
}

// one workgroup per plane: per row of the table thread i adds the chunk sums i, i + 256, ... in ascending order, then
// the fixed tree (k_err_chan's order). Without an analysis its four rows are NaN
__global__ __launch_bounds__(256) void k_obs_stats_final(const double* partial, unsigned nck, int has_a, double* out) {
#pragma clang fp contract(off)
  __shared__ double red[4];
  const double* part = partial + (size_t)blockIdx.x * nck * kObsStatN;
  for (int i = 0; i < kObsStatN; ++i) {
    double s = 0.0;
    for (unsigned q = threadIdx.x; q < nck; q += 256) s += part[(size_t)q * kObsStatN + i];
    const double tot = err_block_sum(s, red);
    const bool ana = i == OS_OA || i == OS_OA2 || i == OS_OAOB || i == OS_JA;
    if (threadIdx.x == 0) out[(size_t)blockIdx.x * kObsStatN + i] = ana && !has_a ? (double)NAN : tot;
  }
}

}  // namespace

hipError_t obs_stats(const ObsStatsArgs& in, hipStream_t s) {
  ObsStatsArgs a = in;
  if (!a.xb || !a.yo || !a.Hm || !a.R || !a.partial || !a.out || a.T < 1 || a.C < 1 || a.HW < 1 ||
      a.HW > 0x7fffffff - kErrChunk)
    return hipErrorInvalidValue;
  if (a.P) {
    if (a.nin < 1 || a.nin > kObsMaxIn || a.nout < 1 || a.nout > kObsMaxOut || a.C != 4 + 5 * a.nin)
      return hipErrorInvalidValue;
    a.Ca = 4 + 5 * a.nout;
  } else {
    a.Ca = a.C;
    a.nin = a.nout = 0;
  }
  a.nck = err_chunks(a.HW);
  const long long rows = (long long)a.T * a.Ca, blocks = rows * a.nck;
  if (blocks >= 0x80000000LL) return hipErrorInvalidValue;
  const int ph = prof_begin(s);
  const bool vec = a.HW % 4 == 0 && aligned16(a.xb) && aligned16(a.xa) && aligned16(a.yo) && aligned16(a.Hm) &&
                   aligned16(a.R);
  hipLaunchKernelGGL(vec ? k_obs_stats<true> : k_obs_stats<false>, dim3((unsigned)blocks), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_obs_stats_final, dim3((unsigned)rows), dim3(256), 0, s, a.partial, a.nck, a.xa ? 1 : 0, a.out);
  // a fully observed window: Hmask, yo and R once, each state once; per entry the operator sums and about a dozen
  // fp32 / fp64 operations a state
  const double na = a.xa ? 2.0 : 1.0;
  prof_end(ph, s, PC_MISFIT, (double)a.T * a.HW * a.Ca * (na * (2.0 * (a.P ? a.nin : 0) + 10.0) + 3.0),
           4.0 * (double)a.HW * a.T * (3.0 * a.Ca + na * a.C));
  return hipGetLastError();
}

}  // namespace vv
