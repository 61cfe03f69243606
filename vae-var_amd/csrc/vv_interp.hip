// da_mode 'interpolation' on the device (one_step_DA, da_4dvar.py:968-1061; include/vaevar.h vv_tri_interp and
// vv_obs_project). The reference calls scipy's griddata(method='linear') per observation channel: a Delaunay
// triangulation of the observed cells and, per unobserved cell, a point location and a barycentric sum. The host keeps
// the triangulation (a few thousand points); everything dense happens here.
//
// Query points and vertices are both lattice cells, so the inside test and the barycentric weights of a cell are exact
// integer edge functions of the simplex: no point location structure, no floating-point inside test. A cell on an edge
// or a vertex lies in several simplices; it goes to the one with the lowest table row, which every simplex decides for
// itself from its neighbour across that edge (row < neighbour, or no neighbour): one writer per cell, no owner map, no
// atomics on the field, and the same bits on every call.
//
// Work distribution. A station triangulation has thousands of simplices of a few cells and a handful whose bounding
// boxes span an ocean. A box is cut into tiles of kTriBand rows x kTriSeg columns; a work item is (simplex, tile),
// numbered by the table's prefix columns (work_begin, work_end), which the host fills while packing. The grid is fixed
// (the total is known on the device only, the call does not synchronise): a wave takes chunks of kTriChunk consecutive
// work items round-robin, finds a chunk's first simplex by one binary search of work_begin and walks the rows from
// there. Lanes run along the columns of a tile, so the Hmask reads and xa writes of a row segment coalesce; the cells
// of a tile outside its simplex cost a dozen integer operations and no memory access.
//
// The table is not trusted. Every row is validated before a cell of it is touched (channel, the six coordinates, the
// three neighbours, a non-zero area), and a tile's cells lie inside the bounding box of validated coordinates; the
// prefix columns only select which (row, tile) pairs a wave visits, each tile index is checked against the tile count
// the row's own coordinates give, and every loop over rows is bounded. A malformed prefix can lose cells, it cannot
// move a write.
#include "vv_kernels.h"

namespace vv {

namespace {

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

struct TriRow {
  int ch, r0, c0, r1, c1, r2, c2, n0, n1, n2, begin, end;
};
__device__ __forceinline__ TriRow tri_load(const int* __restrict__ tris, int t) {
  const int* q = tris + (size_t)t * kTriCols;
  TriRow w;
  w.ch = q[0], w.r0 = q[1], w.c0 = q[2], w.r1 = q[3], w.c1 = q[4], w.r2 = q[5], w.c2 = q[6];
  w.n0 = q[7], w.n1 = q[8], w.n2 = q[9], w.begin = q[10], w.end = q[11];
  return w;
}
__device__ __forceinline__ bool tri_in(int v, int size) { return (unsigned)v < (unsigned)size; }
// whether the row may be used; A, the doubled signed area, is formed only from coordinates known to lie in the grid
// (|A| < 2^30 for Hs, Ws <= kTriMaxDim)
__device__ __forceinline__ bool tri_ok(const TriRow& w, int n, int C, int Hs, int Ws, int& A) {
  A = 0;
  if (!tri_in(w.ch, C) || !tri_in(w.r0, Hs) || !tri_in(w.r1, Hs) || !tri_in(w.r2, Hs) || !tri_in(w.c0, Ws) ||
      !tri_in(w.c1, Ws) || !tri_in(w.c2, Ws))
    return false;
  if (w.n0 < -1 || w.n0 >= n || w.n1 < -1 || w.n1 >= n || w.n2 < -1 || w.n2 >= n) return false;
  A = (w.r1 - w.r0) * (w.c2 - w.c0) - (w.c1 - w.c0) * (w.r2 - w.r0);
  return A != 0;
}
__device__ __forceinline__ int min3(int a, int b, int c) { return min(a, min(b, c)); }
__device__ __forceinline__ int max3(int a, int b, int c) { return max(a, max(b, c)); }

// one add to a counter per wave: the number of lanes with `flag`
__device__ __forceinline__ void tri_count(long long* counter, bool flag) {
  const unsigned long long m = __ballot(flag);
  if (m != 0ull && (threadIdx.x & 63) == __builtin_ctzll(m))
    atomicAdd(reinterpret_cast<unsigned long long*>(counter), (unsigned long long)__popcll(m));
}

__global__ __launch_bounds__(256) void k_tri_rows(const int* __restrict__ tris, int n, int C, int Hs, int Ws,
                                                  long long* stats) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  int st = -1, A;
  if (t < n) st = tri_ok(tri_load(tris, (int)t), n, C, Hs, Ws, A) ? 0 : 1;
  tri_count(stats + 0, st == 0);
  tri_count(stats + 1, st == 1);
}

__global__ __launch_bounds__(256) void k_tri_raster(const int* __restrict__ tris, int n, const float* __restrict__ yo,
                                                    const float* __restrict__ Hm, float* __restrict__ xa, int C, int Hs,
                                                    int Ws, long long* stats) {
  const int lane = threadIdx.x & 63;
  const int wave = uni(blockIdx.x * 4 + (threadIdx.x >> 6)), nwaves = gridDim.x * 4;
  const long long total = uni(tris[(size_t)(n - 1) * kTriCols + 11]);  // only bounds the loop below
  const size_t HW = (size_t)Hs * Ws;
  long long written = 0;
  for (long long w0 = (long long)wave * kTriChunk; w0 < total; w0 += (long long)nwaves * kTriChunk) {
    const long long w1 = w0 + kTriChunk < total ? w0 + kTriChunk : total;
    int lo = 0, hi = n;  // the last row with work_begin <= w0
    while (hi - lo > 1) {
      const int mid = lo + (hi - lo) / 2;
      if (uni(tris[(size_t)mid * kTriCols + 10]) <= w0) lo = mid;
      else hi = mid;
    }
    // every row has a work item, so the chunk ends within kTriChunk rows
    for (int t = lo; t < n && t - lo <= kTriChunk; ++t) {
      TriRow w = tri_load(tris, t);
      w.ch = uni(w.ch), w.r0 = uni(w.r0), w.c0 = uni(w.c0), w.r1 = uni(w.r1), w.c1 = uni(w.c1), w.r2 = uni(w.r2);
      w.c2 = uni(w.c2), w.n0 = uni(w.n0), w.n1 = uni(w.n1), w.n2 = uni(w.n2), w.begin = uni(w.begin);
      w.end = uni(w.end);
      if (w.begin >= w1) break;
      int A;
      if (!tri_ok(w, n, C, Hs, Ws, A)) continue;
      const int rmin = min3(w.r0, w.r1, w.r2), rmax = max3(w.r0, w.r1, w.r2);
      const int cmin = min3(w.c0, w.c1, w.c2), cmax = max3(w.c0, w.c1, w.c2);
      const int ns = (cmax - cmin) / kTriSeg + 1;
      const long long ntile = (long long)((rmax - rmin) / kTriBand + 1) * ns;
      long long k0 = (w0 > w.begin ? w0 : (long long)w.begin) - w.begin;
      long long k1 = (w1 < w.end ? w1 : (long long)w.end) - w.begin;
      if (k1 > ntile) k1 = ntile;
      if (k0 >= k1) continue;
      const size_t base = (size_t)w.ch * HW;
      const double v0 = (double)yo[base + (size_t)w.r0 * Ws + w.c0];
      const double v1 = (double)yo[base + (size_t)w.r1 * Ws + w.c1];
      const double v2 = (double)yo[base + (size_t)w.r2 * Ws + w.c2];
      const int sg = A > 0 ? 1 : -1, As = A * sg;
      const double Ad = (double)As;
      // a cell on the edge opposite vertex k is this row's if the hull or a later row lies across it
      const bool own0 = w.n0 == -1 || t < w.n0, own1 = w.n1 == -1 || t < w.n1, own2 = w.n2 == -1 || t < w.n2;
      for (long long k = k0; k < k1; ++k) {
        const int band = (int)(k / ns), seg = (int)(k - (long long)band * ns);
        const int c = cmin + seg * kTriSeg + lane;
        const int rb = rmin + band * kTriBand, re = min(rmax, rb + kTriBand - 1);
        if (c > cmax) continue;
        for (int r = rb; r <= re; ++r) {
          const int e0 = ((w.r1 - r) * (w.c2 - c) - (w.c1 - c) * (w.r2 - r)) * sg;
          const int e1 = ((w.r2 - r) * (w.c0 - c) - (w.c2 - c) * (w.r0 - r)) * sg;
          const int e2 = As - e0 - e1;
          if (e0 < 0 || e1 < 0 || e2 < 0) continue;
          if ((e0 == 0 && !own0) || (e1 == 0 && !own1) || (e2 == 0 && !own2)) continue;
          const size_t i = base + (size_t)r * Ws + c;
          if (!(Hm[i] == 0.0f)) continue;
          // ((e0 v0 + e1 v1) + e2 v2) / A, every operation rounded on its own, then once to fp32
          const double num = __dadd_rn(__dadd_rn(__dmul_rn((double)e0, v0), __dmul_rn((double)e1, v1)),
                                       __dmul_rn((double)e2, v2));
          const double q = __ddiv_rn(num, Ad);
          if (q != q) continue;
          xa[i] = (float)q;
          ++written;
        }
      }
    }
  }
  if (stats) {
    for (int off = 32; off > 0; off >>= 1) written += __shfl_down(written, off);
    if (lane == 0 && written)
      atomicAdd(reinterpret_cast<unsigned long long*>(stats + 2), (unsigned long long)written);
  }
}

// x[4 + nout v + o] = sum_j P[o][j] x_aug[4 + nin v + j], j ascending, fp32; channels 0..3 copied
__global__ __launch_bounds__(256) void k_obs_project(const float* __restrict__ P, int nin, int nout,
                                                     const float* __restrict__ xa, float* __restrict__ x, int HW) {
  __shared__ float Ps[kProjMaxOut * kProjMaxIn];
  for (int i = threadIdx.x; i < nout * nin; i += 256) Ps[i] = P[i];
  __syncthreads();
  const float* xt = xa + (size_t)blockIdx.y * (4 + 5 * nin) * HW;
  float* yt = x + (size_t)blockIdx.y * (4 + 5 * nout) * HW;
  for (int p = blockIdx.x * 256 + threadIdx.x; p < HW; p += gridDim.x * 256) {
#pragma unroll
    for (int c = 0; c < 4; ++c) yt[(size_t)c * HW + p] = xt[(size_t)c * HW + p];
    for (int v = 0; v < 5; ++v) {
      float acc[kProjMaxOut];
#pragma unroll
      for (int o = 0; o < kProjMaxOut; ++o) acc[o] = 0.0f;
      for (int j = 0; j < nin; ++j) {
        const float xj = xt[(size_t)(4 + nin * v + j) * HW + p];
#pragma unroll
        for (int o = 0; o < kProjMaxOut; ++o)
          if (o < nout) acc[o] += Ps[o * nin + j] * xj;
      }
#pragma unroll
      for (int o = 0; o < kProjMaxOut; ++o)
        if (o < nout) yt[(size_t)(4 + nout * v + o) * HW + p] = acc[o];
    }
  }
}

}  // namespace

hipError_t tri_interp(const TriInterpArgs& a, hipStream_t s) {
  if (!a.yo || !a.Hm || !a.xa || a.n < 0 || a.n > 0x7fffffffLL || (a.n > 0 && !a.tris) || a.C < 1 || a.Hs < 1 ||
      a.Ws < 1 || a.Hs > kTriMaxDim || a.Ws > kTriMaxDim)
    return hipErrorInvalidValue;
  const int ph = prof_begin(s);
  if (a.stats) {
    hipError_t e = hipMemsetAsync(a.stats, 0, 3 * sizeof(long long), s);
    if (e != hipSuccess) return e;
  }
  if (a.n > 0) {
    const int n = (int)a.n;
    if (a.stats)
      hipLaunchKernelGGL(k_tri_rows, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, s, a.tris, n, a.C, a.Hs, a.Ws,
                         a.stats);
    const long long blocks = std::min(2048LL, std::max(64LL, (a.n + 3) / 4));
    hipLaunchKernelGGL(k_tri_raster, dim3((unsigned)blocks), dim3(256), 0, s, a.tris, n, a.yo, a.Hm, a.xa, a.C, a.Hs,
                       a.Ws, a.stats);
  }
  // the unobserved cells inside the hulls: Hmask read and xa written once; the table read once
  const double cells = (double)a.C * a.Hs * a.Ws;
  prof_end(ph, s, PC_MISFIT, 12.0 * cells, 8.0 * cells + 48.0 * (double)a.n);
  return hipGetLastError();
}

hipError_t obs_project(const float* P, int nin, int nout, const float* x_aug, float* x, int T, int HW,
                       hipStream_t s) {
  if (nin < 1 || nin > kProjMaxIn || nout < 1 || nout > kProjMaxOut || T < 1 || HW < 1) return hipErrorInvalidValue;
  const int ph = prof_begin(s);
  hipLaunchKernelGGL(k_obs_project, dim3(std::min((HW + 255) / 256, 2048), T), dim3(256), 0, s, P, nin, nout, x_aug, x,
                     HW);
  prof_end(ph, s, PC_MISFIT, 10.0 * nin * nout * (double)T * HW, 4.0 * (double)T * HW * (8 + 5 * (nin + nout)));
  return hipGetLastError();
}

}  // namespace vv
