// Model-error statistics and the static R on the device (calculate_q, model/model.py:469-490; init_q_matrix,
// da_4dvar.py:528-550; get_static_info's R, :630-634; get_R_matrix_from_gt, :729-756; include/vaevar.h vv_err_accum,
// vv_err_finalize, vv_r_fill).
//
// Accumulate: the planes are walked in the chunk layout of vv_stats.h (ChunkWalk). A thread owns its cells
// for the whole call and takes the B samples in order, so cell += (double)((pred - tgt)^2) is the reference's numpy
// loop word for word. The signed differences go to a per-thread fp64 sum (cells ascending, samples inside a cell),
// then lanes, waves and chunks are added in a fixed tree: k_err_chan adds the chunk sums of a channel in ascending
// order onto chan[c]. No atomics anywhere, so two runs give the same bits.
//
// Finalize: q = cell / n per cell (IEEE division) and the same chunk / channel tree for the plane mean.
//
// Fill: R[t][c][p] = the table value of plane (t, c); with the level operator the value of an interpolated channel is
// k_obs_augment's sum over the 13 model levels, formed once per workgroup from the table row. The kernel only stores.
#include "vv_kernels.h"
#include "vv_stats.h"  // ChunkWalk, load4 / store4, err_block_sum

namespace vv {

namespace {

__device__ __forceinline__ void err_one(float p, float t, double& cell, double& sum) {
  const float d = p - t;
  const float s = d * d;
  cell += (double)s;
  sum += (double)d;
}

// grid: C * nck workgroups, plane c of every sample. VEC: H W is a multiple of four, the strides too and every pointer
// is 16-byte aligned. A cell takes its samples in order on both paths, but the thread's `sum` does not add in the
// same order on both, and each keeps its own: a group of four takes the samples outside and its cells inside on the
// 16-byte path, a cell after the other with the samples inside on the element path
template <bool VEC>
__global__ __launch_bounds__(256) void k_err_accum(ErrAccumArgs a) {
#pragma clang fp contract(off)
  __shared__ double red[4];
  const ChunkWalk w(a.nck);
  const size_t plane = (size_t)w.row * a.HW;
  const float* pr = a.pred + plane;
  const float* tg = a.tgt + plane;
  double* cl = a.cell ? a.cell + plane : nullptr;
  double sum = 0.0;
  w.each<VEC>(a.HW, [&](long long p0, int n) {
    if (VEC) {
      double v[4] = {0.0, 0.0, 0.0, 0.0};
      if (cl) load4<true>(cl + p0, 4, v);
      for (int b = 0; b < a.B; ++b) {
        float x[4], y[4];
        load4<true>(pr + (size_t)b * a.pstride + p0, 4, x);
        load4<true>(tg + (size_t)b * a.tstride + p0, 4, y);
#pragma unroll
        for (int e = 0; e < 4; ++e) err_one(x[e], y[e], v[e], sum);
      }
      if (cl) store4<true>(cl + p0, 4, v);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (e >= n) break;
        const long long p = p0 + e;
        double v = cl ? cl[p] : 0.0;
        for (int b = 0; b < a.B; ++b) err_one(pr[(size_t)b * a.pstride + p], tg[(size_t)b * a.tstride + p], v, sum);
        if (cl) cl[p] = v;
      }
    }
  });
  if (a.partial) {  // null iff chan is
    const double t = err_block_sum(sum, red);
    if (threadIdx.x == 0) a.partial[blockIdx.x] = t;
  }
}

// one workgroup per channel: thread t adds the chunk sums t, t + 256, ... in ascending order, then the fixed tree.
// out[c] = out[c] + total (scale 0) or total / scale
__global__ __launch_bounds__(256) void k_err_chan(const double* partial, unsigned nck, double* out, double scale) {
#pragma clang fp contract(off)
  __shared__ double red[4];
  const double* row = partial + (size_t)blockIdx.x * nck;
  double s = 0.0;
  for (unsigned i = threadIdx.x; i < nck; i += 256) s += row[i];
  const double t = err_block_sum(s, red);
  if (threadIdx.x == 0) out[blockIdx.x] = scale == 0.0 ? out[blockIdx.x] + t : t / scale;
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_err_finalize(ErrFinalArgs a) {
#pragma clang fp contract(off)
  __shared__ double red[4];
  const ChunkWalk w(a.nck);
  const size_t plane = (size_t)w.row * a.HW;
  const double* cl = a.cell + plane;
  double* qf = a.q_field ? a.q_field + plane : nullptr;
  double sum = 0.0;
  w.each<VEC>(a.HW, [&](long long p0, int n) {
    double q[4];
    load4<VEC>(cl + p0, n, q);
#pragma unroll
    for (int e = 0; e < 4; ++e) q[e] = q[e] / a.n;
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (e < n) sum += q[e];
    if (qf) store4<VEC>(qf + p0, n, q);
  });
  if (a.partial) {  // null iff q_tab is
    const double t = err_block_sum(sum, red);
    if (threadIdx.x == 0) a.partial[blockIdx.x] = t;
  }
}

// grid: planes * nck workgroups; the value of plane (t, c) is uniform over its workgroups. The operator sum is
// k_obs_augment's statement (vv_ops.hip), y = 0 then y += P[o][j] * x[j] for j ascending under the same contraction
// mode, so the two round alike
template <bool VEC>
__global__ __launch_bounds__(256) void k_r_fill(RFillArgs a) {
  const ChunkWalk w(a.nck);
  const unsigned pl = w.row;
  const unsigned t = pl / (unsigned)a.Ca, c = pl - t * (unsigned)a.Ca;
  const float* row = a.rtab + (size_t)t * a.C;
  float v;
  if (!a.P || c < 4u) {
    v = row[c];
  } else {
    const unsigned i = (c - 4u) / (unsigned)a.nout, o = (c - 4u) - i * (unsigned)a.nout;
    float xs[kObsMaxIn];
#pragma unroll
    for (int j = 0; j < kObsMaxIn; ++j) xs[j] = j < a.nin ? row[4 + a.nin * i + j] : 0.0f;
    float y = 0.0f;
#pragma unroll
    for (int j = 0; j < kObsMaxIn; ++j)
      if (j < a.nin) y += a.P[o * a.nin + j] * xs[j];
    v = y;
  }
  float* out = a.R + (size_t)pl * a.HW;
  const float v4[4] = {v, v, v, v};
  w.each<VEC>(a.HW, [&](long long p0, int n) { store4<VEC>(out + p0, n, v4); });
}

}  // namespace

hipError_t err_accum(const ErrAccumArgs& in, hipStream_t s) {
  ErrAccumArgs a = in;
  const long long CHW = (long long)a.C * a.HW;
  if (!a.pred || !a.tgt || (!a.cell && !a.chan) || a.B < 1 || a.C < 1 || a.HW < 1 || CHW >= 0x80000000LL ||
      a.pstride < CHW || a.tstride < CHW || (a.chan && !a.partial))
    return hipErrorInvalidValue;
  a.nck = err_chunks(a.HW);
  if (!a.chan) a.partial = nullptr;
  const int ph = prof_begin(s);
  const bool vec = a.HW % 4 == 0 && a.pstride % 4 == 0 && a.tstride % 4 == 0 && aligned16(a.pred) &&
                   aligned16(a.tgt) && aligned16(a.cell);
  const unsigned blocks = (unsigned)a.C * a.nck;
  chunk_launch(vec, k_err_accum<true>, k_err_accum<false>, a.C, a.nck, s, a);
  if (a.chan) hipLaunchKernelGGL(k_err_chan, dim3(a.C), dim3(256), 0, s, a.partial, a.nck, a.chan, 0.0);
  // per cell and sample a subtract, a multiply and two fp64 adds; pred and tgt are read once, cell read and written
  prof_end(ph, s, PC_MISFIT, 4.0 * (double)a.B * (double)CHW,
           (8.0 * (double)a.B + (a.cell ? 16.0 : 0.0)) * (double)CHW + (a.chan ? 16.0 * (double)blocks : 0.0));
  return hipGetLastError();
}

hipError_t err_chan_sum(const double* partial, unsigned nck, double* out, unsigned rows, hipStream_t s) {
  if (!partial || !out || nck < 1 || rows < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_err_chan, dim3(rows), dim3(256), 0, s, partial, nck, out, 1.0);  // t / 1.0 is t
  return hipGetLastError();
}

hipError_t err_finalize(const ErrFinalArgs& in, hipStream_t s) {
  ErrFinalArgs a = in;
  const long long CHW = (long long)a.C * a.HW;
  if (!a.cell || (!a.q_field && !a.q_tab) || a.C < 1 || a.HW < 1 || CHW >= 0x80000000LL || !(a.n >= 1.0) ||
      (a.q_tab && !a.partial))
    return hipErrorInvalidValue;
  a.nck = err_chunks(a.HW);
  if (!a.q_tab) a.partial = nullptr;
  const int ph = prof_begin(s);
  const bool vec = a.HW % 4 == 0 && aligned16(a.cell) && aligned16(a.q_field);
  const unsigned blocks = (unsigned)a.C * a.nck;
  chunk_launch(vec, k_err_finalize<true>, k_err_finalize<false>, a.C, a.nck, s, a);
  if (a.q_tab) hipLaunchKernelGGL(k_err_chan, dim3(a.C), dim3(256), 0, s, a.partial, a.nck, a.q_tab, (double)a.HW);
  prof_end(ph, s, PC_MISFIT, 2.0 * (double)CHW,
           (8.0 + (a.q_field ? 8.0 : 0.0)) * (double)CHW + (a.q_tab ? 16.0 * (double)blocks : 0.0));
  return hipGetLastError();
}

hipError_t r_fill(const RFillArgs& in, hipStream_t s) {
  RFillArgs a = in;
  if (!a.rtab || !a.R || a.T < 1 || a.C < 1 || a.HW < 1) return hipErrorInvalidValue;
  if (a.P) {
    if (a.nin < 1 || a.nin > kObsMaxIn || a.nout < 1 || a.nout > kObsMaxOut || a.C != 4 + 5 * a.nin)
      return hipErrorInvalidValue;
    a.Ca = 4 + 5 * a.nout;
  } else {
    a.Ca = a.C;
  }
  a.nck = err_chunks(a.HW);
  const long long blocks = (long long)a.T * a.Ca * a.nck;
  if (blocks >= 0x80000000LL) return hipErrorInvalidValue;
  const int ph = prof_begin(s);
  const bool vec = a.HW % 4 == 0 && aligned16(a.R);
  chunk_launch(vec, k_r_fill<true>, k_r_fill<false>, (unsigned)(a.T * a.Ca), a.nck, s, a);
  prof_end(ph, s, PC_MISFIT, a.P ? 2.0 * a.nin * (double)blocks : 0.0, 4.0 * (double)a.T * a.Ca * (double)a.HW);
  return hipGetLastError();
}

}  // namespace vv
