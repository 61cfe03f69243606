// Model-error statistics and the static R on the device (calculate_q, model/model.py:469-490; init_q_matrix,
// da_4dvar.py:528-550; get_static_info's R, :630-634; get_R_matrix_from_gt, :729-756; include/vaevar.h vv_err_accum,
// vv_err_finalize, vv_r_fill).
//
// Accumulate: a plane of H W cells is cut into chunks of kErrChunk cells, one workgroup each. A thread owns its cells
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
#include "vv_stats.h"  // err_block_sum

namespace vv {

namespace {

constexpr int kErrItems = kErrChunk / (256 * 4);  // groups of four cells per thread

__device__ __forceinline__ void err_one(float p, float t, double& cell, double& sum) {
  const float d = p - t;
  const float s = d * d;
  cell += (double)s;
  sum += (double)d;
}

// grid: C * nck workgroups, workgroup c * nck + k takes cells [k kErrChunk, (k + 1) kErrChunk) of channel c.
// VEC: H W is a multiple of four, the strides too and every pointer is 16-byte aligned: four cells per access
template <bool VEC>
__global__ __launch_bounds__(256) void k_err_accum(ErrAccumArgs a) {
#pragma clang fp contract(off)
  __shared__ double red[4];
  const unsigned c = blockIdx.x / a.nck, k = blockIdx.x - c * a.nck;
  const size_t plane = (size_t)c * a.HW;
  const float* pr = a.pred + plane;
  const float* tg = a.tgt + plane;
  double* cl = a.cell ? a.cell + plane : nullptr;
  double sum = 0.0;
#pragma unroll
  for (int i = 0; i < kErrItems; ++i) {
    const long long p0 = (long long)k * kErrChunk + ((long long)i * 256 + threadIdx.x) * 4;
    if (p0 >= a.HW) break;
    if (VEC) {
      double2 lo = make_double2(0.0, 0.0), hi = lo;
      if (cl) {
        lo = *reinterpret_cast<const double2*>(cl + p0);
        hi = *reinterpret_cast<const double2*>(cl + p0 + 2);
      }
      for (int b = 0; b < a.B; ++b) {
        const float4 x = *reinterpret_cast<const float4*>(pr + (size_t)b * a.pstride + p0);
        const float4 y = *reinterpret_cast<const float4*>(tg + (size_t)b * a.tstride + p0);
        err_one(x.x, y.x, lo.x, sum);
        err_one(x.y, y.y, lo.y, sum);
        err_one(x.z, y.z, hi.x, sum);
        err_one(x.w, y.w, hi.y, sum);
      }
      if (cl) {
        *reinterpret_cast<double2*>(cl + p0) = lo;
        *reinterpret_cast<double2*>(cl + p0 + 2) = hi;
      }
    } else {
      for (int e = 0; e < 4; ++e) {
        const long long p = p0 + e;
        if (p >= a.HW) break;
        double v = cl ? cl[p] : 0.0;
        for (int b = 0; b < a.B; ++b) err_one(pr[(size_t)b * a.pstride + p], tg[(size_t)b * a.tstride + p], v, sum);
        if (cl) cl[p] = v;
      }
    }
  }
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
  const unsigned c = blockIdx.x / a.nck, k = blockIdx.x - c * a.nck;
  const size_t plane = (size_t)c * a.HW;
  const double* cl = a.cell + plane;
  double* qf = a.q_field ? a.q_field + plane : nullptr;
  double sum = 0.0;
#pragma unroll
  for (int i = 0; i < kErrItems; ++i) {
    const long long p0 = (long long)k * kErrChunk + ((long long)i * 256 + threadIdx.x) * 4;
    if (p0 >= a.HW) break;
    if (VEC) {
      double2 lo = *reinterpret_cast<const double2*>(cl + p0), hi = *reinterpret_cast<const double2*>(cl + p0 + 2);
      lo.x = lo.x / a.n, lo.y = lo.y / a.n, hi.x = hi.x / a.n, hi.y = hi.y / a.n;
      sum += lo.x;
      sum += lo.y;
      sum += hi.x;
      sum += hi.y;
      if (qf) {
        *reinterpret_cast<double2*>(qf + p0) = lo;
        *reinterpret_cast<double2*>(qf + p0 + 2) = hi;
      }
    } else {
      for (int e = 0; e < 4; ++e) {
        const long long p = p0 + e;
        if (p >= a.HW) break;
        const double q = cl[p] / a.n;
        sum += q;
        if (qf) qf[p] = q;
      }
    }
  }
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
  const unsigned pl = blockIdx.x / a.nck, k = blockIdx.x - pl * a.nck;
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
  const float4 v4 = make_float4(v, v, v, v);
#pragma unroll
  for (int i = 0; i < kErrItems; ++i) {
    const long long p0 = (long long)k * kErrChunk + ((long long)i * 256 + threadIdx.x) * 4;
    if (p0 >= a.HW) break;
    if (VEC) {
      *reinterpret_cast<float4*>(out + p0) = v4;
    } else {
      for (int e = 0; e < 4; ++e)
        if (p0 + e < a.HW) out[p0 + e] = v;
    }
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

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
  if (vec) hipLaunchKernelGGL(k_err_accum<true>, dim3(blocks), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(k_err_accum<false>, dim3(blocks), dim3(256), 0, s, a);
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
  if (vec) hipLaunchKernelGGL(k_err_finalize<true>, dim3(blocks), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(k_err_finalize<false>, dim3(blocks), dim3(256), 0, s, a);
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
  if (vec) hipLaunchKernelGGL(k_r_fill<true>, dim3((unsigned)blocks), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(k_r_fill<false>, dim3((unsigned)blocks), dim3(256), 0, s, a);
  prof_end(ph, s, PC_MISFIT, a.P ? 2.0 * a.nin * (double)blocks : 0.0, 4.0 * (double)a.T * a.Ca * (double)a.HW);
  return hipGetLastError();
}

}  // namespace vv
