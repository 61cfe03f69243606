// Evaluating a VAE on the device (nf_model/vae.py:72-107: encoder's chunk, sampling, loss_function; the training
// sample of vae_nmc_model.train, model/model.py:593-596; include/vaevar.h vv_vae_sample, vv_vae_sse, vv_err_sample;
// DESIGN.md §5i). Forwards only: no weight gradient is formed anywhere.
//
// All three kernels walk their planes in the chunk layout of vv_stats.h (ChunkWalk): chunks of kErrChunk cells, one
// workgroup each, a thread takes groups of four consecutive cells, 16 bytes per access where the shapes and pointers
// allow and element by element otherwise (load4 / store4), with the same results. Sums are fp64 and follow the fixed
// tree of vv_err_accum: a thread adds its cells ascending, err_block_sum adds lanes and waves, k_err_chan
// (err_chan_sum) the chunks of a plane in ascending order. No atomics: two runs give the same bits.
//
// Sample: one pass over the encoder output reads mu and log_var once and writes z = eps * exp(log_var / 2) + mu and
// the four fp64 sums of the plane. eps(e) is vv_normal_fill's stream (synth_eps4, vv_stats.h) at the element index of
// z; on the element path a thread's four cells may lie in two Philox groups.
#include "vv_kernels.h"

// z = eps * s + mu rounds the product, then the sum (the reference's eps.mul(std).add_(mu)); the fp64 terms of the
// statistics are single operations too
#pragma clang fp contract(off)

#include "vv_stats.h"

namespace vv {

namespace {

// ep[i] for a run-time i in 0..7 without indexing registers through memory
__device__ __forceinline__ float pick8(const float* ep, unsigned i) {
  float v = ep[0];
#pragma unroll
  for (unsigned j = 1; j < 8; ++j) v = i == j ? ep[j] : v;
  return v;
}

// the posterior sample of one element: s = exp(lv / 2) evaluated in fp64 and rounded once
__device__ __forceinline__ float vae_z(float eps, float mu, float lv) {
  const float s = (float)exp(0.5 * (double)lv);
  const float prod = eps * s;
  return prod + mu;
}

struct VaeSums {
  double t, m, q, e;
};
__device__ __forceinline__ void vae_terms(float mu, float lv, VaeSums& a) {
  const double m = (double)mu, v = (double)lv;
  const double q = m * m, ex = exp(v);
  a.t += ((1.0 + v) - q) - ex;
  a.m += m;
  a.q += q;
  a.e += ex;
}

// grid: B * L * nck workgroups; workgroup r * nck + k, r = b L + l, takes a chunk of the planes mu[b][l], lv[b][l].
// VEC: H W is a multiple of four and enc and z are 16-byte aligned, so a thread's four cells are one Philox group
template <bool VEC>
__global__ __launch_bounds__(256) void k_vae_sample(VaeSampleArgs a) {
  __shared__ double red[4];
  const ChunkWalk w(a.nck);
  const unsigned r = w.row, b = r / (unsigned)a.L, l = r - b * (unsigned)a.L;
  const float* mu = a.enc + ((size_t)b * 2 * a.L + l) * a.HW;
  const float* lv = mu + (size_t)a.L * a.HW;
  float* z = a.z ? a.z + (size_t)r * a.HW : nullptr;
  const unsigned long long base = (unsigned long long)r * (unsigned long long)a.HW;
  VaeSums sum{0.0, 0.0, 0.0, 0.0};
  w.each<VEC>(a.HW, [&](long long p0, int n) {
    float m[4], v[4], o[4];
    load4<VEC>(mu + p0, n, m);
    load4<VEC>(lv + p0, n, v);
    if (a.stat) {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (e < n) vae_terms(m[e], v[e], sum);
    }
    if (!z) return;
    if (a.mean) {
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = m[e];
    } else {
      const unsigned long long e0 = base + (unsigned long long)p0, g = e0 >> 2;
      const unsigned off = VEC ? 0u : (unsigned)(e0 & 3);
      float ep[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
      synth_eps4(a.k0, a.k1, a.draw, g, ep);
      if (!VEC && off + (unsigned)n > 4u) synth_eps4(a.k0, a.k1, a.draw, g + 1, ep + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = vae_z(VEC ? ep[e] : pick8(ep, off + e), m[e], v[e]);
    }
    store4<VEC>(z + p0, n, o);
  });
  if (a.stat) {  // partial is given with it
    const double t = err_block_sum(sum.t, red), m = err_block_sum(sum.m, red), q = err_block_sum(sum.q, red),
                 e = err_block_sum(sum.e, red);
    if (threadIdx.x == 0) {
      double* row = a.partial + (size_t)r * 4 * a.nck + w.k;
      row[0] = t;
      row[a.nck] = m;
      row[2 * (size_t)a.nck] = q;
      row[3 * (size_t)a.nck] = e;
    }
  }
}

// grid: B * C * nck workgroups; row r = b C + c
template <bool VEC>
__global__ __launch_bounds__(256) void k_vae_sse(VaeSseArgs a) {
  __shared__ double red[4];
  const ChunkWalk w(a.nck);
  const unsigned b = w.row / (unsigned)a.C, c = w.row - b * (unsigned)a.C;
  const float* rc = a.recon + (size_t)b * a.rstride + (size_t)c * a.HW;
  const float* xs = a.x + (size_t)b * a.xstride + (size_t)c * a.HW;
  double sum = 0.0;
  w.each<VEC>(a.HW, [&](long long p0, int n) {
    float u[4], x[4];
    load4<VEC>(rc + p0, n, u);
    load4<VEC>(xs + p0, n, x);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float d = u[e] - x[e];
      const float s = d * d;
      if (e < n) sum += (double)s;
    }
  });
  const double t = err_block_sum(sum, red);
  if (threadIdx.x == 0) a.partial[blockIdx.x] = t;
}

// the source index of output index d: torch's nearest rule as the host's nearest_map states it (vv_engine.hip; pinned
// by tests/golden/g4_nearest_maps.npz), scale = (float)in / (float)out formed on the host
__device__ __forceinline__ int near_src(int d, int in, int out, float scale) {
  if (in == out) return d;
  if (out == 2 * in) return d >> 1;
  const int s = (int)floorf((float)d * scale);
  return s < in - 1 ? s : in - 1;
}

// grid: B * C * nck workgroups over the OUTPUT planes of Hn Wn cells. VEC: the maps are the identity, H W and the
// strides are multiples of four and every pointer is 16-byte aligned
template <bool VEC>
__global__ __launch_bounds__(256) void k_err_sample(ErrSampleArgs a) {
  const ChunkWalk w(a.nck);
  const unsigned b = w.row / (unsigned)a.C, c = w.row - b * (unsigned)a.C;
  const int HWn = a.Hn * a.Wn;
  const size_t src = (size_t)c * a.Hs * a.Ws;
  const float* pr = a.pred + (size_t)b * a.pstride + src;
  const float* tg = a.tgt + (size_t)b * a.tstride + src;
  float* out = a.out + (size_t)w.row * HWn;
  const float sd = a.err_std[c];
  w.each<VEC>(HWn, [&](long long p0, int n) {
    float u[4] = {0.0f, 0.0f, 0.0f, 0.0f}, t[4] = {0.0f, 0.0f, 0.0f, 0.0f}, o[4];
    if (VEC) {
      load4<true>(pr + p0, 4, u);
      load4<true>(tg + p0, 4, t);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (e >= n) break;
        const int p = (int)p0 + e, oi = p / a.Wn, oj = p - oi * a.Wn;
        const size_t q = (size_t)near_src(oi, a.Hs, a.Hn, a.sh) * a.Ws + near_src(oj, a.Ws, a.Wn, a.sw);
        u[e] = pr[q], t[e] = tg[q];
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float d = t[e] - u[e];
      o[e] = d / sd;
    }
    store4<VEC>(out + p0, n, o);
  });
}

}  // namespace

hipError_t vae_sample(const VaeSampleArgs& in, hipStream_t s) {
  VaeSampleArgs a = in;
  const long long n = 2LL * a.B * a.L * a.HW;
  if (!a.enc || (!a.z && !a.stat) || a.B < 1 || a.L < 1 || a.HW < 1 || n >= 0x80000000LL || (a.stat && !a.partial))
    return hipErrorInvalidValue;
  a.nck = err_chunks(a.HW);
  if (!a.stat) a.partial = nullptr;
  const int ph = prof_begin(s);
  const bool vec = a.HW % 4 == 0 && aligned16(a.enc) && aligned16(a.z);
  const unsigned rows = (unsigned)a.B * (unsigned)a.L, blocks = rows * a.nck;
  chunk_launch(vec, k_vae_sample<true>, k_vae_sample<false>, rows, a.nck, s, a);
  hipError_t e = hipSuccess;
  if (a.stat) e = err_chan_sum(a.partial, a.nck, a.stat, rows * 4, s);
  // per element: a Philox quarter and a Box-Muller half (~30), two fp64 exponentials (~60 each) and the sums; mu and
  // log_var are read once, z written once
  const double ne = 0.5 * (double)n;
  prof_end(ph, s, PC_MISFIT, ((a.z && !a.mean ? 90.0 : 0.0) + (a.stat ? 70.0 : 0.0)) * ne,
           (8.0 + (a.z ? 4.0 : 0.0)) * ne + (a.stat ? 64.0 * (double)blocks : 0.0));
  return e != hipSuccess ? e : hipGetLastError();
}

hipError_t vae_sse(const VaeSseArgs& in, hipStream_t s) {
  VaeSseArgs a = in;
  const long long CHW = (long long)a.C * a.HW;
  if (!a.recon || !a.x || !a.sse || !a.partial || a.B < 1 || a.C < 1 || a.HW < 1 || CHW >= 0x80000000LL ||
      a.rstride < CHW || a.xstride < CHW || (long long)a.B * a.C * err_chunks(a.HW) >= 0x80000000LL)
    return hipErrorInvalidValue;
  a.nck = err_chunks(a.HW);
  const int ph = prof_begin(s);
  const bool vec = a.HW % 4 == 0 && a.rstride % 4 == 0 && a.xstride % 4 == 0 && aligned16(a.recon) && aligned16(a.x);
  const unsigned rows = (unsigned)a.B * (unsigned)a.C, blocks = rows * a.nck;
  chunk_launch(vec, k_vae_sse<true>, k_vae_sse<false>, rows, a.nck, s, a);
  const hipError_t e = err_chan_sum(a.partial, a.nck, a.sse, rows, s);
  prof_end(ph, s, PC_MISFIT, 3.0 * (double)a.B * (double)CHW, 8.0 * (double)a.B * (double)CHW + 16.0 * (double)blocks);
  return e != hipSuccess ? e : hipGetLastError();
}

hipError_t err_sample(const ErrSampleArgs& in, hipStream_t s) {
  ErrSampleArgs a = in;
  const long long CHW = (long long)a.C * a.Hs * a.Ws, HWn = (long long)a.Hn * a.Wn;
  if (!a.pred || !a.tgt || !a.err_std || !a.out || a.B < 1 || a.C < 1 || a.Hs < 1 || a.Ws < 1 || a.Hn < 1 ||
      a.Wn < 1 || CHW >= 0x80000000LL || (long long)a.B * a.C * HWn >= 0x80000000LL || a.pstride < CHW ||
      a.tstride < CHW)
    return hipErrorInvalidValue;
  a.nck = err_chunks(HWn);
  a.sh = (float)a.Hs / (float)a.Hn;
  a.sw = (float)a.Ws / (float)a.Wn;
  const int ph = prof_begin(s);
  const bool vec = a.Hs == a.Hn && a.Ws == a.Wn && HWn % 4 == 0 && a.pstride % 4 == 0 && a.tstride % 4 == 0 &&
                   aligned16(a.pred) && aligned16(a.tgt) && aligned16(a.out);
  chunk_launch(vec, k_err_sample<true>, k_err_sample<false>, (unsigned)a.B * (unsigned)a.C, a.nck, s, a);
  const double no = (double)a.B * a.C * (double)HWn;
  prof_end(ph, s, PC_MISFIT, 2.0 * no, 12.0 * no);
  return hipGetLastError();
}

}  // namespace vv
