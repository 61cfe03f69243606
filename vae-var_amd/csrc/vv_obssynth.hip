// Synthetic observations on the device (obs_type free_*, da_4dvar.py:276-292; get_obs_gt's noise term, :449; the
// static R of get_static_info, :630-634; include/vaevar.h vv_obs_synth, vv_select_smallest, vv_normal_fill; DESIGN.md
// §5g): a random network of exactly n_obs cells, Gaussian observation noise and the (T, C) variance table broadcast
// over the grid, every bit a function of (seed, draw) alone.
//
// Generator. Philox4x32-10 with the key (seed & 0xffffffff, seed >> 32); counter word 3 is the draw number, word 2 the
// stream (1 the mask keys, 2 the noise), words 0..1 the cell or the group of four elements.
//
// Selection: the k cells smallest in (key32, p), by a most-significant-digit radix select over the 32-bit keys in three
// passes of 11, 11 and 10 bits. A pass recomputes the keys (nothing is stored per cell), histograms the digit of the
// cells that match the prefix chosen so far in LDS and adds the block's bins to the global histogram (integer adds:
// any order gives the same counts); one workgroup then scans the bins and records in SelRec the digit that holds the
// rank still wanted and the rank inside it. After the last pass the prefix is the threshold key and the rank is the
// number of cells with that key to admit; they are taken in ascending p: k_sel_tie_count (ties per wave chunk of 1024
// cells), k_sel_scan (exclusive scan of the chunk counts by one workgroup) and k_sel_mask (ballot prefix inside the
// chunk), which writes the 0 / 1 plane. Hand-offs happen only across kernel boundaries; nothing is read back.
//
// Fill: k_synth_fill, a thread per four consecutive elements (one Philox call), reads gt and the plane once and writes
// yo, H and R, 16 bytes per lane where the shapes and pointers allow.
#include "vv_kernels.h"

// yo = gt + sd * eps rounds the product, then the sum: no expression of this file may be fused into an FMA (the
// rounded-operation intrinsics of the HIP headers are plain operators, which the default contraction mode fuses)
#pragma clang fp contract(off)

#include "vv_stats.h"  // philox4x32_10, synth_pair, synth_eps4: the noise stream, shared with vv_vae.hip; aligned16

namespace vv {

namespace {

__device__ __forceinline__ float synth_noisy(unsigned g, float sd, float eps) {
  const float prod = sd * eps;
  return __uint_as_float(g) + prod;
}

// ---------------------------------------------------------------------------------------------------------------
// selection
// ---------------------------------------------------------------------------------------------------------------
constexpr int kSelBins = 2048;       // bins of one pass in the workspace (the last pass uses 1024 of them)
constexpr int kSelChunk = 1024;      // cells per wave of the tie kernels: 16 rounds of 64
constexpr int kSelScanThreads = 1024;

struct SelRec {
  unsigned prefix;               // the digits chosen so far; after the last pass the threshold key
  unsigned rem;                  // the rank still wanted among the cells that match the prefix (1-based; 0: k = 0)
  unsigned ties;                 // cells whose key equals the threshold
  unsigned pad;
  unsigned long long selected;   // cells k_sel_mask set to 1
};

struct SelArgs {
  const unsigned* keys;  // the caller's keys, or null: key32(p) of the mask stream
  unsigned k0, k1, draw;
  long long n, k;
  unsigned nu;           // wave chunks = ceil(n / 1024)
  SelRec* rec;
  unsigned* hist;        // [3][kSelBins]
  unsigned* wt;          // [nu] ties of a chunk
  unsigned* wx;          // [nu] ties before the chunk
  float* mask;           // [n]
};

__device__ __forceinline__ unsigned sel_key(const SelArgs& a, long long p) {
  if (a.keys) return a.keys[p];
  return philox4x32_10(make_uint4((unsigned)p, 0u, kStreamMask, a.draw), a.k0, a.k1).x;
}

// pass D: the digit is (key >> SHIFT) & (2^BITS - 1); the cells above it must equal the prefix
template <int D>
struct SelPass {
  static constexpr int kBits = D == 2 ? 10 : 11;
  static constexpr int kShift = D == 0 ? 21 : D == 1 ? 10 : 0;
};

template <int D>
__global__ __launch_bounds__(256) void k_sel_hist(SelArgs a) {
  __shared__ unsigned h[kSelBins];
  constexpr int bits = SelPass<D>::kBits, shift = SelPass<D>::kShift, bins = 1 << bits;
  for (int i = threadIdx.x; i < bins; i += 256) h[i] = 0u;
  __syncthreads();
  const unsigned prefix = D == 0 ? 0u : a.rec->prefix;
  for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < a.n; p += (long long)gridDim.x * 256) {
    const unsigned key = sel_key(a, p);
    bool in = true;
    if (D > 0) in = (key >> (shift + bits)) == prefix;
    if (in) atomicAdd(&h[(key >> shift) & (unsigned)(bins - 1)], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < bins; i += 256)
    if (h[i]) atomicAdd(&a.hist[D * kSelBins + i], h[i]);
}

// one workgroup: the bin j with (cells in bins below j) < rem <= (cells in bins up to j); there is exactly one while
// 1 <= rem <= the cells of the pass, and none for rem = 0 (k = 0: prefix, rem and ties keep their zeros)
__global__ __launch_bounds__(kSelScanThreads) void k_sel_pick(SelArgs a, int d) {
  __shared__ unsigned s[kSelScanThreads];
  const int t = threadIdx.x;
  const unsigned* h = a.hist + d * kSelBins;
  const unsigned h0 = h[2 * t], h1 = h[2 * t + 1];
  const unsigned rem = d == 0 ? (unsigned)a.k : a.rec->rem, prefix = d == 0 ? 0u : a.rec->prefix;
  s[t] = h0 + h1;
  __syncthreads();
  for (int o = 1; o < kSelScanThreads; o <<= 1) {
    const unsigned add = t >= o ? s[t - o] : 0u;
    __syncthreads();
    s[t] += add;
    __syncthreads();
  }
  const unsigned e0 = s[t] - h0 - h1, e1 = e0 + h0;
  int j = -1;
  unsigned below = 0u, cnt = 0u;
  if (rem >= 1u && e0 < rem && rem <= e0 + h0) {
    j = 2 * t;
    below = e0;
    cnt = h0;
  } else if (rem >= 1u && e1 < rem && rem <= e1 + h1) {
    j = 2 * t + 1;
    below = e1;
    cnt = h1;
  }
  if (j >= 0) {  // every thread has read the record before the first barrier above
    const int bits = d == 2 ? 10 : 11;
    a.rec->prefix = (prefix << bits) | (unsigned)j;
    a.rec->rem = rem - below;
    if (d == 2) a.rec->ties = cnt;
  }
}

__global__ __launch_bounds__(256) void k_sel_tie_count(SelArgs a) {
  const unsigned u = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (u >= a.nu) return;
  const int lane = threadIdx.x & 63;
  const unsigned K = a.rec->prefix;
  const long long base = (long long)u * kSelChunk;
  unsigned cnt = 0u;
  for (int j = 0; j < kSelChunk / 64; ++j) {
    const long long p = base + j * 64 + lane;
    const bool tie = p < a.n && sel_key(a, p) == K;
    cnt += (unsigned)__popcll(__ballot(tie));
  }
  if (lane == 0) a.wt[u] = cnt;
}

// exclusive scan of the nu chunk counts by one workgroup: a contiguous run per thread, the run totals scanned by
// thread 0, then each run written out (the scheme of k_ol_scan_sums, vv_obslist.hip)
__global__ __launch_bounds__(kSelScanThreads) void k_sel_scan(SelArgs a) {
  __shared__ unsigned su[kSelScanThreads];
  const unsigned t = threadIdx.x, run = (a.nu + kSelScanThreads - 1) / kSelScanThreads;
  const unsigned long long lo = (unsigned long long)t * run;
  const unsigned long long hi = lo + run < a.nu ? lo + run : a.nu;
  unsigned c = 0u;
  for (unsigned long long i = lo; i < hi; ++i) c += a.wt[i];
  su[t] = c;
  __syncthreads();
  if (t == 0) {
    unsigned acc = 0u;
    for (int i = 0; i < kSelScanThreads; ++i) {
      const unsigned v = su[i];
      su[i] = acc;
      acc += v;
    }
  }
  __syncthreads();
  c = su[t];
  for (unsigned long long i = lo; i < hi; ++i) {
    a.wx[i] = c;
    c += a.wt[i];
  }
}

__global__ __launch_bounds__(256) void k_sel_mask(SelArgs a) {
  const unsigned u = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (u >= a.nu) return;
  const int lane = threadIdx.x & 63;
  const unsigned K = a.rec->prefix, r = a.rec->rem;
  const long long base = (long long)u * kSelChunk;
  unsigned before = a.wx[u], nsel = 0u;
  for (int j = 0; j < kSelChunk / 64; ++j) {
    const long long p = base + j * 64 + lane;
    const bool valid = p < a.n;
    const unsigned key = valid ? sel_key(a, p) : 0u;
    const bool tie = valid && key == K;
    const unsigned long long m = __ballot(tie);
    const unsigned rank = before + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
    const bool sel = valid && (key < K || (tie && rank < r));
    if (valid) a.mask[p] = sel ? 1.0f : 0.0f;
    before += (unsigned)__popcll(m);
    nsel += (unsigned)__popcll(__ballot(sel));
  }
  if (lane == 0 && nsel) atomicAdd(&a.rec->selected, (unsigned long long)nsel);
}

__global__ void k_sel_stats(const SelRec* rec, long long* out) {
  if (threadIdx.x == 0) {
    out[0] = (long long)rec->selected;
    out[1] = (long long)rec->ties;
  }
}

// workspace: the record, the three histograms, the two chunk arrays, then (obs_synth) the plane
constexpr size_t kSelHead = 256 + 3 * kSelBins * sizeof(unsigned);
inline size_t sel_up(size_t v) { return (v + 255) & ~(size_t)255; }
inline unsigned sel_chunks(long long n) { return (unsigned)((n + kSelChunk - 1) / kSelChunk); }

hipError_t select_launch(SelArgs a, char* ws, hipStream_t s) {
  a.nu = sel_chunks(a.n);
  a.rec = reinterpret_cast<SelRec*>(ws);
  a.hist = reinterpret_cast<unsigned*>(ws + 256);
  a.wt = reinterpret_cast<unsigned*>(ws + kSelHead);
  a.wx = reinterpret_cast<unsigned*>(ws + kSelHead + sel_up((size_t)a.nu * 4));
  if (hipError_t e = hipMemsetAsync(ws, 0, kSelHead, s)) return e;
  const long long want = (a.n + 1023) / 1024;
  const unsigned hb = (unsigned)(want < 512 ? want : 512), tb = (a.nu + 3) / 4;
  hipLaunchKernelGGL(k_sel_hist<0>, dim3(hb), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_sel_pick, dim3(1), dim3(kSelScanThreads), 0, s, a, 0);
  hipLaunchKernelGGL(k_sel_hist<1>, dim3(hb), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_sel_pick, dim3(1), dim3(kSelScanThreads), 0, s, a, 1);
  hipLaunchKernelGGL(k_sel_hist<2>, dim3(hb), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_sel_pick, dim3(1), dim3(kSelScanThreads), 0, s, a, 2);
  hipLaunchKernelGGL(k_sel_tie_count, dim3(tb), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_sel_scan, dim3(1), dim3(kSelScanThreads), 0, s, a);
  hipLaunchKernelGGL(k_sel_mask, dim3(tb), dim3(256), 0, s, a);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------
// fill
// ---------------------------------------------------------------------------------------------------------------
struct FillArgs {
  const float* gt;
  const float* sd;     // [C] or null
  const float* rtab;   // [T C] or null (then R is null)
  const float* mask;   // [HW] the plane
  float* yo;
  float* Hm;
  float* R;
  long long n;         // T C HW < 2^31
  int C, HW;
  unsigned k0, k1, draw;  // the noise key
  const SelRec* rec;
  long long* stats;
};

// VEC: HW is a multiple of four and every pointer is 16-byte aligned, so the four elements of a thread lie in one
// (t, c) plane and move as one 16-byte access each
template <bool VEC>
__global__ __launch_bounds__(256) void k_synth_fill(FillArgs a) {
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x, e0 = 4 * j;
  if (j == 0 && a.stats) {
    a.stats[0] = (long long)a.rec->selected;
    a.stats[1] = (long long)a.rec->ties;
  }
  if (e0 >= a.n) return;
  const bool noise = a.sd != nullptr;
  float ep[4];
  if (noise) synth_eps4(a.k0, a.k1, a.draw, (unsigned long long)j, ep);
  if (VEC) {
    const unsigned pl = (unsigned)e0 / (unsigned)a.HW, p = (unsigned)e0 - pl * (unsigned)a.HW;
    const uint4 g = *reinterpret_cast<const uint4*>(a.gt + e0);
    const float4 m = *reinterpret_cast<const float4*>(a.mask + p);
    if (noise) {
      const float sd = a.sd[pl % (unsigned)a.C];
      float4 y;
      y.x = synth_noisy(g.x, sd, ep[0]);
      y.y = synth_noisy(g.y, sd, ep[1]);
      y.z = synth_noisy(g.z, sd, ep[2]);
      y.w = synth_noisy(g.w, sd, ep[3]);
      *reinterpret_cast<float4*>(a.yo + e0) = y;
    } else if (a.yo != a.gt) {
      *reinterpret_cast<uint4*>(a.yo + e0) = g;
    }
    *reinterpret_cast<float4*>(a.Hm + e0) = m;
    if (a.R) {
      const float rv = a.rtab[pl];
      *reinterpret_cast<float4*>(a.R + e0) = make_float4(rv, rv, rv, rv);
    }
  } else {
    const unsigned* gw = reinterpret_cast<const unsigned*>(a.gt);
    unsigned* yw = reinterpret_cast<unsigned*>(a.yo);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const long long e = e0 + i;
      if (e >= a.n) break;
      const unsigned pl = (unsigned)e / (unsigned)a.HW, p = (unsigned)e - pl * (unsigned)a.HW;
      const unsigned g = gw[e];
      if (noise) a.yo[e] = synth_noisy(g, a.sd[pl % (unsigned)a.C], ep[i]);
      else if (a.yo != a.gt) yw[e] = g;
      a.Hm[e] = a.mask[p];
      if (a.R) a.R[e] = a.rtab[pl];
    }
  }
}

__global__ __launch_bounds__(256) void k_normal_fill(float* out, unsigned long long n, unsigned long long first,
                                                     unsigned long long ng, unsigned k0, unsigned k1, unsigned draw) {
  const unsigned long long g0 = first >> 2;
  for (unsigned long long j = (unsigned long long)blockIdx.x * 256 + threadIdx.x; j < ng;
       j += (unsigned long long)gridDim.x * 256) {
    float ep[4];
    synth_eps4(k0, k1, draw, g0 + j, ep);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const unsigned long long e = 4 * (g0 + j) + i;
      if (e >= first && e - first < n) out[e - first] = ep[i];
    }
  }
}

}  // namespace

size_t select_ws_bytes(long long n) { return kSelHead + 2 * sel_up((size_t)sel_chunks(n) * 4); }
size_t obs_synth_ws_bytes(long long HW) { return select_ws_bytes(HW) + sel_up((size_t)HW * 4); }

hipError_t select_smallest(const unsigned* keys, long long n, long long k, float* mask, long long* stats, char* ws,
                           hipStream_t s) {
  if (!keys || !mask || !ws || n < 1 || n >= 0x80000000LL || k < 0 || k > n) return hipErrorInvalidValue;
  SelArgs a{};
  a.keys = keys;
  a.n = n;
  a.k = k;
  a.mask = mask;
  if (hipError_t e = select_launch(a, ws, s)) return e;
  if (stats) hipLaunchKernelGGL(k_sel_stats, dim3(1), dim3(64), 0, s, reinterpret_cast<const SelRec*>(ws), stats);
  return hipGetLastError();
}

hipError_t obs_synth(const ObsSynthArgs& o, hipStream_t s) {
  const long long HW = (long long)o.Hs * o.Ws, n = (long long)o.T * o.C * HW;
  if (!o.gt || !o.yo || !o.Hm || !o.ws || (o.R == nullptr) != (o.rtab == nullptr) || o.T < 1 || o.C < 1 || HW < 1 ||
      n >= 0x80000000LL || o.n_obs < 0 || o.n_obs > HW)
    return hipErrorInvalidValue;
  const int ph = prof_begin(s);
  float* plane = reinterpret_cast<float*>(o.ws + select_ws_bytes(HW));
  SelArgs a{};
  a.k0 = (unsigned)(o.seed & 0xffffffffull);
  a.k1 = (unsigned)(o.seed >> 32);
  a.draw = o.draw;
  a.n = HW;
  a.k = o.n_obs;
  a.mask = plane;
  if (hipError_t e = select_launch(a, o.ws, s)) return e;
  FillArgs f{o.gt, o.sd, o.rtab, plane, o.yo, o.Hm, o.R, n, o.C, (int)HW, (unsigned)(o.noise_seed & 0xffffffffull),
             (unsigned)(o.noise_seed >> 32), o.draw, reinterpret_cast<const SelRec*>(o.ws), o.stats};
  const bool vec = HW % 4 == 0 && aligned16(o.gt) && aligned16(o.yo) && aligned16(o.Hm) && aligned16(o.R);
  const unsigned blocks = (unsigned)(((n + 3) / 4 + 255) / 256);
  if (vec) hipLaunchKernelGGL(k_synth_fill<true>, dim3(blocks), dim3(256), 0, s, f);
  else hipLaunchKernelGGL(k_synth_fill<false>, dim3(blocks), dim3(256), 0, s, f);
  // the selection recomputes the HW keys five times (10 rounds of 4 multiplies each); the fill reads gt and writes yo,
  // H and R once, one Philox call and two Box-Muller pairs per four elements when the noise is on
  prof_end(ph, s, PC_MISFIT, 5.0 * 40.0 * (double)HW + (o.sd ? 30.0 * (double)n : 0.0),
           4.0 * (double)n * (2.0 + (o.sd || o.yo != o.gt ? 1.0 : 0.0) + (o.R ? 1.0 : 0.0)) + 8.0 * (double)HW);
  return hipGetLastError();
}

hipError_t normal_fill(float* out, long long n, long long first, unsigned long long seed, unsigned draw,
                       hipStream_t s) {
  if (n < 0 || first < 0 || first > 0x7fffffffffffffffLL - n || (n > 0 && !out)) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  const unsigned long long ng = ((unsigned long long)(first + n - 1) >> 2) - ((unsigned long long)first >> 2) + 1;
  const unsigned long long want = (ng + 255) / 256;
  hipLaunchKernelGGL(k_normal_fill, dim3((unsigned)(want < 65536 ? want : 65536)), dim3(256), 0, s, out,
                     (unsigned long long)n, (unsigned long long)first, ng, (unsigned)(seed & 0xffffffffull),
                     (unsigned)(seed >> 32), draw);
  return hipGetLastError();
}

}  // namespace vv
