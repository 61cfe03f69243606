// Observation lists (include/vaevar.h vv_set_obs_list): the observation term of the real-observation
// operator driven by a compacted list of the entries with H != 0 instead of the dense (Ca, HW) fields yo / H / R.
//
// Format (vv_kernels.h ObsList). A unit is one observed column (slot s, group v, pixel p): v = 0 the four direct
// channels 0..3, v = 1..5 the five level variables; it exists iff some H != 0 among its group's observation channels
// at p. Units are numbered by slot, then group, then ascending pixel, i.e. in the order of the flat index
// i = (s * 6 + v) * HW + p. A unit holds its records (o, yo, h, r), one per entry with H != 0, in ascending o (the
// observation level, or the direct channel for v = 0); h and r are the fp32 values of the fields.
//   uoff[6 S + 1]   first unit of (slot, group); uoff[6 S] = units
//   upix[units]     the unit's pixel
//   urec[units + 1] the unit's first record; urec[units] = records
//   rec[records]    16-byte records
// Nothing in the numbering depends on a launch geometry, and every step below is integer arithmetic: two builds of the
// same fields give the same bits.
//
// Construction: k_ol_count (a thread per flat index, coalesced along the pixel axis: the number of H != 0 of the
// column), an exclusive scan of (unit flag, record count) in three launches -- k_ol_block_sums per 256 indices,
// k_ol_scan_sums (one workgroup) over the block sums, and the apply step, which k_ol_fill performs on the fly: the
// offsets of a block's 256 indices are its scanned block sum plus a scan in LDS, so the per-index offsets are never
// stored -- one host read-back of the two totals to size the list, then k_ol_fill. Hand-offs happen only across kernel
// boundaries: no workgroup waits for another.
//
// Evaluation: k_obs_list, a lane per unit, the arithmetic of k_obs_misfit (vv_ops.hip) term for term.
#include "vv_kernels.h"
#include "vv_lanes.h"

namespace vv {

namespace {

constexpr int kOlBlock = 256;      // flat indices per workgroup of the count / block-sum / fill kernels
constexpr int kOlScanThreads = 1024;

struct OlBuild {
  const float* yo;
  const float* Hm;
  const float* R;
  int S, nout, Ca, HW;
  long long n;               // 6 S HW flat indices
  unsigned nb;               // workgroups = ceil(n / 256)
  unsigned char* cnt;        // [n]
  unsigned* bu;              // [nb] units of a block
  unsigned* br;              // [nb] records of a block
  unsigned* xu;              // [nb] units before the block
  unsigned long long* xr;    // [nb] records before the block
  unsigned long long* tot;   // [2] units, records
};

// first observation channel and channel count of group v
__device__ __forceinline__ void ol_group(int v, int nout, int& c0, int& nc) {
  c0 = v == 0 ? 0 : 4 + nout * (v - 1);
  nc = v == 0 ? 4 : nout;
}

__global__ __launch_bounds__(kOlBlock) void k_ol_count(OlBuild b) {
  const long long i = (long long)blockIdx.x * kOlBlock + threadIdx.x;
  if (i >= b.n) return;
  const int sv = (int)(i / b.HW), p = (int)(i - (long long)sv * b.HW), s = sv / 6, v = sv - 6 * s;
  int c0, nc;
  ol_group(v, b.nout, c0, nc);
  const float* h = b.Hm + ((size_t)s * b.Ca + c0) * b.HW + p;
  int c = 0;
  for (int k = 0; k < nc; ++k) c += h[(size_t)k * b.HW] != 0.0f ? 1 : 0;
  b.cnt[i] = (unsigned char)c;
}

// the sums of a and b over the workgroup, in every thread (integers: any order gives the same value)
__device__ __forceinline__ void ol_block_total(int& a, int& b, int* sa, int* sb) {
  sa[threadIdx.x] = a;
  sb[threadIdx.x] = b;
  __syncthreads();
  for (int o = kOlBlock / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      sa[threadIdx.x] += sa[threadIdx.x + o];
      sb[threadIdx.x] += sb[threadIdx.x + o];
    }
    __syncthreads();
  }
  a = sa[0];
  b = sb[0];
}

__global__ __launch_bounds__(kOlBlock) void k_ol_block_sums(OlBuild b) {
  __shared__ int sa[kOlBlock], sb[kOlBlock];
  const long long i = (long long)blockIdx.x * kOlBlock + threadIdx.x;
  int c = i < b.n ? b.cnt[i] : 0, f = c > 0 ? 1 : 0;
  ol_block_total(f, c, sa, sb);
  if (threadIdx.x == 0) {
    b.bu[blockIdx.x] = (unsigned)f;
    b.br[blockIdx.x] = (unsigned)c;
  }
}

// exclusive scan of the nb block sums by one workgroup: a contiguous chunk per thread, the chunk totals scanned by
// thread 0, then each chunk written out
__global__ __launch_bounds__(kOlScanThreads) void k_ol_scan_sums(OlBuild b) {
  __shared__ unsigned long long su[kOlScanThreads], sr[kOlScanThreads];
  const unsigned t = threadIdx.x, chunk = (b.nb + kOlScanThreads - 1) / kOlScanThreads;
  const unsigned long long lo = (unsigned long long)t * chunk;
  const unsigned long long hi = lo + chunk < b.nb ? lo + chunk : b.nb;
  unsigned long long u = 0, r = 0;
  for (unsigned long long k = lo; k < hi; ++k) {
    u += b.bu[k];
    r += b.br[k];
  }
  su[t] = u;
  sr[t] = r;
  __syncthreads();
  if (t == 0) {
    unsigned long long au = 0, ar = 0;
    for (int k = 0; k < kOlScanThreads; ++k) {
      const unsigned long long cu = su[k], cr = sr[k];
      su[k] = au;
      sr[k] = ar;
      au += cu;
      ar += cr;
    }
    b.tot[0] = au;
    b.tot[1] = ar;
  }
  __syncthreads();
  u = su[t];
  r = sr[t];
  for (unsigned long long k = lo; k < hi; ++k) {
    b.xu[k] = (unsigned)u;
    b.xr[k] = r;
    u += b.bu[k];
    r += b.br[k];
  }
}

__global__ __launch_bounds__(kOlBlock) void k_ol_fill(OlBuild b, ObsList L) {
  __shared__ int su[kOlBlock], sr[kOlBlock];
  const int t = threadIdx.x;
  const long long i = (long long)blockIdx.x * kOlBlock + t;
  const int c = i < b.n ? b.cnt[i] : 0, f = c > 0 ? 1 : 0;
  su[t] = f;
  sr[t] = c;
  __syncthreads();
  for (int o = 1; o < kOlBlock; o <<= 1) {  // inclusive scan of the block's 256 (flag, count) pairs
    int au = 0, ar = 0;
    if (t >= o) {
      au = su[t - o];
      ar = sr[t - o];
    }
    __syncthreads();
    su[t] += au;
    sr[t] += ar;
    __syncthreads();
  }
  if (i >= b.n) return;
  const unsigned U = b.xu[blockIdx.x] + (unsigned)(su[t] - f);
  const unsigned long long R0 = b.xr[blockIdx.x] + (unsigned long long)(sr[t] - c);
  const int sv = (int)(i / b.HW), p = (int)(i - (long long)sv * b.HW), s = sv / 6, v = sv - 6 * s;
  if (p == 0) L.uoff[sv] = (int)U;
  if (i == 0) {
    L.uoff[6 * b.S] = (int)L.units;
    L.urec[L.units] = (unsigned)L.records;
  }
  if (!f) return;
  L.upix[U] = p;
  L.urec[U] = (unsigned)R0;
  int c0, nc;
  ol_group(v, b.nout, c0, nc);
  const size_t e0 = ((size_t)s * b.Ca + c0) * b.HW + p;
  ObsRec* out = L.rec + R0;
  for (int k = 0; k < nc; ++k) {
    const size_t e = e0 + (size_t)k * b.HW;
    const float h = b.Hm[e];
    if (h != 0.0f) *out++ = ObsRec{k, b.yo[e], h, b.R[e]};
  }
}

// One slot of the observation term from the list: a lane per unit. The terms are those of k_obs_misfit: y = sum_j
// P[o][j] xs[j] (j ascending), d = y - yo, J += (double)((h (d d)) / r), g = coeff ((h d) / r), gs[j] += P[o][j] g; an
// entry with H = 0 adds (+0 to J, +0 to gs) there and is simply absent here. A unit writes its whole group of state
// cells (the n_in levels, or the four direct channels with 0 in the unrecorded ones); cells outside every unit are
// never written (they hold the zeros of the one memset at vv_set_obs_list).
__global__ __launch_bounds__(256) void k_obs_list(ObsListArgs a) {
  __shared__ float Ps[kObsMaxOut * kObsMaxIn];
  __shared__ double red[4];
  __shared__ int go[7];
  const int nin = a.nin, nout = a.nout, HW = a.HW;
  for (int i = threadIdx.x; i < nout * nin; i += 256) Ps[i] = a.P[i];
  if (threadIdx.x < 7) go[threadIdx.x] = a.L.uoff[6 * a.slot + threadIdx.x];
  __syncthreads();
  const int u1 = go[6];
  double acc = 0.0;
  for (int u = go[0] + blockIdx.x * 256 + threadIdx.x; u < u1; u += gridDim.x * 256) {
    int v = 0;
#pragma unroll
    for (int k = 1; k < 6; ++k) v += u >= go[k] ? 1 : 0;
    const int p = a.L.upix[u];
    const unsigned r1 = a.L.urec[u + 1];
    unsigned q = a.L.urec[u];
    if (v == 0) {
      float g0 = 0.0f, g1 = 0.0f, g2 = 0.0f, g3 = 0.0f;
      for (; q < r1; ++q) {
        const ObsRec rc = a.L.rec[q];
        const float d = a.x[(size_t)rc.o * HW + p] - rc.yo;
        acc += (double)((rc.h * (d * d)) / rc.r);
        const float g = a.coeff * ((rc.h * d) / rc.r);
        g0 = rc.o == 0 ? g : g0;
        g1 = rc.o == 1 ? g : g1;
        g2 = rc.o == 2 ? g : g2;
        g3 = rc.o == 3 ? g : g3;
      }
      a.g_obs[p] = g0;
      a.g_obs[(size_t)HW + p] = g1;
      a.g_obs[(size_t)2 * HW + p] = g2;
      a.g_obs[(size_t)3 * HW + p] = g3;
      continue;
    }
    float xs[kObsMaxIn], gs[kObsMaxIn];
    const size_t e0 = (size_t)(4 + nin * (v - 1)) * HW + p;
#pragma unroll
    for (int j = 0; j < kObsMaxIn; ++j) {
      xs[j] = j < nin ? a.x[e0 + (size_t)j * HW] : 0.0f;
      gs[j] = 0.0f;
    }
    for (; q < r1; ++q) {
      const ObsRec rc = a.L.rec[q];
      const float* pr = Ps + rc.o * nin;
      float y = 0.0f;
#pragma unroll
      for (int j = 0; j < kObsMaxIn; ++j)
        if (j < nin) y += pr[j] * xs[j];
      const float d = y - rc.yo, h = rc.h, r = rc.r;
      acc += (double)((h * (d * d)) / r);
      const float g = a.coeff * ((h * d) / r);
#pragma unroll
      for (int j = 0; j < kObsMaxIn; ++j)
        if (j < nin) gs[j] += pr[j] * g;
    }
#pragma unroll
    for (int j = 0; j < kObsMaxIn; ++j)
      if (j < nin) a.g_obs[e0 + (size_t)j * HW] = gs[j];
  }
  acc = lane_sum<64>(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) a.partial[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

}  // namespace

void obs_list_free(ObsList& L) {
  if (L.base) (void)hipFree(L.base);
  L = ObsList{};
}

int obs_list_build(const float* yo, const float* Hm, const float* R, int S, int nout, int HW, ObsList* out,
                   std::string& err, hipStream_t s) {
  *out = ObsList{};
  const long long n = 6LL * S * HW;
  if (S < 1 || HW < 1 || nout < 1 || nout > kObsMaxOut || n > kObsListMaxIndex) {
    err = "observation list: " + std::to_string(S) + " slots of " + std::to_string(HW) +
          " pixels: 6 S HW must stay below 2^31 - 2^24";
    return -1;
  }
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  OlBuild b{};
  b.yo = yo;
  b.Hm = Hm;
  b.R = R;
  b.S = S;
  b.nout = nout;
  b.Ca = 4 + 5 * nout;
  b.HW = HW;
  b.n = n;
  b.nb = (unsigned)((n + kOlBlock - 1) / kOlBlock);
  const size_t o_cnt = 0, o_bu = o_cnt + up((size_t)n), o_br = o_bu + up((size_t)b.nb * 4),
               o_xu = o_br + up((size_t)b.nb * 4), o_xr = o_xu + up((size_t)b.nb * 4),
               o_tot = o_xr + up((size_t)b.nb * 8), ws_bytes = o_tot + 256;
  char* ws = nullptr;
  if (hipMalloc(&ws, ws_bytes) != hipSuccess) {
    (void)hipGetLastError();
    err = "observation list: " + std::to_string(ws_bytes) + " bytes of scan workspace";
    return -2;
  }
  b.cnt = reinterpret_cast<unsigned char*>(ws + o_cnt);
  b.bu = reinterpret_cast<unsigned*>(ws + o_bu);
  b.br = reinterpret_cast<unsigned*>(ws + o_br);
  b.xu = reinterpret_cast<unsigned*>(ws + o_xu);
  b.xr = reinterpret_cast<unsigned long long*>(ws + o_xr);
  b.tot = reinterpret_cast<unsigned long long*>(ws + o_tot);
  auto done = [&](int rc, const std::string& m) {
    (void)hipStreamSynchronize(s);
    (void)hipFree(ws);
    if (rc) {
      obs_list_free(*out);
      err = m;
    }
    return rc;
  };
  hipLaunchKernelGGL(k_ol_count, dim3(b.nb), dim3(kOlBlock), 0, s, b);
  hipLaunchKernelGGL(k_ol_block_sums, dim3(b.nb), dim3(kOlBlock), 0, s, b);
  hipLaunchKernelGGL(k_ol_scan_sums, dim3(1), dim3(kOlScanThreads), 0, s, b);
  unsigned long long tot[2] = {0, 0};
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(tot, b.tot, sizeof(tot), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return done(-3, std::string("observation list count: ") + hipGetErrorString(e));
  if (tot[0] > (unsigned long long)n || tot[1] >= 0xffffffffULL)
    return done(-1, "observation list: " + std::to_string(tot[1]) + " records: the record offsets are 32-bit");
  ObsList L;
  L.S = S;
  L.units = (long long)tot[0];
  L.records = (long long)tot[1];
  const size_t o_uoff = 0, o_upix = o_uoff + up((size_t)(6 * S + 1) * 4), o_urec = o_upix + up((size_t)L.units * 4),
               o_rec = o_urec + up((size_t)(L.units + 1) * 4);
  L.bytes = o_rec + up((size_t)L.records * sizeof(ObsRec)) + 256;
  if (hipMalloc(&L.base, L.bytes) != hipSuccess) {
    (void)hipGetLastError();
    return done(-2, "observation list: " + std::to_string(L.bytes) + " bytes for " + std::to_string(L.units) +
                        " units, " + std::to_string(L.records) + " records");
  }
  L.uoff = reinterpret_cast<int*>(L.base + o_uoff);
  L.upix = reinterpret_cast<int*>(L.base + o_upix);
  L.urec = reinterpret_cast<unsigned*>(L.base + o_urec);
  L.rec = reinterpret_cast<ObsRec*>(L.base + o_rec);
  *out = L;
  hipLaunchKernelGGL(k_ol_fill, dim3(b.nb), dim3(kOlBlock), 0, s, b, L);
  e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return done(-3, std::string("observation list fill: ") + hipGetErrorString(e));
  return done(0, "");
}

hipError_t obs_list_eval(const ObsListArgs& a, hipStream_t s) {
  // nblk <= 32768: a unit number plus the grid's stride stays in an int (kObsListMaxIndex)
  if (!a.L.uoff || !a.P || !a.x || !a.g_obs || !a.partial || a.slot < 0 || a.slot >= a.L.S || a.nblk < 1 ||
      a.nblk > 32768 || a.nin < 1 || a.nin > kObsMaxIn || a.nout < 1 || a.nout > kObsMaxOut)
    return hipErrorInvalidValue;
  const int ph = prof_begin(s);
  hipLaunchKernelGGL(k_obs_list, dim3(a.nblk), dim3(256), 0, s, a);
  // per record: the dot product, the term and the gradient accumulation; the record, and per unit the state column
  // read and the gradient column written (the whole list as an upper bound for one slot)
  prof_end(ph, s, PC_MISFIT, (double)a.L.records / a.L.S * (4.0 * a.nin + 8.0),
           ((double)a.L.records * 16.0 + (double)a.L.units * (8.0 + 8.0 * a.nin)) / a.L.S);
  return hipGetLastError();
}

}  // namespace vv
