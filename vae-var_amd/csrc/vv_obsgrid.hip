// Gridding of station reports on the device (data_reader.get_real_obs, da_4dvar.py:301-440, and get_obs_mask for
// obs_type prepbufr*, :190-274; include/vaevar.h vv_obs_grid). The host uploads the (n, 12) fp64 report table; the
// dense grids yo and H are produced here and never cross PCIe.
//
// Real mode. The reference adds the values of a cell in fp32 in the order of the reports, so the sum must not depend on
// the order in which threads arrive. Every report owns the nine pair slots row * 9 + slot (vv_kernels.h), and the
// pairs of a cell are chained through the H grid itself, which holds the list heads until the cell is finished:
//  1. both grids are zeroed (hipMemsetAsync);
//  2. k_grid_link, a thread per report: decodes the row in fp64, stores cell[i] (-1: no pair) and val[i] (the value
//     rounded to fp32) and links: next[i] = atomicExch((int*)&H[cell], -(i + 1)). Heads are NEGATIVE pair numbers, 0
//     is the empty list: no head has the bits of the 1.0f that finished cells receive while other threads still test
//     theirs (9 n + 1 < 2^31 would otherwise allow the collision).
//  3. k_grid_reduce, a thread per pair: the head of a cell walks its list. Up to kGridShort members it visits them in
//     increasing pair number by repeated next-larger selection (the list order depends on the atomics, the visiting
//     order does not), adds in fp32 and writes yo = sum / count and H = 1. A longer list is appended to a queue.
//  4. k_grid_long, a wave per queued list: copies the members into a dense segment of `ord`, sorts them by pair number
//     with a bottom-up merge sort in which every lane places its elements by binary search in the sibling run
//     (O(L log^2 L / 64); the keys are unique), and adds the values in sorted order, 64 loads at a time. The queue order
//     and the segment positions depend on arrival, the results do not.
// Hand-offs happen only across kernel boundaries. Mask mode needs no lists: k_grid_mask stores 1.0f (an atomicExch, so
// that the thread that finds the cell empty counts it), then k_grid_mask_copy fills channels 0..2.
#include "vv_kernels.h"

namespace vv {

namespace {

struct GridWs {
  long long* stats;  // [4] rows used, rows skipped, rows dropped, cells observed
  int* qcount;
  int* ordalloc;
  int* cell;
  float* val;
  int* next;
  int* ord;
  int* queue;
};
__host__ __device__ inline GridWs grid_ws(char* ws, long long n) {
  const size_t M = (size_t)n * kGridSlots;
  int* w = reinterpret_cast<int*>(ws);
  GridWs g;
  g.stats = reinterpret_cast<long long*>(ws);
  g.qcount = w + 8;
  g.ordalloc = w + 9;
  g.cell = w + 16;
  g.val = reinterpret_cast<float*>(w + 16 + M);
  g.next = w + 16 + 2 * M;
  g.ord = w + 16 + 3 * M;
  g.queue = w + 16 + 5 * M;
  return g;
}

// int(np.round(x)) as an index into an axis of `size`: `size` itself becomes `at_size`, [-size, -1] wraps as Python
// indexing does, anything else (a NaN or infinite x included) is -1
__device__ __forceinline__ int grid_index(double x, int size, int at_size) {
  const double r = rint(x);  // ties to even
  if (!(r >= -(double)size && r <= (double)size)) return -1;
  int i = (int)r;
  if (i == size) i = at_size;
  if (i < 0) i += size;
  return i;
}
__device__ __forceinline__ bool grid_present(double v) { return v == v && v != 0.0; }  // `if elem_arr[i]:`

enum { kRowUse = 0, kRowSkip = 1, kRowDrop = 2 };
// the position of a report: time level t, level h, pixel; in the reference's order of tests
__device__ __forceinline__ int grid_row(const ObsGridArgs& a, const double* r, int& t, int& h, int& pix) {
  const double src = r[0], lon = r[1], lat = r[2], plev = r[3], dt = r[4], p = r[5];
  if (a.da_win == 1 && src != 0.0) return kRowSkip;  // the second file is read only for da_win > 3
  if (lon != lon || lat != lat || plev != plev || dt != dt) return kRowSkip;
  const int lon_i = grid_index(lon / 360.0 * (double)a.Ws, a.Ws, 0);
  const int lat_i = grid_index((90.0 - lat) / 180.0 * (double)a.Hs, a.Hs, a.Hs - 1);
  const double pl = a.mode == kGridMask ? plev : p;
  if (lon_i < 0 || lat_i < 0 || pl != pl) return kRowDrop;
  h = 0;
  for (int k = 0; k < a.nlev - 1; ++k) h += a.bounds[k] <= pl ? 1 : 0;
  t = -1;
  if (a.da_win == 1) {
    if (dt >= -0.5 && dt < 0.5) t = 0;
  } else if (src == 0.0) {
    if (dt >= -0.5 && dt < 0.5) t = 0;
    else if (dt >= 0.5 && dt < 1.5) t = 1;
    else if (dt >= 1.5 && dt < 2.5) t = 2;
    else if (dt >= 2.5) t = 3;
  } else {
    if (dt < -2.5) t = 3;
    else if (dt >= -2.5 && dt < -1.5) t = 4;
    else if (dt >= -1.5 && dt < -0.5) t = 5;
  }
  if (t < 0) return kRowSkip;
  pix = lat_i * a.Ws + lon_i;
  return kRowUse;
}
// one add to a counter per wave: the number of lanes with `flag`
__device__ __forceinline__ void grid_count(long long* counter, bool flag) {
  const unsigned long long m = __ballot(flag);
  if (m != 0ull && (threadIdx.x & 63) == __builtin_ctzll(m))
    atomicAdd(reinterpret_cast<unsigned long long*>(counter), (unsigned long long)__popcll(m));
}

__global__ __launch_bounds__(256) void k_grid_link(ObsGridArgs a) {
  const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
  const GridWs w = grid_ws(a.ws, a.n);
  int st = -1, t = 0, h = 0, pix = 0;
  if (row < a.n) st = grid_row(a, a.rep + row * 12, t, h, pix);
  grid_count(w.stats + 0, st == kRowUse);
  grid_count(w.stats + 1, st == kRowSkip);
  grid_count(w.stats + 2, st == kRowDrop);
  if (row >= a.n) return;
  const int i0 = (int)row * kGridSlots;
  if (st != kRowUse) {
    for (int s = 0; s < kGridSlots; ++s) w.cell[i0 + s] = -1;
    return;
  }
  const double* r = a.rep + row * 12;
  const double p = r[5];
  const int HW = a.Hs * a.Ws, Ca = 4 + 5 * a.nlev;
  const int base = t * Ca * HW + pix;  // the whole grid has fewer than 2^31 cells
  const double dl = __dsub_rn(log(p), a.log_lev[h]);
  const bool surf = h == a.nlev - 1;
  for (int s = 0; s < kGridSlots; ++s) {
    // slots 0..4 z q u v t, 5 msl, 6..8 the surface u v t; the operations of :344-370, each rounded on its own
    const double x = s < 5 ? r[6 + s] : s == 5 ? r[11] : r[2 + s];
    int layer;
    double v = x;
    if (s < 5) {
      layer = 4 + h + s * a.nlev;
      if (s == 0) v = __dadd_rn(__dmul_rn(x, 9.8), __dmul_rn(a.zcoef[h], dl));
      else if (s == 1) v = __dmul_rn(x, 1e-6);
      else if (s == 4) v = __dadd_rn(__dadd_rn(x, 273.15), __dmul_rn(a.tcoef[h], dl));
    } else if (s == 5) {
      layer = 3;
      v = __dmul_rn(x, 100.0);
    } else {
      layer = s - 6;
      if (s == 8) v = __dadd_rn(x, 273.15);
    }
    const bool on = grid_present(x) && (s < 6 || surf);
    const int i = i0 + s;
    if (!on) {
      w.cell[i] = -1;
      continue;
    }
    const int c = base + layer * HW;
    w.cell[i] = c;
    w.val[i] = (float)v;
    w.next[i] = atomicExch(reinterpret_cast<int*>(a.Hm) + c, -(i + 1));
  }
}

// the pair after j in a list: next holds 0 at the end, else -(pair + 1)
__device__ __forceinline__ int grid_next(const int* next, int j) {
  const int nx = next[j];
  return nx ? -nx - 1 : -1;
}

__global__ __launch_bounds__(256) void k_grid_reduce(ObsGridArgs a) {
  const long long M = a.n * kGridSlots;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const GridWs w = grid_ws(a.ws, a.n);
  int c = -1;
  if (i < M) {
    c = w.cell[i];
    if (c >= 0 && reinterpret_cast<const int*>(a.Hm)[c] != -((int)i + 1)) c = -1;  // not the head
  }
  grid_count(w.stats + 3, c >= 0);
  if (c < 0) return;
  int L = 0;
  for (int j = (int)i; j >= 0 && L <= kGridShort; j = grid_next(w.next, j)) ++L;
  if (L > kGridShort) {
    const int q = atomicAdd(w.qcount, 1);
    w.queue[2 * q] = c;
    w.queue[2 * q + 1] = (int)i;
    return;
  }
  float s = 0.0f;
  int prev = -1;
  for (int k = 0; k < L; ++k) {  // the smallest member above prev
    int best = 0x7fffffff;
    for (int j = (int)i; j >= 0; j = grid_next(w.next, j))
      if (j > prev && j < best) best = j;
    s = s + w.val[best];
    prev = best;
  }
  a.yo[c] = __fdiv_rn(s, (float)L);
  a.Hm[c] = 1.0f;
}

__global__ __launch_bounds__(64) void k_grid_long(ObsGridArgs a) {
  __shared__ int s_off;
  const long long M = a.n * kGridSlots;
  const GridWs w = grid_ws(a.ws, a.n);
  const int lane = threadIdx.x, nq = *w.qcount;
  for (int q = blockIdx.x; q < nq; q += gridDim.x) {
    const int c = w.queue[2 * q], head = w.queue[2 * q + 1];
    int L = 0;
    for (int j = head; j >= 0; j = grid_next(w.next, j)) ++L;
    if (lane == 0) s_off = atomicAdd(w.ordalloc, L);  // the lists are disjoint: the marks stay below M
    __syncthreads();
    int* A = w.ord + s_off;
    int* B = w.ord + M + s_off;
    {
      int k = 0;
      for (int j = head; j >= 0; j = grid_next(w.next, j), ++k)
        if ((k & 63) == lane) A[k] = j;
    }
    __syncthreads();
    for (long long wd = 1; wd < L; wd *= 2) {  // runs of wd sorted members -> runs of 2 wd
      for (int p = lane; p < L; p += 64) {
        const long long run = p / wd, lo_own = run * wd, lo_sib = (run ^ 1) * wd;
        const int key = A[p];
        int cnt = 0;  // members of the sibling run below key
        if (lo_sib < L) {
          int lo = (int)lo_sib, hi = (int)(lo_sib + wd < L ? lo_sib + wd : L);
          while (lo < hi) {
            const int mid = lo + (hi - lo) / 2;
            if (A[mid] < key) lo = mid + 1;
            else hi = mid;
          }
          cnt = lo - (int)lo_sib;
        }
        B[(run & ~1ll) * wd + (p - lo_own) + cnt] = key;
      }
      __syncthreads();
      int* T = A;
      A = B;
      B = T;
    }
    float s = 0.0f;
    for (int k0 = 0; k0 < L; k0 += 64) {
      const float v = k0 + lane < L ? w.val[A[k0 + lane]] : 0.0f;
      const int m = L - k0 < 64 ? L - k0 : 64;
      for (int j = 0; j < m; ++j) s = s + __shfl(v, j);
    }
    if (lane == 0) {
      a.yo[c] = __fdiv_rn(s, (float)L);
      a.Hm[c] = 1.0f;
    }
    __syncthreads();  // s_off and the segment are reused by the next list
  }
}

__global__ __launch_bounds__(256) void k_grid_mask(ObsGridArgs a) {
  const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
  const GridWs w = grid_ws(a.ws, a.n);
  int st = -1, t = 0, h = 0, pix = 0;
  if (row < a.n) st = grid_row(a, a.rep + row * 12, t, h, pix);
  grid_count(w.stats + 0, st == kRowUse);
  grid_count(w.stats + 1, st == kRowSkip);
  grid_count(w.stats + 2, st == kRowDrop);
  const double* r = a.rep + (row < a.n ? row : 0) * 12;
  const int HW = a.Hs * a.Ws, Ca = 4 + 5 * a.nlev;
  const int base = t * Ca * HW + pix;
  for (int s = 0; s < 6; ++s) {  // value[1..5] at the level, value[7] (msl) at layer 3 (:225-236)
    bool fresh = false;
    if (st == kRowUse && grid_present(s < 5 ? r[6 + s] : r[11])) {
      const int layer = s < 5 ? 4 + h + s * a.nlev : 3;
      fresh = atomicExch(a.Hm + base + layer * HW, 1.0f) == 0.0f;
    }
    grid_count(w.stats + 3, fresh);
  }
}
// H[:, k] = H[:, 4 + (k + 2) nlev + nlev - 1], k = 0, 1, 2 (:272-274); channels 0..2 are zero before
__global__ __launch_bounds__(256) void k_grid_mask_copy(ObsGridArgs a) {
  const int HW = a.Hs * a.Ws, Ca = 4 + 5 * a.nlev;
  const int p = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y, t = blockIdx.z;
  const GridWs w = grid_ws(a.ws, a.n);
  float v = 0.0f;
  if (p < HW) {
    float* Ht = a.Hm + (size_t)t * Ca * HW;
    v = Ht[(size_t)(4 + (k + 2) * a.nlev + a.nlev - 1) * HW + p];
    if (v != 0.0f) Ht[(size_t)k * HW + p] = v;
  }
  grid_count(w.stats + 3, v != 0.0f);
}
__global__ void k_grid_stats(const long long* in, long long* out) {
  if (threadIdx.x < 4) out[threadIdx.x] = in[threadIdx.x];
}

}  // namespace

hipError_t obs_grid(const ObsGridArgs& a, hipStream_t s) {
  const bool real = a.mode == kGridReal;
  if (!a.Hm || !a.ws || a.n < 0 || (a.n > 0 && !a.rep) || (real && !a.yo) || a.nlev < 1 || (a.nlev > 1 && !a.bounds) ||
      (real && (!a.log_lev || !a.zcoef || !a.tcoef)))
    return hipErrorInvalidValue;
  const long long cells = (long long)a.da_win * (4 + 5 * a.nlev) * a.Hs * a.Ws, M = a.n * kGridSlots;
  if (cells >= 0x80000000LL || M + 1 >= 0x80000000LL) return hipErrorInvalidValue;
  const int ph = prof_begin(s);
  hipError_t e = hipMemsetAsync(a.ws, 0, 64, s);
  if (e == hipSuccess) e = hipMemsetAsync(a.Hm, 0, (size_t)cells * 4, s);
  if (e == hipSuccess && real) e = hipMemsetAsync(a.yo, 0, (size_t)cells * 4, s);
  if (e != hipSuccess) return e;
  const GridWs w = grid_ws(a.ws, a.n);
  if (a.n > 0) {
    const unsigned rows = (unsigned)((a.n + 255) / 256);
    if (real) {
      hipLaunchKernelGGL(k_grid_link, dim3(rows), dim3(256), 0, s, a);
      hipLaunchKernelGGL(k_grid_reduce, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, a);
      const size_t qcap = obs_grid_queue_cap(a.n);
      hipLaunchKernelGGL(k_grid_long, dim3((unsigned)(qcap < 2048 ? qcap : 2048)), dim3(64), 0, s, a);
    } else {
      hipLaunchKernelGGL(k_grid_mask, dim3(rows), dim3(256), 0, s, a);
      hipLaunchKernelGGL(k_grid_mask_copy, dim3((a.Hs * a.Ws + 255) / 256, 3, a.da_win), dim3(256), 0, s, a);
    }
  }
  if (a.stats) hipLaunchKernelGGL(k_grid_stats, dim3(1), dim3(64), 0, s, w.stats, a.stats);
  // the two memsets dominate: the grids written once, the table and the pair arrays read and written
  prof_end(ph, s, PC_MISFIT, 20.0 * (double)M,
           4.0 * (double)cells * (real ? 2 : 1) + 96.0 * (double)a.n + 24.0 * (double)M);
  return hipGetLastError();
}

}  // namespace vv
