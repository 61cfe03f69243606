// C ABI of the stand-alone field operations (include/vaevar.h): entry points that take device fields and a stream and
// touch no model and no bound problem. Each one checks its arguments with the small vocabulary below -- every check
// runs before the context is first used, so a refused call does no device work --, selects the device, reserves its
// family's workspace and hands over to the vv:: launcher, which validates again for its internal callers.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <initializer_list>
#include <string>

#include "vv_api.h"
#include "vv_kernels.h"

namespace {

using vv::fail;

// argument checks: 0, or VV_E_ARG with a message that names the offending values
std::string dims(std::initializer_list<long long> v) {
  std::string s = "(";
  for (long long x : v) s += (s.size() > 1 ? ", " : "") + std::to_string(x);
  return s + ")";
}

bool all_set(std::initializer_list<const void*> ptrs) {
  for (const void* p : ptrs)
    if (!p) return false;
  return true;
}
#define VV_NEED(...) \
  if (!all_set({__VA_ARGS__})) return fail(VV_E_ARG, "null argument")
#define VV_CHECK(call)                \
  do {                                  \
    if (int rc_ = (call)) return rc_; \
  } while (0)

// every extent of a shape is 1 at least
int check_shape(const char* what, std::initializer_list<long long> v) {
  for (long long x : v)
    if (x < 1) return fail(VV_E_ARG, "bad %s shape %s", what, dims(v).c_str());
  return 0;
}

// a positive grid of at most max_cells cells; the limit is the entry point's own
int check_grid(int Hs, int Ws, long long max_cells) {
  if (Hs < 1 || Ws < 1 || (long long)Hs * Ws > max_cells)
    return fail(VV_E_ARG, "bad grid (%d, %d): 1 .. %lld cells", Hs, Ws, max_cells);
  return 0;
}

// the product of positive extents stays below 2^31 (formed in double: it cannot overflow)
int check_count(const char* what, std::initializer_list<long long> v) {
  double n = 1.0;
  for (long long x : v) n *= (double)x;
  if (n >= 2147483648.0) return fail(VV_E_ARG, "%s %s: 2^31 elements or more", what, dims(v).c_str());
  return 0;
}

// the (n_out, n_in) level operator within the kernel's bounds (kObsMax* or, for vv_obs_project, kProjMax*)
int check_operator(int n_out, int n_in, int max_out, int max_in) {
  if (n_in < 1 || n_in > max_in || n_out < 1 || n_out > max_out)
    return fail(VV_E_ARG, "operator %dx%d outside 1..%d x 1..%d", n_out, n_in, max_out, max_in);
  return 0;
}

// the optional level operator of the observation space and the channel count it implies: C == 4 + 5 n_in
int check_obs_operator(const float* interp, int n_out, int n_in, int C) {
  if (!interp) return 0;
  VV_CHECK(check_operator(n_out, n_in, vv::kObsMaxOut, vv::kObsMaxIn));
  if (C != 4 + 5 * n_in) return fail(VV_E_ARG, "%d channels, the operator needs 4 + 5*%d", C, n_in);
  return 0;
}

// samples of CHW elements each lie at least CHW apart
int check_strides(long long CHW, int64_t a, int64_t b) {
  if (a < CHW || b < CHW)
    return fail(VV_E_ARG, "sample strides %lld / %lld below %lld elements a sample", (long long)a, (long long)b, CHW);
  return 0;
}

// [a, a + na) and [b, b + nb) share an element; a null buffer overlaps nothing
template <class T>
bool overlap(const T* a, size_t na, const T* b, size_t nb) {
  return a && b && a < b + nb && b < a + na;
}

int check_distinct(const void* a, const void* b, const char* names) {
  if (a == b) return fail(VV_E_ARG, "%s are the same buffer", names);
  return 0;
}

// latitude weights in fp32 as utils/metrics.py:4-9 + :287-289 form them: lat = 90 - j*180/(H-1),
// c = cos(3.1416/180 * lat), w = k * c / sum(c) over the rows [lo, hi) of a set
std::vector<float> cos_lat(int H) {
  std::vector<float> cw(H);
  for (int j = 0; j < H; ++j) {
    const float lat = 90.0f - ((float)j * 180.0f) / (float)(H - 1);
    cw[j] = cosf((float)(3.1416 / 180.0) * lat);
  }
  return cw;
}

// w[j] for j in [lo, hi); returns the fp64 sum of the weights written. torch.sum of a float32 vector is pairwise: a
// double sum rounded once differs from it by < 1 ulp of the total
double lat_weights(const std::vector<float>& cw, int lo, int hi, int k, float* w) {
  double cs = 0.0, sw = 0.0;
  for (int j = lo; j < hi; ++j) cs += cw[j];
  const float csum = (float)cs;
  for (int j = lo; j < hi; ++j) {
    w[j] = ((float)k * cw[j]) / csum;
    sw += (double)w[j];
  }
  return sw;
}

// out = `bytes` of a family's workspace, or VV_E_ALLOC
template <class T>
int reserve(vv::Scratch& ws, size_t bytes, const char* who, T*& out) {
  out = reinterpret_cast<T*>(ws.reserve(bytes));
  return out ? 0 : fail(VV_E_ALLOC, "%s workspace", who);
}

}  // namespace

extern "C" {

int vv_metrics(vv_ctx* ctx, const float* pred, const float* gt, const float* mean, const float* std_,
               const double* scale, int B, int C, int H, int W, double* wrmse, double* bias, void* stream) {
  VV_NEED(ctx, pred, gt, mean, std_, scale, wrmse, bias);
  VV_CHECK(check_shape("field", {B, C, H, W}));
  if (H < 2) return fail(VV_E_ARG, "H = %d: the latitude weights need two rows", H);
  VV_CHECK(vv::set_dev(ctx));
  std::vector<float> wl_host(H);
  lat_weights(cos_lat(H), 0, H, H, wl_host.data());
  const int nchunk = std::max(1, std::min(64, H / 8));
  const size_t n_part = (size_t)B * C * nchunk * 2 * sizeof(double);
  hipStream_t st = (hipStream_t)stream;
  char* ws;
  VV_CHECK(reserve(vv::field_state(ctx).metric, n_part + (size_t)H * sizeof(float), "metric", ws));
  double* part = reinterpret_cast<double*>(ws);
  float* wl = reinterpret_cast<float*>(ws + n_part);
  VV_HIP(hipMemcpyAsync(wl, wl_host.data(), (size_t)H * sizeof(float), hipMemcpyHostToDevice, st));
  vv::MetricArgs a{pred, gt, mean, std_, scale, wl, B, C, H, W, part, nchunk, wrmse, bias};
  VV_HIP(vv::metrics(a, st));
  // the host weight table must outlive the async copy
  VV_HIP(hipStreamSynchronize(st));
  return 0;
}

int vv_verify(vv_ctx* ctx, const float* pred, const float* gt, const float* clim, const float* mean,
              const float* std_, const double* scale, int B, int C, int H, int W, double* out, void* stream) {
  VV_NEED(ctx, pred, gt, mean, std_, scale, out);
  VV_CHECK(check_shape("field", {B, C, W}));
  if ((long long)B * C > 65535) return fail(VV_E_ARG, "bad field shape %s: B*C above 65535", dims({B, C}).c_str());
  // the region bounds of utils/metrics.py:71-72 (Python floats are doubles, int() truncates)
  const int si = H < 1 ? 0 : (int)(70.0 / 180.0 * H + 0.5), ni = H < 1 ? 0 : (int)(110.0 / 180.0 * H + 0.5);
  if (si < 1 || ni <= si || ni >= H)
    return fail(VV_E_ARG, "H = %d leaves a latitude region empty (rows [0,%d), [%d,%d), [%d,%d))", H, si, si, ni, ni,
                H);
  VV_CHECK(vv::set_dev(ctx));
  vv::FieldState& f = vv::field_state(ctx);
  hipStream_t st = (hipStream_t)stream;
  const vv::VerifyTab* tab = nullptr;
  for (const auto& t : f.verify_tabs)
    if (t.H == H) tab = &t;
  if (!tab) {
    // (k, rows) of the four sets: (H, all rows), (si, [0,si)), (ni - si, [si,ni)), (si -- not H - ni --, [ni,H))
    const std::vector<float> cw = cos_lat(H);
    std::vector<float> w(2 * (size_t)H);
    const int lo[4] = {0, 0, si, ni}, hi[4] = {H, si, ni, H}, kf[4] = {H, si, ni - si, si};
    vv::VerifyTab t{H, nullptr, {0.0, 0.0, 0.0, 0.0}};
    for (int s = 0; s < 4; ++s) t.sw[s] = lat_weights(cw, lo[s], hi[s], kf[s], w.data() + (s ? H : 0));
    if (hipMalloc(&t.w, w.size() * sizeof(float)) != hipSuccess) return fail(VV_E_ALLOC, "verify weight table");
    // a blocking copy from pageable memory: the table is on the device when this returns, whatever `stream` is
    if (hipError_t e = hipMemcpy(t.w, w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice)) {
      (void)hipFree(t.w);
      return fail((int)e, "verify weight table upload -> %s", hipGetErrorString(e));
    }
    f.verify_tabs.push_back(t);
    tab = &f.verify_tabs.back();
  }
  // about 12 rows a chunk at H = 721 (62 chunks a plane), never more chunks than rows
  const int rpc = std::max(1, (H + 63) / 64);
  vv::VerifyArgs a{};
  a.pred = pred, a.gt = gt, a.clim = clim, a.mean = mean, a.std_ = std_, a.scale = scale, a.wtab = tab->w;
  for (int s = 0; s < 4; ++s) a.sw[s] = tab->sw[s];
  a.B = B, a.C = C, a.H = H, a.W = W, a.si = si, a.ni = ni;
  a.nck[0] = (si + rpc - 1) / rpc, a.nck[1] = (ni - si + rpc - 1) / rpc, a.nck[2] = (H - ni + rpc - 1) / rpc;
  const size_t nchunk = (size_t)a.nck[0] + a.nck[1] + a.nck[2];
  const size_t n_part = (size_t)B * C * nchunk * vv::kVerifyPart, n_tot = (size_t)B * C * 4 * vv::kVerifyTot;
  VV_CHECK(reserve(f.verify, (n_part + n_tot) * sizeof(double), "verify", a.partial));
  a.total = a.partial + n_part;
  a.out = out;
  VV_HIP(vv::verify(a, st));
  return 0;
}

int vv_obs_augment(vv_ctx* ctx, const float* interp, int n_out, int n_in, const float* x, float* x_aug, int T,
                   int Hs, int Ws, void* stream) {
  VV_NEED(ctx, interp, x, x_aug);
  VV_CHECK(check_operator(n_out, n_in, vv::kObsMaxOut, vv::kObsMaxIn));
  VV_CHECK(check_shape("field", {T, Hs, Ws}));
  VV_CHECK(vv::set_dev(ctx));
  VV_HIP(vv::obs_augment(interp, n_in, n_out, x, x_aug, T, Hs * Ws, (hipStream_t)stream));
  return 0;
}

int vv_obs_error(vv_ctx* ctx, const float* x, const float* yo, const float* Hmask, const float* mask,
                 const float* interp, int n_out, int n_in, int C, int Hs, int Ws, float* err, double* sums,
                 void* stream) {
  VV_NEED(ctx, x, yo, Hmask, mask, err);
  VV_CHECK(check_shape("field", {C, Hs, Ws}));
  VV_CHECK(check_grid(Hs, Ws, 0x7fffffffLL - vv::kObsErrChunk));
  VV_CHECK(check_obs_operator(interp, n_out, n_in, C));
  VV_CHECK(vv::set_dev(ctx));
  const int HW = Hs * Ws, Ca = interp ? 4 + 5 * n_out : C;
  double* part;
  const size_t need = (size_t)vv::obs_error_blocks(HW) * Ca * 2 * sizeof(double);
  VV_CHECK(reserve(vv::field_state(ctx).obs_err, need, "obs_error", part));
  vv::ObsErrArgs a{interp ? n_in : 0, interp ? n_out : 0, C, Ca, HW, interp, x, yo, Hmask, mask, part, err, sums};
  VV_HIP(vv::obs_error(a, (hipStream_t)stream));
  return 0;
}

int vv_obs_qc(vv_ctx* ctx, const float* gt, float* yo, float* Hmask, const float* interp, int n_out, int n_in,
              const float* thr, int flags, int T, int C, int Hs, int Ws, double* counts, void* stream) {
  VV_NEED(ctx, gt, yo, Hmask, thr);
  VV_CHECK(check_shape("field", {T, C, Hs, Ws}));
  VV_CHECK(check_grid(Hs, Ws, 0x80000000LL - vv::kObsQcChunk - 1));
  VV_CHECK(check_obs_operator(interp, n_out, n_in, C));
  if (flags & ~15) return fail(VV_E_ARG, "flags %d outside 0..15", flags);
  if ((flags & VV_QC_EXEMPT_Z) && !(flags & VV_QC_FILTER)) return fail(VV_E_ARG, "VV_QC_EXEMPT_Z without VV_QC_FILTER");
  if ((flags & VV_QC_YO_SIMU) && (flags & VV_QC_YO_SIMU_Z))
    return fail(VV_E_ARG, "VV_QC_YO_SIMU and VV_QC_YO_SIMU_Z are exclusive");
  if (!interp && (flags & (VV_QC_EXEMPT_Z | VV_QC_YO_SIMU_Z)))
    return fail(VV_E_ARG, "the z block (flags %d) needs the level operator", flags);
  VV_CHECK(check_distinct(yo, Hmask, "yo and Hmask"));
  VV_CHECK(vv::set_dev(ctx));
  const int HW = Hs * Ws, Ca = interp ? 4 + 5 * n_out : C;
  double* part;
  const size_t need =
      (size_t)T * vv::obs_qc_blocks(HW) * vv::obs_qc_groups(interp != nullptr, Ca) * 2 * sizeof(double);
  VV_CHECK(reserve(vv::field_state(ctx).obs_qc, need, "obs_qc", part));
  vv::ObsQcArgs a{interp ? n_in : 0, interp ? n_out : 0, C, Ca, HW, T, flags, interp, gt, yo, Hmask, thr, part, counts};
  VV_HIP(vv::obs_qc(a, (hipStream_t)stream));
  return 0;
}

int vv_obs_grid(vv_ctx* ctx, const double* reports, int64_t n, int mode, int da_win, int n_lev, int Hs, int Ws,
                const double* bounds, const double* log_lev, const double* zcoef, const double* tcoef, float* yo,
                float* Hmask, long long* stats, void* stream) {
  VV_NEED(ctx, Hmask);
  if (mode != VV_GRID_REAL && mode != VV_GRID_MASK)
    return fail(VV_E_ARG, "mode %d is neither VV_GRID_REAL nor VV_GRID_MASK", mode);
  const bool real = mode == VV_GRID_REAL;
  if (da_win != 1 && da_win != 6) return fail(VV_E_ARG, "da_win %d: must equal six or one", da_win);
  if (n < 0 || (n > 0 && !reports)) return fail(VV_E_ARG, "%lld reports at %p", (long long)n, (const void*)reports);
  if (n_lev < 1 || n_lev > vv::kObsMaxOut) return fail(VV_E_ARG, "%d levels outside 1..%d", n_lev, vv::kObsMaxOut);
  VV_CHECK(check_shape("grid", {Hs, Ws}));
  if ((n_lev > 1 && !bounds) || (real && (!yo || !log_lev || !zcoef || !tcoef)))
    return fail(VV_E_ARG, "null level table or yo");
  VV_CHECK(check_distinct(yo, Hmask, "yo and Hmask"));
  VV_CHECK(check_count("the grid", {da_win, 4 + 5 * n_lev, Hs, Ws}));
  if (n > (0x7fffffffLL - 1) / vv::kGridSlots)
    return fail(VV_E_ARG, "%lld reports: 9 n + 1 must stay below 2^31", (long long)n);
  VV_CHECK(vv::set_dev(ctx));
  char* ws;
  VV_CHECK(reserve(vv::field_state(ctx).obs_grid, real ? vv::obs_grid_ws_bytes(n) : 64, "obs_grid", ws));
  vv::ObsGridArgs a{reports, (long long)n, mode, da_win, n_lev, Hs, Ws, bounds, log_lev, zcoef, tcoef,
                    real ? yo : nullptr, Hmask, stats, ws};
  VV_HIP(vv::obs_grid(a, (hipStream_t)stream));
  return 0;
}

int vv_obs_synth(vv_ctx* ctx, const float* gt, int T, int C, int Hs, int Ws, int64_t n_obs, unsigned long long seed,
                 unsigned long long noise_seed, unsigned draw, const float* sd, const float* rtab, float* yo,
                 float* Hmask, float* R, long long* stats, void* stream) {
  VV_NEED(ctx, gt, yo, Hmask);
  VV_CHECK(check_shape("field", {T, C, Hs, Ws}));
  VV_CHECK(check_count("the fields", {T, C, Hs, Ws}));
  const long long HW = (long long)Hs * Ws;
  if (n_obs < 0 || n_obs > HW)
    return fail(VV_E_ARG, "%lld observed cells out of %lld: cannot draw without replacement", (long long)n_obs, HW);
  if ((R == nullptr) != (rtab == nullptr)) return fail(VV_E_ARG, "R and rtab must both be given or both be NULL");
  const size_t n = (size_t)T * C * HW;
  auto ov = [n](const float* a, const float* b) { return overlap(a, n, b, n); };
  if (ov(Hmask, gt) || ov(Hmask, yo) || ov(Hmask, R) || ov(R, gt) || ov(R, yo))
    return fail(VV_E_ARG, "Hmask or R overlaps another field");
  if (yo != gt && ov(yo, gt)) return fail(VV_E_ARG, "yo overlaps gt without being gt");
  VV_CHECK(vv::set_dev(ctx));
  char* ws;
  VV_CHECK(reserve(vv::field_state(ctx).obs_synth, vv::obs_synth_ws_bytes(HW), "obs_synth", ws));
  vv::ObsSynthArgs a{gt, T, C, Hs, Ws, (long long)n_obs, seed, noise_seed, draw, sd, rtab, yo, Hmask, R, stats, ws};
  VV_HIP(vv::obs_synth(a, (hipStream_t)stream));
  return 0;
}

int vv_select_smallest(vv_ctx* ctx, const unsigned* keys, int64_t n, int64_t k, float* mask, long long* stats,
                       void* stream) {
  VV_NEED(ctx, keys, mask);
  if (n < 1 || n >= 0x80000000LL) return fail(VV_E_ARG, "%lld keys outside 1 .. 2^31 - 1", (long long)n);
  if (k < 0 || k > n) return fail(VV_E_ARG, "k = %lld outside 0 .. %lld", (long long)k, (long long)n);
  VV_CHECK(vv::set_dev(ctx));
  char* ws;
  VV_CHECK(reserve(vv::field_state(ctx).obs_synth, vv::select_ws_bytes(n), "select_smallest", ws));
  VV_HIP(vv::select_smallest(keys, n, k, mask, stats, ws, (hipStream_t)stream));
  return 0;
}

int vv_normal_fill(vv_ctx* ctx, float* out, int64_t n, int64_t first, unsigned long long seed, unsigned draw,
                   void* stream) {
  if (!ctx || (n > 0 && !out)) return fail(VV_E_ARG, "null argument");
  if (n < 0 || first < 0 || first > INT64_MAX - n)
    return fail(VV_E_ARG, "elements %lld .. %lld + %lld", (long long)first, (long long)first, (long long)n);
  VV_CHECK(vv::set_dev(ctx));
  VV_HIP(vv::normal_fill(out, n, first, seed, draw, (hipStream_t)stream));
  return 0;
}

int vv_err_accum(vv_ctx* ctx, const float* pred, int64_t pred_bstride, const float* tgt, int64_t tgt_bstride, int B,
                 int C, int H, int W, double* cell, double* chan, void* stream) {
  VV_NEED(ctx, pred, tgt);
  if (!cell && !chan) return fail(VV_E_ARG, "cell and chan are both NULL: nothing to accumulate");
  VV_CHECK(check_shape("field", {B, C, H, W}));
  VV_CHECK(check_count("a sample", {C, H, W}));
  VV_CHECK(check_strides((long long)C * H * W, pred_bstride, tgt_bstride));
  VV_CHECK(vv::set_dev(ctx));
  const int HW = H * W;
  double* part = nullptr;
  if (chan)
    VV_CHECK(reserve(vv::field_state(ctx).err, (size_t)C * vv::err_chunks(HW) * sizeof(double), "err_accum", part));
  vv::ErrAccumArgs a{pred, tgt, (long long)pred_bstride, (long long)tgt_bstride, B, C, HW, cell, chan, part, 0u};
  VV_HIP(vv::err_accum(a, (hipStream_t)stream));
  return 0;
}

int vv_err_finalize(vv_ctx* ctx, const double* cell, int64_t n_samples, int C, int H, int W, double* q_field,
                    double* q_tab, void* stream) {
  VV_NEED(ctx, cell);
  if (!q_field && !q_tab) return fail(VV_E_ARG, "q_field and q_tab are both NULL: nothing to write");
  if (n_samples < 1) return fail(VV_E_ARG, "%lld samples: the mean needs one at least", (long long)n_samples);
  VV_CHECK(check_shape("field", {C, H, W}));
  VV_CHECK(check_count("the field", {C, H, W}));
  VV_CHECK(vv::set_dev(ctx));
  const int HW = H * W;
  double* part = nullptr;
  if (q_tab)
    VV_CHECK(reserve(vv::field_state(ctx).err, (size_t)C * vv::err_chunks(HW) * sizeof(double), "err_finalize", part));
  vv::ErrFinalArgs a{cell, (double)n_samples, C, HW, q_field, q_tab, part, 0u};
  VV_HIP(vv::err_finalize(a, (hipStream_t)stream));
  return 0;
}

int vv_r_fill(vv_ctx* ctx, const float* rtab, const float* interp, int n_out, int n_in, int T, int C, int Hs, int Ws,
              float* R, void* stream) {
  VV_NEED(ctx, rtab, R);
  VV_CHECK(check_shape("table / field", {T, C, Hs, Ws}));
  VV_CHECK(check_grid(Hs, Ws, 0x7fffffffLL));
  VV_CHECK(check_obs_operator(interp, n_out, n_in, C));
  const int HW = Hs * Ws, Ca = interp ? 4 + 5 * n_out : C;
  if ((double)T * Ca * vv::err_chunks(HW) >= 2147483648.0)
    return fail(VV_E_ARG, "R (%d, %d, %d, %d) needs 2^31 workgroups or more", T, Ca, Hs, Ws);
  VV_CHECK(vv::set_dev(ctx));
  vv::RFillArgs a{rtab, interp, interp ? n_out : 0, interp ? n_in : 0, T, C, HW, R, 0, 0u};
  VV_HIP(vv::r_fill(a, (hipStream_t)stream));
  return 0;
}

int vv_obs_stats(vv_ctx* ctx, const float* xb_win, const float* xa_win, const float* yo, const float* Hmask,
                 const float* R, const float* interp, int n_out, int n_in, int T, int C, int Hs, int Ws, double* out,
                 void* stream) {
  VV_NEED(ctx, xb_win, yo, Hmask, R, out);
  VV_CHECK(check_shape("field", {T, C, Hs, Ws}));
  VV_CHECK(check_grid(Hs, Ws, 0x80000000LL - vv::kErrChunk - 1));
  VV_CHECK(check_obs_operator(interp, n_out, n_in, C));
  const int HW = Hs * Ws, Ca = interp ? 4 + 5 * n_out : C;
  const double blocks = (double)T * Ca * vv::err_chunks(HW);
  if (blocks >= 2147483648.0)
    return fail(VV_E_ARG, "the window (%d, %d, %d, %d) needs 2^31 workgroups or more", T, Ca, Hs, Ws);
  VV_CHECK(vv::set_dev(ctx));
  double* part;
  VV_CHECK(reserve(vv::field_state(ctx).obs_stats, (size_t)blocks * vv::kObsStatN * sizeof(double), "obs_stats", part));
  vv::ObsStatsArgs a{xb_win, xa_win, yo, Hmask, R, interp, interp ? n_in : 0, interp ? n_out : 0, T, C, HW, part, out,
                     0, 0u};
  VV_HIP(vv::obs_stats(a, (hipStream_t)stream));
  return 0;
}

int vv_vae_sample(vv_ctx* ctx, const float* enc, int B, int L, int H, int W, unsigned long long seed, unsigned draw,
                  int flags, float* z, double* stat, void* stream) {
  VV_NEED(ctx, enc);
  if (!z && !stat) return fail(VV_E_ARG, "z and stat are both NULL: nothing to write");
  if (flags & ~VV_VAE_MEAN) return fail(VV_E_ARG, "unknown flag bits 0x%x", (unsigned)(flags & ~VV_VAE_MEAN));
  VV_CHECK(check_shape("latent", {B, L, H, W}));
  VV_CHECK(check_count("the encoder output", {B, 2LL * L, H, W}));
  const size_t nz = (size_t)B * L * H * W;
  if (overlap<float>(z, nz, enc, 2 * nz)) return fail(VV_E_ARG, "z overlaps the encoder output");
  VV_CHECK(vv::set_dev(ctx));
  const int HW = H * W;
  double* part = nullptr;
  if (stat)
    VV_CHECK(reserve(vv::field_state(ctx).err, (size_t)B * L * 4 * vv::err_chunks(HW) * sizeof(double), "vae_sample",
                     part));
  vv::VaeSampleArgs a{enc, B, L, HW, (unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32), draw,
                      (flags & VV_VAE_MEAN) ? 1 : 0, z, stat, part, 0u};
  VV_HIP(vv::vae_sample(a, (hipStream_t)stream));
  return 0;
}

int vv_vae_sse(vv_ctx* ctx, const float* recon, int64_t recon_bstride, const float* x, int64_t x_bstride, int B, int C,
               int H, int W, double* sse, void* stream) {
  VV_NEED(ctx, recon, x, sse);
  VV_CHECK(check_shape("field", {B, C, H, W}));
  VV_CHECK(check_count("a sample", {C, H, W}));
  VV_CHECK(check_strides((long long)C * H * W, recon_bstride, x_bstride));
  const int HW = H * W;
  if ((double)B * C * vv::err_chunks(HW) >= 2147483648.0)
    return fail(VV_E_ARG, "the fields (%d, %d, %d, %d) need 2^31 workgroups or more", B, C, H, W);
  VV_CHECK(vv::set_dev(ctx));
  double* part;
  VV_CHECK(reserve(vv::field_state(ctx).err, (size_t)B * C * vv::err_chunks(HW) * sizeof(double), "vae_sse", part));
  vv::VaeSseArgs a{recon, x, (long long)recon_bstride, (long long)x_bstride, B, C, HW, sse, part, 0u};
  VV_HIP(vv::vae_sse(a, (hipStream_t)stream));
  return 0;
}

int vv_err_sample(vv_ctx* ctx, const float* pred, int64_t pred_bstride, const float* tgt, int64_t tgt_bstride, int B,
                  int C, int Hs, int Ws, const float* err_std, int Hn, int Wn, float* out, void* stream) {
  VV_NEED(ctx, pred, tgt, err_std, out);
  VV_CHECK(check_shape("field", {B, C, Hs, Ws}));
  VV_CHECK(check_shape("output grid", {Hn, Wn}));
  VV_CHECK(check_count("a sample", {C, Hs, Ws}));
  VV_CHECK(check_count("the output", {B, C, Hn, Wn}));
  VV_CHECK(check_strides((long long)C * Hs * Ws, pred_bstride, tgt_bstride));
  VV_CHECK(vv::set_dev(ctx));
  vv::ErrSampleArgs a{pred, tgt, (long long)pred_bstride, (long long)tgt_bstride, B, C, Hs, Ws, err_std, Hn, Wn, out,
                      0.0f, 0.0f, 0u};
  VV_HIP(vv::err_sample(a, (hipStream_t)stream));
  return 0;
}

int vv_tri_interp(vv_ctx* ctx, const int* tris, int64_t n_tri, const float* yo, const float* Hmask, float* xa, int C,
                  int Hs, int Ws, long long* stats, void* stream) {
  VV_NEED(ctx, yo, Hmask, xa);
  if (n_tri < 0 || (n_tri > 0 && !tris))
    return fail(VV_E_ARG, "%lld simplices at %p", (long long)n_tri, (const void*)tris);
  if (n_tri > 0x7fffffffLL) return fail(VV_E_ARG, "%lld simplices: the table rows are int32", (long long)n_tri);
  VV_CHECK(check_shape("field", {C, Hs, Ws}));
  if (Hs > vv::kTriMaxDim || Ws > vv::kTriMaxDim)
    return fail(VV_E_ARG, "grid (%d, %d): the int32 edge functions hold up to %d", Hs, Ws, vv::kTriMaxDim);
  const size_t cells = (size_t)C * Hs * Ws;
  if (overlap<float>(xa, cells, yo, cells) || overlap<float>(xa, cells, Hmask, cells))
    return fail(VV_E_ARG, "xa overlaps yo or Hmask");
  VV_CHECK(vv::set_dev(ctx));
  vv::TriInterpArgs a{tris, (long long)n_tri, yo, Hmask, xa, C, Hs, Ws, stats};
  VV_HIP(vv::tri_interp(a, (hipStream_t)stream));
  return 0;
}

int vv_obs_project(vv_ctx* ctx, const float* interp_inv, int n_out, int n_in, const float* x_aug, float* x, int T,
                   int Hs, int Ws, void* stream) {
  VV_NEED(ctx, interp_inv, x_aug, x);
  VV_CHECK(check_operator(n_out, n_in, vv::kProjMaxOut, vv::kProjMaxIn));
  VV_CHECK(check_shape("field", {T, Hs, Ws}));
  VV_CHECK(check_grid(Hs, Ws, 0x7fffffffLL - 256 * 2048 - 1));
  VV_CHECK(check_distinct(x, x_aug, "x and x_aug"));
  VV_CHECK(vv::set_dev(ctx));
  VV_HIP(vv::obs_project(interp_inv, n_in, n_out, x_aug, x, T, Hs * Ws, (hipStream_t)stream));
  return 0;
}

}  // extern "C"
