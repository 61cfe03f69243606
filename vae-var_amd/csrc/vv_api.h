// What the two C-ABI translation units share (vv_engine.hip: models, problems, the closure; vv_fieldapi.hip: the
// stand-alone field operations): the error record, the HIP status macro and the part of a context the field operations
// use. vv_ctx itself stays private to vv_engine.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <vector>

#include "../../include/vaevar.h"

namespace vv {

// stores the formatted message for the calling thread's vv_last_error and returns `code` (vv_engine.hip)
int fail(int code, const char* fmt, ...);

#define VV_HIP(expr)                                                                                   \
  do {                                                                                                 \
    hipError_t e_ = (expr);                                                                            \
    if (e_ != hipSuccess)                                                                              \
      return ::vv::fail((int)e_, "%s:%d %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(e_)); \
  } while (0)

// An on-demand device workspace that goes with its context. reserve(bytes), bytes > 0: the buffer, at least that
// large, or null when the allocation fails. Contents are not kept across a growth, and the old buffer is freed
// without draining any stream (hipFree waits for the device)
struct Scratch {
  char* p = nullptr;
  size_t cap = 0;
  Scratch() = default;
  Scratch(const Scratch&) = delete;
  Scratch& operator=(const Scratch&) = delete;
  ~Scratch() {
    if (p) (void)hipFree(p);
  }
  char* reserve(size_t bytes) {
    if (bytes <= cap) return p;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    if (hipMalloc(&p, bytes) != hipSuccess) {
      p = nullptr;
      return nullptr;
    }
    cap = bytes;
    return p;
  }
};

// vv_verify's latitude weights of one grid height: uploaded once, then reused without a host wait
struct VerifyTab {
  int H;
  float* w;      // device [2][H]: the "all" weight of each row, then the weight of the row in its region
  double sw[4];  // per row set (all, [0, si), [si, ni), [ni, H)) the sum of its weights over its rows
};

// The field operations' share of a context, held by value in vv_ctx. One workspace per family: two field operations
// may be queued on different streams
struct FieldState {
  int device = 0;
  Scratch metric;     // vv_metrics partial sums + latitude weights
  Scratch verify;     // vv_verify chunk sums and per-(b, c) totals
  Scratch obs_err;    // vv_obs_error per-chunk partial sums
  Scratch obs_qc;     // vv_obs_qc per-workgroup partial counts
  Scratch obs_grid;   // vv_obs_grid pair lists, long-list queue and counters
  Scratch obs_synth;  // vv_obs_synth / vv_select_smallest record, histograms, chunk counts and plane
  Scratch obs_stats;  // vv_obs_stats per-chunk partial tables
  Scratch err;        // chunk sums of vv_err_accum / vv_err_finalize / vv_vae_sample / vv_vae_sse
  std::vector<VerifyTab> verify_tabs;
  ~FieldState() {
    for (auto& t : verify_tabs) (void)hipFree(t.w);
  }
};

FieldState& field_state(vv_ctx* ctx);  // vv_engine.hip

inline int set_dev(vv_ctx* ctx) {
  VV_HIP(hipSetDevice(field_state(ctx).device));
  return 0;
}

}  // namespace vv
