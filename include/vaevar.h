/*
 * vaevar.h — C ABI of libvaevar.so, the MI355X-native (gfx950, HIP) VAE-Var 4D-Var inner loop.
 *
 * The reference (xiaoyi018/VAE-Var) has no FFI: its boundary is the PyTorch module + optimiser
 * protocol. Each entry point below replaces one piece of that protocol:
 *
 *   vv_lgunet_param_count/_info   the state_dict key set of networks_old.transformer.LGUnet_all
 *                                 (networks_old/transformer.py:716-745, swinblock.py:189-262), or with
 *                                 arch = VV_ARCH_LGUNET1 of networks.LGUnet_all.LGUnet_all_1 (LGUnet_all.py:742-776)
 *   vv_model_create/load_weights  LGUnet_all(**cfg) + load_state_dict (da_4dvar.py:590-603, 571-588)
 *   vv_model_forward              LGUnet_all.forward (transformer.py:747-752) = VAE_lr.decoder (vae.py:83-85)
 *   vv_model_backward             autograd of the above w.r.t. its input (input gradient only, quirk Q5)
 *   vv_bind_problem               the closure state of one_step_DA 'vae4dvar' (da_4dvar.py:1179-1251)
 *   vv_closure                    closure() -> loss(z); backward (da_4dvar.py:1183-1208, 1242-1246)
 *   vv_decode                     the analysis xa = decoder_hr(z)*stdTr*std + xb (da_4dvar.py:1301-1306)
 *   vv_set_obs_operator/_augment  the real-observation operator obs_interpolater (da_4dvar.py:62-94, :1196-1206)
 *   vv_metrics                    WRMSE / Bias of the DA logging (utils/metrics.py, da_4dvar.py:1256-1262)
 *   vv_verify                     --forecast_eval: the lead-time scores of utils/metrics.py Metrics (WRMSE, Bias,
 *                                 Activity, Anomaly, WACC, regional forms) of a forecast against the truth
 *   vv_obs_error                  error_obs of --use_eval: the analysis against the held-out station observations
 *                                 (da_4dvar.py:934-937, :1154-1155, :1285-1286)
 *   vv_obs_qc                     get_obs_info's departure filter and yo / H update for obs_type real*
 *                                 (da_4dvar.py:764-800)
 *   vv_obs_grid                   get_real_obs / get_obs_mask: the station reports gridded to yo and H
 *                                 (da_4dvar.py:301-440, :190-274)
 *   vv_obs_synth                  obs_type free_*: a random network of exactly N cells, observation noise and the
 *                                 static R drawn on the device (da_4dvar.py:276-292, :449, :630-634)
 *   vv_obs_stats                  (not in the reference) the O-B / O-A departure moments of a window per time level
 *                                 and observation channel: the Desroziers check of the prescribed R
 *   vv_tri_interp/vv_obs_project  one_step_DA 'interpolation': the linear griddata analysis of the observed cells and
 *                                 the way back to the model levels (da_4dvar.py:968-1061)
 *   vv_integrate                  integrate(x, model, 1) (da_4dvar.py:666-681): the outer-cycle forecast with
 *                                 the 0.25-degree LGUnet_all_1 (da_4dvar.py:1329, :652), forward only
 *   vv_dot/axpy/... , vv_adam     vector arithmetic of torch/optim/lbfgs.py:333-535 and adam.py
 *
 * Conventions: every function returns 0 on success, a non-zero status otherwise (HIP error code or
 * VV_E_*), never throws; vv_last_error() describes the last failure of the calling thread.
 *   vv_nearest_map                F.interpolate(mode='nearest') index maps (nf_model/vae.py:90, da_4dvar.py:671,679)
 * All float pointers passed to compute entry points are DEVICE pointers (fp32, 16-byte aligned)
 * owned by the caller; `stream` is a hipStream_t (NULL = default stream). A context is bound to
 * one device and is not thread-safe. All work is enqueued on the given stream; only functions
 * that return host scalars (vv_closure, vv_dot, ...) synchronise it.
 */
#ifndef VAEVAR_H
#define VAEVAR_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VV_E_ARG 1001     /* invalid argument / unsupported configuration */
#define VV_E_STATE 1002   /* call out of order (e.g. closure before bind_problem) */
#define VV_E_ALLOC 1003   /* device allocation failed */

typedef struct vv_ctx vv_ctx;

#define VV_ARCH_LGUNET 0   /* networks_old.transformer.LGUnet_all (VAE decoder, flow model): fwd + input bwd */
#define VV_ARCH_LGUNET1 1  /* networks.LGUnet_all.LGUnet_all_1 (forecast model): forward only */

/* LGUnet_all keyword arguments (nf_model/parameters0_old.yaml:49-96; for VV_ARCH_LGUNET1
   output/model/model_0.25degree/training_options.yaml:64-119). Zero-initialise, then fill. */
typedef struct vv_lgunet_config {
  int img_size[2];
  int patch_size[2];   /* must equal stride: (2,2) */
  int stride[2];
  int n_groups;        /* len(inchans_list) == len(outchans_list) */
  int inchans[8];
  int outchans[8];
  int enc_dim;
  int embed_dim;
  int window_size;     /* 4 */
  int n_enc_levels;    /* len(enc_depths) == 2 */
  int enc_depths[4];
  int enc_heads[4];
  int n_lg_layers;
  int lg_depths[8];
  int lg_heads[8];
  /* appended for VV_ARCH_LGUNET1 (ignored by VV_ARCH_LGUNET, whose window is window_size x window_size) */
  int arch;            /* VV_ARCH_* */
  int window_hw[2];    /* [wh, ww] (LGUnet_all_1 window_size); patch_size may then exceed stride (3,2)/(2,2) */
} vv_lgunet_config;

/* 102: the "bs_tile" values 25 / 26 and the "patch_pers" values 2 / 4 are no longer accepted by vv_set_tuning
   103: absmax returns NaN when an element is NaN (it returned the largest finite |a_i|); the vector primitives take
        n = 0 as a no-op and refuse n < 0; vv_adam forms its bias corrections in double
   104: vv_obs_qc, the departure filter of the obs_type real* family
   105: vv_obs_grid, the gridding of station reports (get_real_obs, get_obs_mask)
   106: vv_closure_memo / vv_closure_recall, the closure memo; vv_bits_match; the counters "closure_recall_hit" and
        "closure_recall_miss"
   107: vv_tri_interp and vv_obs_project, the da_mode 'interpolation' analysis
   108: vv_verify, the forecast verification scores of --forecast_eval
   110: vv_obs_synth, vv_select_smallest and vv_normal_fill: obs_type free_* networks and observation noise
   111: vv_err_accum, vv_err_finalize and vv_r_fill: model-error statistics (calculate_q) and the static R
   112: vv_vae_sample, vv_vae_sse and vv_err_sample: evaluating a VAE (posterior samples, ELBO terms, error samples)
   113: vv_obs_stats: O-B / O-A departure moments of a window per time level and observation channel */
int vv_version(void);
int vv_last_error(char* buf, int cap);

/* parameter enumeration (no device needed) */
int vv_lgunet_param_count(const vv_lgunet_config* cfg, int* count);
int vv_lgunet_param_info(const vv_lgunet_config* cfg, int index, char* name, int name_cap, int64_t* shape,
                         int* ndim);

int vv_ctx_create(int device, vv_ctx** out);
/* frees the context with its networks, bound problems and graphs (synchronises the device); the handle and every model
   id of it are dead afterwards. NULL is a no-op. Returns 0. */
int vv_ctx_destroy(vv_ctx* ctx);

/* a network instance: `batch` images per forward, `n_slots` independent saved-activation sets
   (one per forecast step of the 4D-Var window) */
int vv_model_create(vv_ctx* ctx, const vv_lgunet_config* cfg, int batch, int n_slots, int* model_id);
/* free a network instance (its weights, planes, saved activations and workspace; `del model` in the reference): the
   id becomes invalid (every later call that names it, a second vv_model_destroy included, returns VV_E_ARG; ids are
   not reused); a problem bound to it (vv_bind_problem / vv_sc4dvar_bind) is unbound (vv_closure, vv_state_ptr, ...
   return VV_E_STATE until the next bind) and the context's closure graphs are dropped: a problem bound to other
   networks stays bound and captures its graphs again. The context-wide calls (vv_set_gemm_math, vv_set_tuning,
   vv_ctx_destroy) skip the freed entry. Synchronises the device. */
int vv_model_destroy(vv_ctx* ctx, int model_id);
/* ptrs[i] points to parameter i in vv_lgunet_param_info order (host or device memory, fp32) */
int vv_load_weights(vv_ctx* ctx, int model_id, const void* const* ptrs, int n);
/* out: (batch, sum(outchans), H, W); only channels < out_limit are written (0 = all) */
int vv_model_forward(vv_ctx* ctx, int model_id, int slot, const float* in, float* out, int out_limit, void* stream);
/* din = add + (d out / d in)^T dout, reading only dout channels < out_limit; add may be NULL */
int vv_model_backward(vv_ctx* ctx, int model_id, int slot, const float* dout, float* din, const float* add,
                      int out_limit, void* stream);
int vv_model_workspace_bytes(vv_ctx* ctx, int model_id, int64_t* bytes);

/* one_step_DA 'vae4dvar' problem: state (C,Hs,Ws), window of T times; flow_model_id < 0 when T == 1.
   When (Hs,Ws) differs from the network grid (e.g. 721x1440 vs 128x256) the decoder output and each forecast are
   nearest-up-sampled to the state grid and the forecast input nearest-down-sampled, as decoder_hr / integrate do.
   B independent analyses (ensemble members / windows) are bound at once when the decoder model (and the flow model)
   were created with batch B: every evaluation then runs ONE decoder launch sequence over the B latents (GEMMs of
   B x 2048 rows) and one flow sequence per forecast step; each analysis keeps its own J.
   xb (B,C,Hs,Ws); yo, Hmask, R (B,T,C,Hs,Ws); mean, std, std_tr (C). Buffers stay owned by the caller. */
int vv_bind_problem(vv_ctx* ctx, int dec_model_id, int flow_model_id, int T, int C, int Hs, int Ws,
                    const float* xb, const float* yo, const float* Hmask, const float* R, const float* mean,
                    const float* std_, const float* std_tr, float obs_coeff);
/* J = J_b + obs_coeff * J_o at latent z (B,32,128,256); grad_z = dJ/dz (B,32,128,256); J_b, J_o: B doubles each
   (host), one per analysis. Synchronises `stream`. With the closure memo on (vv_closure_memo) and grad_z != NULL the
   latent is looked up first and a hit is returned without an evaluation. */
int vv_closure(vv_ctx* ctx, const float* z, float* grad_z, double* J_b, double* J_o, void* stream);
/* same, leaving {J_b, J_o} per analysis in device memory d_J[2B]; no synchronisation, and never a memo lookup (no
   host round trip); with the memo on a gradient evaluation is recorded */
int vv_closure_async(vv_ctx* ctx, const float* z, float* grad_z, double* d_J, void* stream);
/* The closure memo: a ring of the last `slots` gradient evaluations of the bound problem (device copies of z, grad_z
   and {J_b, J_o}), so that an evaluation asked for again at a latent whose content has not changed is answered from
   the ring. torch.optim.LBFGS.step() begins with closure() at the point the previous step's line search accepted
   (torch/optim/lbfgs.py:333-350), and one_step_DA calls step Nit times on a latent nothing touches in between
   (da_4dvar.py:1255-1299): the first evaluation of every step after the first repeats one already made, bit for bit.
   slots 1..16 turns the memo on and empties it (calling it again empties it); 0 turns it off and frees the slots.
   VV_E_ARG out of range, VV_E_STATE without a bound problem. OFF BY DEFAULT: the problem buffers (xb, yo, Hmask, R,
   ...) are the caller's and the engine cannot see an in-place edit of them, so the caller turns the memo on for the
   span in which it promises that their contents stay fixed.
   Recording: while on, every vv_closure / vv_closure_async with grad_z != NULL copies its z, grad_z and J pair into
   the oldest slot (two latent-sized device copies queued after the evaluation); a J-only evaluation neither records
   nor evicts. Emptied by every call after which an old result need not hold: vv_bind_problem (which also turns the
   memo off when the latent size changes), vv_set_obs_operator, vv_set_obs_list, vv_set_tuning (any key), vv_set_gemm_math,
   vv_set_closure_graph, vv_load_weights, vv_model_destroy (of a bound network: off, the problem is unbound),
   vv_sc4dvar_bind; vv_ctx_destroy frees it.
   A hit touches none of the state buffers behind vv_state_ptr: they stay those of the last EVALUATED closure. */
int vv_closure_memo(vv_ctx* ctx, int slots);
/* Look z up in the memo: one launch compares it with every recorded latent bit for bit (as 32-bit words: -0.0 is not
   +0.0, a NaN equals itself), one 4-byte read-back; synchronises `stream`. The newest equal slot wins: its gradient is
   copied to grad_z and its J pair to d_J (device, 2B doubles laid out as vv_closure_async leaves them; may be NULL),
   queued on `stream`, and *hit = 1. On a miss nothing is written and *hit = 0; with the memo off every call is a miss
   (and is not counted). vv_get_counter "closure_recall_hit" / "closure_recall_miss" count the lookups, those of
   vv_closure included. */
int vv_closure_recall(vv_ctx* ctx, const float* z, float* grad_z, double* d_J, void* stream, int* hit);
/* the memo's compare kernel on its own (kernel tests): bit i of *match (host) is set iff cand[i][0..n) equals z[0..n)
   bit for bit; count 1..16 device vectors, n >= 0, any alignment (16-byte aligned vectors are read as 128-bit
   groups). Synchronises `stream`. */
int vv_bits_match(vv_ctx* ctx, const float* z, const float* const* cand, int count, int64_t n, unsigned* match,
                  void* stream);
/* replay the closure from a hipGraph (default on; the Python Context turns it off for VAEVAR_GRAPH=0): the evaluation's
   ~540 kernel launches are captured once per kind (J only / J + gradient) and replayed as one graph launch, with z
   and grad_z copied through problem-owned buffers; results are bit-identical to the eager launches */
int vv_set_closure_graph(vv_ctx* ctx, int enable);
/* state of the closure graph of one kind (0: J only, 1: J + gradient) since the last bind / vv_set_closure_graph:
   info[0] graphs enabled, info[1] graph instantiated, info[2] capture failed (this kind runs eagerly: a silent
   slowdown otherwise, the results are identical), info[3] graph launches */
int vv_get_closure_graph(vv_ctx* ctx, int kind, long long* info);
/* process-wide host-side launch counters (monotonic; eager launches only, a graph replay does not count):
   "rowsplit" (k_rowsplit passes building a GEMM's fp16x3 A planes), "fixup_ln" (split-K fixups fused into a
   LayerNorm), "splitk_fixup" (stand-alone split-K fixups of tile 48, and of tile 49's plain GEMMs:
   k_gemm_fixup49), "gather_scales" (k_gather_scales passes of tile 48),
   "h5_split" (fused fixup + LayerNorm launches consuming tile 49's split-K partials, tuning key "h5_split").
   Tests use them to show a fused path ran. "closure_recall_hit" / "closure_recall_miss": the closure memo's lookups
   (vv_closure_recall, and vv_closure with the memo on) that found / did not find the latent. */
int vv_get_counter(const char* name, long long* value);
/* analysis states xa (B,C,Hs,Ws) */
int vv_decode(vv_ctx* ctx, const float* z, float* xa, void* stream);
/* out = integrate(x, model, steps) (da_4dvar.py:666-681): z = (x - mean)/std (nearest to the model grid when
   (Hs,Ws) differs, interpolation=True); `steps` times z = model(z)[:, :C]; nearest back to (Hs,Ws); *std + mean.
   x, out (C,Hs,Ws); mean, std (C). The model (either arch, batch 1) must map C channels to >= C. */
int vv_integrate(vv_ctx* ctx, int model_id, const float* x, float* out, int C, int Hs, int Ws, const float* mean,
                 const float* std_, int steps, void* stream);
/* sc4dvar (da_4dvar.py:1064-1177): the B-matrix control-variable transform of the static 3D/4D-Var mode.
   Replaces init_b_matrix (:520-526), get_static_info (:608-628: RealSHT/InverseRealSHT of torch_harmonics on the
   equiangular 128x256 grid, the zonal Gaussian kernel of the first hpad = 112 rows, sph_scale) and binds the
   loss of :1071-1101. B-matrix tables as the reference loads them from dataset/bq_info_lr (one .npy per table, float64, host):
   len_scale[69] (multiplied by scale_factor, :521), reg_coeff[69][n_reg] (n_reg 13 or 26, :890-893),
   std_sur[4], vert_eig_value[5][13], vert_eig_vec[5][13][13]. Problem buffers (device, caller-owned) as in
   vv_bind_problem: xb (69,Hs,Ws), yo/Hmask/R (T, C_obs, Hs, Ws), mean/std (69) for the flow steps; C = 69 and
   (Hs,Ws) >= (128,256). interp: null for observations of the state (C_obs = 69), else the (n_out, 13)
   obs_interpolater.interp of obs_type 'real*' (C_obs = 4 + 5*n_out, host or device, copied). T > 1 needs a
   networks_old LGUnet_all flow model (69 -> >= 69 channels, 128x256, batch 1): x_t = integrate(x_{t-1}) is
   detached in the reference (:1080), so those terms enter J but not dJ/dw. */
int vv_sc4dvar_bind(vv_ctx* ctx, int flow_model_id, int T, int C, int Hs, int Ws, const float* xb, const float* yo,
                    const float* Hmask, const float* R, const float* mean, const float* std_, float obs_coeff,
                    const float* interp, int n_out, const double* len_scale, const double* reg_coeff, int n_reg,
                    const double* std_sur, const double* vert_eig_value, const double* vert_eig_vec,
                    double scale_factor, int hpad);
/* loss(w) = J_b + obs_coeff * J_o (:1099-1101) at w (69,128,256); grad_w (may be null) = its gradient with the
   reference's detach; J_b, J_o to the host. Synchronises `stream`. */
int vv_sc4dvar_closure(vv_ctx* ctx, const float* w, float* grad_w, double* J_b, double* J_o, void* stream);
/* xhat (69,Hs,Ws) = transform(w, xb) (:878-931) */
int vv_sc4dvar_transform(vv_ctx* ctx, const float* w, float* xhat, void* stream);
/* F.interpolate(x, (Ho, Wo)) with the default mode 'nearest' (quirk Q3; nf_model/vae.py:90 decoder_hr,
   da_4dvar.py:671/679/928) on (BC, Hi, Wi) device fields -> out (BC, Ho, Wo); with adjoint != 0 the transposed
   map: in (BC, Ho, Wo) -> out (BC, Hi, Wi), each source pixel the sum over its nearest preimage (deterministic).
   Synchronises `stream`. */
int vv_resample_nearest(vv_ctx* ctx, const float* in, float* out, int BC, int Hi, int Wi, int Ho, int Wo, int adjoint,
                        void* stream);
/* real-observation operator (da_4dvar.py:62-94 obs_interpolater; the loss's x_aug, :1196-1206): after
   vv_bind_problem, the bound yo, Hmask, R become (T, 4 + 5*n_out, Hs, Ws) observation-space fields. Channels 0..3
   are observed directly; for each of the five 13-level variables i (z, q, u, v, t) x_aug[4 + n_out*i + o] =
   sum_j interp[o][j] x[4 + n_in*i + j]. interp: (n_out, n_in) fp32, host or device, copied. Needs C = 4 + 5*n_in,
   n_in <= 16, n_out <= 64; n_out = 0 restores the identity operator (synthetic observations). */
int vv_set_obs_operator(vv_ctx* ctx, int n_out, int n_in, const float* interp);
/* x_aug (T, 4 + 5*n_out, Hs, Ws) = the operator applied to x (T, 4 + 5*n_in, Hs, Ws); interp on the device.
   Also get_R_matrix_from_gt (da_4dvar.py:729-756) when applied to R. */
int vv_obs_augment(vv_ctx* ctx, const float* interp, int n_out, int n_in, const float* x, float* x_aug, int T,
                   int Hs, int Ws, void* stream);
/* Observation lists: the observation term of the real-observation operator evaluated from a compacted list of the
   entries with Hmask != 0 instead of the dense observation-space fields. With the list set, an evaluation reads the
   state, the list and nothing of yo / Hmask / R: its cost follows the number of observations, not the grid.
   Format. A unit is one observed column (time slot, pixel p, group v): v = 0 the four direct channels 0..3,
   v = 1..5 the five level variables; it exists iff some Hmask != 0 among its group's observation channels at p. A unit
   holds one record (o, yo, h, r) per entry with Hmask != 0, o (the observation level, or the direct channel for
   v = 0) ascending, h and r the fp32 values of Hmask and R: every term is the arithmetic of the dense kernel
   (d = x_aug - yo, J += (double)((h (d d)) / r), g = coeff ((h d) / r)), only the fp64 order of the J sum differs.
   Units are ordered by slot (for B analyses: b * T + t), then group, then ascending pixel; the order depends on
   nothing else, and two builds of the same fields give the same bits. Device arrays: uoff[6 S + 1] (first unit of
   each (slot, group)), upix[units], urec[units + 1] (first record of each unit), rec[records] (16 bytes each).
   which: 0 the vae4dvar problem (vv_bind_problem + vv_set_obs_operator), 1 the sc4dvar problem (vv_sc4dvar_bind
   with interp). enable != 0 builds the list on the device from the bound fields (a count pass, a three-launch
   exclusive scan, one read-back of the two totals, a fill pass), zeroes the engine's observation-gradient field once
   (evaluations write the cells of existing units only), drops the closure graphs and empties the closure memo;
   enable == 0 frees the list and restores the dense path. Synchronises the device. VV_E_ARG: null context, which
   outside 0..1, 6 * slots * Hs * Ws above 2^31 - 2^24 or 2^32 - 1 records and more; VV_E_STATE: no such problem
   bound, or enable with the identity operator (lists for synthetic observations of the state are not provided).
   vv_bind_problem, vv_set_obs_operator and vv_sc4dvar_bind drop the list of the problem they rebind.
   CONTRACT. The list is a SNAPSHOT of yo / Hmask / R at the call: a later in-place edit of them is not seen until
   vv_set_obs_list(.., 1) is called again. While a list is set, no evaluation (vv_closure*, vv_sc4dvar_closure) reads
   the bound yo, Hmask or R: the caller may release them. The path is never chosen automatically. */
int vv_set_obs_list(vv_ctx* ctx, int which, int enable);
/* info[0] list set, info[1] units, info[2] records, info[3] device bytes held (all 0 without a list) */
int vv_get_obs_list(vv_ctx* ctx, int which, long long* info);
/* the list kernels on their own (kernel tests): builds a temporary list of the device fields yo, Hmask, R
   (T, 4 + 5*n_out, Hs, Ws), evaluates it once on x (T, 4 + 5*n_in, Hs, Ws) with interp (n_out, n_in) on the device,
   and writes g_obs (T, 4 + 5*n_in, Hs, Ws; device; fully defined: zero off the units), J[T] = the slot's sum of
   h d^2 / r (host; the closure's J_o is half the sum over the slots) and counts[2 T] = {units, records} per slot
   (host). Synchronises `stream`. Arguments are validated before any device work: VV_E_ARG for a null pointer,
   T < 1, n_in outside 1..16, n_out outside 1..64, Hs * Ws >= 2^31 or 6 * T * Hs * Ws above 2^31 - 2^24. */
int vv_obs_list_eval(vv_ctx* ctx, const float* interp, int n_out, int n_in, const float* x, const float* yo,
                     const float* Hmask, const float* R, int T, int Hs, int Ws, float coeff, float* g_obs, double* J,
                     long long* counts, void* stream);
/* latitude-weighted WRMSE and Bias per channel as one_step_DA logs them (da_4dvar.py:1256-1262 with
   utils/metrics.py Metrics.WRMSE / Metrics.Bias, weighted_rmse_torch_channels :282-289, type_weighted_bias_torch
   'all' :65-82): both fields normalised by (x - mean)/std, then scaled by `scale` (the float64 model_std).
   pred, gt (B,C,H,W); mean, std_ (C) fp32; scale (C) fp64; wrmse, bias (C) fp64 device. Synchronises `stream`. */
int vv_metrics(vv_ctx* ctx, const float* pred, const float* gt, const float* mean, const float* std_,
               const double* scale, int B, int C, int H, int W, double* wrmse, double* bias, void* stream);
/* forecast verification (--forecast_eval): the score family of utils/metrics.py Metrics in ONE pass over pred, gt
   (B,C,H,W) and, when given, the climatology clim (C,H,W), all physical fp32 on the device. Fields are normalised
   inside, (x - mean)/std_ in fp32 as vv_metrics does, and the statistics equal the Metrics methods of the same names
   run on those normalised fields with data_std = scale (fp64). out: VV_VERIFY_NSTAT x C doubles on the device, row
   VV_VERIFY_<name> holding the per-channel vector of Metrics.<name>.

   Rows and weights (fp32, built on the host as the reference builds them): lat_j = 90 - j*180/(H-1),
   c_j = cos(3.1416/180 * lat_j) (the reference's constant, not pi), si = int(70/180*H + 0.5),
   ni = int(110/180*H + 0.5).
     plain  (WRMSE, Bias, ..)    every row,      w_j = H * c_j / sum(c)
     S..    "southern"           rows [0, si),   w_j = si * c_j / sum(c over the rows)
     T..    "tropics"            rows [si, ni),  w_j = (ni - si) * c_j / sum(c over the rows)
     N..    "northern"           rows [ni, H),   w_j = si * c_j / sum(c over the rows)   (si, not H - ni)
   The names follow the reference's row ranges (row 0 is +90 degrees, so "southern" is the north); they are kept.
   With d = pred_n - gt_n, p' = pred_n - clim_n, t' = gt_n - clim_n, mean_R the plain mean over the rows of the set
   and W columns, and <.> the mean over B taken AFTER the per-sample root or quotient:
     *WRMSE     < sqrt(mean_R(w d^2)) > * scale              *Bias   < mean_R(w d) > * scale
     Channel_MSE  mean over (B,H,W) of d^2                    MSE, MAE  mean over (B,C,H,W) of d^2, |d|: scalars in the
                                                              reference, here the same value in every channel's slot
     *Activity  < sqrt(mean_R(w (p' - m_p)^2)) > * scale,  m_p = mean_R(w p')  (centred on the weighted slice mean)
     *Anomaly   < nume / (sqrt(mean_R(w (p' - m_p)^2)) * sqrt(mean_R(w (t' - m_t)^2))) >, where nume =
                mean(w (p' - m_p)(t' - m_t)) is taken WITHOUT a dim in all four forms of the reference
                (type_weighted_anomaly_torch_channels): one scalar over (B, C, rows, W), so a channel's Anomaly depends
                on every channel. Mirrored as it is.
     *WACC      < sum_R(w p' t') / sqrt(sum_R(w p'^2) * sum_R(w t'^2)) >   (not centred)
   Error family (rows 0..10): always. Climatology family (rows 11..22): only with clim; with clim == NULL those rows
   are NaN and clim is never read. Left out: Metrics.RMSE (its dim=[1,2] mean is not a per-channel score of a 4-D
   input) and Position_MSE (a field of H*W values, not a statistic per channel).
   Every term is the reference's fp32 product; sums are fp64 in a fixed order without atomics, so two calls give the
   same bits, and the error family does not depend on clim in any bit. An fp32 rounding stands where the reference rounds
   an fp32 tensor (slice mean, root, quotient, batch mean). Rows are read as float4 when W % 4 == 0 and pred, gt, clim
   are 16-byte aligned, else element by element. The weight tables are cached in the context per H: the first call
   at a height uploads them and waits for that copy; later calls are queued without a host wait (a first call or a
   larger shape also allocates the workspace). Counted by the profiler in class 4 (misfit) as one group of
   4*B*C*H*W*(clim ? 3 : 2) bytes.
   VV_E_ARG before any device work: a null context, pred, gt, mean, std_, scale or out; B, C or W < 1; B*C > 65535;
   an H that leaves one of the three regions empty (H = 1, 2 and 4; H = 3 is the smallest height with three rows
   sets, H = 5 gives rows [0,2), [2,3), [3,5)). */
enum {
  VV_VERIFY_WRMSE = 0, VV_VERIFY_NWRMSE, VV_VERIFY_SWRMSE, VV_VERIFY_TWRMSE,
  VV_VERIFY_BIAS, VV_VERIFY_NBIAS, VV_VERIFY_SBIAS, VV_VERIFY_TBIAS,
  VV_VERIFY_CHANNEL_MSE, VV_VERIFY_MSE, VV_VERIFY_MAE,
  VV_VERIFY_ACTIVITY, VV_VERIFY_NACTIVITY, VV_VERIFY_SACTIVITY, VV_VERIFY_TACTIVITY,
  VV_VERIFY_ANOMALY, VV_VERIFY_NANOMALY, VV_VERIFY_SANOMALY, VV_VERIFY_TANOMALY,
  VV_VERIFY_WACC, VV_VERIFY_NWACC, VV_VERIFY_SWACC, VV_VERIFY_TWACC,
  VV_VERIFY_NSTAT
};
int vv_verify(vv_ctx* ctx, const float* pred, const float* gt, const float* clim, const float* mean,
              const float* std_, const double* scale, int B, int C, int H, int W, double* out, void* stream);
/* held-out observation verification of --use_eval (da_4dvar.py:1154-1155 sc4dvar, :1285-1286 vae4dvar): the analysis
   against the station observations that H * (1 - mask_eval) kept out of the assimilation (:934-937),
     err[c] = sqrt( sum_p (x_aug[c][p]-yo[c][p])^2 * mask[p] * Hmask[c][p]  /  sum_p mask[p] * Hmask[c][p] )
   x (C,Hs,Ws) state; yo, Hmask (C_obs,Hs,Ws), Hmask the ORIGINAL station mask (H_old); mask (Hs,Ws) the pixel mask
   shared by all channels (mask_eval); interp (n_out,n_in) DEVICE pointer or NULL (identity, C_obs = C, n_out / n_in
   ignored); with an operator C = 4 + 5*n_in and C_obs = 4 + 5*n_out, applied in registers as vv_obs_augment applies it
   (x_aug is never stored). err (C_obs) fp32 device; sums (2*C_obs doubles, device, may be NULL): {numerator,
   denominator} per channel. Each term is formed in fp32 in the reference's order, ((d*d)*mask)*Hmask and mask*Hmask,
   and summed in fp64 in a fixed order without atomics (two calls are bitwise equal); err = sqrtf((float)num /
   (float)den), so a channel without a held-out observation is NaN (0/0) as in the reference. Only pixels with
   mask != 0 are read beyond the mask itself: a pixel with mask == 0 adds exactly 0 to both sums (for finite fields
   whose squared misfit does not overflow; the reference's inf * 0 = NaN at such a pixel is not reproduced).
   Hs*Ws < 2^31 - 4096. Counted by the profiler in class 4 (misfit). No synchronisation (the first call, or a larger
   shape, allocates the context's partial-sum workspace). */
int vv_obs_error(vv_ctx* ctx, const float* x, const float* yo, const float* Hmask, const float* mask,
                 const float* interp, int n_out, int n_in, int C, int Hs, int Ws, float* err, double* sums,
                 void* stream);
/* quality control of real observations: the departure filter of get_obs_info for the obs_type real* family
   (da_4dvar.py:764-800), in place on the device. gt (T,C,Hs,Ws) the truth window; yo, Hmask (T,C_obs,Hs,Ws) the
   gridded station observations and their mask, both UPDATED IN PLACE; interp (n_out,n_in) DEVICE pointer or NULL
   (identity, C_obs = C, n_out / n_in ignored), with an operator C = 4 + 5*n_in and C_obs = 4 + 5*n_out; thr (C_obs)
   fp32 device, filter_coeff * std_layer_aug (:779); counts (2*T doubles, device, may be NULL).
   The "z block" is channels 4 .. 4+n_out-1, the first interpolated variable (geopotential); it equals the
   reference's hard-coded 4:44 at interp_dim 40 (n_out = 40). flags, by obs_type prefix in the reference's order:
     real_simu_nofilteringz  FILTER | EXEMPT_Z | YO_SIMU      real_simuz  FILTER | EXEMPT_Z | YO_SIMU_Z
     real_simu_nofiltering   YO_SIMU      real_simu  FILTER | YO_SIMU      real  FILTER
   Per element (t, c, p) with h = Hmask[t][c][p]:
     h == 0: Hmask keeps its bits; yo becomes +0 on a simu channel (every channel under YO_SIMU, the z block under
             YO_SIMU_Z) and is untouched otherwise; neither gt nor yo is read, so junk (NaN included) at unobserved
             entries changes no output bit. The reference's gt_aug * 0 gives -0 for a negative gt_aug and NaN for a
             non-finite one; that is not reproduced.
     h != 0: g = x_aug(gt)[t][c][p] as vv_obs_augment forms it (the same j order, the level column in registers,
             interp in LDS; x_aug is never stored); m = 1 unless FILTER applies to the channel (not the z block under
             EXEMPT_Z), then d = yo - g in fp32 and m = (d < thr[c]) && (d > -thr[c]), both strict, a NaN d rejected;
             h' = h * m in fp32 is stored to Hmask (only where m == 0: h * 1 has h's bits); yo = g * h' on a simu
             channel, else unchanged.
   counts[2t] = sum h and counts[2t+1] = sum h' over (c, p) of time t, the amounts printed at :768 and :793, summed in
   fp64 in a fixed order without atomics (two calls on the same inputs are bitwise equal). Hmask is read, not assumed
   binary, and is the only field read densely: a pixel's level column is gathered only where a channel of its group
   has h != 0, yo is read only where the filter applies and h != 0, and flags = FILTER writes rejected entries only.
   VV_E_ARG: a null context, gt, yo, Hmask or thr; T, C, Hs or Ws < 1; with an operator C != 4 + 5*n_in, n_in outside
   1..16 or n_out outside 1..64; flag bits outside 0..15; EXEMPT_Z without FILTER; both YO_SIMU bits; EXEMPT_Z or
   YO_SIMU_Z with interp == NULL; yo == Hmask; Hs*Ws >= 2^31 - 4096. Counted by the profiler in class 4 (misfit). No
   synchronisation (the first call, or a larger shape, allocates the context's partial-count workspace). */
#define VV_QC_FILTER     1  /* apply the departure test */
#define VV_QC_EXEMPT_Z   2  /* channels 4 .. 4+n_out-1 always pass (mask[:, 4:44] = 1, :782) */
#define VV_QC_YO_SIMU    4  /* yo = gt_aug * H' in every channel (:797-798) */
#define VV_QC_YO_SIMU_Z  8  /* yo = gt_aug * H' in channels 4 .. 4+n_out-1 only (:795-796) */
int vv_obs_qc(vv_ctx* ctx, const float* gt, float* yo, float* Hmask, const float* interp, int n_out, int n_in,
              const float* thr, int flags, int T, int C, int Hs, int Ws, double* counts, void* stream);
/* gridding of station reports: data_reader.get_real_obs (da_4dvar.py:301-440, VV_GRID_REAL) and, for obs_type
   prepbufr*, get_obs_mask (:190-274, VV_GRID_MASK) on the device. reports (n, 12) fp64 DEVICE table, one row per
   message in the files' order (vaevar.reports.pack_reports):
     src lon lat plev dt p z q u v t msl
   position = [lon, lat, plev, dt], value = [p, z, q, u, v, t, _, msl], a JSON null as NaN; src 0 the file at tstamp, 1
   the file at tstamp + cycle_time (read for da_win 6 only: at da_win 1 its rows are skipped). bounds (n_lev - 1),
   log_lev, zcoef, tcoef (n_lev each) fp64 DEVICE level tables (vaevar.reports.level_tables: the geometric means of
   neighbouring levels of :311-313, log(height_level_new), and the coefficient functions of :315-327 per index; mask
   mode takes the twelve `height` values of :195 as bounds and ignores the other three, which may be NULL). yo, Hmask
   (da_win, 4 + 5*n_lev, Hs, Ws) fp32 are OVERWRITTEN COMPLETELY (the caller does not pre-zero); stats 4 int64 on the
   device or NULL. Nothing synchronises (a first call, or a larger table, allocates the context's pair workspace).
   Per row, in fp64 and in the reference's order of tests:
     skipped   lon, lat, plev or dt NaN (:376); then, after the indices below, dt outside the time bins:
               da_win 1: t = 0 iff -0.5 <= dt < 0.5; da_win 6, src 0: [-0.5,0.5) 0, [0.5,1.5) 1, [1.5,2.5) 2, >= 2.5 3;
               src 1: < -2.5 3, [-2.5,-1.5) 4, [-1.5,-0.5) 5
     indices   lon_i = rint(lon / 360 * Ws) (ties to even, np.round), Ws -> 0; lat_i = rint((90 - lat) / 180 * Hs)
               (times Hs, not Hs - 1: the reference's / 180 * 721), Hs -> Hs - 1; an index in [-size, -1] wraps as Python
               indexing does (lon -10 degrees lands at 1400 of 1440)
     dropped   any other index, or a NaN p in the real mode: the reference raises there. THE ONE DIVERGENCE: the row
               is dropped and counted in stats[2]
     level     h = #{k : bounds[k] <= p} (:384); the mask mode takes plev instead of p, and a NaN p is fine there
   A value is MISSING if it is NaN OR EQUAL TO 0.0: the reference tests `if elem_arr[i]:` on the raw value, so a
   temperature of 0 degrees C, a calm wind component and the like are dropped. The quirk is kept.
   VV_GRID_REAL, with d = log p - log_lev[h]: z*9.8 + zcoef[h]*d, q*1e-6, u, v, t + 273.15 + tcoef[h]*d to layer
   4 + h + i*n_lev (i = 0..4, :340-357); msl*100 to layer 3 (:359-362); where h == n_lev - 1 also u, v, t + 273.15 to
   layers 0, 1, 2 (:364-370). Every operation rounds on its own in fp64 (no contraction); only the fp64 log may differ
   from numpy's in its last bit. Each value is rounded to fp32 and the values of a cell are added IN FP32 IN ROW ORDER
   (`obs[...] += value` on an fp32 tensor); yo = sum / float(count), an IEEE fp32 division; H = 1; an unobserved cell
   is exactly 0 in both. Two calls on the same table are bitwise equal.
   VV_GRID_MASK: H = 1 at layer 4 + h + i*n_lev for each present value[1..5] and at layer 3 for a present msl, no
   surface assignment, then H[:, k] = H[:, 4 + (k+2)*n_lev + n_lev-1] for k = 0, 1, 2 (:272-274; n_lev = 13 gives the
   reference's 42, 55, 68). yo is not touched and may be NULL.
   stats: rows used (a time level and a cell position, whether or not a value is present), rows skipped, rows dropped,
   and the number of cells with H = 1 (H.sum()).
   VV_E_ARG: a null context or Hmask; a mode other than the two; da_win other than 1 or 6 (the reference raises, :306);
   n < 0, or n > 0 with reports NULL; n_lev outside 1..64; Hs or Ws < 1; bounds NULL with n_lev > 1; in the real mode a
   NULL yo, log_lev, zcoef or tcoef; yo == Hmask; da_win*(4 + 5*n_lev)*Hs*Ws >= 2^31; 9*n + 1 >= 2^31. Counted by
   the profiler in class 4 (misfit). */
#define VV_GRID_REAL 0
#define VV_GRID_MASK 1
int vv_obs_grid(vv_ctx* ctx, const double* reports, int64_t n, int mode, int da_win, int n_lev, int Hs, int Ws,
                const double* bounds, const double* log_lev, const double* zcoef, const double* tcoef, float* yo,
                float* Hmask, long long* stats, void* stream);
/* synthetic observations for obs_type free_NNNN (get_obs_mask, da_4dvar.py:276-292), the observation noise of
   get_obs_gt (:449, commented out in the reference) and the static R of get_static_info (:630-634) in one pass on the
   device: gt (T, C, Hs, Ws) fp32, the truth window, becomes yo, Hmask and R of the same shape, all OVERWRITTEN
   COMPLETELY (the caller does not pre-zero). Every bit is a function of the arguments: two calls are bitwise equal, and
   a resumed cycle that passes the same (seed, draw) redraws the same network. Nothing synchronises (a first call, or a
   larger grid, allocates the context's workspace) and nothing is read back.
   Generator: Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85; one round
   (c0,c1,c2,c3) <- (hi(M1*c2)^c1^k0, lo(M1*c2), hi(M0*c0)^c3^k1, lo(M0*c0)), then k0 += W0, k1 += W1; ten rounds) with
   the key (seed & 0xffffffff, seed >> 32); counter word 3 = draw, word 2 = the stream (1 mask, 2 noise).
   Network: key32(p) = output word 0 of counter (p, 0, 1, draw) under `seed`, p the row-major cell < Hs*Ws; the network
   is the n_obs cells smallest in the lexicographic order (key32, p): a uniform n_obs-subset, unique because the
   position breaks ties. Hmask[t][c][p] = 1.0f on it and +0.0f off it, for every t and c (the reference stacks one
   matrix 69 times and adds it to every time slot). np.random.choice is not reproduced: it draws from numpy's global
   Mersenne Twister.
   Noise: element e = (t*C + c)*Hs*Ws + p, g = e >> 2, (w0..w3) = the output of counter (g & 0xffffffff, g >> 32, 2,
   draw) under `noise_seed`; u1(w) = ((w >> 8) + 1) * 2^-24 in (0, 1], u2(w) = (w >> 8) * 2^-24 in [0, 1), r(w) =
   sqrtf(-2 * logf(u1(w))); eps(e) = r(w0)*cospif(2*u2(w1)), r(w0)*sinpif(2*u2(w1)), r(w2)*cospif(2*u2(w3)),
   r(w2)*sinpif(2*u2(w3)) for e & 3 = 0, 1, 2, 3. yo[e] = gt[e] + sd[c]*eps(e), the fp32 product rounded, then the fp32
   sum (no contraction), at every cell, observed or not: yo does not depend on the mask. sd (C) DEVICE fp32 standard
   deviations, or NULL: yo is gt copied as 32-bit words (NaN payloads, -0.0 and subnormals kept) and no Philox call of
   the noise stream is evaluated. yo == gt is allowed (in place).
   R[t][c][p] = rtab[t*C + c]; rtab (T*C) DEVICE fp32 (vaevar.problem.r_table). R and rtab are both given or both NULL.
   stats: 2 int64 on the device or NULL: the number of selected cells (= n_obs) and the number of cells whose key32
   equals the threshold key, i.e. the largest selected key (0 for n_obs = 0).
   VV_E_ARG, decided before any device work: a null context, gt, yo or Hmask; T, C, Hs or Ws < 1; T*C*Hs*Ws >= 2^31;
   n_obs < 0 or n_obs > Hs*Ws (np.random.choice(..., replace=False) raises there); exactly one of R and rtab NULL;
   Hmask or R overlapping gt, yo or each other; yo overlapping gt without being equal to it. Counted by the profiler in
   class 4 (misfit). */
int vv_obs_synth(vv_ctx* ctx, const float* gt, int T, int C, int Hs, int Ws, int64_t n_obs, unsigned long long seed,
                 unsigned long long noise_seed, unsigned draw, const float* sd, const float* rtab, float* yo,
                 float* Hmask, float* R, long long* stats, void* stream);
/* the selection of vv_obs_synth on the caller's keys: mask[i] = 1.0f for the k entries of keys (n uint32, DEVICE)
   that are smallest in the order (keys[i], i), +0.0f for the others; mask (n) fp32 is overwritten completely. stats as
   in vv_obs_synth. Exact and deterministic for any 0 <= k <= n and any keys, equal ones included: a radix select over
   the key bits (three passes; the keys are read, never sorted or moved) and, among the entries equal to the threshold
   key, the lowest positions. No read-back, no synchronisation. VV_E_ARG: a null context, keys or mask; n < 1 or
   n >= 2^31; k < 0 or k > n. */
int vv_select_smallest(vv_ctx* ctx, const unsigned* keys, int64_t n, int64_t k, float* mask, long long* stats,
                       void* stream);
/* out[i] = eps(first + i), i < n, of vv_obs_synth's noise stream under the noise seed `seed` and `draw`: the same
   device function, hence the same bits as the eps the fill adds. n = 0 is a no-op. VV_E_ARG: a null context; out NULL
   with n > 0; n < 0, first < 0 or first + n beyond int64. */
int vv_normal_fill(vv_ctx* ctx, float* out, int64_t n, int64_t first, unsigned long long seed, unsigned draw,
                   void* stream);
/* Model-error statistics (calculate_q, model/model.py:469-490; the per-channel moments of :538-593) and the static R
   of get_static_info (da_4dvar.py:630-634) on the device. None of the three calls synchronises or reads anything
   back; a first call, or a larger shape, allocates the context's workspace (the chunk sums of the channel totals), and
   a call that writes no channel total allocates nothing. The profiler counts them in class 4 (misfit). VV_E_ARG is
   decided before any device work.

   vv_err_accum: one step of `error_var += ((output - batch[1:2])**2).numpy()` (:485-486) for B samples. pred and tgt
   are fp32 DEVICE fields; sample b starts at pred + b*pred_bstride (tgt + b*tgt_bstride) and holds at least C
   contiguous (H, W) channels, of which the first C are read. The strides are in elements, so pred may be a network's
   (B, 138, H, W) output and tgt the time slice window[:, k] of a (B, L+1, C, H, W) window (stride (L+1)*C*H*W) with no
   slice copy. cell (C, H, W) and chan (C) are fp64 DEVICE accumulators updated in place; either may be NULL.
   Per cell e = (c, p), for b = 0 .. B-1 in that order: d = pred - tgt in fp32, s = d*d in fp32 (rounded on its own),
   cell[e] = cell[e] + (double)s. Successive calls continue the sequence, so the samples enter in the order (call, b)
   and cell equals the numpy loop over those samples bit for bit.
   chan[c] = chan[c] + S, S the fp64 sum of (double)d over the B*H*W differences of the channel in a fixed order: a
   thread adds its cells ascending, the samples of a cell in order; the 64 lanes of a wave, the 4 waves of a workgroup
   (4096 consecutive cells) and the workgroups of a channel (ascending) are added in a fixed tree. There are no
   atomics: two runs on equal inputs give equal bits. |S - exact| <= 2*N*2^-53 * sum|d| for N = B*H*W terms.
   A NaN or Inf in pred or tgt reaches cell[e] of its own cell and chan[c] of its own channel, nothing else.
   Rows move as 16-byte accesses when H*W % 4 == 0, both strides are multiples of four and pred, tgt and cell are
   16-byte aligned; otherwise element by element, with the same results.
   VV_E_ARG: a null context, pred or tgt; cell and chan both NULL; B, C, H or W < 1; C*H*W >= 2^31; a stride below
   C*H*W. */
int vv_err_accum(vv_ctx* ctx, const float* pred, int64_t pred_bstride, const float* tgt, int64_t tgt_bstride, int B,
                 int C, int H, int W, double* cell, double* chan, void* stream);
/* `error_var / total_step` (model/model.py:490) and the table of init_q_matrix, q_type 0 (da_4dvar.py:535-536):
   q_field[e] = cell[e] / (double)n_samples, one IEEE fp64 division per cell, hence numpy's bits; q_tab[c] = (the fp64
   sum of q_field[c] over its H*W cells, in vv_err_accum's fixed order) / (double)(H*W), which is
   torch.mean(q0, (1, 2)) up to the order of the sum: relative difference <= 2*H*W*2^-53 (no term is negative).
   cell, q_field (C, H, W) and q_tab (C) are fp64 on the DEVICE. Either output may be NULL; q_field may equal cell
   (in place). q_tab is computed from the quotients whether or not q_field is stored.
   VV_E_ARG: a null context or cell; both outputs NULL; n_samples < 1; C, H or W < 1; C*H*W >= 2^31. */
int vv_err_finalize(vv_ctx* ctx, const double* cell, int64_t n_samples, int C, int H, int W, double* q_field,
                    double* q_tab, void* stream);
/* The dense R from its (T, C) table rtab (DEVICE fp32, row t = obs_var + q[t-1]; vaevar.problem.static_r_table): the
   broadcast of get_static_info (:631-634) and, with an operator, get_R_matrix_from_gt (:729-756) of that broadcast,
   without the dense intermediate. R is OVERWRITTEN COMPLETELY; the kernel loads the table and only stores fields
   (16 bytes per lane when Hs*Ws % 4 == 0 and R is 16-byte aligned).
   interp NULL: R (T, C, Hs, Ws), R[t][c][p] = rtab[t*C + c].
   interp (n_out, n_in) fp32 on the DEVICE, C = 4 + 5*n_in: R (T, 4 + 5*n_out, Hs, Ws); channels 0..3 are rtab[t][0..3];
   channel 4 + n_out*i + o holds y = sum_j interp[o][j] * rtab[t][4 + n_in*i + j], formed as vv_obs_augment forms it
   (y = 0, then y = fma(interp[o][j], x[j], y) for j ascending), so R equals vv_obs_augment of the broadcast field bit
   for bit.
   VV_E_ARG (vv_obs_augment's limits): a null context, rtab or R; T, C, Hs or Ws < 1; with interp, n_in outside 1..16,
   n_out outside 1..64 or C != 4 + 5*n_in; a field of 2^31 workgroups (4096 cells each) or more. */
int vv_r_fill(vv_ctx* ctx, const float* rtab, const float* interp, int n_out, int n_in, int T, int C, int Hs, int Ws,
              float* R, void* stream);
/* Departure statistics of an assimilation window: the moments of the background departures d_b = yo - H(xb_t) and the
   analysis departures d_a = yo - H(xa_t) per time level and observation channel, from which the consistency relations
   of Desroziers et al. (2005) are formed: E[d_a d_b] ~ R, E[(d_b - d_a) d_b] ~ H B H^T, E[d_b^2] ~ H B H^T + R,
   2 J_o(xa) / N < 1. This checks the R that vv_r_fill / vv_obs_synth prescribe. It is not in the reference.
   xb_win, xa_win (T, C, Hs, Ws) fp32 physical states, the two trajectories over the window; xa_win may be NULL. yo,
   Hmask, R (T, C_obs, Hs, Ws) fp32. interp (n_out, n_in) DEVICE pointer or NULL (identity, C_obs = C, n_out / n_in
   ignored); with an operator C = 4 + 5*n_in and C_obs = 4 + 5*n_out. out (T, C_obs, VV_OSTAT_N) fp64 on the DEVICE is
   OVERWRITTEN COMPLETELY. Inputs are read only; xa_win == xb_win is allowed.
   The observed set of a row (t, c) is S = {p : Hmask[t][c][p] != 0.0f}; Hmask is read, not assumed binary. For p in S:
   x_b = channel c of the operator applied to xb_win[t] at p, as vv_obs_augment forms it (the same j order, the level
   column in registers; x_aug is never stored), x_a the same from xa_win; d_b = yo - x_b and d_a = yo - x_a, one fp32
   subtraction each; h = Hmask[t][c][p], r = R[t][c][p]. The rows are fp64 sums over S:
     VV_OSTAT_COUNT 1.0            VV_OSTAT_H  (double)h          VV_OSTAT_R  (double)r
     VV_OSTAT_OB    (double)d_b    VV_OSTAT_OB2  (double)d_b*(double)d_b    VV_OSTAT_JB  (double)((h*(d_b*d_b))/r)
     VV_OSTAT_OA    (double)d_a    VV_OSTAT_OA2  (double)d_a*(double)d_a    VV_OSTAT_JA  (double)((h*(d_a*d_a))/r)
     VV_OSTAT_OAOB  (double)d_a*(double)d_b
   The fp64 products of two widened fp32 values are exact. The JB / JA term is the fp32 term of the closure's J_o,
   widened afterwards: 0.5 * sum over (t, c) of row JA is J_o at the analysis up to the order of the fp64 sums.
   With xa_win == NULL rows OA, OA2, OAOB and JA are NaN and xa_win is never read (as clim in vv_verify).
   Sums follow vv_err_accum's fixed order: a thread adds its cells ascending; the 64 lanes of a wave, the 4 waves of a
   workgroup (4096 consecutive cells of a plane) and the workgroups of a plane (ascending) are added in a fixed tree,
   so |S - exact| <= 2*N*2^-53 * sum|term| for N = Hs*Ws. No atomics: two calls on equal inputs give equal bits, and
   a row's bits depend neither on T nor on the other channels (slice t of a T = 3 call equals the T = 1 call on it).
   Hmask is the only field read densely: yo, R and the states are read only where h != 0 (with an operator a pixel's
   level column only where the channel at hand is observed), so junk, NaN included, at unobserved entries changes no
   output bit. A NaN, Inf or r == 0 at an observed entry stays in its own (t, c) row. Rows move as 16-byte accesses
   when Hs*Ws % 4 == 0 and the five fields are 16-byte aligned; otherwise element by element, with the same results.
   No synchronisation and no read-back (the first call, or a larger shape, allocates the context's partial workspace).
   Counted by the profiler in class 4 (misfit) as one group with the algorithmic bytes of a fully observed window,
   4*Hs*Ws*T*(3*C_obs + (xa_win ? 2 : 1)*C).
   VV_E_ARG, decided before any device work: a null context, xb_win, yo, Hmask, R or out; T, C, Hs or Ws < 1; with an
   operator n_in outside 1..16, n_out outside 1..64 or C != 4 + 5*n_in; Hs*Ws >= 2^31 - 4096; 2^31 workgroups (one per
   row and 4096 cells) or more. */
enum {
  VV_OSTAT_COUNT = 0, /* number of observed entries */
  VV_OSTAT_H = 1,
  VV_OSTAT_OB = 2,
  VV_OSTAT_OA = 3,
  VV_OSTAT_OB2 = 4,
  VV_OSTAT_OA2 = 5,
  VV_OSTAT_OAOB = 6,
  VV_OSTAT_R = 7,
  VV_OSTAT_JB = 8,
  VV_OSTAT_JA = 9,
  VV_OSTAT_N = 10 /* rows of a table */
};
int vv_obs_stats(vv_ctx* ctx, const float* xb_win, const float* xa_win, const float* yo, const float* Hmask,
                 const float* R, const float* interp, int n_out, int n_in, int T, int C, int Hs, int Ws, double* out,
                 void* stream);
/* Evaluating a VAE (nf_model/vae.py:72-107: VAE_lr.encoder's chunk, sampling, loss_function; the training sample of
   vae_nmc_model.train, model/model.py:593-596) on the device. Forwards only: no weight gradient. The three calls queue
   on `stream`, read nothing back and do not synchronise; a first call, or a larger shape, allocates the context's
   workspace (the chunk sums, shared with vv_err_accum); they use no atomics, so two calls on equal inputs give equal
   bits. The profiler counts them in class 4 (misfit). VV_E_ARG is decided before any device work. Sums are fp64 and
   follow vv_err_accum's fixed order: a thread adds its cells ascending; the 64 lanes of a wave, the 4 waves of a
   workgroup (4096 consecutive cells of a plane) and the workgroups of a plane (ascending) are added in a fixed tree, so
   |S - exact| <= 2*N*2^-53 * sum|term| for the N = H*W terms of a plane.

   vv_vae_sample: `encoded.chunk(2, dim=1)` (:76), `sampling` (:78-81) and the summand of the KLD (:106) in one pass over
   the encoder output. enc is (B, 2L, H, W) fp32 on the DEVICE; mu = channels [0, L), log_var = channels [L, 2L).
   z is (B, L, H, W) fp32 or NULL. With e = (b*L + l)*H*W + p the element index in z, eps(e) is the value
   vv_normal_fill writes to out[e] for (first = 0, seed, draw): the same device function, the same bits. Per element
       s = (float)exp(0.5 * (double)log_var)        the fp64 exponential rounded once, hence within half an fp32 ulp
                                                    (plus the fp64 routine's error) whatever the device's expf does
       z = fl32(fl32(eps * s) + mu)                 the reference's eps.mul(std).add_(mu): no contraction
   With VV_VAE_MEAN in flags z is mu copied as 32-bit words (the posterior mean) and no noise is evaluated; seed and
   draw are ignored.
   stat is (B, L, 4) fp64 or NULL and is OVERWRITTEN: for the plane (b, l), in fp64 from the fp32 inputs,
       stat[0] = sum_p t,  t = ((1 + log_var) - mu*mu) - exp(log_var)      KLD of the plane = -0.5 * stat[0] (:106)
       stat[1] = sum_p mu,  stat[2] = sum_p mu*mu,  stat[3] = sum_p exp(log_var).
   DEVIATION: the reference rounds every summand to fp32 and adds them in fp32 in torch.sum's order; here the terms are
   fp64 and the sum follows the fixed tree above. stat does not depend on z, seed, draw or flags.
   A NaN or Inf in enc reaches its own element of z and the row (b, l) of stat, nothing else.
   Rows move as 16-byte accesses when H*W % 4 == 0 and enc and z are 16-byte aligned; otherwise element by element,
   with the same results.
   VV_E_ARG: a null context or enc; z and stat both NULL; B, L, H or W < 1; B*2L*H*W >= 2^31; z overlapping enc; flag
   bits other than VV_VAE_MEAN. */
#define VV_VAE_MEAN 1
int vv_vae_sample(vv_ctx* ctx, const float* enc, int B, int L, int H, int W, unsigned long long seed, unsigned draw,
                  int flags, float* z, double* stat, void* stream);
/* The reconstruction term `torch.sum((recon_x - x)**2)` (:105) per sample and channel: sse (B, C) fp64 on the DEVICE is
   OVERWRITTEN with sum_p (double)fl32(d*d), d = fl32(recon - x): the reference's fp32 elements, summed in fp64 in the
   fixed order above (the reference adds them in fp32). recon and x are fp32 DEVICE fields addressed as vv_err_accum
   addresses pred and tgt: sample b starts at recon + b*recon_bstride (x + b*x_bstride) and holds at least C contiguous
   (H, W) channels, strides in elements, so recon may be a wider network output. A NaN or Inf reaches sse[b][c] of its
   own sample and channel only. 16-byte accesses when H*W % 4 == 0, both strides are multiples of four and recon and x
   are 16-byte aligned.
   VV_E_ARG: a null context, recon, x or sse; B, C, H or W < 1; C*H*W >= 2^31; a stride below C*H*W; 2^31 workgroups
   (4096 cells each) or more. */
int vv_vae_sse(vv_ctx* ctx, const float* recon, int64_t recon_bstride, const float* x, int64_t x_bstride, int B, int C,
               int H, int W, double* sse, void* stream);
/* The VAE's training sample `err = (pred2 - pred1) / err_std; err = F.interpolate(err, (Hn, Wn))` (model/model.py:593-596):
   out[b][c][i][j] = (tgt[b][c][si][sj] - pred[b][c][si][sj]) / err_std[c] in fp32, one IEEE subtraction and one IEEE
   division, with si = map_H[i], sj = map_W[j] the source indices vv_nearest_map(Hs, Hn) / (Ws, Wn) gives
   (F.interpolate mode 'nearest'); the maps are evaluated in the kernel by the same rule. Selecting elements commutes
   with the elementwise arithmetic, so out equals the reference's "divide on (Hs, Ws), then interpolate" bit for bit.
   With Hs == Hn and Ws == Wn the maps are the identity. pred and tgt are addressed as in vv_err_accum (strides in
   elements, C contiguous (Hs, Ws) channels per sample); err_std is (C) fp32 on the DEVICE; out (B, C, Hn, Wn) is
   OVERWRITTEN COMPLETELY and must not overlap pred or tgt.
   VV_E_ARG: a null context, pred, tgt, err_std or out; B, C, Hs, Ws, Hn or Wn < 1; C*Hs*Ws >= 2^31; B*C*Hn*Wn >= 2^31;
   a stride below C*Hs*Ws. */
int vv_err_sample(vv_ctx* ctx, const float* pred, int64_t pred_bstride, const float* tgt, int64_t tgt_bstride, int B,
                  int C, int Hs, int Ws, const float* err_std, int Hn, int Wn, float* out, void* stream);
/* da_mode 'interpolation' (one_step_DA, da_4dvar.py:968-1061): per observation channel the reference
   Delaunay-triangulates the observed cells of time level 0 and fills every unobserved cell inside their hull with
   scipy.interpolate.griddata(known_coords, known_values, unknown_coords, method='linear') (:1017-1027). The host keeps
   the triangulation (vaevar.interp.pack_triangles: scipy.spatial.Delaunay of a channel's observed cells, as griddata
   runs it); this call rasterises the simplices into the field. Cells and vertices are both lattice points, so the
   simplex of a cell and its barycentric weights are exact integer edge functions.
   tris: DEVICE table of n_tri rows of VV_TRI_COLS int32, the rows of one channel contiguous and in scipy's simplex
   order:
     ch r0 c0 r1 c1 r2 c2 nb0 nb1 nb2 work_begin work_end
   (rk, ck) vertex k as (row, column); nbk the table row of the simplex across the edge opposite vertex k, -1 on the
   hull (Delaunay.neighbors plus the channel's first row). The last two columns number the work items of the call: a
   row's bounding box is cut into tiles of VV_TRI_BAND rows x VV_TRI_SEG columns, ((rmax - rmin) / VV_TRI_BAND + 1) *
   ((cmax - cmin) / VV_TRI_SEG + 1) of them, work_begin is the number of tiles of all rows before it and work_end =
   work_begin + its own (so no wave walks a large box alone; the last row's work_end is the total, < 2^31).
   yo, Hmask, xa (C, Hs, Ws) fp32; xa holds the background in observation space and is UPDATED IN PLACE.
   Per row, with A = (r1-r0)(c2-c0) - (c1-c0)(r2-r0), and per cell (r, c) of its bounding box
     e0 = (r1-r)(c2-c) - (c1-c)(r2-r),  e1 = (r2-r)(c0-c) - (c2-c)(r0-r),  e2 = A - e0 - e1,
   all three multiplied by sign(A) (and A by it): the cell belongs to the row if e0, e1, e2 >= 0 and, for every k
   with ek == 0, nbk == -1 or the row's index < nbk. That is "the lowest simplex index that contains the cell" decided
   locally: one writer per cell, no atomics on the field; hull edges are inclusive as in scipy's find_simplex.
   The cell is written only if Hmask[ch][r][c] == 0.0f: observed cells KEEP THE BACKGROUND, not the observation (the
   reference assigns xa[i][b == 0] only), and a mask value that is neither 0 nor 1 leaves its cell alone. The value is
     ((e0*v0 + e1*v1) + e2*v2) / A   with vk = (double)yo[ch][rk][ck],
   in fp64 with every operation rounded on its own (no contraction), rounded once to fp32; a NaN result is not written
   (xa[isnan] = xb0[isnan], :1029-1030), nor is any cell outside the hull or of a channel without rows (the caller
   gives no rows to a channel with <= 10 observed cells, :1025).
   The table is NOT TRUSTED: a row whose ch is outside [0, C), with a coordinate outside the grid, a neighbour outside
   [-1, n_tri) or A == 0 is skipped and counted, and no table content can move a write out of xa (a wrong prefix can
   only lose cells). stats: 3 int64 on the device or NULL: rows used, rows skipped, cells written.
   No synchronisation; two calls on the same inputs give the same bits. Counted by the profiler in class 4 (misfit).
   VV_E_ARG: a null context, yo, Hmask or xa; n_tri < 0 or >= 2^31, or n_tri > 0 with tris NULL; C, Hs or Ws < 1; Hs
   or Ws > 16384 (the int32 edge functions); xa overlapping yo or Hmask. */
#define VV_TRI_COLS 12
#define VV_TRI_BAND 16
#define VV_TRI_SEG 64
int vv_tri_interp(vv_ctx* ctx, const int* tris, int64_t n_tri, const float* yo, const float* Hmask, float* xa, int C,
                  int Hs, int Ws, long long* stats, void* stream);
/* the way back from observation space (da_4dvar.py:1033-1044): x (T, 4 + 5*n_out, Hs, Ws) from x_aug
   (T, 4 + 5*n_in, Hs, Ws); channels 0..3 are copied, x[4 + n_out*i + o] = sum_j interp_inv[o][j] x_aug[4 + n_in*i + j]
   for the five variables i, in fp32 with j ascending. interp_inv (n_out, n_in) fp32 on the DEVICE
   (obs_interpolater.interp_inv: n_in = 40 levels to n_out = 13); the sum is dense whatever the matrix holds.
   vv_obs_augment is the other direction (n_in <= 16 there). No synchronisation; profiler class 4.
   VV_E_ARG: a null context, interp_inv, x_aug or x; n_in outside 1..64, n_out outside 1..16; T, Hs or Ws < 1;
   x == x_aug. */
int vv_obs_project(vv_ctx* ctx, const float* interp_inv, int n_out, int n_in, const float* x_aug, float* x, int T,
                   int Hs, int Ws, void* stream);
/* trajectories x_t (B,T,C,Hs,Ws) of the last EVALUATED closure / forward (device pointer, read-only): a closure
   answered from the memo (vv_closure_recall, vv_closure's lookup) evaluates nothing and leaves them as they were. On an
   interpolated state grid with the one-pass misfit ("grid_fused", config 5) a gradient closure does not store x_t (the
   state fields are read once and nothing is written at the state grid); a J-only evaluation (cal_loss, vv_closure with
   grad_z = NULL) does, so the per-outer-pass logging of da_4dvar.py:1256-1262 sees the pass's x_t. */
int vv_state_ptr(vv_ctx* ctx, const float** x);

/* vector primitives (n floats). Host-returning ones synchronise `stream`.
   Length: n = 0 is a no-op with status 0 (no operand is touched; vv_dot, vv_abssum and vv_absmax, alone or as a
   vv_reduce_batch / vv_reduce_enqueue request, give 0); n < 0 is VV_E_ARG in every one of them, vv_lbfgs_two_loop and
   vv_adam included. The pointers must be valid all the same.
   Non-finite values: vv_dot and vv_abssum accumulate in fp64 and follow IEEE 754 (a NaN element gives NaN, an
   infinite one +-inf or NaN). vv_absmax returns NaN if any element is NaN, as torch.max does (a.abs().max(), the
   optimality test of torch/optim/lbfgs.py), else the largest |a_i|, +inf included; 0 for n = 0. */
int vv_dot(vv_ctx* ctx, const float* a, const float* b, int64_t n, double* out, void* stream);
int vv_abssum(vv_ctx* ctx, const float* a, int64_t n, double* out, void* stream);
int vv_absmax(vv_ctx* ctx, const float* a, int64_t n, float* out, void* stream);
/* Several of the reductions above in one host round trip: op i = 0 dot(a[i], b[i]), 1 abssum(a[i]), 2 absmax(a[i])
   over n floats each (count <= 8), with the same kernels and partial layouts as vv_dot / vv_abssum / vv_absmax (the
   same values bit for bit, op 2 with vv_absmax's NaN rule); then n_extra (<= 16) device doubles at dev_extra (e.g.
   the J of a vv_closure_async) are appended: out[count + n_extra], one synchronisation. The L-BFGS mirror
   (vaevar/lbfgs.py) asks for the scalars of an iteration together instead of one synchronising call each
   (torch/optim/lbfgs.py computes them one by one). */
int vv_reduce_batch(vv_ctx* ctx, int count, const int* ops, const float* const* a, const float* const* b, int64_t n,
                    const double* dev_extra, int n_extra, double* out, void* stream);
/* The same reductions queued without a host round trip: the results stay in the caller's device doubles dev_out[count]
   (absmax widened exactly), to be fetched later as another call's dev_extra. The partial sums live in the context's
   reduction scratch, which vv_reduce_batch and the next vv_reduce_enqueue reuse: every such call of one context must
   go to the same stream (calls on two streams race on that scratch). */
int vv_reduce_enqueue(vv_ctx* ctx, int count, const int* ops, const float* const* a, const float* const* b, int64_t n,
                      double* dev_out, void* stream);
int vv_axpy(vv_ctx* ctx, float* y, const float* x, float alpha, int64_t n, void* stream);
int vv_axpby(vv_ctx* ctx, float* out, const float* x, float a, const float* y, float b, int64_t n, void* stream);
int vv_scale(vv_ctx* ctx, float* y, float alpha, int64_t n, void* stream);
int vv_copy(vv_ctx* ctx, float* dst, const float* src, int64_t n, void* stream);
/* L-BFGS two-loop recursion (torch/optim/lbfgs.py:404-442): q holds -g on entry and the direction d on return;
   S, Y: host arrays of m device vectors (old_stps, old_dirs, oldest first), ro[m] = 1/(y.s) (host, fp32),
   m <= 256. The dot products and coefficients stay on the device (fp32 as torch's 0-d tensors); no sync. */
int vv_lbfgs_two_loop(vv_ctx* ctx, float* q, const float* const* S, const float* const* Y, const float* ro, int m,
                      float H_diag, int64_t n, void* stream);
/* torch.optim.Adam step (no weight decay / amsgrad): step is the 1-based step count. The bias corrections
   1 - beta^step are formed in double, as torch forms them; the recurrences run in fp32. */
int vv_adam(vv_ctx* ctx, float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
            float beta2, float eps, int step, void* stream);

/* live profiler: HIP events around every kernel launch, summed per kernel class
   (0 GEMM (bf16x6 / f32), 1 window attention, 2 LayerNorm, 3 patch conv/convT, 4 misfit, 5 vector, 6 fp16x3 GEMM,
   7 fused Swin-tower sub-blocks); ncls >= 8.
   ms = summed launch durations, flops/bytes = algorithmic work, launches = count. stop synchronises. */
int vv_profile_start(vv_ctx* ctx);
int vv_profile_stop(vv_ctx* ctx, double* ms, double* flops, double* bytes, int* launches, int ncls);

/* F.interpolate(mode='nearest') source index map for in_size -> out_size (quirk Q3), as used by
   decoder_hr (nf_model/vae.py:90) and integrate (da_4dvar.py:671, 679); map has out_size entries (host) */
int vv_nearest_map(int in_size, int out_size, int* map);

/* GEMM arithmetic for every nn.Linear of the context's models (per context; default VV_GEMM_SPLIT16; the Python
   Context applies VAEVAR_GEMM_MATH=f32|split|split16 through this call, the library reads no environment):
   VV_GEMM_F32     = v_mfma_f32_32x32x2_f32, an exact fp32 fma chain (torch fp32 matmul semantics);
   VV_GEMM_SPLIT   = each fp32 operand split exactly into three bf16 planes (x = h + m + l) and the six
                     products of order >= 2^-16 accumulated in fp32 by v_mfma_f32_32x32x16_bf16;
   VV_GEMM_SPLIT16 = each fp32 operand scaled by a power of two per row (its maximum to [2^14, 2^15)) and
                     split into two fp16 planes (x = h + l, 22 bits), three products (hh, hl, lh) accumulated
                     in fp32 by v_mfma_f32_32x32x16_f16.
   Both split modes have fp32-level error (measured vs fp64, tests/test_gpu_kernels.py). */
#define VV_GEMM_F32 0
#define VV_GEMM_SPLIT 1
#define VV_GEMM_SPLIT16 2
int vv_set_gemm_math(vv_ctx* ctx, int math);
int vv_get_gemm_math(vv_ctx* ctx, int* math);

/* Per-context dispatch knobs, for A/B runs without a rebuild (defaults = the measured choices).
   Keys: "h3_mink" (smallest K on the fp16x3 kernels, 768), "h3_big" (256x128 fp16x3 tiles, 1), "h3_mf16" (their
   16x16x32-MFMA form, 1), "small_split" (whole-grid split-K of sub-chip fp16x3 GEMMs, 1), "small_split_minkt"
   (24), "tail_minkt" (k-tiles per split-K tail chunk, 12), "ln_scales" (row scales from the LayerNorm, 1),
   "win_attn" (LGUnet_all_1 LDS window attention, 1), "win_mfma" (that kernel on the exact-f32 MFMA, 1),
   "fc_h3_mink" (smallest K of the forecast network's fp16x3 GEMMs, 192), "fuse_mlp" (the fused Swin-tower
   LN2 + fc1 + GELU + fc2 + residual sub-block and its backward: bit 0 at dim 96, bit 1 at dim 192, 3), "fuse_attn" (the fused Swin-tower
   LN1 + qkv + window attention + proj + residual sub-block at dim 96: bits 0 / 1 forward / backward, 3), "attn_mfma" (the window attention of
   the LG stage, head dim 192, and of the unfused tower stages, head dim 32, on the exact-f32 MFMA, 1), "gelu_planes" (the LG-stage GELU / gelu' GEMM
   epilogues write the fp16x3 planes of the K = 4C GEMM after them, 1), "attn_planes" (the LG-stage attention
   forward writes the planes of a tile-48 proj GEMM, 1), "fixup_ln" (that GEMM's split-K fixup fused into the LN2
   after it, 1), "h4" (the split-operand LDS-DMA fp16x3 kernel, tile 48, where
   the 256x128 tiles run, 1), "ln_planes" (the LayerNorm writes that kernel's fp16 A planes, 1), "gattn" (the
   LGUnet_all_1 global window on the flash MFMA kernel, vv_attention_global, 1), "gattn_qf" (its 16-query blocks per
   wave: 1 = eight waves, two per SIMD; 2 = four waves of 32 queries, 1), "h4_small" (tile 48 with whole-chip split-K
   also for 64..143 256-row tiles, 1), "h4_split_minkt" (k-tiles per chunk of that split, 12), "h5" (tile 49, 256x144, where its
   tiles fill whole rounds of the chip and tile 48's leave a split-K tail: the N = 4608 GEMMs at 2048 rows, 1), "fc_conv_mf" (LGUnet_all_1's PatchEmbed / ConvTranspose2d as direct
   exact-f32 MFMA kernels instead of im2col / col2im + GEMM, 1), "mlp_hc" (the fused dim-192 MLP: 32 or 64 hidden units
   per chunk step, or 2 = 32-unit chunks with the hidden layer split over two waves per 16 tokens, 2), "h4_gather"
   (tiles 48 and 49 read a gathered A's producer row scales through the row map themselves instead of a
   k_gather_scales launch, 1), "fixup_ln_rows" (the fused fixup + LN1 after fc2 walks the GEMM's rows in order through the
   inverse window map, 1), "h5_split" (the N = 1152 split-K GEMMs -- those whose fixup is fused into a LayerNorm and the
   plain ones, summed by k_gemm_fixup49 -- on tile 49 with every tile split P / T ways, 256 workgroups at 2048 rows,
   instead of tile 48's 216, 1), "fixup_stage" (the fused fixup + LayerNorm reads a workgroup's split-K partials as whole 128-B lines into LDS, 1, or per row, 0), "grid_fused" (interpolated state grids, Hs >= Hl and Ws >= Wl with synthetic observations:
   the misfit reads each state field once per evaluation and its adjoint runs on the network grid, k_misfit_grid /
   k_misfit_net_bwd, 3 rows of a band in flight per pass; 2 = the same with 6 rows; read by vv_bind_problem, 1), "host_wait" (how
   vv_reduce_batch waits for the stream: 0 hipStreamSynchronize, which keeps a host CPU busy; 1 sleeps, then polls
   hipStreamQuery), "patch_pers" (the decoder PatchEmbed / ConvTranspose2d kernels in their persistent form, one
   workgroup of 8 waves per CU share with the weights staged once, bit-identical to 0 = one workgroup per 64-token
   tile, 1), "bs_tile" (the bf16x6 tile of the short-K tower GEMMs: 27 = 64x64 with one LDS buffer, 27; 24 = two buffers,
   bit-identical), "fixup_ln_cross" (the fused fixup + LN1 also between
   consecutive LG stages, 1). Results stay fp32-level for every value; a change drops the
   context's captured closure graphs. Unknown key, or a value the dispatch does not accept (switches 0 / 1; "mlp_hc"
   0, 2, 32, 64; "gattn_qf" 1, 2; "grid_fused" 0..2; "fuse_mlp" and "fuse_attn" 0..3; "bs_tile" 24, 27; the k-tile
   floors >= 1; the minimum K >= 0): VV_E_ARG, and the knob keeps its value. */
int vv_set_tuning(vv_ctx* ctx, const char* key, int value);
int vv_get_tuning(vv_ctx* ctx, const char* key, int* value);
/* process-wide debug aid: synchronise after every library launch and report the first failing op (default 0) */
int vv_set_debug_sync(int enable);

/* give a device weight B[N][K] (used as the B operand of vv_gemm) precomputed split planes, as the
   engine does for every model weight at vv_load_weights; B must stay alive and unchanged until
   vv_ctx_destroy (which frees the planes) */
int vv_gemm_register_weight(vv_ctx* ctx, const float* B, int N, int K);

/* global-window attention as LGUnet_all_1's LG layer 0 runs it (networks/LGUnet_all.py:689, 696; SD_attn without
   mask, networks/utils/Attention.py:599-664): out[t][h d_h + d] = sum_j softmax_j(q_t . k_j) v_j[d] per head h, for
   qkv [N][3C] (q already scaled by head_dim^-0.5 and rotated, k rotated, as the kernel after the qkv projection
   sees them) and out [N][C]; the flash MFMA kernel of vv_gattn.hip (fp16x3 products, fp32 softmax). head_dim 64,
   96, 128 or 192, otherwise VV_E_ARG. Kernel tests and tools; the forecast model calls the kernel itself. */
int vv_attention_global(vv_ctx* ctx, const float* qkv, float* out, int N, int C, int heads, void* stream);

/* raw GEMM entry for kernel tests: C[M][N] = A[M][K] . B[N][K]^T (+bias), K a multiple of 32. tile = -1 picks the
   kernel as the engine does; otherwise one of the library kernels: 0 / 2 / 4 exact-f32 MFMA 128x128 / 64x64 /
   32x64, 24 / 34 bf16x6 split 64x64 / pipelined 128x128, 36 / 44 fp16x3 split 128x128 / 256x128 (32x32x16 MFMAs),
   46 / 47 the same on 16x16x32 MFMAs, 48 fp16x3 256x128 on pre-split A planes staged by LDS-DMA (the engine's
   default for the LG GEMMs), 49 the same operands on 256x144 tiles (data-parallel only). Any other tile: VV_E_ARG. An fp16x3 tile whose B has no fp16 planes (not registered)
   runs tile 34. */
int vv_gemm(vv_ctx* ctx, int M, int N, int K, const float* A, const float* B, const float* bias, float* C,
            int tile, void* stream);
/* vv_gemm with the Mlp epilogues of the engine (kernel tests): epi 0 store; 1 GELU: C = gelu(acc + bias) and, when aux
   is not null, aux = acc + bias (the fc1 forward, swinblock.py:23-29); 3 GELU': C = acc * gelu'(aux) (the fc1 input
   gradient). Other epi values: VV_E_ARG. */
int vv_gemm_epi(vv_ctx* ctx, int M, int N, int K, const float* A, const float* B, const float* bias, float* C,
                float* aux, int epi, int tile, void* stream);
/* y = GELU(x), dy = GELU'(x) (nn.GELU(), exact erf form) by the device functions of every GEMM / fused-MLP epilogue
   (vv_gelu.h): form 0 the one-value forms, 1 the four-value interleaved forms (kernel tests). */
int vv_gelu_eval(vv_ctx* ctx, const float* x, float* y, float* dy, int64_t n, int form, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VAEVAR_H */
