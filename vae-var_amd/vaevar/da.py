"""The vae4dvar analysis step on the HIP engine — mirror of cyclic_4dvar.one_step_DA(..., 'vae4dvar')
(da_4dvar.py:1179-1306). The WRMSE/Bias logging of :1256-1269 runs on the device (vaevar.metrics) when a truth
field and a Metrics object are given.

  z = zeros(1,32,128,256)                                  (:1238)
  LBFGS(history_size=10, max_iter=10, strong_wolfe)        (:1240)
  for kk in range(Nit+1): cal_loss(z) ; lbfgs.step(closure) while kk < Nit   (:1255-1299)
  xa = decoder_hr(z)[0]*stdTr*std + xb                     (:1301-1306)
"""
from __future__ import annotations

import os
import time

import torch

from .engine import DAProblem
from .lbfgs import LBFGS, Adam


def one_step_da(prob: DAProblem, nit: int, history_size: int = 10, max_iter: int = 10, optimizer: str = "lbfgs",
                lr: float | None = None, log_terms: bool = True, log=None, gt=None, metrics=None, replay=None,
                batch_scalars: bool = True, mask_eval=None, H_old=None, obs_stats: bool = False):
    """Returns dict(xa, z, J=[(J_b, J_o) per outer pass], n_eval, n_iter, n_discarded (speculative evaluations the
    reference would not have made, not in n_eval but in seconds), n_recalled (evaluations of n_eval answered by the
    engine's closure memo and not run, below; VAEVAR_CLOSURE_MEMO=0 keeps it off), seconds); with gt (T,C,Hs,Ws) and a
    vaevar.metrics.Metrics also metrics=[(wrmse[C], bias[C]) per outer pass] of xhat against gt[0] — the
    reference's bg_* (pass 0) and ana_* (pass Nit) entries of metrics_list (:1285-1291).

    --use_eval (:934-937, :1285-1286): with mask_eval (Hs,Ws) and H_old (T,C_obs,Hs,Ws), the station mask before
    the split — both from vaevar.metrics.held_out, whose reduced mask the problem must have been bound with — the
    last pass's xhat is verified against the held-out observations yo[0] * mask_eval * H_old[0] on the device
    (Metrics.obs_error) and returned as error_obs (C_obs,) numpy fp32. Needs `metrics`; single analysis only.

    obs_stats=True adds obs_stats, the (T, C_obs, 10) float64 numpy table of fields.obs_stats (the O-B / O-A departure
    moments per time level and observation channel, calib.DepartureStats) against the problem's own yo, H, R and
    operator: the background window is the trajectory of the J-only evaluation at z = 0, the analysis window that of a
    J-only evaluation at the final z. With log_terms those evaluations run anyway; with log_terms=False this costs
    two extra J-only evaluations (not counted in n_eval). With mask_eval / H_old also obs_stats_heldout, the same
    table over H_old * mask_eval: the observations the analysis never saw. Nothing else of the result changes.
    Single analysis only."""
    if mask_eval is not None:
        _check_eval(prob.B, metrics, H_old)
    if obs_stats and prob.B != 1:
        raise ValueError("obs_stats: the departure statistics take a single analysis (B = 1)")
    dev = prob.xb.device
    z = torch.zeros(prob.latent_shape, device=dev, dtype=torch.float32)
    ctx = prob.ctx
    if optimizer == "lbfgs":
        opt = LBFGS(ctx, z, lr=1 if lr is None else lr, history_size=history_size, max_iter=max_iter,
                    line_search_fn="strong_wolfe")
        opt.replay = list(replay) if replay is not None else None  # fixed-step replay of a reference run
        opt.batch_scalars = batch_scalars  # False: one synchronising call per scalar (vaevar/lbfgs.py)
    elif optimizer == "adam":
        opt = Adam(ctx, z, lr=1e-3 if lr is None else lr)
    else:
        raise ValueError(optimizer)

    def closure(zz, g):
        if optimizer == "lbfgs" and batch_scalars:  # queued: the loss comes with the mirror's next scalars
            return prob.closure_lazy(zz, g)
        jb, jo = prob.closure(zz, g)
        return prob.loss_f32(jb, jo)

    js, ms, err = [], [], None
    wins = {}  # obs_stats: the window at z = 0 (pass 0) and at the final z (pass nit)
    n0 = prob.n_evals
    d0 = prob.n_discarded
    r0 = getattr(prob, "n_recalled", 0)
    t0 = time.time()
    # The closure memo for the span of this analysis, in which nothing edits the bound buffers: the first evaluation of
    # every step after the first is at the latent the previous line search accepted, and max_eval + 1 slots hold every
    # point one step can evaluate plus one discarded speculative evaluation, so that point is still in the ring.
    recall = None
    if (optimizer == "lbfgs" and prob.B == 1 and hasattr(prob, "recall")
            and os.environ.get("VAEVAR_CLOSURE_MEMO", "1") != "0"):
        prob.memo(min(opt.max_eval + 1, 16))
        recall = prob.recall
    for kk in range(nit + 1):
        if log_terms:
            jb, jo = prob.closure(z, None)  # cal_loss (:1210-1236): no gradient
            js.append((jb, jo))
            if obs_stats and kk in (0, nit):
                wins[kk] = prob.trajectory()
            verify = mask_eval is not None and kk == nit
            if (gt is not None and metrics is not None) or verify:
                xhat = prob.trajectory()[0]  # decoder_hr(z)*stdTr*std + xb of this pass (:1256-1258)
            if gt is not None and metrics is not None:
                w, b = metrics.wrmse_bias(xhat, gt[0])
                ms.append((w.cpu().numpy(), b.cpu().numpy()))
            if verify:  # :1264-1286
                err = metrics.obs_error(xhat, prob.yo[0], H_old[0], mask_eval, prob.interp)
            if log is not None:
                log(kk, jb, jo)
        elif obs_stats and kk in (0, nit):  # a J-only evaluation always runs: the state buffers are this z's
            prob.closure(z, None)
            wins[kk] = prob.trajectory()
        if kk < nit:
            opt.step(closure, recall) if recall is not None else opt.step(closure)
    if recall is not None:
        prob.memo(0)
    xa = prob.analysis(z)
    if mask_eval is not None and err is None:  # no per-pass logging: the analysis is the last pass's xhat
        err = metrics.obs_error(xa, prob.yo[0], H_old[0], mask_eval, prob.interp)
    tabs = _departure_tables(prob, wins[0], wins[nit], mask_eval, H_old) if obs_stats else {}
    torch.cuda.synchronize()
    n_log = (nit + 1) if log_terms else len(wins)  # J-only evaluations: the passes logged, or obs_stats' own
    n_iter = opt.state["n_iter"] if optimizer == "lbfgs" else opt.t
    res = {"xa": xa, "z": z, "J": js, "n_eval": prob.n_evals - n0 - n_log, "n_iter": n_iter,
           "n_discarded": prob.n_discarded - d0, "n_recalled": getattr(prob, "n_recalled", 0) - r0,
           "seconds": time.time() - t0, "metrics": ms}
    if err is not None:
        res["error_obs"] = err.cpu().numpy()
    res.update({k: v.cpu().numpy() for k, v in tabs.items()})
    return res


def _departure_tables(prob, xb_win, xa_win, mask_eval=None, H_old=None) -> dict:
    """obs_stats (and, with the held-out split, obs_stats_heldout) of a bound problem's observations against a
    background and an analysis window (T, C, Hs, Ws); xa_win may be None. Device tensors."""
    from .fields import obs_stats as table

    out = {"obs_stats": table(prob.ctx, xb_win, xa_win, prob.yo, prob.H, prob.R, prob.interp)}
    if mask_eval is not None:
        held = (H_old.to(prob.yo.device, torch.float32) * mask_eval.to(prob.yo.device, torch.float32)).contiguous()
        out["obs_stats_heldout"] = table(prob.ctx, xb_win, xa_win, prob.yo, held, prob.R, prob.interp)
    return out


def _check_eval(B: int, metrics, H_old):
    if B != 1:
        raise ValueError("mask_eval: the held-out verification takes a single analysis (B = 1)")
    if metrics is None or H_old is None:
        raise ValueError("mask_eval needs metrics (vaevar.metrics.Metrics) and H_old, the station mask before "
                         "held_out() reduced it")


def one_step_da_batch(prob: DAProblem, nit: int, history_size: int = 10, max_iter: int = 10):
    """B independent one_step_DA analyses (da_4dvar.py:1179-1306) in lockstep over one batched closure: each
    analysis b runs its own L-BFGS mirror on its latent z[b]; whenever every unfinished analysis has requested an
    evaluation, ONE vv_closure evaluates all B latents (the GEMMs of the decoder / flow run on B x 2048 rows) and
    each optimiser resumes with its own J and gradient. Analyses that have finished keep their final latent in
    the batch (their results are not used). Returns dict(xa (B,C,Hs,Ws), z, n_eval per analysis, n_iter per
    analysis, batched_evals, seconds)."""
    dev = prob.xb.device
    B = prob.B
    Z = torch.zeros(prob.latent_shape, device=dev, dtype=torch.float32)
    G = torch.empty_like(Z)
    ctx = prob.ctx
    opts = [LBFGS(ctx, Z[b], lr=1, history_size=history_size, max_iter=max_iter, line_search_fn="strong_wolfe")
            for b in range(B)]

    def run(opt):
        for _ in range(nit):
            yield from opt.step_gen()

    t0 = time.time()
    gens = [run(o) for o in opts]
    pending = [None] * B
    active = [True] * B
    n_eval = [0] * B
    for b in range(B):
        try:
            pending[b] = next(gens[b])
        except StopIteration:
            active[b] = False
    batched = 0
    while any(active):
        jb, jo = prob.closure_batch(Z, G)
        batched += 1
        for b in range(B):
            if not active[b]:
                continue
            zb, gb = pending[b]
            ctx.copy(gb, G[b])
            n_eval[b] += 1
            try:
                pending[b] = gens[b].send(prob.loss_f32(jb[b], jo[b]))
            except StopIteration:
                active[b] = False
    xa = prob.analysis(Z)
    torch.cuda.synchronize()
    return {"xa": xa, "z": Z, "n_eval": n_eval, "n_iter": [o.state["n_iter"] for o in opts],
            "batched_evals": batched, "seconds": time.time() - t0}

