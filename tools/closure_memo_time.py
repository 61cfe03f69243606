"""The closure memo on the benchmarked analysis (bench.py config N, default 3): what it saves and what it costs.

  python tools/closure_memo_time.py [--config 3] [--reps 2] [--evals 20]

One JSON line per measurement:
  analysis   one_step_da with VAEVAR_CLOSURE_MEMO=0 / 1, alternating: seconds, evaluations, recalled, the hit and miss
             counters, graph launches; z and xa of the two compared bit for bit
  record     queued gradient evaluations (vv_closure_async) at one latent, memo off against on (13 slots): ms per
             evaluation, the difference being the two latent-sized copies and the J copy of the recording
  lookup     vv_closure_recall hits with 13 valid slots: ms per call (compare launch, read-back, gradient copy)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "vae-var_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=3)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--evals", type=int, default=20)
    a = ap.parse_args()

    import torch

    import bench
    from vaevar.da import one_step_da
    from vaevar.engine import Context

    w = bench.GpuAnalyses(a.config, 0, 0, 1)
    prob, ctx = w.prob, w.ctx

    def counters():
        return Context.counter("closure_recall_hit"), Context.counter("closure_recall_miss")

    os.environ["VAEVAR_CLOSURE_MEMO"] = "1"
    one_step_da(prob, nit=w.nit, log_terms=False)  # warm-up: graph capture
    last = {}
    for rep in range(a.reps):
        for memo in ("0", "1"):
            os.environ["VAEVAR_CLOSURE_MEMO"] = memo
            (h0, m0), l0 = counters(), ctx.closure_graph_state(1)["launches"]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = one_step_da(prob, nit=w.nit, log_terms=False)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            h1, m1 = counters()
            last[memo] = res
            print(json.dumps({"what": "analysis", "config": a.config, "rep": rep, "memo": int(memo), "seconds": dt,
                              "iters": res["n_iter"], "evals": res["n_eval"], "n_recalled": res["n_recalled"],
                              "n_discarded": res["n_discarded"], "hits": h1 - h0, "misses": m1 - m0,
                              "graph_launches": ctx.closure_graph_state(1)["launches"] - l0,
                              "iters_per_s": res["n_iter"] / dt}), flush=True)
    print(json.dumps({"what": "same_bits", "z": bool(torch.equal(last["0"]["z"], last["1"]["z"])),
                      "xa": bool(torch.equal(last["0"]["xa"], last["1"]["xa"]))}), flush=True)

    z = last["1"]["z"].clone()
    g = torch.empty_like(z)
    per = {}
    for rep in range(a.reps):
        for slots in (0, 13):
            prob.memo(slots)
            prob.closure_lazy(z, g)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.evals):
                prob.closure_lazy(z, g)
            torch.cuda.synchronize()
            per[slots] = 1e3 * (time.perf_counter() - t0) / a.evals
        print(json.dumps({"what": "record", "rep": rep, "evals": a.evals, "ms_per_eval_memo_off": per[0],
                          "ms_per_eval_memo_on": per[13], "record_ms_per_eval": per[13] - per[0]}), flush=True)
    # 13 valid slots holding different latents, the queried one the newest
    prob.memo(13)
    for i in range(13):
        prob.closure_lazy(z * (1.0 + 0.01 * (12 - i)), g)
    torch.cuda.synchronize()
    n = 50
    t0 = time.perf_counter()
    for _ in range(n):
        assert prob.recall(z, g) is not None
    torch.cuda.synchronize()
    print(json.dumps({"what": "lookup", "valid_slots": 13, "calls": n,
                      "ms_per_recall_hit": 1e3 * (time.perf_counter() - t0) / n}), flush=True)
    prob.memo(0)


if __name__ == "__main__":
    main()
