"""Model and context lifecycle on the GPU: vv_model_destroy followed by the context-wide calls that walk the model
list (vv_set_gemm_math over a freed model once crashed), the documented statuses of calls on a dead model or an
unbound problem, re-creation and re-binding, and vv_ctx_destroy through Context.close().

Everything runs on a context of its own: destroying a model drops the context's captured closure graphs, and the
shared Context.get(0) of the other tests must not pay for that. The networks are TINY and TINY_FLOW with synthetic
weights on the problem of test_closure_edge_cases (nch = 4, 32 x 64, T = 2)."""
import ctypes

import pytest
import torch

from conftest import check, check_bitwise

pytestmark = pytest.mark.gpu

VV_E_ARG, VV_E_STATE = 1001, 1002


def test_model_destroy_then_context_calls():
    from vaevar import config as C
    from vaevar._lib import lib
    from vaevar.engine import Context, DAProblem, LGUnet, _ptr
    from vaevar.problem import make_problem
    from vaevar.synth import smooth_field

    ctx = Context(0)
    assert ctx is not Context.get(0)
    try:
        h = ctx.h
        p = make_problem(nch=4, Hs=32, Ws=64, T=2, seed=31, obs_frac=0.2)
        z = torch.from_numpy(0.3 * smooth_field(32, (1, 4, 32, 64), sigma=2.0)).cuda()

        def closure(prob, tag, times=2):
            """(J_b, J_o, g) of the last of `times` evaluations (the second one replays the captured graph), after
            checking that they agree bit for bit and that no capture failed."""
            outs = []
            for _ in range(times):
                g = torch.full_like(z, float("nan"))
                jb, jo = prob.closure(z, g)
                outs.append((jb, jo, g))
            for jb, jo, g in outs[1:]:
                check_bitwise(f"{tag}: repeated closure J", [jb, jo], list(outs[0][:2]))
                check_bitwise(f"{tag}: repeated closure g", g, outs[0][2])
            st = ctx.closure_graph_state(1)
            check(f"{tag}: closure graph capture failed", int(st["eager_only"]), 0, "==")
            check(f"{tag}: closure graph instantiated", int(st["instantiated"]), 1, "==")
            assert st["enabled"] and st["launches"] >= 1, st
            return outs[-1]

        def same(tag, got, want):
            check_bitwise(f"{tag}: J_b, J_o", list(got[:2]), list(want[:2]))
            check_bitwise(f"{tag}: dJ/dz", got[2], want[2])

        # 1. three networks, one of them unrelated to the problem
        dec = LGUnet(C.TINY, 1, 1, ctx=ctx).load_synthetic()
        flow = LGUnet(C.TINY_FLOW, 1, 1, ctx=ctx).load_synthetic()
        other = LGUnet(C.TINY, 1, 1, ctx=ctx).load_synthetic()
        assert dec.ctx is ctx and len({dec.id, flow.id, other.id}) == 3
        prob = DAProblem(dec, p, flow=flow)
        assert prob.ctx is ctx
        first = closure(prob, "step 1")
        assert torch.isfinite(first[2]).all() and first[0] > 0 and first[1] > 0

        # 2. destroy the unrelated network: the bound problem stays, its graphs are captured again
        check("destroy unrelated model", lib.vv_model_destroy(h, other.id), 0, "==")
        dead_other, other.id = other.id, None
        same("after destroying an unrelated model", closure(prob, "step 2"), first)

        # 3. the context-wide calls that walk the model list, over the freed entry
        math = ctx.gemm_math
        alt = "f32" if math != "f32" else "split16"
        for name in (math, alt, math):
            check(f"vv_set_gemm_math({name}) over a freed model", lib.vv_set_gemm_math(h, Context.GEMM_MATH[name]), 0,
                  "==")
        assert ctx.gemm_math == math
        knob = ctx.get_tuning("h3_mink")
        check("vv_set_tuning to its own value", lib.vv_set_tuning(h, b"h3_mink", knob), 0, "==")
        same("after the context-wide calls", closure(prob, "step 3"), first)

        # 4. destroy the bound flow network: the problem is unbound, the id is dead
        check("destroy bound flow model", lib.vv_model_destroy(h, flow.id), 0, "==")
        dead_flow, flow.id = flow.id, None
        g = torch.empty_like(z)
        jb, jo = ctypes.c_double(), ctypes.c_double()
        jbp, jop = ctypes.byref(jb), ctypes.byref(jo)
        check("vv_closure on the unbound problem", lib.vv_closure(h, _ptr(z), _ptr(g), jbp, jop, None), VV_E_STATE,
              "==")
        xp = ctypes.c_void_p()
        check("vv_state_ptr on the unbound problem", lib.vv_state_ptr(h, ctypes.byref(xp)), VV_E_STATE, "==")
        xin = torch.zeros(1, flow.in_ch, flow.H, flow.W, device="cuda")
        xout = torch.zeros(1, flow.out_ch, flow.H, flow.W, device="cuda")
        nbytes = ctypes.c_int64()
        for dead in (dead_flow, dead_other):
            check(f"vv_model_forward on dead id {dead}",
                  lib.vv_model_forward(h, dead, 0, _ptr(xin), _ptr(xout), 0, None), VV_E_ARG, "==")
            check(f"vv_model_workspace_bytes on dead id {dead}",
                  lib.vv_model_workspace_bytes(h, dead, ctypes.byref(nbytes)), VV_E_ARG, "==")
            check(f"second vv_model_destroy of id {dead}", lib.vv_model_destroy(h, dead), VV_E_ARG, "==")
        check("vv_bind_problem with the dead flow id",
              lib.vv_bind_problem(h, dec.id, dead_flow, prob.T, prob.C, prob.Hs, prob.Ws, _ptr(prob.xb), _ptr(prob.yo),
                                  _ptr(prob.H), _ptr(prob.R), _ptr(prob.mean), _ptr(prob.std), _ptr(prob.std_tr), 1.0),
              VV_E_ARG, "==")
        check("vv_closure after the refused bind", lib.vv_closure(h, _ptr(z), _ptr(g), jbp, jop, None), VV_E_STATE,
              "==")
        check("vv_set_gemm_math over two freed models", lib.vv_set_gemm_math(h, Context.GEMM_MATH[math]), 0, "==")

        # 5. a new flow network with the same weights, bound again
        flow2 = LGUnet(C.TINY_FLOW, 1, 1, ctx=ctx).load_synthetic()
        assert flow2.id not in (dead_flow, dead_other, dec.id)
        prob2 = DAProblem(dec, p, flow=flow2)
        same("after re-creating the flow model and re-binding", closure(prob2, "step 5"), first)
    finally:
        # 6. the context goes, once
        rc = ctx.close()
    check("Context.close()", rc, 0, "==")
    assert not ctx.h
    check("second Context.close() is a no-op", ctx.close(), 0, "==")
    # the shared context is untouched by all of the above
    shared = Context.get(0)
    assert shared is not ctx and shared.h
    a = torch.ones(257, device="cuda")
    check("shared context after the other one closed: dot", shared.dot(a, a), 257.0, "==")
