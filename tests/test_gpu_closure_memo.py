"""GPU: the closure memo (vv_closure_memo / vv_closure_recall): an evaluation asked for again at a latent whose bits
have not changed is answered from the ring of recorded gradient evaluations, with the bits a fresh evaluation gives.

The networks are TINY and TINY_FLOW with synthetic weights on the problem of the tiny-network parity tests (nch = 4,
32 x 64, T = 2), on a private context so that the memo, the graph switch and the rebinds stay away from the shared
Context.get(0). The compare kernel is also run on its own (vv_bits_match) at lengths that are no multiple of its
256-thread workgroups or of its 128-bit groups, on more than one grid-stride pass and on unaligned vectors."""
import ctypes
import os

import pytest
import torch

from conftest import GOLD

pytestmark = pytest.mark.gpu

VV_E_ARG, VV_E_STATE = 1001, 1002
S = 3  # slots of the recall test; S + 1 latents are evaluated


class Env:
    pass


@pytest.fixture(scope="module")
def env():
    """One private context with the bound T = 2 problem, S + 1 latents and their fresh evaluations (memo off), which
    every test reads and none changes."""
    from vaevar import config as C
    from vaevar.engine import Context, DAProblem, LGUnet
    from vaevar.problem import make_problem
    from vaevar.synth import smooth_field

    e = Env()
    e.ctx = Context(0)
    e.p = make_problem(nch=4, Hs=32, Ws=64, T=2, seed=777, obs_frac=0.1)
    e.dec = LGUnet(C.TINY, 1, 1, ctx=e.ctx).load_synthetic()
    e.flow = LGUnet(C.TINY_FLOW, 1, 1, ctx=e.ctx).load_synthetic()
    e.prob = DAProblem(e.dec, e.p, flow=e.flow)
    e.zs = [torch.from_numpy(0.3 * smooth_field(300 + i, (1, 4, 32, 64), sigma=2.0)).cuda() for i in range(S + 1)]
    e.zs[2][0, 1, 2, 3] = 0.0  # a +0.0 for the signed-zero case
    e.ref = []
    for z in e.zs:
        g = torch.empty_like(z)
        jb, jo = e.prob.closure(z, g)
        e.ref.append((jb, jo, g))
    yield e
    assert e.ctx.close() == 0


def _flip(z, index):
    """z with the lowest mantissa bit of one element flipped"""
    f = z.clone()
    f.view(-1).view(torch.int32)[index] ^= 1
    return f


def _counters():
    from vaevar.engine import Context

    return Context.counter("closure_recall_hit"), Context.counter("closure_recall_miss")


def test_plain_evaluations_reproduce(env):
    """The precondition of the memo: evaluations at one z give the same J and gradient bits (the eager first one,
    the one that captures the graph, and the replays)."""
    jb0, jo0, g0 = env.ref[0]
    for _ in range(3):
        g = torch.empty_like(g0)
        jb, jo = env.prob.closure(env.zs[0], g)
        assert (jb, jo) == (jb0, jo0) and torch.equal(g, g0)


def test_recall(env):
    prob, zs = env.prob, env.zs
    g = torch.full_like(zs[0], 7.0)
    assert prob.recall(zs[0], g) is None  # off: a miss
    h0, m0 = _counters()
    prob.memo(S)
    try:
        assert prob.recall(zs[0], g) is None  # empty
        assert _counters() == (h0, m0 + 1)
        assert torch.equal(g, torch.full_like(g, 7.0))  # a miss writes nothing
        n0 = prob.n_evals
        for i, z in enumerate(zs):
            prob.closure_lazy(z, torch.empty_like(z))
            if i == 1:  # a J-only evaluation neither records nor evicts
                prob.closure(zs[0], None)
                prob.closure(_flip(zs[3], 0), None)
        assert prob.n_evals == n0 + len(zs) + 2
        r0 = prob.n_recalled
        for i in range(1, S + 1):
            g = torch.empty_like(zs[i])
            lazy = prob.recall(zs[i].clone(), g)  # the content counts, not the pointer
            assert lazy is not None, i
            jb, jo, gr = env.ref[i]
            assert lazy.dev.cpu().tolist() == [jb, jo]
            assert float(lazy) == prob.loss_f32(jb, jo)
            assert torch.equal(g, gr)
        assert prob.n_recalled == r0 + S and prob.n_evals == n0 + len(zs) + 2 + S
        assert prob.recall(zs[0], g) is None  # evicted by the S + 1st recording
        n = zs[3].numel()
        assert prob.recall(_flip(zs[3], 0), g) is None
        assert prob.recall(_flip(zs[3], n - 1), g) is None
        neg = zs[2].clone()
        neg[0, 1, 2, 3] = -0.0
        assert neg[0, 1, 2, 3] == zs[2][0, 1, 2, 3]  # equal as numbers, not as bits
        assert prob.recall(neg, g) is None
        assert prob.recall(zs[2], g) is not None
        h1, m1 = _counters()
        assert (h1 - h0, m1 - m0) == (S + 1, 5)
        # the synchronising closure looks up by itself: a hit gives the recorded bits and launches nothing
        launches = env.ctx.closure_graph_state(1)["launches"]
        g = torch.empty_like(zs[1])
        assert prob.closure(zs[1], g) == env.ref[1][:2] and torch.equal(g, env.ref[1][2])
        assert env.ctx.closure_graph_state(1)["launches"] == launches
        assert _counters() == (h1 + 1, m1)
        prob.memo(S)  # calling it again empties the ring
        assert prob.recall(zs[2], g) is None
    finally:
        prob.memo(0)
    assert prob.recall(zs[2], g) is None


def test_memo_arguments(env):
    from vaevar import _lib
    from vaevar.engine import Context

    lib, h = _lib.lib, env.ctx.h
    assert lib.vv_closure_memo(None, 1) == VV_E_ARG
    assert lib.vv_closure_memo(h, -1) == VV_E_ARG and lib.vv_closure_memo(h, 17) == VV_E_ARG
    hit = ctypes.c_int(5)
    assert lib.vv_closure_recall(h, None, None, None, None, ctypes.byref(hit)) == VV_E_ARG
    fresh = Context(0)  # no bound problem
    try:
        assert lib.vv_closure_memo(fresh.h, 2) == VV_E_STATE
    finally:
        assert fresh.close() == 0
    assert lib.vv_closure_memo(h, 16) == 0 and lib.vv_closure_memo(h, 0) == 0


INVALIDATORS = ["bind_problem", "set_obs_operator", "set_tuning", "set_gemm_math", "set_closure_graph", "load_weights",
                "model_destroy", "model_destroy_bound", "sc4dvar_bind", "memo_off", "memo_again"]


@pytest.mark.parametrize("call", INVALIDATORS)
def test_invalidation(env, call, monkeypatch):
    """After a recorded evaluation, each call after which an old result need not hold turns the next recall of the
    same z into a miss."""
    from vaevar import _lib, config as C
    from vaevar.engine import Context, DAProblem, LGUnet

    prob, z = env.prob, env.zs[1]
    g = torch.empty_like(z)
    prob.memo(2)
    try:
        prob.closure_lazy(z, g)
        assert prob.recall(z, g) is not None
        if call == "bind_problem":
            prob = env.prob = DAProblem(env.dec, env.p, flow=env.flow)
        elif call == "set_obs_operator":
            _lib.check(_lib.lib.vv_set_obs_operator(env.ctx.h, 0, 0, None))  # the identity operator, as it was
        elif call == "set_tuning":
            env.ctx.set_tuning("host_wait", env.ctx.get_tuning("host_wait"))  # any key, even at its own value
        elif call == "set_gemm_math":
            env.ctx.gemm_math = env.ctx.gemm_math
        elif call == "set_closure_graph":
            env.ctx.set_closure_graph(True)
        elif call == "load_weights":
            env.flow.load_synthetic()
        elif call == "model_destroy":
            LGUnet(C.TINY, 1, 1, ctx=env.ctx).__del__()  # a network the problem does not use
        elif call == "model_destroy_bound":
            env.flow.__del__()  # unbinds the problem: the memo goes with it
            hit = ctypes.c_int()
            assert _lib.lib.vv_closure_recall(env.ctx.h, z.data_ptr(), g.data_ptr(), None, None,
                                              ctypes.byref(hit)) == VV_E_STATE
            env.flow = LGUnet(C.TINY_FLOW, 1, 1, ctx=env.ctx).load_synthetic()
            prob = env.prob = DAProblem(env.dec, env.p, flow=env.flow)
        elif call == "sc4dvar_bind":
            from vaevar.problem import make_problem
            from vaevar.sc4dvar import BMatrix, Sc4dvarProblem

            # a sc4dvar problem without a flow model binds to the device's shared context: make it this one
            monkeypatch.setitem(Context._by_dev, 0, env.ctx)
            Sc4dvarProblem(BMatrix.from_npz(os.path.join(GOLD, "bq_info_lr.npz")),
                           make_problem(nch=69, Hs=128, Ws=256, T=1, seed=21))
        elif call == "memo_off":
            prob.memo(0)
        elif call == "memo_again":
            prob.memo(2)
        h0, _ = _counters()
        assert prob.recall(z, g) is None
        assert _counters()[0] == h0
        # and the problem still evaluates to the same bits
        jb, jo = prob.closure(z, g)
        assert (jb, jo) == env.ref[1][:2] and torch.equal(g, env.ref[1][2])
    finally:
        env.prob.memo(0)


def _graph_launches(ctx):
    return ctx.closure_graph_state(1)["launches"]


@pytest.mark.parametrize("mode", ["free", "replay"])
def test_one_step_da_memo_on_vs_off(env, mode, monkeypatch):
    """one_step_da with the memo (its default) against VAEVAR_CLOSURE_MEMO=0: the same latent, analysis, counts and J
    per pass; every step after the first recalled its first evaluation (nit - 1 hits, no miss: with max_eval + 1
    slots the accepted point cannot have been evicted), and exactly that many graph launches fewer."""
    from vaevar.da import one_step_da

    nit, max_iter = 4, 3
    replay = [(1e-3, 1)] * (nit * max_iter) if mode == "replay" else None
    prob = env.prob
    g = torch.empty_like(env.zs[0])
    for _ in range(2):  # both kinds of the closure replay from their graphs from here on
        prob.closure(env.zs[0], g)
        prob.closure(env.zs[0], None)
    runs = {}
    for memo in ("0", "1"):
        monkeypatch.setenv("VAEVAR_CLOSURE_MEMO", memo)
        l0, (h0, m0) = _graph_launches(env.ctx), _counters()
        res = one_step_da(prob, nit=nit, max_iter=max_iter, log_terms=True, replay=replay)
        h1, m1 = _counters()
        runs[memo] = (res, _graph_launches(env.ctx) - l0, h1 - h0, m1 - m0)
    (off, l_off, h_off, m_off), (on, l_on, h_on, m_on) = runs["0"], runs["1"]
    assert off["n_recalled"] == 0 and (h_off, m_off) == (0, 0)
    assert on["n_recalled"] == nit - 1 and (h_on, m_on) == (nit - 1, 0)
    assert l_off - l_on == on["n_recalled"]
    assert torch.equal(on["z"], off["z"]) and torch.equal(on["xa"], off["xa"])
    assert (on["n_eval"], on["n_iter"], on["n_discarded"]) == (off["n_eval"], off["n_iter"], off["n_discarded"])
    assert on["J"] == off["J"] and len(on["J"]) == nit + 1
    assert on["n_eval"] > nit  # the steps did evaluate beyond their first point
    assert prob.recall(on["z"], g) is None  # one_step_da turned the memo off again


def test_torch_lbfgs_dropin_with_memo(env):
    """torch.optim.LBFGS over engine.loss, the drop-in of INTEGRATION.md: three steps with prob.memo(13) on give the
    final z of three steps with it off, and the first evaluation of steps two and three is a hit."""
    from vaevar.engine import loss

    prob = env.prob
    out = {}
    for memo in (False, True):
        z = torch.zeros(1, 4, 32, 64, device="cuda", requires_grad=True)
        lb = torch.optim.LBFGS([z], history_size=10, max_iter=10, line_search_fn="strong_wolfe")

        def closure():
            lb.zero_grad()
            obj = loss(prob, z)
            obj.backward()
            return obj

        h0, _ = _counters()
        if memo:
            prob.memo(13)  # max_eval + 1 = 10 * 5 // 4 + 1
        try:
            for _ in range(3):
                lb.step(closure)
        finally:
            prob.memo(0)
        out[memo] = (z.detach().clone(), _counters()[0] - h0, lb.state[z]["func_evals"])
    assert torch.equal(out[True][0], out[False][0])
    assert out[True][2] == out[False][2]
    assert (out[False][1], out[True][1]) == (0, 2)


# ---------------------------------------------------------------------------------------------------------------
# the compare kernel on its own
LENGTHS = [1, 3, 4, 5, 255, 256, 257, 1023, 8192, 8195, 2 * (1 << 20) + 3]


def _bits_match(ctx, z, cands, n=None):
    from vaevar import _lib

    ptrs = (ctypes.c_void_p * len(cands))(*[c.data_ptr() for c in cands])
    m = ctypes.c_uint()
    _lib.check(_lib.lib.vv_bits_match(ctx.h, z.data_ptr(), ptrs, len(cands), z.numel() if n is None else n,
                                      ctypes.byref(m), None), "bits_match")
    return m.value


@pytest.mark.parametrize("n", LENGTHS)
def test_bits_match_lengths(env, n):
    """Bit i of the match word is set iff candidate i equals z in every 32-bit word: a difference in the first, the
    last, a middle and (n not a multiple of 4) a tail word is seen, at every length and candidate count."""
    gen = torch.Generator(device="cuda").manual_seed(n)
    z = torch.randn(n, device="cuda", generator=gen)
    places = sorted({0, n - 1, n // 2, max(n - 2, 0), (n // 4) * 4 - 1 if n >= 4 else 0})
    cands, want = [], 0
    for i in range(16):
        c = z.clone()
        if i % 3 != 1:  # candidates 1, 4, 7, ... stay equal
            c.view(torch.int32)[places[i % len(places)]] ^= 1 << (i % 31)
        cands.append(c)
    for count in (1, 3, 16):
        want = sum(1 << i for i in range(count) if torch.equal(cands[i].view(torch.int32), z.view(torch.int32)))
        assert _bits_match(env.ctx, z, cands[:count]) == want, (n, count)
    assert _bits_match(env.ctx, z, [cands[1], z]) == 3


def test_bits_match_words_not_numbers(env):
    """-0.0 is not +0.0, a NaN equals itself (and no other NaN); unaligned vectors are compared word by word."""
    z = torch.randn(1031, device="cuda")
    z[5], z[1030] = 0.0, float("nan")
    neg = z.clone()
    neg[5] = -0.0
    nan2 = z.clone()
    nan2.view(torch.int32)[1030] ^= 1  # another NaN payload
    assert torch.isnan(nan2[1030])
    assert _bits_match(env.ctx, z, [z.clone(), neg, nan2]) == 1
    buf = torch.randn(4 * 300 + 8, device="cuda")
    for off in (1, 2, 3):  # 4-byte aligned only
        a = buf[off:off + 1000]
        b = a.clone()
        c = a.clone()
        c[999] = c[999] + 1.0
        assert _bits_match(env.ctx, a, [b, c, a]) == 0b101
    assert _bits_match(env.ctx, z, [neg, nan2], n=0) == 3  # nothing to differ in
