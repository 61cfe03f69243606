"""CPU: the L-BFGS mirror's side of the closure memo. step_gen marks the first request of every step after the first
(the latent the previous line search accepted, evaluated there already); step(closure, recall) tries `recall` for
exactly those. With a stand-in memo keyed by the latent's bytes the iterates, losses and func_evals are those of the
plain run and the closure runs nit - 1 times fewer; a driver without a recall changes nothing."""
import torch

from test_host_logic import CpuPrims, objective


class StandIn:
    """A problem stand-in: closure(z, g) evaluates and records (the newest `slots` evaluations), like the engine
    with the memo on."""

    def __init__(self, slots):
        self.slots, self.ring, self.calls, self.hits, self.misses = slots, [], 0, 0, 0

    def closure(self, z, g):
        zz = z.clone().requires_grad_(True)
        f = objective(zz)
        f.backward()
        g.copy_(zz.grad)
        self.calls += 1
        self.ring = (self.ring + [(z.numpy().tobytes(), float(f.detach()), zz.grad.clone())])[-self.slots:]
        return float(f.detach())


class StandInRecall(StandIn):
    def recall(self, z, g):
        key = z.numpy().tobytes()
        for k, f, grad in reversed(self.ring):
            if k == key:
                g.copy_(grad)
                self.hits += 1
                return f
        self.misses += 1
        return None


def _run(standin, nit, max_iter=10):
    from vaevar.lbfgs import LBFGS

    z = torch.zeros(4096)
    mir = LBFGS(CpuPrims(), z, history_size=10, max_iter=max_iter, line_search_fn="strong_wolfe")
    recall = getattr(standin, "recall", None)  # as vaevar.da.one_step_da asks its problem
    losses, iterates = [], []
    for _ in range(nit):
        losses.append(mir.step(standin.closure, recall) if recall is not None else mir.step(standin.closure))
        iterates.append(z.clone())
    return losses, iterates, dict(mir.state)


def test_recall_serves_every_step_initial_evaluation():
    nit = 4
    plain, memo = StandIn(13), StandInRecall(13)  # max_eval + 1 = 10 * 5 // 4 + 1 slots
    l0, z0, s0 = _run(plain, nit)
    l1, z1, s1 = _run(memo, nit)
    assert l0 == l1 and all(torch.equal(a, b) for a, b in zip(z0, z1))
    assert s0["n_iter"] == s1["n_iter"] and s0["func_evals"] == s1["func_evals"]
    assert (memo.hits, memo.misses) == (nit - 1, 0)
    assert memo.calls == plain.calls - (nit - 1)
    assert s1["func_evals"] == memo.calls + memo.hits  # a recalled evaluation counts, as the reference counts it


def test_recall_miss_falls_back_to_the_closure():
    """A memo too small to still hold the accepted point misses; the step then evaluates as usual."""
    nit = 3
    plain, memo = StandIn(1), StandInRecall(1)

    def closure_no_record(z, g):  # records nothing: every recall misses
        ring = memo.ring
        out = StandIn.closure(memo, z, g)
        memo.ring = ring
        return out

    memo.closure = closure_no_record
    l0, z0, s0 = _run(plain, nit)
    l1, z1, s1 = _run(memo, nit)
    assert l0 == l1 and all(torch.equal(a, b) for a, b in zip(z0, z1))
    assert (memo.hits, memo.misses) == (0, nit - 1) and memo.calls == plain.calls
    assert s0["func_evals"] == s1["func_evals"]


def test_step_initial_marks_only_the_first_request_of_later_steps():
    """The request stays the (z, grad_out) pair; the mark is an attribute beside it."""
    from vaevar.lbfgs import LBFGS

    z = torch.zeros(4096)
    mir = LBFGS(CpuPrims(), z, history_size=10, max_iter=4, line_search_fn="strong_wolfe")
    plain = StandIn(1)
    assert mir.step_initial is False
    for step in range(3):
        gen = mir.step_gen()
        req = next(gen)
        first = True
        try:
            while True:
                assert isinstance(req, tuple) and len(req) == 2 and req[0] is z and req[1].shape == z.shape
                assert mir.step_initial is (first and step > 0)
                first = False
                req = gen.send(plain.closure(*req))
        except StopIteration:
            pass
        assert mir.step_initial is False
