"""The optimiser's vector arithmetic on the GPU against float64: vv_dot, vv_abssum, vv_absmax, vv_reduce_batch /
vv_reduce_enqueue, vv_axpy, vv_axpby, vv_scale, vv_copy, vv_lbfgs_two_loop and vv_adam. This is what runs between
two closures of the L-BFGS mirror and of Adam: every step length, convergence test and search direction.

Lengths come from the kernels' geometry: the reductions run 1024 blocks x 256 threads (262,144 threads: one element
each, +-1), the elementwise kernels at most 2048 blocks (524,288 threads, +1), k_twoloop_axpy_dot prefetches four
elements per thread (1,048,576 fills the four slots, +1 enters the grid-stride tail), 3 * 2^20 + 5 runs every loop
several times with a ragged end; 1, 3, 255, 256, 257 sit around one block.

Value families: "randn", and "wide" = randn * exp(U(-8, 8)) per element with alternating signs on b, whose dot cancels
to a small fraction of sum |a_i b_i|: the reduction bounds are absolute in that sum, not relative to the result.

Every tolerance is derived where it is used, none is tuned to the library's output. The CPU stand-in of
tests/test_host_logic.py (CpuPrims) is held to the same bounds as the device on the same inputs: that is what lets the
host-logic tests, which validate the mirror against torch.optim with CpuPrims, speak for the GPU path."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import check, check_bitwise, note
from test_host_logic import CpuPrims

pytestmark = pytest.mark.gpu

NMAX = 3 * (1 << 20) + 5
LENGTHS = [1, 3, 255, 256, 257, 262_143, 262_144, 262_145, 524_288, 524_289, 1_048_576, 1_048_577, NMAX]
FAMILIES = ("randn", "wide")
RED_BLOCKS = 1024  # grid of the reduction kernels (blocks of 256 threads, grid-stride)
f32 = np.float32
VV_E_ARG = 1001


def dev(t):
    return t.cuda()


@pytest.fixture(scope="module")
def ctx():
    from vaevar.engine import Context

    return Context.get(0)


@pytest.fixture(scope="module")
def vecs():
    """Per family: a, b (fp32, CPU and device, NMAX long; a test takes the prefix of its length) and the float64
    elementwise |a|, a * b (an fp32 product is exact in float64). Computed once, never written."""
    g = torch.Generator().manual_seed(20250917)
    out = {}
    for fam in FAMILIES:
        a, b = torch.randn(NMAX, generator=g), torch.randn(NMAX, generator=g)
        if fam == "wide":
            a = a * torch.exp(torch.rand(NMAX, generator=g) * 16 - 8)
            b = b.abs() * torch.exp(torch.rand(NMAX, generator=g) * 16 - 8)
            b[1::2] = -b[1::2]
        # the fp32 normal range with room for alpha = 1e4 and for the products
        assert float(a.abs().max()) < 1e6 and float(b.abs().max()) < 1e6
        assert float(a.abs().min()) > 1e-30 and float(b.abs().min()) > 1e-30
        out[fam] = {"a": a, "b": b, "da": dev(a), "db": dev(b), "abs_a": a.double().abs(),
                    "ab": a.double() * b.double()}
    return out


def _enqueue(ctx, reqs):
    out = dev(torch.full((len(reqs),), float("nan"), dtype=torch.float64))
    ctx.reduce_enqueue(reqs, out)
    return out.cpu().tolist()


# --------------------------------------------------------------------------------------------------------------------
# A1. reductions against float64
# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", LENGTHS)
def test_reductions_vs_fp64(ctx, vecs, n):
    """|dot - ref| <= 1e-14 * sum |a_i b_i| and |abssum - ref| <= 1e-14 * sum |a_i|, ref = the torch-CPU float64 sum
    of the exact products / absolute values.

    Derivation: the kernels add exact float64 terms (an fp32 product has 48 significant bits). The longest chain of
    additions at the largest length is 13 per thread, 6 lane steps and 3 waves in the block, then 4 + 6 + 3 in the
    final kernel: 35 roundings of 2^-53 relative to the running sum of absolute values = 3.9e-15. torch's pairwise
    float64 reference adds at most 2.4e-15. An fp32 accumulation sits at 1e-10 .. 1e-7 of the same sum.
    absmax is exact (== the fp32 a.abs().max()); vv_reduce_batch and vv_reduce_enqueue equal the single calls bit
    for bit for all three ops; CpuPrims meets the same bounds against the device."""
    cpu = CpuPrims()
    for fam in FAMILIES:
        v = vecs[fam]
        a, b, da, db = v["a"][:n], v["b"][:n], v["da"][:n], v["db"][:n]
        ref_dot, sum_ab = float(v["ab"][:n].sum()), float(v["ab"][:n].abs().sum())
        ref_abs = float(v["abs_a"][:n].sum())
        dot, abssum, absmax = ctx.dot(da, db), ctx.abssum(da), ctx.absmax(da)
        check(f"{fam} n={n} dot vs fp64 (abs, bound 1e-14 sum|ab|)", abs(dot - ref_dot), 1e-14 * sum_ab, "<=")
        check(f"{fam} n={n} abssum vs fp64 (abs, bound 1e-14 sum|a|)", abs(abssum - ref_abs), 1e-14 * ref_abs, "<=")
        check(f"{fam} n={n} absmax vs fp32 max", absmax, float(a.abs().max()), "==")
        check(f"{fam} n={n} dot vs CpuPrims", abs(dot - cpu.dot(a, b)), 1e-14 * sum_ab, "<=")
        check(f"{fam} n={n} abssum vs CpuPrims", abs(abssum - cpu.abssum(a)), 1e-14 * ref_abs, "<=")
        check(f"{fam} n={n} absmax vs CpuPrims", absmax, cpu.absmax(a), "==")
        reqs = [(0, da, db), (1, da, None), (2, da, None), (0, db, db), (1, db, None), (2, db, None)]
        want = [dot, abssum, absmax, ctx.dot(db, db), ctx.abssum(db), ctx.absmax(db)]
        check_bitwise(f"{fam} n={n} reduce_batch vs single calls", ctx.reduce_batch(reqs), want)
        check_bitwise(f"{fam} n={n} reduce_enqueue vs single calls", _enqueue(ctx, reqs), want)


# --------------------------------------------------------------------------------------------------------------------
# A2. non-finite values
# --------------------------------------------------------------------------------------------------------------------
def _last_block_first(n):
    """First index of the share of the last reduction block that has one (block k starts at 256 k)."""
    return (min((n + 255) // 256, RED_BLOCKS) - 1) * 256


def _all_entry_points(ctx, name, a, b):
    """(dot(a, b), abssum(a), absmax(a)) by the single calls, after checking that vv_reduce_batch and
    vv_reduce_enqueue return the same three values (NaN equal to NaN)."""
    da, db = dev(a), dev(b)
    single = [ctx.dot(da, db), ctx.abssum(da), ctx.absmax(da)]
    reqs = [(0, da, db), (1, da, None), (2, da, None)]
    check_bitwise(f"{name}: reduce_batch vs single calls", ctx.reduce_batch(reqs), single)
    check_bitwise(f"{name}: reduce_enqueue vs single calls", _enqueue(ctx, reqs), single)
    return single


@pytest.mark.parametrize("n", [257, 1_048_577])
def test_nonfinite_reductions(ctx, vecs, n):
    """A NaN anywhere makes absmax NaN through vv_absmax, vv_reduce_batch and vv_reduce_enqueue, as torch's
    a.abs().max() and CpuPrims.absmax do: the mirror's optimality test `|g|_max <= tolerance_grad` is then False and
    the optimiser goes on as torch.optim.LBFGS does, where a NaN-dropping maximum reports 0 and stops as converged.
    +-inf gives inf; dot and abssum follow IEEE 754 (the float64 torch-CPU sum is the reference). Positions: index
    0, n - 1, the first index of the last block's share, and every element."""
    base_a, base_b = vecs["randn"]["a"][:n], vecs["randn"]["b"][:n]
    nan, inf = float("nan"), float("inf")
    cases = [(f"NaN at {k}", {k: nan}) for k in sorted({0, n - 1, _last_block_first(n)})]
    cases += [("all NaN", None),
              (f"+inf at {_last_block_first(n)}", {_last_block_first(n): inf}),
              (f"-inf at {n - 1}", {n - 1: -inf}),
              ("+inf at 0 and -inf at n-1", {0: inf, n - 1: -inf})]
    for name, put in cases:
        a = base_a.clone()
        if put is None:
            a.fill_(nan)
        else:
            for k, val in put.items():
                a[k] = val
        b = base_b.abs()  # positive: an infinite product keeps the sign of its a_i
        dot, abssum, absmax = _all_entry_points(ctx, f"n={n} {name}", a, b)
        check_bitwise(f"n={n} {name}: absmax vs torch a.abs().max()", absmax, float(a.abs().max()))
        check_bitwise(f"n={n} {name}: absmax vs CpuPrims", absmax, CpuPrims().absmax(a))
        check_bitwise(f"n={n} {name}: abssum vs float64", abssum, float(a.double().abs().sum()))
        check_bitwise(f"n={n} {name}: dot vs float64", dot, float((a.double() * b.double()).sum()))
        if put is None or nan in put.values():
            assert np.isnan(absmax) and np.isnan(abssum) and np.isnan(dot), (name, absmax, abssum, dot)
        else:
            assert absmax == inf and abssum == inf, (name, absmax, abssum)
            assert np.isnan(dot) if len(put) == 2 else dot == next(iter(put.values())), (name, dot)


# --------------------------------------------------------------------------------------------------------------------
# A3. elementwise calls
# --------------------------------------------------------------------------------------------------------------------
ALPHAS = (0.3, -1e-3, 1e4)
U = 2.0 ** -24  # unit roundoff of fp32
SLACK = 1 + 2.0 ** -20  # second-order terms and the float64 reference's own rounding


def _max_ratio(out, r64, mag):
    """max_i |out_i - r64_i| / (U * mag_i * SLACK); an element with mag_i = 0 must be exact."""
    err = (out.double() - r64).abs()
    bound = U * mag * SLACK
    ratio = torch.where(bound > 0, err / bound, torch.where(err == 0, torch.zeros_like(err), err * float("inf")))
    return float(ratio.max())


@pytest.mark.parametrize("n", LENGTHS)
def test_axpy_axpby_vs_fp64(ctx, vecs, n):
    """axpy: |out - r64| <= 2^-24 (|r64| + |alpha x|) (1 + 2^-20) per element, r64 = y + alpha x in float64 with
    alpha = np.float32(alpha), the value the C ABI receives. An unfused multiply-add rounds alpha x (2^-24 |alpha x|)
    and the sum (2^-24 |y + fl(alpha x)| <= 2^-24 (|r64| + 2^-24 |alpha x|)); a fused one rounds once (2^-24 |r64|).
    Anything less accurate than one correctly rounded fp32 multiply and add fails. axpby: the same with
    |a x| + |b y| (either product may be the rounded one)."""
    for fam in FAMILIES:
        v = vecs[fam]
        x, y, dx, dy = v["a"][:n], v["b"][:n], v["da"][:n], v["db"][:n]
        x64, y64 = x.double(), y.double()
        for alpha in ALPHAS:
            al = float(f32(alpha))
            out = dy.clone()
            ctx.axpy(out, dx, alpha)
            r64 = y64 + al * x64
            check(f"{fam} n={n} axpy alpha={alpha}: max err / bound",
                  _max_ratio(out.cpu(), r64, r64.abs() + (al * x64).abs()), 1.0, "<=")
            be = float(f32(-0.7))
            out = dev(torch.full((n,), float("nan")))
            ctx.axpby(out, dx, alpha, dy, -0.7)
            r64 = al * x64 + be * y64
            check(f"{fam} n={n} axpby a={alpha} b=-0.7: max err / bound",
                  _max_ratio(out.cpu(), r64, r64.abs() + (al * x64).abs() + (be * y64).abs()), 1.0, "<=")


@pytest.mark.parametrize("n", LENGTHS)
def test_elementwise_bitwise_identities(ctx, vecs, n):
    """What the L-BFGS mirror relies on, bit for bit: axpby(out, x, a, None, 0) is the fp32 product x * a (s = t d and
    d = -g), axpby(y, g, 1, prev, -1) the fp32 difference g - prev, scale the fp32 product y * a; axpby may write over
    either input; copy moves bit patterns (NaN payloads, +-inf and -0.0 included)."""
    for fam in FAMILIES:
        v = vecs[fam]
        x, y, dx, dy = v["a"][:n], v["b"][:n], v["da"][:n], v["db"][:n]
        for alpha in ALPHAS:
            out = dev(torch.full((n,), float("nan")))
            ctx.axpby(out, dx, alpha, None, 0.0)
            check_bitwise(f"{fam} n={n} axpby(x, {alpha}, None, 0) vs fp32 x * a", out, x * float(f32(alpha)))
            out = dy.clone()
            ctx.scale(out, alpha)
            check_bitwise(f"{fam} n={n} scale({alpha}) vs fp32 y * a", out, y * float(f32(alpha)))
            plain = dev(torch.full((n,), float("nan")))
            ctx.axpby(plain, dx, alpha, dy, -0.7)
            ox = dx.clone()
            ctx.axpby(ox, ox, alpha, dy, -0.7)
            check_bitwise(f"{fam} n={n} axpby a={alpha} out aliasing x", ox, plain)
            oy = dy.clone()
            ctx.axpby(oy, dx, alpha, oy, -0.7)
            check_bitwise(f"{fam} n={n} axpby a={alpha} out aliasing y", oy, plain)
        out = dev(torch.full((n,), float("nan")))
        ctx.axpby(out, dx, 1.0, dy, -1.0)
        check_bitwise(f"{fam} n={n} axpby(x, 1, y, -1) vs fp32 x - y", out, x - y)
    bits = vecs["randn"]["a"][:n].clone().view(torch.int32)
    special = [0x7FC00000, 0x7F800001, -1, 0x7F800000, -0x00800000, -0x80000000, 1, 0]  # NaNs, +-inf, -0.0, denormal
    for k, pattern in enumerate(special[:n]):
        bits[k * max(n // len(special), 1)] = pattern
    src = dev(bits.view(torch.float32))
    dst = dev(torch.zeros(n))
    ctx.copy(dst, src)
    check_bitwise(f"n={n} copy as int32", dst.view(torch.int32), bits)


def _raw_args(*tensors):
    return [ctypes.c_void_p(t.data_ptr()) for t in tensors]


def test_zero_length_is_noop(ctx):
    """n = 0 with valid pointers: status 0, no operand touched, reductions of 0 (a grid of 0 blocks would be an
    invalid-configuration launch error)."""
    from vaevar._lib import lib

    x0, y0 = torch.tensor([1.5, -2.0, 3.25, 4.0]), torch.tensor([-7.0, 8.5, 9.0, -10.25])
    x, y, z = dev(x0), dev(y0), dev(y0)
    px, py, pz = _raw_args(x, y, z)
    h = ctx.h
    check("vv_axpy n=0 status", lib.vv_axpy(h, py, px, 2.0, 0, None), 0, "==")
    check("vv_axpby n=0 status", lib.vv_axpby(h, pz, px, 2.0, py, 3.0, 0, None), 0, "==")
    check("vv_axpby (y = NULL) n=0 status", lib.vv_axpby(h, pz, px, 2.0, None, 0.0, 0, None), 0, "==")
    check("vv_scale n=0 status", lib.vv_scale(h, py, 2.0, 0, None), 0, "==")
    check("vv_copy n=0 status", lib.vv_copy(h, pz, px, 0, None), 0, "==")
    d, s, m = ctypes.c_double(123.0), ctypes.c_double(123.0), ctypes.c_float(123.0)
    check("vv_dot n=0 status", lib.vv_dot(h, px, py, 0, ctypes.byref(d), None), 0, "==")
    check("vv_abssum n=0 status", lib.vv_abssum(h, px, 0, ctypes.byref(s), None), 0, "==")
    check("vv_absmax n=0 status", lib.vv_absmax(h, px, 0, ctypes.byref(m), None), 0, "==")
    check("vv_dot n=0", d.value, 0.0, "==")
    check("vv_abssum n=0", s.value, 0.0, "==")
    check("vv_absmax n=0", m.value, 0.0, "==")
    ro = (ctypes.c_float * 1)(1.0)
    S, Y = (ctypes.c_void_p * 1)(px.value), (ctypes.c_void_p * 1)(pz.value)
    check("vv_lbfgs_two_loop n=0 status", lib.vv_lbfgs_two_loop(h, py, S, Y, ro, 1, 0.5, 0, None), 0, "==")
    torch.cuda.synchronize()
    check_bitwise("n=0: x untouched", x, x0)
    check_bitwise("n=0: y untouched", y, y0)
    check_bitwise("n=0: out untouched", z, y0)
    # all three ops as requests of vv_reduce_batch / vv_reduce_enqueue
    ops = (ctypes.c_int * 3)(0, 1, 2)
    A, B = (ctypes.c_void_p * 3)(px.value, px.value, px.value), (ctypes.c_void_p * 3)(py.value, None, None)
    out = (ctypes.c_double * 3)(123.0, 123.0, 123.0)
    check("vv_reduce_batch n=0 status", lib.vv_reduce_batch(h, 3, ops, A, B, 0, None, 0, out, None), 0, "==")
    check_bitwise("vv_reduce_batch n=0", list(out), [0.0] * 3)
    dout = dev(torch.full((3,), 123.0, dtype=torch.float64))
    check("vv_reduce_enqueue n=0 status",
          lib.vv_reduce_enqueue(h, 3, ops, A, B, 0, ctypes.c_void_p(dout.data_ptr()), None), 0, "==")
    check_bitwise("vv_reduce_enqueue n=0", dout, [0.0] * 3)


def test_negative_length_refused(ctx):
    """n < 0 is VV_E_ARG in every vector entry point, as vv_reduce_batch already answered; nothing is launched."""
    from vaevar._lib import lib

    x0 = torch.tensor([1.5, -2.0, 3.25, 4.0])
    x, y, mm, vv = dev(x0), dev(x0), dev(x0), dev(x0)
    px, py, pm, pv = _raw_args(x, y, mm, vv)
    h = ctx.h
    d, m = ctypes.c_double(), ctypes.c_float()
    ops = (ctypes.c_int * 1)(1)
    A, B = (ctypes.c_void_p * 1)(px.value), (ctypes.c_void_p * 1)(py.value)
    out = (ctypes.c_double * 1)()
    dout = dev(torch.zeros(1, dtype=torch.float64))
    ro = (ctypes.c_float * 1)(1.0)
    for n in (-1, -(1 << 40)):
        got = {
            "vv_axpy": lib.vv_axpy(h, py, px, 2.0, n, None),
            "vv_axpby": lib.vv_axpby(h, py, px, 2.0, py, 3.0, n, None),
            "vv_scale": lib.vv_scale(h, py, 2.0, n, None),
            "vv_copy": lib.vv_copy(h, py, px, n, None),
            "vv_dot": lib.vv_dot(h, px, py, n, ctypes.byref(d), None),
            "vv_abssum": lib.vv_abssum(h, px, n, ctypes.byref(d), None),
            "vv_absmax": lib.vv_absmax(h, px, n, ctypes.byref(m), None),
            "vv_reduce_batch": lib.vv_reduce_batch(h, 1, ops, A, B, n, None, 0, out, None),
            "vv_reduce_enqueue": lib.vv_reduce_enqueue(h, 1, ops, A, B, n, ctypes.c_void_p(dout.data_ptr()), None),
            "vv_lbfgs_two_loop": lib.vv_lbfgs_two_loop(h, py, A, B, ro, 1, 0.5, n, None),
            "vv_adam": lib.vv_adam(h, py, px, pm, pv, n, 1e-3, 0.9, 0.999, 1e-8, 1, None),
        }
        for name, rc in got.items():
            check(f"{name} n={n} status", rc, VV_E_ARG, "==")
    torch.cuda.synchronize()
    check_bitwise("n<0: operands untouched", torch.stack([x, y, mm, vv]), torch.stack([x0] * 4))


# --------------------------------------------------------------------------------------------------------------------
# A4. the two-loop recursion
# --------------------------------------------------------------------------------------------------------------------
def _history(n, m, seed):
    """q = -g random and m pairs (s_i random, y_i = D s_i with a fixed diagonal D in [0.5, 2]: y_i . s_i > 0 and a
    stable recursion)."""
    g = torch.Generator().manual_seed(seed)
    D = 0.5 + 1.5 * torch.rand(n, generator=g)
    q = torch.randn(n, generator=g)
    S = [torch.randn(n, generator=g) for _ in range(m)]
    return q, S, [D * s for s in S]


def _ro_h(S, Y):
    """ro_i = 1 / (y_i . s_i) and H_diag = y.s / y.y of the last pair, in the mirror's fp32 scalars."""
    if not S:
        return [], 1.0
    ys = [f32((y.double() * s.double()).sum()) for s, y in zip(S, Y)]
    return [float(f32(1.0) / v) for v in ys], float(ys[-1] / f32((Y[-1].double() * Y[-1].double()).sum()))


def _two_loop_fp64(q, S, Y):
    """The same recursion entirely in float64 (ro and H_diag too) on the fp32 vectors."""
    q, S, Y = q.double(), [s.double() for s in S], [y.double() for y in Y]
    m = len(S)
    ro = [1.0 / float((Y[i] * S[i]).sum()) for i in range(m)]
    H = float((Y[-1] * S[-1]).sum()) / float((Y[-1] * Y[-1]).sum()) if m else 1.0
    al = [0.0] * m
    for i in range(m - 1, -1, -1):
        al[i] = float((S[i] * q).sum()) * ro[i]
        q = q - al[i] * Y[i]
    q = q * H
    for i in range(m):
        be = float((Y[i] * q).sum()) * ro[i]
        q = q + (al[i] - be) * S[i]
    return q


def _two_loop_host_scalars(ctx, q, S, Y, ro, H):
    """The device_two_loop=False branch of vaevar/lbfgs.py: one synchronising dot per coefficient, the coefficient
    formed in fp32 on the host."""
    m = len(S)
    al = [None] * m
    for i in range(m - 1, -1, -1):
        al[i] = f32(ctx.dot(S[i], q)) * f32(ro[i])
        ctx.axpy(q, Y[i], float(-al[i]))
    ctx.scale(q, float(H))
    for i in range(m):
        be = f32(ctx.dot(Y[i], q)) * f32(ro[i])
        ctx.axpy(q, S[i], float(al[i] - be))


def _check_two_loop(ctx, n, ms, seed):
    q, S, Y = _history(n, max(ms), seed)
    dS, dY = [dev(s) for s in S], [dev(y) for y in Y]
    for m in ms:
        # the newest m pairs, oldest first
        s, y, ds, dy = S[len(S) - m:], Y[len(Y) - m:], dS[len(S) - m:], dY[len(Y) - m:]
        ro, H = _ro_h(s, y)
        d_dev = dev(q)
        ctx.lbfgs_two_loop(d_dev, ds, dy, ro, H)
        d_host = dev(q)
        _two_loop_host_scalars(ctx, d_host, ds, dy, ro, H)
        check_bitwise(f"n={n} m={m} device two-loop vs host scalars", d_dev, d_host)
        d_cpu = q.clone()
        CpuPrims().lbfgs_two_loop(d_cpu, s, y, ro, H)
        d64 = _two_loop_fp64(q, s, y)
        scale = float(d64.abs().max())
        yard = float((d_cpu.double() - d64).abs().max()) / scale
        err = float((d_dev.cpu().double() - d64).abs().max()) / scale
        note(f"n={n} m={m} yardstick: CpuPrims two-loop vs fp64 (max-norm rel)", yard)
        check(f"n={n} m={m} device two-loop vs fp64 (max-norm rel, bound 2 x yardstick)", err, 2 * yard, "<=")


@pytest.mark.parametrize("n", [1, 257, 262_145, 1_048_576, 1_048_577, NMAX])
def test_two_loop(ctx, n):
    """vv_lbfgs_two_loop (k_twoloop_axpy_dot: four prefetched elements per thread, then a grid-stride tail that only
    n > 1,048,576 enters) against (1) the host-scalar sequence f32(vv_dot) * f32(ro), vv_axpy, vv_scale, bit for bit,
    for history sizes 0, 1, 2 and 10, and (2) the recursion in float64. Yardstick of (2): the distance of
    CpuPrims.lbfgs_two_loop (torch fp32 axpys, the same fp32 coefficients) from the float64 recursion, in max-norm
    relative to max |d|; the device, whose dots are fp64-accumulated too, stays within 2 x that distance (the factor
    covers fused against unfused fp32 multiply-adds)."""
    _check_two_loop(ctx, n, (0, 1, 2, 10), seed=1000 + n % 997)


def test_two_loop_long_history(ctx):
    """History sizes far from the default 10: 100 and 256 (the ABI's maximum) at n = 4099, checked as in
    test_two_loop; 257 pairs are refused."""
    from vaevar._lib import VVError

    _check_two_loop(ctx, 4099, (100, 256), seed=77)
    q = dev(torch.zeros(4099))
    with pytest.raises(VVError, match=str(VV_E_ARG)):
        ctx.lbfgs_two_loop(q, [q] * 257, [q] * 257, [1.0] * 257, 1.0)
    check_bitwise("m=257 refused: q untouched", q, torch.zeros(4099))


# --------------------------------------------------------------------------------------------------------------------
# A5. Adam
# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lr", [1e-3, 0.1])
def test_adam_vs_fp64(ctx, lr):
    """60 steps of vv_adam at n = 4099 on gradients of magnitudes 1e-3 .. 1e3 with exact zeros (a tenth of every step's
    entries, and 64 entries that never see a gradient). Reference: Adam in float64 on the same fp32 gradients with
    betas, eps and lr as Python doubles. Yardstick: the distance of torch.optim.Adam (fp32, CPU) from that run in
    max-norm; at every 10th step the device is within 2 x the yardstick of the float64 run (it runs the same fp32
    recurrences; the factor covers their rounding in a different order). vv_adam forms 1 - beta^t in double for
    this: with 1 - powf(beta, t) in fp32 (library version 102) the lr = 0.1 run missed the bound from step 10 on
    (8.9e-7 against 2 x 3.6e-7), the lr = 1e-3 run passed."""
    n, steps, b1, b2, eps = 4099, 60, 0.9, 0.999, 1e-8
    g = torch.Generator().manual_seed(4099)
    p0 = torch.rand(n, generator=g) * 2 - 1
    mag = torch.exp(torch.rand(n, generator=g) * (2 * np.log(1e3)) - np.log(1e3))
    pt = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([pt], lr=lr, betas=(b1, b2), eps=eps)
    p64, m64, v64 = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    p, m, v = dev(p0), dev(torch.zeros(n)), dev(torch.zeros(n))
    for t in range(1, steps + 1):
        gr = mag * torch.randn(n, generator=g)
        gr[torch.rand(n, generator=g) < 0.1] = 0.0
        gr[:64] = 0.0
        opt.zero_grad()
        pt.grad = gr.clone()
        opt.step()
        g64 = gr.double()
        m64 = m64 + (g64 - m64) * (1 - b1)
        v64 = b2 * v64 + (1 - b2) * g64 * g64
        p64 = p64 - lr / (1 - b1 ** t) * (m64 / (v64.sqrt() / np.sqrt(1 - b2 ** t) + eps))
        ctx.adam(p, dev(gr), m, v, lr, b1, b2, eps, t)
        if t % 10 == 0:
            yard = float((pt.detach().double() - p64).abs().max())
            err = float((p.cpu().double() - p64).abs().max())
            note(f"lr={lr} step {t} yardstick: torch.optim.Adam fp32 vs fp64 (max abs)", yard)
            check(f"lr={lr} step {t} vv_adam vs fp64 (max abs, bound 2 x yardstick)", err, 2 * yard, "<=")
    check_bitwise(f"lr={lr}: entries without a gradient never move", p[:64], p0[:64])
