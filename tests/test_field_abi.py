"""CPU: every stand-alone field operation of the C ABI (vv_metrics ... vv_obs_project, csrc/vv_fieldapi.hip) refuses a
bad call before any device work. One table of refused calls: per entry point each required pointer null, each extent
zero, the operator bounds on both sides, every 2^31-type limit at its first refused value and every overlap, flag and
mode refusal. Every case returns VV_E_ARG (1001) and leaves a fresh message in vv_last_error; none reaches the context
(a dummy non-null handle stands in for it), so no GPU is needed -- and with one present the test skips itself: a call
that is wrongly accepted would go on to launch on made-up pointers."""
import ctypes

import pytest
import torch

_KEEP = ctypes.create_string_buffer(1 << 20)  # never dereferenced
_BASE = ctypes.addressof(_KEEP)


def P(i):
    """Made-up buffer number i: 32 KiB apart, so the small base shapes below never overlap by accident."""
    return _BASE + (i << 15)


I64_MAX = (1 << 63) - 1
CTX = P(31)

# entry point -> (arguments in ABI order with an accepted value each, required pointers, extents refused at zero,
# further refused calls as name -> overrides)
SPEC = {
    "vv_metrics": (
        dict(ctx=CTX, pred=P(0), gt=P(1), mean=P(2), std=P(3), scale=P(4), B=1, C=2, H=8, W=8, wrmse=P(5), bias=P(6),
             stream=None),
        ["pred", "gt", "mean", "std", "scale", "wrmse", "bias"], ["B", "C", "W"],
        {"H_1": dict(H=1)}),
    "vv_verify": (
        dict(ctx=CTX, pred=P(0), gt=P(1), clim=P(2), mean=P(3), std=P(4), scale=P(5), B=1, C=2, H=9, W=8, out=P(6),
             stream=None),
        ["pred", "gt", "mean", "std", "scale", "out"], ["B", "C", "W"],
        {"BC_65536": dict(B=1, C=65536), "H_0": dict(H=0), "H_2_empty_region": dict(H=2)}),
    "vv_obs_augment": (
        dict(ctx=CTX, interp=P(0), n_out=40, n_in=13, x=P(1), x_aug=P(2), T=1, Hs=8, Ws=8, stream=None),
        ["interp", "x", "x_aug"], ["T", "Hs", "Ws"],
        {"n_in_0": dict(n_in=0), "n_in_17": dict(n_in=17), "n_out_0": dict(n_out=0), "n_out_65": dict(n_out=65)}),
    "vv_obs_error": (
        dict(ctx=CTX, x=P(0), yo=P(1), H=P(2), mask=P(3), interp=P(4), n_out=40, n_in=13, C=69, Hs=8, Ws=8, err=P(5),
             sums=None, stream=None),
        ["x", "yo", "H", "mask", "err"], ["Hs", "Ws"],
        {"identity_C_0": dict(interp=None, C=0), "n_in_0": dict(n_in=0, C=4), "n_in_17": dict(n_in=17, C=4 + 5 * 17),
         "n_out_0": dict(n_out=0), "n_out_65": dict(n_out=65), "C_68_n_in_13": dict(C=68),
         "HW_2^31-4096": dict(Hs=1, Ws=0x7FFFFFFF - 4096 + 1)}),
    "vv_obs_qc": (
        dict(ctx=CTX, gt=P(0), yo=P(1), H=P(2), interp=P(3), n_out=40, n_in=13, thr=P(4), flags=1, T=1, C=69, Hs=8,
             Ws=8, counts=None, stream=None),
        ["gt", "yo", "H", "thr"], ["T", "Hs", "Ws"],
        {"identity_C_0": dict(interp=None, C=0), "n_in_0": dict(n_in=0, C=4), "n_in_17": dict(n_in=17, C=4 + 5 * 17),
         "n_out_0": dict(n_out=0), "n_out_65": dict(n_out=65), "C_68_n_in_13": dict(C=68),
         "HW_2^31-4096": dict(Hs=1, Ws=0x80000000 - 4096),
         "flags_16": dict(flags=16), "flags_exempt_without_filter": dict(flags=2), "flags_simu_and_simu_z": dict(flags=12),
         "flags_exempt_z_identity": dict(interp=None, flags=3), "flags_simu_z_identity": dict(interp=None, flags=8),
         "yo_is_H": dict(H=P(1))}),
    "vv_obs_grid": (
        dict(ctx=CTX, reports=P(0), n=1, mode=0, da_win=6, n_lev=2, Hs=8, Ws=8, bounds=P(1), log_lev=P(2), zcoef=P(3),
             tcoef=P(4), yo=P(5), H=P(6), stats=None, stream=None),
        ["H"], ["Hs", "Ws"],
        {"mode_2": dict(mode=2), "da_win_2": dict(da_win=2), "n_-1": dict(n=-1), "reports_null": dict(reports=None),
         "n_lev_0": dict(n_lev=0), "n_lev_65": dict(n_lev=65), "bounds_null": dict(bounds=None),
         "yo_null_real": dict(yo=None), "log_lev_null_real": dict(log_lev=None), "zcoef_null_real": dict(zcoef=None),
         "tcoef_null_real": dict(tcoef=None), "yo_is_H": dict(yo=P(6)),
         "cells_2^31": dict(da_win=1, n_lev=1, Hs=1, Ws=238609295),  # 9 * 238609295 = 2^31 + 7, 9 * ...294 is below
         "n_238609295": dict(n=(0x7FFFFFFF - 1) // 9 + 1)}),
    "vv_obs_synth": (
        dict(ctx=CTX, gt=P(0), T=1, C=2, Hs=8, Ws=8, n_obs=5, seed=1, noise_seed=2, draw=0, sd=None, rtab=P(1),
             yo=P(2), H=P(3), R=P(4), stats=None, stream=None),
        ["gt", "yo", "H"], ["T", "C", "Hs", "Ws"],
        {"elements_2^31": dict(T=2, C=1, Hs=1, Ws=1 << 30),
         "n_obs_-1": dict(n_obs=-1), "n_obs_HW+1": dict(n_obs=65), "R_without_rtab": dict(rtab=None),
         "rtab_without_R": dict(R=None), "H_overlaps_gt": dict(H=P(0) + 4 * 127), "H_overlaps_yo": dict(H=P(2) - 4 * 127),
         "H_overlaps_R": dict(H=P(4)), "R_overlaps_gt": dict(R=P(0) - 4 * 127), "R_overlaps_yo": dict(R=P(2) + 4 * 127),
         "yo_overlaps_gt": dict(yo=P(0) + 4)}),
    "vv_select_smallest": (
        dict(ctx=CTX, keys=P(0), n=64, k=5, mask=P(1), stats=None, stream=None),
        ["keys", "mask"], ["n"],
        {"n_2^31": dict(n=1 << 31, k=0), "k_-1": dict(k=-1), "k_n+1": dict(k=65)}),
    "vv_normal_fill": (
        dict(ctx=CTX, out=P(0), n=64, first=0, seed=1, draw=0, stream=None),
        ["out"], [],
        {"n_-1": dict(n=-1), "first_-1": dict(first=-1), "first+n_overflows": dict(first=I64_MAX, n=1)}),
    "vv_err_accum": (
        dict(ctx=CTX, pred=P(0), ps=128, tgt=P(1), ts=128, B=2, C=2, H=8, W=8, cell=P(2), chan=P(3), stream=None),
        ["pred", "tgt"], ["B", "C", "H", "W"],
        {"cell_and_chan_null": dict(cell=None, chan=None), "CHW_2^31": dict(C=2, H=1, W=1 << 30, ps=1 << 31, ts=1 << 31),
         "pred_stride_CHW-1": dict(ps=127), "tgt_stride_CHW-1": dict(ts=127)}),
    "vv_err_finalize": (
        dict(ctx=CTX, cell=P(0), n_samples=3, C=2, H=8, W=8, q_field=P(1), q_tab=P(2), stream=None),
        ["cell"], ["n_samples", "C", "H", "W"],
        {"q_field_and_q_tab_null": dict(q_field=None, q_tab=None), "CHW_2^31": dict(C=2, H=1, W=1 << 30)}),
    "vv_r_fill": (
        dict(ctx=CTX, rtab=P(0), interp=P(1), n_out=40, n_in=13, T=1, C=69, Hs=8, Ws=8, R=P(2), stream=None),
        ["rtab", "R"], ["T", "Hs", "Ws"],
        {"identity_C_0": dict(interp=None, C=0), "n_in_0": dict(n_in=0, C=4), "n_in_17": dict(n_in=17, C=4 + 5 * 17),
         "n_out_0": dict(n_out=0), "n_out_65": dict(n_out=65), "C_68_n_in_13": dict(C=68),
         "HW_2^31": dict(interp=None, C=1, Hs=2, Ws=1 << 30),
         # 4096 planes of 2^19 chunks each: (2^19 - 1) * 4096 < Hs * Ws
         "workgroups_2^31": dict(interp=None, T=4096, C=1, Hs=1, Ws=(1 << 31) - 4095)}),
    "vv_vae_sample": (
        dict(ctx=CTX, enc=P(0), B=1, L=2, H=8, W=8, seed=1, draw=0, flags=0, z=P(1), stat=P(2), stream=None),
        ["enc"], ["B", "L", "H", "W"],
        {"z_and_stat_null": dict(z=None, stat=None), "flags_2": dict(flags=2),
         "elements_2^31": dict(B=1, L=1, H=1, W=1 << 30, z=None), "z_is_enc": dict(z=P(0)),
         "z_overlaps_enc_end": dict(z=P(0) + 4 * 255), "z_overlaps_enc_start": dict(z=P(0) - 4 * 127)}),
    "vv_vae_sse": (
        dict(ctx=CTX, recon=P(0), rs=128, x=P(1), xs=128, B=2, C=2, H=8, W=8, sse=P(2), stream=None),
        ["recon", "x", "sse"], ["B", "C", "H", "W"],
        {"CHW_2^31": dict(C=2, H=1, W=1 << 30, rs=1 << 31, xs=1 << 31), "recon_stride_CHW-1": dict(rs=127),
         "x_stride_CHW-1": dict(xs=127),
         "workgroups_2^31": dict(B=4096, C=1, H=1, W=(1 << 31) - 4095, rs=1 << 31, xs=1 << 31)}),
    "vv_err_sample": (
        dict(ctx=CTX, pred=P(0), ps=128, tgt=P(1), ts=128, B=2, C=2, Hs=8, Ws=8, err_std=P(2), Hn=4, Wn=4, out=P(3),
             stream=None),
        ["pred", "tgt", "err_std", "out"], ["B", "C", "Hs", "Ws", "Hn", "Wn"],
        {"CHW_2^31": dict(C=2, Hs=1, Ws=1 << 30, ps=1 << 31, ts=1 << 31), "output_2^31": dict(B=1, Hn=1, Wn=1 << 30),
         "pred_stride_CHW-1": dict(ps=127), "tgt_stride_CHW-1": dict(ts=127)}),
    "vv_tri_interp": (
        dict(ctx=CTX, tris=P(0), n_tri=3, yo=P(1), H=P(2), xa=P(3), C=2, Hs=8, Ws=8, stats=None, stream=None),
        ["yo", "H", "xa"], ["C", "Hs", "Ws"],
        {"n_tri_-1": dict(n_tri=-1), "tris_null": dict(tris=None), "n_tri_2^31": dict(n_tri=1 << 31),
         "Hs_16385": dict(Hs=16385, C=1, Ws=1), "Ws_16385": dict(Ws=16385, C=1, Hs=1),
         "xa_overlaps_yo": dict(xa=P(1) + 4 * 127), "xa_overlaps_H": dict(xa=P(2) - 4 * 127)}),
    "vv_obs_project": (
        dict(ctx=CTX, interp_inv=P(0), n_out=13, n_in=40, x_aug=P(1), x=P(2), T=1, Hs=8, Ws=8, stream=None),
        ["interp_inv", "x_aug", "x"], ["T", "Hs", "Ws"],
        {"n_in_0": dict(n_in=0), "n_in_65": dict(n_in=65), "n_out_0": dict(n_out=0), "n_out_17": dict(n_out=17),
         "HW_2^31-1-2^19": dict(Hs=1, Ws=0x7FFFFFFF - 256 * 2048), "x_is_x_aug": dict(x=P(1))}),
}


def _cases():
    out = []
    for fn, (base, ptrs, extents, more) in SPEC.items():
        out.append((fn, "null_ctx", dict(ctx=None)))
        out += [(fn, f"null_{p}", {p: None}) for p in ptrs]
        out += [(fn, f"{e}_0", {e: 0}) for e in extents]
        out += [(fn, name, over) for name, over in more.items()]
    return out


CASES = _cases()


def _msg(lib):
    buf = ctypes.create_string_buffer(512)
    lib.vv_last_error(buf, 512)
    return buf.value


def test_table_covers_every_field_operation():
    from vaevar import _lib

    assert len(SPEC) == 17 and all(fn in _lib.EXPORTED for fn in SPEC)
    for fn, (base, ptrs, extents, more) in SPEC.items():
        assert len(base) == len(getattr(_lib.lib, fn).argtypes), fn
        assert all(k in base for k in ptrs + extents) and all(k in base for o in more.values() for k in o), fn


@pytest.mark.parametrize("fn,name,over", CASES, ids=[f"{fn}-{name}" for fn, name, _ in CASES])
def test_field_operation_refuses(fn, name, over):
    if torch.cuda.is_available():
        pytest.skip("a wrongly accepted call would launch on made-up pointers")
    from vaevar import _lib

    lib = _lib.lib
    args = dict(SPEC[fn][0])
    args.update(over)
    # clear the thread's last error with a call that fails differently, so the message below is this call's
    assert lib.vv_set_tuning(None, b"h3_mink", 1) == 1001
    before = _msg(lib)
    assert getattr(lib, fn)(*args.values()) == 1001
    after = _msg(lib)
    assert after and after != before
