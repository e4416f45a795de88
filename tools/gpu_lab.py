#!/usr/bin/env python3
"""Bring-up lab: runs every kernel family against a torch reference and the tiny model against the oracle,
printing errors for ALL cases (never stops at the first failure).  Usage on the GPU box:
    python tools/gpu_lab.py [kernels] [model] > gpurun_out/lab.log
"""
import ctypes as C
import os
import sys
import time
import traceback

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dmmfods_amd import _lib  # noqa: E402
from tools import exact_operands  # noqa: E402

DEV = "cuda"
L = _lib.lib()


def nhwc(x, dt):
    return x.permute(0, 2, 3, 1).contiguous().to(dt)


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous().float()


def relerr(a, b):
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def _check_family(res_name, expect):
    """Did the family the case names really run?  (The single-kernel entry points fall back to the generic kernels silently.)"""
    if expect is None:
        return True
    ran = _lib.impls_since_reset()
    ok = expect in ran
    if not ok:
        print(f"FAIL {res_name}: expected kernel family {expect!r}, ran {sorted(ran)}", flush=True)
    return ok


def _absdiff(a, b):
    """max |a - b| in fp64: what the exact-operand cases hold to zero."""
    return (a.double() - b.double()).abs().max().item()


def _ndiff(a, b):
    """Number of elements of a that are not equal to b (a NaN equals nothing): what the single-rounding cases hold to zero."""
    return float((a.double() != b.double()).sum())


def _ratio(got, ref, bound):
    """Worst |got - ref| / bound, element by element; a bound of zero must be met exactly (ratio 0 or inf), a NaN is infinitely far."""
    diff = (got.double() - ref.double()).abs()
    rk = torch.where(bound > 0, diff / bound.clamp_min(1e-300), (diff != 0).double() * float("inf"))
    return _maxabs(rk)


def _verdict(res, exact, tol, bounded=()):
    """Names of the compared tensors that miss: any difference at all on exact operands - on the single-rounding operands
    (exact="round") any differing element, and for the `bounded` quantities any |diff| / bound above 1 - else the relative tolerance
    (a number or a dict per tensor)."""
    if exact:
        return [k for k, v in res.items() if not ((v <= 1) if k in bounded else (v == 0))]
    return [k for k, v in res.items() if not (v < (tol[k] if isinstance(tol, dict) else tol))]


def _show(res, exact, bounded=()):
    if exact == "round":   # per tensor the number of differing elements; for the bounded quantities the worst |diff| / bound
        return " ".join(f"{k}/bound={v:.3g}" if k in bounded else f"{k}={int(v)}" for k, v in res.items())
    return " ".join(f"{k}={v:.2e}" for k, v in res.items())


def _operands(exact, *args, **kw):
    """The operands and fp64 reference of an exact case, their conditions checked on the reference alone before anything is launched:
    exact=True the round-8 operands (nothing rounds), exact="round" the single-rounding operands (every store rounds once)."""
    if exact == "round":
        o = exact_operands.cached_rounding_operands(*args, **kw)
        o.check_rounding()
    else:
        o = exact_operands.cached_operands(*args, **kw)
        o.check()
    return o


def conv_case(name, dtype, mfma, B, H, W, Cin, Cout, R, S, stride, pad, transposed=0, mode=0, bn=1, seed=0, expect_wgrad=None,
              expect_fwd=None, expect_dgrad=None, exact=False, parts=("fwd", "wgrad", "dgrad"), exact_kw=None, merged=False,
              expect_launches=None, keep=None):
    """Forward (+ statistics), weight gradient and BN-fused data gradient of one convolution through the single-kernel entry points.
    expect_*: the kernel family that must have run that launch.  exact: operands of tools/exact_operands.py and an fp64 CPU reference;
    ok only if every compared tensor is equal bit for bit (parts: which of the three launches to run and compare; exact_kw: further arguments of make_operands).
    exact="round": the single-rounding operands (make_rounding_operands) - every tensor stored in the storage type, stat_sum and red1
    equal bit for bit; stat_sq, red2 and a weight gradient that is not exact in fp32 within the bounds derived from the reference.
    merged: the forward of a ConvTranspose as a plan launches it (dmm_conv_forward_merged: the four output-parity phases in ONE launch
    where the plan's merge accepts them) - parts=("fwd",) only; the output and the statistics lie between guard bands of NaN, which
    must still be NaN afterwards; expect_launches: what the entry point must report (1 merged, 4 kept apart); expect_fwd may then be
    a set: exactly the families that must have noted the launch(es).  keep: a dict that receives output and statistics as read back."""
    dt = {0: torch.float32, 1: torch.float16, 2: torch.bfloat16}[dtype]
    assert not merged or (transposed and exact and tuple(parts) == ("fwd",))
    if exact:
        o = _operands(exact, dtype, B, H, W, Cin, Cout, R, S, stride, pad, transposed=transposed, mode=mode, bn=bn,
                      parts=tuple(parts), seed=seed, **(exact_kw or {}))
        parts = o.parts
        x, scale, shift, w, dy, mean, invstd = (t.float() for t in (o.x, o.scale, o.shift, o.w, o.dy, o.mean, o.invstd))
        wshape = tuple(w.shape)
        y = o.y
    else:
        g = torch.Generator().manual_seed(seed)
        x = (torch.randn(B, Cin, H, W, generator=g) * 2 + 0.5)
        scale = torch.rand(Cin, generator=g) + 0.5
        shift = torch.randn(Cin, generator=g) * 0.5
        wshape = (Cin, Cout, 3, 3) if transposed else (Cout, Cin, R, S)
        w = torch.randn(wshape, generator=g) / (Cin * R * S) ** 0.5
        xq = x.to(dt).float()
        a = F.relu(xq * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)) if bn else xq
        a = a.requires_grad_(True)
        wq = w.clone().requires_grad_(True)
        if transposed:
            y = F.conv_transpose2d(a, wq, stride=2, padding=1, output_padding=1)
        elif mode == 1:
            y = F.conv2d(F.interpolate(a, scale_factor=2, mode="nearest"), wq, padding=pad)
        elif mode == 2:
            y = F.avg_pool2d(F.conv2d(a, wq), 2, 2)
        else:
            y = F.conv2d(a, wq, stride=stride, padding=pad)
        dy = torch.randn(y.shape, generator=g)
        dyq = dy.to(dt).float()
        (y * dyq).sum().backward()
        # dgrad entry point wants [shift | mean | invstd]; any mean/invstd define xhat for the second reduction
        mean = torch.randn(Cin, generator=g)
        invstd = torch.rand(Cin, generator=g) + 0.5
    rnd = exact == "round"
    err = _ndiff if rnd else (_absdiff if exact else relerr)
    bounded = set()
    d = _lib.ConvDesc(dtype=dtype, use_mfma=mfma, B=B, H=H, W=W, Cin=Cin, Cout=Cout, R=R, S=S, stride=stride, pad=pad,
                      transposed=transposed, mode=mode, bn_relu=bn)
    nsc = L.dmm_conv_scratch_bytes(C.byref(d))
    scratch = torch.zeros(nsc, dtype=torch.uint8, device=DEV)
    xd = nhwc(x, dt).to(DEV)
    wd, sd, hd = w.to(DEV), scale.to(DEV), torch.cat([shift, mean, invstd]).to(DEV)
    st = _lib.stream_ptr()
    res = {}
    fam_ok = True
    if "fwd" in parts and merged:
        ny = B * y.shape[2] * y.shape[3] * Cout
        ybuf = torch.full((ny + 2 * GUARD,), float("nan"), dtype=dt, device=DEV)
        sbuf = torch.full((2 * Cout + 2 * GUARD,), float("nan"), dtype=torch.float64, device=DEV)
        yd, stats = ybuf[GUARD:GUARD + ny].view(B, y.shape[2], y.shape[3], Cout), sbuf[GUARD:GUARD + 2 * Cout]
        nl = C.c_int(-1)
        _lib.impls_since_reset()
        _lib.check(L.dmm_conv_forward_merged(C.byref(d), xd.data_ptr(), wd.data_ptr(), sd.data_ptr(), hd.data_ptr(), yd.data_ptr(),
                                             stats.data_ptr(), scratch.data_ptr(), st, C.byref(nl)))
        torch.cuda.synchronize()
        fam_ok &= _check_merged(name + " fwd", expect_fwd, expect_launches, nl.value)
        res["guard"] = _guard_hits(ybuf, ny) + _guard_hits(sbuf, 2 * Cout)
        yo = nchw(yd).cpu()
        if keep is not None:
            keep.update(y=yd.cpu().clone(), stats=stats.cpu().clone(), launches=nl.value)
    elif "fwd" in parts:
        yd = torch.full((B, y.shape[2], y.shape[3], Cout), float("nan"), dtype=dt, device=DEV)
        stats = torch.zeros(2 * Cout, dtype=torch.float64, device=DEV)
        _lib.impls_since_reset()
        _lib.check(L.dmm_conv_forward(C.byref(d), xd.data_ptr(), wd.data_ptr(), sd.data_ptr(), hd.data_ptr(), yd.data_ptr(),
                                      stats.data_ptr(), scratch.data_ptr(), st))
        torch.cuda.synchronize()
        fam_ok &= _check_family(name + " fwd", expect_fwd)
        yo = nchw(yd).cpu()
    if "fwd" in parts:
        res["fwd"] = err(yo, y.detach())
        res["sum"] = err(stats[:Cout].cpu(), o.stat_sum if exact else yo.double().sum(dim=(0, 2, 3)))
        if rnd:
            res["sq"] = _ratio(stats[Cout:].cpu(), o.stat_sq, o.sq_bound)
            bounded.add("sq")
        else:
            res["sq"] = err(stats[Cout:].cpu(), o.stat_sq if exact else (yo.double() ** 2).sum(dim=(0, 2, 3)))
    dyd = nhwc(dy, dt).to(DEV)
    if "wgrad" in parts:
        dwd = torch.full(wshape, float("nan"), device=DEV)
        _lib.impls_since_reset()
        _lib.check(L.dmm_conv_wgrad(C.byref(d), xd.data_ptr(), dyd.data_ptr(), sd.data_ptr(), hd.data_ptr(), dwd.data_ptr(),
                                    scratch.data_ptr(), st))
        torch.cuda.synchronize()
        fam_ok &= _check_family(name + " wgrad", expect_wgrad)
        if rnd and not o.dw_exact:
            res["wgrad"] = _ratio(dwd.cpu(), o.dw, o.dw_bound)
            bounded.add("wgrad")
        else:
            res["wgrad"] = err(dwd.cpu(), o.dw if exact else wq.grad)
    # dgrad (BN fused)
    if "dgrad" in parts and bn and not (mode == 0 and not transposed and stride != 1):
        if exact:
            gx_ref, red1_ref, red2_ref = o.gx, o.red1, o.red2
        else:
            z = xq * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
            dz = a.grad * (z > 0)
            gx_ref = dz * scale.view(1, -1, 1, 1)
            xhat = (xq.double() - mean.double().view(1, -1, 1, 1)) * invstd.double().view(1, -1, 1, 1)
            red1_ref, red2_ref = dz.double().sum(dim=(0, 2, 3)), (dz.double() * xhat).sum(dim=(0, 2, 3))
        gxd = torch.full((B, H, W, Cin), float("nan"), dtype=dt, device=DEV)
        red = torch.zeros(2 * Cin, dtype=torch.float64, device=DEV)
        _lib.impls_since_reset()
        _lib.check(L.dmm_conv_dgrad(C.byref(d), xd.data_ptr(), dyd.data_ptr(), wd.data_ptr(), sd.data_ptr(), hd.data_ptr(),
                                    gxd.data_ptr(), red.data_ptr(), scratch.data_ptr(), st))
        torch.cuda.synchronize()
        fam_ok &= _check_family(name + " dgrad", expect_dgrad)
        res["dgrad"] = err(nchw(gxd).cpu(), gx_ref)
        res["red1"] = err(red[:Cin].cpu(), red1_ref)
        if rnd:
            res["red2"] = _ratio(red[Cin:].cpu(), red2_ref, o.red2_bound)
            bounded.add("red2")
        else:
            res["red2"] = err(red[Cin:].cpu(), red2_ref)
    tol = {0: 2e-5, 1: 3e-3, 2: 2.5e-2}[dtype]   # relative to the tensor's max: fp32 / f16 (11 bits) / bf16 (8 bits) storage
    bad = _verdict(res, exact, tol, bounded)
    print(f"{'FAIL' if bad else 'ok  '} {name:28s} dt={dtype} mfma={mfma}{(' round' if rnd else ' exact') if exact else ''} " + _show(res, exact, bounded), flush=True)
    return not bad and fam_ok


LOGITS_GUARD = 4096   # floats of NaN on either side of the logits tensor
GUARD = 4096          # elements of NaN on either side of an output of the merged-phase cases


def _guard_hits(buf, n):
    """Elements of the two guard bands around buf[GUARD:GUARD + n] that are no longer NaN."""
    host = buf.cpu()
    return float(int((~torch.isnan(host[:GUARD])).sum()) + int((~torch.isnan(host[GUARD + n:])).sum()))


def _check_merged(res_name, expect, expect_launches, launches):
    """A *_merged entry point: the number of launches it reports, and the families that noted them - a name (must be among them, as
    _check_family) or a set (must be exactly them)."""
    ran = _lib.impls_since_reset()
    ok = (expect_launches is None or launches == expect_launches) and (expect is None or (ran == expect if isinstance(expect, (set, frozenset)) else expect in ran))
    if not ok:
        print(f"FAIL {res_name}: expected {expect_launches} launch(es) on {expect!r}, got {launches} on {sorted(ran)}", flush=True)
    return ok


def logits_case(name, dtype, mfma, B, H, W, Cin, Cout, R, pad, exact=True, expect=None, exact_kw=None, seed=0, keep=None):
    """The logits launch (dmm_conv_logits: the network's last convolution, fp32 NCHW output, no statistics) on the exact operands
    (exact=True) or the single-rounding operands (exact="round") of tools/exact_operands.py, part "logits", behind BN+ReLU.  The
    output lies between two guard bands; tensor and bands start as NaN.  ok only if every logit equals the fp64 reference, both bands
    are still all NaN and the family `expect` ran.  keep: a dict that receives the logits as read back (for run-to-run comparisons)."""
    assert exact in (True, "round")
    dt = {0: torch.float32, 1: torch.float16, 2: torch.bfloat16}[dtype]
    o = _operands(exact, dtype, B, H, W, Cin, Cout, R, R, 1, pad, bn=1, parts=("logits",), seed=seed, **(exact_kw or {}))
    x, scale, shift, w = (t.float() for t in (o.x, o.scale, o.shift, o.w))
    rnd = exact == "round"
    d = _lib.ConvDesc(dtype=dtype, use_mfma=mfma, B=B, H=H, W=W, Cin=Cin, Cout=Cout, R=R, S=R, stride=1, pad=pad, transposed=0, mode=0, bn_relu=1)
    scratch = torch.zeros(L.dmm_conv_scratch_bytes(C.byref(d)), dtype=torch.uint8, device=DEV)
    xd, wd, sd, hd = nhwc(x, dt).to(DEV), w.to(DEV), scale.to(DEV), shift.to(DEV)
    n = B * Cout * o.Ho * o.Wo
    buf = torch.full((n + 2 * LOGITS_GUARD,), float("nan"), device=DEV)
    out = buf[LOGITS_GUARD:LOGITS_GUARD + n]
    _lib.impls_since_reset()
    _lib.check(L.dmm_conv_logits(C.byref(d), xd.data_ptr(), wd.data_ptr(), sd.data_ptr(), hd.data_ptr(), out.data_ptr(), scratch.data_ptr(),
                                 _lib.stream_ptr()))
    torch.cuda.synchronize()
    fam_ok = _check_family(name + " logits", expect)
    host = buf.cpu()
    got = host[LOGITS_GUARD:LOGITS_GUARD + n].view(B, Cout, o.Ho, o.Wo)
    if keep is not None:
        keep["logits"] = got.clone()
    res = {"logits": (_ndiff if rnd else _absdiff)(got, o.y)}
    guard = int((~torch.isnan(host[:LOGITS_GUARD])).sum()) + int((~torch.isnan(host[LOGITS_GUARD + n:])).sum())
    bad = _verdict(res, exact, None) + (["guard"] if guard else [])
    wrong = got.double() != o.y
    where = ""
    if bool(wrong.any()):   # where: the first differing element, how many are NaN, and whether the output is that of padding before the prologue
        b, cl, yy, xx = (int(v) for v in wrong.nonzero()[0])
        where = f" first at (b={b}, class={cl}, y={yy}, x={xx}) got {float(got[b, cl, yy, xx])} want {float(o.y[b, cl, yy, xx])}, {int(wrong.sum())} differ, {int(torch.isnan(got).sum())} NaN"
        if hasattr(o, "y_padnorm") and torch.equal(got.double(), o.y_padnorm):
            where += " - equal to the convolution with the prologue applied to the padding"
    print(f"{'FAIL' if bad else 'ok  '} logits {name:34s} dt={dtype} mfma={mfma}{' round' if rnd else ' exact'} " + _show(res, exact) +
          f" guard={guard}{where}", flush=True)
    return not bad and fam_ok


def _eff_setup(g, dt, B, Cout, Ho, Wo, with_q):
    """Incoming gradient of a convolution output as the plan's launches see it: raw gradient dy, and optionally the deferred
    BatchNorm-backward correction q + r * yfwd of the layer behind it (yfwd = that layer's input = this convolution's output)."""
    kw = dict(generator=g, device=g.device)
    dy = torch.randn(B, Cout, Ho, Wo, **kw)
    dyq = dy.to(dt).float()
    if not with_q:
        return dy, dyq, None, None, None, dyq
    yf = torch.randn(B, Cout, Ho, Wo, **kw) * 1.5
    yfq = yf.to(dt).float()
    q = torch.randn(Cout, **kw) * 0.3
    r = torch.randn(Cout, **kw) * 0.2
    eff = dyq + q.view(1, -1, 1, 1) + r.view(1, -1, 1, 1) * yfq
    return dy, dyq, yf, q, r, eff


def backward_case(name, dtype, B, H, W, Cin, Cout, R, S, pad, transposed=0, with_q=1, acc=0, what="dgrad", seed=0, ref_dev="cpu", mode=0,
                  expect=None, exact=False, exact_kw=None, merged=False, expect_launches=None, keep=None):
    """The backward launches of the timed configuration, each through its C-ABI entry point against autograd of
    torch.nn.functional on the CPU (fp32 reference of the same op, 16-bit-rounded operands):
      what = "fused":  dmm_conv1x1_backward_fused (bw1.hip): data + weight gradient of a 1x1 bottleneck convolution
             "dgrad":  dmm_conv_dgrad_ex with the effective-gradient prologue (conv3.hip PRO=2 for the dense 3x3)
             "wgradT": dmm_conv_wgrad_ex in the transposed form (wg3.hip for the dense 3x3)
             "wgrad":  dmm_conv_wgrad_ex, normal form, with the effective-gradient prologue (wgp.hip for ConvTranspose phases)
    exact: operands of tools/exact_operands.py, fp64 CPU reference, every compared tensor equal bit for bit.  exact="round": the
    single-rounding operands, compared as in conv_case.
    merged (what="wgrad", a ConvTranspose): dmm_conv_wgrad_merged - the four parity phases as ONE launch where the plan's merge accepts
    them; dw lies between guard bands of NaN; expect_launches / a set as expect / keep: as conv_case."""
    dt = {0: torch.float32, 1: torch.float16, 2: torch.bfloat16}[dtype]
    assert not merged or (transposed and exact and what == "wgrad")
    rnd = exact == "round"
    bounded = set()
    if exact:
        parts = {"fused": ("wgrad", "dgrad"), "dgrad": ("dgrad",)}.get(what, ("wgrad",))
        o = _operands(exact, dtype, B, H, W, Cin, Cout, R, S, 2 if transposed else 1, pad, transposed=transposed, mode=mode,
                      bn=1, with_q=with_q, acc=acc, parts=parts, seed=seed, **(exact_kw or {}))
        f32 = lambda t: t.float() if t is not None else None  # noqa: E731
        x, scale, shift, mean, invstd, w, dy, yf, q, r, gold = (f32(t) for t in (o.x, o.scale, o.shift, o.mean, o.invstd, o.w, o.dy, o.yf,
                                                                                 o.q, o.r, o.gold))
        wshape = tuple(w.shape)
        if "dgrad" in parts:
            gx_ref, red1_ref, red2_ref = o.gx, o.red1, o.red2
        dw_ref = o.dw
    else:
        # ref_dev="cuda": the torch reference itself runs on the GPU (production sizes; fp32 autograd of the same op)
        g = torch.Generator(device=ref_dev).manual_seed(seed)
        kw = dict(generator=g, device=ref_dev)
        x = (torch.randn(B, Cin, H, W, **kw) * 2 + 0.5)
        scale = torch.rand(Cin, **kw) + 0.5
        shift = torch.randn(Cin, **kw) * 0.5
        mean = torch.randn(Cin, **kw)
        invstd = torch.rand(Cin, **kw) + 0.5
        wshape = (Cin, Cout, 3, 3) if transposed else (Cout, Cin, R, S)
        w = torch.randn(wshape, **kw) / (Cin * R * S) ** 0.5
        xq = x.to(dt).float()
        z = xq * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
        a = F.relu(z).requires_grad_(True)
        wq = w.clone().requires_grad_(True)
        if transposed:
            y = F.conv_transpose2d(a, wq, stride=2, padding=1, output_padding=1)
        elif mode == 1:   # the head's 3x3 over the nearest-x2 upsampled input (M:120, M:126)
            y = F.conv2d(F.interpolate(a, scale_factor=2, mode="nearest"), wq, padding=pad)
        else:
            y = F.conv2d(a, wq, padding=pad)
        Ho, Wo = y.shape[2], y.shape[3]
        dy, dyq, yf, q, r, eff = _eff_setup(g, dt, B, Cout, Ho, Wo, with_q)
        (y * eff).sum().backward()
        dz = a.grad * (z > 0)
        gold = (torch.randn(B, Cin, H, W, **kw)).to(dt) if acc else None
        gx_ref = dz * scale.view(1, -1, 1, 1) + (gold.float() if acc else 0.0)
        xhat = (xq.double() - mean.double().view(1, -1, 1, 1)) * invstd.double().view(1, -1, 1, 1)
        red1_ref, red2_ref = dz.double().sum(dim=(0, 2, 3)), (dz.double() * xhat).sum(dim=(0, 2, 3))
        dw_ref = wq.grad
    d = _lib.ConvDesc(dtype=dtype, use_mfma=1, B=B, H=H, W=W, Cin=Cin, Cout=Cout, R=R, S=S, stride=2 if transposed else 1, pad=pad,
                      transposed=transposed, mode=mode, bn_relu=1)
    scratch = torch.zeros(L.dmm_conv_scratch_bytes(C.byref(d)), dtype=torch.uint8, device=DEV)
    xd, dyd = nhwc(x, dt).to(DEV), nhwc(dy, dt).to(DEV)
    yfd = nhwc(yf, dt).to(DEV) if with_q else None
    qd, rd = (q.to(DEV), r.to(DEV)) if with_q else (None, None)
    wd, sd, hd = w.to(DEV), scale.to(DEV), torch.cat([shift, mean, invstd]).to(DEV)
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    st = _lib.stream_ptr()
    res = {}
    err = _ndiff if rnd else (_absdiff if exact else relerr)
    gxd = nhwc(gold.float(), dt).to(DEV) if acc else torch.full((B, H, W, Cin), float("nan"), dtype=dt, device=DEV)
    red = torch.zeros(2 * Cin, dtype=torch.float64, device=DEV)
    nw = Cin * Cout * R * S
    wbuf = torch.full((nw + 2 * GUARD,), float("nan"), device=DEV)
    dwd = wbuf[GUARD:GUARD + nw].view(wshape)
    nl = C.c_int(-1)
    _lib.impls_since_reset()
    if merged:
        _lib.check(L.dmm_conv_wgrad_merged(C.byref(d), xd.data_ptr(), dyd.data_ptr(), sd.data_ptr(), hd.data_ptr(), ptr(yfd), ptr(qd), ptr(rd),
                                           dwd.data_ptr(), scratch.data_ptr(), st, C.byref(nl)))
    elif what == "fused":
        _lib.check(L.dmm_conv1x1_backward_fused(C.byref(d), xd.data_ptr(), dyd.data_ptr(), wd.data_ptr(), sd.data_ptr(), hd.data_ptr(),
                                                ptr(yfd), ptr(qd), ptr(rd), gxd.data_ptr(), acc, dwd.data_ptr(), red.data_ptr(),
                                                scratch.data_ptr(), st))
    elif what == "dgrad":
        _lib.check(L.dmm_conv_dgrad_ex(C.byref(d), xd.data_ptr(), dyd.data_ptr(), wd.data_ptr(), sd.data_ptr(), hd.data_ptr(),
                                       ptr(yfd), ptr(qd), ptr(rd), gxd.data_ptr(), acc, red.data_ptr(), scratch.data_ptr(), st))
    else:
        _lib.check(L.dmm_conv_wgrad_ex(C.byref(d), xd.data_ptr(), dyd.data_ptr(), sd.data_ptr(), hd.data_ptr(), ptr(yfd), ptr(qd), ptr(rd),
                                       1 if what == "wgradT" else 0, dwd.data_ptr(), scratch.data_ptr(), st))
    torch.cuda.synchronize()
    fam_ok = _check_merged(f"{what} {name}", expect, expect_launches, nl.value) if merged else _check_family(f"{what} {name}", expect)
    if merged:
        res["guard"] = _guard_hits(wbuf, nw)
        if keep is not None:
            keep.update(dw=dwd.cpu().clone(), launches=nl.value)
    if what in ("fused", "dgrad"):
        res["dgrad"] = err(nchw(gxd).cpu(), gx_ref.cpu())
        res["red1"] = err(red[:Cin].cpu(), red1_ref.cpu())
        if rnd:
            # bw1's f16 epilogue (gather.h bnbwd_slot) adds dz * x in fp32 and centres the total in fp64; every other kernel adds the
            # centred product dz * xhat, with xhat exact in fp32 on these operands
            unc = what == "fused" and dtype == 1
            res["red2"] = _ratio(red[Cin:].cpu(), red2_ref, o.red2_bound + (o.red2_unc if unc else 0.0))
            bounded.add("red2")
        else:
            res["red2"] = err(red[Cin:].cpu(), red2_ref.cpu())
    if what != "dgrad":
        if rnd and not o.dw_exact:
            res["wgrad"] = _ratio(dwd.cpu(), dw_ref, o.dw_bound)
            bounded.add("wgrad")
        else:
            res["wgrad"] = err(dwd.cpu(), dw_ref.cpu())
    tol = {0: 2e-5, 1: 3e-3, 2: 2.5e-2}[dtype]
    bad = _verdict(res, exact, tol, bounded)
    print(f"{'FAIL' if bad else 'ok  '} {what:6s} {name:28s} dt={dtype} q={with_q} acc={acc}{(' round' if rnd else ' exact') if exact else ''} " + _show(res, exact, bounded), flush=True)
    return not bad and fam_ok


def conv5_stats_case(name, dtype, B, H, W, Cout=3, seed=0, ref_dev="cpu", exact=False, exact_kw=None):
    """dmm_conv5_wgrad_stats (round 5; wg5.hip PA = 3 + wg5_fin64_kernel): the head's 5x5 convolution behind BN+ReLU - weight gradient
    AND the two BatchNorm-backward sums of the norm in front of it from one pass over x and dy - against fp64 torch on the same
    16-bit-rounded operands: dz = [bn(x) > 0] * conv_dgrad(dy, w rounded to the storage type).  The sums are held to 1e-6 (f16) of the
    largest channel sum: they feed a norm ON the data-gradient chain, where a per-channel offset is amplified ~1e4-fold by the
    encoder behind it (the data-gradient pass these sums used to come from staged dz in 16 bits: 3e-6 / 3e-5 off)."""
    dt = {1: torch.float16, 2: torch.bfloat16}[dtype]
    Cin = 64
    if exact:   # operands of tools/exact_operands.py: weight gradient and both sums equal to fp64 bit for bit
        o = _operands(exact, dtype, B, H, W, Cin, Cout, 5, 5, 1, 2, parts=("wgrad", "dgrad"), seed=seed, **(exact_kw or {}))
        x, scale, shift, mean, invstd, w, dy = (t.float() for t in (o.x, o.scale, o.shift, o.mean, o.invstd, o.w, o.dy))
        red1_ref, red2_ref, dw_ref = o.red1, o.red2, o.dw
    else:
        g = torch.Generator(device=ref_dev).manual_seed(seed)
        kw = dict(generator=g, device=ref_dev)
        x = torch.randn(B, Cin, H, W, **kw) * 2 + 0.5
        scale = torch.rand(Cin, **kw) + 0.5
        shift = torch.randn(Cin, **kw) * 0.5
        mean = torch.randn(Cin, **kw)
        invstd = torch.rand(Cin, **kw) + 0.5
        w = torch.randn(Cout, Cin, 5, 5, **kw) / (Cin * 25) ** 0.5
        dy = torch.rand(B, Cout, H, W, **kw) - 0.3            # like sigmoid(logit) - target: a non-zero mean
        xq, dyq, wq = x.to(dt).double(), dy.to(dt).double(), w.to(dt).double()
        z = xq.float() * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)       # the forward's own fp32 fma ...
        m = (z.to(dt).float() > 0).double()                                       # ... rounded to the storage type, then ReLU
        a = m * (xq * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1))   # scale (m x) + shift m: the activation, unrounded
        dz = m * F.conv_transpose2d(dyq, wq, padding=2)                           # conv_dgrad of a unit-stride conv = conv_transpose
        xhat = (xq - mean.double().view(1, -1, 1, 1)) * invstd.double().view(1, -1, 1, 1)
        red1_ref, red2_ref = dz.sum(dim=(0, 2, 3)), (dz * xhat).sum(dim=(0, 2, 3))
        wr = wq.clone().requires_grad_(True)
        (F.conv2d(a, wr, padding=2) * dyq).sum().backward()
        dw_ref = wr.grad
    d = _lib.ConvDesc(dtype=dtype, use_mfma=1, B=B, H=H, W=W, Cin=Cin, Cout=Cout, R=5, S=5, stride=1, pad=2, transposed=0, mode=0, bn_relu=1)
    scratch = torch.zeros(L.dmm_conv_scratch_bytes(C.byref(d)), dtype=torch.uint8, device=DEV)
    xd, dyd = nhwc(x, dt).to(DEV), nhwc(dy, dt).to(DEV)
    wd, sd, hd = w.to(DEV), scale.to(DEV), torch.cat([shift, mean, invstd]).to(DEV)
    red = torch.full((2 * Cin,), float("nan"), dtype=torch.float64, device=DEV)
    dwd = torch.full((Cout, Cin, 5, 5), float("nan"), device=DEV)
    _lib.impls_since_reset()
    _lib.check(L.dmm_conv5_wgrad_stats(C.byref(d), xd.data_ptr(), dyd.data_ptr(), wd.data_ptr(), sd.data_ptr(), hd.data_ptr(), dwd.data_ptr(),
                                       red.data_ptr(), scratch.data_ptr(), _lib.stream_ptr()))
    torch.cuda.synchronize()
    fam_ok = _check_family(f"conv5 {name}", "wg5")
    rnd = exact == "round"
    bounded = set()
    err = _ndiff if rnd else (_absdiff if exact else relerr)
    res = {"red1": err(red[:Cin].cpu(), red1_ref.cpu()), "red2": err(red[Cin:].cpu(), red2_ref.cpu()),
           "wgrad": err(dwd.cpu(), dw_ref.cpu())}
    if rnd:
        res["red2"] = _ratio(red[Cin:].cpu(), red2_ref, o.red2_bound + o.red2_unc)
        bounded.add("red2")
        if not o.dw_exact:
            res["wgrad"] = _ratio(dwd.cpu(), dw_ref, o.dw_bound)
            bounded.add("wgrad")
    tol = {"red1": 1e-6, "red2": 1e-6, "wgrad": {1: 3e-3, 2: 2.5e-2}[dtype]}
    bad = _verdict(res, exact, tol, bounded)
    print(f"{'FAIL' if bad else 'ok  '} conv5  {name:28s} dt={dtype}{(' round' if rnd else ' exact') if exact else ''} " + _show(res, exact, bounded), flush=True)
    return not bad and fam_ok


def production_forward_case(name, dtype, B, H, W, Cin, Cout, R, stride, pad, bn, transposed=0, reps=3, expect=None):
    """A forward convolution at a PRODUCTION size through the C ABI, several times on identical operands: against torch's GPU
    convolution (fp32 on the same 16-bit-rounded operands) and run to run (bitwise), the BatchNorm statistics of every repetition
    against fp64 sums of its own stored output at the rounding bound of the kernels' fp32 partials.  Timing-dependent hazards of the LDS pipelines
    (a refill landing before a queued fragment read has executed) only show with the chip full; parity-test shapes cannot see them."""
    g = torch.Generator(device=DEV).manual_seed(1)
    dt = {1: torch.float16, 2: torch.bfloat16}[dtype]
    x = torch.randn(B, Cin, H, W, device=DEV, generator=g) * 2 + 0.5
    scale = torch.rand(Cin, device=DEV, generator=g) + 0.5
    shift = torch.randn(Cin, device=DEV, generator=g) * 0.5
    wshape = (Cin, Cout, 3, 3) if transposed else (Cout, Cin, R, R)
    w = torch.randn(wshape, device=DEV, generator=g) / (Cin * R * R) ** 0.5
    xq = x.to(dt).float()
    a = F.relu(xq * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)).to(dt).float() if bn else xq
    wq = w.to(dt).float()
    ref = F.conv_transpose2d(a, wq, stride=2, padding=1, output_padding=1) if transposed else F.conv2d(a, wq, stride=stride, padding=pad)
    d = _lib.ConvDesc(dtype=dtype, use_mfma=1, B=B, H=H, W=W, Cin=Cin, Cout=Cout, R=R, S=R, stride=stride, pad=pad, transposed=transposed,
                      mode=0, bn_relu=bn)
    scratch = torch.zeros(L.dmm_conv_scratch_bytes(C.byref(d)), dtype=torch.uint8, device=DEV)
    xd = x.permute(0, 2, 3, 1).contiguous().to(dt)
    outs, sts = [], []
    ratio = {"sum": 0.0, "sq": 0.0}
    _lib.impls_since_reset()
    for _ in range(reps):
        yd = torch.full((B, ref.shape[2], ref.shape[3], Cout), float("nan"), dtype=dt, device=DEV)
        stats = torch.zeros(2 * Cout, dtype=torch.float64, device=DEV)
        _lib.check(L.dmm_conv_forward(C.byref(d), xd.data_ptr(), w.data_ptr(), scale.data_ptr(), shift.data_ptr(), yd.data_ptr(),
                                      stats.data_ptr(), scratch.data_ptr(), _lib.stream_ptr()))
        torch.cuda.synchronize()
        outs.append(yd.permute(0, 3, 1, 2).float())
        # the statistics against fp64 sums of this repetition's own stored output.  Every forward family adds at most STAT_CHAIN stored
        # values in fp32 (a lane's 16 rows, folded with the other lane half: 32 in pig / conv3 / cf / cvw / cvp and the generic MFMA
        # kernel) before the partial goes to fp64: |stat - ref| <= STAT_CHAIN * 2**-24 * sum |y| per channel (sum y**2 for stat_sq)
        y64 = yd.double()
        mag = {"sum": y64.abs().sum(dim=(0, 1, 2)), "sq": (y64 * y64).sum(dim=(0, 1, 2))}
        want = {"sum": y64.sum(dim=(0, 1, 2)), "sq": mag["sq"]}
        del y64
        for k, got in (("sum", stats[:Cout]), ("sq", stats[Cout:])):
            bound = STAT_CHAIN * 2.0 ** -24 * mag[k]
            # (a channel of zeros has bound 0 and must be met exactly: its ratio is 0 or inf)
            rk = torch.where(bound > 0, (got - want[k]).abs() / bound.clamp_min(1e-300), ((got - want[k]) != 0).double() * float("inf"))
            ratio[k] = max(ratio[k], _maxabs(rk))
        sts.append((stats.clone(), mag))
    top = float(ref.abs().max())
    tol = {1: 3e-3, 2: 2.5e-2}[dtype]
    errs = [float((o - ref).abs().max()) / top for o in outs]
    nbad = [int(((o - ref).abs() > tol * top).sum()) for o in outs]
    ndiff = [int((o != outs[0]).sum()) for o in outs[1:]]
    # run to run the outputs are equal bit for bit.  The statistics are per-workgroup partials added by fp64 atomics in the order the
    # workgroups happen to finish: sums of fp32 values, which fp64 adds without rounding while their span stays below 53 bits - equal
    # bit for bit in every case measured (profiles/r08/exact_parity.txt) - but where a channel's partials span more, two orders may round
    # differently in the last bits: held to 2**-50 of sum |y| (sum y**2) per channel
    sdiff = 0.0
    for st, mag in sts[1:]:
        den = torch.cat([mag["sum"], mag["sq"]]).clamp_min(1e-300)
        sdiff = max(sdiff, _maxabs((st - sts[0][0]).abs() / den))
    stats_ok = max(ratio.values()) <= 1.0 and sdiff <= 2.0 ** -50
    ok = max(errs) < tol and not any(ndiff) and stats_ok and _check_family("production " + name, expect)
    print(f"{'ok  ' if ok else 'FAIL'} production {name:36s} dt={dtype} err " + " ".join(f"{e:.2e}" for e in errs) + f" bad {nbad} run-to-run differing {ndiff}"
          f" stats/bound sum {ratio['sum']:.3g} sq {ratio['sq']:.3g} stats run-to-run {sdiff:.2e}{' (bitwise equal)' if sdiff == 0 else ''}", flush=True)
    return ok


STAT_CHAIN = 128   # the longest fp32 partial of a forward kernel's statistics, in stored values (bound; what the kernels do: 32)


def _maxabs(t):
    """max |t|, infinite if any element is not finite (Python's max() drops a NaN silently)."""
    m = float(t.abs().max())
    return m if m == m else float("inf")


def large_operand_case(name, what, dtype, B, H, W, Cin, Cout, R, pad, transposed=0, mode=0, expect=None, chunk=1):
    """One convolution launch on operands of 4 GiB and more through the C ABI, where the 32-bit-offset families refuse and the fallback
    kernels take over.  backward_case / production_forward_case keep fp32 copies of every operand; here the operands are generated per
    batch chunk directly in 16 bits on the GPU, and the reference - torch fp32 on the GPU on the same rounded operands - runs per chunk:
    forward outputs and data gradients are compared chunk by chunk, weight gradients and the BatchNorm-backward sums are added up over
    the chunks in fp64.  what = "fwd" (dmm_conv_forward), "wgrad" (dmm_conv_wgrad_ex, normal form, materialised gradient), "dgrad"
    (dmm_conv_dgrad_ex, assign).  expect: the exact set of families that must have noted the launch(es).
    For "wgrad" the reference is also measured against itself: the same sum from chunks of twice the size, and fp32 against fp64
    accumulation of the per-chunk results (printed; returned in the result for the test to look at)."""
    dt = {1: torch.float16, 2: torch.bfloat16}[dtype]
    tol = {1: 3e-3, 2: 2.5e-2}[dtype]
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    g = torch.Generator(device=DEV).manual_seed(7)
    kw = dict(generator=g, device=DEV)
    scale = torch.rand(Cin, **kw) + 0.5
    shift = torch.randn(Cin, **kw) * 0.5
    mean = torch.randn(Cin, **kw)
    invstd = torch.rand(Cin, **kw) + 0.5
    wshape = (Cin, Cout, 3, 3) if transposed else (Cout, Cin, R, R)
    w = torch.randn(wshape, **kw) / (Cin * R * R) ** 0.5
    wq = w.to(dt).float()
    up = 2 if (transposed or mode == 1) else 1
    Ho, Wo = H * up, W * up
    x = torch.empty(B, H, W, Cin, dtype=dt, device=DEV)
    for b in range(B):
        x[b] = (torch.randn(H, W, Cin, **kw) * 2 + 0.5).to(dt)
    dy = None
    if what != "fwd":
        dy = torch.empty(B, Ho, Wo, Cout, dtype=dt, device=DEV)
        for b in range(B):
            dy[b] = torch.randn(Ho, Wo, Cout, **kw).to(dt)

    def act(b0, b1):   # relu(bn(x)) of a chunk, NCHW fp32, rounded to the storage type as the kernels hold it
        z = x[b0:b1].permute(0, 3, 1, 2).float() * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
        return z, F.relu(z).to(dt).float()

    def conv(a, wt):
        if transposed:
            return F.conv_transpose2d(a, wt, stride=2, padding=1, output_padding=1)
        if mode == 1:
            return F.conv2d(F.interpolate(a, scale_factor=2, mode="nearest"), wt, padding=pad)
        return F.conv2d(a, wt, padding=pad)

    d = _lib.ConvDesc(dtype=dtype, use_mfma=1, B=B, H=H, W=W, Cin=Cin, Cout=Cout, R=R, S=R, stride=2 if transposed else 1, pad=pad,
                      transposed=transposed, mode=mode, bn_relu=1)
    scratch = torch.zeros(L.dmm_conv_scratch_bytes(C.byref(d)), dtype=torch.uint8, device=DEV)
    hd = torch.cat([shift, mean, invstd])
    st = _lib.stream_ptr()
    res, extra = {}, {}
    _lib.impls_since_reset()
    if what == "fwd":
        yd = torch.full((B, Ho, Wo, Cout), float("nan"), dtype=dt, device=DEV)
        stats = torch.zeros(2 * Cout, dtype=torch.float64, device=DEV)
        _lib.check(L.dmm_conv_forward(C.byref(d), x.data_ptr(), w.data_ptr(), scale.data_ptr(), hd.data_ptr(), yd.data_ptr(), stats.data_ptr(),
                                      scratch.data_ptr(), st))
        torch.cuda.synchronize()
        ran = _lib.impls_since_reset()
        err = top = 0.0
        ssum = torch.zeros(Cout, dtype=torch.float64, device=DEV)
        ssq = torch.zeros(Cout, dtype=torch.float64, device=DEV)
        for b0 in range(0, B, chunk):
            ref = conv(act(b0, b0 + chunk)[1], wq)
            o = yd[b0:b0 + chunk].permute(0, 3, 1, 2).float()
            err = max(err, _maxabs(o - ref))
            top = max(top, float(ref.abs().max()))
            ssum += o.double().sum(dim=(0, 2, 3))
            ssq += (o.double() ** 2).sum(dim=(0, 2, 3))
            del ref, o
        res["fwd"] = err / top
        res["sum"] = relerr(stats[:Cout], ssum)
        res["sq"] = relerr(stats[Cout:], ssq)
    elif what == "wgrad":
        dwd = torch.full(wshape, float("nan"), device=DEV)
        _lib.check(L.dmm_conv_wgrad_ex(C.byref(d), x.data_ptr(), dy.data_ptr(), scale.data_ptr(), hd.data_ptr(), None, None, None, 0,
                                       dwd.data_ptr(), scratch.data_ptr(), st))
        torch.cuda.synchronize()
        ran = _lib.impls_since_reset()

        def ref_sum(ch):
            s64 = torch.zeros(wshape, dtype=torch.float64, device=DEV)
            s32 = torch.zeros(wshape, dtype=torch.float32, device=DEV)
            for b0 in range(0, B, ch):
                wt = wq.clone().requires_grad_(True)
                (conv(act(b0, b0 + ch)[1], wt) * dy[b0:b0 + ch].permute(0, 3, 1, 2).float()).sum().backward()
                s64 += wt.grad.double()
                s32 += wt.grad
            return s64, s32
        ref64, ref32 = ref_sum(chunk)
        alt64, _ = ref_sum(2 * chunk)
        extra["ref_chunkings"] = relerr(alt64, ref64)       # the fp32 reference against itself: another chunking ...
        extra["ref_fp32_accumulation"] = relerr(ref32, ref64)  # ... and fp32 against fp64 accumulation of the chunks
        res["wgrad"] = relerr(dwd, ref64)
    else:
        gxd = torch.full((B, H, W, Cin), float("nan"), dtype=dt, device=DEV)
        red = torch.zeros(2 * Cin, dtype=torch.float64, device=DEV)
        _lib.check(L.dmm_conv_dgrad_ex(C.byref(d), x.data_ptr(), dy.data_ptr(), w.data_ptr(), scale.data_ptr(), hd.data_ptr(), None, None, None,
                                       gxd.data_ptr(), 0, red.data_ptr(), scratch.data_ptr(), st))
        torch.cuda.synchronize()
        ran = _lib.impls_since_reset()
        err = top = 0.0
        r1 = torch.zeros(Cin, dtype=torch.float64, device=DEV)
        r2 = torch.zeros(Cin, dtype=torch.float64, device=DEV)
        for b0 in range(0, B, chunk):
            z, _ = act(b0, b0 + chunk)
            a = F.relu(z).requires_grad_(True)          # (as backward_case: the data gradient does not depend on the activation's rounding)
            (conv(a, wq) * dy[b0:b0 + chunk].permute(0, 3, 1, 2).float()).sum().backward()
            dz = a.grad * (z > 0)
            gx_ref = dz * scale.view(1, -1, 1, 1)
            o = gxd[b0:b0 + chunk].permute(0, 3, 1, 2).float()
            err = max(err, _maxabs(o - gx_ref))
            top = max(top, float(gx_ref.abs().max()))
            xq = x[b0:b0 + chunk].permute(0, 3, 1, 2).double()
            xhat = (xq - mean.double().view(1, -1, 1, 1)) * invstd.double().view(1, -1, 1, 1)
            r1 += dz.double().sum(dim=(0, 2, 3))
            r2 += (dz.double() * xhat).sum(dim=(0, 2, 3))
            del z, a, dz, gx_ref, o, xq, xhat
        res["dgrad"] = err / top
        res["red1"] = relerr(red[:Cin], r1)
        res["red2"] = relerr(red[Cin:], r2)
    fam_ok = expect is None or ran == set(expect)
    if not fam_ok:
        print(f"FAIL {what} {name}: expected kernel families {sorted(expect)}, ran {sorted(ran)}", flush=True)
    peak = torch.cuda.max_memory_allocated() / 2 ** 30
    big = max(x.numel() * 2, (dy.numel() * 2) if dy is not None else 0, Ho * Wo * B * Cout * 2) / 2 ** 30
    bad = [k for k, v in res.items() if not (v < tol)]
    print(f"{'FAIL' if bad else 'ok  '} large {what:5s} {name:30s} dt={dtype} " + " ".join(f"{k}={v:.2e}" for k, v in res.items()) +
          "".join(f" [{k}={v:.2e}]" for k, v in extra.items()) + f" ran={'+'.join(sorted(ran))} largest operand {big:.2f} GiB peak {peak:.1f} GiB", flush=True)
    del x, dy, scratch
    torch.cuda.empty_cache()
    return dict(ok=not bad and fam_ok, res=res, extra=extra, ran=ran, peak_gib=peak, tol=tol)


CASES = exact_operands.CASES   # name, B,H,W,Cin,Cout,R,S,stride,pad, transposed, mode, bn


def run_kernels():
    ok = True
    for dtype in (0, 1):
        for mfma in (0, 1):
            for c in CASES:
                try:
                    ok &= conv_case(c[0], dtype, mfma, *c[1:])
                except Exception:
                    ok = False
                    print(f"EXC  {c[0]} dt={dtype} mfma={mfma}\n" + traceback.format_exc(), flush=True)
    ok &= all([logits_case(exact_operands.logits_id(f, dt, m, off, s), dt, m, *s, expect=f) for f, dt, m, off, s, _ in exact_operands.LOGITS if not off])
    return ok


def run_model(variants=("no", "early", "mid3", "mid2", "mid4"), dtypes=("fp32", "fp16"), mfma=True, loss_scale=None):
    from oracle import restatement as R
    from dmmfods_amd.graphs.models.Dense_U_Net_lidar import Dense_U_Net_lidar
    from dmmfods_amd.utils.Dense_U_Net_lidar_helper import get_config
    V = {"no": (1, 0), "early": (1, 3), "mid2": (2, 3), "mid3": (3, 3), "mid4": (4, 3)}
    ok = True
    for v in variants:
        cbb, s2 = V[v]
        arch = R.Arch(growth_rate=8, block_config=(2, 2, 2, 2), num_init_features=16, concat_before_block_num=cbb,
                      stream_2_in_channels=s2)
        # oracle in fp64 (truth) and fp32 (noise floor)
        outs = {}
        for odt in (torch.float64, torch.float32):
            P = {k: (t.to(odt) if t.is_floating_point() else t.clone()) for k, t in R.make_state(arch, seed=123).items()}
            tr = R.Trainer(arch, P)
            rgb, lidar, tgt = R.make_inputs(arch, 2, 64, 96, seed=0)
            o = tr.step(rgb.to(odt), lidar.to(odt), tgt.to(odt), do_update=False)
            outs[odt] = (o, {k: t.grad.clone() for k, t in tr.leaves}, P)
        o64, g64, P64 = outs[torch.float64]
        o32, g32, _ = outs[torch.float32]
        # fp16-storage emulation (fp64 arithmetic, fp16 rounding where the HIP path stores fp16)
        Ph = {k: (t.double() if t.is_floating_point() else t.clone()) for k, t in R.make_state(arch, seed=123).items()}
        trh = R.Trainer(arch, Ph, storage=torch.float16)
        rgb, lidar, tgt = R.make_inputs(arch, 2, 64, 96, seed=0)
        oh = trh.step(rgb.double(), lidar.double(), tgt.double(), do_update=False)
        gh = {k: t.grad.clone() for k, t in trh.leaves}
        for dts in dtypes:
            try:
                cfg = get_config("/tmp/dmm")
                cfg.model.growth_rate, cfg.model.block_config, cfg.model.num_init_features = 8, (2, 2, 2, 2), 16
                cfg.model.concat_before_block_num, cfg.model.stream_2_in_channels = cbb, s2
                model = Dense_U_Net_lidar(cfg, compute_dtype=dts, use_mfma=mfma, loss_scale=loss_scale)
                model.load_state_dict(R.make_state(arch, seed=123))
                model = model.to(DEV).train()
                rgb, lidar, tgt = R.make_inputs(arch, 2, 64, 96, seed=0)
                logits = model(rgb.to(DEV), lidar.to(DEV))
                met = model.loss_backward(tgt.to(DEV))
                torch.cuda.synchronize()
                if dts == "fp16":  # judge the fp16 build against fp16-storage emulation
                    o64, g64 = oh, gh
                else:
                    o64, g64 = outs[torch.float64][0], outs[torch.float64][1]
                e_log = relerr(logits.detach().cpu(), o64["logits"])
                n_log = relerr(o32["logits"], o64["logits"])
                e_loss = relerr(met["loss_per_class"].cpu(), o64["loss_per_class"])
                iou_ok = torch.allclose(met["iou_per_instance_per_class"].cpu(), o64["iou"].float(), atol=2e-2, equal_nan=True)
                worst = []
                num = den = 0.0
                for k, p in model.named_parameters():
                    ref = g64[k]
                    s = ref.abs().max().clamp_min(1e-30)
                    num += (p.grad.detach().cpu().double() - ref).pow(2).sum().item()
                    den += ref.pow(2).sum().item()
                    e = ((p.grad.detach().cpu().double() - ref).abs().max() / s).item()
                    n = ((g32[k].double() - ref).abs().max() / s).item()
                    worst.append((e, n, k))
                worst.sort(reverse=True)
                sd = model.state_dict()
                e_rm = max(relerr(sd[k].cpu(), P64[k]) for k in sd if k.endswith("running_mean"))
                e_rv = max(relerr(sd[k].cpu(), P64[k]) for k in sd if k.endswith("running_var"))
                tol = 1e-3 if dts == "fp32" else 5e-2
                bad = e_log > tol or worst[0][0] > (3e-3 if dts == "fp32" else 0.2) or not iou_ok
                ok &= not bad
                print(f"{'FAIL' if bad else 'ok  '} model {v:6s} {dts} mfma={int(mfma)} logits={e_log:.2e} (cpu32 {n_log:.1e}) loss={e_loss:.2e} "
                      f"iou_ok={iou_ok} rm={e_rm:.1e} rv={e_rv:.1e} gradL2={(num / den) ** 0.5:.2e} ls={loss_scale}", flush=True)
                for e, n, k in worst[:6]:
                    print(f"        grad err {e:.2e} (cpu32 {n:.1e}) {k}", flush=True)
            except Exception:
                ok = False
                print(f"EXC  model {v} {dts}\n" + traceback.format_exc(), flush=True)
    return ok


if __name__ == "__main__":
    what = sys.argv[1:] or ["kernels", "model"]
    print(torch.cuda.get_device_name(0), flush=True)
    t0 = time.time()
    ok = True
    if "kernels" in what:
        ok &= run_kernels()
    if "model" in what:
        ok &= run_model()
    if "scale" in what:
        for ls in (1.0, 64.0, 4096.0, 1.0 / 64):
            run_model(variants=("no",), dtypes=("fp16",), loss_scale=ls)
        run_model(variants=("no",), dtypes=("fp16",), mfma=False)
    if "model_scalar" in what:
        ok &= run_model(variants=("no",), dtypes=("fp32",), mfma=False)
    print(f"LAB {'PASS' if ok else 'FAIL'} in {time.time() - t0:.1f}s", flush=True)
