"""Transitions over a pooled buffer (plan.cpp: transition_pools): p = avgpool2(relu(bn(x))) is written once by avgpool2_kernel
(pointwise.hip) and the forward and the weight gradient of the transition run as a plain 1x1 layer over p.  p holds, bit for bit, the
operand the generic kernels pool inside their gather, so the two plans of one network - DMM_TRANSITION_POOL_ROWS=0: every transition on
the new path; a huge threshold: none - must agree

  forward   logits, BatchNorm running statistics, every transition output: EQUAL (training and eval mode);
  backward  every gradient but the transitions' conv weights: equal, or - where the old plan is not reproducible from run to run (fp32 /
            fp64 atomics) - within the old plan's own run-to-run difference, with no factor and no allowance: the new plan's tensor is
            no further from the NEAREST of OLD_RUNS runs of the old plan than the two old runs furthest apart are from each other.
            The distance is the max-abs difference, or - for the tensors whose runs differ by single fp32 ulps - the largest
            elementwise difference in units of the last place (_ulpdiff): as a max-abs figure the same one-ulp flip weighs twice as
            much in an element of [128, 256) as in one of [64, 128), and which element flips is chance (seen: 32 old runs 2^-17
            apart, the new run 2^-16 from the nearest - one ulp each); in ulps alone, elements that cancel to nearly zero dominate
            (seen: 8192 against 16384 ulp in a ConvTranspose weight whose max-abs figures agree).  A tensor passes when it lies within
            the old plan's own spread in either unit;
            OLD_RUNS = 32 so that the difference is observed, not supposed.  Measured on MI355X over ten old runs per case
            (profiles/r19/transition_parity.txt section 3): the last ConvTranspose, refine0.weight and the head's norm0 differ in
            every run; the stems' conv0.weight (fp32 atomics of the generic weight gradient) takes 3-7 distinct values one fp32 ulp
            apart, the second stream's with one value in about eight runs of ten - so three, and now and then ten, old runs agree
            bit for bit while the next run, of either plan, does not (seen: ten equal old runs, the new plan one ulp away, in two of
            24 cases).  At 0.8 per run 32 runs all agree in under one case of a thousand.  Everything else is reproducible and
            therefore has to be EQUAL;
  rerouted  the transitions' dW: bit-identical operands in another fp32 summation order.  (a) new against old directly, which pins the
            plan's wiring (operand pointer, pitch, row grid, prologue constants): each element is a sum over the M pooled rows in
            fp32, two orders of it differ by roundings of 2^-24 of the partial sums, so |new - old| <= M * 2^-24 * max |dW| with M
            the largest transition's rows (measured: 0 in every case of 14 runs each);
            (b) each plan's distance from the oracle's evaluation of the network in fp64 arithmetic on 16-bit-stored tensors
            (oracle.restatement.Trainer(storage=...)); the new plan's may be at most 1.5 x the old plan's.  (c) the same 1.5 x for the
            layer alone, through the single-kernel entry points, against fp64 torch on the very operand p both paths multiply.

Every launch of both plans passes the executor's recorded-family check (capi.cpp: launch_checked) - a forward or backward call fails
otherwise.  Measured pairs: profiles/r19/transition_parity.txt."""
import ctypes as C
import re

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
OFF, ON = "1000000000", "0"
OLD_RUNS = 32
TRANSITION_W = re.compile(r"(features|stream_2_features)\.transition\d+\.conv\.weight$")
STORAGE = {"fp16": torch.float16, "bf16": torch.bfloat16}


def _arch(kind):
    from oracle import restatement as R
    return R.Arch(growth_rate=32, block_config=(2, 2, 2), num_init_features=64, concat_before_block_num={"tiny_early": 1, "tiny_mid": 2}[kind],
                  stream_2_in_channels=3)


def _labels(plan, which):
    from dmmfods_amd import _lib
    L = _lib.lib()
    out = []
    for i in range(L.dmm_plan_profile_num_ops(plan.handle, which)):
        label, fl, by = C.c_char_p(), C.c_double(), C.c_double()
        _lib.check(L.dmm_plan_profile_op(plan.handle, which, i, C.byref(label), C.byref(fl), C.byref(by)))
        out.append((label.value or b"").decode())
    return out


def _transition_outputs(plan, labels):
    """{layer: the transition's output as the workspace holds it, raw 16-bit words (B * H * W, N)}"""
    from dmmfods_amd import _lib
    out = {}
    for i, lab in enumerate(labels):
        if not re.search(r"transition\d+\.conv$", lab):
            continue
        off, dims = C.c_int64(), (C.c_int32 * 5)()
        _lib.check(_lib.lib().dmm_plan_record_output(plan.handle, i, C.byref(off), C.byref(dims)))
        B, H, W, N, ld = list(dims)
        words = plan.workspace[off.value: off.value + ((B * H * W - 1) * ld + N) * 2].view(torch.int16)
        out[lab.split("/", 1)[1]] = torch.as_strided(words, (B * H * W, N), (ld, 1)).clone()
    return out


def _run(kind, dtype, B, H, W, rows, monkeypatch):
    """One training step and one eval forward of a fresh model whose plans are built under DMM_TRANSITION_POOL_ROWS=rows."""
    from oracle import restatement as R
    from dmmfods_amd.graphs.models import Dense_U_Net_lidar as M
    from dmmfods_amd.utils.Dense_U_Net_lidar_helper import get_config
    arch = _arch(kind)
    cfg = get_config("/tmp/dmm_test")
    cfg.model.growth_rate, cfg.model.block_config, cfg.model.num_init_features = arch.growth_rate, arch.block_config, arch.num_init_features
    cfg.model.concat_before_block_num, cfg.model.stream_2_in_channels = arch.concat_before_block_num, arch.stream_2_in_channels
    monkeypatch.setenv("DMM_TRANSITION_POOL_ROWS", rows)
    model = M.Dense_U_Net_lidar(cfg, compute_dtype=dtype)
    model.load_state_dict(R.make_state(arch, seed=11))
    model = model.to(DEV).train()
    rgb, lidar, tgt = (t.to(DEV) for t in R.make_inputs(arch, B, H, W, seed=3))
    res = {}
    res["logits"] = model(rgb, lidar).detach().clone()
    plan = model._last[0]
    fwd = _labels(plan, 0)
    res["labels"] = fwd + _labels(plan, 1)
    torch.cuda.synchronize()
    res["transitions"] = _transition_outputs(plan, fwd)
    model.loss_backward(tgt)
    torch.cuda.synchronize()
    res["grads"] = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    res["buffers"] = {k: b.detach().clone() for k, b in model.named_buffers()}
    model.eval()
    with torch.no_grad():
        res["eval_logits"] = model(rgb, lidar).detach().clone()
    torch.cuda.synchronize()
    model.close()
    monkeypatch.delenv("DMM_TRANSITION_POOL_ROWS", raising=False)
    return res


def _maxdiff(a, b):
    return float((a.double() - b.double()).abs().max())


def _ulpdiff(a, b):
    """Largest elementwise |a - b| of two fp32 tensors in units of the last place of the larger of the two elements."""
    _, e = torch.frexp(torch.maximum(a.abs(), b.abs()))      # |x| = m * 2^e, m in [0.5, 1): one ulp is 2^(e - 24)
    return float(((a.double() - b.double()).abs() * torch.pow(2.0, (24 - e).double())).max())


_ORACLE = {}


def _oracle_grads(kind, dtype, B, H, W):
    """The transitions' dW of the network in fp64 arithmetic on tensors stored in `dtype` (computed once per case, never changed)."""
    key = (kind, dtype, B, H, W)
    if key not in _ORACLE:
        from oracle import restatement as R
        arch = _arch(kind)
        P = {k: (t.double() if t.is_floating_point() else t.clone()) for k, t in R.make_state(arch, seed=11).items()}
        tr = R.Trainer(arch, P, storage=STORAGE[dtype])
        rgb, lidar, tgt = R.make_inputs(arch, B, H, W, seed=3)
        tr.step(rgb.double(), lidar.double(), tgt.double(), do_update=False)
        _ORACLE[key] = {k: t.grad.clone() for k, t in tr.leaves if TRANSITION_W.search(k)}
    return _ORACLE[key]


@pytest.mark.parametrize("B,H,W", [(2, 64, 96), (1, 96, 160)], ids=["2x64x96", "1x96x160"])   # pooled rows of transition1: 192; 240 = 128 + a ragged tile
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("kind", ["tiny_early", "tiny_mid"])
def test_both_plans_of_a_network_agree(kind, dtype, B, H, W, monkeypatch):
    old = [_run(kind, dtype, B, H, W, OFF, monkeypatch) for _ in range(OLD_RUNS)]
    new = _run(kind, dtype, B, H, W, ON, monkeypatch)
    ntrans = sum(bool(TRANSITION_W.search(k)) for k in new["grads"])
    assert ntrans == (2 if kind == "tiny_early" else 3)
    # the switch selects the path: one pooling launch per transition and list (training forward only here), none on the old plan
    assert sum(lab.startswith("avgpool2.fwd/") for lab in new["labels"]) == ntrans
    assert not any(lab.startswith("avgpool2.fwd/") for lab in old[0]["labels"])
    assert sum("transition" in lab and lab.split("/")[0].startswith("wgrad.") for lab in new["labels"]) == ntrans
    # ---- forward: equal
    assert torch.equal(new["logits"], old[0]["logits"]), _maxdiff(new["logits"], old[0]["logits"])
    assert torch.equal(new["eval_logits"], old[0]["eval_logits"]), _maxdiff(new["eval_logits"], old[0]["eval_logits"])
    assert new["transitions"].keys() == old[0]["transitions"].keys() and len(new["transitions"]) == ntrans
    for k, t in new["transitions"].items():
        assert torch.equal(t, old[0]["transitions"][k]), k
        assert int(t.count_nonzero()) > t.numel() // 2, k
    for k, b in new["buffers"].items():
        assert torch.equal(b, old[0]["buffers"][k]), (k, _maxdiff(b, old[0]["buffers"][k]))
    # ---- backward, everything but the rerouted weights: equal, or within the old plan's own run-to-run difference
    for k, g in new["grads"].items():
        if TRANSITION_W.search(k) or torch.equal(g, old[0]["grads"][k]):
            continue
        assert g.dtype == torch.float32
        pairs = [(i, j) for i in range(OLD_RUNS) for j in range(i)]
        own = max(_maxdiff(old[i]["grads"][k], old[j]["grads"][k]) for i, j in pairs)
        got = min(_maxdiff(g, o["grads"][k]) for o in old)
        own_u = max(_ulpdiff(old[i]["grads"][k], old[j]["grads"][k]) for i, j in pairs)
        got_u = min(_ulpdiff(g, o["grads"][k]) for o in old)
        print(f"   {kind} {dtype} {B}x{H}x{W} {k}: nearest old run {got:.3e} ({got_u:.1f} ulp), old runs furthest apart {own:.3e} ({own_u:.1f} ulp)")
        assert got <= own or got_u <= own_u, (k, got, own, got_u, own_u)
    # ---- the rerouted weights: new against old, to the order of an fp32 sum over the pooled rows
    rows = B * (H // 8) * (W // 8)        # transition1 pools the stem's H/4 x W/4 map
    for k, g in new["grads"].items():
        if TRANSITION_W.search(k):
            top = float(old[0]["grads"][k].abs().max())
            d = _maxdiff(g, old[0]["grads"][k])
            print(f"   {kind} {dtype} {B}x{H}x{W} {k}: |dW new - old| {d:.3e}, max |dW| {top:.3e}")
            assert top > 0 and d <= rows * 2.0 ** -24 * top, (k, d, top)
    # ---- ... and against fp64 arithmetic on the same stored tensors
    ref = _oracle_grads(kind, dtype, B, H, W)
    assert len(ref) == ntrans
    for k, r in ref.items():
        top = float(r.abs().max())
        assert top > 0
        e_old = _maxdiff(old[0]["grads"][k].cpu(), r) / top
        e_new = _maxdiff(new["grads"][k].cpu(), r) / top
        print(f"   {kind} {dtype} {B}x{H}x{W} {k}: rel err of dW old {e_old:.4e} new {e_new:.4e} ratio {e_new / max(e_old, 1e-300):.3f}")
        assert e_new <= 1.5 * e_old, (k, e_new, e_old)


def _pool(dt, xwin_of, ld, B, H, W, Cc, scale, shift, out, ldo):
    from dmmfods_amd import _lib
    _lib.check(_lib.lib().dmm_avgpool2_bnrelu(dt, xwin_of.data_ptr(), ld, B, H, W, Cc, scale.data_ptr(), shift.data_ptr(), out.data_ptr(), ldo,
                                              _lib.stream_ptr()))
    torch.cuda.synchronize()


@pytest.mark.parametrize("dt,tt", [(0, torch.float32), (1, torch.float16), (2, torch.bfloat16)], ids=["fp32", "fp16", "bf16"])
def test_pooling_kernel_on_a_channel_window_is_the_generic_gather(dt, tt):
    """C = 40 channels at ch0 = 16 of a 72-channel NHWC buffer, 2 x 6 x 10 pixels, written to a window of a 56-channel buffer: against
    dmm_conv_forward in mode 2 (the generic kernel's G_POOL2 gather) with an identity weight, whose output is its operand - bit for bit;
    nothing outside the output window, and nothing of the input, changes."""
    from dmmfods_amd import _lib
    L = _lib.lib()
    B, H, W, Cc, ld, ch0, ldo, och0 = 2, 6, 10, 40, 72, 16, 56, 8
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(B, H, W, ld, generator=g) * 2).to(tt).to(DEV)
    scale = (torch.rand(Cc, generator=g) + 0.5).to(DEV)
    shift = (torch.randn(Cc, generator=g) * 0.7).to(DEV)
    x0 = x.clone()
    out = torch.full((B, H // 2, W // 2, ldo), 7.0, dtype=tt, device=DEV)
    _pool(dt, x[0, 0, 0, ch0:], ld, B, H, W, Cc, scale, shift, out[0, 0, 0, och0:], ldo)
    bits = lambda t: t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)   # noqa: E731
    assert torch.equal(bits(x), bits(x0))
    outside = torch.ones(ldo, dtype=torch.bool)
    outside[och0:och0 + Cc] = False
    assert bool((out[..., outside.to(DEV)] == 7.0).all())
    got = out[..., och0:och0 + Cc].contiguous()
    # the generic path on the window copied out
    d = _lib.ConvDesc(dtype=dt, use_mfma=1, B=B, H=H, W=W, Cin=Cc, Cout=Cc, R=1, S=1, stride=1, pad=0, transposed=0, mode=2, bn_relu=1)
    xw = x[..., ch0:ch0 + Cc].contiguous()
    w = torch.eye(Cc, device=DEV).view(Cc, Cc, 1, 1).contiguous()
    y = torch.zeros(B, H // 2, W // 2, Cc, dtype=tt, device=DEV)
    scratch = torch.zeros(int(L.dmm_conv_scratch_bytes(C.byref(d))), dtype=torch.uint8, device=DEV)
    _lib.check(L.dmm_conv_forward(C.byref(d), xw.data_ptr(), w.data_ptr(), scale.data_ptr(), shift.data_ptr(), y.data_ptr(), None,
                                  scratch.data_ptr(), _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(bits(got), bits(y)), _maxdiff(got, y)
    assert float(got.float().abs().max()) > 0.5 and float((got == 0).float().mean()) < 0.5


@pytest.mark.parametrize("dt,tt", [(1, torch.float16), (2, torch.bfloat16)], ids=["fp16", "bf16"])
@pytest.mark.parametrize("B,H,W,Cin", [(2, 16, 24, 128), (1, 24, 40, 256)], ids=["192rows-128to64", "240rows-256to128"])
def test_transition_layer_weight_gradient_both_paths_against_fp64(dt, tt, B, H, W, Cin):
    """The layer alone: dW from the generic kernel's pooling gather (mode 2) and from the plain one-tap launch over the pooled buffer with
    the identity prologue (scale 1, shift 0), each against fp64 torch on the operand p both multiply; new <= 1.5 x old."""
    from dmmfods_amd import _lib
    L = _lib.lib()
    Cout = Cin // 2
    g = torch.Generator().manual_seed(B * 1000 + Cin)
    x = torch.randn(B, H, W, Cin, generator=g).to(tt).to(DEV)
    dy = torch.randn(B, H // 2, W // 2, Cout, generator=g).to(tt).to(DEV)
    scale = (torch.rand(Cin, generator=g) + 0.5).to(DEV)
    shift = (torch.randn(Cin, generator=g) * 0.5).to(DEV)
    p = torch.zeros(B, H // 2, W // 2, Cin, dtype=tt, device=DEV)
    _pool(dt, x, Cin, B, H, W, Cin, scale, shift, p, Cin)
    ref = torch.einsum("bhwn,bhwk->nk", dy.double().cpu(), p.double().cpu())
    res = {}
    for name, mode, src, h, w, sc, sh in (("old", 2, x, H, W, scale, shift),
                                          ("new", 0, p, H // 2, W // 2, torch.ones(Cin, device=DEV), torch.zeros(Cin, device=DEV))):
        d = _lib.ConvDesc(dtype=dt, use_mfma=1, B=B, H=h, W=w, Cin=Cin, Cout=Cout, R=1, S=1, stride=1, pad=0, transposed=0, mode=mode, bn_relu=1)
        dw = torch.full((Cout, Cin, 1, 1), float("nan"), device=DEV)
        scratch = torch.zeros(int(L.dmm_conv_scratch_bytes(C.byref(d))), dtype=torch.uint8, device=DEV)
        _lib.check(L.dmm_conv_wgrad(C.byref(d), src.data_ptr(), dy.data_ptr(), sc.data_ptr(), sh.data_ptr(), dw.data_ptr(), scratch.data_ptr(),
                                    _lib.stream_ptr()))
        torch.cuda.synchronize()
        res[name] = _maxdiff(dw.view(Cout, Cin).cpu(), ref) / float(ref.abs().max())
    print(f"   layer {B}x{H}x{W} {Cin}->{Cout} dt{dt}: rel err of dW old {res['old']:.4e} new {res['new']:.4e}")
    assert res["new"] <= 1.5 * res["old"], res
