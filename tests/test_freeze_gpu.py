"""Frozen encoder on the GPU: model.freeze_encoder() / requires_grad_ -> dmm_plan_set_encoder_frozen -> a backward list that ends in
front of the encoder, and FusedAdam over the trainable ranges with per-range step counts (one segmented Adam launch, a class per step origin).

THE GRADIENT RULE (_check_frozen_against_default), frozen against default on the same model and batch, per tensor of the arena:
  * encoder tensors (features, stream_2_features, concat_module): all zero (the whole arena is still cleared and no launch of the
    frozen list writes them) - or, with gradient accumulation on, exactly the sentinel the arena was filled with;
  * decoder / head BatchNorm weight and bias gradients: BIT FOR BIT the default path's (the same launches on the same operands) -
    wherever the default path's own two evaluations are bit-equal.  They are on every net but DenseNet-121 in 16-bit storage, where
    the head's norm0 takes part of its sums from the weight gradient's factor correlations (wg5.hip, fp32 atomic adds): that
    tensor differs between two DEFAULT runs already and is held to the convolutions' noise rule instead (MEASURED below);
  * decoder / head convolution gradients: the rule and the measurement procedure of tests/test_accum_gpu.py - d0 = max-abs difference
    of two default-path runs (the order noise of the fp32 atomic adds), max|frozen - default| <= max(4 d0, 2^-21 max|g|).
Every case prints its figures ([freeze] lines).

MEASURED on one MI355X (the tensor with the largest difference / bound; encoder tensors zero and BatchNorm tensors bit-equal in every
case except as noted):
  case                      d0        max|frozen - default|  bound     max|g|  tensor
  fp32 no fusion            1.95e-3   1.95e-3                7.81e-3   3216    h.refine1.weight
  fp32 early, accumulating  1.22e-3   1.71e-3                4.88e-3   3187    h.refine1.weight
  fp32 mid3, accumulating   1.53e-5   3.05e-5                1.19e-4   250     decoder.Transposed_Convolution_4.weight
  fp16 d121 early           3.05e-5   3.05e-5                1.22e-4   186     decoder.Transposed_Convolution_4.weight
  bf16 d121, accumulating   1.53e-5   3.05e-5                8.15e-5   171     decoder.Transposed_Convolution_4.weight
  fp16 mid3 external        1.53e-5   1.53e-5                6.10e-5   116     h.refine0.weight
  fp16 mid3 graph replay    1.53e-5   1.53e-5                6.10e-5   116     h.refine0.weight
The largest difference / bound ratio seen is 0.375.  d121 in fp16 / bf16: dec_out_to_heat_maps.norm0.weight / .bias differ between
two DEFAULT runs by 1.9e-6 / 9.5e-7 .. 1.9e-6 and between frozen and default by 7.2e-7 .. 1.9e-6 (values of order 1): noise rule.
External gradient against loss_backward on the frozen model: relative L2 distance of the arenas 2.4e-5 (bound 2^-10).
Trajectories against torch (bounds 2e-3 / 5e-3): weights 2e-9 .. 2.4e-7 relative L2, running statistics 6e-8 .. 1.3e-7; first
released step: |dp| / lr within 1 % of 1 on 100.00 % of the encoder's elements, plain and guarded."""
import ctypes as C
import math
import os

import pytest
import torch

from dmmfods_amd.utils.Dense_U_Net_lidar_helper import get_config

pytestmark = pytest.mark.gpu

DEV = "cuda"
ENCODER = ("features.", "stream_2_features.", "concat_module.")
TINY = dict(growth_rate=8, block_config=(2, 2, 2, 2), num_init_features=16)
D121 = dict(growth_rate=32, block_config=(6, 12, 24, 16), num_init_features=64)
VARIANTS = {"no": (1, 0), "early": (1, 3), "mid3": (3, 3)}


def _arch(R, base, variant):
    cbb, s2 = VARIANTS[variant]
    return R.Arch(**base, concat_before_block_num=cbb, stream_2_in_channels=s2)


def _model(R, arch, dtype="fp32", seed=123):
    from dmmfods_amd.graphs.models.Dense_U_Net_lidar import Dense_U_Net_lidar
    cfg = get_config("/tmp/dmm_test")
    cfg.model.growth_rate, cfg.model.block_config, cfg.model.num_init_features = arch.growth_rate, arch.block_config, arch.num_init_features
    cfg.model.concat_before_block_num, cfg.model.stream_2_in_channels = arch.concat_before_block_num, arch.stream_2_in_channels
    model = Dense_U_Net_lidar(cfg, compute_dtype=dtype)
    model.load_state_dict(R.make_state(arch, seed=seed))
    return model.to(DEV).train()


def _batch(R, arch, seed, H=64, W=96, B=2):
    return tuple(None if t is None else t.to(DEV) for t in R.make_inputs(arch, B, H, W, seed=seed))


def _fused(model, batch):
    rgb, lidar, tgt = batch
    with torch.no_grad():
        model(rgb, lidar)
    return model.loss_backward(tgt)


def _external(model, batch):
    rgb, lidar, tgt = batch
    logits = model(rgb, lidar)
    logits.backward(gradient=torch.sigmoid(logits.detach()) - tgt)


def _labels(plan, which=1):
    from dmmfods_amd import _lib
    L = _lib.lib()
    out = []
    for i in range(L.dmm_plan_profile_num_ops(plan.handle, which)):
        lab, fl, by = C.c_char_p(), C.c_double(), C.c_double()
        _lib.check(L.dmm_plan_profile_op(plan.handle, which, i, C.byref(lab), C.byref(fl), C.byref(by)))
        out.append(lab.value.decode())
    return out


def _check_frozen_against_default(model, got, want, want_again, tag, sentinel=None):
    """The module docstring's rule: `got` (frozen) against `want` (default), `want_again` the default path's second evaluation."""
    from dmmfods_amd import _lib
    torch.cuda.synchronize()
    assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0, tag
    worst = dict(ratio=-1.0)
    n_enc = n_bn = n_conv = 0
    bn_noisy = []
    for name, kind, shape, off in model._table:
        if kind > _lib.T_BN_BIAS:
            continue
        n = int(math.prod(shape))
        g, w, w2 = got[off:off + n], want[off:off + n], want_again[off:off + n]
        if name.startswith(ENCODER):
            n_enc += 1
            if sentinel is None:
                assert int(torch.count_nonzero(g)) == 0, (tag, name)
            else:
                assert bool((g == sentinel).all()), (tag, name)
            continue
        if sentinel is not None:
            w, w2 = w + sentinel, w2 + sentinel          # accumulation on: the trainable ranges hold sentinel + gradient
        if kind in (_lib.T_BN_WEIGHT, _lib.T_BN_BIAS) and torch.equal(w, w2):
            n_bn += 1
            assert torch.equal(g, w), (tag, name, float((g - w).abs().max()))
            continue
        if kind in (_lib.T_BN_WEIGHT, _lib.T_BN_BIAS):   # the default path itself is not reproducible on this tensor: the noise rule below
            bn_noisy.append((name, float((w - w2).abs().max()), float((g - w).abs().max())))
        n_conv += 1
        d0 = float((w - w2).abs().max())
        bound = max(4 * d0, 2.0 ** -21 * float(w.abs().max()))
        diff = float((g - w).abs().max())
        if diff / bound > worst["ratio"]:
            worst = dict(ratio=diff / bound, name=name, diff=diff, d0=d0, bound=bound, top=float(w.abs().max()))
        assert diff <= bound, (tag, name, dict(diff=diff, d0=d0, bound=bound))
    print(f"[freeze] {tag}: {n_enc} encoder tensors {'zero' if sentinel is None else 'keep the sentinel'}, {n_bn} BatchNorm tensors bit-equal, "
          f"{n_conv} conv (and run-to-run noisy BatchNorm) tensors within the rule, worst {worst}; noisy BatchNorm tensors (name, d0, difference): {bn_noisy}")
    assert n_enc > 0 and n_bn > 0 and n_conv > 0


# ------------------------------------------------------------------------------------------------ 1. gradients
@pytest.mark.parametrize("case", ["fp32-no", "fp32-early", "fp32-mid3", "fp16-d121", "bf16-d121"])
def test_frozen_gradients_equal_the_default_paths(case):
    """Same model, same batch, 2 x 64 x 96: the default backward twice (d0), then frozen.  Also: .grad of frozen parameters is None and
    the others are views of the arena; with accumulation on the encoder ranges keep a sentinel; a bound plan refuses a mode change;
    on DenseNet-121 the frozen list has no wg3 launch and no encoder bw1 launch left (the decoder's own bw1 pair, its last
    conv_reduce, stays as every decoder launch does) and what is left carries the default list's labels (class = kernel
    family + role, which run_ops checks against the family that really took each launch) in the default list's order."""
    from oracle import restatement as R
    from dmmfods_amd import _lib
    dtype, net = case.split("-")
    arch = _arch(R, D121, "early") if net == "d121" else _arch(R, TINY, net)
    model = _model(R, arch, dtype)
    batch = _batch(R, arch, 0)
    _fused(model, batch)
    g1 = model.grad_arena.clone()
    default_labels, default_fwd = _labels(model._last[0]), _labels(model._last[0], 0)
    _fused(model, batch)
    g2 = model.grad_arena.clone()
    params = dict(model.named_parameters())
    assert all(p.grad is not None for p in params.values())

    assert model.freeze_encoder() is model and model.encoder_frozen and not model._plans      # the plans of the other mode are closed
    met = _fused(model, batch)
    gf = model.grad_arena.clone()
    plan = model._last[0]
    assert plan.encoder_frozen and bool(torch.isfinite(met["loss_per_class"]).all())
    assert _lib.lib().dmm_plan_set_encoder_frozen(plan.handle, 0) == _lib.ERR_STATE              # bound: refused
    _check_frozen_against_default(model, gf, g1, g2, case)
    for name, p in params.items():
        if name.startswith(ENCODER):
            assert p.grad is None and not p.requires_grad, name
        else:
            assert p.grad is not None and p.grad.untyped_storage().data_ptr() == model.grad_arena.untyped_storage().data_ptr(), name
    # buckets: trainable tensors only
    spans = [(off, off + int(math.prod(shape))) for name, kind, shape, off in model._table if kind <= _lib.T_BN_BIAS and name.startswith(ENCODER)]
    for off, cnt in model.grad_buckets():
        assert all(hi <= off or off + cnt <= lo for lo, hi in spans)
    # the launch list
    labels = _labels(plan)
    assert len(labels) < len(default_labels)
    core = lambda labs: [x for x in labs if not x.startswith("unpack/")]   # noqa: E731  (one unpack per bucket: fewer buckets)
    assert core(labels) == core(default_labels)[:len(core(labels))]
    assert not any(x.split("/", 1)[-1].startswith(("f.", "s2.", "concat_module", "pool0")) for x in labels)
    if net == "d121":
        assert any(x.startswith("bw1.") for x in default_labels) and any(x.startswith("wg3.") for x in default_labels)
        # every wg3 launch and every bw1 launch but one belongs to the encoder's dense layers; the decoder's last conv_reduce
        # (128 outputs) is a bw1 pair in the default list too, and a decoder launch stays what it was
        assert not any(x.startswith("wg3.") for x in labels)
        left = [x for x in labels if x.startswith("bw1.")]
        assert left == [x for x in default_labels if x.startswith("bw1.") and "/d." in x] and len(left) <= 2, left
    assert _labels(plan, 0) == default_fwd and len(default_fwd) > 10                      # the forward list is the default one
    # accumulation on: the encoder ranges keep what they held
    model.set_grad_accumulation(True)
    model.grad_arena.fill_(0.5)
    _fused(model, batch)
    _check_frozen_against_default(model, model.grad_arena.clone(), g1, g2, case + ", accumulation on", sentinel=0.5)
    model.set_grad_accumulation(False)
    # released again: the default list and the default gradients are back
    model.freeze_encoder(False)
    _fused(model, batch)
    assert _labels(model._last[0]) == default_labels and all(p.grad is not None for p in params.values())
    model.close()


# ------------------------------------------------------------------------------------------------ 2./3. trajectories against torch
def _rel_l2(pairs):
    num = sum(float((a.detach().cpu().double() - b.detach().double()).pow(2).sum()) for a, b in pairs)
    den = sum(float(b.detach().double().pow(2).sum()) for _, b in pairs)
    return (num / den) ** 0.5


def _torch_side(R, arch, frozen):
    P = R.make_state(arch, seed=123)
    leaves = R.leaf_params(P, arch)
    for k, t in leaves:
        t.requires_grad_(not (frozen and k.startswith(ENCODER)))
    opt = torch.optim.Adam([t for _, t in leaves], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, amsgrad=False)
    return P, leaves, opt


def _compare_step(R, arch, P, leaves, ref_opt, model, opt, cpu_batch, step):
    """One optimiser step on both sides; tests/test_accum_gpu.py's three-step bounds: loss sums rtol 2e-3, weights and running
    statistics 5e-3 relative L2."""
    rgb, lidar, tgt = cpu_batch
    ref_opt.zero_grad()
    loss = R.bce_with_logits(R.forward(P, arch, rgb, lidar, training=True), tgt)
    loss.backward(torch.ones_like(loss))
    ref_opt.step()
    met = _fused(model, (rgb.to(DEV), lidar.to(DEV), tgt.to(DEV)))
    opt.step()
    torch.testing.assert_close(met["loss_per_class"].cpu().double(), loss.detach().double().sum(dim=(0, 2, 3)), rtol=2e-3, atol=0)
    sd = model.state_dict()
    e_w = _rel_l2([(sd[k], t) for k, t in leaves])
    e_enc = _rel_l2([(sd[k], t) for k, t in leaves if k.startswith(ENCODER)])
    e_s = _rel_l2([(sd[k], P[k]) for k in sd if k.endswith(("running_mean", "running_var"))])
    print(f"[freeze] step {step}: weights rel L2 {e_w:.3e} (encoder alone {e_enc:.3e}), running statistics rel L2 {e_s:.3e}")
    assert e_w < 5e-3 and e_enc < 5e-3 and e_s < 5e-3, (step, e_w, e_enc, e_s)


def test_three_frozen_steps_against_torch_adam_over_the_decoder_leaves():
    """Tiny mid-3 net, fp32, weight_decay 0.01: three steps with the encoder frozen against the oracle restatement's forward under
    torch.autograd with torch.optim.Adam over the leaves, the encoder's with requires_grad False (torch skips them: no gradient,
    no decay, no state).  Encoder parameters and their moments stay bit-identical; its running statistics keep moving."""
    from oracle import restatement as R
    from dmmfods_amd.optim import FusedAdam
    arch = _arch(R, TINY, "mid3")
    P, leaves, ref_opt = _torch_side(R, arch, frozen=True)
    model = _model(R, arch).freeze_encoder()
    opt = FusedAdam(model, weight_decay=0.01)
    g = torch.Generator().manual_seed(3)
    opt.exp_avg.copy_(torch.randn(opt.exp_avg.shape, generator=g).to(DEV) * 1e-3)          # "loaded" moments everywhere ...
    opt.exp_avg_sq.copy_(torch.rand(opt.exp_avg_sq.shape, generator=g).to(DEV) * 1e-6)
    spans = [(off, off + p.numel()) for (name, p), off in zip(model.named_parameters(), _offsets(model)) if name.startswith(ENCODER)]
    for (name, p), off in zip(model.named_parameters(), _offsets(model)):
        if not name.startswith(ENCODER):                                                   # ... but torch's side starts from zero: clear the trainable ones
            opt.exp_avg[off:off + p.numel()].zero_()
            opt.exp_avg_sq[off:off + p.numel()].zero_()
    p0, m0, v0 = model.param_arena.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone()
    rm0 = model.state_dict()["features.norm0.running_mean"].clone()
    for step in range(3):
        _compare_step(R, arch, P, leaves, ref_opt, model, opt, R.make_inputs(arch, 2, 64, 96, seed=step), step + 1)
    for lo, hi in spans:
        assert torch.equal(model.param_arena[lo:hi], p0[lo:hi]) and torch.equal(opt.exp_avg[lo:hi], m0[lo:hi]) and torch.equal(opt.exp_avg_sq[lo:hi], v0[lo:hi])
    assert not torch.equal(model.param_arena, p0) and opt.step_count == 3
    assert not torch.equal(model.state_dict()["features.norm0.running_mean"], rm0)         # frozen norms still track statistics, as torch's
    assert sorted(opt.state_dict()["state"]) == [i for i, (n, _) in enumerate(model.named_parameters()) if not n.startswith(ENCODER)]
    model.close()


def _offsets(model):
    off, out = 0, []
    for p in model.parameters():
        out.append(off)
        off += p.numel()
    return out


@pytest.mark.parametrize("path", ["plain", "guarded"])
def test_unfreezing_starts_the_encoder_at_its_own_step_one(path):
    """Two frozen steps, release, two more, against the same torch construction with requires_grad flipped on the leaves at the same
    point (torch creates their Adam state then: step 1, zero moments), same bounds.  Plain path and guarded path (max_grad_norm far
    above the norm: nothing is clipped).
    The check that tells a shared step count apart: Adam's FIRST step of a parameter moves it by lr * g / (|g| + eps * sqrt(1 - b2)) -
    lr in magnitude wherever |g| >> 1e-8 - whereas zero moments under the bias corrections of the optimiser's third step give
    lr * (0.1 / (1 - 0.9^3)) / sqrt(0.001 / (1 - 0.999^3)) = 0.64 lr.  So behind the first released step at least 90 % of the
    encoder's elements must have moved by lr to within 1 % (the rest: gradients at eps level, fp32 rounding of p)."""
    from oracle import restatement as R
    from dmmfods_amd.optim import FusedAdam
    arch = _arch(R, TINY, "mid3")
    P, leaves, ref_opt = _torch_side(R, arch, frozen=True)
    model = _model(R, arch).freeze_encoder()
    opt = FusedAdam(model, weight_decay=0.01, max_grad_norm=1e9) if path == "guarded" else FusedAdam(model, weight_decay=0.01)
    enc = torch.zeros(model.param_arena.numel(), dtype=torch.bool, device=DEV)
    for (name, p), off in zip(model.named_parameters(), _offsets(model)):
        if name.startswith(ENCODER):
            enc[off:off + p.numel()] = True
    for step in range(4):
        if step == 2:
            for k, t in leaves:
                t.requires_grad_(True)
            model.freeze_encoder(False)
        before = model.param_arena.clone()
        _compare_step(R, arch, P, leaves, ref_opt, model, opt, R.make_inputs(arch, 2, 64, 96, seed=step), step + 1)
        moved = (model.param_arena - before).abs()
        if step < 2:
            assert float(moved[enc].max()) == 0.0
        if step == 2:
            ratio = moved[enc].double() / 1e-3
            near = float(((ratio - 1.0).abs() < 0.01).double().mean())
            print(f"[freeze] {path}: first released step, |dp| / lr over the encoder: median {float(ratio.median()):.4f}, within 1 % of 1: {near:.4f}")
            assert near >= 0.9, (path, near, float(ratio.median()))
    assert opt.step_count == 4
    assert [r[2] for r in opt.trainable_ranges()] == [2, 0, 2]
    steps = {float(s["step"]) for s in opt.state_dict()["state"].values()}
    assert steps == {2.0, 4.0}
    if path == "guarded":
        assert int(opt.last_found_inf) == 0
    model.close()


# ------------------------------------------------------------------------------------------------ 4. guarded overflow while frozen
def test_guarded_step_sees_the_trainable_ranges_only():
    """An inf planted in an ENCODER range of the arena is not seen by the norm (the step is applied, the reported norm is that of the
    trainable ranges); one inf in a decoder gradient skips the step: nothing is written, the scale backs off once."""
    from oracle import restatement as R
    from dmmfods_amd import _lib
    from dmmfods_amd.optim import DynamicLossScaler, FusedAdam
    arch = _arch(R, TINY, "mid3")
    model = _model(R, arch).freeze_encoder()
    scaler = DynamicLossScaler(init_scale=4.0, growth_interval=10 ** 6)
    opt = FusedAdam(model, weight_decay=0.01, max_grad_norm=1e9, loss_scaler=scaler)
    batch = _batch(R, arch, 0)
    offs = dict(zip((n for n, _ in model.named_parameters()), _offsets(model)))
    (lo, n, t0), = opt.trainable_ranges()
    _fused(model, batch)
    want_norm = float(model.grad_arena[lo:lo + n].double().norm()) / 4.0
    model.grad_arena[offs["features.conv0.weight"] + 5] = float("inf")
    model.grad_arena[offs["concat_module.conv.weight"]] = float("nan")
    p0 = model.param_arena.clone()
    opt.step()
    torch.cuda.synchronize()
    s = _lib.GuardState.from_buffer_copy(scaler._state.cpu().numpy().tobytes())
    assert s.found_inf == 0 and s.applied_steps == 1 and s.skipped_steps == 0 and s.scale == 4.0
    assert abs(s.grad_norm - want_norm) <= 1e-5 * want_norm
    assert torch.equal(model.param_arena[:lo], p0[:lo]) and torch.equal(model.param_arena[lo + n:], p0[lo + n:])
    assert not torch.equal(model.param_arena[lo:lo + n], p0[lo:lo + n]) and bool(torch.isfinite(model.param_arena).all())
    # a decoder gradient overflows
    _fused(model, batch)
    model.grad_arena[offs["decoder.Transposed_Convolution_2.weight"] + 1] = float("inf")
    before = (model.param_arena.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone())
    opt.step()
    torch.cuda.synchronize()
    s = _lib.GuardState.from_buffer_copy(scaler._state.cpu().numpy().tobytes())
    assert s.found_inf == 1 and s.applied_steps == 1 and s.skipped_steps == 1 and s.scale == 2.0 and opt.step_count == 1
    assert torch.equal(model.param_arena, before[0]) and torch.equal(opt.exp_avg, before[1]) and torch.equal(opt.exp_avg_sq, before[2])
    model.close()


# ------------------------------------------------------------------------------------------------ 5. other paths
def test_graph_replay_external_gradient_and_two_plans_on_a_frozen_model():
    """fp16 (K = 48 / 72 / 96 net, mid fusion), every path under the gradient rule:
      * loss_backward() frozen against default (d0 from two default runs) - the reference of what follows;
      * a second plan of another size on the frozen model (both plans frozen, one arena), then the first plan again;
      * the external-gradient path (dmm_plan_backward), frozen against the default model's external-gradient arena, and against the
        frozen loss_backward() arena: torch's sigmoid(x) - t and the loss kernel's d(loss)/d(logit) are both rounded to fp16 storage
        (ulp 2^-11 relative) and may differ there by one ulp on some elements, so that pair is held to a relative L2 distance of 2^-10
        over the arena (two storage ulps; the figure is printed) instead of the bitwise BatchNorm clause;
      * the frozen lists replayed from a captured graph."""
    from oracle import restatement as R
    from dmmfods_amd import _lib
    L = _lib.lib()
    arch = _arch(R, dict(growth_rate=24, block_config=(2, 2, 2, 2), num_init_features=48), "mid3")
    model = _model(R, arch, "fp16", seed=321)
    batch, small = _batch(R, arch, 0), _batch(R, arch, 1, 32, 64)
    arenas = []
    for run in (_fused, _fused, _external, _external):          # the default path: two evaluations of each
        run(model, batch)
        arenas.append(model.grad_arena.clone())
    d1, d2, x1, x2 = arenas
    model.freeze_encoder()
    _fused(model, batch)
    e1 = model.grad_arena.clone()
    _check_frozen_against_default(model, e1, d1, d2, "fp16 mid3, loss_backward")
    # two plans of different sizes on one frozen model: both frozen, one arena
    _fused(model, small)
    assert len(model._plans) == 2 and all(p.encoder_frozen for p in model._plans.values())
    gs = model.grad_arena.clone()
    assert bool(torch.isfinite(gs).all()) and not torch.equal(gs, e1)
    for (name, p), off in zip(model.named_parameters(), _offsets(model)):
        if name.startswith(ENCODER):
            assert int(torch.count_nonzero(gs[off:off + p.numel()])) == 0, name
    _fused(model, batch)
    _check_frozen_against_default(model, model.grad_arena.clone(), d1, d2, "two plans, back on the first")
    # the external-gradient path
    _external(model, batch)
    xf = model.grad_arena.clone()
    _check_frozen_against_default(model, xf, x1, x2, "external gradient, frozen against default")
    dist = float((xf.double() - e1.double()).norm() / e1.double().norm())
    print(f"[freeze] external gradient against loss_backward, frozen: relative L2 distance of the arenas {dist:.3e}")
    assert dist <= 2.0 ** -10
    assert dict(model.named_parameters())["features.conv0.weight"].grad is None
    # graph replay
    try:
        _lib.check(L.dmm_set_option(b"graph", 1))
        model.close()
        for _ in range(3):                                       # eager, capture + replay, replay
            _fused(model, batch)
        plan = model._last[0]
        assert plan.encoder_frozen and L.dmm_plan_num_graph_replays(plan.handle, 1) >= 2
        _check_frozen_against_default(model, model.grad_arena.clone(), d1, d2, "graph replay")
    finally:
        _lib.check(L.dmm_set_option(b"graph", 0))
        model.close()


# ------------------------------------------------------------------------------------------------ 6. the agent
class _Loader:
    """Synthetic training batches (the surface the agent's training loop uses)."""

    def __init__(self, batches):
        self.train_loader, self.train_iterations = batches, len(batches)
        self.valid_loader, self.valid_iterations = [], 0


def _agent(tmp_path, monkeypatch, batches, freeze_epochs, resume=False):
    from dmmfods_amd.agents import Dense_U_Net_lidar_Agent as mod
    from dmmfods_amd.graphs.models.Dense_U_Net_lidar import Dense_U_Net_lidar
    cfg = get_config(str(tmp_path))
    cfg.dir.current_run.summary = str(tmp_path / "run" / "summary")
    cfg.dir.current_run.checkpoints = str(tmp_path / "run" / "checkpoints")
    cfg.model.concat_before_block_num, cfg.model.stream_2_in_channels = 3, 3
    cfg.optimizer.weight_decay = 0.01
    if freeze_epochs is not None:
        cfg.optimizer.freeze_encoder_epochs = freeze_epochs

    def factory(pretrained=False, config=None, compute_dtype=None, **kw):
        config.model.growth_rate, config.model.block_config, config.model.num_init_features = 8, (2, 2, 2, 2), 16
        return Dense_U_Net_lidar(config, compute_dtype=compute_dtype)
    monkeypatch.setattr(mod, "densenet121_u_lidar", factory)
    return mod.Dense_U_Net_lidar_Agent(cfg, torchvision_init=not resume, compute_dtype="fp32", data_loader=_Loader(batches))


def test_agent_freezes_for_the_first_epoch_and_a_resume_continues_in_the_right_phase(tmp_path, monkeypatch):
    """config.optimizer.freeze_encoder_epochs = 1, two epochs of three batches: the encoder's parameters are bit-equal after epoch 0
    and have moved after epoch 1.  A checkpoint written between the epochs (as train() writes it, with the epoch it stands for)
    resumes in the phase of its epoch - a fresh agent that loads it has the encoder released, the optimiser's per-parameter steps
    restored - and epoch 1 of the resumed agent reproduces the uninterrupted run's per-class losses to tests/test_accum_gpu.py's bound
    for loss sums (rtol 2e-3).  Without the field nothing is frozen."""
    from oracle import restatement as R
    arch = _arch(R, TINY, "mid3")
    batches = [R.make_inputs(arch, 2, 64, 96, seed=s) for s in range(3)]
    state = R.make_state(arch, seed=99)
    agent = _agent(tmp_path / "a", monkeypatch, batches, 1)
    agent.model.load_state_dict(state)
    assert agent.freeze_encoder_epochs == 1 and agent.model.encoder_frozen
    enc = [(n, p) for n, p in agent.model.named_parameters() if n.startswith(ENCODER)]
    dec = [(n, p) for n, p in agent.model.named_parameters() if not n.startswith(ENCODER)]
    e0, d0 = [p.detach().clone() for _, p in enc], [p.detach().clone() for _, p in dec]
    agent.current_epoch = 0
    agent.train_one_epoch()
    assert all(torch.equal(p.detach(), q) for (_, p), q in zip(enc, e0)) and not all(torch.equal(p.detach(), q) for (_, p), q in zip(dec, d0))
    assert agent.optimizer.step_count == 3 and agent.model.encoder_frozen
    # the checkpoint of the frozen phase: loads frozen
    agent.save_checkpoint()
    ck_dir = agent.config.dir.current_run.checkpoints
    ck = torch.load(os.path.join(ck_dir, "checkpoint.pth.tar"), map_location="cpu")
    assert len(ck["optimizer"]["state"]) == len(dec)                          # no entries for the encoder
    # ... and the one train() would resume epoch 1 from
    agent.current_epoch = 1
    agent.save_checkpoint(is_best=True)
    agent.train_one_epoch()
    assert not agent.model.encoder_frozen and agent.optimizer.step_count == 6
    assert not any(torch.equal(p.detach(), q) for (_, p), q in zip(enc, e0) if p.numel() > 8)
    assert [r[2] for r in agent.optimizer.trainable_ranges()] == [3, 0, 3]
    want = agent.train_history[1]["loss"]
    agent.model.close()

    # a fresh agent on the frozen-phase checkpoint: phase 0
    os.makedirs(str(tmp_path / "b" / "run" / "checkpoints"), exist_ok=True)
    import shutil
    shutil.copy(os.path.join(ck_dir, "checkpoint.pth.tar"), str(tmp_path / "b" / "run" / "checkpoints" / agent.config.agent.best_checkpoint_name))
    frozen = _agent(tmp_path / "b", monkeypatch, batches, 1, resume=True)
    assert frozen.current_epoch == 0 and frozen.model.encoder_frozen and frozen.optimizer.step_count == 3
    frozen.model.close()
    # ... and on the checkpoint of epoch 1: released, steps restored, the same epoch
    os.makedirs(str(tmp_path / "c" / "run" / "checkpoints"), exist_ok=True)
    shutil.copy(os.path.join(ck_dir, agent.config.agent.best_checkpoint_name), str(tmp_path / "c" / "run" / "checkpoints" / agent.config.agent.best_checkpoint_name))
    resumed = _agent(tmp_path / "c", monkeypatch, batches, 1, resume=True)
    assert resumed.current_epoch == 1 and not resumed.model.encoder_frozen and resumed.optimizer.step_count == 3
    assert [r[2] for r in resumed.optimizer.trainable_ranges()] == [3, 0, 3]
    resumed.train_one_epoch()
    got = resumed.train_history[-1]["loss"]
    print(f"[freeze] agent: epoch 1 losses uninterrupted {want.tolist()} resumed {got.tolist()}")
    torch.testing.assert_close(got.double(), want.double(), rtol=2e-3, atol=0)
    assert resumed.optimizer.step_count == 6
    resumed.model.close()
    # without the field: nothing is frozen
    plain = _agent(tmp_path / "d", monkeypatch, batches, None)
    assert plain.freeze_encoder_epochs == 0 and not plain.model.encoder_frozen and all(p.requires_grad for p in plain.model.parameters())
    plain.model.close()
