"""The guarded optimiser step on the GPU: the arena reduction against torch, the guarded Adam kernel against the plain one and
torch.optim.Adam, clipping against the CPU oracle, the dynamic loss scale through the model, the agent and the external-gradient path,
and the skipped step: nothing changes, nothing leaks.  The device's decisions are replayed against the pure-Python restatement of the
rule in tests/test_guard_cpu.py (GuardRule).

Where a check compares two runs that should compute the same thing, the allowed distance is never a number chosen here: it is twice
the distance of two identical runs of the unguarded path measured in the same test (bit-equality when those two are bit-equal)."""
import ctypes as C
import math
import os

import pytest
import torch

from dmmfods_amd.utils.Dense_U_Net_lidar_helper import get_config
from tests.test_guard_cpu import GuardRule

pytestmark = pytest.mark.gpu

DEV = "cuda"
G3_ARCH = dict(growth_rate=24, block_config=(2, 2, 2, 2), num_init_features=48)   # K = 48 / 72 / 96 channels, a few MB


def _arch(R):
    return R.Arch(**G3_ARCH, concat_before_block_num=3, stream_2_in_channels=3)    # mid fusion before block 3


def _model(R, dtype="fp32", scaler=None):
    from dmmfods_amd.graphs.models.Dense_U_Net_lidar import Dense_U_Net_lidar
    arch = _arch(R)
    cfg = get_config("/tmp/dmm_test")
    cfg.model.growth_rate, cfg.model.block_config, cfg.model.num_init_features = arch.growth_rate, arch.block_config, arch.num_init_features
    cfg.model.concat_before_block_num, cfg.model.stream_2_in_channels = arch.concat_before_block_num, arch.stream_2_in_channels
    model = Dense_U_Net_lidar(cfg, compute_dtype=dtype)
    model.load_state_dict(R.make_state(arch, seed=321))
    model = model.to(DEV).train()
    if scaler is not None:
        model.set_loss_scaler(scaler)
    return model


def _inputs(R, seed, H=64, W=96):
    return tuple(t.to(DEV) for t in R.make_inputs(_arch(R), 2, H, W, seed=seed))


def _fwd_bwd(model, rgb, lidar, tgt):
    with torch.no_grad():
        model(rgb, lidar)
    return model.loss_backward(tgt)


def _dist(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def _state_of(block):
    """The 64-byte device block as a ctypes dmm_guard_state (waits for the GPU)."""
    from dmmfods_amd import _lib
    return _lib.GuardState.from_buffer_copy(block.cpu().numpy().tobytes())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class _Raw:
    """dmm_adam_step_guarded on bare tensors: a state block, the scratch, and the call."""

    def __init__(self, n, scale=1.0, applied=0):
        from dmmfods_amd import _lib
        self.lib, self.L = _lib, _lib.lib()
        self.block = torch.zeros(16, dtype=torch.int32, device=DEV)
        self.scratch = torch.zeros(self.L.dmm_grad_guard_scratch_bytes(n) // 8, dtype=torch.float64, device=DEV)
        self.lib.check(self.L.dmm_guard_state_init(self.block.data_ptr(), scale, applied, 0, _stream()))

    def step(self, p, g, m, v, lr=1e-3, max_norm=0.0, growth=2.0, backoff=0.5, interval=0):
        self.lib.check(self.L.dmm_adam_step_guarded(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), lr, 0.9, 0.999, 1e-8, 0.0,
                                                    max_norm, growth, backoff, interval, self.block.data_ptr(), self.scratch.data_ptr(), _stream()))
        return _state_of(self.block)


# ------------------------------------------------------------------------------------------------ 5. the reduction
@pytest.mark.parametrize("n", [1, 255, (1 << 20) + 3, 23567564])
def test_arena_reduction_against_torch(n):
    """sumsq of the whole guarded step against arena.double().pow(2).sum().  Bound: relative error <= n * 2^-53 - the worst case of ANY
    summation order of n non-negative fp64 terms whose squares are exact; nothing is measured into it.  Two runs are bit-equal (no
    floating-point atomics).  One inf / -inf / NaN anywhere sets the flag and the step writes nothing; 3e38 everywhere does not."""
    g = torch.Generator(device=DEV).manual_seed(1234 + n % 1000)
    arena = torch.randn(n, generator=g, device=DEV)
    p0 = torch.randn(n, generator=g, device=DEV)
    p, m, v = p0.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    want = arena.double().pow(2).sum().item()
    s1 = _Raw(n).step(p, arena, m, v)
    s2 = _Raw(n).step(p, arena, m, v)
    rel = abs(s1.sumsq - want) / want
    print(f"n={n}: sumsq {s1.sumsq!r} torch {want!r} rel err {rel:.3e} bound {n * 2.0 ** -53:.3e}")
    assert s1.found_inf == 0 and s1.applied_steps == 1 and s1.skipped_steps == 0
    assert rel <= n * 2.0 ** -53
    assert s1.sumsq == s2.sumsq and math.copysign(1.0, s1.sumsq) == 1.0            # bit-equal run to run
    assert abs(s1.grad_norm - math.sqrt(want)) <= 2.0 ** -23 * math.sqrt(want)
    assert not torch.equal(p, p0)                                                  # the step was applied
    # the reduction alone, on two sub-ranges with an odd split (neither starts on a 16-byte boundary), accumulating: same bound
    from dmmfods_amd import _lib
    L = _lib.lib()
    if n > 8:
        scratch = torch.full((L.dmm_grad_guard_scratch_bytes(n) // 8,), 7.0, dtype=torch.float64, device=DEV)
        cut = n // 3 | 1
        _lib.check(L.dmm_grad_sumsq(arena.data_ptr(), 1, cut - 1, 0, scratch.data_ptr(), _stream()))
        _lib.check(L.dmm_grad_sumsq(arena.data_ptr(), cut, n - cut, 1, scratch.data_ptr(), _stream()))
        want1 = arena[1:].double().pow(2).sum().item()
        got1 = scratch.sum().item()
        assert abs(got1 - want1) / want1 <= n * 2.0 ** -53, (got1, want1)
    # non-finite values are found wherever they sit, and a skipped step leaves params and moments bit-equal
    for where in sorted({0, n // 2, n - 1}):
        for bad in (float("inf"), float("-inf"), float("nan")):
            a = arena.clone()
            a[where] = bad
            pp, mm, vv = p0.clone(), torch.full((n,), 0.5, device=DEV), torch.full((n,), 0.25, device=DEV)
            s = _Raw(n, scale=8.0, applied=3).step(pp, a, mm, vv)
            assert s.found_inf == 1 and s.skipped_steps == 1 and s.applied_steps == 3 and s.scale == 4.0, (where, bad, s.found_inf)
            assert not math.isfinite(s.sumsq)
            assert torch.equal(pp, p0) and bool((mm == 0.5).all()) and bool((vv == 0.25).all())
    big = torch.full((n,), 3e38, device=DEV)
    s = _Raw(n).step(p0.clone(), big, torch.zeros(n, device=DEV), torch.zeros(n, device=DEV))
    assert s.found_inf == 0 and math.isfinite(s.sumsq) and s.applied_steps == 1


# ------------------------------------------------------------------------------------------------ 6. the Adam kernel
def test_guarded_step_equals_plain_step_when_nothing_intervenes():
    """No clipping, S = 1, growth_interval 0, 5 steps on seeded gradients: dmm_adam_step_guarded against the plain dmm_adam_step (moments
    bit-equal after every step: they do not depend on the bias corrections; parameters may differ through the last bit of step_size and
    bc2_sqrt - fp64 pow on the device vs on the host -: |dp| <= k * (2^-20 * lr + 2^-23 * |p|) after k steps) and against torch.optim.Adam
    on the CPU, where the plain kernel's own distance to torch is the yardstick: the guarded kernel may be at most twice as far."""
    from dmmfods_amd import _lib
    L = _lib.lib()
    n, lr = (1 << 20) + 3, 1e-3
    gen = torch.Generator().manual_seed(99)
    p0 = torch.randn(n, generator=gen)
    grads = [torch.randn(n, generator=gen) * (0.1 + k) for k in range(5)]
    pg, mg, vg = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    pp, mp, vp = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    pt = torch.nn.Parameter(p0.clone())
    ref = torch.optim.Adam([pt], lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False)
    raw = _Raw(n)
    for k, g in enumerate(grads, 1):
        gd = g.to(DEV)
        s = raw.step(pg, gd, mg, vg, lr=lr)
        _lib.check(L.dmm_adam_step(pp.data_ptr(), gd.data_ptr(), mp.data_ptr(), vp.data_ptr(), n, lr, 0.9, 0.999, 1e-8, 0.0, k, 1.0, _stream()))
        pt.grad = g.clone()
        ref.step()
        torch.cuda.synchronize()
        assert s.found_inf == 0 and s.applied_steps == k and s.scale == 1.0 and s.grad_scale == 1.0 and s.clip_coef == 1.0
        assert torch.equal(mg, mp) and torch.equal(vg, vp), k
        bound = k * (2.0 ** -20 * lr + 2.0 ** -23 * pp.abs())
        assert bool(((pg - pp).abs() <= bound).all()), (k, float((pg - pp).abs().max()))
        d_plain = float((pp.cpu() - pt.detach()).abs().max())
        d_guard = float((pg.cpu() - pt.detach()).abs().max())
        print(f"step {k}: max |p - torch| plain {d_plain:.3e} guarded {d_guard:.3e}; max |guarded - plain| {float((pg - pp).abs().max()):.3e}")
        assert d_guard <= 2 * d_plain, (k, d_guard, d_plain)


# ------------------------------------------------------------------------------------------------ 7. clipping
@pytest.mark.parametrize("active", [True, False])
def test_clipping_against_the_oracle(active):
    """fp32 model.  Oracle: backward, torch.nn.utils.clip_grad_norm_, Adam on the CPU; here: forward, loss_backward, the guarded step with
    the same max_norm = half of torch's norm of the oracle's gradients (clipping active) or 10 x that norm (coef = 1).  Parameters after
    the step: the bounds of test_adam_steps_follow_oracle (tests/test_model_gpu.py), scaled from two steps to one.  The reported norm
    cannot be further from the oracle's than the gradient arena is from the oracle's gradients (relative L2, computed here; the arena
    itself is held to test_model_gpu.py's fp32 gradient bound): asserted as that inequality."""
    from oracle import restatement as R
    from dmmfods_amd.optim import FusedAdam
    arch = _arch(R)
    rgb, lidar, tgt = R.make_inputs(arch, 2, 64, 96, seed=7)
    tr = R.Trainer(arch, R.make_state(arch, seed=321))
    tr.step(rgb, lidar, tgt, do_update=False)
    leaves = [t for _, t in tr.leaves]
    g_or = {k: t.grad.detach().clone() for k, t in tr.leaves}
    norm_or = float(torch.nn.utils.clip_grad_norm_(leaves, 1e30))          # torch's norm; coef clamps to 1: gradients unchanged
    max_norm = 0.5 * norm_or if active else 10.0 * norm_or
    torch.nn.utils.clip_grad_norm_(leaves, max_norm)
    tr.opt.step()
    # fp64 oracle and the fp32 oracle's own noise, for the arena's bound
    P64 = {k: (t.double() if t.is_floating_point() else t.clone()) for k, t in R.make_state(arch, seed=321).items()}
    tr64 = R.Trainer(arch, P64)
    tr64.step(rgb.double(), lidar.double(), tgt.double(), do_update=False)
    g64 = {k: t.grad.detach().clone() for k, t in tr64.leaves}

    model = _model(R)
    opt = FusedAdam(model, max_grad_norm=max_norm)
    _fwd_bwd(model, rgb.to(DEV), lidar.to(DEV), tgt.to(DEV))
    grads = {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters()}
    opt.step()
    torch.cuda.synchronize()
    s = _state_of(opt._guard._state)
    num = den = 0.0
    for k, g in grads.items():
        refg = g64[k]
        sc = refg.abs().max().clamp_min(1e-30)
        err = ((g.double() - refg).abs().max() / sc).item()
        noise = ((g_or[k].double() - refg).abs().max() / sc).item()
        assert err < max(3e-3, 4 * noise), (k, err, noise)
        num += (g.double() - g_or[k].double()).pow(2).sum().item()
        den += g_or[k].double().pow(2).sum().item()
    arena_dist = math.sqrt(num / den)
    norm_err = abs(s.grad_norm - norm_or) / norm_or
    want_coef = min(1.0, max_norm / (s.grad_norm + 1e-6))
    print(f"clipping active={active}: norm device {s.grad_norm!r} oracle {norm_or!r} rel {norm_err:.3e}; arena rel L2 to the oracle {arena_dist:.3e}; "
          f"coef device {s.clip_coef!r} from the reported norm {want_coef!r}")
    assert s.found_inf == 0 and s.applied_steps == 1 and opt.step_count == 1
    assert norm_err <= arena_dist
    assert abs(s.clip_coef - want_coef) <= 3 * 2.0 ** -24 * want_coef
    assert (s.clip_coef < 0.51) if active else (s.clip_coef == 1.0)
    assert abs(float(opt.last_grad_norm) - s.grad_norm) == 0 and int(opt.last_found_inf) == 0 and float(opt.loss_scale) == 1.0
    sd = model.state_dict()
    bad = tot = 0
    for k, refp in tr.leaves:
        d = (sd[k].cpu() - refp.detach()).abs()
        assert d.max() <= 1 * 2e-3 + 1e-4, k          # at most a sign flip of a noise-level gradient in the one step
        bad += int((d > 1e-4).sum())
        tot += d.numel()
    print(f"  parameters: {bad} of {tot} further than 1e-4 from the oracle's")
    assert bad / tot < 0.05


# ------------------------------------------------------------------------------------------------ 8. a power of two is exact
def _three_steps(R, scaler):
    from dmmfods_amd.optim import FusedAdam
    model = _model(R)
    opt = FusedAdam(model, loss_scaler=scaler)
    out = []
    for step in range(3):
        _fwd_bwd(model, *_inputs(R, step))
        out.append(model.grad_arena.clone())
        opt.step()
        out.append(model.param_arena.clone())
    torch.cuda.synchronize()
    model.close()
    return out


def _allowed(base_a, base_b, what):
    """Twice the distance of two identical runs of the unguarded path, entry by entry (0 = bit-equality is required)."""
    d0 = [_dist(a, b) for a, b in zip(base_a, base_b)]
    print(f"{what}: run-to-run distance of the unguarded path {['%.2e' % d for d in d0]}")
    return [2 * d for d in d0]


def test_power_of_two_scale_changes_nothing_in_fp32():
    """fp32 model, scaler fixed at 2^10 against no scaler, 3 steps.  Scaling by a power of two is exact in fp32 away from overflow and
    underflow, so the two may differ only by what two identical unscaled runs differ by (measured first; x 2)."""
    from oracle import restatement as R
    from dmmfods_amd.optim import DynamicLossScaler
    a, b = _three_steps(R, None), _three_steps(R, None)
    lim = _allowed(a, b, "pow2 scale")
    scaler = DynamicLossScaler(init_scale=2.0 ** 10, growth_interval=0)
    c = _three_steps(R, scaler)
    assert scaler.get_scale() == 2.0 ** 10 and scaler.skipped_steps == 0
    got = []
    for i, (x, y) in enumerate(zip(c, a)):
        x = x / 2.0 ** 10 if i % 2 == 0 else x      # even entries: the gradient arena as stored (scaled)
        got.append(_dist(x, y))
    print("pow2 scale: scaled run vs unscaled run", ["%.2e" % d for d in got])
    for i, (d, l) in enumerate(zip(got, lim)):
        assert d <= l, (i, d, l)


# ------------------------------------------------------------------------------------------------ 9. overflow
def test_overflow_is_caught_the_step_is_skipped_and_nothing_leaks():
    """fp16 model, init_scale 2^24, growth_interval 4, 64 steps.  At 2^24 nearly every loss-gradient element exceeds fp16's 65504, so the
    first step MUST be skipped.  At every step torch.isfinite(grad_arena).all(), computed here, is the independent oracle: the device
    flag equals it; a skipped step leaves params, exp_avg, exp_avg_sq bit-equal and the applied counter unchanged; the scale follows
    the Python rule replayed from the flags; parameters stay finite.  Not vacuous: >= 1 skip, >= 1 growth, >= 24 applied steps (scale 1
    is feasible for this network - test_fp16_training_trajectory_tracks_fp32_oracle - so at most 24 halvings are needed, after which
    at worst one step in five is skipped)."""
    from oracle import restatement as R
    from dmmfods_amd.optim import DynamicLossScaler, FusedAdam
    scaler = DynamicLossScaler(init_scale=2.0 ** 24, growth_interval=4)
    model = _model(R, "fp16")
    opt = FusedAdam(model, loss_scaler=scaler)
    rule = GuardRule(scale=2.0 ** 24, growth_interval=4)
    grew, trace = 0, []
    for step in range(64):
        _fwd_bwd(model, *_inputs(R, step))
        assert float(scaler.loss_scale) == float(rule.scale), step
        finite = bool(torch.isfinite(model.grad_arena).all())
        before = (model.param_arena.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone())
        applied_before, scale_before = rule.applied, float(rule.scale)
        opt.step()
        s = _state_of(scaler._state)
        assert bool(s.found_inf) == (not finite), (step, s.found_inf, finite)
        assert int(opt.last_found_inf) == s.found_inf
        rule.step(not finite)
        if not finite:
            assert torch.equal(model.param_arena, before[0]) and torch.equal(opt.exp_avg, before[1]) and torch.equal(opt.exp_avg_sq, before[2]), step
            assert s.applied_steps == applied_before
        else:
            assert not torch.equal(model.param_arena, before[0]), step
            assert s.grad_scale == 1.0 / scale_before and math.isfinite(s.grad_norm)
        assert (s.scale, s.applied_steps, s.skipped_steps, s.growth_tracker) == (float(rule.scale), rule.applied, rule.skipped, rule.tracker), step
        assert bool(torch.isfinite(model.param_arena).all()), step
        grew += float(rule.scale) > scale_before
        trace.append(("+" if finite else "-") + str(int(math.log2(scale_before))))
        if step == 0:
            assert not finite, "a finite gradient arena at scale 2^24: some store of the fp16 backward saturates instead of overflowing"
    print("overflow trace (+ applied / - skipped, log2 scale):", " ".join(trace))
    assert rule.skipped >= 1 and grew >= 1 and rule.applied >= 24, (rule.skipped, grew, rule.applied)
    assert opt.step_count == rule.applied and scaler.skipped_steps == rule.skipped and scaler.get_scale() == float(rule.scale)


# ------------------------------------------------------------------------------------------------ 10. no trace in the workspace
def _skip_sequence(R, scaler, overflow_at_step_1):
    """Step 0 normal; step 1 either a backward at scale 2^24 whose step is skipped, or the training forward alone (which updates the
    running statistics all the same); step 2 normal.  Returns step 2's gradient arena."""
    from dmmfods_amd.optim import FusedAdam
    model = _model(R, "fp16")
    opt = FusedAdam(model, loss_scaler=scaler)
    _fwd_bwd(model, *_inputs(R, 0))
    opt.step()
    rgb, lidar, tgt = _inputs(R, 1)
    if overflow_at_step_1:
        scaler.set_scale(2.0 ** 24)
        _fwd_bwd(model, rgb, lidar, tgt)
        opt.step()
        assert int(opt.last_found_inf) == 1 and scaler.get_scale() == 2.0 ** 23 and opt.step_count == 1
        scaler.set_scale(1.0)
    else:
        with torch.no_grad():
            model(rgb, lidar)
    _fwd_bwd(model, *_inputs(R, 2))
    g = model.grad_arena.clone()
    torch.cuda.synchronize()
    model.close()
    return g


def test_a_skipped_step_leaves_no_trace_in_the_workspace():
    """No 0 x inf = NaN survives in a padding lane or in an accumulator the next backward assumes to be zero: after a skipped step the
    next step's gradients equal those of a run whose step 1 did no backward at all, within twice the run-to-run distance of the
    unguarded path, and are finite."""
    from oracle import restatement as R
    from dmmfods_amd.optim import DynamicLossScaler
    base = [_skip_sequence(R, None, False) for _ in range(2)]
    lim = _allowed([base[0]], [base[1]], "skipped step")[0]
    fixed = lambda: DynamicLossScaler(init_scale=1.0, growth_interval=0)   # noqa: E731 - scale 1 is feasible for this network
    a = _skip_sequence(R, fixed(), True)
    b = _skip_sequence(R, fixed(), False)
    d = _dist(a, b)
    print(f"skipped step: step-2 gradients with vs without the overflowing backward at step 1: {d:.3e} (allowed {lim:.3e})")
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all())
    assert d <= lim


# ------------------------------------------------------------------------------------------------ 11. trajectory
def test_fp16_trajectory_with_a_dynamic_scale_tracks_the_oracle():
    """fp16 model with DynamicLossScaler(init_scale=2^16, growth_interval=2000) through the agent-style loop for 5 APPLIED steps against
    oracle.Trainer: per-step loss sums within 1e-2 relative, the bound of test_fp16_training_trajectory_tracks_fp32_oracle."""
    from oracle import restatement as R
    from dmmfods_amd.optim import DynamicLossScaler, FusedAdam
    arch = _arch(R)
    tr = R.Trainer(arch, R.make_state(arch, seed=321))
    scaler = DynamicLossScaler(init_scale=2.0 ** 16, growth_interval=2000)
    model = _model(R, "fp16")
    opt = FusedAdam(model, loss_scaler=scaler)
    devs, attempts = [], 0
    for k in range(5):
        rgb, lidar, tgt = R.make_inputs(arch, 2, 64, 96, seed=k)
        ref = tr.step(rgb, lidar, tgt)
        while True:     # a skipped step is repeated on the same batch at the smaller scale
            attempts += 1
            assert attempts <= 5 + 17, "the scale fell below 1/2 without an applied step"
            met = _fwd_bwd(model, rgb.to(DEV), lidar.to(DEV), tgt.to(DEV))
            opt.step()
            if int(opt.last_found_inf) == 0:
                break
        got, want = met["loss_per_class"].double().cpu(), ref["loss_per_class"].double()
        devs.append(((got - want).abs() / want.abs()).max().item())
    print("fp16 + dynamic scale: per-step max rel loss deviation", ["%.2e" % d for d in devs], f"scale now {scaler.get_scale():g}, skipped {scaler.skipped_steps}")
    assert opt.step_count == 5 and scaler.skipped_steps == attempts - 5
    assert max(devs) < 1e-2, devs


# ------------------------------------------------------------------------------------------------ 12. model and agent surface
def test_every_plan_of_the_model_sees_the_scale_and_detaching_restores_the_plain_path():
    from oracle import restatement as R
    from dmmfods_amd.optim import DynamicLossScaler

    def grads(model, size):
        _fwd_bwd(model, *_inputs(R, 3, *size))
        return model.grad_arena.clone()

    def fresh(size):
        m = _model(R)
        g = grads(m, size)
        torch.cuda.synchronize()
        m.close()
        return g
    sizes = [(64, 96), (64, 64)]
    plain = [[fresh(s) for s in sizes] for _ in range(2)]
    lim = _allowed(plain[0], plain[1], "plans")
    scaler = DynamicLossScaler(init_scale=2.0 ** 6, growth_interval=0)
    model = _model(R, scaler=scaler)
    first = grads(model, sizes[0])
    second = grads(model, sizes[1])        # a plan created AFTER set_loss_scaler
    assert len(model._plans) == 2 and all(p.scaler_ptr == scaler._state.data_ptr() for p in model._plans.values())
    d = [_dist(first / 64.0, plain[0][0]), _dist(second / 64.0, plain[0][1])]
    print("plans: scaled / 64 vs the plain model", ["%.2e" % x for x in d])
    assert d[0] <= lim[0] and d[1] <= lim[1]
    scaler.set_scale(2.0 ** 3)             # read from device memory when the kernel runs: no plan is rebuilt
    assert _dist(grads(model, sizes[1]) / 8.0, plain[0][1]) <= lim[1]
    model.set_loss_scaler(None)
    assert all(p.scaler_ptr is None for p in model._plans.values())
    off = [grads(model, s) for s in sizes]
    d = [_dist(off[0], plain[0][0]), _dist(off[1], plain[0][1])]
    print("plans: after set_loss_scaler(None) vs the plain model", ["%.2e" % x for x in d])
    assert d[0] <= lim[0] and d[1] <= lim[1]
    met = _fwd_bwd(model, *_inputs(R, 3))
    model.set_loss_scaler(scaler)
    met_s = _fwd_bwd(model, *_inputs(R, 3))
    # the loss sums never see the scale (8 here: a scaled sum would be 7 away; two forwards of one model agree far below 1e-3)
    assert _dist(met_s["loss_per_class"], met["loss_per_class"]) <= 1e-3


def _agent_cfg(tmp_path):
    cfg = get_config(str(tmp_path))
    cfg.dir.data.root = str(tmp_path / "data")
    cfg.dir.data.file_lists = str(tmp_path / "lists")
    cfg.dir.current_run.summary = str(tmp_path / "run" / "summary")
    cfg.dir.current_run.checkpoints = str(tmp_path / "run" / "checkpoints")
    cfg.loader.num_workers = 0
    cfg.loader.pin_memory = False
    g = torch.Generator().manual_seed(0)
    for mode in ("train", "val"):
        d = os.path.join(cfg.dir.data.root, mode, "part0")
        os.makedirs(os.path.join(d, "labels"), exist_ok=True)
        for i in range(2):
            t = torch.rand(2, 7, 64, 96, generator=g)
            t[:, :4] *= 255
            t[:, 4:] = (t[:, 4:] > 0.9).float()
            torch.save(t, os.path.join(d, f"batch_{i}.pt"))
    return cfg


def test_agent_trains_with_the_guard_checkpoints_and_resumes(tmp_path):
    from dmmfods_amd.agents.Dense_U_Net_lidar_Agent import Dense_U_Net_lidar_Agent
    from dmmfods_amd.optim import DynamicLossScaler
    cfg = _agent_cfg(tmp_path)
    cfg.agent.max_epoch = 2
    scaler = DynamicLossScaler(init_scale=2.0 ** 24, growth_interval=2000)      # the first step(s) overflow in fp16
    agent = Dense_U_Net_lidar_Agent(cfg, compute_dtype="fp16", max_grad_norm=50.0, loss_scaler=scaler)
    assert agent.optimizer.max_grad_norm == 50.0 and agent.optimizer.loss_scaler is scaler and agent.model._loss_scaler is scaler
    agent.run()
    agent.finalize()
    assert agent.current_train_iteration == 4 and len(agent.train_history) == 2
    skipped = scaler.skipped_steps
    assert all({"loss_scale", "skipped_steps"} <= set(h) for h in agent.train_history)
    assert sum(h["skipped_steps"] for h in agent.train_history) == skipped >= 1
    assert agent.train_history[-1]["loss_scale"] == scaler.get_scale() == 2.0 ** (24 - skipped)
    assert agent.optimizer.step_count == 4 - skipped
    assert bool(torch.isfinite(agent.model.param_arena).all())
    agent.save_checkpoint()
    ck_dir = cfg.dir.current_run.checkpoints
    ck = torch.load(os.path.join(ck_dir, "checkpoint.pth.tar"), map_location="cpu")
    assert set(ck) == {"epoch", "train_iteration", "val_iteration", "best_val_iou", "state_dict", "optimizer"}     # the reference's keys
    assert ck["optimizer"]["loss_scaler"] == {"scale": scaler.get_scale(), "growth_tracker": scaler.growth_tracker, "skipped_steps": skipped}
    os.replace(os.path.join(ck_dir, "checkpoint.pth.tar"), os.path.join(ck_dir, cfg.agent.best_checkpoint_name))
    cfg.optimizer.max_grad_norm = 50.0            # this time from the config (fields the reference's create_config does not have)
    cfg.optimizer.dynamic_loss_scale = True
    agent2 = Dense_U_Net_lidar_Agent(cfg, torchvision_init=False, compute_dtype="fp16")
    s2 = agent2.loss_scaler
    assert s2 is not None and s2 is not scaler and agent2.optimizer.max_grad_norm == 50.0
    assert s2.get_scale() == scaler.get_scale() and s2.skipped_steps == skipped and s2.growth_tracker == scaler.growth_tracker
    assert agent2.optimizer.step_count == 4 - skipped
    torch.testing.assert_close(agent2.optimizer.exp_avg.cpu(), agent.optimizer.exp_avg.cpu(), rtol=0, atol=0)
    # ... and it goes on from there: one more epoch, counters continue
    agent2.config.agent.max_epoch = agent2.current_epoch + 1
    agent2.train_one_epoch()
    assert agent2.optimizer.step_count + s2.skipped_steps == 6 and agent2.train_history[-1]["loss_scale"] == s2.get_scale()


# ------------------------------------------------------------------------------------------------ 13. external gradient
def test_external_gradient_path_takes_the_scale():
    """logits.backward(gradient=...) through the autograd bridge with a scaler: the arena equals S x the arena without one."""
    from oracle import restatement as R
    from dmmfods_amd.optim import DynamicLossScaler
    rgb, lidar, tgt = _inputs(R, 5)
    G = torch.randn(tgt.shape, generator=torch.Generator().manual_seed(3)).to(DEV)

    def run(scaler):
        model = _model(R, scaler=scaler)
        logits = model(rgb, lidar)
        logits.backward(gradient=G)
        g = model.grad_arena.clone()
        torch.cuda.synchronize()
        model.close()
        return g
    a, b = run(None), run(None)
    lim = _allowed([a], [b], "external gradient")[0]
    c = run(DynamicLossScaler(init_scale=2.0 ** 5, growth_interval=0))
    d = _dist(c / 32.0, a)
    print(f"external gradient: scaled / 32 vs unscaled {d:.3e} (allowed {lim:.3e})")
    assert float(c.abs().max()) > 16 * float(a.abs().max())
    assert d <= lim
