"""The guarded optimiser step (dynamic loss scale, skipped step on overflow, clipping by global norm), everything that needs no
GPU: the C entry points refuse bad arguments before they touch HIP, the Python surface validates and checkpoints, the sanitizer
harness covers the new host code and shows the dynamic scale pointer in the loss record, and a pure-Python restatement of the rule
(GuardRule) that tests/test_guard_gpu.py replays against the device's decisions."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = dict(growth_rate=8, block_config=(2, 2, 2, 2), num_init_features=16)


# ------------------------------------------------------------------------------------------------ the rule, restated
class GuardRule:
    """include/dmmfods_hip.h, dmm_guard_state: torch.amp.GradScaler's update rule plus torch.nn.utils.clip_grad_norm_'s formula.
    The scale is an fp32 number on the device, so it is one here."""

    def __init__(self, scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, max_norm=None):
        self.scale = np.float32(scale)
        self.growth_factor, self.backoff_factor = np.float32(growth_factor), np.float32(backoff_factor)
        self.growth_interval, self.max_norm = int(growth_interval), max_norm
        self.applied = self.skipped = self.tracker = 0

    def step(self, found_inf, sumsq=0.0):
        """One optimiser step on an arena with sum of squares `sumsq` (as stored: scaled).  Returns (applied?, unscaled norm,
        clip coefficient, multiplier Adam puts on every stored gradient)."""
        S = self.scale
        if found_inf:
            self.scale = np.float32(S * self.backoff_factor)
            self.tracker = 0
            self.skipped += 1
            return False, float("nan"), 0.0, 0.0
        norm = math.sqrt(sumsq) / float(S)
        coef = 1.0 if self.max_norm is None else min(1.0, self.max_norm / (norm + 1e-6))
        self.applied += 1
        self.tracker += 1
        if self.growth_interval > 0 and self.tracker >= self.growth_interval:
            self.scale = np.float32(S * self.growth_factor)
            self.tracker = 0
        return True, norm, coef, coef / float(S)


def test_rule_restatement_behaves_like_gradscaler():
    r = GuardRule(scale=2.0 ** 16, growth_interval=3)
    seq = [True, True, False, False, False, False, True, False, False, False]
    scales = []
    for f in seq:
        r.step(f, sumsq=4.0)
        scales.append(float(r.scale))
    #          inf      inf     ok      ok      ok->grow ok      inf     ok      ok      ok->grow
    assert scales == [2.0 ** 15, 2.0 ** 14, 2.0 ** 14, 2.0 ** 14, 2.0 ** 15, 2.0 ** 15, 2.0 ** 14, 2.0 ** 14, 2.0 ** 14, 2.0 ** 15]
    assert (r.applied, r.skipped, r.tracker) == (7, 3, 0)
    # the same sequence through torch's own scale update (the op behind GradScaler.update), where this torch has it on the CPU
    try:
        sc, tr, got = torch.tensor(2.0 ** 16), torch.tensor(0, dtype=torch.int32), []
        for f in seq:
            torch._amp_update_scale_(sc, tr, torch.tensor(1.0 if f else 0.0), 2.0, 0.5, 3)
            got.append(float(sc))
    except (RuntimeError, NotImplementedError, AttributeError):
        got = scales
    assert got == scales
    # clipping: torch's formula; a fixed scale (growth_interval 0) never grows and still backs off; the scale may fall below 1
    c = GuardRule(scale=4.0, growth_interval=0, max_norm=1.0)
    ok, norm, coef, mult = c.step(False, sumsq=(4.0 * 3.0) ** 2)
    assert ok and norm == 3.0 and coef == 1.0 / (3.0 + 1e-6) and mult == coef / 4.0
    for _ in range(5):
        c.step(False, sumsq=1.0)
    assert float(c.scale) == 4.0
    for _ in range(4):
        c.step(True)
    assert float(c.scale) == 0.25 and c.skipped == 4 and c.applied == 6


# ------------------------------------------------------------------------------------------------ C entry points
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from dmmfods_amd import _lib
    return _lib


def _refused(lib, rc, word):
    assert rc == lib.ERR_INVALID, rc
    msg = lib.lib().dmm_last_error().decode()
    assert word in msg, msg


def test_guard_entry_points_refuse_bad_arguments_without_a_gpu(lib):
    L = lib.lib()
    assert L.dmm_version() >= 101
    assert C.sizeof(lib.GuardState) == 64 and lib.GuardState.scale.offset == 0 and lib.GuardState.sumsq.offset == 8
    assert lib.GuardState.applied_steps.offset == 24 and lib.GuardState.skipped_steps.offset == 32
    nb = L.dmm_grad_guard_scratch_bytes(23567564)
    assert nb > 0 and nb % 8 == 0 and L.dmm_grad_guard_scratch_bytes(1) == nb      # a fixed grid: one partial per workgroup
    P = 1 << 20   # an address nothing dereferences: every refusal below comes before the first HIP call
    # state init
    _refused(lib, L.dmm_guard_state_init(None, 65536.0, 0, 0, None), "null")
    _refused(lib, L.dmm_guard_state_init(P + 4, 65536.0, 0, 0, None), "aligned")
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        _refused(lib, L.dmm_guard_state_init(P, bad, 0, 0, None), "init_scale")
    _refused(lib, L.dmm_guard_state_init(P, 1.0, -1, 0, None), ">= 0")
    _refused(lib, L.dmm_guard_state_init(P, 1.0, 0, -1, None), ">= 0")
    # the step: params, grads, exp_avg, exp_avg_sq, n, lr, b1, b2, eps, wd, max_norm, growth, backoff, interval, state, scratch, stream
    good = [P, P, P, P, 16, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0.0, 2.0, 0.5, 2000, P, P, None]
    for idx in (0, 1, 2, 3, 14, 15):
        a = list(good)
        a[idx] = None
        _refused(lib, L.dmm_adam_step_guarded(*a), "null")
    for idx, val, word in ((4, -1, "n must"), (11, 0.5, "growth_factor"), (11, float("nan"), "growth_factor"), (11, float("inf"), "growth_factor"),
                           (12, 0.0, "backoff_factor"), (12, 1.5, "backoff_factor"), (12, float("nan"), "backoff_factor"), (13, -1, "growth_interval"),
                           (10, float("nan"), "max_norm"), (6, 1.0, "betas"), (7, -0.1, "betas"), (14, P + 4, "misaligned"), (1, P + 2, "misaligned")):
        a = list(good)
        a[idx] = val
        _refused(lib, L.dmm_adam_step_guarded(*a), word)
    # the reduction alone
    _refused(lib, L.dmm_grad_sumsq(None, 0, 4, 0, P, None), "null")
    _refused(lib, L.dmm_grad_sumsq(P, 0, 4, 0, None, None), "null")
    _refused(lib, L.dmm_grad_sumsq(P, -1, 4, 0, P, None), ">= 0")
    _refused(lib, L.dmm_grad_sumsq(P, 0, -4, 0, P, None), ">= 0")
    # the plan's pointer: needs a plan, takes NULL, refuses a misaligned address; an unbound plan keeps it for its bind
    _refused(lib, L.dmm_plan_set_dynamic_loss_scale(None, P), "null plan")
    d = lib.ModelDesc()
    d.growth_rate, d.num_blocks, d.num_init_features, d.bn_size, d.num_classes = 8, 4, 16, 4, 3
    for i in range(4):
        d.block_config[i] = 2
    d.concat_before_block_num, d.stream_1_in_channels, d.stream_2_in_channels = 3, 3, 3
    d.batch, d.height, d.width, d.dtype, d.loss_scale, d.bn_momentum, d.bn_eps, d.iou_threshold, d.use_mfma = 2, 64, 96, lib.DMM_F16, 1.0, 0.1, 1e-5, 0.7, 1
    h = C.c_void_p()
    lib.check(L.dmm_plan_create(C.byref(d), C.byref(h)))
    try:
        _refused(lib, L.dmm_plan_set_dynamic_loss_scale(h, P + 2), "aligned")
        assert L.dmm_plan_set_dynamic_loss_scale(h, P) == 0
        assert L.dmm_plan_set_dynamic_loss_scale(h, None) == 0
    finally:
        lib.check(L.dmm_plan_destroy(h))


# ------------------------------------------------------------------------------------------------ Python surface
def _cpu_model(lib):
    from dmmfods_amd.graphs.models.Dense_U_Net_lidar import Dense_U_Net_lidar
    from dmmfods_amd.utils.Dense_U_Net_lidar_helper import get_config
    cfg = get_config("/tmp/dmm_test")
    cfg.model.growth_rate, cfg.model.block_config, cfg.model.num_init_features = TINY["growth_rate"], TINY["block_config"], TINY["num_init_features"]
    cfg.model.concat_before_block_num, cfg.model.stream_2_in_channels = 3, 3
    return Dense_U_Net_lidar(cfg, compute_dtype="fp16")


def test_optimizer_and_scaler_validate_their_arguments(lib):
    from dmmfods_amd.optim import DynamicLossScaler, FusedAdam
    s = DynamicLossScaler()
    assert (s.get_scale(), s.growth_factor, s.backoff_factor, s.growth_interval) == (65536.0, 2.0, 0.5, 2000)   # torch's defaults
    assert DynamicLossScaler(init_scale=0.25, growth_interval=0).get_scale() == 0.25        # below 1 is allowed; 0 = never grows
    for kw in (dict(init_scale=0), dict(init_scale=-2.0), dict(init_scale=float("inf")), dict(growth_factor=1.0), dict(growth_factor=0.5),
               dict(backoff_factor=0.0), dict(backoff_factor=1.0), dict(backoff_factor=1.5), dict(growth_interval=-1), dict(growth_interval=2.5)):
        with pytest.raises(ValueError):
            DynamicLossScaler(**kw)
    with pytest.raises(ValueError):
        s.set_scale(0.0)
    s.set_scale(1024.0)
    assert s.get_scale() == 1024.0 and s.loss_scale is None        # no device block yet: nothing was allocated on a GPU
    model = _cpu_model(lib)
    for bad in (0, 0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            FusedAdam(model, max_grad_norm=bad)
    with pytest.raises(ValueError):
        FusedAdam(model, loss_scaler=object())
    with pytest.raises(ValueError):
        FusedAdam(model, amsgrad=True, loss_scaler=s)               # still unsupported
    with pytest.raises(ValueError):
        model.set_loss_scaler(object())
    plain = FusedAdam(model)
    assert plain._guard is None and plain.loss_scale is None and plain.last_grad_norm is None and plain.last_found_inf is None
    assert model._loss_scaler is None
    opt = FusedAdam(model, max_grad_norm=1.0, loss_scaler=s)
    assert model._loss_scaler is s and opt._guard is s              # FusedAdam attaches the scaler to the model
    with pytest.raises(ValueError):
        opt.step(grad_scale=0.5)                                    # refused before anything touches a device
    assert FusedAdam(model, max_grad_norm=2.0)._guard is not None   # clipping alone takes the guarded path too (S = 1)
    model.set_loss_scaler(None)
    assert model._loss_scaler is None


def test_state_dict_round_trip_and_torch_adam_compatibility(lib):
    from dmmfods_amd.optim import DynamicLossScaler, FusedAdam
    model = _cpu_model(lib)
    g = torch.Generator().manual_seed(5)
    s = DynamicLossScaler(init_scale=2.0 ** 12, growth_interval=7)
    opt = FusedAdam(model, lr=2e-3, max_grad_norm=3.0, loss_scaler=s)
    opt.exp_avg.copy_(torch.randn(opt.exp_avg.shape, generator=g))
    opt.exp_avg_sq.copy_(torch.rand(opt.exp_avg_sq.shape, generator=g))
    opt.step_count = 11
    s.load_state_dict({"scale": 2.0 ** 9, "growth_tracker": 5, "skipped_steps": 4})
    sd = opt.state_dict()
    assert set(sd) == {"state", "param_groups", "loss_scaler"}
    assert sd["loss_scaler"] == {"scale": 512.0, "growth_tracker": 5, "skipped_steps": 4}
    assert float(sd["state"][0]["step"]) == 11.0 and set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    # ... into a fresh guarded optimiser
    s2 = DynamicLossScaler()
    opt2 = FusedAdam(_cpu_model(lib), loss_scaler=s2)
    opt2.load_state_dict(sd)
    assert opt2.step_count == 11 and opt2.param_groups[0]["lr"] == 2e-3
    assert s2.state_dict() == sd["loss_scaler"] and s2.get_scale() == 512.0 and s2.skipped_steps == 4 and s2.growth_tracker == 5
    assert torch.equal(opt2.exp_avg, opt.exp_avg) and torch.equal(opt2.exp_avg_sq, opt.exp_avg_sq)
    # ... a checkpoint without the key (the plain path's, or the reference's) loads, and the scaler keeps what it had
    plain_sd = {k: v for k, v in sd.items() if k != "loss_scaler"}
    s3 = DynamicLossScaler(init_scale=8.0)
    opt3 = FusedAdam(_cpu_model(lib), loss_scaler=s3)
    opt3.load_state_dict(plain_sd)
    assert opt3.step_count == 11 and s3.get_scale() == 8.0 and s3.skipped_steps == 0
    # ... the plain optimiser ignores the key and writes none
    opt4 = FusedAdam(_cpu_model(lib))
    opt4.load_state_dict(sd)
    assert opt4.step_count == 11 and set(opt4.state_dict()) == {"state", "param_groups"}
    # ... clipping alone: the key carries the skipped count, the scale stays 1
    opt5 = FusedAdam(_cpu_model(lib), max_grad_norm=1.0)
    opt5.load_state_dict(sd)
    assert opt5.state_dict()["loss_scaler"] == {"scale": 1.0, "growth_tracker": 0, "skipped_steps": 4}
    # ... and torch.optim.Adam accepts the dict as it is
    m5 = _cpu_model(lib)
    ref = torch.optim.Adam(list(m5.parameters()), lr=1e-3)
    ref.load_state_dict(sd)
    st = ref.state[next(iter(m5.parameters()))]
    assert float(st["step"]) == 11.0 and torch.equal(st["exp_avg"], sd["state"][0]["exp_avg"])
    assert ref.param_groups[0]["lr"] == 2e-3


def test_agent_takes_the_new_arguments_from_the_config_only_if_present():
    import inspect
    from dmmfods_amd.agents.Dense_U_Net_lidar_Agent import Dense_U_Net_lidar_Agent
    from dmmfods_amd.utils.Dense_U_Net_lidar_helper import get_config
    sig = inspect.signature(Dense_U_Net_lidar_Agent.__init__)
    assert sig.parameters["max_grad_norm"].default is None and sig.parameters["loss_scaler"].default is None
    cfg = get_config("/tmp/dmm_test")
    assert "max_grad_norm" not in cfg.optimizer and "dynamic_loss_scale" not in cfg.optimizer    # create_config keeps the reference's field list
    assert Dense_U_Net_lidar_Agent._optional(cfg.optimizer, "max_grad_norm") is None
    cfg.optimizer.max_grad_norm = 5.0
    assert Dense_U_Net_lidar_Agent._optional(cfg.optimizer, "max_grad_norm") == 5.0


# ------------------------------------------------------------------------------------------------ sanitizer harness
@pytest.fixture(scope="module")
def host_drive():
    out = os.path.join(ROOT, "tools", "hoststub", "_build")
    subprocess.run([os.path.join(ROOT, "tools", "hoststub", "build.sh"), out], check=True, capture_output=True, timeout=900)
    return os.path.join(out, "drive")


def _env(**extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith("DMM_") and not k.startswith("DRIVE_")}
    env.update(ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", **extra)
    return env


def test_sanitizer_harness_covers_the_guarded_step_and_dump_shows_the_scale_pointer(host_drive):
    """guard.hip's host side is part of the harness build; existing life-cycle cases stay clean; with DRIVE_DYN_SCALE=1 the plan
    carries a dynamic scale pointer through loss + backward, the external-gradient backward and a re-run, every guarded-step entry
    point runs under ASan / UBSan, and `drive dump` prints the pointer in the loss record of the backward list (and nowhere else)."""
    for arch, dtype, b, h, w in (("tiny_mid", "bf16", 2, 96, 160), ("d121e", "f16", 2, 64, 96)):
        for extra in ({}, {"DRIVE_DYN_SCALE": "1"}):
            r = subprocess.run([host_drive, arch, dtype, str(b), str(h), str(w), "3"], env=_env(**extra), capture_output=True, text=True, timeout=600)
            tail = (r.stdout + r.stderr)[-3000:]
            assert r.returncode == 0 and "DRIVE OK" in r.stdout, (arch, extra, tail)
            lives = [ln for ln in r.stdout.splitlines() if ln.startswith("life ")]
            assert len(lives) == 3 and all(", 0 bad," in ln and ln.endswith("violations 0") for ln in lives), lives
        args = [arch, dtype, str(b), str(h), str(w)]
        off = subprocess.run([host_drive, "dump"] + args, env=_env(), capture_output=True, text=True, timeout=600)
        on = subprocess.run([host_drive, "dump"] + args, env=_env(DRIVE_DYN_SCALE="1"), capture_output=True, text=True, timeout=600)
        assert off.returncode == 0 and on.returncode == 0, (off.stderr[-2000:], on.stderr[-2000:])
        assert "OUTSIDE" not in on.stdout
        bce_off = [ln for ln in off.stdout.splitlines() if ln.startswith("    bce:")]
        bce_on = [ln for ln in on.stdout.splitlines() if ln.startswith("    bce:")]
        assert len(bce_off) == len(bce_on) == 2                     # the backward list's loss record, and bce_only (validation)
        assert all(ln.endswith(" dyn_scale=null") for ln in bce_off)
        assert bce_on[0].endswith(" dyn_scale=guard+0") and bce_on[1].endswith(" dyn_scale=null")
        conv = [ln for ln in on.stdout.splitlines() if ln.startswith("    convert:")]
        assert conv and all(ln.endswith(" dyn_scale=null") for ln in conv)      # input conversions never take it
        # the pointer is the only difference between the two plans
        assert re.sub(r" dyn_scale=\S+", "", on.stdout) == re.sub(r" dyn_scale=\S+", "", off.stdout)
