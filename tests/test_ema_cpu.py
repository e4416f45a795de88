"""The parameter average (FusedAdam(ema_decay=...), dmm_adam_step_segmented_ema, dmm_adam_step_guarded_segmented_ema) as far as it
goes without a GPU: the constructor's validation, the checkpoint key and its round trip, the decay schedule, the exported state
dict's layout, every refusal of the two entry points before they touch HIP, and the sanitizer harness (DRIVE_EMA=1 drives both entry
points under a table with a gap and a class with t0 > 0; without the switch a pinned enqueue trace keeps its hash)."""
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = dict(growth_rate=8, block_config=(2, 2, 2, 2), num_init_features=16)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from dmmfods_amd import _lib
    return _lib


def _cpu_model():
    from dmmfods_amd.graphs.models.Dense_U_Net_lidar import Dense_U_Net_lidar
    from dmmfods_amd.utils.Dense_U_Net_lidar_helper import get_config
    cfg = get_config("/tmp/dmm_test")
    cfg.model.growth_rate, cfg.model.block_config, cfg.model.num_init_features = TINY["growth_rate"], TINY["block_config"], TINY["num_init_features"]
    cfg.model.concat_before_block_num, cfg.model.stream_2_in_channels = 3, 3
    model = Dense_U_Net_lidar(cfg, compute_dtype="fp32")
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        model.param_arena.copy_(torch.randn(model.param_arena.shape, generator=g))
    return model


# ------------------------------------------------------------------------------------------------ Python surface
def test_constructor_validates_the_decay(lib):
    from dmmfods_amd.optim import FusedAdam
    model = _cpu_model()
    for bad in (1.0, -0.1, float("nan"), "0.9", 1.5, True, 1.0 - 1e-12):    # (the last one is 1 as an fp32 value)
        with pytest.raises(ValueError):
            FusedAdam(model, ema_decay=bad)
    off = FusedAdam(model)
    assert off.ema_decay is None and off.ema_arena is None
    for call in (off.ema_reset, off.ema_state_dict, lambda: off.ema_decay_at(1), lambda: off.ema_num_updates, lambda: off.ema_weights().__enter__()):
        with pytest.raises(RuntimeError):
            call()
    on = FusedAdam(model, ema_decay=0.999)
    assert on.ema_decay == float(np.float32(0.999)) and on.ema_warmup is True and on.ema_num_updates == 0
    assert on.ema_arena.dtype == torch.float32 and on.ema_arena.shape == model.param_arena.shape
    assert on.ema_arena.data_ptr() != model.param_arena.data_ptr() and torch.equal(on.ema_arena, model.param_arena)
    assert FusedAdam(model, ema_decay=0).ema_decay == 0.0 and FusedAdam(model, ema_decay=0.5, ema_warmup=False).ema_warmup is False


def test_decay_schedule_is_the_formula(lib):
    from dmmfods_amd.optim import FusedAdam
    model = _cpu_model()
    d = float(np.float32(0.999))
    warm, flat = FusedAdam(model, ema_decay=0.999), FusedAdam(model, ema_decay=0.999, ema_warmup=False)
    for k in (1, 2, 10, 10 ** 6):
        assert warm.ema_decay_at(k) == min(d, (1.0 + k) / (10.0 + k))
        assert flat.ema_decay_at(k) == d
    assert warm.ema_decay_at(1) == 2.0 / 11.0 and warm.ema_decay_at(10) == 11.0 / 20.0 and warm.ema_decay_at(10 ** 6) == d
    assert np.float32(1.0 - warm.ema_decay_at(1)) == np.float32(9.0 / 11.0)
    with pytest.raises(ValueError):
        warm.ema_decay_at(0)


def test_state_dict_key_and_round_trip(lib):
    from dmmfods_amd.optim import FusedAdam
    g = torch.Generator().manual_seed(3)
    model = _cpu_model()
    assert set(FusedAdam(model).state_dict()) == {"state", "param_groups"}
    assert set(FusedAdam(model, max_grad_norm=1.0).state_dict()) == {"state", "param_groups", "loss_scaler"}
    for guarded in (False, True):
        kw = dict(max_grad_norm=1.0) if guarded else {}
        opt = FusedAdam(model, ema_decay=0.99, ema_warmup=False, **kw)
        opt.exp_avg.copy_(torch.randn(opt.exp_avg.shape, generator=g))
        opt.exp_avg_sq.copy_(torch.rand(opt.exp_avg_sq.shape, generator=g))
        opt.ema_arena.copy_(torch.randn(opt.ema_arena.shape, generator=g))
        opt.step_count = 11
        if guarded:
            opt._ema_t0 = 4           # averaging began at applied step 4: 7 updates
        else:
            opt._ema_k = 7
        sd = opt.state_dict()
        assert set(sd) == {"state", "param_groups", "ema"} | ({"loss_scaler"} if guarded else set())
        assert set(sd["ema"]) == {"decay", "warmup", "num_updates", "params"}
        assert sd["ema"]["decay"] == float(np.float32(0.99)) and sd["ema"]["warmup"] is False and sd["ema"]["num_updates"] == 7
        assert sd["ema"]["params"].device.type == "cpu" and sd["ema"]["params"].dtype == torch.float32 and sd["ema"]["params"].dim() == 1
        assert torch.equal(sd["ema"]["params"], opt.ema_arena) and sd["ema"]["params"].data_ptr() != opt.ema_arena.data_ptr()
        # ... into a fresh optimiser of either path
        for kw2 in ({}, dict(max_grad_norm=2.0)):
            opt2 = FusedAdam(_cpu_model(), ema_decay=0.99, **kw2)
            opt2.load_state_dict(sd)
            assert opt2.step_count == 11 and opt2.ema_num_updates == 7 and torch.equal(opt2.ema_arena, opt.ema_arena)
            assert torch.equal(opt2.exp_avg, opt.exp_avg)
        # ... torch.optim.Adam takes the dict as it is (it ignores the key, as it does loss_scaler)
        ref = torch.optim.Adam([torch.nn.Parameter(p.detach().clone()) for p in model.parameters()])
        ref.load_state_dict(sd)
        # ... a checkpoint written without an average: the average starts at the parameters, after the state is in
        other = _cpu_model()
        with torch.no_grad():
            other.param_arena.mul_(2.0)
        opt3 = FusedAdam(other, ema_decay=0.5, **kw)
        opt3.ema_arena.zero_()
        opt3.load_state_dict({k: v for k, v in sd.items() if k != "ema"})
        assert opt3.step_count == 11 and opt3.ema_num_updates == 0 and torch.equal(opt3.ema_arena, other.param_arena)
        # ... and an optimiser without an average ignores the key and writes none
        opt4 = FusedAdam(_cpu_model(), **kw)
        opt4.load_state_dict(sd)
        assert opt4.step_count == 11 and "ema" not in opt4.state_dict() and opt4.ema_arena is None
    # ema_reset: the parameters again, k from the start
    opt.ema_reset()
    assert opt.ema_num_updates == 0 and torch.equal(opt.ema_arena, model.param_arena)
    # a parameter average of another size is refused
    with pytest.raises(ValueError):
        opt.load_state_dict(dict(sd, ema=dict(sd["ema"], params=sd["ema"]["params"][:-1])))


def test_exported_state_dict_has_the_models_layout(lib):
    from dmmfods_amd.optim import FusedAdam
    model = _cpu_model()
    opt = FusedAdam(model, ema_decay=0.9)
    with torch.no_grad():
        opt.ema_arena.add_(1.0)
    msd, esd = model.state_dict(), opt.ema_state_dict()
    assert list(esd) == list(msd)
    assert [tuple(v.shape) for v in esd.values()] == [tuple(v.shape) for v in msd.values()]
    assert [v.dtype for v in esd.values()] == [v.dtype for v in msd.values()]
    params = {n for n, _ in model.named_parameters()}
    off = 0
    for k, v in esd.items():
        if k in params:
            n = v.numel()
            assert torch.equal(v.reshape(-1), opt.ema_arena[off:off + n]) and torch.equal(v, msd[k] + 1.0), k
            off += n
        else:
            assert torch.equal(v, msd[k]), k                                 # live buffers: running statistics, num_batches_tracked
    assert off == opt.ema_arena.numel()
    before = opt.ema_arena.clone()
    for v in esd.values():
        v.zero_()                                                            # clones: nothing of the optimiser or the model moves
    assert torch.equal(opt.ema_arena, before) and torch.equal(model.state_dict()[next(iter(params))], msd[next(iter(params))])
    other = _cpu_model()
    other.load_state_dict(opt.ema_state_dict())
    assert torch.equal(other.param_arena, opt.ema_arena)


def test_ema_weights_exchanges_the_arenas_on_the_host_too(lib):
    """(The GPU test runs the model inside the block; the exchange itself, its guards and the restore on an exception need no device.)"""
    from dmmfods_amd.optim import FusedAdam
    model = _cpu_model()
    opt = FusedAdam(model, ema_decay=0.9)
    with torch.no_grad():
        opt.ema_arena.mul_(0.5)
    p0, e0, addr = model.param_arena.clone(), opt.ema_arena.clone(), model.param_arena.data_ptr()
    model._last = ("a plan", "its logits")
    with opt.ema_weights():
        assert model._last is None
        assert torch.equal(model.param_arena, e0) and torch.equal(opt.ema_arena, p0) and model.param_arena.data_ptr() == addr
        for call in (opt.step, lambda: opt.load_state_dict({}), opt.ema_reset, opt.state_dict, lambda: opt.ema_weights().__enter__()):
            with pytest.raises(RuntimeError):
                call()
    assert torch.equal(model.param_arena, p0) and torch.equal(opt.ema_arena, e0)
    with pytest.raises(KeyError):
        with opt.ema_weights():
            raise KeyError("the body fails")
    assert torch.equal(model.param_arena, p0) and torch.equal(opt.ema_arena, e0) and not opt._ema_swapped


def test_agent_reads_the_config_fields_only_if_present():
    import inspect
    from dmmfods_amd.agents.Dense_U_Net_lidar_Agent import Dense_U_Net_lidar_Agent
    from dmmfods_amd.optim import FusedAdam
    from dmmfods_amd.utils.Dense_U_Net_lidar_helper import get_config
    o = get_config("/tmp/dmm_test").optimizer
    assert Dense_U_Net_lidar_Agent._optional(o, "ema_decay") is None and Dense_U_Net_lidar_Agent._optional(o, "ema_warmup") is None
    sig = inspect.signature(FusedAdam.__init__)
    assert sig.parameters["ema_decay"].default is None and sig.parameters["ema_warmup"].default is True
    assert list(sig.parameters)[-2:] == ["ema_decay", "ema_warmup"]


# ------------------------------------------------------------------------------------------------ C entry points
def test_struct_layout_matches_the_header(lib, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dmmfods_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu\\n", sizeof(dmm_adam_ema), offsetof(dmm_adam_ema, ema), offsetof(dmm_adam_ema, decay),\n'
                   '         offsetof(dmm_adam_ema, warmup), offsetof(dmm_adam_ema, k_or_t0));\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    cc = next(c for c in ("cc", "gcc", "clang", "/opt/rocm/lib/llvm/bin/clang") if subprocess.run(["sh", "-c", f"command -v {c}"], capture_output=True).returncode == 0)
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True, timeout=120)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    E = lib.AdamEma
    assert got == [C.sizeof(E), E.ema.offset, E.decay.offset, E.warmup.offset, E.k_or_t0.offset] == [24, 0, 8, 12, 16]


def test_both_entry_points_refuse_bad_averages_before_any_hip_call(lib):
    """Every refusal of the average's own arguments comes before the table is looked up, so none needs a device; the message names
    the argument.  What the counterparts refuse (here: a table that was never initialised) is still refused behind them."""
    L = lib.lib()
    n = 4096
    bufs = [(C.c_float * n)() for _ in range(5)]
    p, g, m, v, e = (C.addressof(b) for b in bufs)
    table = (C.c_int64 * 64)()
    cls = (lib.AdamClass * 1)(lib.AdamClass(1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 0))
    state, scratch = (C.c_int64 * 8)(), (C.c_double * 1024)()

    def plain(ema, step=3):
        return L.dmm_adam_step_segmented_ema(p, g, m, v, n, C.addressof(table), 1, cls, 1, step, 1.0, None, ema)

    def guarded(ema):
        return L.dmm_adam_step_guarded_segmented_ema(p, g, m, v, n, C.addressof(table), 1, cls, 1, 1.0, 2.0, 0.5, 2000, C.addressof(state),
                                                     C.addressof(scratch), None, ema)

    def E(ema=e, decay=0.9, warmup=1, k=1):
        return C.byref(lib.AdamEma(ema, decay, warmup, k))

    cases = [(None, b"ema is null"), (E(ema=None), b"ema->ema is null"), (E(ema=e + 2), b"ema->ema is misaligned"),
             (E(ema=p), b"ema->ema aliases params"), (E(ema=g), b"ema->ema aliases grads"), (E(ema=m), b"ema->ema aliases exp_avg"),
             (E(ema=v), b"ema->ema aliases exp_avg_sq"), (E(ema=p + 4 * (n - 1)), b"ema->ema aliases params"),
             (E(ema=v - 4 * (n - 1)), b"ema->ema aliases"),
             (E(decay=1.0), b"ema->decay"), (E(decay=-0.1), b"ema->decay"), (E(decay=2.0), b"ema->decay"), (E(decay=float("nan")), b"ema->decay")]
    for fn, who in ((plain, b"dmm_adam_step_segmented_ema: "), (guarded, b"dmm_adam_step_guarded_segmented_ema: ")):
        for ema, text in cases:
            rc = fn(ema)
            assert rc == lib.ERR_INVALID and L.dmm_last_error().startswith(who) and text in L.dmm_last_error(), (text, rc, L.dmm_last_error())
        # a good average: the counterpart's own refusal is reached (no table was initialised at this address; nothing was launched)
        rc = fn(E())
        assert rc == lib.ERR_INVALID and b"not initialised by dmm_adam_table_init" in L.dmm_last_error(), L.dmm_last_error()
    for k in (0, -3):
        rc = plain(E(k=k))
        assert rc == lib.ERR_INVALID and b"ema->k_or_t0" in L.dmm_last_error(), (k, L.dmm_last_error())
    rc = plain(E(), step=0)
    assert rc == lib.ERR_INVALID and b"step must be >= 1" in L.dmm_last_error()
    cls[0].beta1 = 1.0
    assert plain(E()) == lib.ERR_INVALID and b"betas" in L.dmm_last_error()
    assert guarded(E()) == lib.ERR_INVALID and b"betas" in L.dmm_last_error()
    with pytest.raises(ValueError):
        lib.check(plain(None))


# ------------------------------------------------------------------------------------------------ the sanitizer harness
@pytest.fixture(scope="module")
def drive():
    out = os.path.join(ROOT, "tools", "hoststub", "_build")
    subprocess.run([os.path.join(ROOT, "tools", "hoststub", "build.sh"), out], check=True, capture_output=True, timeout=900)
    return os.path.join(out, "drive")


def _run(drive, envx, args):
    env = {k: v for k, v in os.environ.items() if not k.startswith("DMM_") and not k.startswith("DRIVE_")}
    env.update(envx, DRIVE_TRACE_ENQUEUE="1", ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([drive] + args.split(), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "DRIVE OK" in r.stdout, (envx, (r.stdout[-1000:] + r.stderr)[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    return [ln for ln in r.stdout.splitlines() if ln.startswith("T ")]


def test_harness_drives_both_entry_points_and_leaves_the_pinned_trace_alone(drive):
    """DRIVE_FREEZE=1 DRIVE_EMA=1: the freeze life also takes the two steps with an average (a gap in front of the table, then a class
    with t0 > 0) and tries each refusal, under ASan + UBSan.  Every step is still ONE launch of the one Adam kernel on the same grid.  Without the switch the DRIVE_FREEZE row keeps its pinned hash."""
    args = "tiny_mid f16 2 64 96 2"
    base = _run(drive, {"DRIVE_FREEZE": "1"}, args)
    pinned = json.load(open(os.path.join(ROOT, "tests", "golden", "enqueue_trace_sha256.json")))
    assert hashlib.sha256("\n".join(base).encode()).hexdigest() == pinned["DRIVE_FREEZE=1 | " + args]
    ema = _run(drive, {"DRIVE_FREEZE": "1", "DRIVE_EMA": "1"}, args)

    def adam(lines):
        return [ln for ln in lines if ln.startswith("T launch") and "adam" in ln]

    a0, a1 = adam(base), adam(ema)
    assert len(a0) == 4 and len(a1) == 4 * 4, (len(a0), len(a1))              # two lives of two steps; with the switch three more each
    assert {ln.split()[2] for ln in a1} == {ln.split()[2] for ln in a0} and len({ln.split()[2] for ln in a1}) == 1   # one kernel
    assert {tuple(ln.split()[3:5]) for ln in a1} == {tuple(ln.split()[3:5]) for ln in a0}                            # the same grid
    assert not [ln for ln in ema if ln.startswith("T error")]                 # (a refusal that is expected is checked by the driver itself)
