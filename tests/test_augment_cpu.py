"""On-device batch augmentation (dmm_augment_batch, dmmfods_amd/augment.py, config.loader.augment) as far as it goes without a GPU:
the struct layouts against a compiled C probe, every refusal of the entry point before it touches HIP, BatchAugment's validation and
its parameter generator, the agent's config field, and the sanitizer harness (DRIVE_AUGMENT=1 drives one valid call of 33 samples -
two launches - and every refusal under ASan + UBSan; without the switch a pinned enqueue trace keeps its hash)."""
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from dmmfods_amd import _lib
    return _lib


# ------------------------------------------------------------------------------------------------ C entry point
def test_symbol_is_declared_exported_and_bound(lib):
    header = open(os.path.join(ROOT, "include", "dmmfods_hip.h")).read()
    assert "dmm_augment_batch(" in header and "dmm_augment_batch" in lib.EXPORTS and hasattr(lib.lib(), "dmm_augment_batch")
    for name, val in (("DMM_AUG_MAX_TENSORS", lib.AUG_MAX_TENSORS), ("DMM_AUG_MAX_CHANNELS", lib.AUG_MAX_CHANNELS), ("DMM_AUG_LAUNCH_BATCH", lib.AUG_LAUNCH_BATCH)):
        assert any(ln.split()[:3] == ["#define", name, str(val)] for ln in header.splitlines()), name
    assert (lib.AUG_MAX_TENSORS, lib.AUG_MAX_CHANNELS, lib.AUG_LAUNCH_BATCH) == (4, 8, 32)


def test_struct_layouts_match_the_header(lib, tmp_path):
    fields_t, fields_s = ("src", "dst", "src_batch_stride", "channels", "reserved"), ("y0", "x0", "flip", "reserved", "gain", "bias")
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dmmfods_hip.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(dmm_aug_tensor));\n'
                   + "".join(f'  printf(" %zu", offsetof(dmm_aug_tensor, {f}));\n' for f in fields_t)
                   + '  printf(" %zu", sizeof(dmm_aug_sample));\n'
                   + "".join(f'  printf(" %zu", offsetof(dmm_aug_sample, {f}));\n' for f in fields_s)
                   + '  printf("\\n");\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    cc = next(c for c in ("cc", "gcc", "clang", "/opt/rocm/lib/llvm/bin/clang") if subprocess.run(["sh", "-c", f"command -v {c}"], capture_output=True).returncode == 0)
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True, timeout=120)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    T, S = lib.AugTensor, lib.AugSample
    mine = [C.sizeof(T)] + [getattr(T, f).offset for f in fields_t] + [C.sizeof(S)] + [getattr(S, f).offset for f in fields_s]
    assert got == mine == [32, 0, 8, 16, 24, 28, 80, 0, 4, 8, 12, 16, 48]


def _call(lib, B=3, Hs=16, Ws=24, Ho=16, Wo=24, ntensors=2, tensors=None, samples=None, fill=(0.5,) * 8, tweak_tensor=None, tweak_sample=None,
          null_tensors=False, null_samples=False):
    """A call on addresses nothing dereferences (only the structures and `fill` are host memory the checks read)."""
    src, dst = 0x10000000, 0x20000000
    T = (lib.AugTensor * 4)()
    for t in range(4):   # 2 channels each, slices of one (B, 8, Hs, Ws) batch
        T[t].src, T[t].dst, T[t].src_batch_stride, T[t].channels = src + t * 2 * Hs * Ws * 4, dst + t * B * 2 * Ho * Wo * 4, 8 * Hs * Ws, 2
    S = (lib.AugSample * max(B, 1))()
    for b in range(max(B, 1)):
        S[b].y0, S[b].x0, S[b].flip = b - 1, 1 - b, b & 1
        for c in range(8):
            S[b].gain[c], S[b].bias[c] = 1.0 + c, float(-c)
    if tweak_tensor:
        tweak_tensor(T)
    if tweak_sample:
        tweak_sample(S)
    f = None if fill is None else (C.c_float * 8)(*fill)
    return lib.lib().dmm_augment_batch(None if null_tensors else T, ntensors, None if null_samples else S, B, Hs, Ws, Ho, Wo, f, None)


def test_entry_point_refuses_bad_arguments_before_any_hip_call(lib):
    """Every refusal the header lists, on a machine without a device: a call that got past the checks would reach the runtime."""
    nan, inf = float("nan"), float("inf")

    def tt(t, **kw):
        def f(T):
            for k, v in kw.items():
                setattr(T[t], k, v)
        return dict(tweak_tensor=f)

    def ss(b, c=None, **kw):
        def f(S):
            for k, v in kw.items():
                if c is None:
                    setattr(S[b], k, v)
                else:
                    getattr(S[b], k)[c] = v
        return dict(tweak_sample=f)

    plane = 16 * 24
    cases = [
        (dict(null_tensors=True), b"null"), (dict(null_samples=True), b"null"),
        (tt(1, src=None), b"null src or dst"), (tt(0, dst=None), b"null src or dst"),
        (dict(ntensors=0), b"ntensors"), (dict(ntensors=5), b"ntensors"), (dict(ntensors=-1), b"ntensors"),
        (tt(1, channels=0), b"channels must be >= 1"), (tt(0, channels=-2), b"channels must be >= 1"),
        (dict(ntensors=4, **tt(3, channels=3)), b"sum to at most 8"), (tt(0, channels=9), b"sum to at most 8"),
        (dict(B=0), b">= 1"), (dict(Hs=0), b">= 1"), (dict(Ws=-3), b">= 1"), (dict(Ho=0), b">= 1"), (dict(Wo=0), b">= 1"),
        (dict(B=1, Hs=65536, Ws=32768), b"Hs * Ws"), (dict(B=1, Ho=32768, Wo=65536), b"Ho * Wo"),
        (tt(0, src_batch_stride=2 * plane - 1), b"src_batch_stride"), (tt(1, src_batch_stride=0), b"src_batch_stride"),
        (tt(1, src=0x10000000 + 2), b"4-byte aligned"), (tt(0, dst=0x20000000 + 1), b"4-byte aligned"),
        (ss(2, flip=2), b"flip"), (ss(0, flip=-1), b"flip"),
        (ss(1, y0=2 ** 30 + 1), b"2^30"), (ss(1, y0=-2 ** 30 - 1), b"2^30"), (ss(2, x0=2 ** 30 + 1), b"2^30"), (ss(0, x0=-2 ** 30 - 1), b"2^30"),
        (ss(0, 0, gain=nan), b"NaN or infinite"), (ss(2, 3, gain=inf), b"NaN or infinite"), (ss(1, 1, bias=nan), b"NaN or infinite"),
        (ss(2, 2, bias=-inf), b"NaN or infinite"),
        (dict(fill=(0, 0, nan, 0, 0, 0, 0, 0)), b"fill"), (dict(fill=(inf, 0, 0, 0, 0, 0, 0, 0)), b"fill"),
        (tt(1, reserved=1), b"reserved"), (ss(1, reserved=-1), b"reserved"),
        (tt(0, dst=0x10000000), b"overlaps src"),                                            # in place
        (tt(1, dst=0x10000000 + (2 * 8 * plane + 4 * plane) * 4 - 4), b"overlaps src"),      # the last element of tensor 1's span
        (tt(0, dst=0x10000000 - 3 * 2 * plane * 4 + 4), b"overlaps src"),                    # dst's last element on src's first
        (tt(1, dst=0x20000000 + 3 * 2 * plane * 4 - 4), b"overlaps dst"),                    # dst 1 begins on dst 0's last element
    ]
    L = lib.lib()
    for kw, needle in cases:
        rc = _call(lib, **kw)
        assert rc == lib.ERR_INVALID and needle in L.dmm_last_error(), (kw.keys(), needle, rc, L.dmm_last_error())


# ------------------------------------------------------------------------------------------------ BatchAugment
def test_constructor_validates_its_arguments(lib):
    from dmmfods_amd.augment import BatchAugment
    BatchAugment()
    BatchAugment(out_size=(64, 96), hflip=0.5, translate=(4, 8), brightness=0.2, contrast=0.3, channel_gain=0.1, lidar_dropout=0.4,
                 image_dropout=0.6, fill=[0.0] * 7, seed=2 ** 64 - 1, rank=3)
    assert BatchAugment(out_size=64).out_size == (64, 64) and BatchAugment(translate=3).translate == (3, 3)
    bad = [dict(hflip=-0.1), dict(hflip=1.5), dict(hflip=float("nan")), dict(lidar_dropout=1.01), dict(image_dropout=-1e-9),
           dict(lidar_dropout=0.6, image_dropout=0.5), dict(contrast=1.0), dict(contrast=-0.1), dict(channel_gain=1.0), dict(channel_gain=-0.5),
           dict(channel_gain=float("nan")), dict(brightness=-1.0), dict(brightness=float("inf")), dict(out_size=(0, 64)), dict(out_size=(64, -32)),
           dict(out_size=(64,)), dict(out_size=(64.5, 96)), dict(out_size="big"), dict(translate=(-1, 0)), dict(translate=(1, 2, 3)),
           dict(fill=float("nan")), dict(fill=[0.0] * 9), dict(fill=[]), dict(seed=-1), dict(rank=-1), dict(seed=1.5), dict(rank=2 ** 64)]
    for kw in bad:
        with pytest.raises(ValueError):
            BatchAugment(**kw)
    a = BatchAugment()
    x = torch.zeros(2, 3, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        a(x, x[:, :1], x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        a(x, None, x)
    assert a.batches_drawn == 0


def _same(p, q):
    return all(np.array_equal(getattr(p, k), getattr(q, k)) for k in ("y0", "x0", "flip", "image_gain", "image_bias", "drop_lidar", "drop_image"))


def test_params_at_is_a_pure_function(lib):
    from dmmfods_amd.augment import BatchAugment
    kw = dict(out_size=(64, 96), hflip=0.5, translate=(5, 9), brightness=0.2, contrast=0.3, channel_gain=0.1, lidar_dropout=0.3, image_dropout=0.3, seed=7)
    a, b = BatchAugment(rank=1, **kw), BatchAugment(rank=1, **kw)
    p = a.params_at(3, 16, 96, 128)
    assert _same(p, a.params_at(3, 16, 96, 128)) and _same(p, b.params_at(3, 16, 96, 128)) and a.batches_drawn == 0
    b.params_at(0, 16, 96, 128), b.params_at(9, 4, 96, 128)       # other draws in between change nothing
    assert _same(p, b.params_at(3, 16, 96, 128))
    assert not _same(p, a.params_at(4, 16, 96, 128)) and not _same(p, BatchAugment(rank=2, **kw).params_at(3, 16, 96, 128))
    assert not _same(p, BatchAugment(rank=1, **dict(kw, seed=8)).params_at(3, 16, 96, 128))
    # consecutive batches do not share a shifted stream: no run of one batch's draws appears in the next
    q = a.params_at(4, 16, 96, 128)
    assert not set(p.image_gain.ravel().tolist()) & set(q.image_gain.ravel().tolist())
    # types, shapes and ranges
    assert p.y0.dtype == p.x0.dtype == p.flip.dtype == np.int32 and p.image_gain.dtype == p.image_bias.dtype == np.float32
    assert p.y0.shape == p.x0.shape == p.flip.shape == p.image_bias.shape == (16,) and p.image_gain.shape == (16, 8) and p.out_size == (64, 96)
    big = a.params_at(0, 4096, 96, 128)
    assert big.y0.min() == -5 and big.y0.max() == 96 - 64 + 5 and big.x0.min() == -9 and big.x0.max() == 128 - 96 + 9
    assert set(big.flip.tolist()) == {0, 1} and 0.45 < big.flip.mean() < 0.55
    assert np.all(np.abs(big.image_bias) <= 0.2) and big.image_gain.min() >= np.float32(0.7 * 0.9) and big.image_gain.max() <= np.float32(1.3 * 1.1)
    assert not np.any(big.drop_lidar & big.drop_image) and 0.25 < big.drop_lidar.mean() < 0.35 and 0.25 < big.drop_image.mean() < 0.35
    # a window as large as (or larger than) the source starts at 0 and only shifts
    same_size = BatchAugment(translate=(2, 0), seed=1).params_at(0, 512, 96, 128)
    assert same_size.out_size == (96, 128) and set(same_size.y0.tolist()) == {-2, -1, 0, 1, 2} and not same_size.x0.any()
    larger = BatchAugment(out_size=(128, 160), seed=1).params_at(0, 8, 96, 128)
    assert not larger.y0.any() and not larger.x0.any()


def test_flip_dropout_and_identity_parameters(lib):
    from dmmfods_amd.augment import BatchAugment
    B = 64
    assert BatchAugment(hflip=1.0).params_at(5, B, 32, 32).flip.tolist() == [1] * B
    assert BatchAugment(hflip=0.0, translate=(1, 1)).params_at(5, B, 32, 32).flip.tolist() == [0] * B
    p = BatchAugment(lidar_dropout=1.0).params_at(2, B, 32, 32)
    gain, bias = BatchAugment.channel_tables(p, 3, 1, 3)
    assert gain.dtype == bias.dtype == np.float32 and gain.shape == bias.shape == (B, 7)
    assert np.all(gain[:, 3] == 0) and np.all(gain[:, :3] == 1) and np.all(gain[:, 4:] == 1) and not bias.any()
    gain, bias = BatchAugment.channel_tables(p, 3, 0, 3)            # no LiDAR tensor in the call: nothing to blank
    assert gain.shape == (B, 6) and np.all(gain == 1) and not bias.any()
    p = BatchAugment(image_dropout=1.0, brightness=0.5, contrast=0.5).params_at(2, B, 32, 32)
    gain, bias = BatchAugment.channel_tables(p, 3, 1, 3)
    assert not gain[:, :3].any() and not bias.any() and np.all(gain[:, 3:] == 1)
    # all strengths zero: the identity, whatever the seed
    p = BatchAugment(seed=11, rank=4).params_at(9, B, 48, 80)
    gain, bias = BatchAugment.channel_tables(p, 3, 1, 3)
    assert not p.y0.any() and not p.x0.any() and not p.flip.any() and np.all(gain == 1) and not bias.any() and p.out_size == (48, 80)
    assert not p.drop_lidar.any() and not p.drop_image.any()
    # the image's gain is contrast x per-channel, its bias one draw per sample; targets are never touched
    p = BatchAugment(brightness=0.3, contrast=0.4, channel_gain=0.2, seed=3).params_at(0, B, 32, 32)
    gain, bias = BatchAugment.channel_tables(p, 3, 1, 3)
    assert np.array_equal(gain[:, :3], p.image_gain[:, :3]) and np.all(bias[:, :3] == p.image_bias[:, None]) and len(set(p.image_bias.tolist())) == B
    assert np.all(gain[:, 3:] == 1) and not bias[:, 3:].any() and len(set(gain[:, :3].ravel().tolist())) == 3 * B
    with pytest.raises(ValueError):
        BatchAugment.channel_tables(p, 4, 2, 3)


def test_state_dict_round_trip_continues_the_sequence(lib):
    from dmmfods_amd.augment import BatchAugment
    kw = dict(hflip=0.5, translate=(3, 3), contrast=0.2)
    a = BatchAugment(seed=5, rank=2, **kw)
    assert a.state_dict() == {"seed": 5, "rank": 2, "batches_drawn": 0}
    a.batches_drawn = 17                                               # (what 17 calls leave behind; a call itself needs the device)
    st = a.state_dict()
    assert st == {"seed": 5, "rank": 2, "batches_drawn": 17}
    b = BatchAugment(**kw)
    b.load_state_dict(json.loads(json.dumps(st)))
    assert b.state_dict() == st and _same(b.params_at(b.batches_drawn, 8, 32, 32), a.params_at(17, 8, 32, 32))
    assert not _same(b.params_at(b.batches_drawn, 8, 32, 32), BatchAugment(**kw).params_at(17, 8, 32, 32))   # seed and rank came along


# ------------------------------------------------------------------------------------------------ the agent's config field
def test_agent_reads_the_config_field_only_if_present(lib):
    from dmmfods_amd.agents.Dense_U_Net_lidar_Agent import Dense_U_Net_lidar_Agent as Agent
    from dmmfods_amd.utils.Dense_U_Net_lidar_helper import get_config
    cfg = get_config("/tmp/dmm_test")
    assert Agent._optional(cfg.loader, "augment") is None and Agent._make_augment(None) is None
    aug = Agent._make_augment({"out_size": (64, 96), "hflip": 0.5, "seed": 9})
    assert aug.out_size == (64, 96) and aug.hflip == 0.5 and aug.seed == 9 and aug.rank == 0 and aug.batches_drawn == 0
    assert Agent._make_augment({"rank": 3}).rank == 3 and Agent._make_augment({}).out_size is None
    for bad in ({"out_size": (64, 100)}, {"out_size": (48, 96)}, {"out_size": 16}, {"hflip": 2.0}, {"lidar_dropout": 0.7, "image_dropout": 0.7}):
        with pytest.raises(ValueError):
            Agent._make_augment(bad)
    with pytest.raises(TypeError):
        Agent._make_augment({"rotate": 10})                            # (left out on purpose: DESIGN 7)


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
    return r.stdout.splitlines()


def test_harness_drives_the_entry_point_and_leaves_the_pinned_trace_alone(drive):
    """DRIVE_AUGMENT=1: behind the plan's life the stand-alone driver makes one valid call with 33 samples (operands that are addresses
    only) - exactly two launches - and tries every refusal, under ASan + UBSan.  Without the switch the row keeps its pinned hash."""
    args = "tiny_mid f16 2 64 96 2"
    base = [ln for ln in _run(drive, {}, args) if ln.startswith("T ")]
    pinned = json.load(open(os.path.join(ROOT, "tests", "golden", "enqueue_trace_sha256.json")))
    assert hashlib.sha256("\n".join(base).encode()).hexdigest() == pinned["(none) | " + args]
    out = _run(drive, {"DRIVE_AUGMENT": "1"}, args)
    assert "AUGMENT OK" in out and "AUGMENT 33 samples: 2 launches, grid 2 x 7 ok" in out, out[-12:]
    trace = [ln for ln in out if ln.startswith("T ")]
    assert trace[:len(base)] == base                                # the plan's schedule is untouched ...
    extra = trace[len(base):]                                       # ... and behind it: the two launches, nothing else
    assert len(extra) == 2 and all(ln.startswith("T launch") and "augment_kernel" in ln for ln in extra), extra
    assert [tuple(map(int, ln.split()[3:5])) for ln in extra] == [(2, 7), (2, 7)]
