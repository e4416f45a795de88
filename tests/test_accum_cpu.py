"""Gradient accumulation without a GPU: the C entry point's contract, the Python surface on a CPU-resident model, and the library's
host code driven through a window of micro-batches under AddressSanitizer + UBSan (tools/hoststub, `drive accum`)."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from dmmfods_amd import _lib
    return _lib


def _desc(lib, dtype=1):
    d = lib.ModelDesc(growth_rate=8, num_blocks=4, num_init_features=16, bn_size=4, num_classes=3, concat_before_block_num=3,
                      stream_1_in_channels=3, stream_2_in_channels=3, batch=2, height=64, width=96, dtype=dtype, loss_scale=1.0,
                      bn_momentum=0.1, bn_eps=1e-5, iou_threshold=0.7, use_mfma=1)
    for i in range(4):
        d.block_config[i] = 2
    return d


def _tiny_model():
    from dmmfods_amd.graphs.models.Dense_U_Net_lidar import Dense_U_Net_lidar
    from dmmfods_amd.utils.Dense_U_Net_lidar_helper import get_config
    cfg = get_config("/tmp/dmm_test")
    cfg.model.growth_rate, cfg.model.block_config, cfg.model.num_init_features = 8, (2, 2, 2, 2), 16
    cfg.model.concat_before_block_num, cfg.model.stream_2_in_channels = 3, 3
    return Dense_U_Net_lidar(cfg, compute_dtype="fp32")


def test_null_plan_is_refused(lib):
    L = lib.lib()
    assert L.dmm_plan_set_grad_accumulate(None, 1) == lib.ERR_INVALID
    assert b"null plan" in L.dmm_last_error()


def test_setter_on_an_unbound_plan_keeps_the_launch_list(lib):
    """The mode is a run-time property of one launch list: the setter succeeds before dmm_plan_bind, may be called again with the
    same value, and dmm_plan_profile_num_ops answers the same in both modes (the GPU tests ask a bound plan the same question)."""
    L = lib.lib()
    h = C.c_void_p()
    lib.check(L.dmm_plan_create(C.byref(_desc(lib)), C.byref(h)))
    try:
        counts = {}
        for on in (0, 1, 1, 0):
            assert L.dmm_plan_set_grad_accumulate(h, on) == 0
            counts.setdefault(on, set()).add((L.dmm_plan_profile_num_ops(h, 0), L.dmm_plan_profile_num_ops(h, 1)))
        assert counts[0] == counts[1] and len(counts[0]) == 1, counts
    finally:
        lib.check(L.dmm_plan_destroy(h))


def test_header_and_library_export_the_same_symbols(lib):
    hdr = open(os.path.join(ROOT, "include", "dmmfods_hip.h")).read()
    declared = set(re.findall(r"\b(dmm_[a-z0-9_]+)\s*\(", hdr)) - {"dmm_status"}
    assert "dmm_plan_set_grad_accumulate" in declared and "dmm_plan_set_grad_accumulate" in lib.EXPORTS
    L = lib.lib()
    assert not [s for s in sorted(declared) if not hasattr(L, s)]
    assert set(lib.EXPORTS) <= declared
    nm = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (dmm_[a-z0-9_]+)$", nm, re.M))
    assert exported == declared, (sorted(exported - declared), sorted(declared - exported))
    assert "fully overwritten" not in hdr


def test_zero_grad_clears_only_while_the_mode_is_on(lib):
    """A CPU-resident model (before .to("cuda")): set_grad_accumulation returns the model and needs no plan; FusedAdam.zero_grad()
    zeroes a non-zero arena while the mode is on and stays the no-op it was with the mode off."""
    from dmmfods_amd.optim import FusedAdam
    model = _tiny_model()
    assert model.grad_accumulation is False
    opt = FusedAdam(model)
    model.grad_arena.fill_(3.0)
    opt.zero_grad()
    assert float(model.grad_arena.min()) == 3.0 and float(model.grad_arena.max()) == 3.0
    assert model.set_grad_accumulation(True) is model and model.grad_accumulation is True
    assert model.grad_arena.device.type == "cpu"
    opt.zero_grad()
    assert int(torch.count_nonzero(model.grad_arena)) == 0 and model.grad_arena.numel() == model.num_params
    model.grad_arena.fill_(2.0)
    opt.zero_grad(set_to_none=True)          # the signature of torch's zero_grad; .grad stay views of the arena
    assert int(torch.count_nonzero(model.grad_arena)) == 0
    assert model.set_grad_accumulation(False) is model
    model.grad_arena.fill_(5.0)
    opt.zero_grad()
    assert float(model.grad_arena.min()) == 5.0


@pytest.fixture(scope="module")
def host_drive():
    """tools/hoststub: the library's host code built for the CPU with AddressSanitizer + UBSan against a fake HIP runtime, and its
    driver - a stand-alone program, nothing is loaded into Python."""
    out = os.path.join(ROOT, "tools", "hoststub", "_build")
    subprocess.run([os.path.join(ROOT, "tools", "hoststub", "build.sh"), out], check=True, capture_output=True, timeout=900)
    return os.path.join(out, "drive")


ACCUM_CASES = [
    ("g8_mid", "f32", 2, 64, 96, {}),                              # generic unpack, fp32
    ("tiny_mid", "bf16", 2, 96, 160, {}),                          # tile unpack
    ("tiny_mid", "f16", 2, 96, 160, {"DMM_NO_PACK_TILES": "1"}),   # generic unpack in 16-bit storage
    ("d121e", "f16", 2, 64, 96, {}),
]


def test_a_window_of_micro_batches_under_sanitizers(host_drive):
    """`drive accum`: create -> mode on -> bind (the mode survives) -> two training passes without a clear in between -> mode off -> one
    more pass -> mode on -> external-gradient backward -> destroy.  No sanitizer report; every device pointer inside the caller's
    regions; the fake runtime executes memsets, so the gradient arena (filled with a pattern) keeps the pattern while the mode is on
    and reads as zero behind the pass with the mode off; both modes make the same launches from the same, unmodified records."""
    for arch, dtype, b, h, w, envx in ACCUM_CASES:
        env = {k: v for k, v in os.environ.items() if not k.startswith("DMM_") and not k.startswith("DRIVE_")}
        env.update(envx, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        r = subprocess.run([host_drive, "accum", arch, dtype, str(b), str(h), str(w)], env=env, capture_output=True, text=True, timeout=600)
        tail = (r.stdout + r.stderr)[-3000:]
        assert r.returncode == 0 and "ACCUM OK" in r.stdout, (arch, dtype, envx, tail)
        assert "WRONG" not in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, tail
        checks = [ln for ln in r.stdout.splitlines() if ln.startswith("ACCUM ") and ln.endswith(" ok")]
        assert len(checks) == 5, tail
