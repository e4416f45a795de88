"""Exact parity of the logits launch - the network's last convolution (dec_out_to_heat_maps.refine1: 5x5, 64 -> classes, behind
BN+ReLU, fp32 NCHW output) - on each of the three kernels that write logits, through dmm_conv_logits, which builds the launch
plan.cpp builds:

  thin.hip  thin_logits_kernel<T, 2, KN>, KN = 1, 2, 3, f16 and bf16: the strip walk (124 output columns per 128 input columns), the
            row split of thin_resolve, the ring of 6 output rows with its wrap-around and its drain step, zero padding applied AFTER
            BN+ReLU, xcd_remap on a grid that is no multiple of 8;
  halo.hip  the EPI_LOGITS branch, f16 (4 classes, which thin has no instantiation for; 32 input channels, the head of every small
            test network; thin switched off) and fp32 (3x3);
  igemm.hip the EPI_LOGITS epilogue: bf16 where thin refuses, fp32 5x5 (MFMA and scalar), the N = 8 tail, the f16 scalar kernel.

A logits launch stores fp32, so nothing ever rounds on the exact operands (tools/exact_operands.py, part "logits"): every logit must
EQUAL the fp64 reference.  On the single-rounding operands the only rounding points are the weight pack and the BN+ReLU prologue
(kinds "weights" and "main"); the logits are compared unrounded.  The output tensor lies between two guard bands of NaN and starts
as NaN itself: an element never written, or one written outside the tensor, fails the case.  The operands' conditions - among them
that the reference differs on every image's border from a convolution that normalises its padding - are asserted before anything is
launched and, without a GPU, in tests/test_logits_operands_cpu.py, which also holds the launcher arithmetic of every case.
Every case asserts the kernel family that ran."""
import ctypes as C

import pytest
import torch

from tools import exact_operands as E

pytestmark = pytest.mark.gpu
IDS = [E.logits_id(f, dt, m, off, s) for f, dt, m, off, s, _ in E.LOGITS]


@pytest.fixture(scope="module")
def lab():
    assert torch.cuda.is_available()
    from tools import gpu_lab
    return gpu_lab


@pytest.fixture
def thin_switch():
    """Switches the thin family off on request and back on afterwards, whatever happened."""
    from dmmfods_amd import _lib
    L = _lib.lib()
    try:
        yield lambda off: _lib.check(L.dmm_set_option(b"thin_logits", 0 if off else 1))
    finally:
        _lib.check(L.dmm_set_option(b"thin_logits", 1))


@pytest.mark.parametrize("case", range(len(E.LOGITS)), ids=IDS)
def test_logits_are_exact(lab, thin_switch, case):
    family, dtype, mfma, thin_off, s, _ = E.LOGITS[case]
    B, H, W = s[:3]
    if family == "thin":
        want = [g for t, g, _ in E.LOGITS_THIN if t == (B, H, W, s[4])][0]
        got = E.thin_geometry(B, H, W)
        assert {k: got[k] for k in want} == want
    if (B, H, W) == E.LOGITS_HALO_WALK:
        cus = torch.cuda.get_device_properties(0).multi_processor_count     # halo.hip asks the device
        ntiles = E.halo_tiles(B, H, W)
        assert ntiles > cus and ntiles % cus != 0, "no workgroup walks more than one tile / every walk has the same length"
    thin_switch(thin_off)
    assert lab.logits_case(IDS[case], dtype, mfma, *s, exact=True, expect=family)


@pytest.mark.parametrize("kind", E.ROUND_LOGITS_KINDS)
@pytest.mark.parametrize("case", range(len(E.ROUND_LOGITS)), ids=[E.logits_id(f, dt, 1, off, s) for f, dt, off, s in E.ROUND_LOGITS])
def test_logits_round_only_in_pack_and_prologue(lab, thin_switch, case, kind):
    """kind "main": the activation is ONE rounding of relu(x * scale + shift); "weights": the kernel multiplies by rnd(w)."""
    family, dtype, thin_off, s = E.ROUND_LOGITS[case]
    thin_switch(thin_off)
    assert lab.logits_case(E.logits_id(family, dtype, 1, thin_off, s) + " " + kind, dtype, 1, *s, exact="round", expect=family,
                           exact_kw=dict(kind=kind))


def test_thin_logits_are_reproducible(lab):
    """Two runs of the 36-workgroup thin case (a grid that is no multiple of 8) are equal bit for bit."""
    runs = [{}, {}]
    for keep in runs:
        assert lab.logits_case("thin 3x37x255 again", 1, 1, *E.LOGITS_REPRO, exact=True, expect="thin", keep=keep)
    assert torch.equal(runs[0]["logits"].view(torch.int32), runs[1]["logits"].view(torch.int32))


BAD = [   # what dmm_conv_logits refuses: descriptor fields changed from a good one, or a null pointer
    ("transposed", dict(transposed=1, R=3, S=3, stride=2, pad=1), None),
    ("upsampled", dict(mode=1), None),
    ("pooled", dict(mode=2), None),
    ("stride2", dict(stride=2), None),
    ("33classes", dict(Cout=33), None),
    ("null-x", {}, "x"),
    ("null-w", {}, "w"),
    ("null-logits", {}, "logits"),
    ("null-scratch", {}, "scratch"),
    ("null-scale", {}, "scale"),
]


@pytest.mark.parametrize("what,change,null", BAD, ids=[b[0] for b in BAD])
def test_entry_point_refuses(what, change, null):
    """DMM_ERR_INVALID with a message, nothing launched (no family noted), the output tensor still all NaN."""
    from dmmfods_amd import _lib
    L = _lib.lib()
    f = dict(dtype=1, use_mfma=1, B=1, H=9, W=13, Cin=64, Cout=3, R=5, S=5, stride=1, pad=2, transposed=0, mode=0, bn_relu=1)
    good = _lib.ConvDesc(**f)
    f.update(change)
    d = _lib.ConvDesc(**f)
    dev = "cuda"
    scratch = torch.zeros(max(L.dmm_conv_scratch_bytes(C.byref(good)), L.dmm_conv_scratch_bytes(C.byref(d))), dtype=torch.uint8, device=dev)
    x = torch.zeros(1, 18, 26, 64, dtype=torch.float16, device=dev)            # (room for the stride-2 / upsampled readings of the shape)
    w = torch.zeros(64 * 64 * 25, device=dev)
    scale, shift = torch.ones(64, device=dev), torch.zeros(64, device=dev)
    out = torch.full((4 * 64 * 18 * 26,), float("nan"), device=dev)
    p = dict(x=x.data_ptr(), w=w.data_ptr(), scale=scale.data_ptr(), shift=shift.data_ptr(), logits=out.data_ptr(), scratch=scratch.data_ptr())
    if null:
        p[null] = None
    _lib.impls_since_reset()
    rc = L.dmm_conv_logits(C.byref(d), p["x"], p["w"], p["scale"], p["shift"], p["logits"], p["scratch"], _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == _lib.ERR_INVALID and b"dmm_conv_logits" in L.dmm_last_error()
    assert _lib.impls_since_reset() == set()
    assert bool(torch.isnan(out).all())
