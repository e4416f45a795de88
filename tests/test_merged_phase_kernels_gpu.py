"""Exact parity of the decoder's ConvTranspose stages as the benchmarked plans run them: the four output-parity phases (1, 2, 2 and 4
taps) in ONE launch, forward and weight gradient.

dmm_conv_forward and dmm_conv_wgrad_ex launch each parity on its own, so tests/test_exact_kernels_gpu.py and
tests/test_rounding_kernels_gpu.py never reach
  cvp.hip   cvp_multi_kernel (three and more channel groups): blockIdx -> (xcd, slot, j) -> tile, the early return for the rounding
            of per8, the order[] permutation (most taps first), the per-phase weights / taps / parity / tap-box origin;
  cvw.hip   cvw_kernel with nphase = 4 (one or two channel groups): the round-robin start of every phase, the phase records sorted
            by cvw_resolve, the BatchNorm sums flushed at every phase end into the same channels;
  wgpw.hip  wgpw_multi_kernel: blockIdx -> (unit, phase), units rounded up to groups of 8 whose surplus must do nothing, the
            per-phase taps / gradient parity / packed gradient, 64 output channels per workgroup in every phase;
  plan.h    the merge itself: which per-phase records may join, what is copied into the merged record, whether the pick accepts it.
dmm_conv_forward_merged / dmm_conv_wgrad_merged (capi.cpp) fill the four per-phase records as those entry points do, pick each, and
merge them with the SAME functions the plan builder calls (plan.h; plan.cpp merge_last_four_phases) - so what runs here is the launch
a plan builds, and the entry point reports whether it became one launch or stayed four.

On the exact operands (tools/exact_operands.py) every sum is exact in fp32 in any order: output, both BatchNorm sums and the weight
gradient must EQUAL the fp64 reference - a dropped tile at a ragged border, a workgroup that walks an item twice, a statistic counted
once too often at a phase boundary, a surplus unit that adds into the packed gradient is a nonzero difference.  Outputs lie between
guard bands of NaN and start as NaN.  The operands' conditions are asserted before anything is launched and, without a GPU, in
tests/test_exact_operands_cpu.py and tests/test_rounding_operands_cpu.py (which also hold the launcher arithmetic for 256 compute
units); tests/test_host_cpu.py pins, under a fake runtime, which form resolves for every shape of this file.

Every case asserts the number of launches, exactly the families that noted them, and the launcher arithmetic that makes the case
meaningful, recomputed from the formulas of cvp_resolve, cvw_resolve (256 compute units: DESIGN_CUS) and wgp_split (the device's).

Where this file departs from what was first proposed for it, after reading the launchers: the weight gradient under the deferred
correction stays four launches, but not all on wgp - wgp.hip has no one-tap form for a gradient that carries q and r (wgp_resolve),
so the (0, 0) phase runs on the generic kernel and the other three on wgp.hip's own kernel.  The case asserts exactly that.

Not here: the head's launches (hf, conv3's merged form, wgp.hip's own multi-phase kernel with four taps per phase), which need a
two-segment descriptor no entry point has."""
import ctypes as C

import pytest
import torch

from tools import exact_operands as E

pytestmark = pytest.mark.gpu
DT = [1, 2]
DT_IDS = ["fp16", "bf16"]
FWD_FAMILIES = {"cvw": {"cvp", "cvw"}, "cvp": {"cvp"}}       # the dispatcher notes the family, cvp_launch the form beside it
WGPW = {"wgp", "wgpw"}


@pytest.fixture(scope="module")
def lab():
    assert torch.cuda.is_available()
    from tools import gpu_lab
    return gpu_lab


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count   # wgp_split asks the device


def _fwd_id(f, c):
    return f"{f}-{c[0].replace(' ', '_')}"


def _forward_geometry(case):
    """The launcher arithmetic a merged forward case is there for."""
    form, c, _ = E.FORWARD_MERGED[case]
    _, B, H, W, Cin, Cout = c[:6]
    g = E.merged_fwd_geometry(form, B, H, W, Cin, Cout)
    assert Cin % 128 == 0 and Cout % 128 == 0
    if form == "cvw":
        assert g["groups"] <= 2, "more than two channel groups stay off cvw"
        assert len(set(g["done_mod"])) == 4, "two phases start at the same workgroup"
        if case == 0:
            assert g["nwg"] < E.DESIGN_CUS and g["per"] < g["nwg"] and g["done_mod"] == [0, 2, 4, 6], g
        else:
            assert g["nwg"] == E.DESIGN_CUS and g["per"] > g["nwg"] and g["per"] % g["nwg"] != 0, "no workgroup walks / every walk has the same length"
            assert H % 8 != 0 and W % 16 != 0, "whole tiles only"
        if case == 2:
            assert g["groups"] == 2 and g["ntn"] == 2, "one channel group / one column tile"
    else:
        assert g["groups"] > 2
        if case == 3:
            assert g["per8"] == 1 and g["idle"] == 0
        else:
            assert g["per"] % 8 != 0 and g["per8"] == 2 and g["idle"] == 4 * (8 * g["per8"] - g["per"]) > 0, "no workgroup exits at once"
    return form, c


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("case", range(len(E.FORWARD_MERGED)), ids=[_fwd_id(f, c) for f, c, _ in E.FORWARD_MERGED])
def test_merged_forward_output_and_statistics_are_exact(lab, case, dtype):
    form, c = _forward_geometry(case)
    assert lab.conv_case(c[0] + " merged", dtype, 1, *c[1:], exact=True, parts=("fwd",), merged=True, expect_launches=1,
                         expect_fwd=FWD_FAMILIES[form])


# ------------------------------------------------------------------------------------------------ weight gradient
def _wgrad_geometry(case, cus):
    B, H, W, Cin, Cout = E.BACKWARD_MERGED[case][0]
    g = E.merged_wgrad_geometry(B, H, W, Cin, Cout, cus)
    assert Cin % 128 == 0 and Cout % 64 == 0 and g["nwg"] == 4 * 8 * ((g["units"] + 7) // 8)
    if case == 0:
        assert g["units"] == 8 and g["nwg"] == 32, ("idle units", g)
    elif case == 1:
        assert g["units"] == 3 and g["nwg"] == 32, ("not 5 idle units per phase", g)
    else:
        assert g["tiles_per_wg"] > 1 and g["ntiles"] % g["tiles_per_wg"] != 0 and g["units"] % 8 != 0, g
    return B, H, W, Cin, Cout


def _wname(B, H, W, Cin, Cout):
    return f"3x3 {Cin}->{Cout} {B}x{H}x{W} convT merged"


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("case", range(len(E.BACKWARD_MERGED)), ids=["{3}to{4}-{0}x{1}x{2}".format(*s) for s, _ in E.BACKWARD_MERGED])
def test_merged_weight_gradient_is_exact(lab, cus, case, dtype):
    B, H, W, Cin, Cout = _wgrad_geometry(case, cus)
    assert lab.backward_case(_wname(B, H, W, Cin, Cout), dtype, B, H, W, Cin, Cout, 3, 3, 1, transposed=1, with_q=0, acc=0, what="wgrad",
                             exact=True, merged=True, expect_launches=1, expect=WGPW)


# ------------------------------------------------------------------------------------------------ kept apart
@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
def test_forward_with_64_input_channels_stays_four_launches(lab, dtype):
    """cvp refuses 64 input channels: every phase is picked as the generic kernel's, the merge is not eligible, the result is exact."""
    c = E.FORWARD_APART
    assert c[4] == 64
    assert lab.conv_case(c[0] + " apart", dtype, 1, *c[1:], exact=True, parts=("fwd",), merged=True, expect_launches=4, expect_fwd={"generic"})


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
def test_weight_gradient_under_the_deferred_correction_stays_four_launches(lab, dtype):
    """q and r on the gradient: the one-tap phase is the generic kernel's (wgp.hip has no one-tap form with the correction), so the
    merge is not eligible; the 2- and 4-tap phases run on wgp.hip's own kernel, never on wgpw.hip."""
    B, H, W, Cin, Cout = E.BACKWARD_APART
    assert lab.backward_case(_wname(B, H, W, Cin, Cout) + " q", dtype, B, H, W, Cin, Cout, 3, 3, 1, transposed=1, with_q=1, acc=0, what="wgrad",
                             exact=True, merged=True, expect_launches=4, expect={"generic", "wgp"})


# ------------------------------------------------------------------------------------------------ run to run
def test_merged_forward_is_reproducible(lab):
    """The 1056-item cvw walk twice: output and fp64-atomic statistics equal bit for bit (sums of exact operands do not depend on order)."""
    form, c = _forward_geometry(E.FORWARD_MERGED_REPRO)
    runs = [{}, {}]
    for keep in runs:
        assert lab.conv_case(c[0] + " again", 1, 1, *c[1:], exact=True, parts=("fwd",), merged=True, expect_launches=1,
                             expect_fwd=FWD_FAMILIES[form], keep=keep)
    assert torch.equal(runs[0]["y"].view(torch.int16), runs[1]["y"].view(torch.int16))
    assert torch.equal(runs[0]["stats"].view(torch.int64), runs[1]["stats"].view(torch.int64))


def test_phase_boundary_keeps_the_halo_images_apart(lab):
    """What this file found in cvw.hip: every phase of the four-phase walk began its halo double buffer at image 0, so a workgroup
    whose phase had an odd number of channel groups wrote the NEXT phase's first halo into the image its matrix waves could still be
    reading for the last stage of that phase - nothing but the double buffering orders the two (the loaders run ahead behind the
    phase's last barrier).  On this shape (one channel group, one item per phase for 248 of the 256 workgroups) 5 of 24 launches
    stored wrong tiles, always a band of one loader wave's pixels in a tile of the second phase; since the image parity is carried
    across the phases, 80 of 80 were exact.  A race is not shown by one launch: the case runs eight times."""
    form, c = _forward_geometry(E.FORWARD_MERGED_REPRO)
    g = E.merged_fwd_geometry(form, *c[1:6])
    items = lambda p, b: len(range(g["first"][p][b], g["per"], g["nwg"]))  # noqa: E731
    exposed = sum(1 for b in range(g["nwg"]) for p in range(3) if (items(p, b) * g["groups"]) % 2 == 1 and items(p + 1, b) > 0)
    assert exposed > g["nwg"], "no workgroup ends a phase on halo image 0 with another phase to come"
    for run in range(8):
        assert lab.conv_case(f"{c[0]} run {run}", 1, 1, *c[1:], exact=True, parts=("fwd",), merged=True, expect_launches=1,
                             expect_fwd=FWD_FAMILIES[form])


def test_merged_weight_gradient_is_reproducible(lab, cus):
    """The 52-unit weight gradient twice: fp32 atomics into the packed gradient on exact operands do not depend on order."""
    B, H, W, Cin, Cout = _wgrad_geometry(E.BACKWARD_MERGED_REPRO, cus)
    runs = [{}, {}]
    for keep in runs:
        assert lab.backward_case(_wname(B, H, W, Cin, Cout) + " again", 1, B, H, W, Cin, Cout, 3, 3, 1, transposed=1, with_q=0, acc=0,
                                 what="wgrad", exact=True, merged=True, expect_launches=1, expect=WGPW, keep=keep)
    assert torch.equal(runs[0]["dw"].view(torch.int32), runs[1]["dw"].view(torch.int32))


# ------------------------------------------------------------------------------------------------ single rounding
@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("case", range(len(E.ROUND_FORWARD_MERGED)), ids=[_fwd_id(f, c) for f, c, _ in E.ROUND_FORWARD_MERGED])
def test_merged_forward_rounds_once(lab, case, dtype):
    """Every 16-bit store of the merged launch is ONE rounding of conv(a, w_T); stat_sum is the sum of the output as stored."""
    form, c, kw = E.ROUND_FORWARD_MERGED[case]
    assert lab.conv_case(c[0] + " merged", dtype, 1, *c[1:], exact="round", parts=("fwd",), merged=True, expect_launches=1,
                         expect_fwd=FWD_FAMILIES[form], exact_kw=kw)


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
def test_merged_weight_gradient_of_once_rounded_operands(lab, dtype):
    """wgpw_multi_kernel: sums of the once-rounded activation times the gradient (bit for bit where exact in fp32, else within the bound
    derived from the reference, as tests/test_rounding_kernels_gpu.py)."""
    for B, H, W, Cin, Cout in E.ROUND_BACKWARD_MERGED:
        assert lab.backward_case(_wname(B, H, W, Cin, Cout), dtype, B, H, W, Cin, Cout, 3, 3, 1, transposed=1, with_q=0, acc=0, what="wgrad",
                                 exact="round", merged=True, expect_launches=1, expect=WGPW)


# ------------------------------------------------------------------------------------------------ refusals
BAD = [   # entry point, what is wrong: a descriptor field changed from a good one, a null pointer, or q / r / yfwd not given together
    ("fwd", "not-transposed", dict(transposed=0, stride=1), None),
    ("fwd", "null-x", {}, "x"),
    ("fwd", "null-w", {}, "w"),
    ("fwd", "null-y", {}, "y"),
    ("fwd", "null-scratch", {}, "scratch"),
    ("fwd", "null-launches", {}, "launches"),
    ("fwd", "null-scale", {}, "scale"),
    ("wgrad", "not-transposed", dict(transposed=0, stride=1), None),
    ("wgrad", "null-x", {}, "x"),
    ("wgrad", "null-dy", {}, "dy"),
    ("wgrad", "null-dw", {}, "dw"),
    ("wgrad", "null-scratch", {}, "scratch"),
    ("wgrad", "null-launches", {}, "launches"),
    ("wgrad", "q-without-r", {}, "r"),
    ("wgrad", "r-without-q", {}, "q"),
    ("wgrad", "q-r-without-yfwd", {}, "yfwd"),
    ("wgrad", "yfwd-alone", {}, "q,r"),
]


@pytest.mark.parametrize("entry,what,change,null", BAD, ids=[f"{b[0]}-{b[1]}" for b in BAD])
def test_entry_points_refuse(entry, what, change, null):
    """DMM_ERR_INVALID with a message that names the entry point, nothing launched (no family noted), every output still all NaN, the
    launch count untouched."""
    from dmmfods_amd import _lib
    L = _lib.lib()
    f = dict(dtype=1, use_mfma=1, B=1, H=8, W=16, Cin=128, Cout=64, R=3, S=3, stride=2, pad=1, transposed=1, mode=0, bn_relu=1)
    good = _lib.ConvDesc(**f)
    f.update(change)
    d = _lib.ConvDesc(**f)
    dev = "cuda"
    scratch = torch.zeros(max(L.dmm_conv_scratch_bytes(C.byref(good)), L.dmm_conv_scratch_bytes(C.byref(d))), dtype=torch.uint8, device=dev)
    x = torch.zeros(1, 8, 16, 128, dtype=torch.float16, device=dev)
    big = torch.full((1, 16, 32, 64), float("nan"), dtype=torch.float16, device=dev)     # y (forward) / dy, yfwd (weight gradient)
    w = torch.full((128 * 64 * 9,), float("nan"), device=dev)                               # w (forward, never read) / dw
    stats = torch.full((128,), float("nan"), dtype=torch.float64, device=dev)
    scale, shift, qr = torch.ones(128, device=dev), torch.zeros(3 * 128, device=dev), torch.zeros(2 * 64, device=dev)
    nl = C.c_int(-7)
    p = dict(x=x.data_ptr(), w=w.data_ptr(), y=big.data_ptr(), dy=big.data_ptr(), yfwd=big.data_ptr(), dw=w.data_ptr(), scale=scale.data_ptr(),
             shift=shift.data_ptr(), q=qr.data_ptr(), r=qr[64:].data_ptr(), scratch=scratch.data_ptr(), launches=C.byref(nl))
    if entry == "wgrad" and null not in ("r", "q", "yfwd", "q,r"):
        p.update(q=None, r=None, yfwd=None)
    for k in (null.split(",") if null else []):
        p[k] = None
    _lib.impls_since_reset()
    if entry == "fwd":
        rc = L.dmm_conv_forward_merged(C.byref(d), p["x"], p["w"], p["scale"], p["shift"], p["y"], stats.data_ptr(), p["scratch"],
                                       _lib.stream_ptr(), p["launches"])
    else:
        rc = L.dmm_conv_wgrad_merged(C.byref(d), p["x"], p["dy"], p["scale"], p["shift"], p["yfwd"], p["q"], p["r"], p["dw"], p["scratch"],
                                     _lib.stream_ptr(), p["launches"])
    torch.cuda.synchronize()
    name = b"dmm_conv_forward_merged" if entry == "fwd" else b"dmm_conv_wgrad_merged"
    assert rc == _lib.ERR_INVALID and name in L.dmm_last_error()
    assert _lib.impls_since_reset() == set() and nl.value == -7
    assert bool(torch.isnan(big).all()) and bool(torch.isnan(w).all()) and bool(torch.isnan(stats).all())
    assert int(scratch.count_nonzero()) == 0
