"""Exact-operand parity of every convolution kernel family that has a single-kernel entry point.

The operands (tools/exact_operands.py) are small dyadic numbers: every product and every partial sum is exact in fp32 in any order,
and rounding to f16 / bf16 is the identity.  Each kernel must therefore equal an fp64 CPU reference (torch.nn.functional autograd
of the same op) BIT FOR BIT - outputs, BatchNorm statistics, data gradients, both BatchNorm-backward sums, weight gradients.  No
tolerance: a dropped row, a tile counted twice, a wrong tap or column, a padded lane that leaks is a nonzero difference.  The
conditions that make this so are asserted on the reference before anything is launched (Operands.check) and, without a GPU, for
every case of this file in tests/test_exact_operands_cpu.py.

Every case asserts the kernel family that ran and the launcher arithmetic that makes the case meaningful (for example that a
workgroup walks more than one tile), so that a later change to a launcher fails here instead of emptying the test.

fp32 chains of condition (c) - the stored values a kernel adds in fp32 before the partial reaches fp64 - as read off the kernels:
  pig, conv3 (forward), cvp, generic MFMA forward: a lane's 16 rows of one 32-row block, folded with the other lane half: 32
  cf, cvw: a lane's rows of one 8 x 16 tile, folded with the other lane half: at most 128
  generic scalar / fp32 forward and every generic data gradient: a thread's rows of a 128-row tile, folded over the lanes: 128
    (the pooled data gradient adds the 4 pixels of a pooling window per row: 512 - EXACT_KW)
  bw1: 4 rows per thread of a 64-row tile, folded over 4 lanes; conv3 EPI_BNBWD, cvd3: one 128-row tile at most
  wg5 (conv5_stats_case): the factor correlations are fp32 MFMA accumulators over a workgroup's whole walk - condition (b), not (c)
The cases use 128 (512 where noted), the upper bound of all of these.

Not here: hf.hip - no single-kernel entry point builds its launch, and hf is held bit-equal to conv3 inside a plan
(tests/test_timed_kernels_gpu.py); the logits launch (thin.hip, halo.logits, igemm.logits), which has a file of its own:
tests/test_logits_kernels_gpu.py; cvp_multi_kernel, cvw's four-phase walk and wgpw_multi_kernel - the ConvTranspose stages as ONE
launch of four output-parity phases, which dmm_conv_forward and dmm_conv_wgrad_ex never build (they launch each parity on its own) -
which have a file of their own: tests/test_merged_phase_kernels_gpu.py.  What still has none is the head: hf.hip, conv3.hip's
MULTI form and wgp.hip's own multi-phase path with four taps per phase (all need the head's two-segment launch), and cvd_kernel, the
lab fallback of cvd3 that only lab flags reach.

Where this file departs from the shapes first proposed for it, after reading the launchers:
  * dmm_conv_forward pads the output columns to a multiple of 32 only, and pig / cvp / cvw refuse Npad % 128 != 0: no case with a
    C_out that is not a multiple of 128 reaches them through this entry point (such a launch runs on the generic kernel, which the
    parity cases cover) - so there is no "column validity of the statistics" case for pig, and the cvw case has 256 output channels;
  * the same entry point launches cvw once per output parity with min(256, items) workgroups, items = pixel tiles x column tiles:
    the cvw cases have more than 256 items per parity (264 and 288), the smallest ragged maps that make a workgroup walk;
  * cf: 3 x 216 x 416 has 702 tiles per image, a multiple of the 9 tiles a workgroup walks - no walk would cross an image.  224 rows
    (728 tiles per image) do."""
import pytest
import torch

from tools import exact_operands as E

pytestmark = pytest.mark.gpu
DESIGN_CUS = 256          # common.h: cf, cvw and bw1 lay their launches out for the MI355X's 256 compute units
DT = [1, 2]
DT_IDS = ["fp16", "bf16"]


@pytest.fixture(scope="module")
def lab():
    assert torch.cuda.is_available()
    from tools import gpu_lab
    return gpu_lab


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count   # pig and conv3 ask the device


def cdiv(a, b):
    return (a + b - 1) // b


# ------------------------------------------------------------------------------------------------ forward
def _walks(family, c, cus):
    """The launcher arithmetic of a forward case: asserts that the path the case is there for is taken."""
    _, B, H, W, Cin, Cout, R, S, stride, pad, transposed, mode, bn = c
    if family == "pig":          # pig.hip pig_resolve / pig_launch
        M = B * H * W
        mtiles, ntiles = cdiv(M, 128), Cout // 128
        assert Cout % 128 == 0
        lds = 64 * 1024 + (4 * 2 * 128 * 4 + 2 * 128 * 8) + 2 * Cin * 4 + 16
        fit = 2 if lds <= 80 * 1024 else 1
        walkers = max(1, min(mtiles, fit * cus // ntiles))
        assert mtiles > walkers, "no workgroup walks more than one row tile"
        assert M % 128 != 0, "the last row tile is full"
        assert mtiles % walkers != 0, "every walk has the same length"
        assert Cin % 64 != 0, "no K tail"
        if Cin > 1278:
            assert fit == 1 and lds <= 160 * 1024
    elif family == "conv3":      # conv3.hip launch_c3: nwg capped at per_cu * CUs, per_cu <= 4
        Ho, Wo = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1
        assert B * cdiv(Ho, 8) * cdiv(Wo, 16) > 4 * cus, "one tile per workgroup"
        assert Ho % 8 != 0 and Wo % 16 != 0, "whole tiles only"
    elif family == "cf":         # cf.hip cf_resolve: whole 8 x 16 tiles, >= 8 per CU; 256 workgroups of `per` consecutive tiles
        assert H % 8 == 0 and W % 16 == 0
        per_image = (H // 8) * (W // 16)
        ntiles = B * per_image
        assert ntiles >= 8 * DESIGN_CUS
        per = cdiv(ntiles, DESIGN_CUS)
        assert ntiles % per != 0 and cdiv(ntiles, per) < DESIGN_CUS, "no short last walk / no workgroup without a tile"
        if B > 1:
            assert per_image % per != 0, "no walk crosses an image boundary"
    elif family == "cvw":        # cvw.hip cvw_resolve, one launch per output parity: min(256, items) workgroups
        assert Cin % 128 == 0 and Cin // 128 <= 2 and Cout % 128 == 0
        items = B * cdiv(H, 8) * cdiv(W, 16) * (Cout // 128)
        assert items > DESIGN_CUS, "one item per workgroup"
        assert items % DESIGN_CUS != 0 and H % 8 != 0 and W % 16 != 0
    elif family == "cvp":        # cvp.hip cvp_resolve: more than two channel groups stay off cvw
        assert Cin % 128 == 0 and Cin // 128 > 2 and Cout % 128 == 0 and H % 8 != 0 and W % 16 != 0
    else:
        assert family == "generic" and mode == 2


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("case", range(len(E.FORWARD)), ids=[f"{f}-{c[0].replace(' ', '_')}" for f, c, _ in E.FORWARD])
def test_forward_output_and_statistics_are_exact(lab, cus, case, dtype):
    family, c, kw = E.FORWARD[case]
    _walks(family, c, cus)
    assert lab.conv_case(c[0], dtype, 1, *c[1:], exact=True, parts=("fwd",), expect_fwd=family, exact_kw=kw.get(dtype))


# ------------------------------------------------------------------------------------------------ backward
def _bw1_geometry(M, Cin):
    """bw1.hip bw1_geometry."""
    nct, ntiles = cdiv(Cin, 128), cdiv(M, 64)
    nsplit = max(1, cdiv(2 * DESIGN_CUS, nct))
    nsplit = min(nsplit, max(1, ntiles // 4))
    per = cdiv(ntiles, nsplit)
    nsplit = cdiv(ntiles, per)
    xcd = nct > 1 and nsplit >= 32 and per >= 8
    nwg = cdiv(nsplit, 8) * 8 * nct if xcd else nsplit * nct
    return dict(nct=nct, ntiles=ntiles, tiles_per_wg=per, nsplit=nsplit, xcd_group=int(xcd), nwg=nwg)


def _backward_ids():
    out = []
    for i, (what, fam, s, qa) in enumerate(E.BACKWARD):
        for q, a in qa:
            out.append(pytest.param(i, q, a, id=f"{fam.split('/')[0 if q else -1]}-{what}-{s[3]}to{s[4]}-{s[0]}x{s[1]}x{s[2]}-q{q}a{a}"))
    return out


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("case,with_q,acc", _backward_ids())
def test_backward_gradients_and_sums_are_exact(lab, case, with_q, acc, dtype):
    what, family, (B, H, W, Cin, Cout, R, S, pad, transposed, mode), _ = E.BACKWARD[case]
    if family == "wgp/wgpw":     # the deferred correction on the gradient keeps the four-wave kernel; the materialised gradient: wgpw
        family = "wgp" if with_q else "wgpw"
    if family == "bw1" and B * H * W > 100000:
        g = _bw1_geometry(B * H * W, Cin)
        assert g == dict(nct=2, ntiles=1796, tiles_per_wg=8, nsplit=225, xcd_group=1, nwg=464), g
        assert g["nwg"] > g["nsplit"] * g["nct"], "no surplus workgroups"
        assert B * H * W - (g["ntiles"] - 1) * 64 == 41
    if family == "bw1" and B * H * W < 100000:
        assert Cin % 128 == 32, "no ragged channel slice"
    name = f"{R}x{S} {Cin}->{Cout} {B}x{H}x{W}" + (" convT" if transposed else (" up2" if mode == 1 else ""))
    assert lab.backward_case(name, dtype, B, H, W, Cin, Cout, R, S, pad, transposed=transposed, with_q=with_q, acc=acc, what=what,
                             mode=mode, expect=family, exact=True)


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
def test_stem_weight_gradient_is_exact(lab, dtype):
    """wg5.hip, 49 taps at stride 2 over the raw input (no BatchNorm in front), normal form - with the forward on conv3.hip."""
    c = E.STEM_WGRAD
    assert lab.conv_case(c[0], dtype, 1, *c[1:], exact=True, parts=("fwd", "wgrad"), expect_fwd="conv3", expect_wgrad="wg5")


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
def test_conv5_weight_gradient_and_sums_are_exact(lab, dtype):
    """dmm_conv5_wgrad_stats (wg5.hip PA = 3 + wg5_fin64_kernel) on a ragged map: weight gradient and both sums from the factor
    correlations, equal to fp64 bit for bit."""
    assert lab.conv5_stats_case("5x5 64->3 ragged", dtype, *E.CONV5_STATS, exact=True)


# ------------------------------------------------------------------------------------------------ the generic kernel, fp32
@pytest.mark.parametrize("mfma", [1, 0], ids=["mfma", "scalar"])
@pytest.mark.parametrize("case", range(len(E.CASES) + len(E.RAGGED)), ids=[c[0].replace(" ", "_") for c in E.CASES + E.RAGGED])
def test_generic_kernel_fp32_is_exact(lab, case, mfma):
    """igemm.hip / wgrad.hip in fp32 storage on the parity cases and the ragged / tail cases: forward, statistics, weight gradient,
    data gradient and both sums."""
    c = (E.CASES + E.RAGGED)[case]
    assert lab.conv_case(c[0], 0, mfma, *c[1:], exact=True, expect_fwd="generic", expect_wgrad="generic", expect_dgrad="generic",
                         exact_kw=E.EXACT_KW.get(c[0]))
