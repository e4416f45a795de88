"""Single-rounding parity of every convolution kernel family that has a single-kernel entry point: every 16-bit store met bit for bit.

The random-operand tests hold a 16-bit result to 3e-3 / 2.5e-2 of the tensor's maximum, the exact-operand tests
(tests/test_exact_kernels_gpu.py) are built so that nothing ever rounds: neither sees a conversion that rounds the wrong way, statistics
taken from the accumulators instead of the stored values, or a doubly rounded accumulate.  On the operands of this file
(tools/exact_operands.py make_rounding_operands) all fp32 arithmetic is exact in any order, as there, but the values that reach a 16-bit
store need more significant bits than the type holds: each store is exactly ONE round-to-nearest-even of an exactly known number.
The fp64 reference applies every rounding point the kernels document, in their order - the weight pack, the BN+ReLU prologue, the
output (statistics: sums of the output AS STORED), the effective gradient, ONE rounding of gold + scale * dz - and

  * everything stored in the storage type, stat_sum and red1 must be EQUAL BIT FOR BIT, ties included;
  * stat_sq, red2 and a weight gradient that is not exact in fp32 are held to bounds derived from the reference alone
    (chain * 2**-24 * sum y'**2;  chain * 2**-24 * sum |dz xhat|, plus |mean| invstd sum |dz| for bw1's f16 epilogue and the 5x5
    factor form, which add dz * x in fp32 and centre in fp64;  n * 2**-23 * sum |a| |eff|, n the number of added terms); a weight
    gradient whose terms are exact in fp32 (bf16 on small maps) is compared bit for bit.

The conditions that make this so, and the shares of inexact values and exact ties that keep a case from passing emptily, are asserted
on the reference before anything is launched (Operands.check_rounding) and, without a GPU, for every case of this file in
tests/test_rounding_operands_cpu.py.  Every case asserts the kernel family that ran: a fallback to the generic kernel fails it.
Rounding needs no multi-tile walk, so the shapes are the smallest each family's resolve accepts (cf: at least eight tiles per CU).

Not here, as in tests/test_exact_kernels_gpu.py: cvp_multi_kernel, cvw's four-phase walk and wgpw_multi_kernel, whose single-rounding
cases are in tests/test_merged_phase_kernels_gpu.py; the head's launches, which still have no file (hf, conv3's MULTI form, wgp.hip's
own multi-phase path with four taps per phase: no entry point builds a two-segment launch) and cvd_kernel, the lab fallback; the logits launch, whose rounding cases are in tests/test_logits_kernels_gpu.py; fp32 storage, whose stores do not round; bf16 on the scalar kernels, which the library does not have; the
effective-gradient prologue on cvd3 and on wg5's transposed form, which their resolves refuse."""
import pytest
import torch

from tools import exact_operands as E

pytestmark = pytest.mark.gpu
DT = [1, 2]
DT_IDS = ["fp16", "bf16"]
GENERIC_OFF = (b"thin_logits", b"conv3", b"cvp", b"pig")     # the forward / data-gradient families dmm_set_option switches


@pytest.fixture(scope="module")
def lab():
    assert torch.cuda.is_available()
    from tools import gpu_lab
    return gpu_lab


@pytest.fixture
def generic_only():
    """Every switchable forward / data-gradient family off: the launch runs on igemm.hip (the case asserts it)."""
    from dmmfods_amd import _lib
    L = _lib.lib()
    try:
        for name in GENERIC_OFF:
            _lib.check(L.dmm_set_option(name, 0))
        yield
    finally:
        for name in GENERIC_OFF:
            _lib.check(L.dmm_set_option(name, 1))


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("case", range(len(E.ROUND_FORWARD)), ids=[f"{f}-{c[0].replace(' ', '_')}" for f, c, _ in E.ROUND_FORWARD])
def test_forward_output_and_statistics_round_once(lab, case, dtype):
    """Output: one rounding of conv(a, w_T), a = one rounding of relu(x * scale + shift); stat_sum: the sum of the output as stored."""
    family, c, kw = E.ROUND_FORWARD[case]
    assert lab.conv_case(c[0], dtype, 1, *c[1:], exact="round", parts=("fwd",), expect_fwd=family, exact_kw=kw)


@pytest.mark.parametrize("kernel", ["mfma-fp16", "mfma-bf16", "scalar-fp16"])
@pytest.mark.parametrize("case", range(len(E.CASES)), ids=[c[0].replace(" ", "_") for c in E.CASES])
def test_generic_forward_rounds_once(lab, generic_only, case, kernel):
    """igemm.hip's MFMA and scalar forward on the parity cases (plain, strided, transposed, pooled, upsampled)."""
    c = E.CASES[case]
    mfma, dtype = int(kernel.startswith("mfma")), 1 if kernel.endswith("fp16") else 2
    assert lab.conv_case(c[0], dtype, mfma, *c[1:], exact="round", parts=("fwd",), expect_fwd="generic", exact_kw=E.generic_kw(c[0], mfma))


# ------------------------------------------------------------------------------------------------ backward
def _backward_ids():
    out = []
    for i, (what, fam, s, qa) in enumerate(E.ROUND_BACKWARD):
        for q, a in qa:
            out.append(pytest.param(i, q, a, id=f"{fam.split('/')[0 if q else -1]}-{what}-{s[3]}to{s[4]}-{s[0]}x{s[1]}x{s[2]}-q{q}a{a}"))
    return out


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("case,with_q,acc", _backward_ids())
def test_backward_stores_round_once(lab, case, with_q, acc, dtype):
    """Stored data gradient: ONE rounding of gold + scale * dz, dz from the once-rounded effective gradient, the mask and red1 from the
    unrounded dz; weight gradients: sums of the once-rounded activation times the once-rounded effective gradient."""
    what, family, (B, H, W, Cin, Cout, R, S, pad, transposed, mode), _ = E.ROUND_BACKWARD[case]
    if family == "wgp/wgpw":
        family = "wgp" if with_q else "wgpw"
    name = f"{R}x{S} {Cin}->{Cout} {B}x{H}x{W}" + (" convT" if transposed else (" up2" if mode == 1 else ""))
    assert lab.backward_case(name, dtype, B, H, W, Cin, Cout, R, S, pad, transposed=transposed, with_q=with_q, acc=acc, what=what,
                             mode=mode, expect=family, exact="round")


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
def test_conv5_weight_gradient_and_sums_round_once(lab, dtype):
    """dmm_conv5_wgrad_stats (wg5.hip PA = 3 + wg5_fin64_kernel).  The factor form never forms the activation: the weight gradient is
    scale * sum m x dy + shift * sum m dy, that of the UNROUNDED activation (round_a=False; the mask m is that of the rounded one)."""
    B, H, W = E.ROUND_CONV5
    assert lab.conv5_stats_case("5x5 64->3 ragged", dtype, B, H, W, exact="round", exact_kw=dict(chain_red=B * H * W, round_a=False))


# ------------------------------------------------------------------------------------------------ the weight pack
@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
def test_weight_pack_rounds_once_pig_forward(lab, dtype):
    """Weights k * 2**-12, k odd of up to 13 bits: the forward must use rnd(w)."""
    c = E.ROUND_PIG
    assert lab.conv_case(c[0] + " w", dtype, 1, *c[1:], exact="round", parts=("fwd",), expect_fwd="pig", exact_kw=dict(kind="weights", chain=32))


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
def test_weight_pack_rounds_once_generic(lab, generic_only, dtype):
    c = E.ROUND_GENERIC
    assert lab.conv_case(c[0] + " w", dtype, 1, *c[1:], exact="round", parts=("fwd",), expect_fwd="generic", exact_kw=dict(kind="weights", chain=32))
    assert lab.conv_case(c[0] + " w", dtype, 1, *c[1:], exact="round", parts=("dgrad",), expect_dgrad="generic", exact_kw=dict(kind="weights"))


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
def test_weight_pack_rounds_once_conv3_data_gradient(lab, dtype):
    B, H, W, Cin, Cout, R, S, pad, transposed, mode = E.ROUND_CONV3_DGRAD
    assert lab.backward_case(f"{R}x{S} {Cin}->{Cout} {B}x{H}x{W} w", dtype, B, H, W, Cin, Cout, R, S, pad, with_q=0, acc=1, what="dgrad",
                             expect="conv3", exact="round", exact_kw=dict(kind="weights"))


# ------------------------------------------------------------------------------------------------ f16 subnormals
def test_subnormal_results_pig_forward(lab):
    """Operands scaled by 2**-12: at least 10 % of the stored outputs in (0, 2**-14); the reference is IEEE gradual underflow.  Every
    value the matrix unit reads is normal or zero."""
    c = E.ROUND_PIG
    assert lab.conv_case(c[0] + " sub", 1, 1, *c[1:], exact="round", parts=("fwd",), expect_fwd="pig", exact_kw=dict(kind="subnormal", chain=32))


def test_subnormal_results_generic_forward(lab, generic_only):
    c = E.ROUND_GENERIC
    assert lab.conv_case(c[0] + " sub", 1, 1, *c[1:], exact="round", parts=("fwd",), expect_fwd="generic", exact_kw=dict(kind="subnormal", chain=32))


def test_subnormal_results_bw1_data_gradient(lab):
    """The stored data gradient of a loss-scaled f16 backward, around 2**-14."""
    B, H, W, Cin, Cout, R, S, pad, transposed, mode = E.ROUND_BW1
    assert lab.backward_case(f"{R}x{S} {Cin}->{Cout} {B}x{H}x{W} sub", 1, B, H, W, Cin, Cout, R, S, pad, with_q=1, acc=0, what="fused",
                             expect="bw1", exact="round", exact_kw=dict(kind="subnormal"))
