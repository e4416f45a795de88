"""The operands of tests/test_rounding_kernels_gpu.py, without a GPU: for every case of that file, build the single-rounding operands
and the fp64 reference (tools/exact_operands.py make_rounding_operands) and run Operands.check_rounding() - (a) everything that enters
a rounding point, every output, data-gradient and red1 term exact in fp32 in any order, (b) the fp32 chains of stat_sum and red1
exact, (c) nothing overflows and at least 90 % of the outputs are nonzero, (d) every compared store: at least 25 % of the elements not
representable in the storage type, 5 % exact ties (resolved upwards and downwards), 5 % each non-tie round-ups and round-downs,
(e) every exercised prologue point: 5 % not representable, 1 % ties.  The shares are printed, as test_exact_operands_cpu.py does."""
import pytest
import torch

from tools import exact_operands as E

DT = [1, 2]
DT_IDS = ["fp16", "bf16"]


def _holds(o, what):
    fig = o.check_rounding()
    sh = fig.pop("shares")
    print(what, {k: f"{v:.4g}" for k, v in fig.items()}, f"density {o.density:.3f}", f"dw_exact {getattr(o, 'dw_exact', None)}")
    for k, s in sh.items():
        print("   ", k, {a: round(b, 4) for a, b in s.items()})
    for k, v in fig.items():
        if k[:2] in ("a_", "b_"):
            assert v < 2 ** 24, (k, v)
    return fig, sh


def _main_shares(o, sh):
    """(d) and (e) again, spelled out: check_rounding() asserts them; a case must not lose them by a change of that function."""
    for k in [k for k in ("y", "gx") if k in sh]:
        s = sh[k]
        assert s["inexact"] >= 0.25 and s["tie"] >= 0.05 and s["tie_up"] > 0 and s["tie_down"] > 0 and s["up"] >= 0.05 and s["down"] >= 0.05, (k, s)
    for k in [k for k in ("a", "eff") if k in sh]:
        assert sh[k]["inexact"] >= 0.05 and sh[k]["tie"] >= 0.01, (k, sh[k])


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("case", range(len(E.ROUND_FORWARD)), ids=[f"{f}-{c[0].replace(' ', '_')}" for f, c, _ in E.ROUND_FORWARD])
def test_forward_cases(case, dtype):
    family, c, kw = E.ROUND_FORWARD[case]
    o = E.make_rounding_operands(dtype, *c[1:], parts=("fwd",), **kw)
    fig, sh = _holds(o, f"{family} {c[0]} dt={dtype}")
    assert "y" in sh and ("a" in sh) == bool(c[12]) and "b_sum" in fig
    _main_shares(o, sh)
    # the reference is what it says: sums of the ROUNDED output; the output one rounding of the convolution of the rounded activation
    assert torch.equal(o.stat_sum, o.y.sum(dim=(0, 2, 3))) and torch.equal(o.y, o.y_pre.float().to(E.DT[dtype]).double())
    assert not torch.equal(o.stat_sum, o.y_pre.sum(dim=(0, 2, 3))), "the statistics of the unrounded output are the same: nothing to see"


@pytest.mark.parametrize("kernel", ["mfma-fp16", "mfma-bf16", "scalar-fp16"])     # (the library has no bf16 scalar kernels)
@pytest.mark.parametrize("case", range(len(E.CASES)), ids=[c[0].replace(" ", "_") for c in E.CASES])
def test_generic_forward_cases(case, kernel):
    c = E.CASES[case]
    mfma, dtype = int(kernel.startswith("mfma")), 1 if kernel.endswith("fp16") else 2
    o = E.make_rounding_operands(dtype, *c[1:], parts=("fwd",), **E.generic_kw(c[0], mfma))
    fig, sh = _holds(o, f"generic {c[0]} dt={dtype} mfma={mfma}")
    _main_shares(o, sh)


def _backward_ids():
    out = []
    for i, (what, fam, s, qa) in enumerate(E.ROUND_BACKWARD):
        for q, a in qa:
            out.append(pytest.param(i, q, a, id=f"{fam.split('/')[0 if q else -1]}-{what}-{s[3]}to{s[4]}-{s[0]}x{s[1]}x{s[2]}-q{q}a{a}"))
    return out


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("case,with_q,acc", _backward_ids())
def test_backward_cases(case, with_q, acc, dtype):
    what, family, (B, H, W, Cin, Cout, R, S, pad, transposed, mode), _ = E.ROUND_BACKWARD[case]
    parts = {"fused": ("wgrad", "dgrad"), "dgrad": ("dgrad",)}.get(what, ("wgrad",))     # as tools/gpu_lab.py backward_case
    o = E.make_rounding_operands(dtype, B, H, W, Cin, Cout, R, S, 2 if transposed else 1, pad, transposed=transposed, mode=mode, bn=1,
                                 with_q=with_q, acc=acc, parts=parts)
    fig, sh = _holds(o, f"{family} {what} {Cin}->{Cout} {B}x{H}x{W} q={with_q} acc={acc} dt={dtype}")
    _main_shares(o, sh)
    assert "a" in sh and ("eff" in sh) == bool(with_q) and ("gx" in sh) == ("dgrad" in parts)
    if "dgrad" in parts:
        assert bool((o.red1 != 0).any()) and bool((o.red2 != 0).any()) and "b_red1" in fig
        if acc:   # ONE rounding of gold + scale * dz: rounding the product first gives another tensor
            dt = E.DT[dtype]
            twice = (o.gold + (o.scale.view(1, -1, 1, 1) * o.dz).float().to(dt).double()).float().to(dt).double()
            assert float((twice != o.gx).double().mean()) > 0.02, "a doubly rounded accumulate would pass"
    if "wgrad" in parts:
        assert float((o.dw != 0).double().mean()) > 0.9 and bool((o.dw_bound >= 0).all())
        # the bound is far below what a one-sided error of half an ulp in the activation does to the sum
        print("    dw bound / |dw| (median)", float((o.dw_bound / o.dw.abs().clamp_min(1e-300)).median()))


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
def test_merged_phase_cases(dtype):
    """The merged four-phase launches of tests/test_merged_phase_kernels_gpu.py: one cvw, one cvp_multi and one wgpw_multi case."""
    for family, c, kw in E.ROUND_FORWARD_MERGED:
        o = E.make_rounding_operands(dtype, *c[1:], parts=("fwd",), **kw)
        fig, sh = _holds(o, f"merged {family} {c[0]} dt={dtype}")
        assert c[10] == 1 and "y" in sh and "a" in sh and "b_sum" in fig
        _main_shares(o, sh)
        for py in (0, 1):       # every output parity has stores that need the rounding
            for px in (0, 1):
                assert float((o.y[:, :, py::2, px::2] != o.y_pre[:, :, py::2, px::2]).double().mean()) > 0.1, (py, px)
    for B, H, W, Cin, Cout in E.ROUND_BACKWARD_MERGED:
        o = E.make_rounding_operands(dtype, B, H, W, Cin, Cout, 3, 3, 2, 1, transposed=1, bn=1, with_q=0, acc=0, parts=("wgrad",))
        fig, sh = _holds(o, f"merged wgpw {Cin}->{Cout} {B}x{H}x{W} dt={dtype}")
        _main_shares(o, sh)
        assert "a" in sh and float((o.dw != 0).double().mean()) > 0.9 and bool((o.dw_bound >= 0).all())


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
def test_conv5_case(dtype):
    """The factor form never forms the activation (round_a=False): its weight gradient is that of the UNROUNDED activation, which is
    another tensor than the one the other weight-gradient kernels must produce."""
    B, H, W = E.ROUND_CONV5
    kw = dict(parts=("wgrad", "dgrad"), chain_red=B * H * W)
    o = E.make_rounding_operands(dtype, B, H, W, 64, 3, 5, 5, 1, 2, round_a=False, **kw)
    fig, sh = _holds(o, f"conv5 dt={dtype}")
    assert "a" not in sh and torch.equal(o.a, o.a_pre)
    rounded = E.make_rounding_operands(dtype, B, H, W, 64, 3, 5, 5, 1, 2, **kw)
    assert float(((rounded.dw - o.dw).abs() > o.dw_bound).double().mean()) > 0.2, "the bound cannot tell the rounded activation from the unrounded"


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
def test_weight_rounding_cases(dtype):
    """The weight-rounding set: w = k 2**-12, k odd of up to 13 bits, on the round-8 activations."""
    kw = dict(kind="weights")
    c, g = E.ROUND_PIG, E.ROUND_GENERIC
    for what, o in (("pig fwd", E.make_rounding_operands(dtype, *c[1:], parts=("fwd",), chain=32, **kw)),
                    ("generic fwd", E.make_rounding_operands(dtype, *g[1:], parts=("fwd",), chain=32, **kw)),
                    ("generic dgrad", E.make_rounding_operands(dtype, *g[1:], parts=("dgrad",), **kw)),
                    ("conv3 dgrad", E.make_rounding_operands(dtype, *E.ROUND_CONV3_DGRAD[:7], 1, E.ROUND_CONV3_DGRAD[7], with_q=0, acc=1,
                                                             parts=("dgrad",), **kw))):
        fig, sh = _holds(o, f"weights {what} dt={dtype}")
        assert sh["w"]["inexact"] >= 0.25 and sh["w"]["tie"] >= 0.01
        assert not torch.equal(o.w_T, o.w)
        # the unrounded weights give another stored result: a kernel that skipped the pack's rounding (or truncated) is seen
        if "fwd" in o.parts:
            other = o.fwd(o.a, o.w).float().to(E.DT[dtype]).double()
            assert float((other != o.y).double().mean()) > 0.05
        else:
            assert sh["gx"]["inexact"] > 0.05


def test_subnormal_cases():
    """The f16 subnormal set: at least 10 % of the compared stores in (0, 2**-14), the reference IEEE gradual underflow."""
    kw = dict(kind="subnormal")
    c, g, b = E.ROUND_PIG, E.ROUND_GENERIC, E.ROUND_BW1
    for what, o in (("pig fwd", E.make_rounding_operands(1, *c[1:], parts=("fwd",), chain=32, **kw)),
                    ("generic fwd", E.make_rounding_operands(1, *g[1:], parts=("fwd",), chain=32, **kw)),
                    ("bw1", E.make_rounding_operands(1, *b[:7], 1, b[7], with_q=1, acc=0, parts=("wgrad", "dgrad"), **kw))):
        fig, sh = _holds(o, f"subnormal {what}")
        key = "subnormal_y" if "fwd" in o.parts else "subnormal_gx"
        assert fig[key] >= 0.10, fig
        # every operand the matrix unit reads is normal or zero: a difference is the kernel's conversion, not the unit's input handling
        for t in (o.a, o.w_T, o.eff):
            assert bool(((t == 0) | (t.abs() >= 2.0 ** -14)).all())


def test_a_violation_is_caught():
    """check_rounding() is not vacuous: operands that need no rounding, or that are not exact in fp32, fail it."""
    c = E.CASES[0]
    o = E.make_rounding_operands(2, *c[1:], parts=("fwd",))
    o.y_pre = o.y.clone()                       # every output representable: condition (d)
    with pytest.raises(AssertionError):
        o.check_rounding()
    o = E.make_rounding_operands(2, *c[1:], parts=("fwd",), chain=1 << 20)   # condition (b)
    with pytest.raises(AssertionError):
        o.check_rounding()
    with pytest.raises(AssertionError):         # a number that is not exact in fp32 cannot enter a rounding point
        E._rnd(torch.tensor([1.0 + 2.0 ** -30], dtype=torch.float64), torch.float16, "x")


def test_rounding_shares_on_known_values():
    """rounding_shares on hand-made f16 values: 2049 is a tie resolved downwards (to 2048), 2051 a tie resolved upwards (2052), 2048.5
    rounds down, 2051.5 up, 2050 is representable; in the subnormal range the step is 2**-24."""
    t = torch.tensor([2049.0, 2051.0, 2048.5, 2051.5, 2050.0, 1.5 * 2.0 ** -24, 2.5 * 2.0 ** -24, 1.25 * 2.0 ** -24], dtype=torch.float64)
    s = E.rounding_shares(t, 1)
    n = t.numel()
    assert s["tie"] * n == 4 and s["tie_up"] * n == 2 and s["tie_down"] * n == 2 and s["up"] * n == 1 and s["down"] * n == 2 and s["inexact"] * n == 7
