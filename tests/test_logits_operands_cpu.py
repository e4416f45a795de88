"""The operands of tests/test_logits_kernels_gpu.py, without a GPU: for every case of that file, build the operands and the fp64
reference (tools/exact_operands.py, part "logits") and assert the conditions under which the logits launch must equal the reference
bit for bit.

Exact class: the activation representable in the storage type, the logits representable in fp32 (the launch stores fp32, whatever the
storage type), sum |term| / u < 2**24 per logit, at least 90 % of the logits nonzero, the weight coverage - and (p): some channel has
relu(shift) > 0 and the reference differs, on the border of EVERY image, from the same convolution with the prologue applied to the
padding, so that a kernel that normalises its padding cannot pass.  There are no statistics, hence no chain conditions.
Single-rounding class: the logits are compared unrounded and are representable in fp32; the rounding points are the prologue (kind
"main": shares of inexact activations and of ties) and the weight pack (kind "weights").

Also here: the launcher arithmetic each case is there for - thin.hip's strip and row split (tools/exact_operands.py thin_geometry, a
restatement of thin_resolve), xcd_remap as a permutation of a grid that is no multiple of 8, halo.hip's tile count."""
import pytest
import torch

from tools import exact_operands as E

DESIGN_CUS = 256
IDS = [E.logits_id(f, dt, m, off, s) for f, dt, m, off, s, _ in E.LOGITS]


def _holds_logits(o):
    """As _holds of tests/test_exact_operands_cpu.py, for a logits launch: one class makes the weights dense by construction (every
    (tap, channel) pair must be nonzero somewhere), so there is no upper bound on the density."""
    fig = o.check()
    assert fig["nonzero_y"] >= 0.9 and 0 < fig["density"] <= 1.0
    assert fig["b_y"] < 2 ** 24 and fig["pad_diff"] > 0
    assert not any(k.startswith("c_") for k in fig), fig       # no statistics to compare
    return fig


def _make(dtype, s, **kw):
    B, H, W, Cin, Cout, R, pad = s
    return E.make_operands(dtype, B, H, W, Cin, Cout, R, R, 1, pad, parts=("logits",), **kw)


@pytest.mark.parametrize("case", range(len(E.LOGITS)), ids=IDS)
def test_exact_cases(case):
    family, dtype, mfma, thin_off, s, _ = E.LOGITS[case]
    B, H, W, Cin, Cout, R, pad = s
    o = _make(dtype, s)
    fig = _holds_logits(o)
    assert o.y.shape == (B, Cout, H, W) and torch.equal(o.y, E.conv(o.a, o.w, o.case))
    assert torch.equal(o.y.float().double(), o.y)
    if Cout == 1:
        assert fig["density"] == 1.0
    # the border really is what tells the two paddings apart: at most the outer `pad` pixels differ, on every image some do
    d = o.y != o.y_padnorm
    assert bool(d.flatten(1).any(dim=1).all()) and not bool(d[:, :, pad:H - pad, pad:W - pad].any())
    # the family the case names is the one the resolves give this launch (pinned under the fake runtime in tests/test_host_cpu.py)
    thin_takes = dtype != 0 and mfma and not thin_off and Cin == 64 and Cout <= 3 and R == 5
    assert (family == "thin") == bool(thin_takes)
    if family == "halo":        # f16 / fp32 only, and the fp32 weights must fit its LDS beside the halo image
        assert dtype in (0, 1) and mfma and (dtype == 1 or R * R * Cin * 32 * 4 <= 80 * 1024)
    if family == "generic":
        assert not thin_takes and (dtype == 2 or not mfma or (dtype == 0 and R * R * Cin * 32 * 4 > 160 * 1024))


@pytest.mark.parametrize("case", range(len(E.LOGITS_THIN)), ids=[f"{s[0]}x{s[1]}x{s[2]}x{s[3]}" for s, _, _ in E.LOGITS_THIN])
def test_thin_geometry(case):
    (B, H, W, N), want, why = E.LOGITS_THIN[case]
    g = E.thin_geometry(B, H, W)
    assert {k: g[k] for k in want} == want, (why, g)
    assert 1 <= N <= 3 and g["rows_per_wg"] * (g["nys"] - 1) < H <= g["rows_per_wg"] * g["nys"]
    assert 124 * (g["nxs"] - 1) < W <= 124 * g["nxs"]
    # the hardware-to-logical workgroup map is a permutation of the grid, whatever its remainder modulo the 8 XCDs
    assert sorted(E.xcd_remap(b, g["nwg"]) for b in range(g["nwg"])) == list(range(g["nwg"]))


def test_thin_cases_cover_what_they_are_there_for():
    geo = {s: E.thin_geometry(*s[:3]) for s, _, _ in E.LOGITS_THIN}
    assert geo[(2, 37, 131, 3)]["steps"] > 2 * 6, "the ring of 6 slots does not wrap twice"
    assert geo[(2, 37, 131, 3)]["last_rows"] < geo[(2, 37, 131, 3)]["rows_per_wg"], "no ragged row strip"
    assert geo[(3, 37, 255, 3)]["nwg"] % 8 != 0, "xcd_remap's remainder branch is not taken"
    assert geo[(2, 45, 249, 2)]["last_rows"] == geo[(2, 45, 249, 2)]["rows_per_wg"]
    assert geo[(1, 3, 5, 3)]["rows_per_wg"] < 6, "as many rows as ring slots"
    assert {s[3] for s in geo} == {1, 2, 3}, "an instantiation of thin_logits_kernel has no case"


def test_halo_walk_case_has_more_tiles_than_compute_units():
    B, H, W = E.LOGITS_HALO_WALK
    nt = E.halo_tiles(B, H, W)
    assert nt == 13 * 22 > DESIGN_CUS and nt % DESIGN_CUS != 0 and H % 8 != 0 and W % 16 != 0
    assert any(s[:3] == (B, H, W) and f == "halo" for f, _, _, _, s, _ in E.LOGITS)


@pytest.mark.parametrize("kind", E.ROUND_LOGITS_KINDS)
@pytest.mark.parametrize("case", range(len(E.ROUND_LOGITS)), ids=[E.logits_id(f, dt, 1, off, s) for f, dt, off, s in E.ROUND_LOGITS])
def test_rounding_cases(case, kind):
    family, dtype, thin_off, s = E.ROUND_LOGITS[case]
    B, H, W, Cin, Cout, R, pad = s
    o = E.make_rounding_operands(dtype, B, H, W, Cin, Cout, R, R, 1, pad, parts=("logits",), kind=kind)
    fig = o.check_rounding()
    sh = fig["shares"]
    assert fig["a_y"] < 2 ** 24 and fig["nonzero_y"] >= 0.9 and "y" not in sh and "b_sum" not in fig
    assert torch.equal(o.y, o.y_pre) and torch.equal(o.y.float().double(), o.y)
    assert torch.equal(o.y, E.conv(o.a, o.w_T, o.case))
    if kind == "main":
        assert sh["a"]["inexact"] >= 0.05 and sh["a"]["tie"] >= 0.01 and not torch.equal(o.a, o.a_pre)
        assert not torch.equal(o.y, E.conv(o.a_pre, o.w_T, o.case)), "the prologue's rounding does not show in the logits"
    else:
        assert sh["w"]["inexact"] >= 0.25 and sh["w"]["tie"] >= 0.01 and not torch.equal(o.w, o.w_T)
        assert not torch.equal(o.y, E.conv(o.a, o.w, o.case)), "the pack's rounding does not show in the logits"
    assert bool((o.wslots != 0).any(dim=0).all()), "a (tap, input channel) pair is zero in every class"


def test_a_violation_is_caught():
    """check() / check_rounding() are not vacuous for the logits part: one deliberately broken operand set per class."""
    s = E.LOGITS[0][4]
    o = _make(1, s)
    o.y = o.y + 2.0 ** -30               # below fp32's resolution at |y| ~ 100: not representable
    with pytest.raises(AssertionError, match="fp32"):
        o.check()
    o = _make(1, s)
    o.shift = -o.shift.abs()             # no channel with relu(shift) > 0: padding before and after the prologue agree
    with pytest.raises(AssertionError, match=r"\(p\)"):
        o.check()
    o = _make(1, s)
    o.y_padnorm = o.y_padnorm.clone()
    o.y_padnorm[1] = o.y[1]              # the second image's border no longer tells the paddings apart
    with pytest.raises(AssertionError, match=r"\(p\)"):
        o.check()
    B, H, W, Cin, Cout, R, pad = E.ROUND_LOGITS[0][3]
    o = E.make_rounding_operands(1, B, H, W, Cin, Cout, R, R, 1, pad, parts=("logits",))
    o.a_pre = o.a                        # nothing for the prologue to round
    with pytest.raises(AssertionError):
        o.check_rounding()
    o = E.make_rounding_operands(1, B, H, W, Cin, Cout, R, R, 1, pad, parts=("logits",))
    o.y = o.y_pre = o.y_pre + 2.0 ** -30
    with pytest.raises(AssertionError, match="fp32"):
        o.check_rounding()
