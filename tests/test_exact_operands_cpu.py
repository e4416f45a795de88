"""The operands of tests/test_exact_kernels_gpu.py, without a GPU: for every case of that file, build the operands and the fp64
reference (tools/exact_operands.py) and assert the conditions under which a kernel must equal the reference bit for bit -
(a) every stored tensor representable in the storage type, (b) every output, data-gradient and weight-gradient element exact in
fp32 in any summation order, (c) the fp32 partials of the per-channel sums exact, (d) at least 90 % of the outputs nonzero - and
the coverage of the {-1, 0, 1} weights.  The GPU tests can then neither pass vacuously nor fail because of their own inputs."""
import pytest
import torch

from tools import exact_operands as E

DT = [1, 2]
DT_IDS = ["fp16", "bf16"]


def _holds(o):
    fig = o.check()      # raises on (a) - (d) and on the weight conditions
    assert fig["nonzero_y"] >= 0.9 and 0 < fig["density"] <= 0.85
    for k, v in fig.items():
        if k[:2] in ("b_", "c_"):
            assert v < 2 ** 24, (k, v)
    return fig


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("case", range(len(E.FORWARD)), ids=[f"{f}-{c[0].replace(' ', '_')}" for f, c, _ in E.FORWARD])
def test_forward_cases(case, dtype):
    family, c, kw = E.FORWARD[case]
    o = E.make_operands(dtype, *c[1:], parts=("fwd",), **(kw.get(dtype) or {}))
    fig = _holds(o)
    assert {"b_y", "c_sum", "c_sq"} <= set(fig)
    # the reference is what it says: the statistics are the sums of the output, the output is the convolution of the activation
    assert torch.equal(o.stat_sum, o.y.sum(dim=(0, 2, 3))) and o.y.shape[1] == c[5]


def test_f16_weights_are_denser_than_bf16():
    """Built separately per storage type: f16 holds 11 bits against bf16's 8."""
    family, c, kw = E.FORWARD[0]
    d16 = _holds(E.make_operands(1, *c[1:], parts=("fwd",)))["density"]
    dbf = _holds(E.make_operands(2, *c[1:], parts=("fwd",)))["density"]
    assert d16 > 3.5 * dbf, (d16, dbf)
    s = E.BACKWARD[2][2]
    k = dict(transposed=s[8], mode=s[9], with_q=1, parts=("dgrad",))
    g16 = _holds(E.make_operands(1, *s[:7], 1, s[7], **k))["density"]
    gbf = _holds(E.make_operands(2, *s[:7], 1, s[7], **k))["density"]
    assert g16 > 5 * gbf, (g16, gbf)


def _backward_ids():
    out = []
    for i, (what, fam, s, qa) in enumerate(E.BACKWARD):
        for q, a in qa:
            out.append(pytest.param(i, q, a, id=f"{fam.split('/')[0 if q else -1]}-{what}-{s[3]}to{s[4]}-{s[0]}x{s[1]}x{s[2]}-q{q}a{a}"))
    return out


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("case,with_q,acc", _backward_ids())
def test_backward_cases(case, with_q, acc, dtype):
    what, family, (B, H, W, Cin, Cout, R, S, pad, transposed, mode), _ = E.BACKWARD[case]
    parts = {"fused": ("wgrad", "dgrad"), "dgrad": ("dgrad",)}.get(what, ("wgrad",))     # as tools/gpu_lab.py backward_case
    o = E.make_operands(dtype, B, H, W, Cin, Cout, R, S, 2 if transposed else 1, pad, transposed=transposed, mode=mode, bn=1,
                        with_q=with_q, acc=acc, parts=parts)
    fig = _holds(o)
    if "dgrad" in parts:
        assert {"b_dz", "c_red1", "c_red2"} <= set(fig)
        assert bool((o.gx != 0).any()) and bool((o.red1 != 0).any()) and bool((o.red2 != 0).any())
        if acc:
            assert not torch.equal(o.gx, o.dz * o.scale.view(1, -1, 1, 1))   # the accumulated gradient is in the reference
    if "wgrad" in parts:
        assert "b_dw" in fig and float((o.dw != 0).double().mean()) > 0.9
    if with_q:
        assert bool((o.eff != o.dy).any())


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
def test_stem_and_conv5_cases(dtype):
    c = E.STEM_WGRAD
    fig = _holds(E.make_operands(dtype, *c[1:], parts=("fwd", "wgrad")))
    assert "b_dw" in fig and "b_y" in fig
    fig = _holds(E.make_operands(dtype, *E.CONV5_STATS, 64, 3, 5, 5, 1, 2, parts=("wgrad", "dgrad")))
    assert "c_red2" in fig


@pytest.mark.parametrize("case", range(len(E.CASES) + len(E.RAGGED)), ids=[c[0].replace(" ", "_") for c in E.CASES + E.RAGGED])
def test_generic_fp32_cases(case):
    c = (E.CASES + E.RAGGED)[case]
    o = E.make_operands(0, *c[1:], **(E.EXACT_KW.get(c[0]) or {}))
    fig = _holds(o)
    bn, strided = c[12], (c[8] != 1 and not c[10] and c[11] == 0)
    assert ("c_red1" in fig) == bool(bn and not strided)     # as conv_case: no BN-fused data gradient without BN or at stride 2


# ------------------------------------------------------------------------------------------------ tests/test_merged_phase_kernels_gpu.py
MERGED_FWD = [(f, c) for f, c, _ in E.FORWARD_MERGED] + [("generic", E.FORWARD_APART)]


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("case", range(len(MERGED_FWD)), ids=[f"{f}-{c[0].replace(' ', '_')}" for f, c in MERGED_FWD])
def test_merged_forward_cases(case, dtype):
    """The merged forward cases and the one kept apart, with the default value ranges (no shape needed narrower ones)."""
    family, c = MERGED_FWD[case]
    o = E.make_operands(dtype, *c[1:], parts=("fwd",))
    fig = _holds(o)
    assert {"b_y", "c_sum", "c_sq"} <= set(fig) and c[10] == 1
    assert torch.equal(o.stat_sum, o.y.sum(dim=(0, 2, 3))) and bool((o.stat_sum != 0).all()) and bool((o.stat_sq != 0).all())
    # every output parity carries outputs: a phase left out, or written to another parity, is seen
    for py in (0, 1):
        for px in (0, 1):
            assert float((o.y[:, :, py::2, px::2] != 0).double().mean()) > 0.5, (py, px)


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("case", range(len(E.BACKWARD_MERGED) + 1),
                         ids=["{3}to{4}-{0}x{1}x{2}-q0".format(*s) for s, _ in E.BACKWARD_MERGED] + ["{3}to{4}-{0}x{1}x{2}-q1".format(*E.BACKWARD_APART)])
def test_merged_weight_gradient_cases(case, dtype):
    with_q = int(case == len(E.BACKWARD_MERGED))
    B, H, W, Cin, Cout = E.BACKWARD_APART if with_q else E.BACKWARD_MERGED[case][0]
    o = E.make_operands(dtype, B, H, W, Cin, Cout, 3, 3, 2, 1, transposed=1, bn=1, with_q=with_q, acc=0, parts=("wgrad",))
    fig = _holds(o)
    assert "b_dw" in fig and (not with_q or bool((o.eff != o.dy).any()))
    # every tap's gradient is there (the taps belong to different phases: 1, 2, 2 and 4 of the 9)
    for t in range(9):
        assert float((o.dw[:, :, t // 3, t % 3] != 0).double().mean()) > 0.9, t


def test_merged_launcher_arithmetic_on_256_compute_units():
    """What each merged case is there for, from the launchers' formulas (tools/exact_operands.py merged_*_geometry) - for the MI355X's
    256 compute units where the launcher asks the device; the GPU test recomputes it for the device at hand."""
    g = [E.merged_fwd_geometry(f, *c[1:6]) for f, c, _ in E.FORWARD_MERGED]
    assert (g[0]["per"], g[0]["nwg"], g[0]["done_mod"]) == (2, 8, [0, 2, 4, 6])
    assert (g[1]["per"], g[1]["nwg"], g[1]["done_mod"]) == (264, 256, [0, 8, 16, 24])
    assert (g[2]["per"], g[2]["nwg"], g[2]["groups"], g[2]["ntn"]) == (288, 256, 2, 2)
    assert (g[3]["per"], g[3]["per8"], g[3]["idle"]) == (8, 1, 0) and g[3]["groups"] == 3
    assert (g[4]["per"], g[4]["per8"], g[4]["nwg"], g[4]["idle"]) == (12, 2, 64, 16)
    for k in g[:3]:      # cvw: every (phase, item) pair is walked by exactly one workgroup
        for p in range(4):
            seen = sorted(i for b in range(k["nwg"]) for i in range(k["first"][p][b], k["per"], k["nwg"]))
            assert seen == list(range(k["per"])), p
            assert all((p * k["per"] + k["first"][p][b]) % k["nwg"] == b for b in range(k["nwg"]))
    w = [E.merged_wgrad_geometry(*s, 256) for s, _ in E.BACKWARD_MERGED]
    assert (w[0]["units"], w[0]["nwg"]) == (8, 32) and (w[1]["units"], w[1]["nwg"]) == (3, 32)
    assert w[2] == dict(ntiles=25, pairs=4, nsplit=13, tiles_per_wg=2, units=52, nwg=224)


def test_a_violation_is_caught():
    """check() is not vacuous: operands outside the recipe fail it."""
    c = E.CASES[0]
    o = E.make_operands(2, *c[1:])
    o.y = o.y + 2.0 ** -9                # off the step: beside |y| >= 0.5 that takes more than bf16's 8 bits
    with pytest.raises(AssertionError):
        o.check()
    o = E.make_operands(2, *c[1:])
    o.wslots = o.wslots.clone()
    o.wslots[:, 3, 0] = 0                # input channel 3 reaches no output channel
    with pytest.raises(AssertionError):
        o.check()
