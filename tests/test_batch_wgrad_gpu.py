"""Launch coalescing of a dense block's weight-gradient side (dmm_set_option("batch_wgrad")): the grouped forms of wg3_kernel,
wg3_reduce_kernel and bw1_reduce_kernel, and the executor that hands consecutive independent records over together.

(1) the grouped wg3 launch through its C test entry (dmm_conv_wgrad_grouped): members of different map sizes in one launch, each
    against fp64 autograd and against the single-launch path, at the tolerance of the single-launch parity test
    (test_timed_kernels_gpu.py: 3e-3 fp16 / 2.5e-2 bf16 of the tensor's maximum); two runs bit-equal;
(2) the grouped bw1 reduction (dmm_bw1_reduce_grouped) on synthetic slots: EQUAL to the per-launch kernel;
(3) a small dense net through the model with the option off and on."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = {1: 3e-3, 2: 2.5e-2}      # tools/gpu_lab.py backward_case: relative to the tensor's maximum
DT = {1: torch.float16, 2: torch.bfloat16}
# the member shapes (B, H, W): one tile; ragged in both directions, 12 tiles; 15 tiles
ONE, RAGGED, MANY = (1, 8, 16), (2, 20, 28), (1, 40, 48)


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    from dmmfods_amd import _lib
    return _lib


def _relerr(a, b):
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


_members = {}


def _member(dtype, with_q, shape, seed):
    """One dense 3x3 weight gradient (128 -> 32 channels behind BN+ReLU): device operands and the fp64 autograd reference, made once."""
    key = (dtype, with_q, shape, seed)
    if key in _members:
        return _members[key]
    B, H, W = shape
    Cin, Cout = 128, 32
    dt = DT[dtype]
    g = torch.Generator().manual_seed(1000 * seed + H)
    x = torch.randn(B, Cin, H, W, generator=g) * 2 + 0.5
    scale = torch.rand(Cin, generator=g) + 0.5
    shift = torch.randn(Cin, generator=g) * 0.5
    dy = torch.randn(B, Cout, H, W, generator=g)
    eff = dy.to(dt).double()
    yf = q = r = None
    if with_q:
        yf = torch.randn(B, Cout, H, W, generator=g) * 1.5
        q = torch.randn(Cout, generator=g) * 0.3
        r = torch.randn(Cout, generator=g) * 0.2
        eff = eff + q.double().view(1, -1, 1, 1) + r.double().view(1, -1, 1, 1) * yf.to(dt).double()
    a = F.relu(x.to(dt).double() * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1))
    w = torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64, requires_grad=True)
    (F.conv2d(a, w, padding=1) * eff).sum().backward()
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to(dt).to(DEV)  # noqa: E731
    m = dict(shape=shape, x=nhwc(x), dy=nhwc(dy), scale=scale.to(DEV), shift=torch.cat([shift, torch.zeros(2 * Cin)]).to(DEV),
             yf=nhwc(yf) if with_q else None, q=q.to(DEV) if with_q else None, r=r.to(DEV) if with_q else None, ref=w.grad.clone())
    _members[key] = m
    return m


def _run_wg3(lib, dtype, members, grouped):
    """dmm_conv_wgrad_grouped on `members`: ([dw per member], kernel launches made)."""
    L = lib.lib()
    n = len(members)
    descs = (lib.ConvDesc * n)()
    keep = []
    arr = lambda vals: (C.c_void_p * n)(*[v.data_ptr() if v is not None else None for v in vals])  # noqa: E731
    dws, scratch = [], []
    for i, m in enumerate(members):
        B, H, W = m["shape"]
        descs[i] = lib.ConvDesc(dtype=dtype, use_mfma=1, B=B, H=H, W=W, Cin=128, Cout=32, R=3, S=3, stride=1, pad=1, transposed=0, mode=0, bn_relu=1)
        dws.append(torch.full((32, 128, 3, 3), float("nan"), device=DEV))
        scratch.append(torch.zeros(L.dmm_conv_scratch_bytes(C.byref(descs[i])), dtype=torch.uint8, device=DEV))
    ptrs = [arr([m[k] for m in members]) for k in ("x", "dy", "scale", "shift", "yf", "q", "r")] + [arr(dws), arr(scratch)]
    keep.append(ptrs)
    nl = C.c_int(-1)
    lib.impls_since_reset()
    lib.check(L.dmm_conv_wgrad_grouped(descs, n, *ptrs, 1 if grouped else 0, C.byref(nl), lib.stream_ptr()))
    torch.cuda.synchronize()
    assert "wg3" in lib.impls_since_reset()
    return dws, nl.value


# 31 one-tile members and one of 2 x 64 x 272 (272 tiles): 303 tiles on 256 workgroups - the one-tile members' proportional share
# rounds to no workgroup at all, each still gets one, and the large member gives up what that takes (the dealing's second pass)
CROWD = [ONE] * 15 + [(2, 64, 272)] + [ONE] * 16
CASES = {
    "one": [RAGGED],
    "two": [ONE, MANY],
    "three-maps": [ONE, RAGGED, MANY],
    "33-members": [(ONE, RAGGED, MANY)[i % 3] for i in range(33)],     # the member cap forces a split into two launches
    "five-tiles": [ONE] * 5,                                           # fewer tiles than workgroups of one compute unit each
    "crowd": CROWD,
}


@pytest.mark.parametrize("dtype", [1, 2], ids=["fp16", "bf16"])
@pytest.mark.parametrize("with_q", [0, 1], ids=["materialised", "effgrad"])
@pytest.mark.parametrize("case", list(CASES))
def test_grouped_dense_3x3_weight_gradient(lib, dtype, with_q, case):
    """wg3_group_kernel<T, PQ> + wg3_group_reduce_kernel: every member against fp64 autograd and against the single-launch path at
    the single-launch test's tolerance; the grouped launches are fewer than the members; two grouped runs are bit-equal (slots are
    added in a fixed order, no float atomics)."""
    members = [_member(dtype, with_q, shape, seed=i) for i, shape in enumerate(CASES[case])]
    single, nl1 = _run_wg3(lib, dtype, members, grouped=False)
    grouped, nlg = _run_wg3(lib, dtype, members, grouped=True)
    again, _ = _run_wg3(lib, dtype, members, grouped=True)
    assert nl1 == len(members) and nlg == (len(members) + 31) // 32, (nl1, nlg)
    worst = (0.0, 0.0)
    for i, m in enumerate(members):
        e_ref, e_one, e_single = _relerr(grouped[i].cpu(), m["ref"]), _relerr(single[i].cpu(), m["ref"]), _relerr(grouped[i], single[i])
        worst = max(worst, (e_ref, e_single))
        assert e_ref < TOL[dtype] and e_single < TOL[dtype] and e_one < TOL[dtype], (case, i, m["shape"], e_ref, e_one, e_single)
        assert torch.equal(grouped[i], again[i]), (case, i)
    print(f"grouped wg3 {case} dt={dtype} q={with_q}: {len(members)} members in {nlg} launches, worst vs fp64 {worst[0]:.2e}, vs single {worst[1]:.2e}")


B1_SLOT_FLOATS = 4 * 128 * 32


def _run_bw1_reduce(lib, parts, dpacks, ncts, nsplits, wcs, grouped):
    L = lib.lib()
    n = len(parts)
    ia = lambda v: (C.c_int * n)(*v)  # noqa: E731
    pa = lambda v: (C.c_void_p * n)(*[t.data_ptr() for t in v])  # noqa: E731
    nl = C.c_int(-1)
    lib.check(L.dmm_bw1_reduce_grouped(n, pa(parts), pa(dpacks), ia(ncts), ia(nsplits), ia(wcs), 1 if grouped else 0, C.byref(nl), lib.stream_ptr()))
    torch.cuda.synchronize()
    return nl.value


@pytest.mark.parametrize("count", [13, 40], ids=["13-members", "40-members"])
def test_grouped_bw1_reduction_equals_the_per_launch_kernel(lib, count):
    """bw1_reduce_group_kernel: nct in {1, 3, 8} x nsplit in {2, 5, 16, 37} (the 16-wide, the 4-wide and the single loop body all run),
    one member whose channel count leaves padding rows behind the packed gradient (nct = 3, 288 channels: 9 of 12 chunks), 40
    members (the cap of 32 splits the launch).  Same loads, same additions in the same order: torch.equal with the per-launch
    kernel, the floats behind each packed gradient untouched; and the sums are the slots' sums (fp64 reference, fp32 rounding)."""
    g = torch.Generator().manual_seed(7)
    combos = [(nct, ns, nct * 128) for nct in (1, 3, 8) for ns in (2, 5, 16, 37)] + [(3, 5, 288)]
    if count == 40:
        combos = [((1, 3)[i % 2], (2, 5, 16, 37, 4, 1)[i % 6], (128, 352)[i % 2]) for i in range(40)]
    parts, ncts, nsplits, wcs = [], [], [], []
    for nct, ns, wc in combos:
        parts.append(torch.randn(ns * nct * B1_SLOT_FLOATS, generator=g).to(DEV))
        ncts.append(nct); nsplits.append(ns); wcs.append(wc)
    out = {}
    for grouped in (0, 1):
        dpacks = [torch.full((nct * B1_SLOT_FLOATS + 64,), -7.0, device=DEV) for nct in ncts]   # (slack: what the kernel must not write)
        nl = _run_bw1_reduce(lib, parts, dpacks, ncts, nsplits, wcs, grouped)
        assert nl == ((len(combos) + 31) // 32 if grouped else len(combos)), nl
        out[grouped] = dpacks
    for i, (nct, ns, wc) in enumerate(combos):
        nfloats = (wc + 31) // 32 * 128 * 32
        assert torch.equal(out[0][i], out[1][i]), (i, nct, ns, wc)
        assert bool((out[1][i][nfloats:] == -7.0).all()), (i, nct, ns, wc)
        ref = parts[i].double().view(ns, nct * B1_SLOT_FLOATS).sum(0)[:nfloats]
        assert _relerr(out[1][i][:nfloats], ref) < 1e-5, (i, nct, ns, wc)


def _model(arch, dtype):
    from dmmfods_amd.graphs.models import Dense_U_Net_lidar as M
    from dmmfods_amd.utils.Dense_U_Net_lidar_helper import get_config
    cfg = get_config("/tmp/dmm_test")
    cfg.model.growth_rate, cfg.model.block_config, cfg.model.num_init_features = arch.growth_rate, arch.block_config, arch.num_init_features
    cfg.model.concat_before_block_num, cfg.model.stream_2_in_channels = arch.concat_before_block_num, arch.stream_2_in_channels
    return M.Dense_U_Net_lidar(cfg, compute_dtype=dtype)


def _oracle(R, arch, B, H, W, seed, wseed, storage=None):
    P = {k: (t.double() if t.is_floating_point() else t.clone()) for k, t in R.make_state(arch, seed=wseed).items()}
    tr = R.Trainer(arch, P, storage=storage)
    rgb, lidar, tgt = R.make_inputs(arch, B, H, W, seed=seed)
    out = tr.step(rgb.double(), lidar.double(), tgt.double(), do_update=False)
    return out, {k: t.grad.clone() for k, t in tr.leaves}


def _errors(model, logits, met, emu, g_emu, o64, g64):
    """As test_timed_kernels_gpu.py measures a network: logits / loss against the emulation (maximum norm), all gradients rel L2, and
    every convolution weight's gradient rel L2 per tensor; y_*: the emulation's own distance from the fp64 oracle."""
    num = den = ynum = 0.0
    per = {}
    for k, p in model.named_parameters():
        got = p.grad.detach().cpu().double()
        num += float((got - g_emu[k]).pow(2).sum())
        ynum += float((g_emu[k] - g64[k]).pow(2).sum())
        den += float(g_emu[k].pow(2).sum())
        if p.dim() == 4:
            per[k] = float((got - g_emu[k]).norm() / g_emu[k].norm().clamp_min(1e-30))
    return dict(per_conv=per, logits=_relerr(logits.detach().cpu(), emu["logits"]), y_logits=_relerr(emu["logits"], o64["logits"]),
                loss=_relerr(met["loss_per_class"].cpu(), emu["loss_per_class"]), grads=(num / den) ** 0.5, y_grads=(ynum / den) ** 0.5,
                worst_conv=max((v, k) for k, v in per.items()))


def test_small_dense_net_with_and_without_batching(lib):
    """Block config (3, 2), growth 32, B = 2, 64 x 96, fp16 through the model, dmm_set_option("batch_wgrad", 0 | 1 | 2) (read at every
    call: the same plan serves all; 1 = grouped on the caller's stream, 2 = on the weight-gradient stream).  The bw1 reductions add the same slots in the same order either way: every conv1 gradient that
    two runs WITHOUT batching reproduce bit for bit is bit-equal with batching.  The dense 3x3 weight gradients are split over
    workgroups differently (another fp32 summation order), so they - and everything else - are held against the oracle's fp16
    emulation at the bounds test_timed_kernels_gpu.py sets per tensor group for the DenseNet-121 'early' network at this map size
    (the same layer shapes; this net is no deeper): dense layers 1.5 x 0.378, decoder 0.5, others 0.62, refine1 / refine0 / the last
    ConvTranspose 1e-3 / 0.06 / 0.10; loss 5e-3; logits and all gradients (rel L2) 2e-2 / 5e-2 or the emulation's own distance from fp64.
    With the option on the step issues fewer weight-gradient and reduction launches than it has records (dmm_plan_wgrad_batch_counts)."""
    from oracle import restatement as R
    L = lib.lib()
    arch = R.Arch(growth_rate=32, block_config=(3, 2), num_init_features=64, concat_before_block_num=1, stream_2_in_channels=3)
    B, H, W = 2, 64, 96
    emu, g_emu = _oracle(R, arch, B, H, W, seed=5, wseed=17, storage=torch.float16)
    o64, g64 = _oracle(R, arch, B, H, W, seed=5, wseed=17)
    model = _model(arch, "fp16")
    model.load_state_dict(R.make_state(arch, seed=17))
    model = model.to(DEV).train()
    rgb, lidar, tgt = (t.to(DEV) for t in R.make_inputs(arch, B, H, W, seed=5))

    def counts():
        c = (C.c_longlong * 4)()
        lib.check(L.dmm_plan_wgrad_batch_counts(model._last[0].handle, C.byref(c)))
        return list(c)

    runs = []
    try:
        for on in (0, 0, 1, 2):
            lib.check(L.dmm_set_option(b"batch_wgrad", on))
            logits = model(rgb, lidar)
            c0 = counts()
            met = model.loss_backward(tgt)
            torch.cuda.synchronize()
            runs.append(dict(grads={k: p.grad.detach().clone() for k, p in model.named_parameters()}, logits=logits.detach().clone(), met=met,
                             counts=[a - b for a, b in zip(counts(), c0)], errors=_errors(model, logits, met, emu, g_emu, o64, g64)))
    finally:
        lib.check(L.dmm_set_option(b"batch_wgrad", 1))
    off, off2, on, on_side = runs
    conv1 = [k for k in off["grads"] if k.endswith("conv1.weight")]
    assert len(conv1) == 5
    stable = [k for k in conv1 if torch.equal(off["grads"][k], off2["grads"][k])]
    print(f"conv1 gradients two unbatched runs reproduce bit for bit: {len(stable)} of {len(conv1)}")
    for k in stable:
        for run in (on, on_side):
            assert torch.equal(run["grads"][k], off["grads"][k]), (k, float((run["grads"][k] - off["grads"][k]).abs().max()))
    for k in on["grads"]:      # the same batches, the same split over workgroups on either stream
        if k.endswith("conv2.weight"):
            assert torch.equal(on["grads"][k], on_side["grads"][k]), k
    print(f"launch counts [wg3 launches, wg3 records, bw1.reduce launches, records]: off {off['counts']}, on {on['counts']}")
    assert off["counts"][0] == off["counts"][1] == 5 and off["counts"][2] == off["counts"][3] > 0, off["counts"]
    assert on["counts"][1] == 5 and on["counts"][3] == off["counts"][3], on["counts"]
    assert on["counts"][0] < on["counts"][1] and on["counts"][2] < on["counts"][3], on["counts"]
    assert on_side["counts"] == on["counts"], (on["counts"], on_side["counts"])
    sharp = {"dec_out_to_heat_maps.refine1.weight": 1e-3, "dec_out_to_heat_maps.refine0.weight": 0.06, "decoder.Transposed_Convolution_2.weight": 0.10}
    for name, run in (("off", off), ("on", on), ("on, weight-gradient stream", on_side)):
        e = run["errors"]
        print(f"batch_wgrad {name}: logits {e['logits']:.3e} (emulation vs fp64 {e['y_logits']:.3e}), loss {e['loss']:.3e}, grads rel L2 {e['grads']:.3e} "
              f"(emulation vs fp64 {e['y_grads']:.3e}), worst conv tensor {e['worst_conv'][0]:.3e} {e['worst_conv'][1]}")
        assert torch.isfinite(run["logits"]).all()
        assert e["loss"] < 5e-3 and e["logits"] < max(2e-2, e["y_logits"]) and e["grads"] < max(5e-2, e["y_grads"]), e
        for k, v in e["per_conv"].items():
            bound = sharp.get(k) or (1.5 * 0.378 if "denselayer" in k else (0.5 if k.startswith("decoder.") else 0.62))
            assert v < bound, (name, k, v, bound)
    assert any(float(on["grads"][k].abs().max()) > 0 for k in on["grads"] if k.endswith("conv2.weight"))
