"""Direct tests of the bandwidth-bound helper kernels (dmmfods_amd/csrc/pointwise.hip), which the network tests reach only at sizes
where every launch cap is far away.

Probe tests: tools/probes/pointwise_probe.hip calls the launchers of the BUILT library on cases whose results are exact (dyadic input
grids; plain fp64 loops as the reference) - one test per group.  The sizes that cross a launch cap:
  convert_input  4096 x 256 threads           B3 H419 W835 (1 049 595 pixels): grid-stride loop
  maxpool_fwd    2048 workgroups x 32 (16) px  B1 H516 W510 C64 (65 790 pooled pixels): grid-stride loop
  maxpool_bwd    2048 workgroups x 32 (16) px  B3 / B5 H122 W190 C64 (69 540 / 115 900 pixels): the (b, y, x) walk, one and two steps
  apply_corr     4 Mi threads / channel slots  5 * 32768 + 3 pixels x 128 slots: the 4-way unrolled loop and its tail (335 MB a tensor)
  bce_metrics    512 workgroups x 4 px/thread  B8 NC3 H260 W256: the 16-byte branch loops
  adam           4096 x 256 threads           n = 4096 * 256 + 13 (below, through dmm_adam_step)
Loss edges, metric ties at the threshold and Adam go through the C ABI from here."""
import ctypes as C
import os
import shutil
import subprocess
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---------------------------------------------------------------------------------------------------- the probe
# `name: ok` lines a complete run of each group prints (an empty or shortened run fails)
GROUP_CASES = {"convert": 22, "bn": 24, "pool": 18, "poolbwd": 18, "corr": 10, "loss": 75}
_probe_dead = []   # the group that ended by signal, timeout or HIP error: nothing of the probe is started after it


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    from dmmfods_amd import _lib
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this box")
    libdir = os.path.dirname(os.path.abspath(_lib.LIB_PATH))
    libname = os.path.basename(_lib.LIB_PATH)
    assert libname.startswith("lib") and libname.endswith(".so"), libname
    exe = str(tmp_path_factory.mktemp("pointwise_probe") / "pointwise_probe")
    subprocess.run([hipcc, "-O2", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-result", "-I", os.path.join(ROOT, "dmmfods_amd", "csrc"),
                    os.path.join(ROOT, "tools", "probes", "pointwise_probe.hip"), "-o", exe, "-L", libdir, "-l" + libname[3:-3],
                    "-Wl,-rpath," + libdir, "-pthread"], check=True, capture_output=True, timeout=600)
    return exe


@pytest.mark.parametrize("group", list(GROUP_CASES))
def test_pointwise_probe(probe, group):
    """One group of tools/probes/pointwise_probe.hip: every case `ok`, none missing."""
    assert not _probe_dead, f"the probe's group {_probe_dead[0]!r} ended by signal or timeout: not started again"
    t0 = time.time()
    try:
        out = subprocess.run([probe, group], capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        _probe_dead.append(group)
        raise
    if out.returncode < 0 or out.returncode == 3:   # a signal, or the probe's own exit after a HIP error
        _probe_dead.append(group)
    print(f"pointwise_probe {group}: {time.time() - t0:.2f} s, exit {out.returncode}")
    assert out.returncode == 0 and "FAIL" not in out.stdout, out.stdout[-4000:] + out.stderr[-2000:]
    assert out.stdout.count(": ok") == GROUP_CASES[group], out.stdout[-4000:]


# ---------------------------------------------------------------------------------------------------- loss edges
LOGITS = [0.0] + [s * v for v in (1e-8, 0.7, 20.0, 50.0, 87.0, 88.5, 95.0, 104.0, 150.0, 1e4) for s in (1.0, -1.0)]
TARGETS = [0.0, 1.0, 0.3]
GAMMAS = [0.0, 0.1, 0.5, 1.0, 2.0, 5.0]
ALPHAS = [0.25, 1.0]
PROBS = [0.0, 1e-30, 1e-6, 0.5, 1 - 1e-6, 1.0]


def _loss_forward(kind, from_prob, alpha, gamma, x, t):
    from dmmfods_amd import _lib
    B, NC, H, W = x.shape
    loss, dx = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
    a, g = (C.c_float * NC)(*alpha), (C.c_float * NC)(*gamma)
    _lib.check(_lib.lib().dmm_loss_forward(kind, from_prob, a, g, x.data_ptr(), t.data_ptr(), loss.data_ptr(), dx.data_ptr(), B, NC, H, W,
                                           _lib.stream_ptr()))
    torch.cuda.synchronize()
    return loss.cpu(), dx.cpu()


def _grid(values, targets, NC):
    """(B, NC, 3, 5) float32 tensors in which every class plane set holds every (value, target) pair."""
    pairs = [(v, t) for v in values for t in targets]
    B = -(-len(pairs) // 15)
    x, t = torch.zeros(B, NC, 15), torch.zeros(B, NC, 15)
    for c in range(NC):
        for i in range(B * 15):
            v, tt = pairs[(i + 7 * c) % len(pairs)]   # another order in every class
            x[i // 15, c, i % 15], t[i // 15, c, i % 15] = v, tt
    return x.view(B, NC, 3, 5).contiguous(), t.view(B, NC, 3, 5).contiguous()


def _focal_ref(x, t, alpha, gamma, from_prob):
    """fp64 autograd of the focal loss as oracle/restatement.py states it, alpha_c * (1 - exp(-bce))**gamma_c * bce, with 1 - exp(-bce)
    formed as -expm1(-bce) (in fp64 the literal difference is 0 below bce = 1.1e-16 and its power's derivative infinite).  The two are
    asserted equal where nothing cancels.  Where bce is exactly 0 in fp64 the derivative of the power is 0 * inf for 0 < gamma < 1:
    there the expected gradient is the limit, 0."""
    import torch.nn.functional as F
    from oracle import restatement as R
    x64 = x.double().requires_grad_(True)
    t64 = t.double()
    if from_prob:
        bce = F.binary_cross_entropy(x64, t64, reduction="none")
    else:
        # the restatement's BCE-with-logits with max(x, 0) written (x + |x|) / 2: the same values, and autograd's derivative at x = 0
        # is sigmoid(0) - t (through clamp it is the one-sided 1 - t)
        bce = (x64 + x64.abs()) / 2 - x64 * t64 + torch.log1p(torch.exp(-x64.abs()))
        assert torch.equal(bce.detach(), R.bce_with_logits(x64.detach(), t64))
    a = torch.tensor(alpha, dtype=torch.float32).double().view(1, -1, 1, 1)
    g = torch.tensor(gamma, dtype=torch.float32).double().view(1, -1, 1, 1)
    loss = a * (-torch.expm1(-bce)) ** g * bce
    loss.sum().backward()
    lit = R.focal_loss(x64.detach(), t64, a.flatten(), g.flatten(), logits=not from_prob)
    plain = bce.detach() > 1e-3
    torch.testing.assert_close(loss.detach()[plain], lit[plain], rtol=1e-12, atol=0)
    grad = x64.grad.clone()
    bad = ~torch.isfinite(grad)
    assert bool((bce.detach()[bad] == 0).all()), "the reference gradient is not finite at a point where bce is not 0"
    grad[bad] = 0.0
    assert bool(torch.isfinite(loss).all())
    return loss.detach(), grad


def _per_class(NC):
    """gamma / alpha of the classes of an NC-class tensor: over NC = 1..8 every (gamma, alpha) pair occurs three times, in mixes."""
    k0 = NC * (NC - 1) // 2
    return [ALPHAS[((k0 + c) // 6) % 2] for c in range(NC)], [GAMMAS[(k0 + c) % 6] for c in range(NC)]


@pytest.mark.parametrize("NC", range(1, 9))
def test_loss_edges_logits(NC):
    """dmm_loss_forward on saturated, tiny and threshold logits, focal with gamma down to 0 (plain alpha-weighted BCE) and plain BCE:
    all finite, loss within rtol 2e-5 / atol 2e-7 and d(loss)/dx within rtol 2e-4 / atol 2e-6 of fp64 autograd (the bounds of
    test_focal_kernel_matches_reference_fixture).

    The edge this test is for: loss_elem formed (1 - pt)^(gamma - 1).  For gamma = 0 and a confidently right logit of magnitude
    88.8 .. 103, 1 - pt is a denormal float and the power overflows: in float arithmetic that keeps denormals x = 95, t = 1, gamma = 0
    gives loss = inf and dx = nan, x = -95, t = 0 gives loss = inf, dx = inf (with denormals flushed, 0 and 0).  The kernel now forms
    (1 - pt)^gamma only.  The values at x = 95 are printed for the record."""
    from dmmfods_amd import _lib
    x, t = _grid(LOGITS, TARGETS, NC)
    alpha, gamma = _per_class(NC)
    for kind in (_lib.LOSS_FOCAL, _lib.LOSS_BCE):
        a, g = (alpha, gamma) if kind == _lib.LOSS_FOCAL else ([1.0] * NC, [0.0] * NC)   # BCE = focal with alpha 1, gamma 0
        loss, dx = _loss_forward(kind, 0, a, g, x.to(DEV), t.to(DEV))
        ref, dref = _focal_ref(x, t, a, g, False)
        for c in range(NC):
            i = (x[:, c] == 95.0) & (t[:, c] == 1.0)
            print(f"NC {NC} kind {kind} class {c} gamma {g[c]} alpha {a[c]}: x=95 t=1 -> loss {loss[:, c][i][0].item():.6g} dx {dx[:, c][i][0].item():.6g}"
                  f" (fp64 {ref[:, c][i][0].item():.6g} {dref[:, c][i][0].item():.6g})")
        assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(dx).all()), (kind, x[~torch.isfinite(loss) | ~torch.isfinite(dx)])
        np.testing.assert_allclose(loss.double().numpy(), ref.numpy(), rtol=2e-5, atol=2e-7)
        np.testing.assert_allclose(dx.double().numpy(), dref.numpy(), rtol=2e-4, atol=2e-6)


@pytest.mark.parametrize("NC", [1, 3, 8])
def test_loss_edges_probabilities(NC):
    """from_prob (torch.binary_cross_entropy: logs clamped at -100, the derivative's denominator at 1e-12): losses everywhere, the clamp
    included; gradients at interior p; p in {0, 1} with the target on the same side gives loss 0 and gradient 0."""
    from dmmfods_amd import _lib
    x, t = _grid(PROBS, TARGETS, NC)
    alpha, gamma = _per_class(NC)
    loss, dx = _loss_forward(_lib.LOSS_FOCAL, 1, alpha, gamma, x.to(DEV), t.to(DEV))
    ref, dref = _focal_ref(x, t, alpha, gamma, True)
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(dx).all())
    np.testing.assert_allclose(loss.double().numpy(), ref.numpy(), rtol=2e-5, atol=2e-7)
    interior = (x > 0) & (x < 1)
    np.testing.assert_allclose(dx.double()[interior].numpy(), dref[interior].numpy(), rtol=2e-4, atol=2e-6)
    same = ((x == 0) & (t == 0)) | ((x == 1) & (t == 1))
    assert int(same.sum()) >= 2 * NC
    assert bool((loss[same] == 0).all()) and bool((dx[same] == 0).all()), (loss[same], dx[same])


# ---------------------------------------------------------------------------------------------------- metric ties
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_metric_ties_at_threshold(dtype):
    """dmm_plan_loss_metrics of a tiny bound plan (the 16-byte branch of bce_metrics): logits and targets exactly at iou_threshold and
    on its two float neighbours.  Equal counts and per-image intersections / unions are exact under the `>=` rule of
    oracle.restatement; loss sums within 1e-6 of host fp64."""
    from oracle import restatement as R
    from dmmfods_amd.graphs.models.Dense_U_Net_lidar import Dense_U_Net_lidar
    from dmmfods_amd.utils.Dense_U_Net_lidar_helper import get_config
    cfg = get_config("/tmp/dmm_test")
    cfg.model.growth_rate, cfg.model.block_config, cfg.model.num_init_features = 8, (2, 2, 2, 2), 16
    cfg.model.concat_before_block_num, cfg.model.stream_2_in_channels = 1, 0
    model = Dense_U_Net_lidar(cfg, compute_dtype=dtype).to(DEV).eval()
    B, NC, H, W = 2, int(model.num_classes), 32, 32
    assert NC == 3
    thr = np.float32(model.iou_threshold)
    assert thr == np.float32(0.7)
    near = np.array([np.nextafter(thr, np.float32(-np.inf)), thr, np.nextafter(thr, np.float32(np.inf))], dtype=np.float32)
    rng = np.random.default_rng(5)

    def draw():   # a third exactly at the threshold, the rest on its neighbours and far from it
        v = rng.uniform(-3, 3, size=(B, NC, H, W)).astype(np.float32)
        k = rng.integers(0, 6, size=v.shape)
        v[k == 0] = near[1]; v[k == 1] = near[1]; v[k == 2] = near[0]; v[k == 3] = near[2]
        return torch.from_numpy(v)
    logits, tgt = draw(), draw().clamp(0, 1)
    assert abs(float((logits == float(thr)).float().mean()) - 1 / 3) < 0.05 and abs(float((tgt == float(thr)).float().mean()) - 1 / 3) < 0.05
    model.loss_metrics(logits.to(DEV), tgt.to(DEV))
    torch.cuda.synchronize()
    m = model._get_plan(B, H, W).metrics.cpu()
    pa, pb = logits >= float(thr), tgt >= float(thr)
    assert torch.equal(m[NC:2 * NC], (pa == pb).sum(dim=(0, 2, 3)).double())
    per = m[2 * NC:].view(B, 2, NC)
    assert torch.equal(per[:, 0], (pa & pb).sum(dim=(2, 3)).double()) and torch.equal(per[:, 1], (pa | pb).sum(dim=(2, 3)).double())
    torch.testing.assert_close(per[:, 0].float() / per[:, 1].float(), R.iou_whole_img_batch(logits, tgt, float(thr)), rtol=0, atol=0)
    torch.testing.assert_close((m[NC:2 * NC] / (B * H * W)).float(), R.accuracy_per_class(tgt, logits, float(thr)).float(), rtol=1e-6, atol=0)
    want = R.bce_with_logits(logits.double(), tgt.double()).sum(dim=(0, 2, 3))
    np.testing.assert_allclose(m[:NC].numpy(), want.numpy(), rtol=1e-6)
    model.close()


# ---------------------------------------------------------------------------------------------------- Adam
ADAM_STRIDE_N = 2048 * 1024 + 1024 + 13   # one chunk and a ragged tail past the kernel's grid of 2048 workgroups x 1024 elements: the stride loop's second step
ADAM_SHIFT = {1027: 1}                    # n -> elements behind a 16-byte boundary: the element path, with a tail


@pytest.mark.parametrize("n", [1, 255, 257, 4096 * 256 + 13, ADAM_STRIDE_N, 1027])
def test_adam_step_every_element(n):
    """dmm_adam_step against torch.optim.Adam (L2 weight decay, amsgrad off) restated in fp64, every element: many workgroups, past
    the grid's cap (ADAM_STRIDE_N; one parameter combination there, the fp64 restatement of twelve takes too long), on pointers that
    are not 16-byte aligned (n = 1027), with weight decay, a gradient scale, late steps, and gradients of 0 and 1e-30.
    m, v: 2^-21 relative (three fp32 operations each, 2x margin) plus the smallest fp32 denormal (v of a 1e-30 gradient underflows);
    |dp - dp_ref| <= 2^-20 |dp_ref| + ulp(p): about eleven roundings on the way to the update, 2x margin, and the rounding of p itself."""
    from dmmfods_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(n)
    lr, b1, b2, eps = np.float32(1e-3), np.float32(0.9), np.float32(0.999), np.float32(1e-8)
    p0 = rng.standard_normal(n).astype(np.float32)
    g0 = (rng.standard_normal(n) * 0.01).astype(np.float32)
    idx = np.arange(n)
    g0[idx % 7 == 0] = 0.0
    g0[idx % 7 == 3] = 1e-30
    shift = ADAM_SHIFT.get(n, 0)
    for wd in (0.0, 0.01):
        for gs in (1.0, 1.0 / 1024):
            for step in (1, 2, 1000):
                if n == ADAM_STRIDE_N and (wd, gs, step) != (0.01, 1.0 / 1024, 1000):
                    continue
                wd32 = np.float32(wd)
                ge = g0.astype(np.float64) * gs + float(wd32) * p0.astype(np.float64)
                # moments of the sign of the effective gradient (nothing cancels: the relative bound is meaningful), zero at step 1
                m0 = np.zeros(n, np.float32) if step == 1 else (ge * rng.uniform(0.5, 1.5, n)).astype(np.float32)
                v0 = np.zeros(n, np.float32) if step == 1 else (ge * ge * rng.uniform(0.5, 1.5, n)).astype(np.float32)
                m = float(b1) * m0.astype(np.float64) + (1 - float(b1)) * ge
                v = float(b2) * v0.astype(np.float64) + (1 - float(b2)) * ge * ge
                bc1, bc2 = 1 - float(b1) ** step, 1 - float(b2) ** step
                dp = -(float(lr) / bc1) * m / (np.sqrt(v) / np.sqrt(bc2) + float(eps))
                P, G, M, V = (torch.zeros(n + 4, device=DEV)[shift:shift + n].copy_(torch.from_numpy(a)) for a in (p0, g0, m0, v0))
                assert P.data_ptr() % 16 == 4 * shift
                _lib.check(L.dmm_adam_step(P.data_ptr(), G.data_ptr(), M.data_ptr(), V.data_ptr(), n, float(lr), float(b1), float(b2), float(eps), float(wd32), step, gs, _lib.stream_ptr()))
                torch.cuda.synchronize()
                gm, gv, gp = M.cpu().numpy().astype(np.float64), V.cpu().numpy().astype(np.float64), P.cpu().numpy().astype(np.float64)
                tiny = 2.0 ** -149
                where = f"wd {wd} grad_scale {gs} step {step}"
                bad = np.abs(gm - m) > 2.0 ** -21 * np.abs(m) + tiny
                assert not bad.any(), (where, "m", np.flatnonzero(bad)[:4], gm[bad][:4], m[bad][:4])
                bad = np.abs(gv - v) > 2.0 ** -21 * np.abs(v) + tiny
                assert not bad.any(), (where, "v", np.flatnonzero(bad)[:4], gv[bad][:4], v[bad][:4])
                bad = np.abs((gp - p0) - dp) > 2.0 ** -20 * np.abs(dp) + np.spacing(np.abs(p0)).astype(np.float64)
                assert not bad.any(), (where, "dp", np.flatnonzero(bad)[:4], (gp - p0)[bad][:4], dp[bad][:4])
                assert torch.equal(G.cpu(), torch.from_numpy(g0)), (where, "the gradient was written")
