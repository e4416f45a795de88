"""The validation threshold sweep on the GPU: dmm_logit_hist against numpy, EXACTLY (int64 counts), and the layers above it.

Reference for every case (numpy, float32 operands):
    bins   = (x[..., None] >= thr).sum(-1)
    g      = t >= np.float32(gt)
    counts = np.bincount(...) per (b, n, g)
1 main case with ties on both comparisons, 2 edges (element path, tiny planes, 255 thresholds, misaligned inputs), 3 special values,
4 more than one step per thread, 5 accumulate, 6 agreement with bce_metrics_kernel's counts, 7 ThresholdSweep over three batches,
8 the agent."""
import collections
import ctypes as C

import numpy as np
import pytest
import torch

from dmmfods_amd.utils.Dense_U_Net_lidar_helper import get_config

pytestmark = pytest.mark.gpu

DEV = "cuda"
TINY = dict(growth_rate=8, block_config=(2, 2, 2, 2), num_init_features=16)
GT = 0.7
THR16 = np.arange(-3.75, 3.76, 0.5, dtype=np.float32)
assert THR16.size == 16 and THR16[0] == -3.75 and THR16[-1] == 3.75


def _reference(x, t, thr, gt=GT):
    B, NC = x.shape[:2]
    K = len(thr)
    bins = (x[..., None] >= thr).sum(-1)
    g = (t >= np.float32(gt)).astype(np.int64)
    plane = (np.arange(B * NC, dtype=np.int64).reshape(B, NC, 1, 1) * 2 + g) * (K + 1) + bins
    return np.bincount(plane.ravel(), minlength=B * NC * 2 * (K + 1)).reshape(B, NC, 2, K + 1).astype(np.int64)


def _dev(a):
    return torch.tensor(a, device=DEV)   # (a copy: the shared arrays are read-only)


def _hist(x, t, thr, gt=GT, accumulate=0, counts=None):
    """x, t: float32 device tensors (B, NC, H, W); returns the int64 device counts."""
    from dmmfods_amd import _lib
    B, NC, H, W = x.shape
    K = len(thr)
    L = _lib.lib()
    if counts is None:
        counts = torch.empty((B, NC, 2, K + 1), dtype=torch.int64, device=DEV)
    assert counts.numel() == L.dmm_logit_hist_elems(B, NC, K)
    thr_c = (C.c_float * K)(*[float(v) for v in thr])
    _lib.check(L.dmm_logit_hist(x.data_ptr(), t.data_ptr(), B, NC, H, W, thr_c, K, gt, accumulate, counts.data_ptr(), _lib.stream_ptr()))
    return counts


def _check(x, t, thr, what, gt=GT):
    want = _reference(x, t, thr, gt)
    got = _hist(_dev(x), _dev(t), thr, gt)
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), torch.from_numpy(want)), (what, int((got.cpu() != torch.from_numpy(want)).sum()))
    return want


_MAIN = {}


def _main_case():
    """2 x 3 x 64 x 96, 16 thresholds; x = N(0, 2), t = U(0, 1) with every 11th logit ON a threshold and every 13th target ON gt.
    Made once, shared, never written to."""
    if not _MAIN:
        rng = np.random.default_rng(0)
        shape = (2, 3, 64, 96)
        x = rng.normal(0, 2, shape).astype(np.float32)
        t = rng.uniform(0, 1, shape).astype(np.float32)
        idx = np.arange(x.size).reshape(shape)
        x[idx % 11 == 0] = THR16[(idx[idx % 11 == 0] // 11) % 16]
        t[idx % 13 == 0] = np.float32(GT)
        x.setflags(write=False)
        t.setflags(write=False)
        _MAIN.update(x=x, t=t, want=_reference(x, t, THR16))
    return _MAIN["x"], _MAIN["t"], _MAIN["want"]


def _grid_x(B, NC, H, W):
    """The launcher's rule, restated: about 512 workgroups in all, never more than one four-pixel step per thread."""
    return min(max(1, 512 // (B * NC)), (H * W + 1023) // 1024)


# ------------------------------------------------------------------------------------------------ 1. main case
def test_main_case_with_ties_on_both_comparisons():
    x, t, want = _main_case()
    assert want.shape == (2, 3, 2, 17) and want.min() >= 1                      # every bin is used (the emptiest holds 43)
    assert np.isin(x, THR16).mean() >= 0.05 and (t == np.float32(GT)).mean() >= 0.05
    assert (want.sum(axis=(2, 3)) == 64 * 96).all()
    print(f"[sweep] main case: emptiest bin {want.min()}, logits on a threshold {np.isin(x, THR16).mean():.3f}, targets on gt {(t == np.float32(GT)).mean():.3f}")
    got = _hist(_dev(x), _dev(t), THR16)
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), torch.from_numpy(want))


# ------------------------------------------------------------------------------------------------ 2. edges
@pytest.mark.parametrize("shape,K", [((1, 1, 33, 35), 1), ((3, 5, 7, 9), 2), ((2, 8, 40, 52), 255)])
def test_edges(shape, K):
    """33 x 35: plane % 4 != 0, the element path.  7 x 9: a plane smaller than a workgroup.  K = 255: the maximal threshold count."""
    rng = np.random.default_rng(K)
    x = rng.normal(0, 2, shape).astype(np.float32)
    t = rng.uniform(0, 1, shape).astype(np.float32)
    thr = {1: np.asarray([0.25], dtype=np.float32), 2: np.asarray([-1.0, 1.0], dtype=np.float32), 255: np.linspace(-6, 6, 255).astype(np.float32)}[K]
    x.ravel()[::7] = thr[np.arange(x.ravel()[::7].size) % K]
    want = _check(x, t, thr, (shape, K))
    if K == 255:
        assert (want == 0).sum() > 0                                             # many bins are empty


def test_inputs_one_element_behind_a_16_byte_boundary():
    x, t, want = _main_case()
    n = x.size
    bx, bt = torch.empty(n + 4, device=DEV), torch.empty(n + 4, device=DEV)
    xd, td = bx[1:n + 1].view(x.shape), bt[1:n + 1].view(t.shape)
    xd.copy_(_dev(x))
    td.copy_(_dev(t))
    assert xd.data_ptr() % 16 == 4 and td.data_ptr() % 16 == 4 and xd.is_contiguous()
    got = _hist(xd, td, THR16)
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), torch.from_numpy(want))


# ------------------------------------------------------------------------------------------------ 3. special values
def test_special_values():
    x0, t0, _ = _main_case()
    x, t = x0.copy(), t0.copy()
    thr = np.arange(-4.0, 4.01, 0.5, dtype=np.float32)                           # 17 thresholds, 0.0 among them
    assert 0.0 in thr
    fx, ft = x.reshape(-1), t.reshape(-1)
    fx[5::101] = np.inf
    fx[6::103] = -np.inf
    fx[7::107] = np.nan                                                          # bin 0
    fx[8::109] = -0.0                                                            # -0.0 >= 0.0
    fx[9::113] = np.float32(1e-40)                                               # subnormal, >= 0.0
    fx[10::127] = np.float32(-1e-40)                                             # subnormal, below 0.0
    ft[11::131] = np.nan                                                         # g = 0
    ft[7::107][::2] = np.nan                                                     # NaN on both sides
    assert np.signbit(fx[8]) and fx[8] == 0 and fx[9] > 0 and fx[9] < np.finfo(np.float32).tiny
    want = _check(x, t, thr, "special values")
    assert (want.sum(axis=(2, 3)) == 64 * 96).all()
    # what the reference itself says about them, spelled out: NaN logits in bin 0, +inf in the last, -0.0 beside +0.0
    only = np.full((1, 1, 4, 4), np.nan, dtype=np.float32)
    tt = np.ones((1, 1, 4, 4), dtype=np.float32)
    assert _check(only, tt, thr, "all NaN")[0, 0, 1, 0] == 16
    only[:] = np.inf
    assert _check(only, tt, thr, "all +inf")[0, 0, 1, 17] == 16
    only[:] = -0.0
    assert _check(only, tt, thr, "all -0.0")[0, 0, 1, 9] == 16                   # -4.0 .. 0.0: nine thresholds reached
    tt[:] = np.nan
    assert _check(only, tt, thr, "NaN targets")[0, 0, 0, 9] == 16


# ------------------------------------------------------------------------------------------------ 4. several steps per thread
def test_more_than_one_step_per_thread():
    shape = (1, 2, 768, 1024)
    gx = _grid_x(*shape)
    assert 768 * 1024 > gx * 256 * 4 and gx == 256                               # three steps of four pixels per thread
    rng = np.random.default_rng(4)
    x = rng.normal(-1, 2, shape).astype(np.float32)
    t = (rng.uniform(0, 1, shape) ** 4).astype(np.float32)
    _check(x, t, THR16, shape)


# ------------------------------------------------------------------------------------------------ 5. accumulate
def test_accumulate():
    x, t, want = _main_case()
    xd, td = _dev(x), _dev(t)
    counts = torch.full((2, 3, 2, 17), 0x5a5a5a5a5a5a5a5a, dtype=torch.int64, device=DEV)
    _hist(xd, td, THR16, accumulate=0, counts=counts)
    assert torch.equal(counts.cpu(), torch.from_numpy(want))
    _hist(xd, td, THR16, accumulate=1, counts=counts)
    assert torch.equal(counts.cpu(), torch.from_numpy(2 * want))
    rng = np.random.default_rng(5)
    x2 = rng.normal(1, 3, x.shape).astype(np.float32)
    t2 = rng.uniform(0, 1, x.shape).astype(np.float32)
    _hist(torch.from_numpy(x2).to(DEV), torch.from_numpy(t2).to(DEV), THR16, accumulate=1, counts=counts)
    assert torch.equal(counts.cpu(), torch.from_numpy(2 * want + _reference(x2, t2, THR16)))


# ------------------------------------------------------------------------------------------------ 6. the existing kernel's counts
def _model(seed=123):
    from oracle import restatement as R
    from dmmfods_amd.graphs.models.Dense_U_Net_lidar import Dense_U_Net_lidar
    arch = R.Arch(**TINY, concat_before_block_num=3, stream_2_in_channels=3)
    cfg = get_config("/tmp/dmm_test")
    cfg.model.growth_rate, cfg.model.block_config, cfg.model.num_init_features = arch.growth_rate, arch.block_config, arch.num_init_features
    cfg.model.concat_before_block_num, cfg.model.stream_2_in_channels = 3, 3
    model = Dense_U_Net_lidar(cfg, compute_dtype="fp32")
    model.load_state_dict(R.make_state(arch, seed=seed))
    return R, arch, cfg, model.to(DEV)


def test_agrees_with_the_loss_kernel_at_its_threshold():
    from dmmfods_amd.metrics import curves_from_counts
    R, arch, cfg, model = _model()
    model.eval()
    rgb, lidar, tgt = (v.to(DEV) for v in R.make_inputs(arch, 2, 64, 96, seed=0))
    with torch.no_grad():
        logits = model(rgb, lidar)
        m = model.loss_metrics(logits, tgt)
    op = np.float32(cfg.agent.iou_threshold)
    thr = np.union1d(np.asarray([-2.0, -0.5, 0.0, 1.5], dtype=np.float32), [op]).astype(np.float32)
    col = int(np.nonzero(thr == op)[0][0])
    c = curves_from_counts(_hist(logits.contiguous(), tgt.contiguous().float(), thr, gt=float(cfg.agent.iou_threshold)))
    tp, fp, fn, tn = (c[k][..., col] for k in ("tp", "fp", "fn", "tn"))          # (B, NC)
    assert m["intersection"].dtype == torch.float64
    assert torch.equal(tp, m["intersection"].long()) and torch.equal(tp.double(), m["intersection"])
    assert torch.equal(tp + fp + fn, m["union"].long()) and torch.equal((tp + fp + fn).double(), m["union"])
    acc = ((tp + tn).sum(0).double() / float(2 * 64 * 96)).float()
    assert torch.equal(acc, m["acc_per_class"])
    assert int(m["union"].sum()) > 0
    model.close()


# ------------------------------------------------------------------------------------------------ 7. ThresholdSweep
def test_threshold_sweep_over_three_batches():
    from dmmfods_amd.agents.Dense_U_Net_lidar_Agent import Dense_U_Net_lidar_Agent as Agent
    from dmmfods_amd.metrics import ThresholdSweep, curves_from_counts
    R, arch, cfg, model = _model()
    model.eval()
    op = np.float32(cfg.agent.iou_threshold)
    thr = np.union1d(THR16, [op]).astype(np.float32)
    col = int(np.nonzero(thr == op)[0][0])
    sweep = ThresholdSweep(3, thresholds=thr.tolist(), gt_threshold=float(cfg.agent.iou_threshold))
    rng = np.random.default_rng(7)
    total = np.zeros((3, 2, 18), dtype=np.int64)
    rows = torch.zeros((3, 3), device=DEV)                                       # the agent's per-epoch IoU rows (n, nc)
    for i, B in enumerate((1, 2, 3)):
        x = rng.normal(0, 2, (B, 3, 64, 96)).astype(np.float32)
        t = rng.uniform(0, 1, (B, 3, 64, 96)).astype(np.float32)
        if B == 2:
            t[1, 1] = 0.0
            x[1, 1] = -9.0                                                       # a sample whose IoU is 0/0 at the upper thresholds
        xd, td = _dev(x), _dev(t)
        batch = sweep.update(xd, td)
        want = _reference(x, t, thr, float(cfg.agent.iou_threshold))
        assert torch.equal(batch.cpu(), torch.from_numpy(want))
        total += want.sum(0)
        with torch.no_grad():
            rows[i] = Agent._batch_metrics(model.loss_metrics(xd, td))[0]
    assert torch.equal(sweep.counts.cpu(), torch.from_numpy(total))
    got, want = sweep.compute(), curves_from_counts(torch.from_numpy(total).to(DEV))
    for k, v in want.items():
        assert got[k].is_cuda and torch.equal(torch.nan_to_num(got[k].double(), nan=-7.0), torch.nan_to_num(v.double(), nan=-7.0)), k
    assert torch.equal(got["thresholds"].cpu(), torch.from_numpy(thr))
    assert got["iou_per_instance"].shape == (3, 17) and got["iou_per_instance"].dtype == torch.float32
    assert torch.equal(got["iou_per_instance"][:, col], rows.mean(0)), (got["iou_per_instance"][:, col], rows.mean(0))
    iou = np.nan_to_num(want["iou"].cpu().numpy(), nan=-np.inf)
    assert np.array_equal(got["best_threshold"].cpu().numpy(), thr[iou.argmax(1)])          # (numpy: first index on ties)
    assert np.array_equal(got["best_iou"].cpu().numpy(), want["iou"].cpu().numpy()[np.arange(3), iou.argmax(1)])
    sweep.reset()
    assert sweep.counts is None
    with pytest.raises(RuntimeError):
        sweep.compute()
    model.close()


# ------------------------------------------------------------------------------------------------ 8. the agent
class _Loader:
    def __init__(self, batches):
        self.train_loader, self.train_iterations = batches, len(batches)
        self.valid_loader, self.valid_iterations = batches, len(batches)


class _Counting:
    """Stands in front of the loaded library and counts the calls of the histogram entry point."""

    def __init__(self, real):
        self._real, self.calls = real, collections.Counter()

    def __getattr__(self, name):
        f = getattr(self._real, name)
        if name != "dmm_logit_hist":
            return f

        def counted(*a):
            self.calls[name] += 1
            return f(*a)
        return counted


def _agent(tmp_path, monkeypatch, batches, sweep, ema):
    from dmmfods_amd.agents import Dense_U_Net_lidar_Agent as mod
    from dmmfods_amd.graphs.models.Dense_U_Net_lidar import Dense_U_Net_lidar
    from oracle import restatement as R
    cfg = get_config(str(tmp_path))
    cfg.dir.current_run.summary = str(tmp_path / "run" / "summary")
    cfg.dir.current_run.checkpoints = str(tmp_path / "run" / "checkpoints")
    cfg.model.concat_before_block_num, cfg.model.stream_2_in_channels = 3, 3
    cfg.agent.max_epoch = 2
    # The step moves nothing (lr 0, no decay): training is not bit-reproducible from run to run (its cross-workgroup sums are atomic),
    # so only then is "the same best_val_iou as a run without the field" a statement about the sweep and not about that noise.
    cfg.optimizer.learning_rate, cfg.optimizer.weight_decay = 0.0, 0.0
    if ema:
        cfg.optimizer.ema_decay = 0.5
    if sweep is not None:
        cfg.agent.threshold_sweep = sweep

    def factory(pretrained=False, config=None, compute_dtype=None, **kw):
        config.model.growth_rate, config.model.block_config, config.model.num_init_features = 8, (2, 2, 2, 2), 16
        return Dense_U_Net_lidar(config, compute_dtype=compute_dtype)
    monkeypatch.setattr(mod, "densenet121_u_lidar", factory)
    agent = mod.Dense_U_Net_lidar_Agent(cfg, torchvision_init=True, compute_dtype="fp32", data_loader=_Loader(batches))
    arch = R.Arch(**TINY, concat_before_block_num=3, stream_2_in_channels=3)
    agent.model.load_state_dict(R.make_state(arch, seed=99))
    if ema:
        agent.optimizer.ema_reset()
    return agent


@pytest.mark.parametrize("ema", [False, True])
def test_agent_sweeps_when_asked_and_only_then(tmp_path, monkeypatch, ema):
    from oracle import restatement as R
    from dmmfods_amd import _lib
    arch = R.Arch(**TINY, concat_before_block_num=3, stream_2_in_channels=3)
    batches = [R.make_inputs(arch, 2, 64, 96, seed=s) for s in range(2)]
    counter = _Counting(_lib.lib())
    monkeypatch.setattr(_lib, "_lib", counter)
    agent = _agent(tmp_path / "a", monkeypatch, batches, 7, ema)
    op = np.float32(agent.config.agent.iou_threshold)
    assert agent.sweep.num_thresholds == 8 and agent.sweep.thresholds[agent.sweep_column] == op
    agent.train()
    assert counter.calls["dmm_logit_hist"] == 2 * 2 and len(agent.val_history) == 2
    for row in agent.val_history:
        sw = row["sweep"]
        assert row.get("ema", False) is ema
        assert all(not v.is_cuda for v in sw.values())
        cols = np.nonzero(sw["thresholds"].numpy() == op)[0]
        assert cols.size == 1 and cols[0] == agent.sweep_column
        assert torch.equal(sw["iou_per_instance"][:, cols[0]], row["iou"]), (sw["iou_per_instance"][:, cols[0]], row["iou"])
        assert int(sw["tp"].sum() + sw["fn"].sum()) > 0 and sw["tp"].dtype == torch.int64
        assert int((sw["tp"] + sw["fp"] + sw["fn"] + sw["tn"])[0, 0]) == 2 * 2 * 64 * 96      # two batches of two samples
        assert sw["best_iou"].shape == (3,) and sw["best_threshold"].shape == (3,)
    best_with = agent.best_val_iou
    agent.model.close()
    counter.calls.clear()
    plain = _agent(tmp_path / "b", monkeypatch, batches, None, ema)
    assert plain.sweep is None
    plain.train()
    assert counter.calls["dmm_logit_hist"] == 0 and all("sweep" not in row for row in plain.val_history)
    assert plain.best_val_iou == best_with, (plain.best_val_iou, best_with)
    assert [torch.equal(a["iou"], b["iou"]) for a, b in zip(agent.val_history, plain.val_history)] == [True, True]
    plain.model.close()
