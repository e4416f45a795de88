"""On-device batch augmentation on the GPU: dmm_augment_batch (csrc/augment.hip) against the numpy restatement of its semantics below,
and what stands on it (dmmfods_amd.augment.BatchAugment, the agent's config.loader.augment).

The oracle is exact.  For sample b, channel c, output pixel (y, x):
    sy = y0 + y;   sx = x0 + (flip ? Wo - 1 - x : x)
    inside the source:  v = src[b][c][sy][sx];  out = v where gain == 1 and bias == 0, else fl(fl(gain * v) + bias)
    outside:            out = fill[c]
and every comparison is BIT FOR BIT - NaN payloads, the sign of zero and infinities included - with one exception that is reasoned,
not measured: where the product or the sum CREATES or PROPAGATES a NaN (0 * inf, inf - inf, a NaN source under a gain), IEEE 754
leaves the sign and payload of the result to the implementation, and the host's SSE unit and the GPU's VALU choose differently
(x86 makes the default NaN negative, 0xffc00000; gfx950 positive, 0x7fc00000).  There - and only in channels that are NOT the
identity - the expected value being a NaN asks for a NaN.  Identity channels and fill pixels keep every bit.

  1. GEOMETRY: one (24, 7, 37, 70) batch (Ws no multiple of 4) passed as three strided tensors (3, 1, 3 channels); x0 in
     {-5, -1, 0, 1, 2, 3, 5, 40} x flip 0 / 1, y0 in {-3, 0, 6}, one window wholly outside; outputs 32 x 64 (16-byte stores) and
     33 x 37 (ragged rows, element stores).  Identity gain, a different non-zero fill per channel.
  2. ALIGNMENT: the 32 x 64 case with every src and dst one element behind a 16-byte boundary.
  3. GAIN AND BIAS: identity, (1.25, -3.5), (0, 0) and random finite pairs mixed over channels and samples.
  4. CHUNKING: B = 33 and B = 65 (two and three launches), every sample with parameters of its own.
  5. 64-BIT OFFSETS: B = 2 with src_batch_stride = 2^31 + 12345 elements (skipped below 12 GB of free device memory).
  6. NOTHING ELSE WRITTEN: sentinel margins around every dst, src unchanged, a second call gives the same bits.
  7. BatchAugment.__call__ on slices of one (4, 7, 96, 128) batch; lidar = None.
  8. THE AGENT: what the model and the loss receive, validation untouched, the checkpoint entry, a resume."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest
import torch

from dmmfods_amd.utils.Dense_U_Net_lidar_helper import get_config

pytestmark = pytest.mark.gpu

DEV = "cuda"
SPECIAL_BITS = np.array([0x7fc12345, 0xffa00001, 0x7f800000, 0xff800000, 0x80000000, 0x7f800001], dtype=np.uint32)   # NaNs with payloads, +-inf, -0
X0S, Y0S = (-5, -1, 0, 1, 2, 3, 5, 40), (-3, 0, 6)
FILL7 = (0.5, -1.5, 2.25, -7.0, 11.0, 1e-3, -3e4)


# ------------------------------------------------------------------------------------------------ the restatement
def restate(src, y0, x0, flip, gain, bias, fill, Ho, Wo):
    """src (B, C, Hs, Ws) float32; y0, x0, flip (B,); gain, bias (B, C); fill (C,).  Returns the uint32 bits of the (B, C, Ho, Wo) output
    and the mask of elements whose value the arithmetic made a NaN (see the head of the file)."""
    src = np.ascontiguousarray(src, dtype=np.float32)
    B, Cn, Hs, Ws = src.shape
    out = np.empty((B, Cn, Ho, Wo), dtype=np.uint32)
    made_nan = np.zeros((B, Cn, Ho, Wo), dtype=bool)
    fill_bits = np.asarray(fill, dtype=np.float32).view(np.uint32)
    ys, xs = np.arange(Ho, dtype=np.int64), np.arange(Wo, dtype=np.int64)
    for b in range(B):
        sy = int(y0[b]) + ys
        sx = int(x0[b]) + (Wo - 1 - xs if flip[b] else xs)
        inside = ((sy >= 0) & (sy < Hs))[:, None] & ((sx >= 0) & (sx < Ws))[None, :]
        syc, sxc = np.clip(sy, 0, Hs - 1)[:, None], np.clip(sx, 0, Ws - 1)[None, :]
        for c in range(Cn):
            v = src[b, c][syc, sxc]
            g, bi = np.float32(gain[b, c]), np.float32(bias[b, c])
            if g == 1 and bi == 0:
                val = v.view(np.uint32)
            else:
                with np.errstate(all="ignore"):
                    w = (g * v).astype(np.float32) + bi
                assert w.dtype == np.float32
                val = w.view(np.uint32)
                made_nan[b, c] = inside & np.isnan(w)
            out[b, c] = np.where(inside, val, fill_bits[c])
    return out, made_nan


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _check(got, want, made_nan, what):
    got = _bits(got) if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape, (what, got.shape, want.shape)
    exact = ~made_nan
    bad = np.flatnonzero((got != want) & exact)
    assert bad.size == 0, (what, bad.size, [np.unravel_index(i, got.shape) for i in bad[:6]], got.ravel()[bad[:6]], want.ravel()[bad[:6]])
    assert np.isnan(got.view(np.float32)[made_nan]).all(), what


def _source(B, Cn, Hs, Ws, seed=0):
    """Distinct per element, with the special patterns sprinkled in (about one element in 40)."""
    n = B * Cn * Hs * Ws
    rng = np.random.default_rng(seed)
    a = ((np.arange(n, dtype=np.float64) - n // 3) * 0.0625).astype(np.float32)
    assert n < 2 ** 24 and np.unique(a).size == n
    pos = rng.choice(n, size=n // 40, replace=False)
    a.view(np.uint32)[pos] = SPECIAL_BITS[np.arange(pos.size) % SPECIAL_BITS.size]
    return a.reshape(B, Cn, Hs, Ws)


# ------------------------------------------------------------------------------------------------ the raw call
def _launch(tensors, y0, x0, flip, gain, bias, fill, Hs, Ws, Ho, Wo):
    """tensors: [(src tensor or (data_ptr, batch stride), channels, dst tensor)]; one dmm_augment_batch call on the current stream."""
    from dmmfods_amd import _lib
    B = len(y0)
    T = (_lib.AugTensor * len(tensors))()
    for d, (src, ch, dst) in zip(T, tensors):
        if isinstance(src, torch.Tensor):
            assert src.stride()[1:] == (Hs * Ws, Ws, 1) and src.shape[1] == ch
            src = (src.data_ptr(), src.stride(0))
        d.src, d.src_batch_stride, d.channels, d.dst = src[0], src[1], ch, dst.data_ptr() if isinstance(dst, torch.Tensor) else dst
    S = (_lib.AugSample * B)()
    nch = sum(ch for _, ch, _ in tensors)
    for b in range(B):
        S[b].y0, S[b].x0, S[b].flip = int(y0[b]), int(x0[b]), int(flip[b])
        for c in range(8):   # (entries past the call's channels are not read: a NaN there must not matter)
            S[b].gain[c], S[b].bias[c] = (float(gain[b, c]), float(bias[b, c])) if c < nch else (float("nan"), float("inf"))
    f = None if fill is None else (C.c_float * nch)(*[float(v) for v in fill])
    _lib.check(_lib.lib().dmm_augment_batch(T, len(tensors), S, B, Hs, Ws, Ho, Wo, f, _lib.stream_ptr()))


def _windows24():
    """x0 crossed with flip (16 samples), then 8 more; y0 cycles through its three values; the last window lies wholly outside."""
    x0 = np.array([X0S[i % 8] for i in range(24)])
    flip = np.array([(i // 8) % 2 if i < 16 else i & 1 for i in range(24)])
    y0 = np.array([Y0S[(i % 8 + i // 8) % 3] for i in range(24)])
    assert {(int(a), int(f)) for a, f in zip(x0[:16], flip[:16])} == {(a, f) for a in X0S for f in (0, 1)}
    assert {(int(a), int(b)) for a, b in zip(x0, y0)} == {(a, b) for a in X0S for b in Y0S}      # every x0 meets every y0 ...
    x0[23], y0[23] = -64, 0                                                                        # ... but for the pair this one replaces
    return y0, x0, flip


@pytest.fixture(scope="module")
def batch24():
    host = _source(24, 7, 37, 70)
    return host, torch.from_numpy(host).to(DEV)


def _three(dev, outs):
    return [(dev[:, 0:3], 3, outs[0]), (dev[:, 3:4], 1, outs[1]), (dev[:, 4:7], 3, outs[2])]


def _split(bits):
    return bits[:, 0:3], bits[:, 3:4], bits[:, 4:7]


# ------------------------------------------------------------------------------------------------ 1. geometry
@pytest.mark.parametrize("Ho,Wo", [(32, 64), (33, 37)])
def test_geometry(batch24, Ho, Wo):
    host, dev = batch24
    y0, x0, flip = _windows24()
    gain, bias = np.ones((24, 7), np.float32), np.zeros((24, 7), np.float32)
    want, made_nan = restate(host, y0, x0, flip, gain, bias, FILL7, Ho, Wo)
    assert not made_nan.any()
    assert (want[23] == np.asarray(FILL7, np.float32).view(np.uint32)[:, None, None]).all()      # the window wholly outside
    outs = [torch.empty((24, ch, Ho, Wo), device=DEV) for ch in (3, 1, 3)]
    _launch(_three(dev, outs), y0, x0, flip, gain, bias, FILL7, 37, 70, Ho, Wo)
    for o, w, name in zip(outs, _split(want), ("image", "lidar", "target")):
        _check(o, w, np.zeros_like(w, dtype=bool), f"geometry {Ho}x{Wo} {name}")
    assert np.array_equal(_bits(dev), host.view(np.uint32))


# ------------------------------------------------------------------------------------------------ 2. alignment
def _behind_boundary(shape, fill_from=None):
    """A contiguous tensor of `shape` whose first element sits 4 bytes behind a 16-byte boundary."""
    n = int(np.prod(shape))
    flat = torch.empty(n + 8, device=DEV)
    off = ((16 - flat.data_ptr() % 16) % 16) // 4 + 1
    t = flat[off:off + n].view(shape)
    assert t.data_ptr() % 16 == 4
    if fill_from is not None:
        t.copy_(fill_from)
    return t


def test_every_pointer_one_element_behind_a_16_byte_boundary(batch24):
    host, dev = batch24
    y0, x0, flip = _windows24()
    gain, bias = np.ones((24, 7), np.float32), np.zeros((24, 7), np.float32)
    want, _ = restate(host, y0, x0, flip, gain, bias, FILL7, 32, 64)
    srcs = [_behind_boundary((24, ch, 37, 70), dev[:, lo:lo + ch]) for lo, ch in ((0, 3), (3, 1), (4, 3))]
    outs = [_behind_boundary((24, ch, 32, 64)) for ch in (3, 1, 3)]
    _launch([(s, s.shape[1], o) for s, o in zip(srcs, outs)], y0, x0, flip, gain, bias, FILL7, 37, 70, 32, 64)
    for o, w, name in zip(outs, _split(want), ("image", "lidar", "target")):
        _check(o, w, np.zeros_like(w, dtype=bool), f"misaligned {name}")


# ------------------------------------------------------------------------------------------------ 3. gain and bias
def test_gain_and_bias(batch24):
    host, dev = batch24
    y0, x0, flip = _windows24()
    rng = np.random.default_rng(5)
    gain = rng.uniform(-3, 3, (24, 7)).astype(np.float32)
    bias = rng.uniform(-100, 100, (24, 7)).astype(np.float32)
    for b in range(24):   # the fixed pairs wander through the channels with the sample
        for k, (g, bi) in enumerate(((1.0, 0.0), (1.25, -3.5), (0.0, 0.0))):
            gain[b, (b + 2 * k) % 7], bias[b, (b + 2 * k) % 7] = g, bi
    gain[3, 5], bias[3, 5] = 1.0, 2.0          # gain 1 alone is not the identity
    gain[4, 5], bias[4, 5] = 0.5, 0.0          # nor is bias 0
    gain[5, 6], bias[5, 6] = 1.0, -0.0         # bias -0 == 0: the identity
    want, made_nan = restate(host, y0, x0, flip, gain, bias, FILL7, 32, 64)
    ident = (gain == 1) & (bias == 0)
    assert ident.sum() >= 24 and made_nan.any() and not made_nan[ident].any()
    outs = [torch.empty((24, ch, 32, 64), device=DEV) for ch in (3, 1, 3)]
    _launch(_three(dev, outs), y0, x0, flip, gain, bias, FILL7, 37, 70, 32, 64)
    got = np.concatenate([_bits(o) for o in outs], axis=1)
    _check(got, want, made_nan, "gain and bias")
    # identity channels carried the special patterns through, bit for bit; every fill pixel is the fill
    carried = got[ident]
    assert all((carried == s).any() for s in SPECIAL_BITS)
    print(f"[augment] gain/bias: {int((~made_nan).sum())} elements bit-equal, {int(made_nan.sum())} NaNs made by the arithmetic, "
          f"{int(ident.sum())} identity (sample, channel) pairs")


# ------------------------------------------------------------------------------------------------ 4. chunking
@pytest.mark.parametrize("B", [33, 65])
def test_more_samples_than_one_launch_carries(B):
    host = _source(B, 7, 9, 13, seed=B)
    dev = torch.from_numpy(host).to(DEV)
    b = np.arange(B)
    y0, x0, flip = b % 5 - 2, b % 7 - 3, b & 1
    gain, bias = np.ones((B, 7), np.float32), np.zeros((B, 7), np.float32)
    gain[:, 0], bias[:, 1] = 1.0 + b / 64.0, b - 20.0
    want, made_nan = restate(host, y0, x0, flip, gain, bias, FILL7, 8, 12)
    assert len({w.tobytes() for w in want}) == B
    outs = [torch.empty((B, ch, 8, 12), device=DEV) for ch in (3, 1, 3)]
    _launch(_three(dev, outs), y0, x0, flip, gain, bias, FILL7, 9, 13, 8, 12)
    _check(np.concatenate([_bits(o) for o in outs], axis=1), want, made_nan, f"B = {B}")


# ------------------------------------------------------------------------------------------------ 5. 64-bit offsets
def test_sample_stride_past_2_31_elements():
    free, _ = torch.cuda.mem_get_info()
    if free < 12 * 2 ** 30:
        pytest.skip(f"needs 12 GB of free device memory, {free / 2 ** 30:.1f} GB are free")
    stride, Cn, Hs, Ws, Ho, Wo = 2 ** 31 + 12345, 2, 37, 70, 32, 64
    host = _source(2, Cn, Hs, Ws, seed=9)
    big = torch.empty(stride + Cn * Hs * Ws, device=DEV)            # 8.6 GB, of which only the two samples' planes are written
    view = big.as_strided((2, Cn, Hs, Ws), (stride, Hs * Ws, Ws, 1))
    view.copy_(torch.from_numpy(host).to(DEV))
    y0, x0, flip = np.array([2, -1]), np.array([3, 5]), np.array([0, 1])
    gain, bias = np.array([[1, 2], [1, 1]], np.float32), np.array([[0, 1], [0, 0]], np.float32)
    want, made_nan = restate(host, y0, x0, flip, gain, bias, FILL7[:2], Ho, Wo)
    out = torch.empty((2, Cn, Ho, Wo), device=DEV)
    _launch([(view, Cn, out)], y0, x0, flip, gain, bias, FILL7[:2], Hs, Ws, Ho, Wo)
    _check(out, want, made_nan, "stride 2^31 + 12345")
    assert np.array_equal(_bits(view), host.view(np.uint32))
    del view, big


# ------------------------------------------------------------------------------------------------ 6. nothing else is written
def test_nothing_else_is_written_and_a_second_call_gives_the_same_bits(batch24):
    host, dev = batch24
    y0, x0, flip = _windows24()
    gain, bias = np.ones((24, 7), np.float32), np.zeros((24, 7), np.float32)
    gain[:, 1], bias[:, 4] = 0.75, 3.0
    MARGIN, SENT = 1024, 0x7fa5a5a5
    for Ho, Wo in ((32, 64), (33, 37)):
        fill = FILL7 if Ho == 33 else None                           # (a null fill: zeros)
        want, made_nan = restate(host, y0, x0, flip, gain, bias, fill or (0,) * 7, Ho, Wo)
        bufs, outs = [], []
        for ch in (3, 1, 3):
            n = 24 * ch * Ho * Wo
            buf = torch.full((n + 2 * MARGIN,), SENT, dtype=torch.int32, device=DEV)
            bufs.append(buf)
            outs.append(buf[MARGIN:MARGIN + n].view(torch.float32).view(24, ch, Ho, Wo))
        first = None
        for _ in range(2):
            _launch(_three(dev, outs), y0, x0, flip, gain, bias, fill, 37, 70, Ho, Wo)
            got = np.concatenate([_bits(o) for o in outs], axis=1)
            _check(got, want, made_nan, f"sentinels {Ho}x{Wo}")
            for buf in bufs:
                m = buf.cpu().numpy()
                assert (m[:MARGIN] == SENT).all() and (m[-MARGIN:] == SENT).all()
            first = got if first is None else first
            assert np.array_equal(got, first)
            for o in outs:                       # (the second call has to write every element again)
                o.view(torch.int32).fill_(SENT)
    assert np.array_equal(_bits(dev), host.view(np.uint32))


# ------------------------------------------------------------------------------------------------ 7. BatchAugment
def _restate_params(batch_host, p, fill, with_lidar=True):
    from dmmfods_amd.augment import BatchAugment
    src = batch_host if with_lidar else np.concatenate([batch_host[:, :3], batch_host[:, 4:]], axis=1)
    gain, bias = BatchAugment.channel_tables(p, 3, 1 if with_lidar else 0, 3)
    return restate(src, p.y0, p.x0, p.flip, gain, bias, fill, *p.out_size)


def test_batch_augment_call_equals_the_restatement_under_params_at():
    from dmmfods_amd.augment import BatchAugment
    host = _source(4, 7, 96, 128, seed=3)
    dev = torch.from_numpy(host).to(DEV)
    aug = BatchAugment(out_size=(64, 96), hflip=0.5, translate=(7, 9), brightness=0.3, contrast=0.4, channel_gain=0.2, lidar_dropout=0.3,
                       image_dropout=0.3, fill=list(FILL7), seed=12, rank=1)
    seen = set()
    for i in range(3):
        p = aug.params_at(i, 4, 96, 128)
        seen |= {("flip", int(f)) for f in p.flip} | {("dl", bool(d)) for d in p.drop_lidar} | {("di", bool(d)) for d in p.drop_image}
        image, lidar, target = aug(dev[:, 0:3], dev[:, 3:4], dev[:, 4:7])
        assert aug.batches_drawn == i + 1 and image.shape == (4, 3, 64, 96) and lidar.shape == (4, 1, 64, 96) and target.shape == (4, 3, 64, 96)
        want, made_nan = _restate_params(host, p, FILL7)
        _check(np.concatenate([_bits(image), _bits(lidar), _bits(target)], axis=1), want, made_nan, f"BatchAugment batch {i}")
    assert seen == {("flip", 0), ("flip", 1), ("dl", False), ("dl", True), ("di", False), ("di", True)}, seen   # the three batches took every branch
    # explicit params: nothing advances, the same bits again
    p = aug.params_at(1, 4, 96, 128)
    again = aug(dev[:, 0:3], dev[:, 3:4], dev[:, 4:7], params=p)
    want, made_nan = _restate_params(host, p, FILL7)
    _check(np.concatenate([_bits(t) for t in again], axis=1), want, made_nan, "explicit params")
    assert aug.batches_drawn == 3
    # lidar = None: image and target alone, a fill of one number, a contiguous (not sliced) image
    solo = BatchAugment(out_size=(64, 96), hflip=0.5, translate=(7, 9), contrast=0.4, lidar_dropout=0.5, fill=2.5, seed=12)
    p = solo.params_at(0, 4, 96, 128)
    image, lidar, target = solo(dev[:, 0:3].contiguous(), None, dev[:, 4:7])
    assert lidar is None and solo.batches_drawn == 1
    want, made_nan = _restate_params(host, p, (2.5,) * 6, with_lidar=False)
    _check(np.concatenate([_bits(image), _bits(target)], axis=1), want, made_nan, "lidar = None")
    # out_size None: the source's size; all strengths zero: a copy, bit for bit
    image, lidar, target = BatchAugment()(dev[:, 0:3], dev[:, 3:4], dev[:, 4:7])
    assert np.array_equal(np.concatenate([_bits(image), _bits(lidar), _bits(target)], axis=1), host.view(np.uint32))
    assert np.array_equal(_bits(dev), host.view(np.uint32))
    with pytest.raises(ValueError):
        aug(dev[:, 0:3], dev[:, 3:4], dev[:2, 4:7])
    with pytest.raises(ValueError):
        aug(dev[:, 0:3].double(), dev[:, 3:4], dev[:, 4:7])
    with pytest.raises(ValueError):
        aug(dev[:, 0:3], dev[:, 3:7], dev[:, 0:7])                    # 14 channels
    assert aug.batches_drawn == 3


# ------------------------------------------------------------------------------------------------ 8. the agent
class _Loader:
    def __init__(self, batches):
        self.train_loader, self.train_iterations = batches, len(batches)
        self.valid_loader, self.valid_iterations = batches[:1], 1


def _agent(tmp_path, monkeypatch, batches, augment, resume=False):
    from dmmfods_amd.agents import Dense_U_Net_lidar_Agent as mod
    from dmmfods_amd.graphs.models.Dense_U_Net_lidar import Dense_U_Net_lidar
    cfg = get_config(str(tmp_path))
    cfg.dir.current_run.summary = str(tmp_path / "run" / "summary")
    cfg.dir.current_run.checkpoints = str(tmp_path / "run" / "checkpoints")
    if augment is not None:
        cfg.loader.augment = augment

    def factory(pretrained=False, config=None, compute_dtype=None, **kw):
        config.model.growth_rate, config.model.block_config, config.model.num_init_features = 8, (2, 2, 2, 2), 16
        return Dense_U_Net_lidar(config, compute_dtype=compute_dtype)
    monkeypatch.setattr(mod, "densenet121_u_lidar", factory)
    agent = mod.Dense_U_Net_lidar_Agent(cfg, torchvision_init=not resume, compute_dtype="fp32", data_loader=_Loader(batches))
    # what the model and the two loss tails receive
    agent.seen = {"forward": [], "loss_backward": [], "loss_metrics": []}
    model = agent.model
    fwd, lb, lm = model.forward, model.loss_backward, model.loss_metrics

    def forward(image, lidar):
        agent.seen["forward"].append((model.training, _bits(image).copy(), _bits(lidar).copy()))
        return fwd(image, lidar)

    def loss_backward(target):
        agent.seen["loss_backward"].append(_bits(target).copy())
        return lb(target)

    def loss_metrics(logits, target):
        agent.seen["loss_metrics"].append(_bits(target).copy())
        return lm(logits, target)
    model.forward, model.loss_backward, model.loss_metrics = forward, loss_backward, loss_metrics
    return agent


def test_agent_augments_training_batches_only_and_a_resume_continues(tmp_path, monkeypatch):
    host = [_source(2, 7, 96, 128, seed=20 + s) for s in range(2)]
    for h in host:   # finite inputs for the net: the special patterns stay in the kernel's own tests
        h[~np.isfinite(h)] = 1.0
        h[:, 4:] = (h[:, 4:] > 0).astype(np.float32)
    batches = [(torch.from_numpy(h[:, 0:3].copy()), torch.from_numpy(h[:, 3:4].copy()), torch.from_numpy(h[:, 4:7].copy())) for h in host]
    spec = dict(out_size=(64, 96), hflip=0.5, translate=(5, 6), brightness=2.0, contrast=0.3, channel_gain=0.1, lidar_dropout=0.25, seed=4)
    agent = _agent(tmp_path / "a", monkeypatch, batches, spec)
    assert agent.augment is not None and agent.augment.state_dict() == {"seed": 4, "rank": 0, "batches_drawn": 0}
    agent.train_one_epoch()
    assert agent.augment.batches_drawn == 2 and len(agent.seen["forward"]) == 2 and len(agent.seen["loss_backward"]) == 2

    def check_train(agent, k, i):
        want, made_nan = _restate_params(host[k], agent.augment.params_at(i, 2, 96, 128), (0,) * 7)
        training, image, lidar = agent.seen["forward"][-2 + k]
        assert training and image.shape == (2, 3, 64, 96)
        _check(np.concatenate([image, lidar, agent.seen["loss_backward"][-2 + k]], axis=1), want, made_nan, f"agent batch {i}")
    for k in range(2):
        check_train(agent, k, k)
    with torch.no_grad():
        agent.validate()
    training, image, lidar = agent.seen["forward"][-1]
    assert not training and agent.augment.batches_drawn == 2           # validation: the loader's tensors, untouched
    assert np.array_equal(np.concatenate([image, lidar, agent.seen["loss_metrics"][-1]], axis=1), host[0].view(np.uint32))
    agent.save_checkpoint(is_best=True)
    name = agent.config.agent.best_checkpoint_name
    ck = torch.load(os.path.join(agent.config.dir.current_run.checkpoints, name), map_location="cpu")
    assert set(ck) == {"epoch", "train_iteration", "val_iteration", "best_val_iou", "state_dict", "optimizer", "augment"}
    assert ck["augment"] == {"seed": 4, "rank": 0, "batches_drawn": 2}
    agent.model.close()
    # a resumed agent goes on with batch 2 (its own seed argument does not matter: the checkpoint's comes back)
    os.makedirs(str(tmp_path / "b" / "run" / "checkpoints"), exist_ok=True)
    shutil.copy(os.path.join(agent.config.dir.current_run.checkpoints, name), str(tmp_path / "b" / "run" / "checkpoints" / name))
    resumed = _agent(tmp_path / "b", monkeypatch, batches, dict(spec, seed=99), resume=True)
    assert resumed.augment.state_dict() == {"seed": 4, "rank": 0, "batches_drawn": 2}
    resumed.train_one_epoch()
    for k in range(2):
        check_train(resumed, k, 2 + k)
    resumed.model.close()
    # without the field: no augmentation, today's checkpoint keys, the loader's tensors reach the model
    plain = _agent(tmp_path / "c", monkeypatch, batches, None)
    assert plain.augment is None
    plain.train_one_epoch()
    training, image, lidar = plain.seen["forward"][-1]
    assert np.array_equal(np.concatenate([image, lidar, plain.seen["loss_backward"][-1]], axis=1), host[1].view(np.uint32))
    plain.save_checkpoint(is_best=True)
    pck = torch.load(os.path.join(plain.config.dir.current_run.checkpoints, name), map_location="cpu")
    assert set(pck) == {"epoch", "train_iteration", "val_iteration", "best_val_iou", "state_dict", "optimizer"}
    plain.model.close()
    # an agent WITH the field resumed from that checkpoint starts at batch 0
    os.makedirs(str(tmp_path / "d" / "run" / "checkpoints"), exist_ok=True)
    shutil.copy(os.path.join(plain.config.dir.current_run.checkpoints, name), str(tmp_path / "d" / "run" / "checkpoints" / name))
    late = _agent(tmp_path / "d", monkeypatch, batches, spec, resume=True)
    assert late.augment.state_dict() == {"seed": 4, "rank": 0, "batches_drawn": 0}
    late.model.close()
