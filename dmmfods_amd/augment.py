"""Training-time augmentation of a batch that already sits on the device (nothing upstream: the reference feeds the model what its
loader yields).

``dmm_augment_batch`` (csrc/augment.hip) reads a per-sample window of every plane of image, LiDAR and target - cropped or shifted,
optionally mirrored left-right, with a per-channel gain and bias - and writes new tensors, in one launch per 32 samples.  The
rearrangements are label-preserving: the three tensors move together, the heat-map values are left-right symmetric, and targets
never get a gain or a bias.  With a ``scale`` or a ``rotate`` the launch is ``dmm_warp_batch`` (csrc/warp.hip) instead: the same
window seen through a zoom and a rotation about its centre, a fixed-point affine map per sample; the image is interpolated
bilinearly, LiDAR and target are sampled nearest, so a heat-map level stays a level and a LiDAR code is never averaged.  The parameters are drawn on the host from a counter-based generator, so batch number ``i`` of rank
``r`` has the same parameters wherever and whenever it is drawn; nothing is drawn on the device and nothing is synchronised."""
import ctypes as C
import math
import types

import numpy as np
import torch

from . import _lib

MAX_CHANNELS = _lib.AUG_MAX_CHANNELS
WARP_ONE = 1 << _lib.WARP_FRAC_BITS


def _pair(v, name):
    if isinstance(v, (int, np.integer)) and not isinstance(v, bool):
        v = (v, v)
    try:
        a, b = (int(x) for x in v)
        exact = all(float(x) == int(x) for x in v)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be an integer or a pair of integers") from None
    if not exact:
        raise ValueError(f"{name} must be an integer or a pair of integers")
    return a, b


class BatchAugment:
    """Per-sample crop, shift, horizontal flip, image gain / bias and modality dropout of a device batch.

    out_size        (Ho, Wo) of the outputs; None: the source's size.  Smaller than the source: a random crop.
    hflip           probability that a sample is mirrored left-right.
    translate       (ty, tx): the window is moved by whole pixels, uniform in [-ty, ty] x [-tx, tx]; where it overhangs the source
                    the outputs hold `fill`.
    brightness      image bias, uniform in [-brightness, brightness], one draw per sample.
    contrast        image gain factor, uniform in [1 - contrast, 1 + contrast], one draw per sample.
    channel_gain    image gain factor, uniform in [1 - channel_gain, 1 + channel_gain], one draw per sample AND channel.
                    The gain of an image channel is contrast_draw * per_channel_draw (formed in double, rounded to fp32 once).
    lidar_dropout   probability that a sample's LiDAR tensor is blanked (gain 0, bias 0).
    image_dropout   the same for the image tensor; never the same sample as lidar_dropout (lidar_dropout + image_dropout <= 1).
    scale           zoom factor s, uniform in [1 - scale, 1 + scale], one draw per sample; scale in [0, 63/64] (the launch takes matrix
                    entries up to 64, and 1 / s is one).  s > 1 magnifies.
    rotate          degrees, in [0, 180]; the angle is uniform in [-rotate, rotate], one draw per sample.
    fill            what a window shows outside the source: None (zeros), one number, or one number per channel (image channels,
                    then LiDAR, then target).  Gain and bias do not touch it.
    seed, rank      the generator's key.  Give every data-parallel rank its own `rank`.

    The parameters of batch ``i`` are a pure function of (seed, rank, i, B, Hs, Ws): ``params_at(i, B, Hs, Ws)``.  They come from
    ``numpy.random.Generator(numpy.random.Philox(key=(seed, rank), counter=(0, i, 0, 0)))`` - batches sit 2^64 counter blocks apart, so
    their streams never meet - with these draws, each a vector over the B samples, ALWAYS all of them and in this order (a strength
    of 0 still takes its draw, so turning one knob does not move the others):
      1. flip          random(B) < hflip
      2. crop y        integers(0, max(Hs - Ho, 0) + 1, B)
      3. crop x        integers(0, max(Ws - Wo, 0) + 1, B)
      4. shift y       integers(-ty, ty + 1, B)                 y0 = crop y + shift y
      5. shift x       integers(-tx, tx + 1, B)                 x0 = crop x + shift x
      6. contrast      uniform(1 - contrast, 1 + contrast, B)
      7. channel gain  uniform(1 - channel_gain, 1 + channel_gain, (B, 8))      an image of C channels uses the first C columns
      8. brightness    uniform(-brightness, brightness, B)
      9. dropout       u = random(B):  u < lidar_dropout blanks the LiDAR tensor,  lidar_dropout <= u < lidar_dropout + image_dropout the image
     10. zoom          uniform(1 - scale, 1 + scale, B)
     11. angle         uniform(-rotate, rotate, B)              degrees
    THE MAP.  Zoom and rotation act about the window's centre; today's window and flip follow.  For output pixel (x, y) of a sample with
    zoom s and angle t, with u = x - (Wo - 1) / 2 and v = y - (Ho - 1) / 2:
        (u', v') = (1 / s) R(t) (u, v),     R(t) = [[cos t, -sin t], [sin t, cos t]]
        xw = u' + (Wo - 1) / 2;   yw = v' + (Ho - 1) / 2
        sx = x0 + (flip ? Wo - 1 - xw : xw);   sy = y0 + yw
    ``matrices`` forms the six coefficients of (x, y) -> (sx, sy) in double and rounds each with ``numpy.rint`` to Q20, the fixed point
    of ``dmm_warp_batch``; at s = 1, t = 0 they are whole numbers and the map is the window's.  With scale == 0 and rotate == 0
    ``__call__`` issues ``dmm_augment_batch`` as it always did; otherwise ``dmm_warp_batch`` with the image bilinear, LiDAR and target nearest.
    Targets always get gain 1 and bias 0.  ``__call__`` draws batch number ``batches_drawn`` and advances; ``state_dict`` carries
    that counter, so a resumed run continues the sequence."""

    def __init__(self, out_size=None, hflip=0.0, translate=(0, 0), brightness=0.0, contrast=0.0, channel_gain=0.0, lidar_dropout=0.0,
                 image_dropout=0.0, fill=None, seed=0, rank=0, scale=0.0, rotate=0.0):
        if out_size is not None:
            out_size = _pair(out_size, "out_size")
            if min(out_size) < 1:
                raise ValueError("out_size must be positive")
        self.out_size = out_size
        self.translate = _pair(translate, "translate")
        if min(self.translate) < 0 or max(self.translate) > 1 << 29:
            raise ValueError("translate must be a pair of integers in [0, 2^29]")
        for name, p in (("hflip", hflip), ("lidar_dropout", lidar_dropout), ("image_dropout", image_dropout)):
            if not 0.0 <= float(p) <= 1.0:   # (NaN fails both comparisons)
                raise ValueError(f"{name} is a probability: it must lie in [0, 1]")
        if float(lidar_dropout) + float(image_dropout) > 1.0:
            raise ValueError("lidar_dropout + image_dropout must be at most 1 (they never hit the same sample)")
        for name, s in (("contrast", contrast), ("channel_gain", channel_gain)):
            if not 0.0 <= float(s) < 1.0:
                raise ValueError(f"{name} must lie in [0, 1)")
        if not (float(brightness) >= 0.0 and math.isfinite(float(brightness))):
            raise ValueError("brightness must be finite and >= 0")
        if not 0.0 <= float(scale) <= 63.0 / 64.0:
            raise ValueError("scale must lie in [0, 63/64]")
        if not 0.0 <= float(rotate) <= 180.0:
            raise ValueError("rotate is in degrees: it must lie in [0, 180]")
        self.scale, self.rotate = float(scale), float(rotate)
        if fill is not None:
            fill = [float(fill)] if isinstance(fill, (int, float, np.number)) else [float(v) for v in fill]
            if not 1 <= len(fill) <= MAX_CHANNELS or not all(math.isfinite(v) for v in fill):
                raise ValueError(f"fill: one finite number, or one per channel (at most {MAX_CHANNELS})")
        for name, v in (("seed", seed), ("rank", rank)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) < 1 << 64:
                raise ValueError(f"{name} must be an integer in [0, 2^64)")
        self.hflip, self.brightness, self.contrast, self.channel_gain = float(hflip), float(brightness), float(contrast), float(channel_gain)
        self.lidar_dropout, self.image_dropout = float(lidar_dropout), float(image_dropout)
        self.fill = fill
        self.seed, self.rank = int(seed), int(rank)
        self.batches_drawn = 0

    # ------------------------------------------------------------------ parameters
    def output_size(self, Hs, Ws):
        return self.out_size if self.out_size is not None else (int(Hs), int(Ws))

    def params_at(self, i, B, Hs, Ws):
        """The parameters of batch number `i` (B samples of Hs x Ws); does not advance.  A namespace of numpy arrays over the samples:
        y0, x0, flip (int32), image_gain (B, 8) and image_bias (B,) (float32), drop_lidar, drop_image (bool), zoom and angle (float64, the
        angle in degrees); out_size (Ho, Wo)."""
        i, B, Hs, Ws = int(i), int(B), int(Hs), int(Ws)
        if i < 0 or B < 1 or Hs < 1 or Ws < 1:
            raise ValueError("params_at(i, B, Hs, Ws): i >= 0 and B, Hs, Ws >= 1")
        Ho, Wo = self.output_size(Hs, Ws)
        ty, tx = self.translate
        rng = np.random.Generator(np.random.Philox(key=np.array([self.seed, self.rank], dtype=np.uint64),
                                                   counter=np.array([0, i, 0, 0], dtype=np.uint64)))
        flip = rng.random(B) < self.hflip
        y0 = rng.integers(0, max(Hs - Ho, 0) + 1, B)
        x0 = rng.integers(0, max(Ws - Wo, 0) + 1, B)
        y0 = y0 + rng.integers(-ty, ty + 1, B)
        x0 = x0 + rng.integers(-tx, tx + 1, B)
        contrast = rng.uniform(1.0 - self.contrast, 1.0 + self.contrast, B)
        per_channel = rng.uniform(1.0 - self.channel_gain, 1.0 + self.channel_gain, (B, MAX_CHANNELS))
        bias = rng.uniform(-self.brightness, self.brightness, B)
        u = rng.random(B)
        zoom = rng.uniform(1.0 - self.scale, 1.0 + self.scale, B)
        angle = rng.uniform(-self.rotate, self.rotate, B)
        return types.SimpleNamespace(
            y0=y0.astype(np.int32), x0=x0.astype(np.int32), flip=flip.astype(np.int32),
            image_gain=(contrast[:, None] * per_channel).astype(np.float32), image_bias=bias.astype(np.float32),
            drop_lidar=u < self.lidar_dropout, drop_image=(u >= self.lidar_dropout) & (u < self.lidar_dropout + self.image_dropout),
            zoom=zoom, angle=angle, out_size=(Ho, Wo))

    @staticmethod
    def channel_tables(params, image_channels, lidar_channels, target_channels):
        """(gain, bias): float32 (B, channels) over the call's channels - image, LiDAR, target in this order - as the launch gets them."""
        ci, cl, ct = int(image_channels), int(lidar_channels), int(target_channels)
        if ci < 1 or cl < 0 or ct < 1 or ci + cl + ct > MAX_CHANNELS:
            raise ValueError(f"image, LiDAR and target must have between them at most {MAX_CHANNELS} channels")
        B = len(params.y0)
        gain, bias = np.ones((B, ci + cl + ct), dtype=np.float32), np.zeros((B, ci + cl + ct), dtype=np.float32)
        gain[:, :ci] = params.image_gain[:, :ci]
        bias[:, :ci] = params.image_bias[:, None]
        gain[params.drop_image, :ci] = 0.0
        bias[params.drop_image, :ci] = 0.0
        gain[params.drop_lidar, ci:ci + cl] = 0.0
        return gain, bias

    @staticmethod
    def matrices(params, Hs=None, Ws=None):
        """(a, b): int32 (B, 2, 2) and int64 (B, 2) - a00, a01, a10, a11 and b0, b1 of every sample in Q20, as dmm_warp_batch gets them
        (see THE MAP above; the source size does not enter the map and is accepted for symmetry with params_at)."""
        Ho, Wo = params.out_size
        cx, cy = (Wo - 1) / 2.0, (Ho - 1) / 2.0
        t = np.deg2rad(np.asarray(params.angle, dtype=np.float64))
        s = np.asarray(params.zoom, dtype=np.float64)
        m = np.empty((len(s), 2, 2), dtype=np.float64)
        m[:, 0, 0], m[:, 0, 1], m[:, 1, 0], m[:, 1, 1] = np.cos(t) / s, -np.sin(t) / s, np.sin(t) / s, np.cos(t) / s
        off = np.array([cx, cy]) - m @ np.array([cx, cy])           # (xw, yw) = m (x, y) + off
        flip = np.asarray(params.flip) != 0
        m[flip, 0, :] = -m[flip, 0, :]
        off[:, 0] = np.where(flip, (Wo - 1) - off[:, 0], off[:, 0])
        off[:, 0] += np.asarray(params.x0, dtype=np.float64)
        off[:, 1] += np.asarray(params.y0, dtype=np.float64)
        return np.rint(m * WARP_ONE).astype(np.int32), np.rint(off * WARP_ONE).astype(np.int64)

    # ------------------------------------------------------------------ the launch
    def __call__(self, image, lidar, target, params=None):
        """Returns new (image, lidar, target) tensors of the output size (lidar: None when None was given).  The inputs are fp32 (B, C, H, W)
        device tensors whose planes and channels are contiguous - channel slices of one (B, 7, H, W) batch are.  params: use these
        (from params_at) and do not advance; None: draw batch number `batches_drawn` and advance."""
        tensors = [t for t in (image, lidar, target) if t is not None]
        if image is None or target is None or not all(torch.is_tensor(t) for t in tensors):
            raise ValueError("image and target must be tensors (lidar may be None)")
        if not all(t.is_cuda for t in tensors):
            raise RuntimeError("dmmfods_amd computes on the GPU only; move image, lidar and target to 'cuda' (no CPU fallback)")
        B, _, Hs, Ws = image.shape if image.dim() == 4 else (0, 0, 0, 0)
        for t in tensors:
            if t.dim() != 4 or t.dtype != torch.float32 or t.shape[0] != B or tuple(t.shape[2:]) != (Hs, Ws) or t.device != image.device:
                raise ValueError("image, lidar and target must be fp32 (B, C, H, W) tensors of one batch size, image size and device")
            if t.numel() == 0:
                raise ValueError("empty tensor")
        nch = [t.shape[1] for t in tensors]
        if sum(nch) > MAX_CHANNELS:
            raise ValueError(f"image, LiDAR and target must have between them at most {MAX_CHANNELS} channels")
        if params is None:
            params = self.params_at(self.batches_drawn, B, Hs, Ws)
            self.batches_drawn += 1
        elif len(params.y0) != B:
            raise ValueError("params were drawn for another batch size")
        Ho, Wo = params.out_size
        gain, bias = self.channel_tables(params, image.shape[1], 0 if lidar is None else lidar.shape[1], target.shape[1])
        warp = self.scale != 0.0 or self.rotate != 0.0
        samples = ((_lib.WarpSample if warp else _lib.AugSample) * B)()
        if warp:
            ma, mb = self.matrices(params, Hs, Ws)
        for b in range(B):
            s = samples[b]
            if warp:
                (s.a00, s.a01), (s.a10, s.a11) = ma[b].tolist()
                s.b0, s.b1 = mb[b].tolist()
            else:
                s.y0, s.x0, s.flip = int(params.y0[b]), int(params.x0[b]), int(params.flip[b])
            s.gain[:sum(nch)] = gain[b].tolist()
            s.bias[:sum(nch)] = bias[b].tolist()
        descs = ((_lib.WarpTensor if warp else _lib.AugTensor) * len(tensors))()
        outs = []
        for d, t in zip(descs, tensors):
            if warp:
                d.mode = _lib.WARP_BILINEAR if t is image else _lib.WARP_NEAREST
            ch = t.shape[1]
            t = t.detach()
            sb, sc, sh, sw = t.stride()
            if B == 1:
                sb = ch * Hs * Ws       # (a stride nothing is multiplied with)
            if (sc, sh, sw) != (Hs * Ws, Ws, 1) or sb < ch * Hs * Ws:
                t = t.contiguous()      # a layout the launch does not read (channels-last, a spatial slice): one copy
                sb = ch * Hs * Ws
            out = torch.empty((B, ch, Ho, Wo), dtype=torch.float32, device=t.device)
            d.src, d.dst, d.src_batch_stride, d.channels = t.data_ptr(), out.data_ptr(), sb, ch
            outs.append((t, out))       # (keeps a contiguous copy alive until the launch is enqueued)
        fill = None
        if self.fill is not None:
            if len(self.fill) not in (1, sum(nch)):
                raise ValueError(f"fill has {len(self.fill)} values, the call has {sum(nch)} channels")
            fill = (C.c_float * sum(nch))(*(self.fill * sum(nch) if len(self.fill) == 1 else self.fill))
        with torch.cuda.device(image.device):
            entry = _lib.lib().dmm_warp_batch if warp else _lib.lib().dmm_augment_batch
            _lib.check(entry(descs, len(tensors), samples, B, Hs, Ws, Ho, Wo, fill, _lib.stream_ptr()))
        res = [o for _, o in outs]
        return (res[0], None, res[1]) if lidar is None else (res[0], res[1], res[2])

    # ------------------------------------------------------------------ resuming
    def state_dict(self):
        return {"seed": self.seed, "rank": self.rank, "batches_drawn": self.batches_drawn}

    def load_state_dict(self, state):
        self.seed, self.rank, self.batches_drawn = int(state["seed"]), int(state["rank"]), int(state["batches_drawn"])
