"""Cost of the on-device affine warp at C2's shapes: B = 4, image + LiDAR + target = 3 + 1 + 3 planes of
1280 x 1920 fp32 (slices of one (4, 7, 1280, 1920) batch), outputs of the same size - 275 MB written per call and, where the map stays
inside the source, as much read.  The image is sampled bilinearly, LiDAR and target nearest, as BatchAugment does it.
  (y) yardstick 1: torch's device-to-device copy of the same bytes.  NOT the code under test.
  (w) yardstick 2: dmm_augment_batch on the identity window.
  dmm_warp_batch with the map of BatchAugment.matrices about the window's centre:
  (a) the identity matrix (a lattice map: both modes copy)      (b) a shift by half a pixel in x and y: all four taps live
  (c) 5 degrees      (d) 30 degrees      (e) zoom 0.8      (f) zoom 1.25
  --lab-lib <a libdmmfods_hip.so whose warp.hip was built with -DDMM_LAB=1, tools/build_variant.sh>: (a) .. (f) again for every
  candidate tile shape (DMM_WARP_LXB = 3 .. 6: 32 x 32, 64 x 16, 128 x 8, 256 x 4 pixels) and, at the shape that ships, with plain
  16-byte stores in place of the non-temporal ones (DMM_WARP_NT=0).
HIP events around every call, REPS calls per variant and round after warm-up, ROUNDS rounds with the variants taking turns inside each
round (so that what else the machine does falls on all of them alike); per variant the median over all calls, the spread of the round
medians, and the ratios to the two yardsticks.
Then the training loop: C2's net (DenseNet-121, early fusion, fp16, batch 4, 1280 x 1920) with ONE LiDAR plane, stepping on one
resident batch, without and with BatchAugment(scale, rotate, flip, shift, gains) in front of the model, the two taking turns; images
per second from events around each block of steps.  Needs an MI355X:
    python tools/warp_cost.py [--lab-lib <path>] [--no-train] [--out profiles/r17/warp_cost.txt]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from dmmfods_amd import _lib  # noqa: E402
from dmmfods_amd.augment import BatchAugment  # noqa: E402

B, H, W = 4, 1280, 1920
CH = (3, 1, 3)
ROUNDS, REPS, WARM = 5, 30, 5
TRAIN_ROUNDS, TRAIN_STEPS, TRAIN_WARM = 3, 10, 4
HALF = 1 << (_lib.WARP_FRAC_BITS - 1)
# (name, angle in degrees, zoom, offset added to b0 and b1)
CASES = [("(a) identity matrix", 0.0, 1.0, 0), ("(b) half-pixel shift", 0.0, 1.0, HALF), ("(c) 5 degrees", 5.0, 1.0, 0),
         ("(d) 30 degrees", 30.0, 1.0, 0), ("(e) zoom 0.8", 0.0, 0.8, 0), ("(f) zoom 1.25", 0.0, 1.25, 0)]
SHAPES = {3: "32 x 32", 4: "64 x 16", 5: "128 x 8", 6: "256 x 4"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lab-lib", default=None, help="a lab build of the library: every tile shape and both store kinds")
    ap.add_argument("--no-train", action="store_true", help="skip the training loop")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    L = _lib.lib()
    dev = "cuda"
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    gen = torch.Generator(device=dev).manual_seed(0)
    batch = torch.rand((B, sum(CH), H, W), device=dev, generator=gen)
    outs = [torch.empty((B, ch, H, W), device=dev) for ch in CH]
    copy_dst = torch.empty_like(batch)
    nbytes = 2 * batch.numel() * 4

    TA, TW = (_lib.AugTensor * 3)(), (_lib.WarpTensor * 3)()
    lo = 0
    for da, dw, ch, o in zip(TA, TW, CH, outs):
        for d in (da, dw):
            d.src, d.dst, d.src_batch_stride, d.channels = batch[:, lo:lo + ch].data_ptr(), o.data_ptr(), batch.stride(0), ch
        dw.mode = _lib.WARP_BILINEAR if lo == 0 else _lib.WARP_NEAREST
        lo += ch
    fill = (C.c_float * 7)(*[0.5] * 7)

    SA = (_lib.AugSample * B)()
    for b in range(B):
        for c in range(7):
            SA[b].gain[c], SA[b].bias[c] = 1.0, 0.0

    def warp_samples(angle, zoom, shift):
        p = types.SimpleNamespace(y0=np.zeros(B, np.int32), x0=np.zeros(B, np.int32), flip=np.zeros(B, np.int32), zoom=np.full(B, zoom),
                                  angle=np.full(B, angle), out_size=(H, W))
        ma, mb = BatchAugment.matrices(p, H, W)
        S = (_lib.WarpSample * B)()
        for b in range(B):
            (S[b].a00, S[b].a01), (S[b].a10, S[b].a11) = ma[b].tolist()
            S[b].b0, S[b].b1 = int(mb[b, 0]) + shift, int(mb[b, 1]) + shift
            for c in range(7):
                S[b].gain[c], S[b].bias[c] = 1.0, 0.0
        return S

    def warp_call(lib, S):
        def run():
            rc = lib.dmm_warp_batch(TW, 3, S, B, H, W, H, W, fill, st())
            assert rc == 0, rc
        return run

    def aug_call():
        rc = L.dmm_augment_batch(TA, 3, SA, B, H, W, H, W, fill, st())
        assert rc == 0, rc

    def env(**kw):
        def prep():
            for k in ("DMM_WARP_LXB", "DMM_WARP_NT"):
                os.environ.pop(k, None)
            os.environ.update(kw)
        return prep

    # (name, what to put into the environment before the variant's turn, the call)
    variants = [("(y) torch device-to-device copy", env(), lambda: copy_dst.copy_(batch)), ("(w) dmm_augment_batch, identity window", env(), aug_call)]
    variants += [(name, env(), warp_call(L, warp_samples(ang, zoom, sh))) for name, ang, zoom, sh in CASES]
    if args.lab_lib:
        lab = C.CDLL(os.path.abspath(args.lab_lib))
        lab.dmm_warp_batch.argtypes = L.dmm_warp_batch.argtypes
        for lxb, shape in SHAPES.items():
            variants += [(f"{name[:3]} tile {shape}", env(DMM_WARP_LXB=str(lxb)), warp_call(lab, warp_samples(ang, zoom, sh))) for name, ang, zoom, sh in CASES]
        variants += [(f"{name[:3]} shipped tile, plain stores", env(DMM_WARP_NT="0"), warp_call(lab, warp_samples(ang, zoom, sh))) for name, ang, zoom, sh in CASES]

    def measure(prep, fn):
        prep()
        for _ in range(WARM):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(REPS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
        return ts

    calls = {name: [] for name, _, _ in variants}
    rounds = {name: [] for name, _, _ in variants}
    for _ in range(ROUNDS):
        for name, prep, fn in variants:
            ts = measure(prep, fn)
            calls[name] += ts
            rounds[name].append(statistics.median(ts))
    env()()
    # (a) is a copy: the outputs of an identity call are the batch, bit for bit - from every library and tile shape measured
    for lib, preps in ((L, [env()]), (lab if args.lab_lib else None, [env(DMM_WARP_LXB=str(k)) for k in SHAPES])):
        for prep in preps if lib is not None else []:
            prep()
            for o in outs:
                o.zero_()
            warp_call(lib, warp_samples(0.0, 1.0, 0))()
            assert all(torch.equal(o.view(torch.int32), batch[:, lo:lo + ch].contiguous().view(torch.int32)) for o, ch, lo in zip(outs, CH, (0, 3, 4)))
    env()()
    lines = [f"{torch.cuda.get_device_name(0)}; B = {B}, {' + '.join(map(str, CH))} planes of {H} x {W} fp32 to the same size: {nbytes / 1e6:.0f} MB read + written per copy",
             f"HIP events around each call, microseconds; {ROUNDS} rounds x {REPS} calls per variant (after {WARM} warm-up calls), the variants taking turns inside a round",
             "variant                                            median   round medians min .. max (spread)   time / (y)   time / (w)"]
    ymed, wmed = statistics.median(calls[variants[0][0]]), statistics.median(calls[variants[1][0]])
    for name, _, _ in variants:
        med, lo_, hi = statistics.median(calls[name]), min(rounds[name]), max(rounds[name])
        lines.append(f"{name:50s} {med:7.1f}   {lo_:7.1f} .. {hi:7.1f} ({hi - lo_:5.1f})            {med / ymed:5.2f}        {med / wmed:5.2f}")
    del copy_dst, outs

    if not args.no_train:
        from dmmfods_amd.graphs.models.Dense_U_Net_lidar import Dense_U_Net_lidar
        from dmmfods_amd.optim import FusedAdam
        from dmmfods_amd.utils.Dense_U_Net_lidar_helper import get_config
        cfg = get_config("/tmp/dmm_warp_cost")
        cfg.model.growth_rate, cfg.model.block_config, cfg.model.num_init_features = 32, (6, 12, 24, 16), 64
        cfg.model.concat_before_block_num, cfg.model.stream_2_in_channels = 1, 1
        torch.manual_seed(123)
        model = Dense_U_Net_lidar(cfg, compute_dtype="fp16").to(dev).train()
        opt = FusedAdam(model)
        batch[:, 0:3] *= 255.0
        batch[:, 3:4] = batch[:, 3:4] * 255.0 * (torch.rand((B, 1, H, W), device=dev, generator=gen) > 0.9)
        batch[:, 4:7] = (batch[:, 4:7] > 0.9).float()
        rgb, lidar, tgt = batch[:, 0:3], batch[:, 3:4], batch[:, 4:7]
        aug = BatchAugment(out_size=(H, W), hflip=0.5, translate=(32, 48), brightness=8.0, contrast=0.2, channel_gain=0.1, lidar_dropout=0.1, seed=1,
                           scale=0.2, rotate=10.0)

        def step(augment):
            x1, x2, t = aug(rgb, lidar, tgt) if augment else (rgb, lidar, tgt)
            with torch.no_grad():
                model(x1, x2)
            model.loss_backward(t)
            opt.step()

        def block(augment, n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(n):
                step(augment)
            b.record()
            b.synchronize()
            return B * n / (a.elapsed_time(b) * 1e-3)

        for augment in (False, True):
            block(augment, TRAIN_WARM)
        rates = {False: [], True: []}
        for _ in range(TRAIN_ROUNDS):
            for augment in (False, True):
                rates[augment].append(block(augment, TRAIN_STEPS))
        assert bool(torch.isfinite(model.param_arena).all())
        lines.append(f"training loop, DenseNet-121 early fusion, 3 + 1 input planes, fp16, batch {B}, {H} x {W}: {TRAIN_ROUNDS} rounds x {TRAIN_STEPS} steps per variant "
                     f"(after {TRAIN_WARM}), taking turns; images / second per round")
        for augment, name in ((False, "without augmentation"), (True, "with BatchAugment(scale 0.2, rotate 10) in front")):
            r = rates[augment]
            lines.append(f"  {name:48s} median {statistics.median(r):7.2f}   rounds {', '.join(f'{v:.2f}' for v in r)}")
        w, wo = statistics.median(rates[True]), statistics.median(rates[False])
        lines.append(f"  with / without = {w / wo:.4f}  ({(1 / w - 1 / wo) * B * 1e6:+.0f} us a step)")
        model.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
