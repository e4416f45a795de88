"""Cost of the on-device batch augmentation at C2's shapes: B = 4, image + LiDAR + target = 3 + 1 + 3 planes of
1280 x 1920 fp32 (slices of one (4, 7, 1280, 1920) batch), outputs of the same size - 275 MB read and 275 MB written per call.
  (y) the yardstick: torch's device-to-device copy of the same bytes, (4, 7, 1280, 1920) -> (4, 7, 1280, 1920).  NOT the code under test.
  (a) dmm_augment_batch, identity window (y0 = x0 = 0): one aligned 16-byte load and one 16-byte store per lane
  (b) the same window mirrored left-right
  (c) x0 = 1: every quad from the two aligned loads that cover it
  (d) a shifted window with fill (y0 = -37, x0 = 53, a gain and a bias on the image): element paths along two edges
  --lab-lib <a libdmmfods_hip.so whose augment.hip was built with -DDMM_LAB=1, tools/build_variant.sh>: (a) .. (d) again with plain
  16-byte stores in place of the non-temporal ones (DMM_AUG_NT=0), (a') .. (d').
HIP events around every call, REPS calls per variant and round after warm-up, ROUNDS rounds with the variants taking turns inside each
round (so that what else the machine does falls on all of them alike); per variant the median over all calls, the spread of the round
medians, and the ratio to the yardstick.
Then the training loop: C2's net (DenseNet-121, early fusion, fp16, batch 4, 1280 x 1920) with ONE LiDAR plane - the call carries at
most 8 channels, and 3 + 1 + 3 is what the Waymo loader yields; BASELINE's C2 feeds three - stepping on one resident batch, without
and with BatchAugment (flip, shift, crop to the same size, gains, LiDAR dropout) in front of the model, the two taking turns; images
per second from events around each block of steps.  Needs an MI355X:
    python tools/augment_cost.py [--lab-lib <path>] [--no-train] [--out profiles/r14/augment_cost.txt]"""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from dmmfods_amd import _lib  # noqa: E402
from dmmfods_amd.augment import BatchAugment  # noqa: E402

B, H, W = 4, 1280, 1920
CH = (3, 1, 3)
ROUNDS, REPS, WARM = 5, 30, 5
TRAIN_ROUNDS, TRAIN_STEPS, TRAIN_WARM = 3, 10, 4
CASES = [("(a) identity window", 0, 0, 0, False), ("(b) mirrored", 0, 0, 1, False), ("(c) x0 = 1", 0, 1, 0, False),
         ("(d) y0 = -37, x0 = 53, gain, fill", -37, 53, 0, True)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lab-lib", default=None, help="a lab build of the library: the kernel with plain stores (DMM_AUG_NT=0)")
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

    T = (_lib.AugTensor * 3)()
    lo = 0
    for d, ch, o in zip(T, CH, outs):
        d.src, d.dst, d.src_batch_stride, d.channels = batch[:, lo:lo + ch].data_ptr(), o.data_ptr(), batch.stride(0), ch
        lo += ch
    fill = (C.c_float * 7)(*[0.5] * 7)

    def samples(y0, x0, flip, gains):
        S = (_lib.AugSample * B)()
        for b in range(B):
            S[b].y0, S[b].x0, S[b].flip = y0, x0, flip
            for c in range(7):
                S[b].gain[c], S[b].bias[c] = (1.25, -0.5) if gains and c < 3 else (1.0, 0.0)
        return S

    def call(lib, S):
        def run():
            rc = lib.dmm_augment_batch(T, 3, S, B, H, W, H, W, fill, st())
            assert rc == 0, rc
        return run

    variants = [("(y) torch device-to-device copy", lambda: copy_dst.copy_(batch))]
    variants += [(name, call(L, samples(y0, x0, fl, g))) for name, y0, x0, fl, g in CASES]
    if args.lab_lib:
        lab = C.CDLL(os.path.abspath(args.lab_lib))
        lab.dmm_augment_batch.argtypes = L.dmm_augment_batch.argtypes
        os.environ["DMM_AUG_NT"] = "0"   # read once, at the library's first launch (here, before anything is timed)
        call(lab, samples(0, 0, 0, False))()
        os.environ.pop("DMM_AUG_NT", None)
        variants += [(name[:2] + "'" + name[2:] + ", plain stores", call(lab, samples(y0, x0, fl, g))) for name, y0, x0, fl, g in CASES]

    def measure(fn):
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

    calls = {name: [] for name, _ in variants}
    rounds = {name: [] for name, _ in variants}
    for _ in range(ROUNDS):
        for name, fn in variants:
            ts = measure(fn)
            calls[name] += ts
            rounds[name].append(statistics.median(ts))
    # (a) is a copy: the outputs of the last identity call are the batch, bit for bit
    call(L, samples(0, 0, 0, False))()
    assert all(torch.equal(o.view(torch.int32), batch[:, lo:lo + ch].contiguous().view(torch.int32))
               for o, ch, lo in zip(outs, CH, (0, 3, 4)))
    lines = [f"{torch.cuda.get_device_name(0)}; B = {B}, {' + '.join(map(str, CH))} planes of {H} x {W} fp32 to the same size: {nbytes / 1e6:.0f} MB read + written per call",
             f"HIP events around each call, microseconds; {ROUNDS} rounds x {REPS} calls per variant (after {WARM} warm-up calls), the variants taking turns inside a round",
             "variant                                            median   round medians min .. max (spread)    GB/s   time / (y)"]
    ymed = statistics.median(calls[variants[0][0]])
    for name, _ in variants:
        med, lo_, hi = statistics.median(calls[name]), min(rounds[name]), max(rounds[name])
        lines.append(f"{name:50s} {med:7.1f}   {lo_:7.1f} .. {hi:7.1f} ({hi - lo_:5.1f})           {nbytes / med / 1e3:6.0f}   {med / ymed:5.2f}")
    del copy_dst, outs

    if not args.no_train:
        from dmmfods_amd.graphs.models.Dense_U_Net_lidar import Dense_U_Net_lidar
        from dmmfods_amd.optim import FusedAdam
        from dmmfods_amd.utils.Dense_U_Net_lidar_helper import get_config
        cfg = get_config("/tmp/dmm_augment_cost")
        cfg.model.growth_rate, cfg.model.block_config, cfg.model.num_init_features = 32, (6, 12, 24, 16), 64
        cfg.model.concat_before_block_num, cfg.model.stream_2_in_channels = 1, 1
        torch.manual_seed(123)
        model = Dense_U_Net_lidar(cfg, compute_dtype="fp16").to(dev).train()
        opt = FusedAdam(model)
        batch[:, 0:3] *= 255.0
        batch[:, 3:4] = batch[:, 3:4] * 255.0 * (torch.rand((B, 1, H, W), device=dev, generator=gen) > 0.9)
        batch[:, 4:7] = (batch[:, 4:7] > 0.9).float()
        rgb, lidar, tgt = batch[:, 0:3], batch[:, 3:4], batch[:, 4:7]
        aug = BatchAugment(out_size=(H, W), hflip=0.5, translate=(32, 48), brightness=8.0, contrast=0.2, channel_gain=0.1, lidar_dropout=0.1, seed=1)

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
        for augment, name in ((False, "without augmentation"), (True, "with BatchAugment in front of the model")):
            r = rates[augment]
            lines.append(f"  {name:42s} median {statistics.median(r):7.2f}   rounds {', '.join(f'{v:.2f}' for v in r)}")
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
