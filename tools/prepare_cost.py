"""Cost of the device-side batch preparation at C2's shapes: B = 4 frames of 1280 x 1920 - uint8 image, 30 000
LiDAR points and 40 boxes per frame - to the (4, 7, Ho, Wo) fp32 batch, at pool 1 (the model's full-size input) and pool 10 (the
reference's stored size).
  (y) the yardstick of bandwidth: torch's device-to-device copy of a (4, 7, 1280, 1920) fp32 tensor.  NOT the code under test.
  (a) dmm_augment_batch, identity window, producing the same (4, 7, Ho, Wo) output from a batch of that size: an existing
      one-read-one-write launch
  the three launches - dmm_prep_image, dmm_prep_lidar (memset + splat + pool), dmm_prep_heat_maps - each alone and all three in a row,
  and BatchPrepare.__call__ from pinned host memory (the copies of the compact arrays included)
  (b) what a user does today: the host preparation in torch / numpy on the CPU (average pool of the image, the per-point splat loop,
      the coding and max pool, the boxes drawn into three planes and max-pooled), wall clock, and the copy of the prepared fp32 batch
      from pinned memory to the device
  (c) the byte floor of each launch: the bytes it has to read and write, at the bandwidth (y) reached
HIP events around every call, REPS calls per variant and round after warm-up, ROUNDS rounds with the variants taking turns inside each
round; per variant the median over all calls and the spread of the round medians.  Needs an MI355X:
    python tools/prepare_cost.py [--out profiles/r16/prepare_cost.txt]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from dmmfods_amd import _lib  # noqa: E402
from dmmfods_amd.prepare import BatchPrepare, collate_raw  # noqa: E402
from tools import prepare_ref as R  # noqa: E402

B, H, W, K = 4, 1280, 1920, 5
NPOINTS, NBOXES = 30000, 40
ROUNDS, REPS, WARM = 5, 20, 3
HOST_REPS = 2


def frames(rng):
    out = []
    for _ in range(B):
        pts = np.stack([rng.uniform(0, W, NPOINTS), rng.uniform(0, H, NPOINTS), rng.uniform(0, 80, NPOINTS)], axis=1).astype(np.float32)
        boxes = np.stack([rng.choice([1, 2, 4], NBOXES), rng.integers(0, W - 300, NBOXES), rng.integers(0, H - 300, NBOXES),
                          rng.integers(20, 300, NBOXES), rng.integers(20, 300, NBOXES)], axis=1).astype(np.int32)
        out.append(dict(image=torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)), points=torch.from_numpy(pts),
                        boxes=torch.from_numpy(boxes)))
    return out


def host_prepare(frame, p):
    """One frame on the CPU, the way the reference's helper does it (its splat is a Python loop over the points)."""
    image = torch.nn.AvgPool2d(p, stride=p)(frame["image"].permute(2, 0, 1).float()) if p > 1 else frame["image"].permute(2, 0, 1).float()
    owner = R.lidar_owner(frame["points"].numpy(), H, W, K)
    d = frame["points"].numpy()[:, 2]
    coded = torch.from_numpy(R.lidar_code(np.where(owner >= 0, d[np.maximum(owner, 0)], np.float32(-1))))[None]
    if p > 1:
        coded = torch.nn.functional.pad(torch.nn.MaxPool2d((2 * p, p), stride=(p, p))(coded)[None], pad=(0, 0, 0, 1), mode="replicate")[0]
    lidar = coded.clamp_min(0)
    maps = torch.from_numpy(R.heat_maps_full(frame["boxes"].numpy(), H, W))
    if p > 1:
        maps = torch.nn.MaxPool2d(p, stride=p)(maps)
    return torch.cat([image, lidar, maps])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    L = _lib.lib()
    dev = "cuda"
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    raw = collate_raw(frames(np.random.default_rng(16)), pin_memory=True)
    image, points, boxes = raw.image.to(dev), raw.points.to(dev), raw.boxes.to(dev)
    po = np.ascontiguousarray(raw.point_offsets.numpy(), dtype=np.int32)
    bo = np.ascontiguousarray(raw.box_offsets.numpy(), dtype=np.int32)
    pop, bop = po.ctypes.data_as(C.POINTER(C.c_int32)), bo.ctypes.data_as(C.POINTER(C.c_int32))
    need = L.dmm_prep_lidar_workspace(B, H, W)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    big = torch.rand((B, 7, H, W), device=dev)
    big_dst = torch.empty_like(big)

    variants = [("(y) torch device-to-device copy, (4, 7, 1280, 1920)", lambda: big_dst.copy_(big), 2 * big.numel() * 4)]
    keep = []
    for p in (1, 10):
        Ho, Wo = H // p, W // p
        plane = Ho * Wo
        out = torch.empty((B, 7, Ho, Wo), device=dev)
        src = big if p == 1 else torch.rand((B, 7, Ho, Wo), device=dev)
        T = (_lib.AugTensor * 3)()
        for d, (lo, ch) in zip(T, ((0, 3), (3, 1), (4, 3))):
            d.src, d.dst, d.src_batch_stride, d.channels = src[:, lo:lo + ch].data_ptr(), out.data_ptr() + 4 * B * lo * plane, src.stride(0), ch
        S = (_lib.AugSample * B)()
        for b in range(B):
            for c in range(8):
                S[b].gain[c], S[b].bias[c] = 1.0, 0.0
        keep += [out, src, T, S]
        ptr, stride = out.data_ptr(), out.stride(0)

        def aug(T=T, S=S, Ho=Ho, Wo=Wo):
            assert L.dmm_augment_batch(T, 3, S, B, Ho, Wo, Ho, Wo, None, st()) == 0

        def prep_image(ptr=ptr, stride=stride, p=p):
            assert L.dmm_prep_image(image.data_ptr(), H * W * 3, ptr, stride, B, H, W, 3, p, st()) == 0

        def prep_lidar(ptr=ptr, stride=stride, p=p, plane=plane):
            assert L.dmm_prep_lidar(points.data_ptr(), pop, ptr + 12 * plane, stride, B, H, W, p, K, ws.data_ptr(), need, st()) == 0

        def prep_heat(ptr=ptr, stride=stride, p=p, plane=plane):
            assert L.dmm_prep_heat_maps(boxes.data_ptr(), bop, ptr + 16 * plane, stride, B, H, W, p, st()) == 0

        def all_three(f=(prep_image, prep_lidar, prep_heat)):
            for g in f:
                g()
        bp = BatchPrepare(pool=p, kernel_size=K)
        owner = B * H * W * 4
        variants += [
            (f"pool {p:2d}: (a) dmm_augment_batch, identity, same output", aug, 2 * B * 7 * plane * 4),
            (f"pool {p:2d}: dmm_prep_image", prep_image, B * H * W * 3 + B * 3 * plane * 4),
            (f"pool {p:2d}: dmm_prep_lidar (memset, splat, pool)", prep_lidar, owner + owner * (2 if p > 1 else 1) + B * NPOINTS * 12 + B * plane * 4),
            (f"pool {p:2d}: dmm_prep_heat_maps", prep_heat, B * NBOXES * 20 + B * 3 * plane * 4),
            (f"pool {p:2d}: the three in a row", all_three, None),
            (f"pool {p:2d}: BatchPrepare(raw) from pinned memory", lambda bp=bp: bp(raw), None),
        ]
        # what is timed is what the tests check: the three slices against the restatement of frame 0
        all_three()
        torch.cuda.synchronize()
        want = R.batch(raw.image.numpy()[:1], raw.points.numpy()[:po[1]], po[:2], raw.boxes.numpy()[:bo[1]], bo[:2], p, K)
        assert np.array_equal(out[:1].cpu().numpy().view(np.uint32), want.view(np.uint32)), p

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

    calls = {name: [] for name, _, _ in variants}
    rounds = {name: [] for name, _, _ in variants}
    for _ in range(ROUNDS):
        for name, fn, _ in variants:
            ts = measure(fn)
            calls[name] += ts
            rounds[name].append(statistics.median(ts))
    ymed = statistics.median(calls[variants[0][0]])
    ybw = variants[0][2] / ymed / 1e3   # GB/s
    lines = [f"{torch.cuda.get_device_name(0)}; B = {B} frames of {H} x {W}: uint8 image, {NPOINTS} points and {NBOXES} boxes per frame, kernel_size {K}",
             f"HIP events around each call, microseconds; {ROUNDS} rounds x {REPS} calls per variant (after {WARM} warm-up calls), the variants taking turns inside a round",
             f"(c) byte floor: the bytes a launch must read and write, at the {ybw:.0f} GB/s that (y) reaches",
             "variant                                                     median   round medians min .. max (spread)    MB moved   floor (c)   time / floor"]
    for name, _, nbytes in variants:
        med, lo_, hi = statistics.median(calls[name]), min(rounds[name]), max(rounds[name])
        tail = f"{nbytes / 1e6:9.1f}   {nbytes / ybw / 1e3:8.1f}   {med / (nbytes / ybw / 1e3):8.2f}" if nbytes else ""
        lines.append(f"{name:58s} {med:8.1f}   {lo_:8.1f} .. {hi:8.1f} ({hi - lo_:6.1f})      {tail}")
    for p in (1, 10):
        a = statistics.median(calls[f"pool {p:2d}: (a) dmm_augment_batch, identity, same output"])
        t = statistics.median(calls[f"pool {p:2d}: the three in a row"])
        lines.append(f"pool {p:2d}: the three launches / (a) = {t / a:.2f}")

    # (b) the host path: preparation on the CPU, then the copy of the fp32 batch from pinned memory
    fr = [dict(image=raw.image[b], points=raw.points[po[b]:po[b + 1]], boxes=raw.boxes[bo[b]:bo[b + 1]]) for b in range(B)]
    lines.append(f"(b) host path, {torch.get_num_threads()} torch threads: CPU preparation of the {B} frames (wall clock, best of {HOST_REPS}), then the copy of the fp32 batch from pinned memory (events, median of {REPS})")
    for p in (1, 10):
        best, batch = None, None
        for _ in range(HOST_REPS):
            t0 = time.perf_counter()
            batch = torch.stack([host_prepare(f, p) for f in fr])
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        assert np.array_equal(batch[:1].numpy().view(np.uint32),
                              R.batch(raw.image.numpy()[:1], raw.points.numpy()[:po[1]], po[:2], raw.boxes.numpy()[:bo[1]], bo[:2], p, K).view(np.uint32))
        pinned = batch.pin_memory()
        dst = torch.empty_like(pinned, device=dev)
        ts = measure(lambda: dst.copy_(pinned, non_blocking=True))
        med = statistics.median(ts)
        lines.append(f"  pool {p:2d}: CPU preparation {best * 1e3:9.1f} ms; copy of {pinned.numel() * 4 / 1e6:6.1f} MB {med:9.1f} us ({pinned.numel() * 4 / med / 1e3:5.1f} GB/s)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
