"""Cost of dmm_heat_components at C2's validation shape, 4 x 3 x 1280 x 1920 fp32 (118 MB), against
  (a) dmm_logit_hist on the same tensor (19 thresholds; the map is also passed as its target, so it reads 236 MB): the launch that
      reads those bytes once - the yardstick for "how far above one read are we"
  (b) the copy to the host plus scipy.ndimage.label + find_objects per plane, where scipy is importable: what a user does today
      (a few calls only: it takes seconds)
on two inputs: random rectangles at a realistic density (a few dozen boxes per plane) and i.i.d. noise at 50 % foreground, the
adversarial case for the merge.  Before anything is timed the GPU result on the rectangles input is checked against scipy's, up to
relabelling (labels), and exactly on boxes and areas.
HIP events around every call, REPS calls per variant and round after warm-up, ROUNDS rounds with the variants taking turns inside each
round; per variant the median over all calls and the spread of the round medians.
--lab-lib <a libdmmfods_hip.so whose components.hip was built with -DDMM_LAB=1, tools/build_variant.sh>: the call is also timed cut
behind its first k launches (DMM_CC_LAUNCHES=k), k = 1 .. 7, and each launch is reported as the difference of two prefixes.
Needs an MI355X:
    python tools/components_cost.py [--lab-lib <path>] [--out profiles/r15/components_cost.txt]"""
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
from dmmfods_amd.metrics import logit_thresholds  # noqa: E402

B, NC, H, W = 4, 3, 1280, 1920
CAP = 1024
ROUNDS, REPS, WARM = 5, 20, 5
BYTES = B * NC * H * W * 4
LAUNCHES = ("cc_local", "cc_merge", "cc_flatten", "cc_scan", "cc_slots", "cc_stats", "cc_finish")


def rectangles_input(seed):
    """About forty non-touching boxes per plane, 8 .. 200 pixels a side, value 1.0 on 0.0 (cut at 0.7)."""
    rng = np.random.default_rng(seed)
    maps = np.zeros((B, NC, H, W), dtype=np.float32)
    for b in range(B):
        for n in range(NC):
            used = np.zeros((H, W), dtype=bool)
            placed = 0
            while placed < 40:
                h, w = int(rng.integers(8, 200)), int(rng.integers(8, 200))
                y, x = int(rng.integers(0, H - h)), int(rng.integers(0, W - w))
                if used[max(0, y - 1):y + h + 1, max(0, x - 1):x + w + 1].any():
                    continue
                used[y:y + h, x:x + w] = True
                maps[b, n, y:y + h, x:x + w] = 1.0
                placed += 1
    return maps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lab-lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    L = _lib.lib()
    dev = "cuda"
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    lab_lib = None
    if args.lab_lib:
        lab_lib = C.CDLL(os.path.abspath(args.lab_lib))
        lab_lib.dmm_heat_components.argtypes = L.dmm_heat_components.argtypes
    nbytes = L.dmm_heat_components_workspace(B, NC, H, W, CAP)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    labels = torch.empty((B, NC, H, W), dtype=torch.int32, device=dev)
    records = torch.empty((B, NC, CAP, 8), dtype=torch.int32, device=dev)
    counts = torch.empty((B, NC), dtype=torch.int32, device=dev)
    K = 19
    thr = logit_thresholds([(k + 1) / (K + 1) for k in range(K)])
    thr_c = (C.c_float * K)(*thr.tolist())
    hist_counts = torch.empty((B, NC, 2, K + 1), dtype=torch.int64, device=dev)

    def measure(fn, reps=REPS, warm=WARM):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
        return ts

    lines = [f"{torch.cuda.get_device_name(0)}; maps {B} x {NC} x {H} x {W} fp32 ({BYTES / 1e6:.0f} MB), max_per_plane {CAP}, 8-connectivity, HIP events around each call, microseconds",
             f"{ROUNDS} rounds x {REPS} calls per variant (after {WARM} warm-up calls), the variants taking turns inside a round",
             f"byte floor of the call: one {BYTES / 1e6:.0f} MB read, one label write and two label reads = {4 * BYTES / 1e6:.0f} MB"]
    inputs = [("rectangles, 40 boxes per plane", rectangles_input(0), 0.7),
              ("i.i.d. noise, 50 % foreground", np.random.default_rng(1).uniform(0, 1, (B, NC, H, W)).astype(np.float32), 0.5)]
    for which, maps_np, cut in inputs:
        maps = torch.from_numpy(maps_np).to(dev)

        def components(lib=L, lab=labels):
            rc = lib.dmm_heat_components(maps.data_ptr(), B, NC, H, W, cut, 8, CAP, ws.data_ptr(), nbytes, lab.data_ptr() if lab is not None else None,
                                         records.data_ptr(), counts.data_ptr(), st())
            assert rc == 0, rc

        def hist():
            rc = L.dmm_logit_hist(maps.data_ptr(), maps.data_ptr(), B, NC, H, W, thr_c, K, 0.7, 0, hist_counts.data_ptr(), st())
            assert rc == 0, rc

        def host_scipy():
            m = maps.cpu().numpy()
            out = []
            for b in range(B):
                for n in range(NC):
                    lab, k = ndimage.label(m[b, n] >= np.float32(cut), structure=np.ones((3, 3)))
                    out.append((lab, k, ndimage.find_objects(lab)))
            return out

        components()
        torch.cuda.synchronize()
        cnt = counts.cpu().numpy()
        if ndimage is not None and which.startswith("rectangles"):
            got_lab = labels.cpu().numpy()
            rec = records.cpu().numpy()
            for i, (lab, k, objs) in enumerate(host_scipy()):
                b, n = divmod(i, NC)
                assert k == cnt[b, n], "the component counts differ from scipy's"
                g = got_lab[b, n]
                assert np.array_equal(g >= 0, lab > 0)
                pairs = np.unique(np.stack([g[g >= 0], lab[lab > 0]]), axis=1)   # a bijection between the two labellings
                assert pairs.shape[1] == k and np.unique(pairs[0]).size == k and np.unique(pairs[1]).size == k
                theirs = sorted((s[1].start, s[0].start, s[1].stop - 1, s[0].stop - 1, int((lab[s] == j + 1).sum())) for j, s in enumerate(objs))
                ours = sorted(tuple(int(v) for v in r[1:6]) for r in rec[b, n, :k])
                assert ours == theirs, "boxes or areas differ from scipy's"
            lines.append("checked against scipy.ndimage.label / find_objects on the rectangles input: labels up to relabelling, boxes and areas exactly")
        variants = [("(a) dmm_logit_hist (reads 236 MB)", hist), ("dmm_heat_components, labels returned", components),
                    ("dmm_heat_components, labels = NULL", lambda: components(L, None))]
        calls = {name: [] for name, _ in variants}
        rounds = {name: [] for name, _ in variants}
        for _ in range(ROUNDS):
            for name, fn in variants:
                ts = measure(fn)
                calls[name] += ts
                rounds[name].append(statistics.median(ts))
        lines.append("")
        lines.append(f"{which} (cut at {cut}): {int(cnt.min())} .. {int(cnt.max())} components per plane")
        lines.append("variant                                   median   round medians min .. max (spread)")
        med = {}
        for name, _ in variants:
            med[name], lo, hi = statistics.median(calls[name]), min(rounds[name]), max(rounds[name])
            lines.append(f"{name:40s} {med[name]:8.1f}   {lo:8.1f} .. {hi:8.1f} ({hi - lo:6.1f})")
        a, c = variants[0][0], variants[1][0]
        lines.append(f"the call over (a): {med[c]:.1f} / {med[a]:.1f} = {med[c] / med[a]:.2f}x;  {4 * BYTES / med[c] / 1e3:.0f} GB/s of the byte floor")
        if ndimage is not None:
            ts = []
            for _ in range(2):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                host_scipy()
                ts.append((time.perf_counter() - t0) * 1e6)
            lines.append(f"(b) copy to the host + scipy.ndimage.label + find_objects, 12 planes: {min(ts) / 1e3:.0f} ms (best of 2) = {min(ts) / med[c]:.0f}x the call")
        else:
            lines.append("(b) scipy is not importable here: left out")
        if lab_lib is not None:
            prefix = []
            for k in range(1, len(LAUNCHES) + 1):
                os.environ["DMM_CC_LAUNCHES"] = str(k)
                prefix.append(statistics.median(measure(lambda: components(lab_lib, labels), reps=30)))
            os.environ.pop("DMM_CC_LAUNCHES", None)
            parts = [prefix[0]] + [prefix[k] - prefix[k - 1] for k in range(1, len(prefix))]
            lines.append("per launch (lab build, differences of the call cut behind k launches): " +
                         ", ".join(f"{n} {p:.1f}" for n, p in zip(LAUNCHES, parts)) + f"  (sum {prefix[-1]:.1f})")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
