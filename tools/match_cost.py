"""Cost of object matching for one validation batch at C2's validation shape: B = 4 samples, NC = 3 classes,
objects of a 1280 x 1920 frame, with 40 and with 1024 objects a plane (predictions and ground truth alike), max_per_plane 1024.
The records are synthetic (tools/match_cases.py: a jittered grid, contests and score ties) and live on the device, as
dmm_heat_components leaves them.
  (a) what ObjectMetrics.update() does: two Detections.to_host() - the stall and the two copies - plus match_objects in Python.
      Wall clock around the whole, the stream idle before it.  This is the host path as the parent commit has it (detect.py's
      to_host / match_objects are unchanged), not code under test.
  (b) dmm_match_objects: HIP events around the call; with --lab-lib also cut behind its first k launches (DMM_MATCH_LAUNCHES=k), each
      launch reported as the difference of two prefixes.
  (e) an empty stream round trip - two events around nothing - and one trivial launch (a one-element fill): what "a launch overhead"
      is on this machine, the yardstick for the claim that (b) at 40 objects costs a few of them.
Before anything is timed (b)'s result is checked against (a)'s on the same records.
ROUNDS rounds with the paths taking turns inside a round, REPS calls per path and round after warm-up; per path the median over all
calls and the spread of the round medians.  At 1024 objects a plane one call of (a) takes tens of seconds (12 planes x a million
box_iou calls in Python), so it is timed --host-big-calls times (default 1) and not in turns.  Needs an MI355X:
    python tools/match_cost.py [--lab-lib <path>] [--out profiles/r18/match_cost.txt]"""
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
from dmmfods_amd.detect import Detections, match_objects  # noqa: E402
from tools import match_cases as M  # noqa: E402

B, NC, CAP = 4, 3, 1024
ROUNDS, REPS, WARM = 5, 20, 3
LAUNCHES = ("match_count", "match_offsets", "match_plane")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lab-lib", default=None)
    ap.add_argument("--host-big-calls", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    L = _lib.lib()
    dev = "cuda"
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    lab_lib = None
    if args.lab_lib:
        lab_lib = C.CDLL(os.path.abspath(args.lab_lib))
        lab_lib.dmm_match_objects.argtypes = L.dmm_match_objects.argtypes
    nbytes = L.dmm_match_objects_workspace(B, NC, CAP, CAP)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    capacity = 1 << 20
    totals = torch.zeros((NC, 8), dtype=torch.int64, device=dev)
    entries = torch.empty((NC, capacity, 2), dtype=torch.int32, device=dev)
    matched = torch.empty((B, NC, CAP), dtype=torch.uint8, device=dev)
    one = torch.zeros(1, device=dev)

    def events(fn, reps=REPS, warm=WARM):
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

    def wall(fn, reps=REPS, warm=WARM):
        for _ in range(warm):
            fn()
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e6)
        return ts

    lines = [f"{torch.cuda.get_device_name(0)}; B = {B}, NC = {NC}, max_per_plane {CAP}, boxes of a 1280 x 1920 frame, iou 0.5, min_area 1; microseconds",
             f"command line: python tools/match_cost.py {' '.join(sys.argv[1:])}",
             f"{ROUNDS} rounds x {REPS} calls per path (after {WARM} warm-up calls), the paths taking turns inside a round; (a) wall clock, the others HIP events"]
    for objects in (40, CAP):
        planes = [M.jittered(objects, objects, seed=300 + i, frame=1280) for i in range(B * NC)]
        pa, pc = M.pack([p for p, _ in planes], B, NC, CAP)
        ga, gc = M.pack([g for _, g in planes], B, NC, CAP)
        dp = Detections(torch.from_numpy(pa).to(dev), torch.from_numpy(pc).to(dev), None, 1)
        dg = Detections(torch.from_numpy(ga).to(dev), torch.from_numpy(gc).to(dev), None, 1)

        def device(lib=L):
            rc = lib.dmm_match_objects(dp.records.data_ptr(), dp.counts.data_ptr(), CAP, dg.records.data_ptr(), dg.counts.data_ptr(), CAP, B, NC, 1, 0.5,
                                       ws.data_ptr(), nbytes, matched.data_ptr(), totals.data_ptr(), entries.data_ptr(), capacity, st())
            assert rc == 0, rc

        def host():
            return match_objects(dp.to_host(), dg.to_host(), 0.5)

        big = objects > 100
        lines.append("")
        lines.append(f"{objects} objects a plane, predictions and ground truth ({B * NC} planes)")
        totals.zero_()
        device()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        want = host()
        first_host = (time.perf_counter() - t0) * 1e6
        got = totals.cpu().numpy()
        assert np.array_equal(got[:, 0], want["tp"]) and np.array_equal(got[:, 1], want["fp"]) and np.array_equal(got[:, 2], want["fn"])
        m = matched.cpu().numpy()
        for b in range(B):
            for n in range(NC):
                assert np.array_equal(m[b, n, :objects].astype(bool), want["matched"][b][n])
        lines.append(f"checked: tp {want['tp'].tolist()}, fp {want['fp'].tolist()}, fn {want['fn'].tolist()} and every matched flag equal on both paths")
        variants = [("(b) dmm_match_objects", lambda: device(), events), ("(e) empty stream round trip", lambda: None, events),
                    ("(e) one trivial launch", lambda: one.fill_(1.0), events)]
        if not big:
            variants.insert(0, ("(a) 2 x to_host() + match_objects", host, wall))
        calls = {name: [] for name, _, _ in variants}
        rounds = {name: [] for name, _, _ in variants}
        for _ in range(ROUNDS):
            for name, fn, measure in variants:
                ts = measure(fn)
                calls[name] += ts
                rounds[name].append(statistics.median(ts))
        lines.append("path                                      median   round medians min .. max (spread)")
        med = {}
        for name, _, _ in variants:
            med[name], lo, hi = statistics.median(calls[name]), min(rounds[name]), max(rounds[name])
            lines.append(f"{name:40s} {med[name]:9.1f}   {lo:9.1f} .. {hi:9.1f} ({hi - lo:7.1f})")
        if big:
            ts = [first_host] + wall(host, reps=args.host_big_calls - 1, warm=0) if args.host_big_calls > 1 else [first_host]
            lines.append(f"(a) 2 x to_host() + match_objects: {min(ts) / 1e6:.1f} s (best of {len(ts)} call(s), wall clock, NOT in turns with the others) "
                         f"= {min(ts) / med['(b) dmm_match_objects']:.0f}x (b)")
        else:
            lines.append(f"(a) over (b): {med['(a) 2 x to_host() + match_objects'] / med['(b) dmm_match_objects']:.1f}x;  "
                         f"(b) over one trivial launch: {med['(b) dmm_match_objects'] / med['(e) one trivial launch']:.1f}x")
        if lab_lib is not None:
            prefix = []
            for k in range(1, len(LAUNCHES) + 1):
                os.environ["DMM_MATCH_LAUNCHES"] = str(k)
                prefix.append(statistics.median(events(lambda: device(lab_lib), reps=30)))
            os.environ.pop("DMM_MATCH_LAUNCHES", None)
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
