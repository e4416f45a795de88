"""Cost of gradient accumulation at C2 (d121 early fusion, batch 4, 1280 x 1920, fp16 storage), mode off against mode
on in ONE process on one MI355X, alternating, two rounds:
  * step time (forward + loss_backward + Adam; with the mode on zero_grad() in front: a window of one micro-batch) and the micro-step
    alone (forward + loss_backward), HIP events around each step, median of --steps after warm-up;
  * the in-step time of the `unpack` launches (a profile filtered to that class runs the two-stream schedule of production);
  * from an unfiltered profile (everything on one stream, each launch bracketed alone): the arena's memset, the `unpack` launches and the
    unlabelled launches behind the loss kernel (the BatchNorm-backward finalize kernels; stream joins launch nothing).
Needs an MI355X:  python tools/accum_cost.py [--steps 30]"""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from dmmfods_amd import _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--config", default="c2", choices=sorted(bench.CONFIGS))
args = ap.parse_args()
L = _lib.lib()
dev = torch.device("cuda:0")
w = bench.Workload(bench.CONFIGS[args.config], dev, 0, False, False)
m, opt = w.model, w.opt


def micro():
    with torch.no_grad():
        m(w.rgb, w.lidar)
    m.loss_backward(w.tgt)


def full():
    opt.zero_grad()       # a no-op with the mode off
    micro()
    opt.step()


def timed(fn, n):
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
    torch.cuda.synchronize()
    marks[0].record()
    for i in range(n):
        fn()
        marks[i + 1].record()
    torch.cuda.synchronize()
    ts = [marks[i].elapsed_time(marks[i + 1]) for i in range(n)]
    return statistics.median(ts), min(ts), max(ts)


def profile(prefix, passes):
    """Per-launch milliseconds of the backward list, averaged over `passes` steps: [(index, label, ms)]."""
    plan = m._last[0]
    _lib.check(L.dmm_plan_profile_filter(plan.handle, prefix))
    _lib.check(L.dmm_plan_profile_begin(plan.handle, passes))
    for _ in range(passes):
        full()
    torch.cuda.synchronize()
    n = L.dmm_plan_profile_num_ops(plan.handle, 1)
    ms, got = (C.c_double * n)(), C.c_int()
    _lib.check(L.dmm_plan_profile_collect(plan.handle, 1, ms, n, C.byref(got)))
    _lib.check(L.dmm_plan_profile_begin(plan.handle, 0))
    _lib.check(L.dmm_plan_profile_filter(plan.handle, None))
    out = []
    for i in range(n):
        label = C.c_char_p()
        L.dmm_plan_profile_op(plan.handle, 1, i, C.byref(label), None, None)
        out.append((i, (label.value or b"").decode(), ms[i] / max(got.value, 1)))
    return out


for _ in range(10):
    full()
print(f"{w.c['name']}: {m.num_params} parameters, arena {4 * m.num_params / 1e6:.1f} MB", flush=True)
for rnd in range(2):
    for on in (False, True):
        m.set_grad_accumulation(on)
        for _ in range(3):
            full()
        tag = f"round {rnd} mode {'on ' if on else 'off'}"
        med, lo, hi = timed(full, args.steps)
        print(f"{tag} step       median {med:7.3f} ms  min {lo:7.3f}  max {hi:7.3f}", flush=True)
        med, lo, hi = timed(micro, args.steps)
        print(f"{tag} micro-step median {med:7.3f} ms  min {lo:7.3f}  max {hi:7.3f}", flush=True)
        opt.zero_grad()
        ops = profile(b"unpack", 10)
        un = [t for _, lab, t in ops if lab.startswith("unpack")]
        print(f"{tag} in-step unpack: {len(un)} launches, {1e3 * sum(un):7.1f} us per step", flush=True)
        ops = profile(None, 3)
        first_labelled = next(i for i, lab, _ in ops if lab)          # the loss kernel
        un = sum(t for _, lab, t in ops if lab.startswith("unpack"))
        memsets = [t for i, lab, t in ops if i < first_labelled]
        other = [t for i, lab, t in ops if i > first_labelled and not lab]
        print(f"{tag} serial pass: memsets in front of the loss kernel {['%.1f us' % (1e3 * t) for t in memsets]}, unpack {1e3 * un:7.1f} us, "
              f"{len(other)} unlabelled launches behind the loss kernel {1e3 * sum(other):7.1f} us", flush=True)
m.set_grad_accumulation(False)
m.close()
