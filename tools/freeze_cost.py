"""Cost of a training step with the encoder frozen at C2 (d121 early fusion, batch 4, 1280 x 1920, fp16 storage),
default against frozen in ONE process on one MI355X, alternating, two rounds (each change of mode closes the plan and builds it
again in the other mode: a few steps of warm-up follow):
  * the step (forward + loss_backward + Adam), HIP events around each step, median of --steps;
  * the backward alone (loss_backward behind a forward that is not timed: events around the call);
  * the number of launch records of the backward list and of optimiser launches per step.
Needs an MI355X:  python tools/freeze_cost.py [--steps 30]"""
import argparse
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


def full():
    with torch.no_grad():
        m(w.rgb, w.lidar)
    m.loss_backward(w.tgt)
    opt.step()


def timed_steps(n):
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
    torch.cuda.synchronize()
    marks[0].record()
    for i in range(n):
        full()
        marks[i + 1].record()
    torch.cuda.synchronize()
    ts = [marks[i].elapsed_time(marks[i + 1]) for i in range(n)]
    return statistics.median(ts), min(ts), max(ts)


def timed_backward(n):
    pairs = []
    for _ in range(n):
        with torch.no_grad():
            m(w.rgb, w.lidar)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        m.loss_backward(w.tgt)
        b.record()
        opt.step()
        pairs.append((a, b))
    torch.cuda.synchronize()
    ts = [a.elapsed_time(b) for a, b in pairs]
    return statistics.median(ts), min(ts), max(ts)


for _ in range(10):
    full()
print(f"{w.c['name']}: {m.num_params} parameters", flush=True)
for rnd in range(2):
    for frozen in (False, True):
        m.freeze_encoder(frozen)
        for _ in range(5):
            full()
        tag = f"round {rnd} {'frozen ' if frozen else 'default'}"
        plan = m._last[0]
        nb = L.dmm_plan_profile_num_ops(plan.handle, 1)
        ranges = opt.trainable_ranges()
        trainable = sum(r[1] for r in ranges)
        print(f"{tag} backward list {nb} launch records, {len(m.grad_buckets())} gradient buckets, optimiser over {len(ranges)} range(s), "
              f"{trainable} of {m.num_params} parameters trainable, workspace {plan.workspace.numel() / 2 ** 30:.2f} GiB", flush=True)
        med, lo, hi = timed_steps(args.steps)
        print(f"{tag} step     median {med:7.3f} ms  min {lo:7.3f}  max {hi:7.3f}", flush=True)
        med, lo, hi = timed_backward(args.steps)
        print(f"{tag} backward median {med:7.3f} ms  min {lo:7.3f}  max {hi:7.3f}", flush=True)
m.freeze_encoder(False)
m.close()
