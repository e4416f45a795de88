"""Cost of the optimiser step under parameter groups on the arena of C2 (d121 early fusion, 22 M parameters), one
MI355X, one process, the three cases alternating, HIP events around each, medians of --steps:
  (a) dmm_adam_step over the whole arena: the single-group launch;
  (b) dmm_adam_step_segmented under the table of fine_tune_groups(no_decay_norm_bias=True): one launch;
  (c) the same grouping as one dmm_adam_step per segment: what a launch per contiguous range costs.
Also (b) for fine_tune_groups(encoder_lr_scale=0.1, no_decay_norm_bias=True) with decoupled decay, and the guarded forms.
Needs an MI355X:  python tools/groups_cost.py [--steps 30]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from dmmfods_amd import _lib  # noqa: E402
from dmmfods_amd.optim import FusedAdam, fine_tune_groups  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--config", default="c2", choices=sorted(bench.CONFIGS))
args = ap.parse_args()
L = _lib.lib()
dev = torch.device("cuda:0")
w = bench.Workload(bench.CONFIGS[args.config], dev, 0, False, False)
m = w.model
n = m.param_arena.numel()
m.grad_arena.copy_(torch.randn(n, device=dev) * 0.01)
st = _lib.stream_ptr


cases = {"single": FusedAdam(m, weight_decay=0.01),
         "grouped": FusedAdam(m, param_groups=fine_tune_groups(m, 1e-3, 0.01, no_decay_norm_bias=True)),
         "grouped4-adamw": FusedAdam(m, param_groups=fine_tune_groups(m, 1e-3, 0.01, encoder_lr_scale=0.1, no_decay_norm_bias=True), decoupled_weight_decay=True),
         "single-guarded": FusedAdam(m, weight_decay=0.01, max_grad_norm=1e9),
         "grouped-guarded": FusedAdam(m, param_groups=fine_tune_groups(m, 1e-3, 0.01, no_decay_norm_bias=True), max_grad_norm=1e9)}
segs = cases["grouped"].segments()
per_segment_opt = cases["single"]


def per_segment():
    """(c): one single-range launch per segment of the grouped table, on offset pointers."""
    p, g, e1, e2 = m.param_arena.data_ptr(), m.grad_arena.data_ptr(), per_segment_opt.exp_avg.data_ptr(), per_segment_opt.exp_avg_sq.data_ptr()
    s = st()
    for b, c, gi, _ in segs:
        L.dmm_adam_step(p + 4 * b, g + 4 * b, e1 + 4 * b, e2 + 4 * b, c, 1e-3, 0.9, 0.999, 1e-8, 0.0 if gi else 0.01, 5, 1.0, s)


runs = {k: v.step for k, v in cases.items()}
runs["per-segment"] = per_segment
print(f"{w.c['name']}: arena of {n} elements; table of fine_tune_groups(no_decay_norm_bias=True): {len(segs)} segments, "
      f"{len(cases['grouped']._classes)} classes; with encoder_lr_scale: {len(cases['grouped4-adamw'].segments())} segments, "
      f"{len(cases['grouped4-adamw']._classes)} classes", flush=True)
for f in runs.values():
    for _ in range(3):
        f()
torch.cuda.synchronize()
times = {k: [] for k in runs}
for _ in range(args.steps):
    for k, f in runs.items():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        f()
        b.record()
        times[k].append((a, b))
torch.cuda.synchronize()
med = {}
for k, ev in times.items():
    ts = [a.elapsed_time(b) for a, b in ev]
    med[k] = statistics.median(ts)
    print(f"{k:16s} median {med[k] * 1e3:8.1f} us  min {min(ts) * 1e3:8.1f}  max {max(ts) * 1e3:8.1f}", flush=True)
print(f"(b) / (a) = {med['grouped'] / med['single']:.3f}   (c) / (b) = {med['per-segment'] / med['grouped']:.2f}   "
      f"guarded: grouped / single = {med['grouped-guarded'] / med['single-guarded']:.3f}", flush=True)
assert bool(torch.isfinite(m.param_arena).all())
m.close()
