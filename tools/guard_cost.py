"""Cost of the guarded optimiser step on the C2 arena size, 22 015 244 elements: the plain dmm_adam_step, dmm_adam_step_guarded and
the arena reduction alone (GB/s), HIP events, median of 50 repetitions after warm-up, two rounds.  Needs an MI355X:  python tools/guard_cost.py"""
import ctypes as C
import statistics
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from dmmfods_amd import _lib

L = _lib.lib()
n = 22015244
dev = "cuda"
g = torch.Generator(device=dev).manual_seed(0)
p = torch.randn(n, device=dev, generator=g); gr = torch.randn(n, device=dev, generator=g) * 1e-2
m = torch.zeros(n, device=dev); v = torch.zeros(n, device=dev)
block = torch.zeros(16, dtype=torch.int32, device=dev)
scratch = torch.zeros(L.dmm_grad_guard_scratch_bytes(n) // 8, dtype=torch.float64, device=dev)
st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
_lib.check(L.dmm_guard_state_init(block.data_ptr(), 1.0, 0, 0, st()))
step = [0]
def plain():
    step[0] += 1
    _lib.check(L.dmm_adam_step(p.data_ptr(), gr.data_ptr(), m.data_ptr(), v.data_ptr(), n, 1e-3, 0.9, 0.999, 1e-8, 0.0, step[0], 1.0, st()))
def guarded():
    _lib.check(L.dmm_adam_step_guarded(p.data_ptr(), gr.data_ptr(), m.data_ptr(), v.data_ptr(), n, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 2.0, 0.5, 2000,
                                       block.data_ptr(), scratch.data_ptr(), st()))
def reduce_only():
    _lib.check(L.dmm_grad_sumsq(gr.data_ptr(), 0, n, 0, scratch.data_ptr(), st()))
def measure(fn, reps=50, warm=10):
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts), min(ts), max(ts)
for rnd in range(2):
    for name, fn in (("plain dmm_adam_step", plain), ("dmm_adam_step_guarded", guarded), ("grad_sumsq alone", reduce_only)):
        med, lo, hi = measure(fn)
        extra = f"  {4 * n / med / 1e3:.0f} GB/s" if fn is reduce_only else f"  {28 * n / med / 1e3:.0f} GB/s of Adam's 28 B/elem"
        print(f"round {rnd} {name:24s} median {med:7.1f} us  min {lo:7.1f}  max {hi:7.1f}{extra}", flush=True)
s = _lib.GuardState.from_buffer_copy(block.cpu().numpy().tobytes())
print("state:", s.scale, s.applied_steps, s.skipped_steps, s.found_inf, s.grad_norm, s.clip_coef)
