"""Cost of the parameter average on the C2 arena size, 22 015 244 elements, one segment [0, n) of class 0:
  (a) dmm_adam_step_segmented of the PARENT commit's library (built from its csrc; --parent-lib <its libdmmfods_hip.so>)
  (b) dmm_adam_step_segmented of this tree, average off
  (c) dmm_adam_step_segmented_ema: the average kept by the Adam launch
  (d) (b) followed by ema.lerp_(p, omd): the average as a second pass
HIP events around every call, 50 calls per variant and round after warm-up, ROUNDS rounds with the variants taking turns inside each
round (so that what else the machine does falls on all of them alike); per variant the median over all calls and the spread of the
round medians.  The two inequalities the feature stands on are printed with their verdicts.  Needs an MI355X:
    python tools/ema_cost.py --parent-lib <path> [--out profiles/r11/ema_cost.txt]"""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from dmmfods_amd import _lib  # noqa: E402

N = 22015244
ROUNDS, REPS, WARM = 6, 50, 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libdmmfods_hip.so built from the parent commit's csrc (without it (a) is left out)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    L = _lib.lib()
    dev = "cuda"
    gen = torch.Generator(device=dev).manual_seed(0)
    p = torch.randn(N, device=dev, generator=gen)
    gr = torch.randn(N, device=dev, generator=gen) * 1e-2
    m, v, e = torch.zeros(N, device=dev), torch.zeros(N, device=dev), p.clone()
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    seg = (_lib.AdamSegment * 1)(_lib.AdamSegment(0, N, 0))
    cls = (_lib.AdamClass * 1)(_lib.AdamClass(1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 0))
    omd = float(torch.tensor(1.0 - float(torch.tensor(0.999, dtype=torch.float32)), dtype=torch.float32))
    step = [0]

    def table_for(lib):
        t = torch.zeros((lib.dmm_adam_table_bytes(1, N) + 7) // 8, dtype=torch.int64, device=dev)
        assert lib.dmm_adam_table_init(t.data_ptr(), seg, 1, N, 1, st()) == 0
        return t

    def segmented(lib, table):
        def run():
            step[0] += 1
            rc = lib.dmm_adam_step_segmented(p.data_ptr(), gr.data_ptr(), m.data_ptr(), v.data_ptr(), N, table.data_ptr(), 1, cls, 1, step[0], 1.0, st())
            assert rc == 0, rc
        return run

    table = table_for(L)
    this_off = segmented(L, table)

    def fused():
        step[0] += 1
        ema = _lib.AdamEma(e.data_ptr(), 0.999, 0, step[0])
        _lib.check(L.dmm_adam_step_segmented_ema(p.data_ptr(), gr.data_ptr(), m.data_ptr(), v.data_ptr(), N, table.data_ptr(), 1, cls, 1, step[0], 1.0, st(),
                                                 C.byref(ema)))

    def two_pass():
        this_off()
        e.lerp_(p, omd)

    variants = [("(b) this tree, average off", this_off), ("(c) _ema: average in the Adam launch", fused), ("(d) (b) + ema.lerp_(p, omd)", two_pass)]
    if args.parent_lib:
        P = C.CDLL(os.path.abspath(args.parent_lib))
        P.dmm_adam_table_bytes.argtypes, P.dmm_adam_table_bytes.restype = L.dmm_adam_table_bytes.argtypes, C.c_size_t
        P.dmm_adam_table_init.argtypes = L.dmm_adam_table_init.argtypes
        P.dmm_adam_step_segmented.argtypes = L.dmm_adam_step_segmented.argtypes
        assert not hasattr(P, "dmm_adam_step_segmented_ema"), "--parent-lib is not the parent's library: it has the _ema entry points"
        variants.insert(0, ("(a) parent commit, dmm_adam_step_segmented", segmented(P, table_for(P))))

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
    assert bool(torch.isfinite(p).all()) and bool(torch.isfinite(e).all())
    lines = [f"{torch.cuda.get_device_name(0)}; n = {N} fp32 elements, one segment, HIP events around each call, microseconds",
             f"{ROUNDS} rounds x {REPS} calls per variant (after {WARM} warm-up calls), the variants taking turns inside a round",
             "variant                                      median   round medians min .. max (spread)   GB/s at the variant's B/elem"]
    med, spread = {}, {}
    for name, _ in variants:
        med[name], lo, hi = statistics.median(calls[name]), min(rounds[name]), max(rounds[name])
        spread[name] = hi - lo
        bpe = 28 if name[1] in "ab" else (36 if name[1] == "c" else 40)
        lines.append(f"{name:44s} {med[name]:7.1f}   {lo:7.1f} .. {hi:7.1f} ({hi - lo:5.1f})          {bpe * N / med[name] / 1e3:6.0f} ({bpe} B)")
    names = [n for n, _ in variants]
    b, c, d = names[-3:]
    if args.parent_lib:
        a = names[0]
        ok = med[b] - med[a] <= spread[a]   # (one-sided: the default path must not have become slower)
        lines.append(f"(b) no slower than (a) by more than (a)'s own spread:  {med[b]:.2f} - {med[a]:.2f} = {med[b] - med[a]:+.2f} <= {spread[a]:.2f}  ->  {'holds' if ok else 'DOES NOT HOLD'}")
    ok = med[c] < med[d]
    lines.append(f"(c) beats (d):  {med[c]:.1f} < {med[d]:.1f} (saves {med[d] - med[c]:.1f} us a step; the average costs {med[c] - med[b]:.1f} us over (b))  ->  {'holds' if ok else 'DOES NOT HOLD'}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
