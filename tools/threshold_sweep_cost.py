"""Cost of the validation threshold sweep at C2's validation shape, 4 x 3 x 1280 x 1920 fp32 logits and targets
(118 MB each, 236 MB read per call):
  (a) dmm_plan_loss_metrics alone - the launch validation already makes; it reads the same 236 MB and is the yardstick
  (b) dmm_logit_hist
  (c) the torch composite on the device: bucketize + bincount per class and truth value
  (d) (b) with another number of aggregation rounds in front of its per-lane LDS atomics ((b) as it ships takes one): 0 = plain per-lane
      adds, 4 = four rounds.  --lab-lib <rounds>=<a libdmmfods_hip.so whose lhist.hip was built with -DDMM_LAB=1, tools/build_variant.sh>,
      once per form and each a file of its own (a library reads DMM_HIST_ROUNDS once); without it (d) is left out
for K = 19 and K = 255 thresholds and two inputs: realistic logits (at least 90 % below every threshold) and logits uniform over the bins.
HIP events around every call, 50 calls per variant and round after warm-up, ROUNDS rounds with the variants taking turns inside each
round (so that what else the machine does falls on all of them alike); per variant the median over all calls and the spread of the
round medians.  Needs an MI355X:
    python tools/threshold_sweep_cost.py [--lab-lib <path>] [--out profiles/r12/threshold_sweep_cost.txt]"""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from dmmfods_amd import _lib  # noqa: E402
from dmmfods_amd.graphs.models.Dense_U_Net_lidar import Dense_U_Net_lidar  # noqa: E402
from dmmfods_amd.metrics import logit_thresholds  # noqa: E402
from dmmfods_amd.utils.Dense_U_Net_lidar_helper import get_config  # noqa: E402

B, NC, H, W = 4, 3, 1280, 1920
GT = 0.7
ROUNDS, REPS, WARM = 6, 50, 10
BYTES = 2 * B * NC * H * W * 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lab-lib", action="append", default=[], help="<rounds>=<path>: a lab build of the library (DMM_LAB=1) for variant (d)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    L = _lib.lib()
    dev = "cuda"
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    gen = torch.Generator(device=dev).manual_seed(0)
    target = (torch.rand((B, NC, H, W), device=dev, generator=gen) ** 8).contiguous()          # 4 % of the pixels at or above 0.7

    # (a): the tiny net's plan at this shape - the loss kernel does not depend on the net
    cfg = get_config("/tmp/dmm_sweep_cost")
    cfg.model.growth_rate, cfg.model.block_config, cfg.model.num_init_features = 8, (2, 2, 2, 2), 16
    cfg.model.concat_before_block_num, cfg.model.stream_2_in_channels = 3, 3
    model = Dense_U_Net_lidar(cfg, compute_dtype="fp16").to(dev).eval()
    plan = model._get_plan(B, H, W)
    model._apply_loss(plan)

    labs = []
    for spec in args.lab_lib:
        r, path = spec.split("=", 1)
        assert r in ("0", "4"), "variant (d): 0 or 4 rounds"
        lab = C.CDLL(os.path.abspath(path))
        lab.dmm_logit_hist.argtypes = L.dmm_logit_hist.argtypes
        os.environ["DMM_HIST_ROUNDS"] = r   # read once, at the library's first launch (below, before anything is timed)
        probe = torch.zeros(8, dtype=torch.int64, device=dev)
        one = torch.zeros(4, device=dev)
        assert lab.dmm_logit_hist(one.data_ptr(), one.data_ptr(), 1, 1, 2, 2, (C.c_float * 1)(0.5), 1, GT, 0, probe.data_ptr(), st()) == 0
        labs.append((r, lab))
    os.environ.pop("DMM_HIST_ROUNDS", None)

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

    lines = [f"{torch.cuda.get_device_name(0)}; logits and target {B} x {NC} x {H} x {W} fp32 ({BYTES / 1e6:.0f} MB read per call), HIP events around each call, microseconds",
             f"{ROUNDS} rounds x {REPS} calls per variant (after {WARM} warm-up calls), the variants taking turns inside a round"]
    for K in (19, 255):
        thr = logit_thresholds([(k + 1) / (K + 1) for k in range(K)])
        thr_c = (C.c_float * K)(*thr.tolist())
        thr_t = torch.from_numpy(thr).to(dev)
        for kind in ("realistic", "uniform"):
            if kind == "realistic":   # far-negative logits, a few near and above the cuts: more than 90 % lie below every threshold
                logits = (torch.randn((B, NC, H, W), device=dev, generator=gen) * 1.5 - 9.0)
                logits = torch.where(torch.rand((B, NC, H, W), device=dev, generator=gen) < 0.05, logits + 9.0, logits).contiguous()
            else:                     # every bin equally likely
                u = torch.rand((B, NC, H, W), device=dev, generator=gen) * (K + 1)
                edges = torch.cat([thr_t[:1] - 1.0, thr_t, thr_t[-1:] + 1.0])
                i = u.long().clamp_(0, K)
                logits = (edges[i] + (u - i) * (edges[i + 1] - edges[i]) * 0.999).contiguous()
            below = float((logits < thr_t[0]).float().mean())
            counts = torch.empty((B, NC, 2, K + 1), dtype=torch.int64, device=dev)

            def loss_metrics():
                _lib.check(L.dmm_plan_loss_metrics(plan.handle, logits.data_ptr(), target.data_ptr(), plan.metrics.data_ptr(), st()))

            def hist(lib=L, out=counts):
                rc = lib.dmm_logit_hist(logits.data_ptr(), target.data_ptr(), B, NC, H, W, thr_c, K, GT, 0, out.data_ptr(), st())
                assert rc == 0, rc

            def composite():
                # bucketize(right=True) counts the thresholds <= x (a NaN logit would land in the LAST bin here, not the first)
                g = target >= GT
                out = []
                for n in range(NC):
                    bins = torch.bucketize(logits[:, n], thr_t, right=True)
                    key = (torch.arange(B, device=dev).view(B, 1, 1) * 2 + g[:, n]) * (K + 1) + bins
                    out.append(torch.bincount(key.flatten(), minlength=B * 2 * (K + 1)).view(B, 2, K + 1))
                return torch.stack(out, dim=1)

            hist()
            assert torch.equal(counts, composite()), "the kernel and the torch composite disagree"
            variants = [("(a) dmm_plan_loss_metrics alone", loss_metrics), ("(b) dmm_logit_hist", hist), ("(c) torch bucketize + bincount", composite)]
            for r, lab in labs:
                out_d = torch.empty_like(counts)
                hist(lab, out_d)
                assert torch.equal(counts, out_d), "two builds of the kernel disagree"
                variants.append((f"(d) (b) with {r} rounds" + (": plain LDS adds" if r == "0" else ""), lambda lab=lab, out_d=out_d: hist(lab, out_d)))
            calls = {name: [] for name, _ in variants}
            rounds = {name: [] for name, _ in variants}
            for _ in range(ROUNDS):
                for name, fn in variants:
                    ts = measure(fn)
                    calls[name] += ts
                    rounds[name].append(statistics.median(ts))
            lines.append("")
            lines.append(f"K = {K}, {kind} logits ({100 * below:.1f} % below every threshold)")
            lines.append("variant                                   median   round medians min .. max (spread)   GB/s of the 236 MB")
            med, spread = {}, {}
            for name, _ in variants:
                med[name], lo, hi = statistics.median(calls[name]), min(rounds[name]), max(rounds[name])
                spread[name] = hi - lo
                rate = f"{BYTES / med[name] / 1e3:6.0f}" if name[1] != "c" else "     -"
                lines.append(f"{name:40s} {med[name]:8.1f}   {lo:8.1f} .. {hi:8.1f} ({hi - lo:6.1f})          {rate}")
            a, b, c = (n for n, _ in variants[:3])
            lines.append(f"(b) beats (c):  {med[b]:.1f} < {med[c]:.1f}  ->  {'holds' if med[b] < med[c] else 'DOES NOT HOLD'} ({med[c] / med[b]:.1f}x)")
            lines.append(f"(b) over (a), the pure read with the loss arithmetic:  {med[b]:.1f} - {med[a]:.1f} = {med[b] - med[a]:+.1f} us ((a)'s own spread {spread[a]:.1f})")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    model.close()


if __name__ == "__main__":
    main()
