"""Exact operands for the convolution kernels: inputs on which every product and every partial sum is a small dyadic number, so
that fp32 accumulation is exact in ANY order and rounding to f16 / bf16 is the identity.  A kernel then has to equal an fp64
reference bit for bit - outputs, BatchNorm statistics, data gradients, both BatchNorm-backward sums and weight gradients - and a
dropped row, a duplicated tile, a wrong tap or a padded lane that leaks is a nonzero difference, not 2e-4 of a tolerance.

Needs torch on the CPU only (tools/gpu_lab.py launches on these operands; tests/test_exact_operands_cpu.py checks the conditions
below for every case the GPU tests run, so that those can neither pass vacuously nor fail because of their own inputs).

Recipe: x integers in [-3, 3]; scale, invstd in {0.5, 1, 2}; shift in {-1, 0, 1}; mean integers in [-2, 2]; dy integers in [-2, 2];
yfwd even integers in [-4, 4]; q in {-1, 0, 1}; r in {-1, -0.5, 0, 0.5, 1}; gold integers in [-2, 2]; weights in {-1, 0, +1}.
(The data gradient of the nearest-x2 upsampled 3x3 adds 4 x 9 taps per output channel into one element: with scale = 2 no weight
tensor that covers every tap fits bf16's 8 bits.  Those cases draw scale from {0.5, 1} and dy from [-1, 1]: `narrow`.)

Conditions, asserted by Operands.check() on the reference alone:
 (a) every tensor a kernel stores in the storage type is representable there: the activation after the prologue, the output, the
     stored data gradient dz * scale (+ gold), the effective gradient dy + q + r * yfwd;
 (b) outputs, data gradients and weight gradients are exact in fp32 for any summation order: sum |term| / u < 2**24 per element, u
     the common power-of-two step of the terms (the same convolution over the operands' absolute values);
 (c) per-channel sums (stat_sum, stat_sq, red1, red2): chain * max |term| / u < 2**24, chain = the longest fp32 partial of a kernel
     before it reaches fp64 (at most one 128-row tile; the generic kernel's pooled data gradient: 4 pixels per row, 512);
 (d) at least 90 % of the output elements are nonzero;
 and the weights: entries in {-1, 0, 1}, every (tap, input channel) pair nonzero in some output channel, every output channel
 nonzero somewhere.

The weights are as dense as (a) allows BY CONSTRUCTION (worst-case bounds from the per-channel maxima of the other operand, not
luck): per output channel the |activation| maxima of its nonzero weights add up to at most the largest representable output, per
input channel the |gradient| maxima likewise for the stored data gradient.  bf16 holds 8 significant bits, f16 11 - f16 weights for
the data gradient are 8 times as dense; for the forward they are 4 times as dense, because (c) for stat_sq (128 y**2 / u**2 < 2**24)
caps |y| / u near 2**8.5 whatever the storage type (the budget of 2**10 relies on signs cancelling; check() holds the actual values
to (c)).

Below them, the single-rounding operands (make_rounding_operands, Operands.check_rounding): the same exactness in fp32, but every
16-bit store rounds once - see the comment there.  At the end, the logits launch (part "logits" of both generators): an fp32 output
without statistics, and the padding condition (p) - see the comment there."""
import functools
from types import SimpleNamespace

import torch
import torch.nn.functional as F

DT = {0: torch.float32, 1: torch.float16, 2: torch.bfloat16}
SIG_BITS = {0: 24, 1: 11, 2: 8}        # significant bits of the storage type
FWD_BITS = {0: 10, 1: 10, 2: 8}        # budget of |y| / u (see the module docstring on stat_sq)
LOGITS_BITS = 20                       # ... of a logits launch, which stores fp32: sum |term| / u stays 16 times below (b)'s 2**24
DENSITY_CAP = 0.75                     # keep a quarter of the weights zero wherever the budgets would allow all of them


def _pick(g, values, shape):
    v = torch.tensor(values, dtype=torch.float64)
    return v[torch.randint(0, len(values), shape, generator=g)]


def conv(a, w, c):
    """The case's convolution on NCHW operands (any floating type)."""
    if c.transposed:
        return F.conv_transpose2d(a, w, stride=2, padding=1, output_padding=1)
    if c.mode == 1:
        return F.conv2d(F.interpolate(a, scale_factor=2, mode="nearest"), w, padding=c.pad)
    if c.mode == 2:
        return F.avg_pool2d(F.conv2d(a, w), 2, 2)
    return F.conv2d(a, w, stride=c.stride, padding=c.pad)


def out_hw(c):
    if c.transposed or c.mode == 1:
        return 2 * c.H, 2 * c.W
    if c.mode == 2:
        return c.H // 2, c.W // 2
    return (c.H + 2 * c.pad - c.R) // c.stride + 1, (c.W + 2 * c.pad - c.S) // c.stride + 1


def _tap_groups(c):
    """Sets of taps that can meet in one output element.  ConvTranspose (3x3, stride 2): the output parities see 1, 2, 2 and 4 taps."""
    T = c.R * c.S
    if not c.transposed:
        return [list(range(T))]
    cls = {}
    for ky in range(3):
        for kx in range(3):
            cls.setdefault((ky == 1, kx == 1), []).append(ky * 3 + kx)
    return list(cls.values())


def _prefix_within(key, wts, budget):
    """Per row: the slots, in ascending order of `key`, whose running sum of `wts` stays within `budget` (a tensor per row)."""
    order = torch.argsort(key, dim=1)
    cs = torch.cumsum(torch.gather(wts, 1, order), dim=1)
    keep = torch.zeros_like(key, dtype=torch.bool)
    keep.scatter_(1, order, cs <= budget.view(-1, 1))
    return keep


def build_weights(g, c, amax, effmax, scale, ylim, glim):
    """{-1, 0, 1} weights [Cout][Cin][T], as dense as the budgets allow: per output channel and tap group sum amax[cin] |w| <= ylim,
    per input channel gain * scale[cin] * sum effmax[cout] |w| <= glim (None: no such bound).  The slots that cover every (tap, input
    channel) pair and every output channel come first in every order, so they are the last to go."""
    Cout, Cin, T = c.Cout, c.Cin, c.R * c.S
    key = torch.rand(Cout, Cin, T, generator=g, dtype=torch.float64)
    sel = key < DENSITY_CAP
    ci, tt = torch.meshgrid(torch.arange(Cin), torch.arange(T), indexing="ij")
    must = torch.zeros(Cout, Cin, T, dtype=torch.bool)
    must[(ci * T + tt) % Cout, ci, tt] = True
    co = torch.arange(Cout)
    must[co, co % Cin, (co // Cin) % T] |= ~must.view(Cout, -1).any(dim=1)
    key = key - must.double()
    sel |= must
    if ylim is not None:
        for grp in _tap_groups(c):
            k = key[:, :, grp].reshape(Cout, -1)
            s = sel[:, :, grp].reshape(Cout, -1)
            wts = amax.view(1, Cin, 1).expand(Cout, Cin, len(grp)).reshape(Cout, -1) * s
            sel[:, :, grp] = (s & _prefix_within(k, wts, torch.full((Cout,), float(ylim), dtype=torch.float64))).view(Cout, Cin, len(grp))
    if glim is not None:
        k = key.permute(1, 0, 2).reshape(Cin, -1)
        s = sel.permute(1, 0, 2).reshape(Cin, -1)
        wts = effmax.view(1, Cout, 1).expand(Cin, Cout, T).reshape(Cin, -1) * s
        keep = s & _prefix_within(k, wts, glim / scale)
        sel = keep.view(Cin, Cout, T).permute(1, 0, 2).contiguous()
    sign = _pick(g, [-1.0, 1.0], (Cout, Cin, T))
    return sign * sel


class Operands(SimpleNamespace):
    def check(self):
        """Conditions (a)-(d) and the weight coverage, on the reference alone.  Returns the measured figures."""
        o, c = self, self.case
        dt, lim = DT[c.dtype], float(2 ** 24)
        fig = {}

        def rep(name, t):
            assert torch.equal(t.to(dt).double(), t), f"(a) {name} is not representable in {dt}: max |t| = {float(t.abs().max())}"
        rep("activation", o.a)
        rep("effective gradient", o.eff)
        w3 = o.wslots
        assert bool(((w3 == 0) | (w3.abs() == 1)).all()), "weights outside {-1, 0, 1}"
        assert bool((w3 != 0).any(dim=0).all()), "a (tap, input channel) pair is zero in every output channel"
        assert bool((w3 != 0).view(c.Cout, -1).any(dim=1).all()), "an output channel has no nonzero weight"
        fig["density"] = float((w3 != 0).double().mean())
        fig["nonzero_y"] = float((o.y != 0).double().mean())
        assert fig["nonzero_y"] >= 0.9, f"(d) only {fig['nonzero_y']:.3f} of the outputs are nonzero"
        aa = o.a.abs().requires_grad_(True)
        wa = o.w.abs().requires_grad_(True)
        ya = conv(aa, wa, c)
        if "logits" in o.parts:     # the logits launch stores fp32 and keeps no statistics: (a) in fp32, (b), and the padding
            assert torch.equal(o.y.float().double(), o.y), f"(a) logits are not representable in fp32: max |y| = {float(o.y.abs().max())}"
            fig["b_y"] = float(ya.detach().max()) / o.uy
            # a kernel that pads BEFORE the prologue (relu(shift) in place of zero) must differ from the reference on every image's border
            assert c.bn and bool((F.relu(o.shift) > 0).any()), "(p) no channel has relu(shift) > 0: padding before and after the prologue agree"
            d = o.y != o.y_padnorm
            inner = d[:, :, c.pad:o.Ho - c.pad, c.pad:o.Wo - c.pad]
            assert not bool(inner.any()), "(p) the two references differ away from the border"
            fig["pad_diff"] = float(d.double().mean())
            assert bool(d.flatten(1).any(dim=1).all()), "(p) an image's border does not tell padding before the prologue from padding after it"
        if "fwd" in o.parts:
            rep("output", o.y)
            fig["b_y"] = float(ya.detach().max()) / o.uy
            fig["c_sum"] = o.chain * float(o.y.abs().max()) / o.uy
            fig["c_sq"] = o.chain * float(o.y.abs().max()) ** 2 / o.uy ** 2
        if o.backward:
            (ya * o.eff.abs()).sum().backward()
            if "wgrad" in o.parts:
                fig["b_dw"] = float(wa.grad.max()) / (o.ua * o.udz)
            if "dgrad" in o.parts:
                rep("stored data gradient", o.gx)
                fig["b_dz"] = float(aa.grad.max()) / o.udz
                fig["c_red1"] = o.chain_red * float(o.dz.abs().max()) / o.udz
                fig["c_red2"] = o.chain_red * float((o.dz * o.xhat).abs().max()) / (o.udz * 0.5)
        for k, v in fig.items():
            if k[:2] in ("b_", "c_"):
                assert v < lim, f"({k[0]}) {k[2:]}: {v:.3g} >= 2**24"
        return fig


def make_operands(dtype, B, H, W, Cin, Cout, R, S, stride, pad, transposed=0, mode=0, bn=1, with_q=0, acc=0,
                  parts=("fwd", "wgrad", "dgrad"), seed=0, chain=128, chain_red=128, fwd_bits=None):
    """Operands and fp64 reference of one case.  parts: what the caller will launch and compare - "fwd" (output and statistics), "wgrad",
    "dgrad" (stored data gradient, red1, red2), or "logits" alone (dmm_conv_logits: the output as fp32, no statistics); the weights are bounded only by what is stored.  chain / chain_red: the fp32 chain of
    condition (c) for the forward statistics / the BatchNorm-backward sums; fwd_bits: log2 of the budget of |y| / u (default: FWD_BITS).
    NCHW fp64 tensors on the CPU."""
    c = SimpleNamespace(dtype=dtype, B=B, H=H, W=W, Cin=Cin, Cout=Cout, R=3 if transposed else R, S=3 if transposed else S,
                        stride=stride, pad=pad, transposed=transposed, mode=mode, bn=bn)
    parts = tuple(parts)
    if not bn or (mode == 0 and not transposed and stride != 1):
        parts = tuple(p for p in parts if p != "dgrad")     # as conv_case: no BN-fused data gradient for these
    g = torch.Generator().manual_seed(seed)
    narrow = mode == 1 and "dgrad" in parts
    x = torch.randint(-3, 4, (B, Cin, H, W), generator=g).double()
    scale = _pick(g, [0.5, 1.0] if narrow else [0.5, 1.0, 2.0], (Cin,))
    shift = _pick(g, [-1.0, 0.0, 1.0], (Cin,))
    mean = torch.randint(-2, 3, (Cin,), generator=g).double()
    invstd = _pick(g, [0.5, 1.0, 2.0], (Cin,))
    v = lambda t: t.view(1, -1, 1, 1)  # noqa: E731
    z = x * v(scale) + v(shift)
    a = F.relu(z) if bn else x.clone()
    Ho, Wo = out_hw(c)
    dyr = 1 if narrow else 2
    dy = torch.randint(-dyr, dyr + 1, (B, Cout, Ho, Wo), generator=g).double()
    yf = q = r = None
    eff = dy
    if with_q:
        yf = 2.0 * torch.randint(-2, 3, (B, Cout, Ho, Wo), generator=g).double()
        q = _pick(g, [-1.0, 0.0, 1.0], (Cout,))
        r = _pick(g, [-1.0, -0.5, 0.0, 0.5, 1.0], (Cout,))
        eff = dy + v(q) + v(r) * yf
    gold = torch.randint(-2, 3, (B, Cin, H, W), generator=g).double() if acc else None
    # steps of the stored values, and what the storage type holds of them
    pool = 0.25 if mode == 2 else 1.0
    ua = 0.5 if bn else 1.0
    uy, udz = ua * pool, pool
    ylim = uy * 2 ** (fwd_bits or min(SIG_BITS[dtype], FWD_BITS[dtype])) if "fwd" in parts else None
    if "logits" in parts:   # stored in fp32 whatever the storage type: the budget is (b)'s, with room to spare
        assert "fwd" not in parts and mode == 0 and not transposed and stride == 1
        ylim = uy * 2 ** (fwd_bits or LOGITS_BITS)
    glim = None
    if "dgrad" in parts:   # |gx| <= gain * scale * sum effmax |w| + |gold|, in steps of udz / 2
        gain = 4.0 if mode == 1 else pool
        glim = (0.5 * udz * 2 ** min(SIG_BITS[dtype], 11) - (2.0 if acc else 0.0)) / gain
    amax = a.abs().amax(dim=(0, 2, 3))
    effmax = eff.abs().amax(dim=(0, 2, 3))
    wslots = build_weights(g, c, amax, effmax, scale, ylim, glim)      # [Cout][Cin][T]
    w = wslots.view(Cout, Cin, c.R, c.S)
    if transposed:
        w = w.permute(1, 0, 2, 3).contiguous()
    o = Operands(case=c, parts=parts, with_q=with_q, acc=acc, chain=chain, chain_red=chain_red, x=x, scale=scale, shift=shift, mean=mean, invstd=invstd, z=z,
                 dy=dy, yf=yf, q=q, r=r, eff=eff, gold=gold, w=w, wslots=wslots, ua=ua, uy=uy, udz=udz, Ho=Ho, Wo=Wo,
                 backward="wgrad" in parts or "dgrad" in parts)
    o.xhat = (x - v(mean)) * v(invstd)
    ar = a.clone().requires_grad_(o.backward)
    wr = w.clone().requires_grad_(o.backward)
    y = conv(ar, wr, c)
    o.a, o.y = a, y.detach()
    o.stat_sum, o.stat_sq = o.y.sum(dim=(0, 2, 3)), (o.y ** 2).sum(dim=(0, 2, 3))
    if "logits" in parts and bn:   # what a kernel computes that normalises its padding: the prologue over the zero-padded input
        o.y_padnorm = F.conv2d(F.relu(F.pad(x, (pad,) * 4) * v(scale) + v(shift)), w)
    if o.backward:
        (y * eff).sum().backward()
        o.dw = wr.grad
        o.dz = ar.grad * (z > 0) if bn else ar.grad
        o.gx = o.dz * v(scale) + (gold if acc else 0.0)
        o.red1, o.red2 = o.dz.sum(dim=(0, 2, 3)), (o.dz * o.xhat).sum(dim=(0, 2, 3))
    return o


@functools.lru_cache(maxsize=2)
def cached_operands(*args, **kw):
    """make_operands, remembered for the last two cases (the GPU tests and the CPU test share a reference per case)."""
    return make_operands(*args, **kw)


# ------------------------------------------------------------------------------------------------ the cases of tests/test_exact_kernels_gpu.py
# (shared with tests/test_exact_operands_cpu.py, which checks the conditions for every one of them without a GPU)
# forward: family, (name, B, H, W, Cin, Cout, R, S, stride, pad, transposed, mode, bn) as CASES below, make_operands arguments per dtype
# (9 x 128 (tap, channel) pairs over 32 output channels: covering every pair takes 36 weights per output channel, whose |activation|
# maxima add up to ~150 - above the 128 that bf16 holds of |y| in steps of 0.5.  fwd_bits = 9 lets them in; the output is then
# representable on the actual values - 36 to 90 terms of random sign, |y| <= 100 - which check() asserts, not by the worst case.)
_B9 = {2: dict(fwd_bits=9)}
FORWARD = [
    ("pig", ("1x1 224->128 1x339x339", 1, 339, 339, 224, 128, 1, 1, 1, 0, 0, 0, 1), {}),
    ("pig", ("1x1 72->256 3x150x150", 3, 150, 150, 72, 256, 1, 1, 1, 0, 0, 0, 1), {}),
    ("pig", ("1x1 1288->128 2x130x130", 2, 130, 130, 1288, 128, 1, 1, 1, 0, 0, 0, 1), {}),
    ("conv3", ("3x3 128->32 3x170x330", 3, 170, 330, 128, 32, 3, 3, 1, 1, 0, 0, 1), _B9),
    ("conv3", ("7x7s2 8->64 1x530x1010", 1, 530, 1010, 8, 64, 7, 7, 2, 3, 0, 0, 0), {}),
    ("cf", ("3x3 128->32 1x328x816", 1, 328, 816, 128, 32, 3, 3, 1, 1, 0, 0, 1), _B9),
    ("cf", ("3x3 128->32 3x224x416", 3, 224, 416, 128, 32, 3, 3, 1, 1, 0, 0, 1), _B9),
    ("cvw", ("convT 128->128 3x85x125", 3, 85, 125, 128, 128, 3, 3, 2, 1, 1, 0, 1), {}),
    ("cvw", ("convT 256->256 3x61x93", 3, 61, 93, 256, 256, 3, 3, 2, 1, 1, 0, 1), {}),
    ("cvp", ("convT 384->256 1x11x19", 1, 11, 19, 384, 256, 3, 3, 2, 1, 1, 0, 1), {}),
    ("generic", ("pool2 1x1 128->64 2x12x20", 2, 12, 20, 128, 64, 1, 1, 1, 0, 0, 2, 1), {}),
]

# backward through backward_case: what, family, (B, H, W, Cin, Cout, R, S, pad, transposed, mode), the (with_q, acc) pairs
BACKWARD = [
    ("fused", "bw1", (1, 339, 339, 224, 128, 1, 1, 0, 0, 0), [(1, 1), (1, 0), (0, 1), (0, 0)]),
    ("fused", "bw1", (1, 16, 24, 160, 128, 1, 1, 0, 0, 0), [(1, 1), (1, 0), (0, 1), (0, 0)]),
    ("dgrad", "conv3", (2, 12, 20, 128, 32, 3, 3, 1, 0, 0), [(1, 0), (1, 1), (0, 0)]),
    ("dgrad", "conv3", (2, 7, 9, 128, 32, 3, 3, 1, 0, 0), [(1, 0), (1, 1), (0, 0)]),
    ("wgradT", "wg3", (2, 12, 20, 128, 32, 3, 3, 1, 0, 0), [(1, 0), (0, 0)]),
    ("wgradT", "wg3", (3, 5, 3, 128, 32, 3, 3, 1, 0, 0), [(1, 0), (0, 0)]),
    ("wgradT", "wg3", (1, 40, 60, 128, 32, 3, 3, 1, 0, 0), [(1, 0), (0, 0)]),
    ("wgrad", "wgp/wgpw", (2, 12, 20, 128, 64, 3, 3, 1, 1, 0), [(1, 0), (0, 0)]),      # with_q 1: wgp, 0: wgpw
    ("wgrad", "wgp/wgpw", (3, 5, 3, 128, 64, 3, 3, 1, 1, 0), [(1, 0), (0, 0)]),
    ("wgrad", "wgp/wgpw", (1, 9, 17, 256, 128, 3, 3, 1, 1, 0), [(1, 0), (0, 0)]),
    ("wgrad", "wgp/wgpw", (1, 24, 40, 256, 64, 3, 3, 1, 1, 0), [(1, 0), (0, 0)]),
    ("dgrad", "cvp", (1, 9, 17, 256, 256, 3, 3, 1, 1, 0), [(0, 0)]),                   # cvd3_kernel: the ConvTranspose's nine taps ...
    ("dgrad", "cvp", (1, 9, 7, 128, 64, 3, 3, 1, 0, 1), [(0, 0)]),                     # ... and the upsampled 3x3's sixteen merged taps
    ("dgrad", "cvp", (2, 12, 20, 128, 64, 3, 3, 1, 0, 1), [(0, 0)]),
    ("wgradT", "wg5", (1, 13, 21, 64, 3, 5, 5, 2, 0, 0), [(0, 0)]),
    ("wgrad", "wg5", (2, 24, 40, 8, 64, 3, 3, 1, 0, 0), [(1, 0)]),                     # the 3x3 over the normalised raw input
]
# ------------------------------------------------------------------------------------------------ the cases of tests/test_merged_phase_kernels_gpu.py
# A decoder ConvTranspose stage as a plan launches it: the four output-parity phases in ONE launch (dmm_conv_forward_merged,
# dmm_conv_wgrad_merged).  The shapes are the smallest at which each path of the merged kernels can still go wrong; the launcher
# arithmetic behind each "why" is recomputed by the test (merged_fwd_geometry / merged_wgrad_geometry below).
# forward: the form that must run ("cvw": cvw.hip's four-phase walk, "cvp": cvp_multi_kernel), case tuple as CASES, why
FORWARD_MERGED = [
    ("cvw", ("convT 128->128 2x7x9", 2, 7, 9, 128, 128, 3, 3, 2, 1, 1, 0, 1), "2 items per phase on 8 workgroups: `first` with done = 2, 4, 6, fewer items than workgroups"),
    ("cvw", FORWARD[7][1], "264 items per phase, 1056 on 256 workgroups: done % 256 = 8, 16, 24; ragged in both directions"),
    ("cvw", FORWARD[8][1], "288 items per phase, two channel groups, two column tiles: the statistics of the last column tile at every phase end"),
    ("cvp", FORWARD[9][1], "per = 8, per8 = 1"),
    ("cvp", ("convT 384->256 1x11x35", 1, 11, 35, 384, 256, 3, 3, 2, 1, 1, 0, 1), "per = 12, per8 = 2: workgroups with xcd * 2 + j >= 12 exit without a store"),
]
# weight gradient on wgpw_multi_kernel, the materialised gradient (with_q = 0): (B, H, W, Cin, Cout), why
BACKWARD_MERGED = [
    ((2, 12, 20, 128, 64), "8 units, none idle"),
    ((3, 5, 3, 128, 64), "3 units rounded to 8: 5 idle units in each of the 4 phases"),
    ((1, 37, 70, 256, 128), "25 tiles, 4 (ci, co) pairs: more than one tile per workgroup with a short last walk, units no multiple of 8"),
]
# kept apart - four launches, still exact: the forward with 64 input channels (cvp refuses: the generic kernel), the weight gradient
# under the deferred correction (mixed tap counts in one launch are wgpw.hip's, which takes the materialised gradient only)
FORWARD_APART = ("convT 64->64 2x6x10", 2, 6, 10, 64, 64, 3, 3, 2, 1, 1, 0, 1)
BACKWARD_APART = (2, 12, 20, 128, 64)
FORWARD_MERGED_REPRO, BACKWARD_MERGED_REPRO = 1, 2        # run twice, equal bit for bit: indices into FORWARD_MERGED / BACKWARD_MERGED
CW_TILE, CW_BN, WP_TILE, DESIGN_CUS = (8, 16), 128, (8, 16), 256


def merged_fwd_geometry(form, B, H, W, Cin, Cout):
    """cvw.hip cvw_resolve / cvp.hip cvp_resolve for a merged forward launch: items per phase, workgroups, and for cvw the first item
    of every workgroup in every phase (cvw_kernel), for cvp the workgroups that exit at once (cvp_multi_kernel)."""
    cd = lambda a, b: -(-a // b)  # noqa: E731
    per = B * cd(H, CW_TILE[0]) * cd(W, CW_TILE[1]) * (Cout // CW_BN)
    g = dict(groups=Cin // 128, ntn=Cout // CW_BN, per=per)
    if form == "cvw":
        nwg = min(DESIGN_CUS, 4 * per)
        g.update(nwg=nwg, done_mod=[(p * per) % nwg for p in range(4)],
                 first=[[(b - (p * per) % nwg + 2 * nwg) % nwg for b in range(nwg)] for p in range(4)])
    else:
        per8 = cd(per, 8)
        g.update(per8=per8, nwg=8 * per8 * 4, idle=sum(1 for b in range(8 * per8 * 4) if (b & 7) * per8 + (b >> 3) % per8 >= per))
    return g


def merged_wgrad_geometry(B, H, W, Cin, Cout, cus):
    """wgp.hip wgp_resolve / wgp_split for a merged weight-gradient launch (nphase = 4: 64 output channels per workgroup)."""
    cd = lambda a, b: -(-a // b)  # noqa: E731
    ntiles = B * cd(H, WP_TILE[0]) * cd(W, WP_TILE[1])
    pairs = (Cin // 128) * (Cout // 64)
    nsplit = min(max(1, cd(cus // 4, pairs)), ntiles)
    tiles_per_wg = cd(ntiles, nsplit)
    nsplit = cd(ntiles, tiles_per_wg)
    units = nsplit * pairs
    return dict(ntiles=ntiles, pairs=pairs, nsplit=nsplit, tiles_per_wg=tiles_per_wg, units=units, nwg=cd(units, 8) * 8 * 4)


STEM_WGRAD = ("7x7s2 8->64 2x32x48", 2, 32, 48, 8, 64, 7, 7, 2, 3, 0, 0, 0)          # wg5 through conv_case (no BatchNorm in front)
CONV5_STATS = (1, 13, 21)                                                             # conv5_stats_case: B, H, W

# the ragged and tail cases of tests/test_kernels_gpu.py (fp32, the generic kernel; beside tools/gpu_lab.py CASES)
EXACT_KW = {   # per case name: what make_operands needs beside the shape
    # 25 x 64 (tap, channel) pairs over 8 output channels: covering every pair takes 200 weights per output channel, more than the
    # default budget of |y| / u <= 2**10 holds; fp32 storage has the bits, and check() holds the actual values to (c)
    "5x5 64->8": dict(fwd_bits=11),
    # the generic kernel's pooled data gradient adds the 4 pixels of a pooling window per row of its 128-row tile in fp32
    "pool2 1x1 128->64": dict(chain_red=512),
    "pool2 2x2 map": dict(chain_red=512),
}
RAGGED = [("1x1 tail M=35", 1, 5, 7, 24, 40, 1, 1, 1, 0, 0, 0, 1),
          ("3x3 1-pixel", 1, 1, 1, 16, 8, 3, 3, 1, 1, 0, 0, 1),
          ("5x5 N=8 tail", 3, 3, 5, 8, 8, 5, 5, 1, 2, 0, 0, 1),
          ("convT 1x1 map", 2, 1, 1, 8, 8, 3, 3, 2, 1, 1, 0, 1),
          ("pool2 2x2 map", 1, 2, 2, 16, 8, 1, 1, 1, 0, 0, 2, 1)]
# name, B, H, W, Cin, Cout, R, S, stride, pad, transposed, mode, bn: the parity cases of tools/gpu_lab.py run_kernels
CASES = [
    ("1x1 72->32", 2, 12, 20, 72, 32, 1, 1, 1, 0, 0, 0, 1),
    ("1x1 256->128", 1, 16, 24, 256, 128, 1, 1, 1, 0, 0, 0, 1),
    ("1x1 64->256", 1, 8, 8, 64, 256, 1, 1, 1, 0, 0, 0, 1),
    ("3x3 128->32", 2, 12, 20, 128, 32, 3, 3, 1, 1, 0, 0, 1),
    ("3x3 32->8", 1, 9, 7, 32, 8, 3, 3, 1, 1, 0, 0, 1),
    ("5x5 64->8", 1, 10, 14, 64, 8, 5, 5, 1, 2, 0, 0, 1),
    ("7x7s2 8->64", 2, 32, 32, 8, 64, 7, 7, 2, 3, 0, 0, 0),
    ("convT 64->64", 2, 6, 10, 64, 64, 3, 3, 2, 1, 1, 0, 1),
    ("convT 16->16", 1, 5, 3, 16, 16, 3, 3, 2, 1, 1, 0, 1),
    ("pool2 1x1 128->64", 2, 12, 20, 128, 64, 1, 1, 1, 0, 0, 2, 1),
    ("up2 3x3 128->64", 1, 6, 10, 128, 64, 3, 3, 1, 1, 0, 1, 1),
    ("up2 3x3 16->8", 2, 4, 4, 16, 8, 3, 3, 1, 1, 0, 1, 1),
]


# ================================================================================================ single-rounding operands (round 10)
# The third operand class.  As above, all fp32 arithmetic is exact in any order; but the values that reach a 16-bit store need more
# significant bits than the storage type holds, so that every store is exactly ONE round-to-nearest-even of an exactly known number -
# and the kernel has to hit it bit for bit, ties included.  The fp64 reference applies every rounding point the kernels document, in
# their order (rnd = to the storage type and back, of a number asserted exact in fp32 - torch converts double to half through float,
# the assertion takes the double rounding out of the reference):
#   w_T = rnd(w)                          the weight pack
#   a   = rnd(relu(x * scale + shift))    the prologue (one fp32 fma, exact by construction; ReLU commutes with the rounding; the
#                                         pooling gather rounds the mean of the four pixels of a window, once)
#   y   = rnd(conv(a, w_T));  stat_sum, stat_sq: sums of the ROUNDED y
#   eff = rnd(dy + q + r * yfwd)          the effective gradient
#   dz  = conv_backward(eff, w_T) * (x * scale + shift > 0), unrounded;  red1 = sum dz;  red2 = sum dz * xhat
#   gx  = rnd(gold + scale * dz)          ONE rounding
#   dw  = sum a * eff
# Recipe ("main"): |x| < 2**(sig - 1) integers (sig = 11 / 8), scale in {0.75, 1, 1.25, 1.5, 3}, shift multiples of 0.5 in [-1.5, 1.5],
# dy and yfwd integers below 2**(sig - 1) (dy below 2**(sig - 2) under the correction), q multiples of 0.5, r in {+-0.75, +-1.5, 0}, gold multiples of 0.25, weights
# in {-1, 0, 1} (w_T leaves them unchanged) with every (tap, input channel) pair covered; the number of nonzero weights per output /
# per input channel is capped so that f16 does not overflow.  "weights": w = k 2**-12, k odd of up to 13 bits, on the round-8
# activations - the forward and the data gradient must use rnd(w).  "subnormal" (f16): the main recipe with x, shift, mean, the
# gradients and the weights scaled by 2**-12, which puts the stored results around 2**-14 - gradual underflow, where loss-scaled f16
# gradients live - while every value the matrix unit reads stays normal (or zero).
ROUND_SCALE = [0.75, 1.0, 1.25, 1.5, 3.0]
ROUND_R = [-1.5, -0.75, 0.0, 0.75, 1.5]
NNZ_OUT = {1: 128, 2: 128}     # nonzero weights per output element / per input-gradient element ("main"): sigma(y) ~ sqrt(nnz) * rms(a) stays
NNZ_IN = {0: 32, 1: 10}        # (by with_q) 4.5 sigma below f16's 65504 with rms(a) ~ 600 and 3 * rms(eff) ~ 2000 - and the stored gradient
                               # only a few bits wider than the type, so that exact ties are common
MIN_ULP = {1: 2.0 ** -24, 2: 2.0 ** -133}


def _rnd(t, dt, name):
    """One round-to-nearest-even to the storage type of a number that is exact in fp32."""
    f = t.float()
    assert torch.equal(f.double(), t), f"(a) {name} is not exact in fp32"
    return f.to(dt).double()


def step_of(*ts):
    """The common power-of-two step of the (fp64, exactly known) values: the largest 2**e that divides all of them."""
    e = None
    for t in ts:
        t = t[t != 0]
        if t.numel() == 0:
            continue
        m, ex = torch.frexp(t.abs())
        mi = (m * 2.0 ** 53).to(torch.int64)
        tz = torch.log2((mi & -mi).double()).round().to(torch.int64)
        s = int((ex.to(torch.int64) - 53 + tz).min())
        e = s if e is None else min(e, s)
    return 2.0 ** (0 if e is None else e)


def rounding_shares(t, dtype):
    """Of the exactly known values t (fp64) rounded to the storage type: the shares that are not representable, that are exact ties
    (resolved to the even neighbour above / below), and that round up / down without being ties."""
    r = t.float().to(DT[dtype]).double()
    _, ex = torch.frexp(t.abs())
    ulp = torch.clamp(torch.ldexp(torch.ones_like(t), ex - SIG_BITS[dtype]), min=MIN_ULP[dtype])
    frac = torch.remainder(t.abs() / ulp, 1.0)
    tie = (frac == 0.5) & (t != 0)
    n = float(t.numel())
    return dict(inexact=float((r != t).sum()) / n, tie=float(tie.sum()) / n, tie_up=float((tie & (r > t)).sum()) / n,
                tie_down=float((tie & (r < t)).sum()) / n, up=float((~tie & (r > t)).sum()) / n, down=float((~tie & (r < t)).sum()) / n)


def _round_weights(g, c, density, cover=True):
    """{-1, 0, 1} weights [Cout][Cin][T] at the given density; cover: every (tap, input channel) pair nonzero in some output channel.
    Every output channel has a nonzero weight."""
    Cout, Cin, T = c.Cout, c.Cin, c.R * c.S
    sel = torch.rand(Cout, Cin, T, generator=g, dtype=torch.float64) < density
    ci, tt = torch.meshgrid(torch.arange(Cin), torch.arange(T), indexing="ij")
    if cover:
        sel[(ci * T + tt) % Cout, ci, tt] = True
    co = torch.arange(Cout)
    sel[co, co % Cin, (co // Cin) % T] = True
    return _pick(g, [-1.0, 1.0], (Cout, Cin, T)) * sel


def _check_rounding(o):
    """Operands.check_rounding: the conditions under which every compared store is exactly one rounding of an exactly known number,
    and under which the comparison is not empty - on the reference alone, before any launch.  Returns the measured figures."""
    c, dt, lim = o.case, DT[o.case.dtype], float(2 ** 24)
    fig = {}
    ua, uw, ueff = step_of(o.a), step_of(o.w_T), step_of(o.eff)
    aa = o.a_in.abs().requires_grad_(True)
    wa = o.w_T.abs().requires_grad_(True)
    ya = o.fwd(aa, wa)
    # (a) exact in fp32 in any order: what enters a rounding point (z, the sum behind eff and gx: asserted by _rnd when the reference was
    # built), every output, data-gradient, red1 term - the same convolution over the operands' absolute values, in units of the step
    fig["a_y"] = float(ya.detach().max()) / (ua * uw * o.pool)
    if "logits" in o.parts:     # the fp32 logits: compared unrounded (y is y_pre), so no share of y is asked for - the rounding points
        assert torch.equal(o.y, o.y_pre) and torch.equal(o.y.float().double(), o.y), "(a) logits are not representable in fp32"   # are a and w
    if o.backward:
        (ya * o.eff.abs()).sum().backward()
        fig["a_dz"] = float(aa.grad.max()) / (ueff * uw * o.pool)
        fig["dw_terms"] = float(wa.grad.max()) / (ua * ueff * o.pool)       # below 2**24: the weight gradient is exact too (see dw_exact)
    for k in ("a_y", "a_dz"):
        assert fig.get(k, 0.0) < lim, f"(a) {k[2:]}: sum |term| / u = {fig[k]:.3g} >= 2**24"
    # (b) the fp32 chains of the per-channel sums of stored values
    if "fwd" in o.parts:
        fig["b_sum"] = o.chain * float(o.y.abs().max()) / step_of(o.y)
        assert fig["b_sum"] < lim, f"(b) stat_sum: {fig['b_sum']:.3g} >= 2**24"
    if "dgrad" in o.parts:
        fig["b_red1"] = o.chain_red * float(o.dz.abs().max()) / step_of(o.dz)
        assert fig["b_red1"] < lim, f"(b) red1: {fig['b_red1']:.3g} >= 2**24"
    # (c) nothing overflows, the outputs are not mostly zero
    stored = [("a", o.a), ("w_T", o.w_T), ("eff", o.eff)] + ([("y", o.y)] if "fwd" in o.parts else []) + ([("gx", o.gx)] if "dgrad" in o.parts else [])
    for name, t in stored:
        assert bool(torch.isfinite(t).all()), f"(c) {name} overflows {dt}"
    fig["nonzero_y"] = float((o.y != 0).double().mean())
    assert fig["nonzero_y"] >= 0.9, f"(c) only {fig['nonzero_y']:.3f} of the outputs are nonzero"
    # (d) / (e): the shares of values that need the rounding, per compared store and per exercised prologue point
    sh = {}
    if "fwd" in o.parts:
        sh["y"] = rounding_shares(o.y_pre, c.dtype)
    if "dgrad" in o.parts:
        sh["gx"] = rounding_shares(o.gx_pre, c.dtype)
    if c.bn and o.round_a:
        sh["a"] = rounding_shares(o.a_pre, c.dtype)
    if o.with_q and o.backward:
        sh["eff"] = rounding_shares(o.eff_pre, c.dtype)
    sh["w"] = rounding_shares(o.w[o.w != 0], c.dtype)
    fig["shares"] = sh
    if o.kind == "main":
        for k in ("y", "gx"):
            if k in sh:
                s = sh[k]
                assert s["inexact"] >= 0.25 and s["tie"] >= 0.05 and s["tie_up"] > 0 and s["tie_down"] > 0 and s["up"] >= 0.05 and s["down"] >= 0.05, \
                    f"(d) {k}: {s}"
        for k in ("a", "eff"):
            if k in sh:
                assert sh[k]["inexact"] >= 0.05 and sh[k]["tie"] >= 0.01, f"(e) {k}: {sh[k]}"
    elif o.kind == "weights":   # the rounding point this set is for: the pack
        assert sh["w"]["inexact"] >= 0.25 and sh["w"]["tie"] >= 0.01 and sh["w"]["up"] >= 0.05 and sh["w"]["down"] >= 0.05, f"weights: {sh['w']}"
    else:                       # "subnormal": at least 10 % of the compared stores in (0, 2**-14), and they need the rounding
        for k, t, pre in (("y", o.y, o.y_pre), ("gx", o.gx if "dgrad" in o.parts else None, getattr(o, "gx_pre", None))):
            if k in sh:
                sub = (t != 0) & (t.abs() < 2.0 ** -14)
                fig["subnormal_" + k] = float(sub.double().mean())
                fig["subnormal_inexact_" + k] = float((sub & (t != pre)).double().mean())
                assert fig["subnormal_" + k] >= 0.10 and fig["subnormal_inexact_" + k] >= 0.05, (k, fig)
    return fig


Operands.check_rounding = _check_rounding


def make_rounding_operands(dtype, B, H, W, Cin, Cout, R, S, stride, pad, transposed=0, mode=0, bn=1, with_q=0, acc=0,
                           parts=("fwd", "wgrad", "dgrad"), seed=0, chain=128, chain_red=128, kind="main", nnz_out=None, nnz_in=None, cover=True, round_a=True):
    """As make_operands - the same case tuple, the same fields - on the single-rounding operands (see above).  kind: "main", "weights"
    (the weight-rounding set) or "subnormal" (f16).  nnz_out / nnz_in: caps on the nonzero weights that meet in one output element / in
    one input-gradient element (defaults NNZ_OUT / NNZ_IN).  round_a=False: the activation enters UNROUNDED - the factor form of
    dmm_conv5_wgrad_stats (wg5.hip PA = 3), which never forms the activation: dw = scale * sum m x dy + shift * sum m dy, m the ReLU mask.
    Further fields: *_pre, the exactly known numbers in front of each
    rounding; w_T; dw_exact, whether the weight gradient is exact in fp32 in any order (then compared bit for bit) and dw_bound, the
    bound it is held to otherwise; sq_bound, red2_bound."""
    assert dtype in (1, 2) and kind in ("main", "weights", "subnormal") and (kind != "subnormal" or (dtype == 1 and not acc))
    dt, sig = DT[dtype], SIG_BITS[dtype]
    c = SimpleNamespace(dtype=dtype, B=B, H=H, W=W, Cin=Cin, Cout=Cout, R=3 if transposed else R, S=3 if transposed else S,
                        stride=stride, pad=pad, transposed=transposed, mode=mode, bn=bn)
    parts = tuple(parts)
    if not bn or (mode == 0 and not transposed and stride != 1):
        parts = tuple(p for p in parts if p != "dgrad")
    g = torch.Generator().manual_seed(seed)
    v = lambda t: t.view(1, -1, 1, 1)  # noqa: E731
    Ho, Wo = out_hw(c)
    ri = lambda bits, shape: torch.randint(-(2 ** bits) + 1, 2 ** bits, shape, generator=g).double()  # noqa: E731
    T = c.R * c.S
    if kind == "weights":       # the round-8 activations and gradients (small halves)
        x = torch.randint(-3, 4, (B, Cin, H, W), generator=g).double()
        scale, shift = _pick(g, [0.5, 1.0, 2.0], (Cin,)), _pick(g, [-1.0, 0.0, 1.0], (Cin,))
        dy = torch.randint(-2, 3, (B, Cout, Ho, Wo), generator=g).double()
        yf = 2.0 * torch.randint(-2, 3, (B, Cout, Ho, Wo), generator=g).double()
        q, r = _pick(g, [-1.0, 0.0, 1.0], (Cout,)), _pick(g, [-1.0, -0.5, 0.0, 0.5, 1.0], (Cout,))
        gold = torch.randint(-2, 3, (B, Cin, H, W), generator=g).double()
    else:
        x = ri(sig - 1, (B, Cin, H, W))
        scale = _pick(g, ROUND_SCALE, (Cin,))
        shift = 0.5 * torch.randint(-3, 4, (Cin,), generator=g).double()
        dy = ri(sig - 2 if with_q else sig - 1, (B, Cout, Ho, Wo))      # (narrower under the correction: the sum is what is stored)
        yf = ri(sig - 1, (B, Cout, Ho, Wo))
        q = 0.5 * torch.randint(-3, 4, (Cout,), generator=g).double()
        r = _pick(g, ROUND_R, (Cout,))
        gold = 0.25 * ri(sig - 1, (B, Cin, H, W))
    mean = torch.randint(-2, 3, (Cin,), generator=g).double()
    invstd = _pick(g, [0.5, 1.0, 2.0], (Cin,))
    # weights: density from the caps
    fan_out = Cin * (4 if transposed else T)                # taps that can meet in one output element
    fan_in = Cout * T * (4 if mode == 1 else 1)             # ... in one input-gradient element
    no = nnz_out or (16 if kind == "weights" else NNZ_OUT[dtype])      # ("weights": the products step in 2**-13, so few of them)
    if "logits" in parts:       # fp32 logits: no stored output to overflow f16 - every weight may be nonzero ((a) holds the sums)
        assert "fwd" not in parts and kind != "subnormal" and mode == 0 and not transposed and stride == 1
        no = nnz_out or fan_out
    ni = nnz_in or (4 if kind == "weights" else NNZ_IN[with_q])
    density = min(0.5, no / fan_out, ni / fan_in if "dgrad" in parts else 1.0)
    wslots = _round_weights(g, c, density, cover)
    if kind == "weights":
        k = 2.0 * torch.randint(0, 2 ** 12, wslots.shape, generator=g).double() + 1.0     # odd, up to 13 bits
        wslots = wslots * k * 2.0 ** -12
    if kind == "subnormal":
        s = 2.0 ** -12
        x, shift, mean, dy, yf, q, wslots = x * s, shift * s, mean * s, dy * s, yf * s, q * s, wslots * s
    w = wslots.view(Cout, Cin, c.R, c.S)
    if transposed:
        w = w.permute(1, 0, 2, 3).contiguous()
    if not with_q:
        yf = q = r = None
    if not acc:
        gold = None
    for name, t in (("x", x), ("dy", dy), ("yfwd", yf), ("gold", gold)):      # the inputs stored in the storage type are representable
        assert t is None or torch.equal(t.to(dt).double(), t), f"{name} is not representable in {dt}"
    # ---- the reference, every rounding point in the kernels' order
    w_T = _rnd(w, dt, "w")
    z = x * v(scale) + v(shift)
    pool = 0.25 if mode == 2 else 1.0
    if bn:
        a_pre = F.avg_pool2d(F.relu(z), 2, 2) if mode == 2 else F.relu(z)     # (the pooling gather: fp32 mean of four, rounded once)
        a = _rnd(a_pre, dt, "relu(x * scale + shift)") if round_a else a_pre
    else:
        a_pre = a = x.clone()

    def fwd(act, wt):
        """The case's convolution of the (for mode 2: already pooled) activation."""
        if mode == 2:
            return F.conv2d(act, wt)
        return conv(act, wt, c)
    backward = "wgrad" in parts or "dgrad" in parts
    eff_pre = eff = dy
    if with_q:
        t = v(r) * yf + v(q)
        assert torch.equal(t.float().double(), t), "(a) fma(yfwd, r, q) is not exact in fp32"
        eff_pre = dy + t
        eff = _rnd(eff_pre, dt, "dy + q + r * yfwd")
    ar = a.clone().requires_grad_(backward)
    wr = w_T.clone().requires_grad_(backward)
    y_pre = fwd(ar, wr)
    o = Operands(case=c, parts=parts, kind=kind, with_q=with_q, acc=acc, chain=chain, chain_red=chain_red, x=x, scale=scale, shift=shift,
                 mean=mean, invstd=invstd, z=z, dy=dy, yf=yf, q=q, r=r, eff=eff, eff_pre=eff_pre, gold=gold, w=w, w_T=w_T, wslots=wslots,
                 Ho=Ho, Wo=Wo, backward=backward, a=a, a_in=a, a_pre=a_pre, pool=1.0, round_a=round_a, fwd=fwd, density=float((wslots != 0).double().mean()))
    o.xhat = (x - v(mean)) * v(invstd)
    o.y_pre = y_pre.detach()
    if "logits" in parts:       # stored unrounded
        assert torch.equal(o.y_pre.float().double(), o.y_pre), "(a) conv(a, w_T) is not representable in fp32"
        o.y = o.y_pre
    else:
        o.y = _rnd(o.y_pre, dt, "conv(a, w_T)")
    o.stat_sum, o.stat_sq = o.y.sum(dim=(0, 2, 3)), (o.y ** 2).sum(dim=(0, 2, 3))
    o.sq_bound = chain * 2.0 ** -24 * o.stat_sq          # per channel: one fp32 rounding per added y**2, `chain` of them per partial
    if backward:
        (y_pre * eff).sum().backward()
        o.dw = wr.grad
        # the number of terms added into one weight-gradient element, and their magnitudes: the same sums over ones / absolute values
        wn = torch.ones_like(w_T).requires_grad_(True)
        fwd(torch.ones_like(a), wn).sum().backward()
        wm = w_T.abs().clone().requires_grad_(True)
        # (the factor form adds scale * x and shift apart: |scale x| + |shift| under the mask in place of |a|)
        amag = a.abs() if round_a else (z > 0) * ((v(scale) * x).abs() + v(shift).abs())
        (fwd(amag, wm) * eff.abs()).sum().backward()
        o.dw_terms, o.dw_mag = wn.grad, wm.grad
        o.dw_exact = float(wm.grad.max()) / (step_of(a) * step_of(eff)) < 2 ** 24
        o.dw_bound = o.dw_terms * 2.0 ** -23 * o.dw_mag
        da = ar.grad
        if mode == 2:    # back through the pooling: a quarter of the pooled pixel's gradient to each pixel of the window
            da = F.interpolate(da, scale_factor=2, mode="nearest") * 0.25
        o.dz = da * (z > 0) if bn else da
        sdz = v(scale) * o.dz
        assert torch.equal(sdz.float().double(), sdz), "(a) scale * dz is not exact in fp32"
        o.gx_pre = sdz + (gold if acc else 0.0)
        o.gx = _rnd(o.gx_pre, dt, "gold + scale * dz")
        o.red1, o.red2 = o.dz.sum(dim=(0, 2, 3)), (o.dz * o.xhat).sum(dim=(0, 2, 3))
        # red2: one fp32 rounding per added product, chain_red of them per partial; `unc` is the further term of a kernel that adds
        # dz * x in fp32 and centres the total in fp64 (|x| <= |x - mean| + |mean|): |mean| invstd sum |dz|
        o.red2_bound = chain_red * 2.0 ** -24 * (o.dz * o.xhat).abs().sum(dim=(0, 2, 3))
        o.red2_unc = chain_red * 2.0 ** -24 * mean.abs() * invstd * o.dz.abs().sum(dim=(0, 2, 3))
    return o


@functools.lru_cache(maxsize=2)
def cached_rounding_operands(*args, **kw):
    return make_rounding_operands(*args, **kw)


# ------------------------------------------------------------------------------------------------ the cases of tests/test_rounding_kernels_gpu.py
# (shared with tests/test_rounding_operands_cpu.py).  Rounding needs no multi-tile walk: the smallest shape each family's resolve
# accepts - the backward shapes above and the parity shapes where the family takes them, else its FORWARD shape (cf: eight tiles per CU).
# forward: family, case tuple as CASES, make_rounding_operands arguments: the fp32 chain of the statistics (header of
# tests/test_exact_kernels_gpu.py) and, where the defaults overflow, the weight caps
ROUND_FORWARD = [
    ("pig", ("1x1 160->128 1x16x24", 1, 16, 24, 160, 128, 1, 1, 1, 0, 0, 0, 1), dict(chain=32)),
    ("pig", ("1x1 72->128 2x12x20", 2, 12, 20, 72, 128, 1, 1, 1, 0, 0, 0, 1), dict(chain=32)),
    ("conv3", ("3x3 128->32 2x7x9", 2, 7, 9, 128, 32, 3, 3, 1, 1, 0, 0, 1), dict(chain=32)),
    ("conv3", ("3x3 128->32 2x12x20", 2, 12, 20, 128, 32, 3, 3, 1, 1, 0, 0, 1), dict(chain=32)),
    ("conv3", ("7x7s2 8->64 2x32x32", 2, 32, 32, 8, 64, 7, 7, 2, 3, 0, 0, 0), dict(chain=32)),      # the stem: no BatchNorm in front
    ("cf", FORWARD[5][1], dict(chain=128, nnz_out=8)),      # (2091 tiles: the largest |y| of 8.6 M outputs, times a chain of 128)
    ("cvw", ("convT 128->128 2x7x9", 2, 7, 9, 128, 128, 3, 3, 2, 1, 1, 0, 1), dict(chain=128)),
    ("cvp", ("convT 384->256 1x11x19", 1, 11, 19, 384, 256, 3, 3, 2, 1, 1, 0, 1), dict(chain=32)),
]
# the generic kernel on CASES (every other forward family switched off), by use_mfma: the MFMA forward (chain 32) and the scalar
# kernel, f16 only - the library has no bf16 scalar kernels.  The scalar kernel's chain of 128 leaves |y| / u two bits less: fewer
# weights per output, and where covering every (tap, channel) pair alone takes too many (5x5 64->8: 200 per output channel) or the
# pooled activation steps in sixteenths, no coverage.
GENERIC_KW = {1: dict(chain=32), 0: dict(chain=128, nnz_out=32)}
SCALAR_KW = {"5x5 64->8": dict(cover=False), "pool2 1x1 128->64": dict(nnz_out=8, cover=False)}


def generic_kw(name, mfma):
    return {**GENERIC_KW[mfma], **(SCALAR_KW.get(name, {}) if not mfma else {})}


_ALL4 = [(1, 1), (1, 0), (0, 1), (0, 0)]
# backward through backward_case, as BACKWARD.  cvd3 and wg5's transposed form refuse the effective-gradient prologue (cvp.hip
# cvd_resolve, wg5.hip wg5_resolve: the gradient segment's q must be null), so they run without it.
ROUND_BACKWARD = [
    ("fused", "bw1", (1, 16, 24, 160, 128, 1, 1, 0, 0, 0), _ALL4),
    ("dgrad", "conv3", (2, 7, 9, 128, 32, 3, 3, 1, 0, 0), _ALL4),
    ("dgrad", "cvp", (1, 9, 17, 256, 256, 3, 3, 1, 1, 0), [(0, 1), (0, 0)]),
    ("dgrad", "cvp", (1, 9, 7, 128, 64, 3, 3, 1, 0, 1), [(0, 1), (0, 0)]),
    ("wgradT", "wg3", (3, 5, 3, 128, 32, 3, 3, 1, 0, 0), [(1, 0), (0, 0)]),
    ("wgradT", "wg3", (2, 12, 20, 128, 32, 3, 3, 1, 0, 0), [(1, 0), (0, 0)]),
    ("wgrad", "wgp/wgpw", (3, 5, 3, 128, 64, 3, 3, 1, 1, 0), [(1, 0), (0, 0)]),
    ("wgrad", "wgp/wgpw", (2, 12, 20, 128, 64, 3, 3, 1, 1, 0), [(1, 0), (0, 0)]),
    ("wgradT", "wg5", (1, 13, 21, 64, 3, 5, 5, 2, 0, 0), [(0, 0)]),
    ("wgrad", "wg5", (2, 12, 20, 8, 64, 3, 3, 1, 0, 0), [(1, 0), (0, 0)]),
]
# the merged four-phase launches (tests/test_merged_phase_kernels_gpu.py) on the single-rounding operands: one per merged kernel, on
# the smallest shape of FORWARD_MERGED / BACKWARD_MERGED it takes - form, case tuple, make_rounding_operands arguments (as ROUND_FORWARD)
ROUND_FORWARD_MERGED = [("cvw",) + ROUND_FORWARD[6][1:], ("cvp",) + ROUND_FORWARD[7][1:]]
ROUND_BACKWARD_MERGED = [BACKWARD_MERGED[1][0]]      # (3, 5, 3, 128, 64): idle units beside rounding stores
ROUND_CONV5 = (1, 13, 21)          # conv5_stats_case: B, H, W (the factor correlations run over the workgroup's whole walk: chain_red = B H W)
ROUND_PIG = ROUND_FORWARD[0][1]
ROUND_GENERIC = CASES[0]             # 1x1 72->32 2x12x20: 32 output channels, which pig refuses
ROUND_BW1 = ROUND_BACKWARD[0][2]
ROUND_CONV3_DGRAD = ROUND_BACKWARD[1][2]


# ================================================================================================ the logits launch (round 13)
# dmm_conv_logits: the network's last convolution (5x5, 64 -> classes, behind BN+ReLU), written UNROUNDED as fp32 NCHW.  Part "logits"
# of make_operands / make_rounding_operands: the output has to be representable in fp32 only, there are no statistics, and - since
# thin.hip zero-pads AFTER the prologue - the reference must tell that from padding before it on every image's border (check(): (p)).
# The cases of tests/test_logits_kernels_gpu.py, shared with tests/test_logits_operands_cpu.py: family that must run, storage type,
# use_mfma, whether the thin family is switched off, (B, H, W, Cin, Cout, R, pad) - all behind BN+ReLU - and why the case is there.
def thin_geometry(B, H, W, R=2, slots=2 * 256):
    """thin.hip thin_resolve: strips of 128 - 2R output columns, the row split whose rounds x (rows + 2R) is smallest (the finer on a tie)."""
    wout = 128 - 2 * R
    nxs = -(-W // wout)
    best, rows_per_wg, nys = -1, 8, -(-H // 8)
    for n in range(1, max(1, H // 8) + 1):
        rows = -(-H // n)
        wgs = B * (-(-H // rows)) * nxs
        cost = -(-wgs // slots) * (rows + 2 * R)
        if best < 0 or cost <= best:
            best, rows_per_wg, nys = cost, rows, -(-H // rows)
    return dict(nxs=nxs, last_cols=W - (nxs - 1) * wout, rows_per_wg=rows_per_wg, nys=nys, last_rows=H - (nys - 1) * rows_per_wg,
                nwg=B * nys * nxs, steps=rows_per_wg + 2 * R + 1)


def xcd_remap(bid, nblocks):
    """common.h xcd_remap: the logical workgroup of hardware workgroup `bid` (every XCD one contiguous range)."""
    x, i = bid & 7, bid >> 3
    lo, rem = nblocks >> 3, nblocks & 7
    return x * lo + min(x, rem) + i


def halo_tiles(B, Ho, Wo):
    """halo.hip halo_plan: 8 x 16 output tiles, walked by min(CUs, tiles) workgroups."""
    return B * (-(-Ho // 8)) * (-(-Wo // 16))


_T = "thin"
LOGITS_THIN = [   # (B, H, W, classes), what thin_geometry must give, why
    ((2, 37, 131, 3), dict(nxs=2, last_cols=7, rows_per_wg=10, nys=4, last_rows=7, nwg=16, steps=15), "two column strips, ragged last row strip, the ring wraps"),
    ((3, 37, 255, 3), dict(nxs=3, nys=4, nwg=36), "a grid that is no multiple of 8: xcd_remap's remainder"),
    ((1, 9, 125, 1), dict(nxs=2, last_cols=1, rows_per_wg=9, nys=1), "KN = 1; the second strip owns one column"),
    ((2, 45, 249, 2), dict(nxs=3, last_cols=1, rows_per_wg=9, nys=5, last_rows=9, nwg=30), "KN = 2; three strips, the last one column wide; no ragged row strip"),
    ((1, 7, 124, 3), dict(nxs=1, last_cols=124), "exactly one full strip"),
    ((1, 3, 5, 3), dict(nwg=1, rows_per_wg=3), "a map smaller than the tap box, fewer rows than ring slots"),
    ((1, 1, 1, 2), dict(nwg=1), "a single pixel"),
]
# family, dtype, use_mfma, thin switched off, (B, H, W, Cin, Cout, R, pad), note
LOGITS = [(_T, dt, 1, 0, (B, H, W, 64, N, 5, 2), why) for (B, H, W, N), _, why in LOGITS_THIN for dt in (1, 2)] + [
    ("halo", 1, 1, 0, (1, 100, 350, 64, 4, 5, 2), "thin has no 4-class instantiation; 286 tiles on 256 CUs, both map edges ragged"),
    ("halo", 1, 1, 0, (2, 20, 24, 32, 3, 5, 2), "32 input channels: the head of every small test network"),
    ("halo", 1, 1, 1, (2, 37, 131, 64, 3, 5, 2), "thin switched off"),
    ("halo", 0, 1, 0, (2, 12, 20, 64, 3, 3, 1), "fp32: the 3x3's weights fit halo's LDS (72 KB; the 64-channel 5x5's 200 KB do not)"),
    ("generic", 2, 1, 0, (2, 37, 131, 64, 4, 5, 2), "bf16, 4 classes: thin and halo both refuse"),
    ("generic", 2, 1, 0, (2, 37, 131, 32, 3, 5, 2), "bf16, 32 input channels"),
    ("generic", 2, 1, 1, (2, 37, 131, 64, 3, 5, 2), "bf16, thin switched off"),
    ("generic", 0, 1, 0, (2, 37, 131, 64, 3, 5, 2), "fp32 5x5, MFMA"),
    ("generic", 0, 0, 0, (2, 37, 131, 64, 3, 5, 2), "fp32 5x5, scalar kernel"),
    # (8 channels x 25 taps are 13 fp32 chunks, 26 KB: THIS 5x5 fits halo's LDS, and halo takes it; the scalar kernel keeps the tail on igemm)
    ("halo", 0, 1, 0, (3, 3, 5, 8, 8, 5, 2), "fp32 5x5 8 -> 8: the N = 8 tail"),
    ("generic", 0, 0, 0, (3, 3, 5, 8, 8, 5, 2), "fp32 5x5 8 -> 8 on the scalar kernel: igemm's N = 8 tail"),
    ("generic", 1, 0, 0, (1, 9, 125, 64, 3, 5, 2), "f16 scalar kernel"),
]
LOGITS_HALO_WALK = (1, 100, 350)      # the halo case whose tiles outnumber the compute units
LOGITS_REPRO = (3, 37, 255, 64, 3, 5, 2)
# single rounding: family, dtype, thin switched off, shape; each with kinds "main" and "weights"
ROUND_LOGITS = [(_T, dt, 0, s) for s in ((2, 37, 131, 64, 3, 5, 2), (1, 9, 125, 64, 1, 5, 2)) for dt in (1, 2)] + [
    ("halo", 1, 0, (2, 12, 20, 64, 4, 5, 2)),
    ("generic", 2, 0, (2, 12, 20, 64, 4, 5, 2)),
]
ROUND_LOGITS_KINDS = ("main", "weights")
DT_NAME = {0: "fp32", 1: "fp16", 2: "bf16"}


def logits_id(family, dtype, mfma, thin_off, s):
    B, H, W, Cin, Cout, R, pad = s
    return f"{family}-{DT_NAME[dtype]}-{R}x{R}-{Cin}to{Cout}-{B}x{H}x{W}" + ("" if mfma else "-scalar") + ("-thinoff" if thin_off else "")
