"""Parameter groups on the GPU: the segmented Adam kernel (dmm_adam_step_segmented, dmm_adam_step_guarded_segmented) and what stands on
it (FusedAdam(param_groups=...), fine_tune_groups, the agent's config fields).

  0. THE RECORDED BITS.  tests/golden/adam_bits_sha256.json holds, per case, the SHA-256 of the inputs, of p, m and v and (guarded) of
     the 64-byte state block, as a library built from the csrc of the commit the file names computed them on an MI355X - the last
     commit that had four Adam kernels (adam_kernel, two guarded ones, the segmented one).  Cases 1 and 3 and the whole-range cases
     compare against it (_golden).  The file was written by running this file as a script against that library,
         DMM_LIB_PATH=<that build>/libdmmfods_hip.so python tests/test_param_groups_gpu.py <commit>
     with the guarded cases put through that commit's guarded step over ranges (an entry point the library no longer has).  A change
     that alters Adam's bits ON PURPOSE renews it from its own build and says so; any other change leaves it alone.
  1. BIT EQUALITY of the two forms of the kernel: for decoupled = 0 the one launch under a table equals dmm_adam_step (the whole-range
     form) called once per segment on offset pointers with the segment's scalars and step - t0, in p, m and v; what lies in no
     segment keeps its bits (NaN / inf patterns), the gradient arena is never written.  No tolerance.  Plus the recorded bits.
  2. Decoupled decay, every element, against the fp64 restatement of tests/test_helpers_gpu.py::test_adam_step_every_element:
     |p - p_ref| <= 2^-20 |u_ref| + 3 ulp(p0) (u_ref the Adam update term; the fp32 rounding of the decay factor, the product and the
     final subtraction are the three ulps); m and v keep that test's bounds.
  3. The guarded segmented step against the recorded bits of the guarded step over ranges on the same runs: p, m, v and the state
     block (sumsq, grad_norm, clip_coef, applied_steps, ...) bit-equal; an inf inside a segment skips the step, an inf in a gap is not
     seen.  Then dmm_adam_step and dmm_adam_step_guarded over a whole range against their recorded bits.
  4. Model level (tiny mid-3 net, fp32, 2 x 64 x 96): three steps with fine_tune_groups against torch.optim.Adam over the same groups
     (tests/test_freeze_gpu.py's bounds), with and without decoupled decay; freeze and release on the guarded path; one Adam entry
     point per step.
  5. The agent with the three config fields, StepLR and a resume.
Every case prints its figures ([groups] lines)."""
import collections
import hashlib
import json
import os
import shutil
import sys

import numpy as np
import pytest
import torch

from dmmfods_amd.utils.Dense_U_Net_lidar_helper import get_config

pytestmark = pytest.mark.gpu

DEV = "cuda"
ENCODER = ("features.", "stream_2_features.", "concat_module.")
TINY = dict(growth_rate=8, block_config=(2, 2, 2, 2), num_init_features=16)
GAP_BITS = np.array([0x7fc00001, 0x7f800000, 0xff800000, 0xffc12345], dtype=np.uint32)   # NaN, +inf, -inf, NaN with a payload
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adam_bits_sha256.json")
_RECORDING = None   # a dict while this file runs as a script: _golden fills it and compares nothing


# ------------------------------------------------------------------------------------------------ recorded bits
def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(a.detach().cpu().contiguous().numpy().tobytes() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _golden(name, inputs, P, M, V, state=None):
    """The result of case `name` against the bits recorded in tests/golden/adam_bits_sha256.json (the file's "commit" built them): the
    SHA-256 of the four input arrays first - a random generator that has changed is reported as that, not as a kernel fault - then
    of p, m and v (whole arenas, gaps included) and, guarded, of the 64-byte state block."""
    row = {"inputs": _sha(*inputs), "p": _sha(P), "m": _sha(M), "v": _sha(V)}
    if state is not None:
        assert state.numel() * state.element_size() == 64
        row["state"] = _sha(state)
    if _RECORDING is not None:
        _RECORDING[name] = row
        return
    pinned = json.load(open(GOLDEN))["cases"][name]
    assert row["inputs"] == pinned["inputs"], (name, "the INPUTS differ from the recorded ones (random generator?), not the kernel's results")
    assert row == pinned, (name, [k for k in row if row[k] != pinned[k]])


# ------------------------------------------------------------------------------------------------ tables
def _layout(lengths, gaps, lead):
    """[(begin, count)] for segments of `lengths` with gaps[i] elements behind segment i, `lead` in front of the first; and n."""
    segs, pos = [], lead
    for ln, gap in zip(lengths, gaps):
        segs.append((pos, ln))
        pos += ln + gap
    return segs, pos


def _case_a():
    """Lengths 1, 2, 3, 5, 255, 257 and 70 001 (many workgroups: 69 chunks), begins at every residue mod 4, a gap in front of the first
    segment, between segments and behind the last, adjacent segments of different classes, all 16 classes."""
    lengths = [1, 2, 3, 5, 255, 257, 70001, 1, 2, 3, 5, 255, 257, 4, 1024, 2049, 9, 6]
    gaps = [0, 0, 2, 0, 1, 3, 0, 0, 1030, 0, 0, 5, 0, 1, 0, 2, 0, 7]
    segs, n = _layout(lengths, gaps, lead=3)
    rows = [(b, c, i % 16) for i, (b, c) in enumerate(segs)]
    assert {b % 4 for b, _, _ in rows} == {0, 1, 2, 3} and {c for _, _, c in rows} == set(range(16))
    assert any(a[0] + a[1] == b[0] and a[2] != b[2] for a, b in zip(rows, rows[1:]))
    return rows, n


def _case_b():
    """n = 4096 * 256 + 13 - past the single-range kernel's grid cap - in three segments: two adjacent, a one-element gap, the third."""
    n = 4096 * 256 + 13
    return [(0, 300001, 0), (300001, 400002, 1), (700004, n - 700004, 2)], n


def _class_rows(k):
    """k classes with differing lr, betas, eps, weight_decay and t0; with step 7 class 5 (t0 = 7) has a count below 1, class 9 is at step 1."""
    rows = []
    for c in range(k):
        t0 = {5: 7, 9: 6}.get(c, c % 4)
        rows.append((1e-3 * (1 + c), 0.9 - 0.02 * c, 0.999 - 0.003 * c, 1e-8 * (1 + 10 * c), 0.0 if c % 3 == 0 else 0.01 * c, 0, t0))
    return rows


def _arenas(rows, n, seed):
    """p, g, m, v (numpy fp32, n elements): random inside the segments (gradients include 0 and 1e-30, v >= 0), NaN / inf bit
    patterns outside."""
    rng = np.random.default_rng(seed)
    p = rng.standard_normal(n).astype(np.float32)
    g = (rng.standard_normal(n) * 0.01).astype(np.float32)
    idx = np.arange(n)
    g[idx % 7 == 0] = 0.0
    g[idx % 7 == 3] = 1e-30
    m = (rng.standard_normal(n) * 0.01).astype(np.float32)
    v = (rng.uniform(0, 1, n) * 1e-4).astype(np.float32)
    inside = np.zeros(n, bool)
    for b, c, _ in rows:
        inside[b:b + c] = True
    fill = GAP_BITS[idx % 4].view(np.float32)
    for a in (p, g, m, v):
        a[~inside] = fill[~inside]
    return p, g, m, v, inside


def _dev(a, shift=0):
    """Device copy; shift: elements the data sits behind a 16-byte boundary (the arenas of a real model are aligned, a caller's need not be)."""
    t = torch.zeros(a.size + 4, dtype=torch.float32, device=DEV)
    out = t[shift:shift + a.size]
    out.copy_(torch.from_numpy(a.copy()))
    return out


def _table(lib, rows, n, nclasses):
    L = lib.lib()
    segs = (lib.AdamSegment * len(rows))(*(lib.AdamSegment(*r) for r in rows))
    table = torch.zeros((L.dmm_adam_table_bytes(len(rows), n) + 7) // 8, dtype=torch.int64, device=DEV)
    lib.check(L.dmm_adam_table_init(table.data_ptr(), segs, len(rows), n, nclasses, lib.stream_ptr()))
    return table


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ 1. bit equality
@pytest.mark.parametrize("case,shift", [("A", 0), ("A", 1), ("B", 0)])
def test_segmented_launch_is_bit_equal_to_the_single_range_kernel_per_segment(case, shift):
    """shift = 1: arenas one element behind a 16-byte boundary - the launch then goes element by element throughout and must still agree."""
    from dmmfods_amd import _lib
    L = _lib.lib()
    rows, n = _case_a() if case == "A" else _case_b()
    ncls = 16 if case == "A" else 3
    classes = _class_rows(ncls)
    step, gs = 7, 1.0 / 1024
    p0, g0, m0, v0, inside = _arenas(rows, n, seed=len(rows))
    # the reference: the whole-range form, once per segment, on offset pointers
    P, G, M, V = (_dev(a, shift) for a in (p0, g0, m0, v0))
    written = 0
    for b, c, k in rows:
        lr, b1, b2, eps, wd, _, t0 = classes[k]
        if step - t0 < 1:
            continue
        written += c
        _lib.check(L.dmm_adam_step(P.data_ptr() + 4 * b, G.data_ptr() + 4 * b, M.data_ptr() + 4 * b, V.data_ptr() + 4 * b, c, lr, b1, b2, eps, wd,
                                   step - t0, gs, _lib.stream_ptr()))
    # the segmented launch
    P2, G2, M2, V2 = (_dev(a, shift) for a in (p0, g0, m0, v0))
    table = _table(_lib, rows, n, ncls)
    cl = (_lib.AdamClass * ncls)(*(_lib.AdamClass(*r) for r in classes))
    _lib.check(L.dmm_adam_step_segmented(P2.data_ptr(), G2.data_ptr(), M2.data_ptr(), V2.data_ptr(), n, table.data_ptr(), len(rows), cl, ncls, step, gs,
                                         _lib.stream_ptr()))
    torch.cuda.synchronize()
    for name, got, want, start in (("p", P2, P, p0), ("m", M2, M, m0), ("v", V2, V, v0)):
        gb, wb = _bits(got), _bits(want)
        bad = torch.nonzero(gb != wb).flatten()
        assert bad.numel() == 0, (case, shift, name, bad[:8].tolist(), got.cpu()[bad[:4]].tolist(), want.cpu()[bad[:4]].tolist())
        sb = torch.from_numpy(start.view(np.int32))
        out = torch.from_numpy(~inside)
        assert torch.equal(gb[out], sb[out]), (case, name, "an element in no segment was written")
        moved = int((gb != sb).sum())
        assert 0.9 * written <= moved <= written, (case, name, moved, written)       # the launch did something, and only inside active segments
    assert torch.equal(_bits(G2), torch.from_numpy(g0.view(np.int32))), "the gradient arena was written"
    _golden(f"segments {case} shift {shift}", (p0, g0, m0, v0), P2, M2, V2)
    if case == "A":                                                                 # the class whose count is below 1 wrote nothing
        sleeping = [(b, c) for b, c, k in rows if step - classes[k][6] < 1]
        assert sleeping
        for b, c in sleeping:
            assert np.array_equal(P2.cpu().numpy()[b:b + c].view(np.int32), p0[b:b + c].view(np.int32))
    print(f"[groups] case {case} shift {shift}: n {n}, {len(rows)} segments, {ncls} classes, {written} elements stepped, bit-equal in p, m, v")


# ------------------------------------------------------------------------------------------------ 2. decoupled decay
def test_decoupled_decay_every_element_against_fp64():
    """Four decoupled classes (wd 0.01 / 0.1 x lr 1e-3 / 1e-4) in four segments of 65 537 elements with gaps, one launch per
    (grad_scale, step) in {1, 1/1024} x {1, 2, 1000}.  Reference, fp64: p_ref = p0 (1 - lr wd) + u_ref with lr, wd the fp32 values,
    u_ref = -(lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps), the gradient without a weight_decay * p term."""
    from dmmfods_amd import _lib
    L = _lib.lib()
    b1, b2, eps = np.float32(0.9), np.float32(0.999), np.float32(1e-8)
    combos = [(wd, lr) for wd in (0.01, 0.1) for lr in (1e-3, 1e-4)]
    segs, n = _layout([65537] * 4, [3, 0, 1026, 2], lead=1)
    rows = [(b, c, k) for k, (b, c) in enumerate(segs)]
    table = _table(_lib, rows, n, 4)
    rng = np.random.default_rng(5)
    worst = dict(p=0.0, m=0.0, v=0.0)
    for gs in (1.0, 1.0 / 1024):
        for step in (1, 2, 1000):
            p0, g0, _, _, inside = _arenas(rows, n, seed=step)
            ge = g0.astype(np.float64) * gs                                   # no weight_decay * p term
            ge[~inside] = 0.0
            m0 = np.zeros(n, np.float32) if step == 1 else (ge * rng.uniform(0.5, 1.5, n)).astype(np.float32)
            v0 = np.zeros(n, np.float32) if step == 1 else (ge * ge * rng.uniform(0.5, 1.5, n)).astype(np.float32)
            P, G, M, V = (_dev(a) for a in (p0, g0, m0, v0))
            cl = (_lib.AdamClass * 4)(*(_lib.AdamClass(lr, float(b1), float(b2), float(eps), wd, 1, 0) for wd, lr in combos))
            _lib.check(L.dmm_adam_step_segmented(P.data_ptr(), G.data_ptr(), M.data_ptr(), V.data_ptr(), n, table.data_ptr(), 4, cl, 4, step, gs, _lib.stream_ptr()))
            torch.cuda.synchronize()
            gp, gm, gv = (t.cpu().numpy().astype(np.float64) for t in (P, M, V))
            for (b, c, k) in rows:
                wd, lr = (float(np.float32(x)) for x in combos[k])
                s = slice(b, b + c)
                m = float(b1) * m0[s].astype(np.float64) + (1 - float(b1)) * ge[s]
                v = float(b2) * v0[s].astype(np.float64) + (1 - float(b2)) * ge[s] * ge[s]
                bc1, bc2 = 1 - float(b1) ** step, 1 - float(b2) ** step
                u = -(lr / bc1) * m / (np.sqrt(v) / np.sqrt(bc2) + float(eps))
                p_ref = p0[s].astype(np.float64) * (1.0 - lr * wd) + u
                tiny = 2.0 ** -149
                where = f"wd {wd} lr {lr} grad_scale {gs} step {step}"
                bm, bv = 2.0 ** -21 * np.abs(m) + tiny, 2.0 ** -21 * np.abs(v) + tiny
                bp = 2.0 ** -20 * np.abs(u) + 3 * np.spacing(np.abs(p0[s])).astype(np.float64)
                em, ev, ep = np.abs(gm[s] - m), np.abs(gv[s] - v), np.abs(gp[s] - p_ref)
                worst = dict(p=max(worst["p"], float((ep / bp).max())), m=max(worst["m"], float((em / bm).max())), v=max(worst["v"], float((ev / bv).max())))
                assert not (em > bm).any(), (where, "m", np.flatnonzero(em > bm)[:4])
                assert not (ev > bv).any(), (where, "v", np.flatnonzero(ev > bv)[:4])
                assert not (ep > bp).any(), (where, "p", np.flatnonzero(ep > bp)[:4], gp[s][ep > bp][:4], p_ref[ep > bp][:4])
                assert float(np.abs(gp[s] - p0[s]).max()) > 0
            out = torch.from_numpy(~inside)
            for got, start in ((P, p0), (M, m0), (V, v0), (G, g0)):
                assert torch.equal(_bits(got)[out], torch.from_numpy(start.view(np.int32))[out])
            assert torch.equal(_bits(G), torch.from_numpy(g0.view(np.int32)))
    print(f"[groups] decoupled decay: largest error / bound over every element: p {worst['p']:.3f}, m {worst['m']:.3f}, v {worst['v']:.3f}")


# ------------------------------------------------------------------------------------------------ 3. guarded
def _state(lib, scale, applied):
    s = torch.zeros(16, dtype=torch.int32, device=DEV)
    lib.check(lib.lib().dmm_guard_state_init(s.data_ptr(), scale, applied, 0, lib.stream_ptr()))
    return s


def _read(lib, s):
    torch.cuda.synchronize()
    return lib.GuardState.from_buffer_copy(s.cpu().numpy().tobytes())


def _guarded_step(lib, arenas, n, rows, classes, tail, st, scratch):
    """One guarded step under the table of `rows` (one class per step origin).  (The recording of tests/golden/adam_bits_sha256.json
    put the parent's guarded step over ranges here: one range per run, the run's origin as its t0.)"""
    table = _table(lib, rows, n, len(classes))
    cl = (lib.AdamClass * len(classes))(*(lib.AdamClass(*r) for r in classes))
    lib.check(lib.lib().dmm_adam_step_guarded_segmented(*(t.data_ptr() for t in arenas), n, table.data_ptr(), len(rows), cl, len(classes), *tail,
                                                        st.data_ptr(), scratch.data_ptr(), lib.stream_ptr()))


@pytest.mark.parametrize("origins", [(0, 0, 0), (0, 2, 0)])
def test_guarded_segmented_step_is_bit_equal_to_the_guarded_step_over_ranges(origins):
    """Three runs separated by gaps (the middle one made of two adjacent segments), one set of hyper-parameters; origins: the step
    origin of each run (all 0: one class; (0, 2, 0): the middle run released at applied step 2, a class of its own).  The state starts
    at 5 applied steps and a scale of 8; max_norm is below the norm, so the step is clipped.  The guarded step over ranges is the
    parent's, by its recorded bits: p, m, v and the whole state block (sumsq, grad_norm, clip_coef, grad_scale, scale, the counters,
    step_size and bc2_sqrt as the finalize kernel leaves them: class 0's)."""
    from dmmfods_amd import _lib
    L = _lib.lib()
    lr, b1, b2, eps, wd = 2e-3, 0.9, 0.999, 1e-8, 0.01
    n = 84200
    split = 1013 + 30003
    cls_of = {t0: k for k, t0 in enumerate(dict.fromkeys(origins))}
    rows = [(5, 1000, cls_of[origins[0]]), (1013, 30003, cls_of[origins[1]]), (split, 70001 - 30003, cls_of[origins[1]]), (80000, 4099, cls_of[origins[2]])]
    classes = [(lr, b1, b2, eps, wd, 0, t0) for t0 in cls_of]
    p0, g0, m0, v0, inside = _arenas(rows, n, seed=3)
    g0 = (g0 * 8.0).astype(np.float32)                                            # the arena holds S x the gradients
    g0[~inside] = GAP_BITS[np.arange(n) % 4].view(np.float32)[~inside]
    scratch = torch.zeros(L.dmm_grad_guard_scratch_bytes(n) // 8, dtype=torch.float64, device=DEV)
    tail = (0.05, 2.0, 0.5, 2000)                                                 # max_norm, growth, backoff, interval

    def segmented(g, raw=False):
        P, G, M, V = (_dev(a) for a in (p0, g, m0, v0))
        st = _state(_lib, 8.0, 5)
        _guarded_step(_lib, (P, G, M, V), n, rows, classes, tail, st, scratch)
        return P, G, M, V, (st if raw else _read(_lib, st))

    got = segmented(g0, raw=True)
    sg = _read(_lib, got[4])
    _golden("guarded origins %d %d %d" % origins, (p0, g0, m0, v0), got[0], got[2], got[3], state=got[4])
    assert torch.equal(_bits(got[1]), torch.from_numpy(g0.view(np.int32))), "the gradient arena was written"
    assert sg.found_inf == 0 and sg.applied_steps == 6 and sg.skipped_steps == 0
    assert sg.sumsq > 0 and 0 < sg.clip_coef < 1
    assert not torch.equal(_bits(got[0]), torch.from_numpy(p0.view(np.int32)))
    out = torch.from_numpy(~inside)
    for a, start in zip(got[:4], (p0, g0, m0, v0)):
        assert torch.equal(_bits(a)[out], torch.from_numpy(start.view(np.int32))[out])
    print(f"[groups] guarded, origins {origins}: sumsq {sg.sumsq:.6e} grad_norm {sg.grad_norm:.6e} clip_coef {sg.clip_coef:.6e}, all bit-equal")
    # an inf inside a segment: the step is skipped, nothing is written, the scale backs off once
    g_inf = g0.copy()
    g_inf[split + 17] = np.inf
    P, G, M, V, s = segmented(g_inf)
    assert s.found_inf == 1 and s.applied_steps == 5 and s.skipped_steps == 1 and s.scale == 4.0
    for a, start in zip((P, G, M, V), (p0, g_inf, m0, v0)):
        assert torch.equal(_bits(a), torch.from_numpy(start.view(np.int32)))
    # an inf in a gap is not seen (the gaps of g0 hold inf and NaN already; one more, next to a segment's edge)
    g_gap = g0.copy()
    g_gap[1005] = np.inf
    assert not inside[1005] and not inside[1012] and inside[1013]
    P, G, M, V, s = segmented(g_gap)
    assert s.found_inf == 0 and s.applied_steps == 6 and np.float64(s.sumsq).view(np.int64) == np.float64(sg.sumsq).view(np.int64)
    assert torch.equal(_bits(P), _bits(got[0]))


@pytest.mark.parametrize("form", ["plain shift 0", "plain shift 1", "guarded"])
def test_whole_range_steps_keep_the_recorded_bits(form):
    """dmm_adam_step and dmm_adam_step_guarded over a whole range, against the parent's recorded bits.  plain: n = 4096 * 256 + 13,
    aligned and one element behind a 16-byte boundary (the element path), weight decay 0.01 and grad_scale 1 / 1024 at step 7.
    guarded: n = 84 200, 5 applied steps, scale 8, clipped (max_norm 0.05)."""
    from dmmfods_amd import _lib
    L = _lib.lib()
    lr, b1, b2, eps, wd = 2e-3, 0.9, 0.999, 1e-8, 0.01
    n = 84200 if form == "guarded" else 4096 * 256 + 13
    p0, g0, m0, v0, _ = _arenas([(0, n, 0)], n, seed=11)
    state = None
    if form == "guarded":
        g0 = (g0 * 8.0).astype(np.float32)
        P, G, M, V = (_dev(a) for a in (p0, g0, m0, v0))
        state = _state(_lib, 8.0, 5)
        scratch = torch.zeros(L.dmm_grad_guard_scratch_bytes(n) // 8, dtype=torch.float64, device=DEV)
        _lib.check(L.dmm_adam_step_guarded(P.data_ptr(), G.data_ptr(), M.data_ptr(), V.data_ptr(), n, lr, b1, b2, eps, wd, 0.05, 2.0, 0.5, 2000,
                                           state.data_ptr(), scratch.data_ptr(), _lib.stream_ptr()))
        s = _read(_lib, state)
        assert s.found_inf == 0 and s.applied_steps == 6 and 0 < s.clip_coef < 1
    else:
        P, G, M, V = (_dev(a, int(form[-1])) for a in (p0, g0, m0, v0))
        _lib.check(L.dmm_adam_step(P.data_ptr(), G.data_ptr(), M.data_ptr(), V.data_ptr(), n, lr, b1, b2, eps, wd, 7, 1.0 / 1024, _lib.stream_ptr()))
        torch.cuda.synchronize()
    assert torch.equal(_bits(G), torch.from_numpy(g0.view(np.int32))), "the gradient arena was written"
    assert int((_bits(P) != torch.from_numpy(p0.view(np.int32))).sum()) > 0.9 * n
    _golden("whole " + form, (p0, g0, m0, v0), P, M, V, state=state)


# ------------------------------------------------------------------------------------------------ 4. model level
VARIANTS = {"no": (1, 0), "early": (1, 3), "mid3": (3, 3)}


def _arch(R, base, variant):
    cbb, s2 = VARIANTS[variant]
    return R.Arch(**base, concat_before_block_num=cbb, stream_2_in_channels=s2)


def _model(R, arch, dtype="fp32", seed=123):
    from dmmfods_amd.graphs.models.Dense_U_Net_lidar import Dense_U_Net_lidar
    cfg = get_config("/tmp/dmm_test")
    cfg.model.growth_rate, cfg.model.block_config, cfg.model.num_init_features = arch.growth_rate, arch.block_config, arch.num_init_features
    cfg.model.concat_before_block_num, cfg.model.stream_2_in_channels = arch.concat_before_block_num, arch.stream_2_in_channels
    model = Dense_U_Net_lidar(cfg, compute_dtype=dtype)
    model.load_state_dict(R.make_state(arch, seed=seed))
    return model.to(DEV).train()


def _fused(model, batch):
    rgb, lidar, tgt = batch
    with torch.no_grad():
        model(rgb, lidar)
    return model.loss_backward(tgt)


def _rel_l2(pairs):
    num = sum(float((a.detach().cpu().double() - b.detach().double()).pow(2).sum()) for a, b in pairs)
    den = sum(float(b.detach().double().pow(2).sum()) for _, b in pairs)
    return (num / den) ** 0.5


def _compare_step(R, arch, P, leaves, ref_opt, model, opt, cpu_batch, step, tag):
    """One optimiser step on both sides; tests/test_freeze_gpu.py's _compare_step: loss sums rtol 2e-3, weights (the encoder alone as
    well) and running statistics 5e-3 relative L2."""
    rgb, lidar, tgt = cpu_batch
    ref_opt.zero_grad()
    loss = R.bce_with_logits(R.forward(P, arch, rgb, lidar, training=True), tgt)
    loss.backward(torch.ones_like(loss))
    ref_opt.step()
    met = _fused(model, (rgb.to(DEV), lidar.to(DEV), tgt.to(DEV)))
    opt.step()
    torch.testing.assert_close(met["loss_per_class"].cpu().double(), loss.detach().double().sum(dim=(0, 2, 3)), rtol=2e-3, atol=0)
    sd = model.state_dict()
    e_w = _rel_l2([(sd[k], t) for k, t in leaves])
    e_enc = _rel_l2([(sd[k], t) for k, t in leaves if k.startswith(ENCODER)])
    e_s = _rel_l2([(sd[k], P[k]) for k in sd if k.endswith(("running_mean", "running_var"))])
    print(f"[groups] {tag} step {step}: weights rel L2 {e_w:.3e} (encoder alone {e_enc:.3e}), running statistics rel L2 {e_s:.3e}")
    assert e_w < 5e-3 and e_enc < 5e-3 and e_s < 5e-3, (tag, step, e_w, e_enc, e_s)


def _both_sides(R, arch, decoupled, frozen=False, **fused_kw):
    """The model with FusedAdam over fine_tune_groups(encoder_lr_scale=0.1, no_decay_norm_bias=True, weight_decay=0.01), and the
    oracle restatement's leaves under torch.optim.Adam over the same groups (by name)."""
    from dmmfods_amd.optim import FusedAdam, fine_tune_groups
    P = R.make_state(arch, seed=123)
    leaves = R.leaf_params(P, arch)
    for k, t in leaves:
        t.requires_grad_(not (frozen and k.startswith(ENCODER)))
    model = _model(R, arch)
    if frozen:
        model.freeze_encoder()
    groups = fine_tune_groups(model, 1e-3, 0.01, encoder_lr_scale=0.1, no_decay_norm_bias=True)
    name_of = {id(p): n for n, p in model.named_parameters()}
    leaf = dict(leaves)
    torch_groups = [{"params": [leaf[name_of[id(p)]] for p in g["params"]], "lr": g["lr"], "weight_decay": g["weight_decay"]} for g in groups]
    ref_opt = torch.optim.Adam(torch_groups, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, amsgrad=False, decoupled_weight_decay=decoupled)
    opt = FusedAdam(model, lr=1e-3, weight_decay=0.01, param_groups=groups, decoupled_weight_decay=decoupled, **fused_kw)
    return P, leaves, ref_opt, model, opt


class _Counting:
    """Stands in front of the loaded library and counts the calls of the Adam entry points."""

    def __init__(self, real):
        self._real, self.calls = real, collections.Counter()

    def __getattr__(self, name):
        f = getattr(self._real, name)
        if not name.startswith("dmm_adam"):
            return f

        def counted(*a):
            self.calls[name] += 1
            return f(*a)
        return counted


@pytest.mark.parametrize("decoupled", [False, True])
def test_three_grouped_steps_against_torch_adam_over_the_same_groups(decoupled, monkeypatch):
    from oracle import restatement as R
    from dmmfods_amd import _lib
    arch = _arch(R, TINY, "mid3")
    P, leaves, ref_opt, model, opt = _both_sides(R, arch, decoupled)
    assert len(opt.param_groups) == 4 and len(opt.segments()) > 8
    counter = _Counting(_lib.lib())
    monkeypatch.setattr(_lib, "_lib", counter)
    enc0 = {k: t.detach().clone() for k, t in leaves if k.startswith(ENCODER)}
    for step in range(3):
        _compare_step(R, arch, P, leaves, ref_opt, model, opt, R.make_inputs(arch, 2, 64, 96, seed=step), step + 1, f"decoupled {decoupled}")
    # one table for the run, one Adam entry point - one launch - per step
    assert dict(counter.calls) == {"dmm_adam_table_init": 1, "dmm_adam_table_bytes": 1, "dmm_adam_step_segmented": 3}, dict(counter.calls)
    # the groups did act: the encoder moved by a tenth of what the decoder's lr would have moved it
    sd = model.state_dict()
    moved = torch.cat([(sd[k].cpu() - enc0[k]).abs().flatten() for k in enc0])
    # (an Adam step is at most (1 - b1) / sqrt(1 - b2) = 3.2 lr and lr on the first: under the decoder's lr the median would be near 3e-3)
    assert 0 < float(moved.median()) <= 3 * 1e-4 * 1.01 and float(moved.max()) < 1e-3, (float(moved.median()), float(moved.max()))
    assert opt.step_count == 3
    # without groups and with nothing frozen: the whole-arena call, one per step
    counter.calls.clear()
    from dmmfods_amd.optim import FusedAdam
    plain = FusedAdam(model, weight_decay=0.01)
    _fused(model, tuple(t.to(DEV) for t in R.make_inputs(arch, 2, 64, 96, seed=0)))
    plain.step()
    clip = FusedAdam(model, weight_decay=0.01, max_grad_norm=1e9)
    clip.step()
    torch.cuda.synchronize()
    assert dict(counter.calls) == {"dmm_adam_step": 1, "dmm_adam_step_guarded": 1}, dict(counter.calls)
    # without groups, the encoder frozen: the segmented call, one per step (one table each, built at the first step)
    counter.calls.clear()
    model.freeze_encoder()
    plain, clip = FusedAdam(model, weight_decay=0.01), FusedAdam(model, weight_decay=0.01, max_grad_norm=1e9)
    _fused(model, tuple(t.to(DEV) for t in R.make_inputs(arch, 2, 64, 96, seed=0)))
    for _ in range(2):
        plain.step()
        clip.step()
    torch.cuda.synchronize()
    assert dict(counter.calls) == {"dmm_adam_table_init": 2, "dmm_adam_table_bytes": 2, "dmm_adam_step_segmented": 2,
                                   "dmm_adam_step_guarded_segmented": 2}, dict(counter.calls)
    model.close()


def test_released_encoder_starts_at_its_own_step_one_with_its_own_lr_on_the_guarded_path(monkeypatch):
    """Two frozen steps, release, two more (tests/test_freeze_gpu.py's check, with groups and the guarded path): behind the first released
    step at least 90 % of the encoder's elements have moved by the ENCODER group's lr, 0.1 x 1e-3, to within 1 %."""
    from oracle import restatement as R
    from dmmfods_amd import _lib
    arch = _arch(R, TINY, "mid3")
    P, leaves, ref_opt, model, opt = _both_sides(R, arch, False, frozen=True, max_grad_norm=1e9)
    counter = _Counting(_lib.lib())
    monkeypatch.setattr(_lib, "_lib", counter)
    enc = torch.zeros(model.param_arena.numel(), dtype=torch.bool, device=DEV)
    off = 0
    for name, p in model.named_parameters():
        if name.startswith(ENCODER):
            enc[off:off + p.numel()] = True
        off += p.numel()
    assert {gi for _, _, gi, _ in opt.segments()} == {0, 1}                                 # frozen: the encoder's groups have no segment
    for step in range(4):
        if step == 2:
            for k, t in leaves:
                t.requires_grad_(True)
            model.freeze_encoder(False)
        before = model.param_arena.clone()
        _compare_step(R, arch, P, leaves, ref_opt, model, opt, R.make_inputs(arch, 2, 64, 96, seed=step), step + 1, "release")
        moved = (model.param_arena - before).abs()
        if step < 2:
            assert float(moved[enc].max()) == 0.0
        if step == 2:
            ratio = moved[enc].double() / 1e-4
            near = float(((ratio - 1.0).abs() < 0.01).double().mean())
            print(f"[groups] guarded: first released step, |dp| / (0.1 lr) over the encoder: median {float(ratio.median()):.4f}, within 1 % of 1: {near:.4f}")
            assert near >= 0.9, (near, float(ratio.median()))
    assert opt.step_count == 4 and int(opt.last_found_inf) == 0
    assert {(gi, t0) for _, _, gi, t0 in opt.segments()} == {(0, 0), (1, 0), (2, 2), (3, 2)}
    steps = {float(s["step"]) for s in opt.state_dict()["state"].values()}
    assert steps == {2.0, 4.0}
    # the table was rebuilt once, at the release; every step was one guarded segmented call
    assert counter.calls["dmm_adam_table_init"] == 2 and counter.calls["dmm_adam_step_guarded_segmented"] == 4
    assert set(counter.calls) == {"dmm_adam_table_init", "dmm_adam_table_bytes", "dmm_adam_step_guarded_segmented"}, dict(counter.calls)
    model.close()


# ------------------------------------------------------------------------------------------------ 5. the agent
class _Loader:
    def __init__(self, batches):
        self.train_loader, self.train_iterations = batches, len(batches)
        self.valid_loader, self.valid_iterations = [], 0


def _agent(tmp_path, monkeypatch, batches, resume=False):
    from dmmfods_amd.agents import Dense_U_Net_lidar_Agent as mod
    from dmmfods_amd.graphs.models.Dense_U_Net_lidar import Dense_U_Net_lidar
    cfg = get_config(str(tmp_path))
    cfg.dir.current_run.summary = str(tmp_path / "run" / "summary")
    cfg.dir.current_run.checkpoints = str(tmp_path / "run" / "checkpoints")
    cfg.model.concat_before_block_num, cfg.model.stream_2_in_channels = 3, 3
    cfg.optimizer.weight_decay = 0.01
    cfg.optimizer.encoder_lr_scale = 0.1
    cfg.optimizer.no_decay_norm_bias = True
    cfg.optimizer.decoupled_weight_decay = True
    cfg.optimizer.lr_scheduler.want, cfg.optimizer.lr_scheduler.every_n_epochs, cfg.optimizer.lr_scheduler.gamma = True, 1, 0.5

    def factory(pretrained=False, config=None, compute_dtype=None, **kw):
        config.model.growth_rate, config.model.block_config, config.model.num_init_features = 8, (2, 2, 2, 2), 16
        return Dense_U_Net_lidar(config, compute_dtype=compute_dtype)
    monkeypatch.setattr(mod, "densenet121_u_lidar", factory)
    return mod.Dense_U_Net_lidar_Agent(cfg, torchvision_init=not resume, compute_dtype="fp32", data_loader=_Loader(batches))


def test_agent_trains_with_groups_and_a_resume_keeps_them(tmp_path, monkeypatch):
    """Two epochs of two batches with optimizer.encoder_lr_scale / no_decay_norm_bias / decoupled_weight_decay and StepLR(1, 0.5): the
    group learning rates after each epoch and the checkpoint's param_groups are those of torch.optim.Adam over the same groups under
    torch's StepLR; a fresh agent that loads the checkpoint has the groups, the steps and the moments, and trains on."""
    from oracle import restatement as R
    from dmmfods_amd.optim import fine_tune_groups
    arch = _arch(R, TINY, "mid3")
    batches = [R.make_inputs(arch, 2, 64, 96, seed=s) for s in range(2)]
    agent = _agent(tmp_path / "a", monkeypatch, batches)
    agent.model.load_state_dict(R.make_state(arch, seed=99))
    opt = agent.optimizer
    assert opt._grouped and len(opt.param_groups) == 4 and all(g["decoupled_weight_decay"] for g in opt.param_groups)
    lr0 = agent.config.optimizer.learning_rate
    assert [(g["lr"], g["weight_decay"]) for g in opt.param_groups] == [(lr0, 0.01), (lr0, 0.0), (lr0 * 0.1, 0.01), (lr0 * 0.1, 0.0)]
    # torch's side of the bookkeeping (no gradients needed: StepLR and the state dict's groups)
    o = agent.config.optimizer
    ref = torch.optim.Adam(fine_tune_groups(agent.model, lr0, 0.01, 0.1, True), lr=lr0, betas=(o.beta1, o.beta2), eps=o.eps, weight_decay=0.01,
                           decoupled_weight_decay=True)
    sched = torch.optim.lr_scheduler.StepLR(ref, step_size=1, gamma=0.5)
    p0 = agent.model.param_arena.clone()
    for epoch in range(2):
        agent.current_epoch = epoch
        agent.train_one_epoch()
        ref.step()
        sched.step()
        assert [g["lr"] for g in opt.param_groups] == pytest.approx([g["lr"] for g in ref.param_groups], rel=1e-12), epoch
    assert opt.step_count == 4 and bool(torch.isfinite(agent.model.param_arena).all()) and not torch.equal(agent.model.param_arena, p0)
    assert all(bool(torch.isfinite(h["loss"]).all()) for h in agent.train_history)
    agent.save_checkpoint(is_best=True)
    ck_dir = agent.config.dir.current_run.checkpoints
    ck = torch.load(os.path.join(ck_dir, agent.config.agent.best_checkpoint_name), map_location="cpu")
    keys = ("lr", "betas", "eps", "weight_decay", "amsgrad", "decoupled_weight_decay", "maximize", "foreach", "capturable", "differentiable", "fused", "params")
    theirs = ref.state_dict()["param_groups"]
    assert len(ck["optimizer"]["param_groups"]) == 4
    for mine, want in zip(ck["optimizer"]["param_groups"], theirs):
        assert {k: mine[k] for k in keys if k != "lr"} == {k: want[k] for k in keys if k != "lr"}
        assert mine["lr"] == pytest.approx(want["lr"], rel=1e-12)
    assert sorted(ck["optimizer"]["state"]) == list(range(len(list(agent.model.parameters()))))
    ref.load_state_dict({"state": ck["optimizer"]["state"], "param_groups": ck["optimizer"]["param_groups"]})   # torch takes the checkpoint
    m_sum = float(opt.exp_avg.abs().sum())
    agent.model.close()
    # resume
    os.makedirs(str(tmp_path / "b" / "run" / "checkpoints"), exist_ok=True)
    shutil.copy(os.path.join(ck_dir, agent.config.agent.best_checkpoint_name), str(tmp_path / "b" / "run" / "checkpoints" / agent.config.agent.best_checkpoint_name))
    resumed = _agent(tmp_path / "b", monkeypatch, batches, resume=True)
    ropt = resumed.optimizer
    assert ropt._grouped and ropt.step_count == 4 and ropt.segments() == opt.segments()
    assert [g["lr"] for g in ropt.param_groups] == [g["lr"] for g in ck["optimizer"]["param_groups"]]
    assert [g["params"] for g in ropt.param_groups] == [g["params"] for g in ck["optimizer"]["param_groups"]]
    assert float(ropt.exp_avg.abs().sum()) == pytest.approx(m_sum, rel=1e-6)
    assert torch.equal(resumed.model.param_arena.cpu(), agent.model.param_arena.cpu())
    resumed.train_one_epoch()
    assert ropt.step_count == 6 and bool(torch.isfinite(resumed.model.param_arena).all())
    print(f"[groups] agent: lrs after two epochs {[g['lr'] for g in opt.param_groups]}, resumed epoch losses {resumed.train_history[-1]['loss'].tolist()}")
    resumed.model.close()


def record(commit):
    """Runs the cases that _golden pins against the loaded library (DMM_LIB_PATH) and writes the golden file, which names `commit`."""
    global _RECORDING
    _RECORDING = {}
    for case, shift in (("A", 0), ("A", 1), ("B", 0)):
        test_segmented_launch_is_bit_equal_to_the_single_range_kernel_per_segment(case, shift)
    for origins in ((0, 0, 0), (0, 2, 0)):
        test_guarded_segmented_step_is_bit_equal_to_the_guarded_step_over_ranges(origins)
    for form in ("plain shift 0", "plain shift 1", "guarded"):
        test_whole_range_steps_keep_the_recorded_bits(form)
    with open(GOLDEN, "w") as f:
        json.dump({"commit": commit, "cases": _RECORDING}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s (%d cases, library of %s)" % (GOLDEN, len(_RECORDING), commit))


if __name__ == "__main__":   # DMM_LIB_PATH=<library built from <commit>'s csrc> python tests/test_param_groups_gpu.py <commit>
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    record(sys.argv[1])
