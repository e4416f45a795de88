"""The parameter average on the GPU: the Adam kernel's `ema` arena (dmm_adam_step_segmented_ema, dmm_adam_step_guarded_segmented_ema) and
what stands on it (FusedAdam(ema_decay=...), ema_weights(), the agent's config fields).

  1. ADAM'S BITS DO NOT MOVE: p, m and v of the launch with an average are bit-equal to those of the launch without, on copies of the
     same inputs (the layout of tests/test_param_groups_gpu.py's case A: 18 segments, every begin residue mod 4, gaps, 16 classes, one
     of them asleep), aligned and one element behind a 16-byte boundary.  No tolerance.
  2. THE AVERAGE, every element, one step.  With p1 the kernel's own new parameter, e0 the average it read and omd the fp32 factor of
     the schedule, r = e0 + omd (p1 - e0) in fp64.  The kernel rounds twice, d = fl(p1 - e0) and e1 = fl(fma(omd, d, e0)), each by at
     most 2^-24 relative, so |e1 - r| <= 2^-24 (omd |p1 - e0| + |r|) to first order; the bound is twice that:
         |e1 - r| <= 2^-23 (omd |p1 - e0| + |r|).
     Derived, not measured.  In a gap and in the sleeping class e keeps its bits (NaN and inf patterns in the gaps).
  3. Past the grid cap (two chunks per workgroup and a ragged tail), also with only `ema` off alignment: the element path throughout.
  4. Guarded: bit-equal p, m, v and state block; k formed on the device; a skipped step writes nothing and is no averaging update.
  5. Model level: three steps against the fp64 chain of lerps over snapshots of the parameters; frozen ranges keep e == p.
  6. ema_weights(): the exchange, the model's answer on the other weights, the guards.
  7. The agent with optimizer.ema_decay and a resume, also from a checkpoint written without an average.
Every case prints its figures ([ema] lines)."""
import os
import shutil

import numpy as np
import pytest
import torch

from dmmfods_amd.utils.Dense_U_Net_lidar_helper import get_config

pytestmark = pytest.mark.gpu

DEV = "cuda"
ENCODER = ("features.", "stream_2_features.", "concat_module.")
TINY = dict(growth_rate=8, block_config=(2, 2, 2, 2), num_init_features=16)
GAP_BITS = np.array([0x7fc00001, 0x7f800000, 0xff800000, 0xffc12345], dtype=np.uint32)   # NaN, +inf, -inf, NaN with a payload
STEP, GRAD_SCALE = 7, 1.0 / 1024
SCHEDULES = {"warm k=1": (0.999, 1, 1), "flat k=5000": (0.999, 0, 5000)}                 # decay, warm-up, k


def _omd(decay, warmup, k):
    """(float)(1 - d_k), d_k in double from the fp32 decay the ABI carries."""
    d = float(np.float32(decay))
    if warmup:
        d = min(d, (1.0 + k) / (10.0 + k))
    return float(np.float32(1.0 - d))


# ------------------------------------------------------------------------------------------------ layouts and arenas
def _layout(lengths, gaps, lead):
    segs, pos = [], lead
    for ln, gap in zip(lengths, gaps):
        segs.append((pos, ln))
        pos += ln + gap
    return segs, pos


def _case_a():
    """Lengths 1 .. 70 001 (69 chunks), begins at every residue mod 4, gaps in front, between and behind, all 16 classes."""
    lengths = [1, 2, 3, 5, 255, 257, 70001, 1, 2, 3, 5, 255, 257, 4, 1024, 2049, 9, 6]
    gaps = [0, 0, 2, 0, 1, 3, 0, 0, 1030, 0, 0, 5, 0, 1, 0, 2, 0, 7]
    segs, n = _layout(lengths, gaps, lead=3)
    rows = [(b, c, i % 16) for i, (b, c) in enumerate(segs)]
    assert {b % 4 for b, _, _ in rows} == {0, 1, 2, 3} and {c for _, _, c in rows} == set(range(16))
    return rows, n


def _case_cap():
    """One segment over n = 2 * 2048 * 1024 + 13: with the grid capped at 2048 workgroups every one walks two chunks, then the tail."""
    n = 2 * 2048 * 1024 + 13
    return [(0, n, 0)], n


def _class_rows(k):
    """k classes with differing lr, betas, eps, weight_decay and t0; at step 7 class 5 (t0 = 7) is asleep, class 9 at its step 1."""
    rows = []
    for c in range(k):
        t0 = {5: 7, 9: 6}.get(c, c % 4)
        rows.append((1e-3 * (1 + c), 0.9 - 0.02 * c, 0.999 - 0.003 * c, 1e-8 * (1 + 10 * c), 0.0 if c % 3 == 0 else 0.01 * c, 0, t0))
    return rows


def _arenas(rows, n, seed):
    """p, g, m, v, e (numpy fp32): random inside the segments, NaN / inf bit patterns outside; and the mask of the segments."""
    rng = np.random.default_rng(seed)
    p = rng.standard_normal(n).astype(np.float32)
    g = (rng.standard_normal(n) * 0.01).astype(np.float32)
    idx = np.arange(n)
    g[idx % 7 == 0] = 0.0
    g[idx % 7 == 3] = 1e-30
    m = (rng.standard_normal(n) * 0.01).astype(np.float32)
    v = (rng.uniform(0, 1, n) * 1e-4).astype(np.float32)
    e = rng.standard_normal(n).astype(np.float32)
    inside = np.zeros(n, bool)
    for b, c, _ in rows:
        inside[b:b + c] = True
    fill = GAP_BITS[idx % 4].view(np.float32)
    for a in (p, g, m, v, e):
        a[~inside] = fill[~inside]
    return p, g, m, v, e, inside


def _dev(a, shift=0):
    """Device copy; shift: elements the data sits behind a 16-byte boundary."""
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
    a = t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
    return a.view(np.int32)


def _same_bits(got, want, what):
    bad = np.flatnonzero(_bits(got) != _bits(want))
    assert bad.size == 0, (what, bad.size, bad[:8].tolist())


def _check_average(e1, e0, p1, omd, written, what):
    """Bound 2 on the written elements, untouched bits elsewhere; returns the largest error / bound."""
    e1 = e1.detach().cpu().numpy() if isinstance(e1, torch.Tensor) else e1
    p1 = p1.detach().cpu().numpy() if isinstance(p1, torch.Tensor) else p1
    keep = ~written
    bad = np.flatnonzero(_bits(e1)[keep] != _bits(e0)[keep])
    assert bad.size == 0, (what, "an average outside the written set was touched", bad.size, bad[:8].tolist())
    pw, ew, gw = p1[written].astype(np.float64), e0[written].astype(np.float64), e1[written].astype(np.float64)
    r = ew + omd * (pw - ew)
    bound = 2.0 ** -23 * (omd * np.abs(pw - ew) + np.abs(r))
    err = np.abs(gw - r)
    over = np.flatnonzero(err > bound)
    assert over.size == 0, (what, over.size, over[:4].tolist(), gw[over[:4]].tolist(), r[over[:4]].tolist())
    assert int((_bits(e1)[written] != _bits(e0)[written]).sum()) > 0.9 * written.sum(), (what, "the average did not move")
    return float((err / np.maximum(bound, 2.0 ** -149)).max())


_RUNS = {}


def _plain_runs(case, shift, ema_shift):
    """Inputs, the launch without an average, and one launch with it per schedule - made once, shared by cases 1 to 3."""
    key = (case, shift, ema_shift)
    if key in _RUNS:
        return _RUNS[key]
    from dmmfods_amd import _lib
    L = _lib.lib()
    rows, n = _case_a() if case == "A" else _case_cap()
    ncls = 16 if case == "A" else 1
    classes = _class_rows(ncls)
    p0, g0, m0, v0, e0, inside = _arenas(rows, n, seed=len(rows) + 40)
    table = _table(_lib, rows, n, ncls)
    cl = (_lib.AdamClass * ncls)(*(_lib.AdamClass(*r) for r in classes))
    P, G, M, V = (_dev(a, shift) for a in (p0, g0, m0, v0))
    _lib.check(L.dmm_adam_step_segmented(P.data_ptr(), G.data_ptr(), M.data_ptr(), V.data_ptr(), n, table.data_ptr(), len(rows), cl, ncls, STEP, GRAD_SCALE,
                                         _lib.stream_ptr()))
    torch.cuda.synchronize()
    written = np.zeros(n, bool)
    for b, c, k in rows:
        if STEP - classes[k][6] >= 1:
            written[b:b + c] = True
    out = dict(n=n, rows=rows, inputs=(p0, g0, m0, v0, e0), inside=inside, written=written, off=tuple(t.cpu().numpy() for t in (P, G, M, V)), on={})
    for name, (decay, warmup, k) in SCHEDULES.items():
        P, G, M, V = (_dev(a, shift) for a in (p0, g0, m0, v0))
        E = _dev(e0, ema_shift)
        ema = _lib.AdamEma(E.data_ptr(), decay, warmup, k)
        _lib.check(L.dmm_adam_step_segmented_ema(P.data_ptr(), G.data_ptr(), M.data_ptr(), V.data_ptr(), n, table.data_ptr(), len(rows), cl, ncls, STEP, GRAD_SCALE,
                                                 _lib.stream_ptr(), ema))
        torch.cuda.synchronize()
        out["on"][name] = tuple(t.cpu().numpy() for t in (P, G, M, V, E))
    _RUNS[key] = out
    return out


def _check_bits(run, what):
    p0, g0, m0, v0, _ = run["inputs"]
    Po, Go, Mo, Vo = run["off"]
    assert int((_bits(Po) != _bits(p0)).sum()) > 0.9 * run["written"].sum()                 # the launch without an average did step
    _same_bits(Go, g0, (what, "g, average off"))
    for name, (P, G, M, V, _) in run["on"].items():
        for tag, got, want in (("p", P, Po), ("m", M, Mo), ("v", V, Vo)):
            _same_bits(got, want, (what, name, tag))
        _same_bits(G, g0, (what, name, "the gradient arena was written"))


# ------------------------------------------------------------------------------------------------ 1. Adam's bits
@pytest.mark.parametrize("shift", [0, 1])
def test_adams_bits_do_not_move_with_an_average(shift):
    run = _plain_runs("A", shift, shift)
    assert run["written"].sum() < run["inside"].sum() < run["n"]                            # a sleeping class, and gaps
    _check_bits(run, ("A", shift))
    print(f"[ema] case A shift {shift}: n {run['n']}, {int(run['written'].sum())} elements stepped, p, m, v bit-equal with and without an average")


# ------------------------------------------------------------------------------------------------ 2. the average
@pytest.mark.parametrize("schedule", list(SCHEDULES))
@pytest.mark.parametrize("shift", [0, 1])
def test_average_every_element_after_one_step(shift, schedule):
    run = _plain_runs("A", shift, shift)
    omd = _omd(*SCHEDULES[schedule])
    assert omd == float(np.float32(9.0 / 11.0)) if schedule == "warm k=1" else abs(omd - 1e-3) < 1e-7
    P, _, _, _, E = run["on"][schedule]
    worst = _check_average(E, run["inputs"][4], P, omd, run["written"], ("A", shift, schedule))
    print(f"[ema] case A shift {shift} {schedule}: omd {omd!r}, largest error / bound over every written element {worst:.3f}")


# ------------------------------------------------------------------------------------------------ 3. past the grid cap
@pytest.mark.parametrize("ema_shift", [0, 1])
def test_past_the_grid_cap_and_with_only_the_average_off_alignment(ema_shift):
    """ema_shift = 1: p, g, m, v aligned, the average one element behind a 16-byte boundary - no 16-byte access anywhere."""
    run = _plain_runs("cap", 0, ema_shift)
    assert run["n"] == 2 * 2048 * 1024 + 13 and run["written"].all()
    _check_bits(run, ("cap", ema_shift))
    for schedule in SCHEDULES:
        P, _, _, _, E = run["on"][schedule]
        worst = _check_average(E, run["inputs"][4], P, _omd(*SCHEDULES[schedule]), run["written"], ("cap", ema_shift, schedule))
        print(f"[ema] grid cap, average shift {ema_shift}, {schedule}: largest error / bound {worst:.3f}")


# ------------------------------------------------------------------------------------------------ 4. guarded
def _state(lib, scale, applied):
    s = torch.zeros(16, dtype=torch.int32, device=DEV)
    lib.check(lib.lib().dmm_guard_state_init(s.data_ptr(), scale, applied, 0, lib.stream_ptr()))
    return s


def _read(lib, s):
    torch.cuda.synchronize()
    return lib.GuardState.from_buffer_copy(s.cpu().numpy().tobytes())


def test_guarded_step_forms_k_on_the_device_and_a_skipped_step_is_no_update():
    """Three runs separated by gaps, origins (0, 2, 0), 5 applied steps, scale 8, clipped - the existing guarded test's set-up.
    Averaging began at applied step 5 (ema_t0 = 5), decay 0.999 with warm-up: the step that makes applied_steps 6 is update k = 1,
    omd = (float)(9 / 11).  Then: an inf in a segment - nothing is written, skipped_steps rises - and a clean step on the same
    state: applied_steps is 6 again, so k = 1 and omd = 9 / 11; had the skipped step counted, omd would be 9 / 12."""
    from dmmfods_amd import _lib
    L = _lib.lib()
    lr, b1, b2, eps, wd = 2e-3, 0.9, 0.999, 1e-8, 0.01
    n, split, origins, t0_ema = 84200, 1013 + 30003, (0, 2, 0), 5
    cls_of = {t0: k for k, t0 in enumerate(dict.fromkeys(origins))}
    rows = [(5, 1000, cls_of[origins[0]]), (1013, 30003, cls_of[origins[1]]), (split, 70001 - 30003, cls_of[origins[1]]), (80000, 4099, cls_of[origins[2]])]
    classes = [(lr, b1, b2, eps, wd, 0, t0) for t0 in cls_of]
    p0, g0, m0, v0, e0, inside = _arenas(rows, n, seed=3)
    g0 = (g0 * 8.0).astype(np.float32)
    g0[~inside] = GAP_BITS[np.arange(n) % 4].view(np.float32)[~inside]
    scratch = torch.zeros(L.dmm_grad_guard_scratch_bytes(n) // 8, dtype=torch.float64, device=DEV)
    tail = (0.05, 2.0, 0.5, 2000)
    table = _table(_lib, rows, n, len(classes))
    cl = (_lib.AdamClass * len(classes))(*(_lib.AdamClass(*r) for r in classes))

    def step(arenas, st, E=None):
        args = (*(t.data_ptr() for t in arenas), n, table.data_ptr(), len(rows), cl, len(classes), *tail, st.data_ptr(), scratch.data_ptr(), _lib.stream_ptr())
        if E is None:
            _lib.check(L.dmm_adam_step_guarded_segmented(*args))
        else:
            _lib.check(L.dmm_adam_step_guarded_segmented_ema(*args, _lib.AdamEma(E.data_ptr(), 0.999, 1, t0_ema)))
        torch.cuda.synchronize()

    # without and with an average
    off, st_off = tuple(_dev(a) for a in (p0, g0, m0, v0)), _state(_lib, 8.0, 5)
    step(off, st_off)
    on, st_on, E = tuple(_dev(a) for a in (p0, g0, m0, v0)), _state(_lib, 8.0, 5), _dev(e0)
    step(on, st_on, E)
    for tag, got, want in zip("pgmv", on, off):
        _same_bits(got, want, ("guarded", tag))
    _same_bits(on[1], g0, "the gradient arena was written")
    _same_bits(st_on, st_off, "the 64-byte state block")
    s = _read(_lib, st_on)
    assert s.found_inf == 0 and s.applied_steps == 6 and 0 < s.clip_coef < 1
    k = s.applied_steps - t0_ema
    assert k == 1
    worst = _check_average(E, e0, on[0], _omd(0.999, 1, k), inside, "guarded, k = 1")
    print(f"[ema] guarded: k {k} from the state block, largest error / bound {worst:.3f}; p, m, v and the state block bit-equal")
    # an average that has not begun (ema_t0 = applied_steps after the step: k = 0) is not written, Adam steps all the same
    on0, st0, E0 = tuple(_dev(a) for a in (p0, g0, m0, v0)), _state(_lib, 8.0, 5), _dev(e0)
    args = (*(t.data_ptr() for t in on0), n, table.data_ptr(), len(rows), cl, len(classes), *tail, st0.data_ptr(), scratch.data_ptr(), _lib.stream_ptr())
    _lib.check(L.dmm_adam_step_guarded_segmented_ema(*args, _lib.AdamEma(E0.data_ptr(), 0.999, 1, 6)))
    torch.cuda.synchronize()
    _same_bits(E0, e0, "k = 0 wrote an average")
    _same_bits(on0[0], off[0], "k = 0: p")
    # an inf inside a segment: everything keeps its bits
    g_inf = g0.copy()
    g_inf[split + 17] = np.inf
    sk, st_sk, Esk = tuple(_dev(a) for a in (p0, g_inf, m0, v0)), _state(_lib, 8.0, 5), _dev(e0)
    step(sk, st_sk, Esk)
    s = _read(_lib, st_sk)
    assert s.found_inf == 1 and s.applied_steps == 5 and s.skipped_steps == 1 and s.scale == 4.0
    for tag, got, want in zip("pgmve", sk + (Esk,), (p0, g_inf, m0, v0, e0)):
        _same_bits(got, want, ("skipped step", tag))
    # the next clean step, same state block: the k that follows the last APPLIED step
    sk[1].copy_(torch.from_numpy(g0))
    step(sk, st_sk, Esk)
    s = _read(_lib, st_sk)
    assert s.found_inf == 0 and s.applied_steps == 6 and s.skipped_steps == 1 and s.applied_steps - t0_ema == 1
    worst = _check_average(Esk, e0, sk[0], _omd(0.999, 1, 1), inside, "the clean step behind a skipped one")
    # by value: 9 / 11 and 9 / 12 differ by far more than the bound - the other k's reference is missed nearly everywhere
    pw, ew, gw = (a.astype(np.float64) for a in (sk[0].cpu().numpy()[inside], e0[inside], Esk.cpu().numpy()[inside]))
    wrong = ew + _omd(0.999, 1, 2) * (pw - ew)
    missed = float((np.abs(gw - wrong) > 2.0 ** -23 * (0.75 * np.abs(pw - ew) + np.abs(wrong))).mean())
    assert missed > 0.99, missed
    print(f"[ema] guarded: clean step behind a skipped one: k = 1 (largest error / bound {worst:.3f}); the k = 2 reference is missed on {missed:.4f} of the elements")


# ------------------------------------------------------------------------------------------------ 5. model level
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


def _train_step(model, opt, batch):
    rgb, lidar, tgt = (t.to(DEV) for t in batch)
    with torch.no_grad():
        model(rgb, lidar)
    model.loss_backward(tgt)
    opt.step()


def _encoder_mask(model):
    enc = torch.zeros(model.param_arena.numel(), dtype=torch.bool)
    off = 0
    for name, p in model.named_parameters():
        if name.startswith(ENCODER):
            enc[off:off + p.numel()] = True
        off += p.numel()
    return enc.numpy()


@pytest.mark.parametrize("path", ["plain", "guarded"])
def test_three_steps_against_the_fp64_chain_of_lerps(path):
    """ema_decay 0.9 without warm-up.  Chain in fp64 over snapshots of the parameter arena: c_s = c_(s-1) + omd (p_s - c_(s-1)), c_0 = p_0.
    One kernel update errs by at most 2^-24 (omd |p - e| + |r|) <= 2^-24 (0.2 + 1) max(|e|, |p|) < 2^-23 max(|e|, |p|) (r lies between
    e and p), and the error carried in is multiplied by the decay; so after step s: |e_s - c_s| <= s 2^-23 max(|e|, |p|), the maximum
    taken over the values the chain has seen so far."""
    from oracle import restatement as R
    from dmmfods_amd.optim import FusedAdam
    arch = _arch(R, TINY, "mid3")
    model = _model(R, arch)
    opt = FusedAdam(model, ema_decay=0.9, ema_warmup=False, **(dict(max_grad_norm=1e9) if path == "guarded" else {}))
    omd = _omd(0.9, 0, 1)
    chain = model.param_arena.cpu().numpy().astype(np.float64)
    _same_bits(opt.ema_arena, model.param_arena, "the average starts as a copy of the parameters")
    seen = np.abs(chain)
    for s in range(1, 4):
        _train_step(model, opt, R.make_inputs(arch, 2, 64, 96, seed=s - 1))
        p = model.param_arena.cpu().numpy().astype(np.float64)
        chain = chain + omd * (p - chain)
        seen = np.maximum(seen, np.maximum(np.abs(p), np.abs(chain)))
        err = np.abs(opt.ema_arena.cpu().numpy().astype(np.float64) - chain)
        bound = s * 2.0 ** -23 * seen
        assert not (err > bound).any(), (path, s, int((err > bound).sum()), float((err / np.maximum(bound, 1e-300)).max()))
        print(f"[ema] model, {path}, step {s}: largest error / bound {float((err[bound > 0] / bound[bound > 0]).max()):.3f}, "
              f"|e - p| max {float(np.abs(chain - p).max()):.3e}")
    assert opt.ema_num_updates == 3 and opt.step_count == 3
    assert float(np.abs(chain - p).max()) > 0
    model.close()


def test_frozen_ranges_keep_the_average_equal_to_the_parameters():
    from oracle import restatement as R
    from dmmfods_amd.optim import FusedAdam
    arch = _arch(R, TINY, "mid3")
    model = _model(R, arch)
    model.freeze_encoder()
    opt = FusedAdam(model, ema_decay=0.9, ema_warmup=False)
    enc = _encoder_mask(model)
    assert 0 < enc.sum() < enc.size
    for s in range(2):
        _train_step(model, opt, R.make_inputs(arch, 2, 64, 96, seed=s))
    e, p = _bits(opt.ema_arena), _bits(model.param_arena)
    assert np.array_equal(e[enc], p[enc]), "a frozen element's average moved away from the parameter"
    assert float((e[~enc] != p[~enc]).mean()) > 0.9
    model.freeze_encoder(False)
    before = opt.ema_arena.cpu().numpy().copy()
    _train_step(model, opt, R.make_inputs(arch, 2, 64, 96, seed=2))
    e, p = opt.ema_arena.cpu().numpy(), model.param_arena.cpu().numpy()
    moved = float((_bits(e)[enc] != _bits(before)[enc]).mean())
    assert moved > 0.9 and float((_bits(e)[enc] != _bits(p)[enc]).mean()) > 0.9, moved
    # the released range simply joined: one more update of e == p_old towards p_new
    r = before[enc].astype(np.float64) + _omd(0.9, 0, 1) * (p[enc].astype(np.float64) - before[enc])
    assert not (np.abs(e[enc] - r) > 2.0 ** -23 * (_omd(0.9, 0, 1) * np.abs(p[enc].astype(np.float64) - before[enc]) + np.abs(r))).any()
    print(f"[ema] freeze: encoder ({int(enc.sum())} elements) bit-equal to the parameters while frozen; {moved:.4f} of it moved at the first released step")
    model.close()


# ------------------------------------------------------------------------------------------------ 6. ema_weights()
def test_ema_weights_runs_the_model_on_the_average_and_restores():
    from oracle import restatement as R
    from dmmfods_amd.optim import FusedAdam
    arch = _arch(R, TINY, "mid3")
    model = _model(R, arch)
    opt = FusedAdam(model, ema_decay=0.9, ema_warmup=False)
    for s in range(2):
        _train_step(model, opt, R.make_inputs(arch, 2, 64, 96, seed=s))
    rgb, lidar, tgt = (t.to(DEV) for t in R.make_inputs(arch, 2, 64, 96, seed=5))
    p0, e0, addr = _bits(model.param_arena).copy(), _bits(opt.ema_arena).copy(), model.param_arena.data_ptr()
    assert not np.array_equal(p0, e0)

    def eval_logits():
        model.eval()
        with torch.no_grad():
            out = model(rgb, lidar).detach().float().cpu().clone()
        model.train()
        return out

    # the model's answer on the other weights (eval forwards only in between: the running statistics are the same on both sides)
    live = eval_logits()
    with opt.ema_weights():
        assert np.array_equal(_bits(model.param_arena), e0) and np.array_equal(_bits(opt.ema_arena), p0) and model.param_arena.data_ptr() == addr
        averaged = eval_logits()
    assert np.array_equal(_bits(model.param_arena), p0) and np.array_equal(_bits(opt.ema_arena), e0)
    delta = float((averaged - live).abs().max())
    assert delta > 0 and bool(torch.isfinite(averaged).all())
    # the guards
    with torch.no_grad():
        model(rgb, lidar)                                                     # a training forward on the live weights ...
    with opt.ema_weights():
        with pytest.raises(RuntimeError, match="needs a preceding training-mode forward"):
            model.loss_backward(tgt)                                          # ... cannot be continued on the other weights
        with pytest.raises(RuntimeError):
            opt.step()
        with pytest.raises(RuntimeError):
            opt.load_state_dict({})
        with pytest.raises(RuntimeError):
            with opt.ema_weights():
                pass
        with torch.no_grad():
            model(rgb, lidar)
    with pytest.raises(RuntimeError, match="needs a preceding training-mode forward"):
        model.loss_backward(tgt)                                              # nor one taken inside, outside
    assert np.array_equal(_bits(model.param_arena), p0) and np.array_equal(_bits(opt.ema_arena), e0)
    with pytest.raises(KeyError):
        with opt.ema_weights():
            raise KeyError("the body fails")
    assert np.array_equal(_bits(model.param_arena), p0) and np.array_equal(_bits(opt.ema_arena), e0)
    # the export: averaged parameters, live buffers, loadable by the model
    esd, msd = opt.ema_state_dict(), model.state_dict()
    assert list(esd) == list(msd)
    other = _model(R, arch, seed=7)
    other.load_state_dict(esd)
    assert np.array_equal(_bits(other.param_arena), e0)
    _train_step(model, opt, (rgb, lidar, tgt))                                 # and training goes on
    assert opt.ema_num_updates == 3
    print(f"[ema] ema_weights: max |eval logits on the average - on the live weights| {delta:.3e}")
    other.close()
    model.close()


# ------------------------------------------------------------------------------------------------ 7. the agent
class _Loader:
    def __init__(self, batches):
        self.train_loader, self.train_iterations = batches, len(batches)
        self.valid_loader, self.valid_iterations = batches[:1], 1


def _agent(tmp_path, monkeypatch, batches, resume=False, ema=True):
    from dmmfods_amd.agents import Dense_U_Net_lidar_Agent as mod
    from dmmfods_amd.graphs.models.Dense_U_Net_lidar import Dense_U_Net_lidar
    cfg = get_config(str(tmp_path))
    cfg.dir.current_run.summary = str(tmp_path / "run" / "summary")
    cfg.dir.current_run.checkpoints = str(tmp_path / "run" / "checkpoints")
    cfg.model.concat_before_block_num, cfg.model.stream_2_in_channels = 3, 3
    if ema:
        cfg.optimizer.ema_decay = 0.5
    cfg.optimizer.lr_scheduler.want, cfg.optimizer.lr_scheduler.every_n_epochs, cfg.optimizer.lr_scheduler.gamma = True, 1, 0.5

    def factory(pretrained=False, config=None, compute_dtype=None, **kw):
        config.model.growth_rate, config.model.block_config, config.model.num_init_features = 8, (2, 2, 2, 2), 16
        return Dense_U_Net_lidar(config, compute_dtype=compute_dtype)
    monkeypatch.setattr(mod, "densenet121_u_lidar", factory)
    return mod.Dense_U_Net_lidar_Agent(cfg, torchvision_init=not resume, compute_dtype="fp32", data_loader=_Loader(batches))


def _resume_from(tmp_path, monkeypatch, batches, agent, where, **kw):
    name = agent.config.agent.best_checkpoint_name
    os.makedirs(str(tmp_path / where / "run" / "checkpoints"), exist_ok=True)
    shutil.copy(os.path.join(agent.config.dir.current_run.checkpoints, name), str(tmp_path / where / "run" / "checkpoints" / name))
    return _agent(tmp_path / where, monkeypatch, batches, resume=True, **kw)


def test_agent_validates_on_the_average_and_a_resume_keeps_it(tmp_path, monkeypatch):
    from oracle import restatement as R
    arch = _arch(R, TINY, "mid3")
    batches = [R.make_inputs(arch, 2, 64, 96, seed=s) for s in range(2)]
    agent = _agent(tmp_path / "a", monkeypatch, batches)
    agent.model.load_state_dict(R.make_state(arch, seed=99))
    opt = agent.optimizer
    opt.ema_reset()                                                            # (the weights were replaced behind the optimiser's back)
    assert opt.ema_decay == 0.5 and opt.ema_warmup is True
    for epoch in range(2):
        agent.current_epoch = epoch
        agent.train_one_epoch()
        p_bits = _bits(agent.model.param_arena).copy()
        with torch.no_grad():
            agent.validate()
        assert np.array_equal(_bits(agent.model.param_arena), p_bits)         # validation gave the live weights back
    assert [h.get("ema") for h in agent.val_history] == [True, True]
    assert all(bool(torch.isfinite(h["loss"]).all()) for h in agent.val_history)
    assert opt.step_count == 4 and opt.ema_num_updates == 4 and not np.array_equal(_bits(opt.ema_arena), p_bits)
    agent.save_checkpoint(is_best=True)
    ck = torch.load(os.path.join(agent.config.dir.current_run.checkpoints, agent.config.agent.best_checkpoint_name), map_location="cpu")
    assert set(ck) == {"epoch", "train_iteration", "val_iteration", "best_val_iou", "state_dict", "optimizer"}
    assert set(ck["optimizer"]) == {"state", "param_groups", "ema"}
    assert ck["optimizer"]["ema"]["decay"] == 0.5 and ck["optimizer"]["ema"]["warmup"] is True and ck["optimizer"]["ema"]["num_updates"] == 4
    assert np.array_equal(_bits(ck["optimizer"]["ema"]["params"]), _bits(opt.ema_arena))
    names = {k for k, _ in agent.model.named_parameters()}
    assert np.array_equal(_bits(torch.cat([t.reshape(-1) for k, t in ck["state_dict"].items() if k in names])), p_bits)
    agent.model.close()
    # resume: the average and its count come back, and training goes on from update 5
    resumed = _resume_from(tmp_path, monkeypatch, batches, agent, "b")
    ropt = resumed.optimizer
    assert ropt.ema_num_updates == 4 and ropt.step_count == 4
    assert np.array_equal(_bits(ropt.ema_arena), _bits(opt.ema_arena)) and np.array_equal(_bits(resumed.model.param_arena), p_bits)
    resumed.train_one_epoch()
    with torch.no_grad():
        resumed.validate()
    assert ropt.ema_num_updates == 6 and resumed.val_history[-1]["ema"] is True and bool(torch.isfinite(ropt.ema_arena).all())
    resumed.model.close()
    # a checkpoint written without an average: the average starts at the loaded parameters
    plain = _agent(tmp_path / "c", monkeypatch, batches, ema=False)
    plain.model.load_state_dict(R.make_state(arch, seed=99))
    assert plain.optimizer.ema_arena is None
    plain.train_one_epoch()
    with torch.no_grad():
        plain.validate()
    assert "ema" not in plain.val_history[-1]
    plain.save_checkpoint(is_best=True)
    pck = torch.load(os.path.join(plain.config.dir.current_run.checkpoints, plain.config.agent.best_checkpoint_name), map_location="cpu")
    assert set(pck["optimizer"]) == {"state", "param_groups"}
    q_bits = _bits(plain.model.param_arena).copy()
    plain.model.close()
    late = _resume_from(tmp_path, monkeypatch, batches, plain, "d")
    assert late.optimizer.step_count == 2 and late.optimizer.ema_num_updates == 0
    assert np.array_equal(_bits(late.optimizer.ema_arena), q_bits) and np.array_equal(_bits(late.model.param_arena), q_bits)
    late.train_one_epoch()
    assert late.optimizer.ema_num_updates == 2
    print(f"[ema] agent: validation rows {[h.get('ema') for h in agent.val_history]}, resumed at update 4, a plain checkpoint starts the average at its parameters")
    late.model.close()
