"""Frozen encoder (dmm_plan_set_encoder_frozen, the segmented Adam calls over the trainable ranges, model.freeze_encoder, FusedAdam's trainable
ranges), everything that needs no GPU: the ABI contract, the buckets and sizes of an unbound frozen plan, the Python surface on a
CPU-resident model, the optimiser's checkpoint format, and the sanitizer harness with DRIVE_FREEZE=1."""
import ctypes as C
import hashlib
import json
import math
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENCODER = ("features.", "stream_2_features.", "concat_module.")
TINY = dict(growth_rate=8, block_config=(2, 2, 2, 2), num_init_features=16)
D121 = dict(growth_rate=32, block_config=(6, 12, 24, 16), num_init_features=64)
NETS = {"tiny_no": (TINY, 1, 0, "f32"), "tiny_early": (TINY, 1, 3, "f32"), "tiny_mid3": (TINY, 3, 3, "f32"), "d121_early": (D121, 1, 3, "f16")}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from dmmfods_amd import _lib
    return _lib


def _desc(lib, net, batch=2, height=64, width=96):
    base, cbb, s2, dtype = NETS[net]
    d = lib.ModelDesc()
    d.growth_rate, d.num_blocks, d.num_init_features, d.bn_size, d.num_classes = base["growth_rate"], 4, base["num_init_features"], 4, 3
    for i, v in enumerate(base["block_config"]):
        d.block_config[i] = v
    d.concat_before_block_num, d.stream_1_in_channels, d.stream_2_in_channels = cbb, 3, s2
    d.batch, d.height, d.width = batch, height, width
    d.dtype = {"f32": lib.DMM_F32, "f16": lib.DMM_F16}[dtype]
    d.loss_scale, d.bn_momentum, d.bn_eps, d.iou_threshold, d.use_mfma = 1.0, 0.1, 1e-5, 0.7, 1
    return d


def _refused(lib, rc, word, code=None):
    assert rc == (lib.ERR_INVALID if code is None else code), rc
    msg = lib.lib().dmm_last_error().decode()
    assert word in msg, msg


# ------------------------------------------------------------------------------------------------ ABI
def test_new_symbols_are_declared_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "dmmfods_hip.h")).read()
    declared = set(re.findall(r"\b(dmm_[a-z0-9_]+)\s*\(", hdr)) - {"dmm_status"}
    L = lib.lib()
    for sym in ("dmm_plan_set_encoder_frozen", "dmm_adam_step_segmented", "dmm_adam_step_guarded_segmented"):
        assert sym in declared and sym in lib.EXPORTS and hasattr(L, sym), sym
    assert not [s for s in sorted(declared) if not hasattr(L, s)]
    assert set(lib.EXPORTS) <= declared


def test_set_encoder_frozen_contract_without_a_gpu(lib):
    L = lib.lib()
    _refused(lib, L.dmm_plan_set_encoder_frozen(None, 1), "null plan")
    h = C.c_void_p()
    lib.check(L.dmm_plan_create(C.byref(_desc(lib, "tiny_mid3")), C.byref(h)))
    try:
        before = (L.dmm_plan_workspace_bytes(h), L.dmm_plan_num_grad_buckets(h))
        assert L.dmm_plan_set_encoder_frozen(h, 0) == 0                      # a fresh plan: nothing changes
        assert (L.dmm_plan_workspace_bytes(h), L.dmm_plan_num_grad_buckets(h)) == before
        assert L.dmm_plan_set_encoder_frozen(h, 1) == 0
        assert L.dmm_plan_workspace_bytes(h) <= before[0]
        assert L.dmm_plan_set_encoder_frozen(h, 1) == 0                      # idempotent
        assert L.dmm_plan_set_encoder_frozen(h, 0) == 0                      # and back: the default plan again
        assert (L.dmm_plan_workspace_bytes(h), L.dmm_plan_num_grad_buckets(h)) == before
        # a bound plan refuses (DMM_ERR_STATE) - checked where a plan can be bound: the harness below, and tests/test_freeze_gpu.py
    finally:
        lib.check(L.dmm_plan_destroy(h))


def test_guarded_ranges_refuses_bad_arguments_without_a_gpu(lib):
    """The guarded step over trainable ranges is the guarded segmented call under a table of the ranges, one class per step origin:
    what the table (dmm_adam_table_init) and the step (dmm_adam_step_guarded_segmented) refuse between them."""
    L = lib.lib()
    P = 1 << 20   # an address nothing dereferences: every refusal below comes before the first HIP call

    def table(ranges=((0, 64, 0), (64, 32, 1)), n=1000, nsegs=None, nclasses=2, table=P):
        arr = None if ranges is None else (lib.AdamSegment * len(ranges))(*(lib.AdamSegment(*r) for r in ranges))
        return L.dmm_adam_table_init(table, arr, (len(ranges) if ranges is not None else 2) if nsegs is None else nsegs, n, nclasses, None)

    def call(t0=(0, 3), nsegs=2, b1=0.9, **over):
        cl = None if t0 is None else (lib.AdamClass * len(t0))(*(lib.AdamClass(1e-3, b1, 0.999, 1e-8, 0.0, 0, t) for t in t0))
        a = dict(params=P, grads=P, m=P, v=P, table=P, max_norm=0.0, growth=2.0, backoff=0.5, interval=2000, state=P, scratch=P)
        a.update(over)
        return L.dmm_adam_step_guarded_segmented(a["params"], a["grads"], a["m"], a["v"], 1000, a["table"], nsegs, cl, 2, a["max_norm"],
                                                 a["growth"], a["backoff"], a["interval"], a["state"], a["scratch"], None)

    for name in ("params", "grads", "m", "v", "table", "state", "scratch"):
        _refused(lib, call(**{name: None}), "null")
    _refused(lib, call(t0=None), "null")
    _refused(lib, table(ranges=None), "null")
    _refused(lib, table(nsegs=0), "nsegs")
    _refused(lib, table(nsegs=-1), "nsegs")
    _refused(lib, call(nsegs=0), "nsegs")
    _refused(lib, table(ranges=((-1, 64, 0), (64, 32, 1))), "lies outside")
    _refused(lib, table(ranges=((0, 64, 0), (64, -2, 1))), "count")
    _refused(lib, call(t0=(0, -1)), "t0")
    _refused(lib, table(ranges=((0, 64, 0), (63, 32, 1))), "overlaps")
    _refused(lib, table(ranges=((64, 32, 0), (0, 65, 1))), "unsorted or overlaps")     # whatever the order
    _refused(lib, table(ranges=((0, 1, 0), (2 ** 62, 2 ** 62, 1))), "lies outside")    # (begin + count would overflow)
    _refused(lib, call(grads=P + 2), "misaligned")
    _refused(lib, call(state=P + 4), "misaligned")
    _refused(lib, call(growth=0.5), "growth_factor")
    _refused(lib, call(backoff=0.0), "backoff_factor")
    _refused(lib, call(interval=-1), "growth_interval")
    _refused(lib, call(max_norm=float("nan")), "max_norm")
    _refused(lib, call(b1=1.0), "betas")
    _refused(lib, call(), "not initialised by dmm_adam_table_init")              # all else in order: the table itself is unknown


# ------------------------------------------------------------------------------------------------ unbound plans
def _tensors(lib, h):
    L = lib.lib()
    out = []
    for i in range(L.dmm_plan_num_tensors(h)):
        name, kind, nd = C.c_char_p(), C.c_int32(), C.c_int32()
        shape, off = (C.c_int64 * 4)(), C.c_int64()
        lib.check(L.dmm_plan_tensor_info(h, i, C.byref(name), C.byref(kind), C.byref(nd), C.byref(shape), C.byref(off)))
        if kind.value <= lib.T_BN_BIAS:
            out.append((name.value.decode(), off.value, int(math.prod(shape[j] for j in range(nd.value)))))
    return out


def _buckets(lib, h):
    L = lib.lib()
    out = []
    for i in range(L.dmm_plan_num_grad_buckets(h)):
        off, cnt = C.c_int64(), C.c_int64()
        lib.check(L.dmm_plan_grad_bucket(h, i, C.byref(off), C.byref(cnt)))
        out.append((off.value, cnt.value))
    return out


@pytest.mark.parametrize("net", sorted(NETS))
def test_frozen_plan_buckets_cover_exactly_the_trainable_tensors(lib, net):
    L = lib.lib()
    h = C.c_void_p()
    lib.check(L.dmm_plan_create(C.byref(_desc(lib, net)), C.byref(h)))
    try:
        tensors = _tensors(lib, h)
        nparams = L.dmm_plan_num_params(h)
        default_ws, default_buckets = L.dmm_plan_workspace_bytes(h), _buckets(lib, h)
        assert sorted(default_buckets)[0][0] == 0 and sum(n for _, n in default_buckets) == nparams
        lib.check(L.dmm_plan_set_encoder_frozen(h, 1))
        assert 0 < L.dmm_plan_workspace_bytes(h) <= default_ws
        buckets = sorted(_buckets(lib, h))
        assert buckets and all(n > 0 for _, n in buckets)
        covered = set()
        for (off, n), nxt in zip(buckets, buckets[1:] + [(nparams, 0)]):
            assert off + n <= nxt[0]                                         # disjoint, inside the arena
            covered.add((off, off + n))
        enc = [(o, o + n) for name, o, n in tensors if name.startswith(ENCODER)]
        train = [(o, o + n) for name, o, n in tensors if not name.startswith(ENCODER)]
        assert enc and train
        for lo, hi in enc:                                                   # no bucket touches an encoder tensor
            assert all(hi <= b0 or b1 <= lo for b0, b1 in covered), (lo, hi)
        for lo, hi in train:                                                 # every trainable tensor lies inside one bucket
            assert any(b0 <= lo and hi <= b1 for b0, b1 in covered), (lo, hi)
        assert sum(b1 - b0 for b0, b1 in covered) == sum(hi - lo for lo, hi in train)   # and the union is no more than those
    finally:
        lib.check(L.dmm_plan_destroy(h))


# ------------------------------------------------------------------------------------------------ Python surface
def _cpu_model(lib, cbb=3, s2=3):
    from dmmfods_amd.graphs.models.Dense_U_Net_lidar import Dense_U_Net_lidar
    from dmmfods_amd.utils.Dense_U_Net_lidar_helper import get_config
    cfg = get_config("/tmp/dmm_test")
    cfg.model.growth_rate, cfg.model.block_config, cfg.model.num_init_features = TINY["growth_rate"], TINY["block_config"], TINY["num_init_features"]
    cfg.model.concat_before_block_num, cfg.model.stream_2_in_channels = cbb, s2
    return Dense_U_Net_lidar(cfg, compute_dtype="fp32")


def _maximal_runs(model):
    runs, off = [], 0
    for p in model.parameters():
        if p.requires_grad:
            if runs and runs[-1][0] + runs[-1][1] == off:
                runs[-1][1] += p.numel()
            else:
                runs.append([off, p.numel()])
        off += p.numel()
    return [tuple(r) for r in runs]


def test_freeze_encoder_flags_exactly_the_encoder_and_mixtures_are_refused(lib):
    from dmmfods_amd.optim import FusedAdam
    model = _cpu_model(lib)
    assert model.encoder_frozen is False
    assert model.freeze_encoder() is model and model.encoder_frozen is True
    for name, p in model.named_parameters():
        assert p.requires_grad == (not name.startswith(ENCODER)), name
    assert any(n.startswith("stream_2_features.") for n, _ in model.named_parameters())
    opt = FusedAdam(model)
    runs = _maximal_runs(model)
    assert len(runs) == 1 and 0 < runs[0][0] and runs[0][0] + runs[0][1] < model.param_arena.numel()   # features | decoder, head | stream 2, concat
    assert opt.trainable_ranges() == [(o, n, 0) for o, n in runs]
    # released: one range again, the encoder's parts with their own origin once steps have been taken
    model.freeze_encoder(False)
    assert model.encoder_frozen is False and all(p.requires_grad for p in model.parameters())
    assert opt.trainable_ranges() == [(0, model.param_arena.numel(), 0)]
    # requires_grad_ set directly: the whole encoder is honoured, anything else refused with the first offending parameter's name
    for n, p in model.named_parameters():
        if n.startswith(ENCODER):
            p.requires_grad_(False)
    assert model.encoder_frozen is True
    model.freeze_encoder(False)
    dec = dict(model.named_parameters())["decoder.Transposed_Convolution_1.weight"]
    dec.requires_grad_(False)
    with pytest.raises(ValueError, match="decoder.Transposed_Convolution_1.weight"):
        model.encoder_frozen
    with pytest.raises(ValueError, match="decoder.Transposed_Convolution_1.weight"):
        model._check_trainable_set()                                         # what a training-mode forward calls first
    dec.requires_grad_(True)
    first = dict(model.named_parameters())["features.conv0.weight"]
    first.requires_grad_(False)
    with pytest.raises(ValueError, match="features.norm0.weight"):           # the first encoder parameter still trainable
        model._check_trainable_set()
    first.requires_grad_(True)
    assert model.encoder_frozen is False
    # early / no fusion: the encoder is `features` alone
    for cbb, s2 in ((1, 3), (1, 0)):
        m = _cpu_model(lib, cbb, s2).freeze_encoder()
        assert {n.split(".")[0] for n, p in m.named_parameters() if not p.requires_grad} == {"features"}
        assert FusedAdam(m).trainable_ranges() == [(o, n, 0) for o, n in _maximal_runs(m)]


def test_state_dict_has_per_parameter_steps_and_restores_the_phase(lib):
    from dmmfods_amd.optim import FusedAdam
    g = torch.Generator().manual_seed(7)
    model = _cpu_model(lib).freeze_encoder()
    opt = FusedAdam(model, lr=2e-3, weight_decay=0.01)
    names = [n for n, _ in model.named_parameters()]
    enc_idx = [i for i, n in enumerate(names) if n.startswith(ENCODER)]
    dec_idx = [i for i, n in enumerate(names) if not n.startswith(ENCODER)]
    opt.exp_avg.copy_(torch.randn(opt.exp_avg.shape, generator=g))
    opt.exp_avg_sq.copy_(torch.rand(opt.exp_avg_sq.shape, generator=g))
    opt.step_count = 5                                                       # five steps with the encoder frozen
    sd = opt.state_dict()
    assert sorted(sd["state"]) == dec_idx                                    # never trained: no entry, as in torch
    assert all(float(sd["state"][i]["step"]) == 5.0 for i in dec_idx)
    model.freeze_encoder(False)                                              # released at step 5 ...
    runs = opt.trainable_ranges()
    assert [r[2] for r in runs] == [5, 0, 5] and sum(r[1] for r in runs) == model.param_arena.numel()
    assert runs[0][0] == 0 and runs[0][0] + runs[0][1] == runs[1][0] and runs[1][0] + runs[1][1] == runs[2][0]
    opt.step_count = 8                                                       # ... and three more steps
    sd = opt.state_dict()
    assert sorted(sd["state"]) == list(range(len(names)))
    assert all(float(sd["state"][i]["step"]) == 8.0 for i in dec_idx) and all(float(sd["state"][i]["step"]) == 3.0 for i in enc_idx)
    # a fresh optimiser on a fresh model resumes in the same phase
    model2 = _cpu_model(lib)
    opt2 = FusedAdam(model2)
    opt2.load_state_dict(sd)
    assert opt2.step_count == 8 and opt2.trainable_ranges() == runs
    assert torch.equal(opt2.exp_avg, opt.exp_avg) and torch.equal(opt2.exp_avg_sq, opt.exp_avg_sq)
    sd2 = opt2.state_dict()
    assert all(float(sd2["state"][i]["step"]) == float(sd["state"][i]["step"]) for i in sd["state"])
    # the frozen-phase checkpoint into a frozen model: the encoder still has no state; released later it starts at its own step 1
    model3 = _cpu_model(lib).freeze_encoder()
    opt3 = FusedAdam(model3)
    model.freeze_encoder(True)                                               # frozen again at step 8, then two more steps of the rest:
    opt.trainable_ranges()
    opt.step_count = 10
    frozen_again = opt.state_dict()                                          # the encoder keeps the 3 steps it has taken
    assert all(float(frozen_again["state"][i]["step"]) == 3.0 for i in enc_idx)
    assert all(float(frozen_again["state"][i]["step"]) == 10.0 for i in dec_idx)
    opt3.load_state_dict({"state": {i: sd["state"][i] for i in dec_idx}, "param_groups": sd["param_groups"]})
    assert opt3.step_count == 8 and sorted(opt3.state_dict()["state"]) == dec_idx
    model3.freeze_encoder(False)
    assert [r[2] for r in opt3.trainable_ranges()] == [8, 0, 8]
    # torch.optim.Adam over the trainable parameters accepts the dict of the frozen phase as it is
    model4 = _cpu_model(lib).freeze_encoder()
    opt4 = FusedAdam(model4)
    opt4.step_count = 5
    sd4 = opt4.state_dict()
    ref = torch.optim.Adam(list(model4.parameters()), lr=1e-3)
    ref.load_state_dict(sd4)
    params = list(model4.parameters())
    assert float(ref.state[params[dec_idx[0]]]["step"]) == 5.0 and params[enc_idx[0]] not in ref.state
    assert ref.param_groups[0]["lr"] == 1e-3 or ref.param_groups[0]["lr"] == sd4["param_groups"][0]["lr"]


def test_agent_reads_freeze_encoder_epochs_only_if_present():
    from dmmfods_amd.agents.Dense_U_Net_lidar_Agent import Dense_U_Net_lidar_Agent
    from dmmfods_amd.utils.Dense_U_Net_lidar_helper import get_config
    cfg = get_config("/tmp/dmm_test")
    assert "freeze_encoder_epochs" not in cfg.optimizer                      # create_config keeps the reference's field list
    assert Dense_U_Net_lidar_Agent._optional(cfg.optimizer, "freeze_encoder_epochs") is None
    cfg.optimizer.freeze_encoder_epochs = 2
    assert Dense_U_Net_lidar_Agent._optional(cfg.optimizer, "freeze_encoder_epochs") == 2


# ------------------------------------------------------------------------------------------------ sanitizer harness
@pytest.fixture(scope="module")
def host_drive():
    out = os.path.join(ROOT, "tools", "hoststub", "_build")
    subprocess.run([os.path.join(ROOT, "tools", "hoststub", "build.sh"), out], check=True, capture_output=True, timeout=900)
    return os.path.join(out, "drive")


def _env(**extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith("DMM_") and not k.startswith("DRIVE_")}
    env.update(ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", **extra)
    return env


def _lists(text):
    """{list name: [label of every record]} and the text of each list, from `drive dump`."""
    labels, bodies, cur = {}, {}, None
    for ln in text.splitlines():
        m = re.match(r"list (\S+) records=", ln)
        if m:
            cur = m.group(1)
            labels[cur], bodies[cur] = [], []
        elif cur is not None and not ln.startswith(" "):
            cur = None
        if cur is not None:
            bodies[cur].append(ln)
            m = re.match(r"  op kind=.* label=(\S*) flops=", ln)
            if m:
                labels[cur].append(m.group(1))
    return labels, {k: "\n".join(v) for k, v in bodies.items()}


HARNESS_CASES = (("tiny_mid", "bf16", 2, 96, 160), ("d121e", "f16", 2, 64, 96), ("tiny_no", "f32", 2, 64, 96))


def test_sanitizer_harness_with_a_frozen_plan(host_drive):
    """Life cycles with DRIVE_FREEZE=1 (the mode set on the unbound plan, null and bound plans refused, bind in the mode, every list run,
    dmm_adam_step_guarded_segmented with two ranges and a class with t0 > 0, overlapping ranges refused, buckets and unpack descriptors checked against
    the encoder's tensors) are clean under ASan / UBSan.  `drive dump`: the forward lists are those of the default plan, the backward
    list is a strict prefix-by-labels of the default one without any encoder record, and no unpack descriptor scatters into the
    encoder.  Without the switch the dump is the parent commit's, byte for byte (tests/golden/plan_dump_sha256.json: SHA-256 of
    `drive dump` built from the commit this feature was added to; a change that alters the default plan on purpose renews it)."""
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "plan_dump_sha256.json")))
    for arch, dtype, b, h, w in HARNESS_CASES:
        args = [arch, dtype, str(b), str(h), str(w)]
        r = subprocess.run([host_drive] + args + ["2"], env=_env(DRIVE_FREEZE="1"), capture_output=True, text=True, timeout=600)
        tail = (r.stdout + r.stderr)[-3000:]
        assert r.returncode == 0 and "DRIVE OK" in r.stdout, (arch, tail)
        lives = [ln for ln in r.stdout.splitlines() if ln.startswith("life ")]
        assert len(lives) == 2 and all(", 0 bad," in ln and ln.endswith("violations 0") for ln in lives), lives
        off = subprocess.run([host_drive, "dump"] + args, env=_env(), capture_output=True, text=True, timeout=600)
        on = subprocess.run([host_drive, "dump"] + args, env=_env(DRIVE_FREEZE="1"), capture_output=True, text=True, timeout=600)
        assert off.returncode == 0 and on.returncode == 0, (off.stderr[-2000:], on.stderr[-2000:])
        assert "OUTSIDE" not in on.stdout
        assert hashlib.sha256(off.stdout.encode()).hexdigest() == golden[" ".join(args)], args
        lab_off, body_off = _lists(off.stdout)
        lab_on, body_on = _lists(on.stdout)
        assert lab_on["fwd_train"] == lab_off["fwd_train"] and lab_on["fwd_eval"] == lab_off["fwd_eval"]
        # the forward lists differ only in where the workspace puts things (the frozen plan reserves less): same records, same fields
        strip = lambda t: re.sub(r"=ws\+\d+", "=ws", t)   # noqa: E731
        assert strip(body_on["fwd_train"]) == strip(body_off["fwd_train"]) and strip(body_on["fwd_eval"]) == strip(body_off["fwd_eval"])
        n_on, n_off = len(lab_on["bwd"]), len(lab_off["bwd"])
        assert 3 < n_on < n_off
        unpack = lambda labs: [x for x in labs if x.startswith("unpack/")]   # noqa: E731  (one per bucket: fewer buckets, fewer of them)
        assert [x for x in lab_on["bwd"] if not x.startswith("unpack/")] == [x for x in lab_off["bwd"] if not x.startswith("unpack/")][:n_on - len(unpack(lab_on["bwd"]))]
        for lab in lab_on["bwd"]:
            layer = lab.split("/", 1)[1] if "/" in lab else lab
            assert not layer.startswith(("f.", "s2.", "concat_module", "features", "stream_2_features", "pool0")), lab
        assert any(lab.split("/", 1)[-1].startswith("f.") for lab in lab_off["bwd"])       # (the default list does have them)
        # unpack rows: no descriptor's master gradient lies in an encoder range of the arena
        m = re.search(r"nparams=(\d+)", on.stdout)
        unp = on.stdout.split("table unpacks entries=")[1].split("unpack_prefix")[0]
        gws = [int(x) // 4 for x in re.findall(r" gw=grads\+(\d+)", unp)]
        unp_off = off.stdout.split("table unpacks entries=")[1].split("unpack_prefix")[0]
        gws_off = [int(x) // 4 for x in re.findall(r" gw=grads\+(\d+)", unp_off)]
        bks = [(int(a), int(a) + int(n)) for a, n in re.findall(r"  bucket off=(\d+) n=(\d+)", on.stdout)]
        assert gws and len(gws) < len(gws_off) and int(m.group(1)) > 0
        assert all(any(lo <= gw < hi for lo, hi in bks) for gw in gws)       # (buckets hold trainable tensors only: the test above)
        assert min(lo for lo, _ in bks) > 0                                  # `features` sits at the front of the arena
