"""Which transitions run over a pooled buffer (plan.cpp: transition_pools) is a pure function of the pooled row count B * H/2 * W/2 and
the threshold (TRANSITION_POOL_MIN_ROWS, or DMM_TRANSITION_POOL_ROWS read when the plan is created).  On the CPU harness
(tools/hoststub/drive: the library's host code under AddressSanitizer + UBSan against the fake HIP runtime):

  * DenseNet-121 early fusion at 2 x 256 x 384 (pooled rows 3072 / 768 / 192) and at 2 x 512 x 768 (12288 / 3072 / 768): the default
    threshold selects exactly the transitions at or above it - a pooling launch behind the norm's finalize, the 1x1 on a specialised
    family (not igemm.store) over a plain operand, the weight gradient a plain one-tap launch, the data gradient untouched - in the
    training AND the eval forward list; the bound pass takes the bytes of the sizing pass (dmm_plan_bind refuses anything else) and
    every pointer of the life-cycle runs lies in the caller's regions;
  * at 64 x 96 the default plan is the pinned one (tests/golden/plan_dump_sha256.json), equal to the plan with the path switched off."""
import hashlib
import json
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def drive():
    out = os.path.join(ROOT, "tools", "hoststub", "_build")
    subprocess.run([os.path.join(ROOT, "tools", "hoststub", "build.sh"), out], check=True, capture_output=True, timeout=900)
    return os.path.join(out, "drive")


def _env(**extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith("DMM_") and not k.startswith("DRIVE_")}
    env.update(ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", **extra)
    return env


def _dump(drive, args, **extra):
    r = subprocess.run([drive, "dump"] + args, env=_env(**extra), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "OUTSIDE" not in r.stdout, (r.stdout[-500:] + r.stderr)[-3000:]
    return r.stdout


def _records(text):
    """{list: [(label, first argument line)]}"""
    out, cur, lines = {}, None, text.splitlines()
    for i, ln in enumerate(lines):
        m = re.match(r"list (\S+) records=", ln)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and not ln.startswith(" "):
            cur = None
        m = re.match(r"  op kind=.* label=(\S*) flops=(\S+) ", ln)
        if m and cur is not None:
            cur.append((m.group(1), float(m.group(2)), lines[i + 1] if i + 1 < len(lines) else ""))
    return out


def _default_threshold():
    src = open(os.path.join(ROOT, "dmmfods_amd", "csrc", "plan.cpp")).read()
    return int(re.search(r"TRANSITION_POOL_MIN_ROWS = (\d+);", src).group(1))


@pytest.mark.parametrize("H,W", [(256, 384), (512, 768)])
def test_default_threshold_selects_transitions_by_pooled_rows(drive, H, W):
    thr = _default_threshold()
    assert 480 < thr <= 12288        # above every pinned launch list's transitions (192 rows; 480 in the pinned dumps); not vacuous here
    args = ["d121e", "f16", "2", str(H), str(W)]
    rows = {n: 2 * (H >> (2 + n)) * (W >> (2 + n)) for n in (1, 2, 3)}       # transition n pools block n's map
    want = {n for n, r in rows.items() if r >= thr}
    text = _dump(drive, args)
    off = _records(_dump(drive, args, DMM_TRANSITION_POOL_ROWS="1000000000"))
    rec = _records(text)
    for lst in ("fwd_train", "fwd_eval"):
        labels = [r[0] for r in rec[lst]]
        pools = [i for i, lab in enumerate(labels) if lab.startswith("avgpool2.fwd/")]
        assert {int(re.search(r"transition(\d)\.pool$", labels[i]).group(1)) for i in pools} == want and len(pools) == len(want), (lst, labels)
        for i in pools:
            n = re.search(r"transition(\d)", labels[i]).group(1)
            assert labels[i - 1] == "" and rec[lst][i - 1][2].lstrip().startswith("bnfin:")          # behind the norm's finalize
            cls, layer = labels[i + 1].split("/")
            assert layer == f"f.transition{n}.conv" and cls.endswith(".store.n128") and not cls.startswith("igemm."), labels[i + 1]
            assert " mode=0 " in rec[lst][i + 1][2] and " Hs=%d " % (H >> (2 + int(n))) in rec[lst][i + 1][2]
        # the 1x1 keeps the reference-convention FLOP tag of the pooled form (x 4), whichever path runs it
        fl = {lab: f for lab, f, _ in rec[lst] if lab.endswith(".conv") and "transition" in lab}
        fl_off = {lab.split("/")[1]: f for lab, f, _ in off[lst] if lab.endswith(".conv") and "transition" in lab}
        assert {lab.split("/")[1]: f for lab, f in fl.items()} == fl_off and len(fl) == 3
        for n in set(rows) - want:
            assert f"igemm.store.n128/f.transition{n}.conv" in labels
    bwd = {lab: arg for lab, _, arg in rec["bwd"] if "transition" in lab}
    for n in (1, 2, 3):
        assert (" mode=0 " in bwd[f"wgrad.n128/f.transition{n}.conv"]) == (n in want)          # seg0 of the weight gradient: plain / pooling gather
        assert f"igemm.bnbwd.n128/f.transition{n}.conv" in bwd
    assert [r[0] for r in rec["bwd"]] == [r[0] for r in off["bwd"]]       # the backward list: the same launches, other operands
    if H != 256:
        return
    # life cycles with every transition on the path: bind accepts the sizes, every pointer of every record lies in the caller's regions
    r = subprocess.run([drive] + args + ["1"], env=_env(DMM_TRANSITION_POOL_ROWS="0"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "DRIVE OK" in r.stdout, (r.stdout + r.stderr)[-3000:]
    assert re.search(r"^life 0: .* 0 bad, .*violations 0$", r.stdout, re.M), r.stdout[-1000:]


def test_small_maps_keep_the_pinned_plan(drive):
    pinned = json.load(open(os.path.join(ROOT, "tests", "golden", "plan_dump_sha256.json")))
    args = ["d121e", "f16", "2", "64", "96"]
    default = _dump(drive, args)
    assert default == _dump(drive, args, DMM_TRANSITION_POOL_ROWS="1000000000")
    assert hashlib.sha256(default.encode()).hexdigest() == pinned[" ".join(args)]
    forced = _records(_dump(drive, args, DMM_TRANSITION_POOL_ROWS="0"))       # (the switch does reach this size)
    assert sum(lab.startswith("avgpool2.fwd/") for lab, _, _ in forced["fwd_train"]) == 3
