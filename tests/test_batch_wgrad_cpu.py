"""Launch coalescing (dmm_set_option("batch_wgrad")) on the CPU harness: tools/hoststub/drive - the library's host code built with
AddressSanitizer + UBSan against the fake HIP runtime - watches every enqueue call of its life-cycle runs (training steps, the
external-gradient backward, a profiled and a filtered-profile pass, one unsynchronised step) and fails if a batch is still pending
where the weight-gradient side is joined or a gradient bucket is signalled, or if at the end of a call a dense 3x3 weight-gradient
record or a bw1.reduce record has not been served exactly once.  Here: both settings of the option, the counts, and the plan dump."""
import hashlib
import json
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [
    # (arch, dtype, batch, H, W, wg3 records per backward pass)
    ("d121e", "f16", 2, 64, 96, 58),
    ("d121e", "bf16", 4, 320, 480, 58),      # the flagship's launch-geometry classes at a quarter of the size
    ("tiny_mid", "f16", 2, 128, 192, 8),     # (2, 2, 2) with mid fusion: the second encoder has a block of its own
    ("g8_mid", "f32", 2, 64, 96, 0),         # nothing to batch: fp32 has neither family
]
BACKWARD_PASSES = 6                          # of one life of the driver


@pytest.fixture(scope="module")
def drive():
    out = os.path.join(ROOT, "tools", "hoststub", "_build")
    subprocess.run([os.path.join(ROOT, "tools", "hoststub", "build.sh"), out], check=True, capture_output=True, timeout=900)
    return os.path.join(out, "drive")


def _env(**extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith("DMM_") and not k.startswith("DRIVE_")}
    env.update(ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", **extra)
    return env


def _life(drive, arch, dtype, b, h, w, lives=2, **extra):
    r = subprocess.run([drive, arch, dtype, str(b), str(h), str(w), str(lives)], env=_env(**extra), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "DRIVE OK" in r.stdout, (arch, dtype, extra, (r.stdout + r.stderr)[-3000:])
    rows = [tuple(int(v) for v in m.groups()) for m in re.finditer(
        r"^batch life \d+: (\d+) wg3 records in (\d+) launches, (\d+) bw1\.reduce records in (\d+) launches, (\d+) join / bucket events checked, (\d+) bad$",
        r.stdout, re.M)]
    assert len(rows) == lives, r.stdout[-2000:]
    launches = [int(m[1]) for m in re.finditer(r"^life \d+: .*?, (\d+) launches,", r.stdout, re.M)]
    return rows, launches


@pytest.mark.parametrize("arch,dtype,b,h,w,nwg3", CASES)
def test_life_cycles_with_and_without_batching(drive, arch, dtype, b, h, w, nwg3):
    on, launches_on = _life(drive, arch, dtype, b, h, w)
    off, launches_off = _life(drive, arch, dtype, b, h, w, DRIVE_OPTIONS_OFF="batch_wgrad")
    side, launches_side = _life(drive, arch, dtype, b, h, w, DRIVE_BATCH_WGRAD="2")
    assert on[0] == on[1] and off[0] == off[1], (on, off)         # a pure function of the launch list and the option
    assert side[0][:4] == on[0][:4] and side[0][5] == 0 and launches_side == launches_on   # the same batches on either stream
    w3_rec, w3_l, rd_rec, rd_l, syncs, bad = on[0]
    assert bad == 0 and off[0][5] == 0 and syncs > 0 and syncs == off[0][4]
    assert w3_rec == BACKWARD_PASSES * nwg3 == off[0][0] and rd_rec == off[0][2]
    assert (off[0][1], off[0][3]) == (w3_rec, rd_rec)             # off: every record is its own launch
    if nwg3:
        assert w3_l < w3_rec and w3_l % BACKWARD_PASSES == 0      # the same batches in every pass: eager, profiled, filtered, external gradient
        assert rd_rec == 0 or rd_l < rd_rec
        # each grouped wg3 launch saves its members' launches and their reductions, each grouped reduction its members' launches
        assert launches_off[0] - launches_on[0] == 2 * (w3_rec - w3_l) + (rd_rec - rd_l), (launches_on, launches_off)
    else:
        assert (w3_l, rd_l) == (0, 0) and launches_on == launches_off


def test_plan_dump_does_not_know_the_option(drive):
    """The batches are the executor's: the plan - records, labels, families, workspace - is the pinned one with the option on or off."""
    pinned = json.load(open(os.path.join(ROOT, "tests", "golden", "plan_dump_sha256.json")))
    args = ["d121e", "f16", "2", "64", "96"]
    outs = []
    for extra in ({}, {"DRIVE_OPTIONS_OFF": "batch_wgrad"}):
        r = subprocess.run([drive, "dump"] + args, env=_env(**extra), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout[-500:] + r.stderr)[-3000:]
        outs.append(r.stdout)
    assert outs[0] == outs[1]
    assert hashlib.sha256(outs[0].encode()).hexdigest() == pinned["d121e f16 2 64 96"]
