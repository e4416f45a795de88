"""The launch-list executor (capi.cpp: run_ops and its parts) pinned on the CPU: the sequence of enqueue calls IS the schedule.

tools/hoststub/drive with DRIVE_TRACE_ENQUEUE=1 prints every kernel launch, event record, stream wait, hipMemsetAsync and
hipMemcpyAsync the library's host code makes against the fake HIP runtime as one `T ...` line (streams and events numbered in the
order they first appear), and a failing library call as `T error <code> <message>`.  A mistake in the executor silently reorders
launches across streams; here it changes a hash.

tests/golden/enqueue_trace_sha256.json maps "environment | arguments" to the SHA-256 of a run's `T` lines.  It was made from the csrc
directory of commit 138dbf9 - the commit in front of the one that split run_ops into routing, batching, profiling and launch -
built with this tree's driver and fake runtime:

    DRIVE_SRC=<checkout of 138dbf9>/dmmfods_amd/csrc tools/hoststub/build.sh <dir>
    python tests/test_enqueue_trace_cpu.py <dir>/drive

so the split is shown to make the parent's calls, call for call.  A change that alters the schedule ON PURPOSE renews the file the
same way from its own build (and says so); any other change leaves it alone.

Renewed once since, from the tree that made adam_segmented_kernel the library's only Adam kernel: the two rows that take an
optimiser step (DRIVE_FREEZE=1; DRIVE_DYN_SCALE=1 DRIVE_GROUPS=1) changed in their Adam launch lines - kernel name and grid - and the
DRIVE_FREEZE row lost one grad_sumsq launch per life, because the driver's two adjacent trainable ranges are one run under a segment
table; the other eleven hashes are those of 138dbf9.  profiles/r09/adam_trace_diff.txt holds the line-by-line comparison.

The second test pins the pure predicates the executor routes by (plan.h: side_forks, batch_kind, flushes_batches, route): `drive route`
walks a table of records through them, and the expected answers are written out here from the expressions run_ops had at 138dbf9."""
import hashlib
import itertools
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "enqueue_trace_sha256.json")
LIFE = "tiny_mid f16 2 64 96"
ROWS = [
    # (environment, arguments, exit status)
    ({}, LIFE + " 2", 0),                                                   # two lives: the pool's events are used again
    ({"DRIVE_OPTIONS_OFF": "batch_wgrad"}, LIFE + " 2", 0),
    ({"DRIVE_BATCH_WGRAD": "2"}, LIFE + " 2", 0),
    ({"DRIVE_OPTIONS_OFF": "overlap_wgrad"}, LIFE + " 2", 0),
    ({"DRIVE_FREEZE": "1"}, LIFE + " 2", 0),
    ({"DRIVE_DYN_SCALE": "1", "DRIVE_GROUPS": "1"}, "tiny_early bf16 2 64 96 1", 0),
    ({"DMM_GRAD_BUCKET_MB": "1"}, "d121e f16 2 64 96 1", 0),                # many bucket signals
    ({"DRIVE_NO_MFMA": "1"}, "tiny_no f16 1 64 96 1", 0),
    ({}, "g8_mid f32 2 64 96 1", 0),
    ({}, "d121m bf16 2 64 96 1", 0),
    ({"DMM_NO_CVP_MERGE": "1", "DMM_PACK_CUT": "1"}, LIFE + " 1", 0),
    ({"DRIVE_TAMPER_RECORDED_FAMILY": "1"}, LIFE + " 1", 2),                # the error exit: the joins in front of it, and its text
    ({}, "accum " + LIFE, 0),
]
TAMPER_ERROR = "T error -4 launch 'wg3.n128/f.b3.l2.conv2': the plan recorded family wg5, generic ran"


def _key(envx, args):
    return (" ".join("%s=%s" % kv for kv in sorted(envx.items())) or "(none)") + " | " + args


def _trace(drive, envx, args, rc):
    env = {k: v for k, v in os.environ.items() if not k.startswith("DMM_") and not k.startswith("DRIVE_")}
    env.update(envx, DRIVE_TRACE_ENQUEUE="1", ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([drive] + args.split(), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == rc, (envx, args, (r.stdout[-1000:] + r.stderr)[-3000:])
    if rc == 0:
        assert ("ACCUM OK" if args.startswith("accum") else "DRIVE OK") in r.stdout, (envx, args, r.stdout[-1000:])
    else:
        assert "DRIVE OK" not in r.stdout
    return [ln for ln in r.stdout.splitlines() if ln.startswith("T ")]


@pytest.fixture(scope="module")
def drive():
    out = os.path.join(ROOT, "tools", "hoststub", "_build")
    subprocess.run([os.path.join(ROOT, "tools", "hoststub", "build.sh"), out], check=True, capture_output=True, timeout=900)
    return os.path.join(out, "drive")


@pytest.mark.parametrize("envx,args,rc", ROWS, ids=[_key(e, a) for e, a, _ in ROWS])
def test_enqueue_calls_are_the_pinned_ones(drive, envx, args, rc):
    pinned = json.load(open(GOLDEN))
    lines = _trace(drive, envx, args, rc)
    assert len(lines) > 100 and {"launch", "record", "wait", "memset"} <= {ln.split()[1] for ln in lines}, len(lines)   # (not vacuous)
    if rc:
        assert lines[-1] == TAMPER_ERROR and lines[-2].startswith("T wait "), lines[-4:]
    digest = hashlib.sha256("\n".join(lines).encode()).hexdigest()
    assert digest == pinned[_key(envx, args)], (_key(envx, args), len(lines))


# ---- the predicates ----
KINDS = ["MEMSET", "CONVERT", "IGEMM", "WGRAD", "BNFIN", "BNBWD", "POOL", "POOLBWD", "BCE", "PACK", "UNPACK", "COPY", "APPLYCORR", "BW1", "JOIN",
         "BW1RED", "RAWFIN", "FIN64"]                                        # plan.h: enum OpKind, in order
WG3, OTHER = 6, 7                                                            # common.h: enum Impl (wg3; wg5 stands for "another family")


def _expected_route_table():
    """The expressions of run_ops at 138dbf9, one per answer (capi.cpp l.419, l.421-428, l.437, l.441-461)."""
    out = []
    for kind, leaf, chain, signal, impl, epi in itertools.product(range(len(KINDS)), range(4), (0, 1), (-1, 0), (WG3, OTHER), (0, 1)):
        if epi == 1 and KINDS[kind] != "JOIN":
            continue
        wgrad, bw1red, join = KINDS[kind] == "WGRAD", KINDS[kind] == "BW1RED", KINDS[kind] == "JOIN"
        forks = (not chain) and leaf != 2 and leaf != 3 and (wgrad or leaf != 0)                                           # l.419
        flushes = forks or leaf == 3 or signal >= 0 or (join and epi != 1)                                                  # l.437
        batch = []
        for mfma in (0, 1):
            if forks and signal < 0 and wgrad and impl == WG3 and mfma:                                                     # l.421-422
                batch.append("W3")
            elif forks and signal < 0 and not (wgrad and impl == WG3 and mfma) and bw1red:                                  # l.428
                batch.append("RD")
            else:
                batch.append("none")
        routes = []
        for overlap, forked, batch_main in itertools.product((0, 1), (0, 1), (0, 1)):
            if overlap and leaf == 3 and forked:                                                                            # l.441
                routes.append("SIDE_CONTINUE")
            elif batch_main and forks and ((wgrad and impl == WG3) or bw1red):                                              # l.447
                routes.append("MAIN")
            elif overlap and (not chain) and (wgrad or leaf != 0):                                                          # l.449
                routes.append("PACK_FORK" if leaf == 2 else "SIDE_FORK")                                                    # l.455
            else:
                routes.append("MAIN")
        out.append("R %s leaf=%d chain=%d signal=%d impl=%s epi=%d : forks=%d flushes=%d batch=%s route=%s" % (
            KINDS[kind], leaf, chain, signal, "wg3" if impl == WG3 else "other", epi, forks, flushes, ",".join(batch), ",".join(routes)))
    return out


def test_route_predicates_answer_as_the_parent_expressions(drive):
    """Every kind x leaf 0-3 x chain x signal -1 / 0 x family wg3 / another (x epi 0 / 1 for OP_JOIN); per record side_forks,
    flushes_batches, batch_kind for mfma 0 / 1 and route for the eight combinations of (overlap, forked, batch_main)."""
    r = subprocess.run([drive, "route"], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout[-500:] + r.stderr)[-3000:]
    got = [ln for ln in r.stdout.splitlines() if ln.startswith("R ")]
    want = _expected_route_table()
    assert len(want) == (len(KINDS) + 1) * 4 * 2 * 2 * 2
    assert {w.split("route=")[1].split(",")[i] for w in want for i in range(8)} == {"MAIN", "SIDE_CONTINUE", "SIDE_FORK", "PACK_FORK"}
    assert {w.split("batch=")[1].split()[0] for w in want} == {"none,none", "none,W3", "RD,RD"}
    for g, w in zip(got, want):
        assert g == w
    assert len(got) == len(want)


if __name__ == "__main__":   # python tests/test_enqueue_trace_cpu.py <drive binary>: writes the golden file from that build
    table = {_key(e, a): hashlib.sha256("\n".join(_trace(sys.argv[1], e, a, rc)).encode()).hexdigest() for e, a, rc in ROWS}
    with open(GOLDEN, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s (%d rows)" % (GOLDEN, len(table)))
