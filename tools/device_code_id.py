"""Identity of the library's device code: for each object of the Makefile's OBJS, sha256 (first 16 hex digits) of the .text section,
of the .rodata section (the kernel descriptors) and of the `llvm-readelf --notes` text (the code-object metadata: kernel names,
registers, LDS, arguments) of the gfx950 device code, built device-side only and unbundled with the Makefile's own commands.  Two
trees whose tables are equal run the same GPU code; the whole ELF is not compared because its symbol table differs between two
builds of one source.

  python tools/device_code_id.py [csrc directory of another checkout] [-j N]
"""
import argparse
import concurrent.futures
import hashlib
import os
import shlex
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")


def compile_commands(csrc):
    """{object: argv} from a dry run of the Makefile, so that the flags are the Makefile's."""
    objs = subprocess.run(["make", "-s", "-f", "Makefile", "-f", "-", "print-objs"], cwd=csrc, check=True, capture_output=True, text=True,
                          input="print-objs:\n\t@echo $(OBJS)\n").stdout.split()
    dry = subprocess.run(["make", "-n", "-B"] + objs, cwd=csrc, check=True, capture_output=True, text=True).stdout
    cmds = {}
    for line in dry.splitlines():
        argv = shlex.split(line)
        if "-c" in argv and "-o" in argv:
            cmds[argv[argv.index("-o") + 1]] = argv
    missing = [o for o in objs if o not in cmds]
    if missing:
        raise SystemExit("no compile command found for: " + " ".join(missing))
    return objs, cmds


def sha(data):
    return hashlib.sha256(data).hexdigest()[:16]


def identify(csrc, obj, argv, tmp):
    out = os.path.join(tmp, obj)
    argv = list(argv)
    argv[argv.index("-o") + 1] = out
    subprocess.run(argv + ["--cuda-device-only", "--no-gpu-bundle-output"], cwd=csrc, check=True)
    ids = []
    for sec in (".text", ".rodata"):
        dump = out + sec
        r = subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", sec + "=" + dump, out, out + ".copy"], capture_output=True)
        ids.append(sha(open(dump, "rb").read()) if r.returncode == 0 else "-" * 16)  # (an object without kernels has no such section)
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", out], check=True, capture_output=True).stdout
    ids.append(sha(notes.replace(out.encode(), obj.encode())))
    return ids


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("csrc", nargs="?", default=os.path.join(ROOT, "dmmfods_amd", "csrc"))
    ap.add_argument("-j", type=int, default=min(16, os.cpu_count() or 1))
    a = ap.parse_args()
    csrc = os.path.abspath(a.csrc)
    objs, cmds = compile_commands(csrc)
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(a.j) as pool:
        rows = list(pool.map(lambda o: identify(csrc, o, cmds[o], tmp), objs))
    print("%-16s %-16s %-16s %-16s" % ("object", ".text", ".rodata", "notes"))
    for o, r in zip(objs, rows):
        print("%-16s %s %s %s" % (o, *r))


if __name__ == "__main__":
    main()
