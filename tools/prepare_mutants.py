"""Do the GPU tests of the batch preparation (tests/test_prepare_gpu.py) see a wrong VALUE?  Each mutant below is csrc/prepare.hip with
one rule changed to a near miss that reads and writes the same addresses - only values differ - built into a library of its own
(build_var/, git-ignored) beside the in-tree objects of everything else:
    python tools/prepare_mutants.py build                                   no GPU needed
    python tools/prepare_mutants.py run [--out profiles/r16/prepare_parity.txt]     on the GPU: the test file once per mutant
`run` loads each library through DMM_LIB_PATH and records which named cases fail.  A mutant no case catches is a hole in the tests.
A run that ends in a signal or a time limit stops the whole tool: nothing more is started on the device."""
import argparse
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dmmfods_amd", "csrc")
OUT = os.path.join(ROOT, "build_var")
FLAGS = "-O3 -std=c++17 -fPIC --offload-arch=gfx950 -munsafe-fp-atomics -Wno-unused-result -Wno-unused-value".split()

# name -> (what it is, [(text in prepare.hip - exactly one occurrence, its replacement)])
MUTANTS = {
    "reciprocal": ("image: a multiplication with the reciprocal in place of the division",
                   [("__fdiv_rn((float)sum, den)", "((float)sum * __fdiv_rn(1.0f, den))")]),
    "fma": ("LiDAR code: one fused multiply-add in place of two roundings",
            [("near + 255.f : far + 150.f", "fmaf(e, -6.2f, 255.f) : fmaf(e, -2.f, 150.f)")]),
    "clip_h": ("LiDAR splat: the upper clip H / W in place of H - 1 / W - 1",
               [("row >= a.H - 1 || col >= a.W - 1", "row >= a.H || col >= a.W")]),
    "first_point": ("LiDAR splat: the first writer (lowest point index) in place of the last",
                    [("atomicMax(a.owner + b * ((size_t)a.H * (size_t)a.W) + (size_t)row * (size_t)a.W + (size_t)col, g);",
                      "atomicMin((unsigned*)(a.owner + b * ((size_t)a.H * (size_t)a.W) + (size_t)row * (size_t)a.W + (size_t)col), (unsigned)g);")]),
    "first_box": ("heat maps: the first box of a class in list order in place of the last",
                  [("for (int n = culled - 1; n >= 0 && found != 7u; --n) {", "for (int n = 0; n < culled && found != 7u; ++n) {")]),
    "own_window": ("LiDAR pool: the padded bottom row from row Ho - 1's own window (cut at the plane's end) in place of row Ho - 2's",
                   [("const int r = min(i, a.Ho - 2);", "const int r = i;"),
                    ("for (int dy = 0; dy < 2 * a.p; ++dy)", "for (int dy = 0; dy < 2 * a.p && y0 + dy < (size_t)a.H; ++dy)")]),
    "side_gt": ("heat maps: c > 3 * wf in place of c >= 3 * wf in the pedestrian pattern",
                [("c >= 3 * wf", "c > 3 * wf")]),
}


def lib_path(name):
    return os.path.join(OUT, f"lib_prep_{name}.so")


def build():
    os.makedirs(OUT, exist_ok=True)
    subprocess.run(["make", "-C", CSRC, "-j", "8"], check=True)
    src = open(os.path.join(CSRC, "prepare.hip")).read()
    objs = re.search(r"^OBJS = (.*)$", open(os.path.join(CSRC, "Makefile")).read(), re.M).group(1).split()
    for name, (_, edits) in MUTANTS.items():
        text = src
        for old, new in edits:
            assert text.count(old) == 1, (name, old, text.count(old))
            text = text.replace(old, new)
        hip, obj = os.path.join(OUT, f"prepare_{name}.hip"), os.path.join(OUT, f"prepare_{name}.o")
        with open(hip, "w") as f:
            f.write(text)
        subprocess.run(["hipcc"] + FLAGS + ["-I", CSRC, "-c", hip, "-o", obj], check=True)
        subprocess.run(["hipcc", "--offload-arch=gfx950", "-shared", "-o", lib_path(name)] +
                       [obj if o == "prepare.o" else os.path.join(CSRC, o) for o in objs], check=True)
        print("built", lib_path(name))


def run(out):
    lines = ["tests/test_prepare_gpu.py (without the agent's test) against libraries whose prepare.hip has ONE rule changed (tools/prepare_mutants.py);",
             "per mutant the cases that fail.  The unchanged library passes every case.", ""]
    for name, (what, _) in [("(none)", ("the library as it is", None))] + list(MUTANTS.items()):
        env = dict(os.environ)
        if name != "(none)":
            env["DMM_LIB_PATH"] = lib_path(name)
            assert os.path.exists(lib_path(name)), f"{lib_path(name)}: run `build` first"
        r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_prepare_gpu.py"), "-m", "gpu",
                            "-q", "-k", "not agent", "-p", "no:cacheprovider"], env=env, capture_output=True, text=True, cwd=ROOT)
        failed = re.findall(r"^FAILED tests/test_prepare_gpu\.py::(\S+)", r.stdout, re.M)   # (the test ids hold no blanks)
        tail = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ""
        lines.append(f"{name}: {what}")
        lines.append(f"  exit {r.returncode}; {tail.strip('= ')}")
        lines += [f"  caught by {t}" for t in failed] or ["  caught by nothing"]
        print("\n".join(lines[-(2 + max(1, len(failed))):]), flush=True)
        if r.returncode not in (0, 1):
            lines.append(f"  stopped: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            break
    text = "\n".join(lines) + "\n"
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text)
    return 0 if lines[-1].startswith("  caught") else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("build", "run"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.mode == "build":
        build()
    else:
        sys.exit(run(a.out))
