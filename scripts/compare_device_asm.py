#!/usr/bin/env python3
"""Compare the gfx950 device code of the kernel files between two source trees (a refactor's parent and its head).

    scripts/compare_device_asm.py PARENT_TREE HEAD_TREE [--shapes "8,2 33,4" | --matrix] [--units mk_kernels,mk_split]
                                  [--jobs 8] [--keep DIR] [--rename 'REGEX=REPLACEMENT' ...]

Every unit (mk_kernels.hip, mk_split.hip, mk_dk.hip and the seven slices of mk_wide.hip) is compiled in both trees with the
Makefile's flags plus --cuda-device-only -S: once with the tree's default MK_SHAPES and once per listed shape as a
single-shape module (-DMK_SHAPE_MODULE '-DMK_SHAPES(X)=X(N,K)'; --matrix lists tests/shape_matrix.py::MATRIX of the head).
The assembly is compared as text after dropping the __hip_cuid_ lines (a hash of the file) and applying the --rename
substitutions to the HEAD's text, which map a kernel that was renamed or split off back to its old mangled name (the
names of its __shared__ variables carry the same prefix).  Prints the count of differing lines per output and exits
non-zero if any differ.  Needs hipcc, no GPU.  --keep DIR keeps the assembly under DIR/<tree name>/ and reuses what a
previous run left there that is newer than every source of its tree.
"""
import argparse
import concurrent.futures
import difflib
import os
import re
import subprocess
import sys
import tempfile

UNITS = ["mk_kernels", "mk_split", "mk_dk"] + ["mk_wide:%d" % p for p in range(7)]
# the one-model-per-wavefront filter was filter_kernel<N, K, 64, ...> before it became a kernel of its own
DEFAULT_RENAMES = [r"18filter_wave_kernelILi(\d+)ELi(\d+)E=13filter_kernelILi\1ELi\2ELi64E"]


def flags(tree):  # metran_amd/csrc/Makefile: CXXFLAGS
    return ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-I%s/include" % tree,
            "-I%s/metran_amd/csrc" % tree, "-Wall", "-Wno-unused-parameter", "--cuda-device-only", "-S"]


def newest_source(tree):
    dirs = [os.path.join(tree, "metran_amd", "csrc"), os.path.join(tree, "include")]
    return max(os.path.getmtime(os.path.join(d, f)) for d in dirs for f in os.listdir(d))


def compile_one(tree, unit, shape, out, stamp):
    if os.path.exists(out) and os.path.getmtime(out) > stamp:
        return out
    name, _, part = unit.partition(":")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + flags(tree)
    if part:
        cmd.append("-DMK_WIDE_PART=" + part)
    if shape:
        cmd += ["-DMK_SHAPE_MODULE", "-DMK_SHAPES(X)=X(%d,%d)" % shape]
    cmd += [os.path.join(tree, "metran_amd", "csrc", name + ".hip"), "-o", out + ".tmp"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError("%s\n%s" % (" ".join(cmd), r.stdout[-4000:]))
    os.replace(out + ".tmp", out)
    return out


def normalised(path, renames):
    with open(path) as f:
        lines = [ln for ln in f if "__hip_cuid_" not in ln]
    for pat, rep in renames:
        lines = [pat.sub(rep, ln) for ln in lines]
    return lines


def differing(a, b):
    if a == b:
        return 0
    sm = difflib.SequenceMatcher(None, a, b, autojunk=False)
    return sum(max(i2 - i1, j2 - j1) for tag, i1, i2, j1, j2 in sm.get_opcodes() if tag != "equal")


def functions(lines):
    """{symbol: its lines}, from a function's label to the next one's (the resource comments behind it included)."""
    out, cur = {}, None
    for ln in lines:
        m = re.match(r"^(_Z\w+):", ln)
        if m:
            cur = out.setdefault(m.group(1), [])
        if cur is not None:
            cur.append(ln)
    return out


RESOURCES = re.compile(r"^; (codeLenInByte|NumSgprs|NumVgprs|NumAgprs|ScratchSize|Occupancy|LDSByteSize)\b.*")


def detail(a, b):
    """Per function whose text differs: differing lines, whether the multiset of instructions (mnemonics) is the same,
    and the resource figures that changed."""
    fa, fb = functions(a), functions(b)
    for name in fa:
        if name not in fb or fa[name] == fb[name]:
            continue
        ops = lambda f: sorted(ln.split()[0] for ln in f if ln.startswith("\t") and not ln.startswith("\t.") and ln.split())
        res = lambda f: [ln.strip() for ln in f if RESOURCES.match(ln)]
        ra, rb = res(fa[name]), res(fb[name])
        print("    %s: %d of %d lines differ; instruction multiset %s; resources %s" % (
            name, differing(fa[name], fb[name]), len(fa[name]), "same" if ops(fa[name]) == ops(fb[name]) else "DIFFERENT",
            "same" if ra == rb else "; ".join("%s -> %s" % (x, y) for x, y in zip(ra, rb) if x != y)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent")
    ap.add_argument("head")
    ap.add_argument("--shapes", default="", help='single-shape modules to compare, "N,K N,K ..."')
    ap.add_argument("--matrix", action="store_true", help="add every shape of tests/shape_matrix.py::MATRIX (head tree)")
    ap.add_argument("--no-default", action="store_true", help="skip the default MK_SHAPES build")
    ap.add_argument("--units", default=",".join(UNITS), help="comma-separated subset of: " + " ".join(UNITS))
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--keep", default=None, help="directory that keeps (and supplies) the assembly")
    ap.add_argument("--rename", action="append", default=None, help="REGEX=REPLACEMENT applied to the head's assembly")
    ap.add_argument("--detail", action="store_true", help="per differing function: instruction multiset and resource usage")
    ap.add_argument("--only", choices=["parent", "head"], default=None, help="compile one side only (fills --keep), compare nothing")
    args = ap.parse_args()

    shapes = [tuple(int(v) for v in s.split(",")) for s in args.shapes.split()]
    if args.matrix:
        sys.path.insert(0, os.path.join(args.head, "tests"))
        import shape_matrix
        shapes += [s for s in shape_matrix.MATRIX if s not in shapes]
    configs = ([] if args.no_default else [None]) + shapes
    units = args.units.split(",")
    renames = [(re.compile(p), r) for p, _, r in (s.partition("=") for s in (args.rename or DEFAULT_RENAMES))]
    keep = args.keep or tempfile.mkdtemp(prefix="device_asm_")
    trees = {"parent": os.path.abspath(args.parent), "head": os.path.abspath(args.head)}
    sides = [args.only] if args.only else ["parent", "head"]

    jobs = {}
    with concurrent.futures.ThreadPoolExecutor(args.jobs) as pool:
        for side in sides:
            stamp = newest_source(trees[side])
            os.makedirs(os.path.join(keep, side), exist_ok=True)
            for shape in configs:
                for unit in units:
                    tag = "%s.%s" % (unit.replace(":", "_p"), "default" if shape is None else "%d_%d" % shape)
                    out = os.path.join(keep, side, tag + ".s")
                    jobs[(side, tag)] = pool.submit(compile_one, trees[side], unit, shape, out, stamp)
        for f in concurrent.futures.as_completed(list(jobs.values())):
            f.result()
    if args.only:
        print("compiled %d outputs of the %s into %s" % (len(jobs), args.only, keep))
        return 0

    total = 0
    for tag in sorted({t for _, t in jobs}):
        a = normalised(jobs[("parent", tag)].result(), [])
        b = normalised(jobs[("head", tag)].result(), renames)
        d = differing(a, b)
        total += d
        print("%-28s %8d lines  %6d differing" % (tag, len(a), d))
        if d and args.detail:
            detail(a, b)
    print("total differing lines: %d in %d outputs" % (total, len(jobs) // 2))
    return 1 if total else 0


if __name__ == "__main__":
    sys.exit(main())
