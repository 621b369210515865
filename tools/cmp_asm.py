"""Device assembly of two source trees, kernel by kernel (no GPU needed): the
check of a change that must leave every kernel's code as it was.

usage: python tools/cmp_asm.py [--pair OLD=NEW ...] <git ref or directory of the old tree> [directory of the new tree, default .]

Every fpm-opencv_amd/csrc/*.hip of both trees is compiled with the Makefile's
flags (the max-memory-clause scheduler for MMC_FILES) to device assembly;
functions are matched by mangled name across files, so a kernel that moved to
another file is compared with itself.  Branch labels are renumbered in order of
appearance; comments, debug and section directives are dropped.  The kernel
descriptors (registers, LDS, scratch) are compared as well.  Exit 1 on any
difference.

--pair OLD=NEW (repeatable; mangled names) compares a kernel whose name changed
with its predecessor: the old tree's OLD against the new tree's NEW, with the
name substituted in body and descriptor.  For every function that differs, the
instruction counts of both sides and whether the descriptors are equal are
printed.
"""
import argparse
import glob
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

FLAGS = "--offload-arch=gfx950 -O3 -fno-slp-vectorize -std=c++17 -fPIC -I../include --cuda-device-only -S".split()
MMC = "-mllvm -amdgpu-sched-strategy=max-memory-clause".split()
MMC_FILES = {"np1024"}


def checkout(ref, dst):
    tar = subprocess.run(["git", "archive", ref, "fpm-opencv_amd/csrc", "include"], check=True, capture_output=True)
    subprocess.run(["tar", "-x", "-C", dst], input=tar.stdout, check=True)
    return dst


def assemble(tree, out):
    src = sorted(glob.glob(os.path.join(tree, "fpm-opencv_amd", "csrc", "*.hip")))

    def one(f):
        b = os.path.basename(f)[:-4]
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), *FLAGS, *(MMC if b in MMC_FILES else []),
                        os.path.join("csrc", b + ".hip"), "-o", os.path.join(out, b + ".s")],
                       check=True, cwd=os.path.join(tree, "fpm-opencv_amd"), stderr=subprocess.DEVNULL)

    with ThreadPoolExecutor(8) as ex:
        list(ex.map(one, src))


def normalise(body):
    lines = [l.split(";")[0].rstrip() for l in body]
    # (section directives: a function that became a template lies in a comdat section of its own)
    drop = (".p2align", ".loc", ".file", ".cfi", ".text", ".section")
    lines = [l for l in lines if l.strip() and not l.strip().startswith(drop)]
    text = "\n".join(lines)
    labels = {}
    for m in re.finditer(r"\.LBB\d+_\d+", text):
        labels.setdefault(m.group(0), f".L{len(labels)}")
    text = re.sub(r"\.LBB\d+_\d+", lambda m: labels[m.group(0)], text)
    return re.sub(r"\.L(tmp|func_begin|func_end|__unnamed_)\d+", r".L\1N", text)


def functions(d):
    """mangled name -> (file, normalised body, kernel descriptor)"""
    out = {}
    for f in sorted(glob.glob(os.path.join(d, "*.s"))):
        text = open(f).read()
        desc = dict(re.findall(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S))
        name, body = None, []
        for line in text.splitlines():
            m = re.match(r"^(_Z\w+):", line)
            if m and name is None:
                name, body = m.group(1), []
            elif name and line.startswith(".Lfunc_end"):
                out[name] = (os.path.basename(f), normalise(body), desc.get(name, ""))
                name = None
            elif name:
                body.append(line)
    return out


def instructions(body):
    return sum(1 for l in body.splitlines() if l.startswith("\t") and not l.lstrip().startswith("."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pair", action="append", default=[], metavar="OLD=NEW")
    ap.add_argument("old")
    ap.add_argument("new", nargs="?", default=".")
    args = ap.parse_args()
    old, new = args.old, os.path.abspath(args.new)
    pairs = dict(p.split("=", 1) for p in args.pair)
    with tempfile.TemporaryDirectory() as tmp:
        if not os.path.isdir(old):
            os.mkdir(os.path.join(tmp, "old"))
            old = checkout(old, os.path.join(tmp, "old"))
        dirs = []
        for tag, tree in (("a", old), ("b", new)):
            dirs.append(os.path.join(tmp, tag))
            os.mkdir(dirs[-1])
            assemble(os.path.abspath(tree), dirs[-1])
        a, b = functions(dirs[0]), functions(dirs[1])
    for o, n in pairs.items():  # the old tree's kernel under its successor's name
        if o not in a or n not in b:
            sys.exit(f"--pair {o}={n}: " + (f"{o} is not in the old tree" if o not in a else f"{n} is not in the new tree"))
        f, body, desc = a.pop(o)
        a[n] = (f, body.replace(o, n), desc.replace(o, n))
    renamed = {n: o for o, n in pairs.items()}
    bad = 0
    for k in sorted(set(a) | set(b)):
        if k not in a or k not in b:
            print("only in the", "new" if k in b else "old", "tree:", k)
            bad += 1
            continue
        same = a[k][1:] == b[k][1:]
        bad += not same
        print("same     " if same else "DIFFERENT", f"{a[k][0]} -> {b[k][0]}", len(a[k][1].splitlines()), k,
              f"(was {renamed[k]})" if k in renamed else "")
        if not same:
            print(f"          instructions {instructions(a[k][1])} -> {instructions(b[k][1])}, descriptor",
                  "equal" if a[k][2] == b[k][2] else "DIFFERENT")
    print(f"{len(a)} / {len(b)} functions, {bad} differ")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
