"""Device-code identity of two trees of this repository, kernel by kernel (no GPU needed).

    python tools/kernel_identity.py PARENT_TREE NEW_TREE [--jobs N] [--only a.hip,b.hip]\
        [--keep DIR] > profiles/<tag>_kernel_identity.txt

Every unit of build.py's UNITS in each tree is compiled device-only (hipcc --cuda-device-only
--no-gpu-bundle-output -c: a linked gfx950 code object), and every function symbol is reduced to
(size, sha1 of its instruction bytes).  Branches are pc-relative and the kernels reference no
other global symbol, so equal bytes mean equal code wherever the linker put the function.  The
report lists kernels per template in both trees, the kernels only one tree has, the kernels
whose bytes differ, and the total .text of both.
"""
from __future__ import annotations

import argparse
import collections
import concurrent.futures as cf
import hashlib
import importlib.util
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")


def load_build(tree):
    spec = importlib.util.spec_from_file_location(
        "gll_build_" + hashlib.sha1(tree.encode()).hexdigest()[:8],
        os.path.join(tree, "graphlearninglayer_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def compile_unit(b, unit, out):
    if os.path.exists(out):   # --keep: an earlier run's object
        return out
    cmd = [b.hipcc(), *b.FLAGS, "--cuda-device-only", "--no-gpu-bundle-output", "-c",
           os.path.join(b.CSRC, unit), "-o", out]
    subprocess.run(cmd, check=True, capture_output=True)
    return out


def functions(obj):
    """{mangled name: (size, sha1 of bytes)} of the code object's functions, and its .text size."""
    data = open(obj, "rb").read()
    sec = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-SW", obj], check=True,
                         capture_output=True, text=True).stdout
    m = re.search(r"\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", sec)
    addr, off, size = (int(x, 16) for x in m.groups())
    sym = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-sW", obj], check=True,
                         capture_output=True, text=True).stdout
    out = {}
    for line in sym.splitlines():
        f = line.split()
        if len(f) >= 8 and f[3] == "FUNC" and f[6] != "UND":
            v, sz = int(f[1], 16), int(f[2], 0)
            out[f[7]] = (sz, hashlib.sha1(data[off + v - addr: off + v - addr + sz]).hexdigest()[:12])
    return out, size


def demangle(names):
    filt = shutil.which("c++filt") or os.path.join(LLVM, "llvm-cxxfilt")
    r = subprocess.run([filt], input="\n".join(names), check=True,
                       capture_output=True, text=True).stdout.splitlines()
    return dict(zip(names, r))


def template_of(dem):
    return re.sub(r"^void ", "", dem).split("<")[0].split("(")[0]


def survey(tree, jobs, tmp, only):
    b = load_build(tree)
    objs = {}
    units = [u for u in b.UNITS if not only or u in only]
    with cf.ThreadPoolExecutor(jobs) as ex:
        futs = {u: ex.submit(compile_unit, b, u, os.path.join(tmp, u + ".co")) for u in units}
        for u, f in futs.items():
            objs[u] = f.result()
    fns, text = {}, {}
    for u, o in objs.items():
        fs, ts = functions(o)
        text[u] = ts
        for k, v in fs.items():
            fns[k] = (u, *v)
    return fns, text


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("--keep", default="", help="directory that keeps the code objects between runs")
    ap.add_argument("--only", default="", help="comma-separated unit files (default: every unit)")
    a = ap.parse_args()
    only = set(filter(None, a.only.split(",")))
    with tempfile.TemporaryDirectory() as t0, tempfile.TemporaryDirectory() as t1:
        if a.keep:
            t0, t1 = os.path.join(a.keep, "parent"), os.path.join(a.keep, "new")
            os.makedirs(t0, exist_ok=True)
            os.makedirs(t1, exist_ok=True)
        pf, pt = survey(os.path.abspath(a.parent), a.jobs, t0, only)
        nf, nt = survey(os.path.abspath(a.new), a.jobs, t1, only)
    dem = demangle(sorted(set(pf) | set(nf)))
    print("# .text bytes per unit")
    for tag, t in (("parent", pt), ("new", nt)):
        print(f"{tag:7s} total {sum(t.values()):9d}  " + "  ".join(f"{u}={s}" for u, s in t.items()))
    cp = collections.Counter(template_of(dem[k]) for k in pf)
    cn = collections.Counter(template_of(dem[k]) for k in nf)
    print("\n# kernels per template: parent / new")
    for k in sorted(set(cp) | set(cn)):
        print(f"{cp[k]:4d} {cn[k]:4d}  {k}")
    same = [k for k in pf if k in nf and pf[k][1:] == nf[k][1:]]
    diff = [k for k in pf if k in nf and pf[k][1:] != nf[k][1:]]
    gone = [k for k in pf if k not in nf]
    added = [k for k in nf if k not in pf]
    print(f"\n# parent {len(pf)} kernels, new {len(nf)}: {len(same)} identical (same mangled name, "
          f"size and bytes), {len(diff)} differ, {len(gone)} removed, {len(added)} added")
    for title, ks in (("differ", diff), ("removed", gone), ("added", added)):
        print(f"\n# {title}: {len(ks)}")
        for k in sorted(ks, key=lambda k: dem[k]):
            a_ = pf.get(k, ("-", 0, "-"))
            b_ = nf.get(k, ("-", 0, "-"))
            name = dem[k].split("(")[0]
            print(f"{a_[0]:>14s} {a_[1]:7d} {a_[2]:12s} | {b_[0]:>14s} {b_[1]:7d} {b_[2]:12s}  {name}")
    sys.exit(1 if diff else 0)


if __name__ == "__main__":
    main()
