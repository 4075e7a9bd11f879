#!/usr/bin/env python3
"""What hipcc makes of every kernel of csrc/specscan.hip in two checkouts, side by side — for changes that must leave the kernels alone.

    scripts/codegen_table.py BEFORE AFTER --out DIR        (BEFORE, AFTER: repository roots, e.g. two `git worktree`s)

Each checkout's specscan.hip is compiled device-only for gfx950 with the product's code-generation flags (build.FLAGS of that checkout)
and -Rpass-analysis=kernel-resource-usage, the two compilations side by side. Per kernel symbol: code size (the symbol's size in the
device code object), VGPRs, AGPRs, SGPRs, spilled VGPRs / SGPRs, scratch bytes per lane, LDS bytes per block (static: the step kernel's is
dynamic), occupancy in waves per SIMD, and a hash of the symbol's bytes in the code object (equal hashes: the same instructions, operand for
operand; a kernel whose code refers to something that moved — another symbol's address — differs here with every other column equal). DIR gets before.tsv, after.tsv and diff.txt: the kernels only one side has, and every kernel both
have whose rows differ. Exit status 1 if one of the latter exists. No GPU needed.
"""
from __future__ import annotations

import argparse
import hashlib
import importlib.util
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

COLUMNS = ["code_bytes", "vgprs", "agprs", "sgprs", "vgpr_spill", "sgpr_spill", "scratch", "lds", "occupancy", "code_hash"]
REMARKS = {"vgprs": r"VGPRs", "agprs": r"AGPRs", "sgprs": r"TotalSGPRs", "vgpr_spill": r"VGPRs Spill", "sgpr_spill": r"SGPRs Spill",
           "scratch": r"ScratchSize \[bytes/lane\]", "lds": r"LDS Size \[bytes/block\]", "occupancy": r"Occupancy \[waves/SIMD\]"}


def tool(name: str) -> str:
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for cand in (shutil.which(name), os.path.join(rocm, "bin", name), os.path.join(rocm, "lib", "llvm", "bin", name), os.path.join(rocm, "llvm", "bin", name)):
        if cand and os.path.exists(cand):
            return cand
    raise SystemExit(f"{name} not found")


def product_flags(root: str) -> list[str]:
    spec = importlib.util.spec_from_file_location("ss_build", os.path.join(root, "rtl-sdr-scanner-cpp_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return [f for f in mod.FLAGS if f.startswith(("--offload-arch", "-O", "-std", "-f")) and f != "-fPIC"]


def table(root: str, tmp: str, label: str) -> dict[str, dict[str, int | str]]:
    csrc = os.path.join(root, "rtl-sdr-scanner-cpp_amd", "csrc")
    obj, elf = os.path.join(tmp, label + ".o"), os.path.join(tmp, label + ".elf")
    out = subprocess.run([tool("hipcc"), *product_flags(root), "--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage", "-o", obj, "specscan.hip"],
                         cwd=csrc, capture_output=True, text=True)
    if out.returncode != 0:
        raise SystemExit(f"{label}: hipcc failed\n{out.stderr[-3000:]}")
    rows: dict[str, dict[str, int]] = {}
    for block in re.split(r"remark: Function Name: ", out.stderr)[1:]:
        name = block.split(" ")[0]
        rows[name] = {col: int(re.search(r"remark:\s+" + key + r": (\d+)", block).group(1)) for col, key in REMARKS.items()}
    # the device object is an offload bundle with one code object in it
    bundler = tool("clang-offload-bundler")
    targets = [t for t in subprocess.run([bundler, "--type=o", "--input=" + obj, "--list"], capture_output=True, text=True, check=True).stdout.split() if "amdgcn" in t]
    subprocess.run([bundler, "--type=o", "--targets=" + targets[0], "--input=" + obj, "--output=" + elf, "--unbundle"], check=True)
    # section number -> (address, file offset), to find a symbol's bytes in the file
    sections = {}
    for ln in subprocess.run([tool("llvm-readelf"), "-SW", elf], capture_output=True, text=True, check=True).stdout.splitlines():
        m = re.match(r"\s*\[\s*(\d+)\]\s+\S+\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s", ln)
        if m:
            sections[m.group(1)] = (int(m.group(2), 16), int(m.group(3), 16))
    image = open(elf, "rb").read()
    for ln in subprocess.run([tool("llvm-readelf"), "-sW", elf], capture_output=True, text=True, check=True).stdout.splitlines():
        f = ln.split()
        if len(f) == 8 and f[3] == "FUNC" and f[7] in rows:
            size, (addr, off) = int(f[2]), sections[f[6]]
            at = off + int(f[1], 16) - addr
            rows[f[7]]["code_bytes"] = size
            rows[f[7]]["code_hash"] = hashlib.sha256(image[at:at + size]).hexdigest()[:16]
    return rows


def write(path: str, rows: dict[str, dict[str, int | str]], demangled: dict[str, str]) -> None:
    with open(path, "w") as fh:
        fh.write("\t".join(["symbol", *COLUMNS, "name"]) + "\n")
        for name in sorted(rows):
            fh.write("\t".join([name, *[str(rows[name].get(c, -1)) for c in COLUMNS], demangled.get(name, "")]) + "\n")


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(2) as pool:
        fa = pool.submit(table, os.path.abspath(args.before), tmp, "before")
        fb = pool.submit(table, os.path.abspath(args.after), tmp, "after")
        a, b = fa.result(), fb.result()
    names = sorted(set(a) | set(b))
    filt = shutil.which("c++filt")
    plain = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True).stdout.split("\n") if filt else []
    demangled = dict(zip(names, plain)) if len(plain) >= len(names) else {}
    write(os.path.join(args.out, "before.tsv"), a, demangled)
    write(os.path.join(args.out, "after.tsv"), b, demangled)
    changed = [n for n in names if n in a and n in b and a[n] != b[n]]
    with open(os.path.join(args.out, "diff.txt"), "w") as fh:
        fh.write(f"kernels: {len(a)} before, {len(b)} after, {len(set(a) & set(b))} in both; columns: {' '.join(COLUMNS)}\n")
        for title, only in (("only before", sorted(set(a) - set(b))), ("only after", sorted(set(b) - set(a)))):
            fh.write(f"\n{title}: {len(only)}\n")
            for n in only:
                fh.write(f"  {demangled.get(n, n)}\n")
        fh.write(f"\nin both, rows differ: {len(changed)}\n")
        for n in changed:
            fh.write(f"  {demangled.get(n, n)}\n    differ: {' '.join(c for c in COLUMNS if a[n].get(c) != b[n].get(c))}\n    before {a[n]}\n    after  {b[n]}\n")
    print(open(os.path.join(args.out, "diff.txt")).read())
    return 1 if changed else 0


if __name__ == "__main__":
    sys.exit(main())
