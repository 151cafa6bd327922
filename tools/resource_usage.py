#!/usr/bin/env python3
"""Per-kernel resource table from a build log (CPU only).

Build the device objects with the compiler's remarks on and the output grouped
per target, e.g.

  make -C word2vec_amd/csrc -j8 -O HIPFLAGS="--offload-arch=gfx950 -O3 -std=c++17 \\
      -fPIC -ffp-contract=off -Wall -Rpass-analysis=kernel-resource-usage" 2> build.log

then `tools/resource_usage.py build.log > table.txt`. One line per kernel:
object, VGPRs, AGPRs, scratch bytes per lane, LDS bytes per block, occupancy
(waves per SIMD), demangled name; sorted, so two trees' tables diff line by
line. Kernels outside namespace w2v (the rocPRIM instantiations of the ingest
and phrase units, ~1,450 of them) are folded into one line per object: their
count and a hash over their figures and names.
With --insts OBJDIR the gfx950 instruction count of each kernel is added.
"""
import argparse
import hashlib
import re
import subprocess
import tempfile
from pathlib import Path

LLVM = Path("/opt/rocm/lib/llvm/bin")
FIELDS = ["VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]"]


def inst_counts(obj: Path) -> dict:
    with tempfile.TemporaryDirectory() as t:
        dst = Path(t) / obj.name
        dst.write_bytes(obj.read_bytes())
        subprocess.run([str(LLVM / "llvm-objdump"), "--offloading", str(dst)], check=True, capture_output=True, cwd=t)
        dev = [p for p in Path(t).iterdir() if p.name.startswith(obj.name + ".") and "gfx950" in p.name]
        if len(dev) != 1:
            return {}
        asm = subprocess.run([str(LLVM / "llvm-objdump"), "-d", str(dev[0])], check=True, capture_output=True,
                             text=True).stdout
    out, cur = {}, None
    for line in asm.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = m.group(1)
            out[cur] = 0
        elif cur and "//" in line:
            out[cur] += 1
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("log")
    ap.add_argument("--insts", metavar="OBJDIR", help="add each kernel's instruction count from the objects here")
    a = ap.parse_args()
    rows, obj, cur = [], "?", None
    for line in Path(a.log).read_text(errors="replace").splitlines():
        m = re.search(r"hipcc .* -o \S*/([\w.]+\.o) ", line)
        if m:
            obj = m.group(1)
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = {"obj": obj, "name": m.group(1)}
            rows.append(cur)
            continue
        m = re.search(r"remark:\s+(.+?): (\S+) \[-Rpass", line)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2)
    names = subprocess.run(["c++filt"], input="\n".join(r["name"] for r in rows), check=True,
                           capture_output=True, text=True).stdout.splitlines()
    counts = {}
    print("# object vgprs agprs scratch_B lds_B occupancy" + (" insts" if a.insts else "") + " kernel")
    lines, lib = [], {}
    for r, dem in zip(rows, names):
        cols = [r["obj"]] + [r.get(f, "?") for f in FIELDS]
        if a.insts:
            if r["obj"] not in counts:
                counts[r["obj"]] = inst_counts(Path(a.insts) / r["obj"])
            cols.append(str(counts[r["obj"]].get(r["name"], "?")))
        if re.match(r"(void )?w2v::", dem) and "rocprim" not in dem and "hipcub" not in dem:
            lines.append(" ".join(cols) + " " + dem)
        else:  # library kernels (rocPRIM instantiations): one line per object, below
            lib.setdefault(r["obj"], []).append(" ".join(cols[1:]) + " " + r["name"])
    for obj, rows_ in lib.items():
        digest = hashlib.sha1("\n".join(sorted(rows_)).encode()).hexdigest()[:16]
        lines.append(f"{obj} library kernels: {len(rows_)}, sha1 of their sorted figures and names {digest}")
    print("\n".join(sorted(lines)))


if __name__ == "__main__":
    main()
