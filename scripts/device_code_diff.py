"""Compares the gfx950 device code of two builds of the library, kernel by kernel: for a change that must leave the GPU's
instructions alone (host-side refactors, header moves).

    python scripts/device_code_diff.py <build dir A> <build dir B> [out.txt]      (build dir = mc_nerf_amd/build of a tree)

Per object of build.SOURCES the gfx950 code object is extracted (llvm-objdump --offloading) and, per kernel symbol, compared:
the set of kernels; the sequence of (encoding, instruction text) of each kernel -- addresses and the order of kernels inside
an object are not compared, a host-side change of instantiation order permutes them; the kernel's metadata note (register
counts, LDS, scratch, kernarg size and argument offsets).  One line per kernel; exit status 1 unless every line says identical.
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mc_nerf_amd import build  # noqa: E402

LLVM = "/opt/rocm/lib/llvm/bin"


def device_elf(obj_path, tmp):
    local = os.path.join(tmp, os.path.basename(obj_path))
    shutil.copy(obj_path, local)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", local], check=True, capture_output=True)
    elf = [f for f in os.listdir(tmp) if f.startswith(os.path.basename(obj_path)) and "gfx950" in f]
    return os.path.join(tmp, elf[0]) if elf else None      # (a translation unit without device code has none)


def kernels(elf):
    """{kernel symbol: ([(encoding, instruction)], metadata note text)}"""
    if elf is None:
        return {}
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", elf], check=True, capture_output=True, text=True).stdout
    meta = {}
    for blk in notes.split("- .agpr_count:")[1:]:
        blk = blk.split("amdhsa.target:")[0]
        meta[re.search(r"\.name:\s+(\S+)", blk).group(1)] = "\n".join(sorted(l.strip() for l in blk.split("\n") if l.strip()))
    dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", elf], check=True, capture_output=True, text=True).stdout
    parts = re.split(r"\n[0-9a-f]+ <([^>\n]+)>:\n", dis)
    code = {}
    for name, body in zip(parts[1::2], parts[2::2]):
        ins = []
        for line in body.split("\n"):
            m = re.match(r"\s*(.*?)\s*//\s*[0-9A-Fa-f]+:\s*(.*)$", line)
            if m:
                ins.append((m.group(2).strip(), m.group(1)))
        code[name] = ins
    return {k: (code.get(k), meta[k]) for k in meta}


def main():
    dir_a, dir_b = sys.argv[1:3]
    out = open(sys.argv[3], "w") if len(sys.argv) > 3 else sys.stdout
    different = 0
    for src in build.SOURCES:
        obj = src.replace(".hip", ".o")
        with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
            ka, kb = kernels(device_elf(os.path.join(dir_a, obj), ta)), kernels(device_elf(os.path.join(dir_b, obj), tb))
        for name in sorted(set(ka) | set(kb)):
            if name not in ka or name not in kb:
                verdict = "ONLY IN " + ("A" if name in ka else "B")
            else:
                (ca, ma), (cb, mb) = ka[name], kb[name]
                what = [w for w, same in (("instructions", ca is not None and ca == cb), ("metadata", ma == mb)) if not same]
                verdict = "identical" if not what else "DIFFERENT " + " + ".join(what)
            different += verdict != "identical"
            n = len(ka[name][0] or ()) if name in ka else 0
            print(f"{obj:18s} {name:75s} {n:7d} instructions  {verdict}", file=out)
    print(f"{different} kernel(s) not identical", file=out)
    return 1 if different else 0


if __name__ == "__main__":
    sys.exit(main())
