"""Compares the gfx950 device code of two builds of the library, kernel by kernel: for a change that must leave the GPU's
instructions alone (host-side refactors, header moves, kernels moved between source files).

    python scripts/device_code_diff.py <build dir A> <build dir B> [out.txt]      (build dir = mc_nerf_amd/build of a tree)

From every *.o of a build directory the gfx950 code object is extracted (llvm-objdump --offloading) and its kernels collected by
symbol, whichever object holds them.  Per symbol are compared: the sequence of (encoding, instruction text) -- addresses, the
order of kernels inside an object and the padding behind a kernel's last instruction are not compared, they depend on its neighbours; the kernel's metadata
note (register counts, LDS, scratch, kernarg size and argument offsets).  One line per kernel, naming its object in A (and in B where
it moved); a kernel that differs, or that only one build has, also gets its instruction count and VGPR / SGPR / LDS / scratch figures of both builds.  Exit
status 1 unless every line says identical.
"""
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

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
        while ins and ins[-1][1].split()[0] in ("s_nop", "s_code_end"):      # padding up to the next symbol: depends on the neighbour
            ins.pop()
        code[name] = ins
    return {k: (code.get(k), meta[k]) for k in meta}


def build_kernels(build_dir):
    """{kernel symbol: (object name, [(encoding, instruction)], metadata note text)} over every *.o of a build directory"""
    out = {}
    for obj in sorted(glob.glob(os.path.join(build_dir, "*.o"))):
        with tempfile.TemporaryDirectory() as tmp:
            for name, (code, meta) in kernels(device_elf(obj, tmp)).items():
                if name in out:      # a kernel compiled into two libraries (ray_bounds.hip includes voxel.hip): the later copy is keyed with its object
                    name += " @" + os.path.basename(obj)
                assert name not in out, name
                out[name] = (os.path.basename(obj), code, meta)
    return out


def figures(code, meta):
    f = dict(re.findall(r"\.(vgpr_count|sgpr_count|group_segment_fixed_size|private_segment_fixed_size):\s+(\d+)", meta))
    return (f"{len(code or ())} instructions, {f['vgpr_count']} VGPR, {f['sgpr_count']} SGPR, {f['group_segment_fixed_size']} B LDS, "
            f"{f['private_segment_fixed_size']} B scratch")


def main():
    ka, kb = build_kernels(sys.argv[1]), build_kernels(sys.argv[2])
    out = open(sys.argv[3], "w") if len(sys.argv) > 3 else sys.stdout
    different = 0
    for name in sorted(set(ka) | set(kb), key=lambda k: ((ka.get(k) or kb[k])[0], k)):
        obj, code, meta = ka.get(name) or kb[name]
        if name not in ka or name not in kb:
            verdict = "ONLY IN " + ("A" if name in ka else "B") + f"  [{figures(code, meta)}]"
        else:
            ob, cb, mb = kb[name]
            obj += "" if ob == obj else " -> " + ob
            what = [w for w, same in (("instructions", code is not None and code == cb), ("metadata", meta == mb)) if not same]
            verdict = "identical" if not what else f"DIFFERENT {' + '.join(what)}  [A: {figures(code, meta)}]  [B: {figures(cb, mb)}]"
        different += verdict != "identical"
        print(f"{obj:18s} {name:75s} {len(code or ()):7d} instructions  {verdict}", file=out)
    print(f"{different} kernel(s) not identical", file=out)
    return 1 if different else 0


if __name__ == "__main__":
    sys.exit(main())
