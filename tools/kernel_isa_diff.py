#!/usr/bin/env python3
"""Are the gfx950 kernels of two builds of librsx_hip.so the same code?

    python tools/kernel_isa_diff.py OLD.so NEW.so

Extracts the gfx950 code objects of each library (one per translation unit with device code), disassembles them with the ROCm
llvm-objdump and compares, kernel by kernel: the instruction text (addresses, encodings and branch-target annotations stripped)
and the kernel descriptor's LDS, scratch, kernarg and register words.  Kernels are matched by demangled name, whichever unit
they sit in; a compiler-added suffix (the unit id of an internalised symbol) is dropped.  An equality comparison of two listings:
what a refactor that moves kernels between units runs to show that it moved them and nothing else.  Exit status 1 on a difference."""
import os
import re
import shutil
import struct
import subprocess
import sys
import tempfile

from build_variant import llvm_tool

TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
# kernel descriptor (64 bytes, llvm AMDGPUUsage "Kernel Descriptor"): the code entry offset (bytes 16..23) depends on the layout
KD_FIELDS = (("lds", 0, "<I"), ("scratch", 4, "<I"), ("kernarg", 8, "<I"), ("rsrc3", 44, "<I"), ("rsrc1", 48, "<I"), ("rsrc2", 52, "<I"),
             ("properties", 56, "<H"), ("kernarg_preload", 58, "<H"))


def run(tool, *args, cwd=None):
    return subprocess.check_output([llvm_tool(tool)] + list(args), text=True, cwd=cwd)


def code_objects(lib, work):
    """the library's gfx950 code objects, extracted into `work`"""
    name = os.path.basename(lib)
    shutil.copy(lib, os.path.join(work, name))
    run("llvm-objdump", "--offloading", name, cwd=work)
    return sorted(os.path.join(work, f) for f in os.listdir(work) if f.startswith(name + ".") and f.endswith(TARGET))


def plain_name(mangled):
    return re.sub(r"\.(intern|llvm|uniq)?\.?[0-9a-f]{8,}$", "", mangled)


def descriptors(obj):
    """{kernel symbol: {field: value}} from the .kd objects in .rodata"""
    syms = {}
    for row in (line.split() for line in run("llvm-readelf", "--dyn-syms", "-W", obj).splitlines()):
        if len(row) == 8 and row[7].endswith(".kd"):
            syms[row[7][:-3]] = int(row[1], 16)
    data = {}
    for line in run("llvm-objdump", "-s", "--section=.rodata", obj).splitlines():
        m = re.match(r"^ ([0-9a-f]+) ((?:[0-9a-f]+ ){1,4})", line)
        if m:
            raw = bytes.fromhex(m.group(2).replace(" ", ""))
            for i, byte in enumerate(raw):
                data[int(m.group(1), 16) + i] = byte
    out = {}
    for k, addr in syms.items():
        kd = bytes(data[addr + i] for i in range(64))
        out[k] = {name: struct.unpack_from(fmt, kd, off)[0] for name, off, fmt in KD_FIELDS}
    return out


def kernels(lib):
    """{demangled kernel name: (instruction lines, descriptor fields)} over every code object of the library"""
    work = tempfile.mkdtemp(prefix="rsx_isa_")
    try:
        found = {}
        for obj in code_objects(lib, work):
            kds = descriptors(obj)
            text, cur = {}, None
            for line in run("llvm-objdump", "-d", "--no-show-raw-insn", obj).splitlines():
                m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
                if m:
                    cur = text.setdefault(m.group(1), [])
                elif cur is not None and line.startswith("\t"):
                    cur.append(re.sub(r"\s*//.*$", "", line).strip())
            names = sorted(kds)
            filt = llvm_tool("llvm-cxxfilt") or shutil.which("c++filt")   # (neither: the mangled names serve as well)
            plain = [plain_name(n) for n in names]
            demangled = subprocess.check_output([filt] + plain, text=True).splitlines() if filt else plain
            for n, d in zip(names, demangled):
                if d in found:
                    raise SystemExit(f"{lib}: kernel {d} is defined in two code objects")
                found[d] = (text[n], kds[n])
        return found
    finally:
        shutil.rmtree(work, ignore_errors=True)


def main(old_lib, new_lib):
    old, new = kernels(old_lib), kernels(new_lib)
    gone, added = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    differ = []
    for k in sorted(set(old) & set(new)):
        what = []
        if old[k][0] != new[k][0]:
            n = next((i for i, (a, b) in enumerate(zip(old[k][0], new[k][0])) if a != b), min(len(old[k][0]), len(new[k][0])))
            what.append(f"code ({len(old[k][0])} -> {len(new[k][0])} instructions, first difference at {n})")
        what += [f"{f} {old[k][1][f]:#x} -> {new[k][1][f]:#x}" for f, _, _ in KD_FIELDS if old[k][1][f] != new[k][1][f]]
        if what:
            differ.append((k, what))
    for k in gone:
        print("only in", old_lib + ":", k)
    for k in added:
        print("only in", new_lib + ":", k)
    for k, what in differ:
        print("differs:", k, "|", "; ".join(what))
    same = len(set(old) & set(new)) - len(differ)
    print(f"kernel_isa_diff: {len(old)} kernels in {old_lib}, {len(new)} in {new_lib}: "
          f"{same} identical, {len(differ)} differ, {len(gone)} only old, {len(added)} only new")
    return 1 if gone or added or differ else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        raise SystemExit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
