#!/usr/bin/env python3
"""Compare the gfx950 device code of two csrc trees, kernel by kernel.

    python tools/kernel_identity.py PARENT/nerf_loc_amd/csrc nerf_loc_amd/csrc > profiles/<name>.txt

For every .hip in the Makefile's SRCS, in both trees: compile with the Makefile's FLAGS plus `--cuda-device-only -c`, unbundle the gfx950
code object, and take every kernel (a function symbol F with a 64-byte descriptor F.kd): its name, size, the sha256 of its code bytes and of
its descriptor — without the descriptor's kernel_code_entry_byte_offset (bytes 16-23), the distance from the descriptor to the code: it says where the unit's
layout put the kernel and moves for every kernel of a unit when another one is added or removed.  One line per kernel; exit status 1 if any kernel differs, is missing or is new.  The __hip_cuid_* marker is not a kernel
and is not looked at.  Nothing is disassembled: a refactor that claims "the same device code" is checked by hashes alone.

Each tree needs its include/ two levels up (csrc includes ../../include/nerfloc_render.h): for the parent, e.g.
    git archive HEAD~ nerf_loc_amd/csrc include | tar -x -C /tmp/parent
--work DIR keeps the code objects (DIR/a, DIR/b) and reuses one that is newer than every source file of its tree.
"""
import argparse
import hashlib
import os
import struct
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
TARGET = "hip-amdgcn-amd-amdhsa--gfx950"


def make_var(csrc, what):
    return subprocess.check_output(["make", "-s", "-C", csrc, what], text=True).split()


def rocm_tool(hipcc, name):
    for d in (os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "llvm", "bin"), os.path.dirname(os.path.realpath(hipcc))):
        if os.path.exists(os.path.join(d, name)):
            return os.path.join(d, name)
    return name


def code_object(csrc, src, flags, hipcc, out_dir):
    """Compile one unit for the device only; return the path of its gfx950 ELF."""
    co = os.path.join(out_dir, src[:-4] + ".co")
    newest = max(os.path.getmtime(os.path.join(csrc, f)) for f in os.listdir(csrc) if f.endswith((".hip", ".h")))
    if os.path.exists(co) and os.path.getmtime(co) > newest:
        return co
    obj = os.path.join(out_dir, src[:-4] + ".dev.o")
    subprocess.check_call([hipcc, *flags, "--cuda-device-only", "-c", os.path.join(csrc, src), "-o", obj])
    with open(obj, "rb") as f:
        bundled = f.read(len(BUNDLE_MAGIC)) == BUNDLE_MAGIC
    if bundled:
        subprocess.check_call([rocm_tool(hipcc, "clang-offload-bundler"), "--unbundle", "--type=o", f"--targets={TARGET}", f"--input={obj}", f"--output={co}"])
        os.remove(obj)
    else:
        os.replace(obj, co)
    return co


def kernels(path):
    """{kernel name: (size, sha256 of the code, sha256 of the .kd descriptor)} of one ELF64 code object."""
    with open(path, "rb") as f:
        d = f.read()
    assert d[:6] == b"\x7fELF\x02\x01", path
    shoff, = struct.unpack_from("<Q", d, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", d, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", d, shoff + i * shentsize) for i in range(shnum)]   # name, type, flags, addr, offset, size, link, info, align, entsize
    syms = {}
    for s in secs:
        if s[1] != 2:   # SHT_SYMTAB (a code object's .symtab holds every .dynsym entry too)
            continue
        strtab = secs[s[6]]
        for o in range(s[4], s[4] + s[5], 24):
            name, info, _, shndx, value, size = struct.unpack_from("<IBBHQQ", d, o)
            if 0 < shndx < shnum:
                n0 = strtab[4] + name
                syms[d[n0:d.index(b"\0", n0)].decode()] = (info & 0xF, shndx, value, size)

    def data(shndx, value, size):
        sec = secs[shndx]
        assert sec[1] != 8 and sec[3] <= value and value + size <= sec[3] + sec[5], path   # not SHT_NOBITS, inside the section
        return d[sec[4] + value - sec[3]:sec[4] + value - sec[3] + size]

    out = {}
    for name, (typ, shndx, value, size) in syms.items():
        kd = syms.get(name + ".kd")
        if typ != 2 or kd is None:   # STT_FUNC with a descriptor
            continue
        assert kd[3] == 64, (path, name)
        desc = data(*kd[1:])
        out[name] = (size, hashlib.sha256(data(shndx, value, size)).hexdigest(), hashlib.sha256(desc[:16] + bytes(8) + desc[24:]).hexdigest())
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("a", help="csrc of the parent")
    ap.add_argument("b", help="csrc of this tree")
    ap.add_argument("--work", help="directory for the code objects (default: a temporary one)")
    ap.add_argument("--only", nargs="*", help="units to compare (default: SRCS of tree b)")
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 1))
    args = ap.parse_args()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    tmp = None if args.work else tempfile.TemporaryDirectory()
    work = args.work or tmp.name
    srcs = args.only or make_var(args.b, "print-objs")
    srcs = [s[:-2] + ".hip" if s.endswith(".o") else s for s in srcs]
    trees = []
    for tag, csrc in (("a", args.a), ("b", args.b)):
        out_dir = os.path.join(work, tag)
        os.makedirs(out_dir, exist_ok=True)
        flags = make_var(csrc, "print-flags")
        have = [s for s in srcs if os.path.exists(os.path.join(csrc, s))]
        with ThreadPoolExecutor(args.jobs) as ex:
            cos = list(ex.map(lambda s: code_object(csrc, s, flags, hipcc, out_dir), have))
        trees.append({(s, k): v for s, co in zip(have, cos) for k, v in kernels(co).items()})
    a, b = trees
    same = diff = 0
    for key in sorted(set(a) | set(b)):
        ka, kb = a.get(key), b.get(key)
        if ka == kb:
            verdict = "same"
        elif ka is None or kb is None:
            verdict = "ONLY-IN-A" if kb is None else "ONLY-IN-B"
        else:
            verdict = "DIFF" + ("" if ka[0] == kb[0] else f" size {ka[0]}->{kb[0]}") + ("" if ka[1] == kb[1] else " code") + ("" if ka[2] == kb[2] else " kd")
        same += verdict == "same"
        diff += verdict != "same"
        k = kb or ka
        print(f"{verdict:9s} {key[0]:18s} {k[0]:7d} {k[1][:16]} {k[2][:16]} {key[1]}")
    print(f"# {len(srcs)} units, {same + diff} kernels: {same} identical, {diff} different")
    return 1 if diff or not same else 0


if __name__ == "__main__":
    sys.exit(main())
