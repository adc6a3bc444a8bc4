#!/usr/bin/env python3
"""Static report of the gfx950 device code of a built object: how much of each kernel is register-spill
traffic, and how much of that sits inside loops.

    python3 profiles/static_report.py fuzzy-aho-corasick-rs_amd/csrc/build/search_kernels.o [name-regex]

The object's gfx950 code object is taken out of its .hip_fatbin (as profiles/kernel_resources.sh does)
and disassembled. Per kernel symbol (a symbol with a kernel descriptor in the code object's notes) one
line:

  insts      instructions of the symbol
  loop / deep  of those, instructions inside a loop / inside four or more nested loops (the window
             kernels' batch loop and what it contains). A loop is the address range between a backward
             branch and its target; an instruction's depth is the number of such ranges that hold it.
  rdl        v_readlane_b32 with a constant lane (the reload of a spilled SGPR), all / in loops / deep
  wrl        v_writelane_b32 (the spill of an SGPR into a VGPR lane), all / in loops / deep
  scr        instructions whose mnemonic begins scratch_ (VGPR spills and stack slots), all / in loops / deep
  vgpr sgpr scratch lds   from the kernel descriptor notes

It counts spill traffic only. Nothing is run; the numbers say what the allocator did, not what a wave
executes.
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"

INST = re.compile(r"^\t(\S+)\s*(.*?)\s*// ([0-9A-F]+): ")
SYM = re.compile(r"^[0-9a-f]+ <(\S+)>:$")


def code_object(obj, tmp):
    fb, co = os.path.join(tmp, "fb"), os.path.join(tmp, "co")
    with open(obj, "rb") as f:
        head = f.read(24)
    if head[:4] == b"\x7fELF" and head[18:20] == b"\xe0\x00":  # EM_AMDGPU: a code object, as it is
        return obj
    if head.startswith(b"__CLANG_OFFLOAD_BUNDLE__"):  # a device-only compile's bundle
        fb = obj
    else:
        subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fb}", obj], check=True)
    subprocess.run([f"{LLVM}/clang-offload-bundler", "--type=o", f"--input={fb}", f"--output={co}", "--unbundle",
                    f"--targets={TARGET}"], check=True)
    return co


def kernel_notes(co):
    """kernel symbol -> (vgpr, sgpr, scratch bytes, lds bytes)"""
    txt = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
    out = {}
    for blk in txt.split("- .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        if not name:
            continue
        g = lambda k: (re.search(r"\." + k + r":\s+(\S+)", blk) or [None, "?"])[1]  # noqa: E731
        out[name.group(1)] = tuple(g(k) for k in ("vgpr_count", "sgpr_count", "private_segment_fixed_size",
                                                  "group_segment_fixed_size"))
    return out


def functions(co):
    """symbol -> list of (address, mnemonic, operands)"""
    txt = subprocess.run([f"{LLVM}/llvm-objdump", "-d", co], check=True, capture_output=True, text=True).stdout
    funcs, cur = {}, None
    for line in txt.splitlines():
        m = SYM.match(line)
        if m:
            cur = funcs.setdefault(m.group(1), [])
            continue
        m = INST.match(line)
        if m and cur is not None:
            cur.append((int(m.group(3), 16), m.group(1), m.group(2)))
    return funcs


def depths(insts):
    """loop depth of every instruction: the backward branches whose range [target, branch] holds it"""
    loops = []
    for addr, mn, ops in insts:
        if mn.startswith("s_cbranch") or mn == "s_branch":
            try:
                imm = int(ops.split()[-1])
            except ValueError:
                continue
            if imm >= 0x8000:
                imm -= 0x10000
            target = addr + 4 + 4 * imm
            if target <= addr:
                loops.append((target, addr))
    return [sum(1 for lo, hi in loops if lo <= addr <= hi) for addr, _, _ in insts]


def report(name, insts, notes):
    d = depths(insts)
    cls = {"rdl": [0, 0, 0], "wrl": [0, 0, 0], "scr": [0, 0, 0]}
    for (addr, mn, ops), depth in zip(insts, d):
        if mn == "v_readlane_b32" and re.fullmatch(r"\d+", ops.split(",")[-1].strip()):
            k = "rdl"
        elif mn == "v_writelane_b32":
            k = "wrl"
        elif mn.startswith("scratch_"):
            k = "scr"
        else:
            continue
        cls[k][0] += 1
        cls[k][1] += depth >= 1
        cls[k][2] += depth >= 4
    three = lambda v: "%d/%d/%d" % tuple(v)  # noqa: E731
    print("%s\n    insts %d loop %d deep %d | rdl %s wrl %s scr %s | vgpr %s sgpr %s scratch %s lds %s" %
          (name, len(insts), sum(1 for x in d if x >= 1), sum(1 for x in d if x >= 4), three(cls["rdl"]),
           three(cls["wrl"]), three(cls["scr"]), *notes))


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    pat = re.compile(sys.argv[2] if len(sys.argv) > 2 else ".")
    with tempfile.TemporaryDirectory() as tmp:
        co = code_object(sys.argv[1], tmp)
        notes = kernel_notes(co)
        funcs = functions(co)
    filt = next((f for f in (f"{LLVM}/llvm-cxxfilt", shutil.which("c++filt")) if f and os.path.exists(f)), None)
    demangle = list(notes)  # (mangled names where no demangler is installed)
    if filt:
        demangle = subprocess.run([filt], input="\n".join(notes), capture_output=True, text=True).stdout.split("\n")
    for sym, nice in sorted(zip(notes, demangle), key=lambda t: t[1]):
        if pat.search(nice) or pat.search(sym):
            report(nice.replace("fac::(anonymous namespace)::", ""), funcs.get(sym, []), notes[sym])


if __name__ == "__main__":
    main()
