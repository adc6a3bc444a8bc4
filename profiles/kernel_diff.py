#!/usr/bin/env python3
"""Per-symbol diff of the gfx950 device code of two sets of built objects:

    python3 profiles/kernel_diff.py --a OLD.o [OLD2.o ...] --b NEW.o [NEW2.o ...]

Every object's gfx950 code object is taken out of its .hip_fatbin (as profiles/kernel_resources.sh
does) and disassembled; the text of every function symbol (kernels and non-inlined device functions)
of side A is compared with the same symbol's of side B. A symbol may live in any object of its side.
Three differences are normalised away before comparing:
  * names inside an anonymous namespace carry no file identity (_GLOBAL__N_1), so they compare as they
    are; a symbol that moved out of one is matched after dropping the anonymous-namespace component;
  * the literals of the s_add_u32 / s_addc_u32 pair that follows s_getpc_b64 (pc-relative call and
    address offsets, which depend on where the linker put the target);
  * the s_nop / s_code_end padding after a function's last instruction.
Prints one line per symbol that differs or exists on one side only, then a summary; exit status 1 if
anything differs.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def code_object(obj, tmp, tag):
    fb, co = os.path.join(tmp, tag + ".fb"), os.path.join(tmp, tag + ".co")
    subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fb}", obj], check=True)
    subprocess.run([f"{LLVM}/clang-offload-bundler", "--type=o", f"--input={fb}", f"--output={co}", "--unbundle",
                    f"--targets={TARGET}"], check=True)
    return co


def functions(co):
    """symbol -> list of instruction lines"""
    txt = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co], check=True,
                         capture_output=True, text=True).stdout
    out, cur = {}, None
    for line in txt.split("\n"):
        m = re.match(r"^<(\S+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None:
            line = re.sub(r"\s*//.*$", "", line).strip()  # the address and encoding comment
            if line:
                cur.append(line)
    for body in out.values():  # the padding between functions and at the end of .text
        while body and re.match(r"(s_nop 0|s_code_end|\.\.\.)$", body[-1]):
            body.pop()
    return out


def kernels(co):
    txt = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
    return set(re.findall(r"\.name:\s+(\S+)", txt)) & set(functions_cache[co])


def normalise(lines):
    out, after_getpc = [], 0
    for l in lines:
        if l.startswith("s_getpc_b64"):
            after_getpc = 2
        elif after_getpc and re.match(r"s_addc?_u32 ", l):
            l = re.sub(r",\s*\S+$", ", <pcrel>", l)
            after_getpc -= 1
        out.append(l)
    return out


def plain(name):  # a symbol with the anonymous-namespace component dropped
    return name.replace("12_GLOBAL__N_1", "")


def side(objs, tmp, tag):
    funcs, kern = {}, set()
    for i, o in enumerate(objs):
        co = code_object(o, tmp, f"{tag}{i}")
        f = functions(co)
        functions_cache[co] = f
        kern |= kernels(co)
        for k, v in f.items():
            if k in funcs:
                sys.exit(f"symbol {k} in two objects of side {tag}")
            funcs[k] = v
    return funcs, kern


functions_cache = {}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--a", nargs="+", required=True)
    ap.add_argument("--b", nargs="+", required=True)
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        fa, ka = side(args.a, tmp, "a")
        fb, kb = side(args.b, tmp, "b")
    pa, pb = {plain(k): k for k in fa}, {plain(k): k for k in fb}
    bad = 0
    for p in sorted(set(pa) | set(pb)):
        if p not in pa or p not in pb:
            print(f"ONLY-{'A' if p in pa else 'B'}  {pa.get(p) or pb.get(p)}")
            bad += 1
            continue
        a, b = fa[pa[p]], fb[pb[p]]
        if pa[p] != pb[p]:
            print(f"RENAMED {pa[p]} -> {pb[p]}")
        if a == b:
            continue
        na, nb = normalise(a), normalise(b)
        if na == nb:
            n = sum(x != y for x, y in zip(a, b))
            print(f"PCREL   {pa[p]}: {n} pc-relative literal(s) differ, nothing else")
        else:
            first = next((i for i, (x, y) in enumerate(zip(na, nb)) if x != y), min(len(na), len(nb)))
            print(f"DIFF    {pa[p]}: {len(na)} vs {len(nb)} instructions, first difference at {first}")
            bad += 1
    if {plain(k) for k in ka} != {plain(k) for k in kb}:
        print("kernel sets differ")
        bad += 1
    print(f"side A: {len(fa)} function symbols, {len(ka)} kernels; side B: {len(fb)} function symbols, {len(kb)} kernels; "
          f"{bad} symbol(s) differ beyond pc-relative literals")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
