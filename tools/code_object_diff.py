#!/usr/bin/env python3
"""Compare the gfx950 device code and the exports of two builds of the libraries.

    python tools/code_object_diff.py <parent lib dir> <new lib dir>

For every libhpccg_hip*.so of either directory: the gfx950 code object is
unbundled (clang-offload-bundler), disassembled (llvm-objdump -d) and compared
kernel by kernel after dropping addresses and encodings, the padding after a
kernel's last instruction, and turning branch targets into a placeholder; the
kernels' resources are the code-object notes' (llvm-readelf --notes, every
numeric key of a kernel's entry); the exports are `nm -D --defined-only` with
__hip_cuid_* left aside. Prints one row per library and exits non-zero on any
difference. It compares and reports only.
"""
import glob
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
PADDING = ("s_nop", "s_code_end")


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def code_object(lib, workdir):
    fb, co = os.path.join(workdir, "fb.bin"), os.path.join(workdir, "co.elf")
    run("objcopy", f"--dump-section=.hip_fatbin={fb}", lib, os.path.join(workdir, "lib.copy"))
    run(os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={fb}",
        f"--targets={TARGET}", f"--output={co}")
    return co


def resources(co):
    """kernel symbol -> {key: value} of the numeric keys of its notes entry"""
    out, cur = {}, None
    for line in run(os.path.join(LLVM, "llvm-readelf"), "--notes", co).splitlines():
        if line.startswith("  - ."):  # a kernel's entry opens (its arguments' are indented further)
            cur = {}
        m = re.match(r"  [- ] \.(\w+):\s+(\S+)\s*$", line)
        if not m or cur is None:
            continue
        key, val = m.groups()
        if key == "name":
            out[val] = cur
        elif re.fullmatch(r"\d+", val):
            cur[key] = int(val)
    return out


def streams(co):
    """kernel symbol -> its instructions, addresses, encodings and trailing padding dropped"""
    out, cur = {}, None
    for line in run(os.path.join(LLVM, "llvm-objdump"), "-d", co).splitlines():
        m = re.match(r"[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        ins = line.split("//")[0].strip()
        if cur is None or not ins or ins == "...":  # ("...": zero bytes after the last kernel)
            continue
        if re.match(r"s_(c?branch|call)", ins):
            ins = ins.split()[0] + " <target>"
        cur.append(ins)
    for body in out.values():
        while body and body[-1].split()[0] in PADDING:
            body.pop()
    return out


def exports(lib):
    syms = [line.split()[-1] for line in run("nm", "-D", "--defined-only", lib).splitlines() if line.strip()]
    return sorted(s for s in syms if not s.startswith("__hip_cuid_"))


def describe(lib):
    with tempfile.TemporaryDirectory() as d:
        co = code_object(lib, d)
        res, code = resources(co), streams(co)
    return {"kernels": {k: (code.get(k), res[k]) for k in res}, "exports": exports(lib)}


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    a_dir, b_dir = sys.argv[1:]
    names = sorted({os.path.basename(p) for d in (a_dir, b_dir) for p in glob.glob(os.path.join(d, "libhpccg_hip*.so"))})
    if not names:
        sys.exit(f"no libhpccg_hip*.so in {a_dir} or {b_dir}")
    print(f"{'library':34} {'kernels':>9} {'names':>6} {'code':>6} {'resources':>9} {'exports':>8}")
    bad = 0
    for name in names:
        a_lib, b_lib = os.path.join(a_dir, name), os.path.join(b_dir, name)
        if not (os.path.exists(a_lib) and os.path.exists(b_lib)):
            print(f"{name:34} only in {a_dir if os.path.exists(a_lib) else b_dir}")
            bad += 1
            continue
        a, b = describe(a_lib), describe(b_lib)
        ka, kb = a["kernels"], b["kernels"]
        only = sorted(set(ka) ^ set(kb))
        both = sorted(set(ka) & set(kb))
        code = [k for k in both if ka[k][0] is None or ka[k][0] != kb[k][0]]
        res = [k for k in both if ka[k][1] != kb[k][1]]
        exp = sorted(set(a["exports"]) ^ set(b["exports"]))
        word = lambda diff: "equal" if not diff else f"{len(diff)} differ"
        print(f"{name:34} {len(ka):>4}/{len(kb):<4} {word(only):>6} {word(code):>6} {word(res):>9} {word(exp):>8}")
        for what, diff in (("kernel in one only", only), ("code", code), ("resources", res), ("export in one only", exp)):
            for k in diff:
                print(f"    {what}: {k}")
        bad += bool(only or code or res or exp)
    print("identical" if not bad else f"{bad} libraries differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
