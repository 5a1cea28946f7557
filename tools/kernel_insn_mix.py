#!/usr/bin/env python3
"""Static instruction mix of the gfx950 kernels in a built library or object file, per kernel symbol, as CSV:

    python tools/kernel_insn_mix.py pointcloudprocessing_amd/libpointnet_hip.so --match 'pn::gemm' > mix.csv
    python tools/kernel_insn_mix.py pointcloudprocessing_amd/csrc/pn_gemm.o

Needs no GPU: the device code objects are cut out of the file's offload bundles (clang-offload-bundler's uncompressed layout, read here
directly because a linked library holds one bundle per translation unit) and disassembled with llvm-objdump -d.  Only instruction CLASSES
are counted, by mnemonic prefix: code bytes, instructions, VALU (v_* without the matrix cores), MFMA, SALU, scalar memory loads, LDS,
global / buffer / flat / scratch loads and stores, the 2-byte forms among them, branches and s_waitcnt.  A symbol holds every path the
compiler inlined into it, so the counts bound the executed path from above; they are exact for straight-line kernels only.
"""
import argparse
import csv
import os
import re
import shutil
import struct
import subprocess
import sys
import tempfile

MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
COLS = ("kernel", "code_bytes", "instructions", "valu", "mfma", "salu", "smem", "lds", "vmem_ld", "vmem_st", "vmem_ld16", "vmem_st16",
        "vmem_atomic", "branches", "waitcnt")


def tool(name):
    for d in (os.environ.get("ROCM_PATH", "/opt/rocm") + "/llvm/bin", os.environ.get("ROCM_PATH", "/opt/rocm") + "/bin"):
        if os.path.exists(os.path.join(d, name)):
            return os.path.join(d, name)
    p = shutil.which(name)
    if not p:
        sys.exit(f"{name} not found")
    return p


def code_objects(blob, arch):
    """every device code object for `arch` in the file's offload bundles; a bare code object is returned as it is"""
    out, at = [], blob.find(MAGIC)
    if at < 0 and blob[:4] == b"\x7fELF" and struct.unpack_from("<H", blob, 18)[0] == 224:     # EM_AMDGPU
        return [blob]
    while at >= 0:
        n, = struct.unpack_from("<Q", blob, at + len(MAGIC))
        p = at + len(MAGIC) + 8
        for _ in range(n):
            off, size, idlen = struct.unpack_from("<QQQ", blob, p)
            ident = blob[p + 24:p + 24 + idlen].decode(errors="replace")
            p += 24 + idlen
            if "amdgcn" in ident and arch in ident and size:
                out.append(blob[at + off:at + off + size])
        at = blob.find(MAGIC, p)
    return out


def classify(mn, c):
    c["instructions"] += 1
    if mn.startswith(("v_mfma", "v_smfmac")):
        c["mfma"] += 1
    elif mn.startswith("v_"):
        c["valu"] += 1
    elif mn.startswith("ds_"):
        c["lds"] += 1
    elif mn.startswith(("global_", "buffer_", "flat_", "scratch_")):
        short = "short" in mn or "byte" in mn
        if "atomic" in mn:
            c["vmem_atomic"] += 1
        elif "_load" in mn:
            c["vmem_ld"] += 1
            c["vmem_ld16"] += short
        elif "_store" in mn:
            c["vmem_st"] += 1
            c["vmem_st16"] += short
    elif mn.startswith(("s_branch", "s_cbranch", "s_setpc", "s_swappc", "s_call")):
        c["branches"] += 1
    elif mn.startswith("s_waitcnt"):
        c["waitcnt"] += 1
    elif mn.startswith(("s_load", "s_buffer_load", "s_memtime", "s_memrealtime")):
        c["smem"] += 1
    elif mn.startswith("s_"):
        c["salu"] += 1


def disassemble(obj_path, arch):
    r = subprocess.run([tool("llvm-objdump"), "-d", f"--mcpu={arch}", obj_path], capture_output=True, text=True, check=True)
    kernels, cur = {}, None
    for line in r.stdout.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = kernels.setdefault(m.group(1), dict.fromkeys(COLS[1:], 0))
            continue
        m = re.match(r"^\s+(\S+).*//\s*[0-9A-Fa-f]+:((?:\s+[0-9A-Fa-f]{8})+)\b", line)
        if m and cur is not None:
            cur["code_bytes"] += 4 * len(m.group(2).split())
            classify(m.group(1), cur)
    return kernels


def kernel_symbols(obj_path):
    """the names that have a kernel descriptor (NAME.kd): device functions the compiler kept out of line are not kernels"""
    r = subprocess.run([tool("llvm-readelf"), "-sW", obj_path], capture_output=True, text=True, check=True)
    return {ln.split()[-1][:-3] for ln in r.stdout.splitlines() if ln.rstrip().endswith(".kd")}


def demangle(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, r.stdout.split("\n")))
    except Exception:
        return {n: n for n in names}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("binary", help="shared library, object file or bare code object")
    ap.add_argument("--arch", default="gfx950")
    ap.add_argument("--match", default="", help="regular expression on the demangled kernel name")
    a = ap.parse_args()
    objs = code_objects(open(a.binary, "rb").read(), a.arch)
    if not objs:
        sys.exit(f"{a.binary}: no uncompressed {a.arch} code object found")
    rows = {}
    with tempfile.TemporaryDirectory() as d:
        for i, o in enumerate(objs):
            path = os.path.join(d, f"{i}.co")
            with open(path, "wb") as f:
                f.write(o)
            keep = kernel_symbols(path)
            for k, v in disassemble(path, a.arch).items():
                if k in keep:
                    rows[k] = v
    names = demangle(sorted(rows))
    w = csv.writer(sys.stdout, lineterminator="\n")
    w.writerow(COLS)
    for k in sorted(rows, key=lambda k: names[k]):
        if a.match and not re.search(a.match, names[k]):
            continue
        w.writerow([names[k]] + [rows[k][c] for c in COLS[1:]])
    return 0


if __name__ == "__main__":
    sys.exit(main())
