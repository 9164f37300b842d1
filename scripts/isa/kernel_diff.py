#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds of libnice_hip.so instruction by
instruction:  python scripts/isa/kernel_diff.py OLD.so NEW.so [name-filter]

Every code object of each library's .hip_fatbin section is disassembled
(llvm-objdump) and its kernels keyed by demangled name (a template argument
appended with the default `false` is stripped, so a kernel keeps its key
across such a change).  Instructions are compared as text without addresses and encodings;
branch targets are compared as offsets from the kernel's start, the literal
of a pc-relative address (the s_add_u32 / s_addc_u32 after s_getpc_b64: a call
into another function of the code object, which moves with the layout) is
masked, and the padding after a function's end is dropped.  Prints the
kernels that differ, those only one side has, and a count of identical ones.
"""
import os
import re
import struct
import subprocess
import sys
import tempfile

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
OBJDUMP = os.path.join(ROCM, "llvm", "bin", "llvm-objdump")
OBJCOPY = os.path.join(ROCM, "llvm", "bin", "llvm-objcopy")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(lib, tmp):
    fat = os.path.join(tmp, os.path.basename(lib) + ".fatbin")
    subprocess.run([OBJCOPY, "-O", "binary", "--only-section=.hip_fatbin", lib, fat], check=True)
    data = open(fat, "rb").read()
    out, pos = [], data.find(MAGIC)
    while pos >= 0:
        n, = struct.unpack_from("<Q", data, pos + len(MAGIC))
        p = pos + len(MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", data, p)
            triple = data[p + 24:p + 24 + tlen].decode()
            p += 24 + tlen
            if "gfx950" in triple and size:
                path = os.path.join(tmp, "%s.%d.co" % (os.path.basename(lib), len(out)))
                with open(path, "wb") as f:
                    f.write(data[pos + off:pos + off + size])
                out.append(path)
        pos = data.find(MAGIC, pos + 1)
    return out


def key_of(name):
    return re.sub(r", false>", ">", name)


def kernels(lib, tmp):
    res = {}
    for co in code_objects(lib, tmp):
        txt = subprocess.run([OBJDUMP, "-d", "-C", "--no-show-raw-insn", co], check=True,
                             capture_output=True, text=True).stdout
        cur, start = None, 0
        for line in txt.splitlines():
            m = re.match(r"^([0-9a-f]+) <(.*)>:$", line)
            if m:
                cur, start = key_of(m.group(2)), int(m.group(1), 16)
                res[cur] = []
                continue
            m = re.match(r"^\s+(\S.*?)\s*//\s*([0-9A-Fa-f]+):", line)
            if cur is None or not m:
                continue
            ins = m.group(1)
            # a branch target: "<symbol+0x..>" or an absolute address
            ins = re.sub(r"<[^>]*\+0x([0-9a-f]+)>", lambda t: "+" + t.group(1), ins)
            ins = re.sub(r"<[^>]*>", "+0", ins)
            if ins.startswith("s_code_end"):
                cur = None
                continue
            if res[cur] and ins.startswith("s_add_u32") and res[cur][-1].startswith("s_getpc_b64"):
                ins = re.sub(r"0x[0-9a-f]+$|-?\d+$", "PCREL", ins)
            elif len(res[cur]) > 1 and ins.startswith("s_addc_u32") and res[cur][-2].startswith("s_getpc_b64"):
                ins = re.sub(r"0x[0-9a-f]+$|-?\d+$", "PCREL", ins)
            res[cur].append(ins)
    for k in res:
        while res[k] and res[k][-1].startswith("s_nop"):
            res[k].pop()
    return res


def main():
    old, new = sys.argv[1], sys.argv[2]
    filt = sys.argv[3] if len(sys.argv) > 3 else ""
    with tempfile.TemporaryDirectory() as tmp:
        a, b = kernels(old, tmp), kernels(new, tmp)
    same = 0
    for k in sorted(a):
        if filt not in k:
            continue
        if k not in b:
            print("only in old:", k)
        elif a[k] != b[k]:
            n = next((i for i, (x, y) in enumerate(zip(a[k], b[k])) if x != y), min(len(a[k]), len(b[k])))
            print("DIFFERS: %s (%d vs %d instructions, first at %d)" % (k, len(a[k]), len(b[k]), n))
        else:
            same += 1
    extra = [k for k in sorted(b) if filt in k and k not in a]
    print("identical: %d   only in new: %d" % (same, len(extra)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
