#!/usr/bin/env python3
"""One line per gfx950 kernel of the given object files, sorted by name: mangled name, sha256 of the function's bytes in
.text, vgpr / agpr / sgpr counts, private and group segment sizes, kernarg size.  Two builds whose listings (or the
sha256 of the listing, printed last) are equal have the same kernels with the same code and resources.  usage: tools/kernel_digest.py a.o b.o ...   (CPU only)"""
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
FIELDS = ["vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size", "kernarg_segment_size"]


def tool(name):
    return shutil.which(name) or os.path.join(LLVM, name)


def readelf(*args):
    exe = tool("llvm-readelf")
    cmd = [exe] if os.path.exists(exe) else [tool("llvm-readobj"), "--elf-output-style=GNU"]
    return subprocess.run(cmd + list(args), check=True, stdout=subprocess.PIPE, text=True).stdout


def kernels(obj, tmp):
    fat, co, text = (os.path.join(tmp, n) for n in ("fatbin", "code.co", "text"))
    subprocess.run([tool("llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj], check=True)
    subprocess.run([tool("clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + TARGET, "--input=" + fat, "--output=" + co], check=True)
    subprocess.run([tool("llvm-objcopy"), "--dump-section", ".text=" + text, co], check=True)
    code = open(text, "rb").read()
    base = next(int(m.group(1), 16) for m in re.finditer(r"\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)", readelf("-S", co)))
    funcs = {}                                                   # name -> (address, size)
    for line in readelf("-s", "-W", co).splitlines():
        f = line.split()
        if len(f) == 8 and f[3] == "FUNC" and f[6] != "UND":
            funcs[f[7]] = (int(f[1], 16), int(f[2], 0))
    out = []
    # the metadata note: one "- .agpr_count:" ... block per kernel, keys sorted
    for block in re.split(r"\n\s*- \.agpr_count:", "\n" + readelf("--notes", co))[1:]:
        block = ".agpr_count:" + block
        meta = {k: v.strip("' ") for k, v in re.findall(r"^\s*\.(\w+):\s*(\S+)\s*$", block, re.M)}
        addr, size = funcs[meta["name"]]
        digest = hashlib.sha256(code[addr - base:addr - base + size]).hexdigest()
        out.append(" ".join([meta["name"], digest] + [f"{k}={meta[k]}" for k in FIELDS]))
    return out


def main(objs):
    lines = []
    for obj in objs:
        with tempfile.TemporaryDirectory() as tmp:
            lines += kernels(obj, tmp)
    text = "\n".join(sorted(lines)) + "\n"
    sys.stdout.write(text)
    print(f"# {len(lines)} kernels in {len(objs)} objects; sha256 of the lines above: {hashlib.sha256(text.encode()).hexdigest()}")


if __name__ == "__main__":
    main(sys.argv[1:])
