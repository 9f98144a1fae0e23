"""Digest of the gfx950 device code of HIP sources, without a GPU: one line per kernel, sorted by (mangled) name, with the SHA-256 of the
kernel's bytes in .text and the resource numbers of its metadata note (.vgpr_count .sgpr_count .vgpr_spill_count .sgpr_spill_count
.private_segment_fixed_size .group_segment_fixed_size).  Two sets of sources whose digests are equal as sets of lines hold the same kernels:

    python tools/kernel_digest.py csrc/conv_igemm.hip csrc/conv_ws.hip ... [--flags "-DCONV_STAMPS"] > digest.txt

Each source is compiled device-only with the library's flags (csrc/Makefile), the gfx950 code object is unbundled, and the symbol table and the
notes are read with llvm-readelf.  Bytes are hashed and numbers are copied: nothing here looks at what a kernel's instructions are.
"""
import argparse
import hashlib
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
LLVM = os.path.join(ROCM, "llvm", "bin")
FIELDS = ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def digest(src, flags, tmp):
    bundle, co = os.path.join(tmp, "dev.o"), os.path.join(tmp, "dev.co")
    run(os.path.join(ROCM, "bin", "hipcc"), "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I" + os.path.join(REPO, "include"), *flags,
        "--cuda-device-only", "-c", src, "-o", bundle)
    run(os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + bundle,
        "--output=" + co)
    readelf = os.path.join(LLVM, "llvm-readelf")
    text = re.search(r"\] \.text\s+PROGBITS\s+([0-9a-f]+) ([0-9a-f]+) ([0-9a-f]+)", run(readelf, "-S", co))
    addr, off, size = (int(x, 16) for x in text.groups())
    image = open(co, "rb").read()
    meta, cur = {}, None   # kernel name -> its note fields (the kernel-level keys sit at four columns, an argument's deeper)
    for line in run(readelf, "--notes", co).splitlines():
        if line.startswith("  - ."):
            cur = {}
            line = "    " + line[4:]
        m = re.match(r"    \.(\w+):\s+(\S+)$", line)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2)
            if m.group(1) == "name":
                meta[m.group(2)] = cur
    lines = []
    for m in re.finditer(r"^\s*\d+: ([0-9a-f]+)\s+(\d+) FUNC\s+\S+\s+\S+\s+\d+ (\S+)$", run(readelf, "-s", "--symbols", co), re.M):
        value, n, name = int(m.group(1), 16), int(m.group(2)), m.group(3)
        if name not in meta:
            continue   # a device function that is not a kernel
        assert addr <= value and value + n <= addr + size, name
        code = image[off + value - addr:off + value - addr + n]
        lines.append("%s sha256=%s %s" % (name, hashlib.sha256(code).hexdigest(), " ".join("%s=%s" % (f, meta[name][f]) for f in FIELDS)))
    assert len(set(lines)) == len(meta), "every kernel of the notes has one symbol"
    return set(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("sources", nargs="+")
    ap.add_argument("--flags", default="", help="extra compiler flags, as one string")
    a = ap.parse_args()
    lines = set()
    with tempfile.TemporaryDirectory() as tmp:
        for src in a.sources:
            lines |= digest(src, a.flags.split(), tmp)
    sys.stdout.write("".join(line + "\n" for line in sorted(lines)))


if __name__ == "__main__":
    main()
