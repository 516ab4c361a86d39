#!/usr/bin/env python3
"""One line per kernel of the HIP sources given: mangled name, hash of its instruction stream, hash of its .amdhsa_kernel descriptor
(registers, LDS, scratch, kernarg layout).  Compiled device-only with the library's flags; needs no GPU.  Comments are stripped and the
.LBB<func>_<n> labels renumbered to .LBB_<n> (the function index changes when a kernel moves between files), so the sorted output of
two trees is equal exactly when their machine code is.
    python tools/kernel_digest.py coala-gnn_amd/csrc/*.hip | sort
    EXTRA=-DCOALA_DEV_KNOBS python tools/kernel_digest.py ...      (more compiler flags: here, the development build's kernels)"""
import hashlib
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sha(text):
    return hashlib.sha256(text.encode()).hexdigest()[:16]


for src in sys.argv[1:]:
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", os.path.join(ROOT, "include"),
           "-mllvm", "-amdgpu-kernarg-preload-count=16", "--cuda-device-only", "-S"] + os.environ.get("EXTRA", "").split() + [src, "-o", "-"]
    asm = subprocess.run(cmd, capture_output=True, text=True, check=True).stdout
    desc = {m.group(1): sha(m.group(2)) for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", asm, re.S)}
    for m in re.finditer(r"^(\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", asm, re.S | re.M):
        name, body = m.group(1), re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", m.group(2))
        lines = [ln.split(";")[0].rstrip() for ln in body.splitlines()]
        if name in desc:
            print(name, sha("\n".join(ln for ln in lines if ln.strip())), desc[name])
