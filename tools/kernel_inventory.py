#!/usr/bin/env python3
"""Kernel inventory of the shipped library: one line per kernel, CPU only, loads no library.

    python tools/kernel_inventory.py [CSRC_DIR] > profiles/kernel_inventory.txt

Every CSRC_DIR/*.hip (default: sl-hwgat_amd/csrc of this tree) is compiled to device assembly with build.FLAGS, and
each kernel gives

    <file>  <demangled name>  <VGPRs> <SGPRs> <LDS bytes> <scratch bytes>  <hash>

(tab-separated).  The name is printed without its parameter list and without "(anonymous namespace)::": the template
arguments tell the kernels of a file apart.  The resources are the kernel descriptor's (.amdhsa_next_free_vgpr,
.amdhsa_next_free_sgpr, .amdhsa_group_segment_fixed_size, .amdhsa_private_segment_fixed_size).  The hash is the
SHA-256 (first 12 hex digits) of the kernel's text from its label to the end of its instructions, after replacing what depends only on the function's
position in the file or on its own name:
  - the function number in local labels: .LBB<n>_<m> and the BB<n>_<m> of the loop comments, .Lfunc_end<n>,
    .LJTI<n>_<m>; .Ltmp<n> is renumbered from 0 in order of appearance;
  - runs of blanks (the printer pads comments to a column, so the padding follows the length of a label);
  - the kernel's own mangled name, function-local LDS symbols (_ZZ<name>E<var>) included.
Two kernels with equal lines run the same instructions with the same resources, so the diff of two inventories is the
list of kernels a change added, removed or altered.
"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sl-hwgat_amd"))
import build  # noqa: E402

JOBS = min(16, os.cpu_count() or 1)
DESC = (".amdhsa_next_free_vgpr", ".amdhsa_next_free_sgpr", ".amdhsa_group_segment_fixed_size",
        ".amdhsa_private_segment_fixed_size")


def _body_hash(name, lines):
    text = "\n".join(lines)
    text = text.replace(name[2:] if name.startswith("_Z") else name, "@K")
    # .LBB<n>_<m> labels and the "Header=BB<n>_<m>" of loop comments
    text = re.sub(r"(?<![\w.])(\.L)?BB\d+_(?=\d)", r"\1BB_", text)
    text = re.sub(r"\.L(func_end|JTI)\d+", r".L\1", text)
    text = re.sub(r"[ \t]+", " ", text)
    tmps = {}
    text = re.sub(r"\.Ltmp\d+", lambda m: tmps.setdefault(m.group(0), ".Ltmp%d" % len(tmps)), text)
    return hashlib.sha256(text.encode()).hexdigest()[:12]


def inventory(src, tmp):
    """[(mangled name, resource string, hash)] of one source file"""
    asm = os.path.join(tmp, os.path.basename(src)[:-4] + ".s")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    extra = build.EXTRA.get(os.path.basename(src), [])
    cmd = [hipcc] + build.FLAGS + extra + ["-S", "--cuda-device-only", src, "-o", asm]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError(res.stdout + res.stderr)
    with open(asm) as fh:
        lines = fh.read().split("\n")
    label = {ln.split(":")[0]: i for i, ln in enumerate(lines) if ln[:1] == "_" and ":" in ln}
    out = []
    for i, ln in enumerate(lines):
        if not ln.startswith("\t.amdhsa_kernel "):
            continue
        name = ln.split()[1]
        desc = {}
        for d in lines[i + 1:lines.index("\t.end_amdhsa_kernel", i)]:
            key, _, val = d.strip().partition(" ")
            desc[key] = val.strip()
        # the descriptor sits in .rodata between the last instruction and .Lfunc_end: the body ends where .rodata begins
        end = max(j for j in range(label[name], i) if lines[j].startswith("\t.section"))
        res = " ".join(desc[k] for k in DESC)
        out.append((name, res, _body_hash(name, lines[label[name]:end])))
    os.remove(asm)
    return out


def main():
    csrc = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else build.CSRC
    srcs = sorted(os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".hip"))
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=JOBS) as ex:
        per_file = list(ex.map(lambda s: inventory(s, tmp), srcs))
    names = [k[0] for ks in per_file for k in ks]
    # binutils' c++filt does not know DF16b (__bf16): demangle it as Dh (half, which no kernel here uses) and rename
    plain = subprocess.run(["c++filt", "-p"], input="\n".join(names).replace("DF16b", "Dh"), capture_output=True, text=True,
                           check=True).stdout
    plain = re.sub(r"\bhalf\b", "__bf16", plain).replace("(anonymous namespace)::", "").split("\n")
    rows, it = [], iter(plain)
    for src, ks in zip(srcs, per_file):
        rows += [(os.path.basename(src), next(it), res, h) for _, res, h in ks]
    print("# file\tkernel\tvgpr sgpr lds scratch\thash")
    for row in sorted(rows):
        print("\t".join(row))
    print(f"# {len(rows)} kernels in {len(srcs)} files", file=sys.stderr)


if __name__ == "__main__":
    main()
