#!/usr/bin/env python3
"""Which kernels of librtmi.so changed their machine code between two builds.  Takes the gfx950 code object out of each library
(llvm-objcopy, clang-offload-bundler), disassembles it (llvm-objdump -d --symbolize-operands, so that branch targets are labels and
not addresses), drops addresses and encodings, renumbers the labels per function, and compares the text of every function by name.  Prints one line per function:
its sha256 in the new build and `same`, `CHANGED`, `new` or `removed`; the exit status is 1 when a function both builds have
differs.
Usage: tools/kernel_code_diff.py PARENT/librtmi.so NEW/librtmi.so [--llvm /opt/rocm/llvm/bin] [--out FILE.txt]"""
import argparse
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ap = argparse.ArgumentParser()
ap.add_argument("parent")
ap.add_argument("new")
ap.add_argument("--llvm", default="/opt/rocm/llvm/bin")
ap.add_argument("--arch", default="gfx950")
ap.add_argument("--out", default=None)
args = ap.parse_args()


def functions(lib):
    """name -> the function's instructions as text, addresses and encodings dropped"""
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "fatbin"), os.path.join(d, "co")
        subprocess.check_call([os.path.join(args.llvm, "llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", lib])
        subprocess.check_call([os.path.join(args.llvm, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={fat}",
                               f"--targets=hipv4-amdgcn-amd-amdhsa--{args.arch}", f"--output={co}"])
        text = subprocess.check_output([os.path.join(args.llvm, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr",
                                        "--symbolize-operands", co], text=True)
    out, name = {}, None
    for line in text.splitlines():
        m = re.match(r"^<([^>]+)>:$", line)
        if m and not re.fullmatch(r"L\d+", m.group(1)):
            name = m.group(1)
            out[name] = []
        elif name is not None:
            out[name].append(line.split("//")[0].rstrip())
    def renumber(body):  # objdump numbers the labels through the whole file: number them per function, in order of appearance
        seen = {}
        return re.sub(r"\bL\d+\b", lambda m: seen.setdefault(m.group(0), f"L{len(seen)}"), body)
    return {k: renumber("\n".join(v)) for k, v in out.items()}


old, new = functions(args.parent), functions(args.new)
lines, changed = [], 0
for k in sorted(set(old) | set(new)):
    if k not in new:
        lines.append(f"{'-' * 64}  removed  {k}")
        continue
    h = hashlib.sha256(new[k].encode()).hexdigest()
    if k not in old:
        lines.append(f"{h}  new      {k}")
    elif old[k] == new[k]:
        lines.append(f"{h}  same     {k}")
    else:
        changed += 1
        lines.append(f"{h}  CHANGED  {k}")
n_same = sum(" same " in l for l in lines)
lines.append(f"# {n_same} functions identical, {changed} changed, {sum(' new ' in l for l in lines)} new, {sum(' removed ' in l for l in lines)} removed")
text = "\n".join(lines) + "\n"
sys.stdout.write(text)
if args.out:
    with open(args.out, "w") as f:
        f.write(text)
sys.exit(1 if changed else 0)
