#!/usr/bin/env python3
"""One line `symbol  sha256` per kernel of the given csrc/*.hip files: a digest of the kernel's gfx950 assembly, made independent of
where the kernel sits in the file.  A host-only edit must leave every line as it was; a line that moves means device code changed.

Each file is compiled device-only to assembly with the flags the library is built with (build.py's FLAGS plus the per-file
EXTRA_FLAGS).  The digest covers the kernel's instruction text from its label to its end marker and its .amdhsa_kernel descriptor
block (registers, LDS, scratch).  Compiler-local labels carry the index of the function within the file (.LBB12_3), which moves with
the order of template instantiation, so that index is dropped; comments are dropped too.

    python tools/kernel_digest.py myrtle-vision_amd/csrc/*.hip > after.txt"""
import hashlib, os, re, subprocess, sys
from concurrent.futures import ThreadPoolExecutor
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "myrtle-vision_amd"))
from myrtle_vision.hip.build import EXTRA_FLAGS, FLAGS, INCLUDE, _hipcc  # noqa: E402

LOCAL = re.compile(r"\.L(BB|func_end|func_begin|tmp|JTI)\d+(_\d+)?")


def normalise(line):
    return LOCAL.sub(lambda m: ".L" + m.group(1) + (m.group(2) or ""), line)


def digests(path):
    asm = subprocess.run([_hipcc()] + FLAGS + EXTRA_FLAGS.get(os.path.basename(path), []) +
                         ["-I", INCLUDE, "--cuda-device-only", "-S", path, "-o", "-"], capture_output=True, text=True, check=True).stdout
    lines = [ln.split(";", 1)[0].rstrip() for ln in asm.splitlines()]       # ';' starts a comment in amdgcn assembly
    label ={ln[:-1]: i for i, ln in enumerate(lines) if ln.endswith(":") and not ln.startswith((".", " ", "\t"))}
    out = []
    for d0, ln in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel (\S+)$", ln)
        if not m: continue
        k, start = m.group(1), label[m.group(1)]
        end = next(i for i in range(start, len(lines)) if re.match(r"\.Lfunc_end\d+:", lines[i]))
        d1 = next(i for i in range(d0, len(lines)) if lines[i].strip() == ".end_amdhsa_kernel")
        h = hashlib.sha256()
        for t in lines[start:end] + lines[d0:d1]:
            t = normalise(t)
            if t.strip():
                h.update(t.encode() + b"\n")
        out.append(f"{k}  {h.hexdigest()}")
    return out


with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
    for group in ex.map(digests, sys.argv[1:]):
        for line in sorted(group):
            print(line)
