#!/usr/bin/env python3
"""Summarise hipcc -Rpass-analysis=kernel-resource-usage for the csrc/*.hip kernels, compiled with the flags the library is built
with (build.py's FLAGS plus the per-file EXTRA_FLAGS, looked up by the file's base name).  "LDS Size" is the static part only: a
kernel with dynamic LDS shows 0 here and gets its size at the launch.

    python tools/kernel_resources.py myrtle-vision_amd/csrc/attention_tiled.hip [more.hip ...]"""
import os, re, subprocess, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "myrtle-vision_amd"))
from myrtle_vision.hip.build import EXTRA_FLAGS, FLAGS, INCLUDE, _hipcc  # noqa: E402

src = sys.argv[1:]
for f in src:
    out = subprocess.run([_hipcc()] + FLAGS + EXTRA_FLAGS.get(os.path.basename(f), []) +
                         ["-I", INCLUDE, "-c", f, "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"],
                         capture_output=True, text=True).stderr
    cur = {}
    for line in out.splitlines():
        m = re.search(r"remark: (?:Function Name: (\S+)|\s*([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+))", line)
        if not m: continue
        if m.group(1):
            if cur: print(cur)
            name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
            cur = {"kernel": name[:90]}
        else:
            k = m.group(2).strip()
            if k in ("VGPRs", "AGPRs", "VGPRs Spill", "ScratchSize", "Occupancy", "LDS Size", "SGPRs"):
                cur[k] = int(m.group(3))
    if cur: print(cur)
