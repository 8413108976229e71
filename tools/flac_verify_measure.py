#!/usr/bin/env python3
"""One process of a FLAC file writer for the verify mode's measurements ("Verify"; tools/flac_verify_profile.sh is
the command set):
    python tools/flac_verify_measure.py <16|24> <0|1> <renders> [out.jsonl]
examples__rainy_thunder at 44100 Hz, stereo, B = 4096, max_lpc_order 8, through sauAmd_render_file_flac_lpc (16) or
sauAmd_render_file_flac_lpc24 (24), with sauAmd_set_flac_file_verify off or on, `renders` times; the wall clock of every render
and one JSON line. A library without the verify mode (the parent commit's, through SAU_AMD_LIB) takes 0 only."""
import hashlib
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import saugns_amd as sa  # noqa: E402

bits, on, reps = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
L = sa.lib()
if on and not hasattr(L, "sauAmd_set_flac_file_verify"):
    sys.exit("this library has no verify mode")
prg = sa.Program.from_image(open(os.path.join(ROOT, "tests", "golden", "programs", "examples__rainy_thunder.saup"), "rb").read())
if on:
    sa.set_flac_file_verify(1)
out = dict(what="writer", bits=bits, max_lpc_order=8, verify=on, lib=os.path.basename(os.environ.get("SAU_AMD_LIB") or "") or "in-tree",
           program="examples__rainy_thunder", rate=44100, channels=2, B=4096)
with tempfile.TemporaryDirectory() as d:
    path = os.path.join(d, "x.flac")
    walls = []
    for _ in range(reps):
        t = time.perf_counter()
        if bits == 24:
            n, info = sa.render_file_flac_lpc24(prg, 44100, path, 2, 4096, max_lpc_order=8, gain=0.5)
        else:
            n, info = sa.render_file_flac(prg, 44100, path, 2, 4096, max_lpc_order=8)
        walls.append(round(time.perf_counter() - t, 6))
    data = open(path, "rb").read()
    out.update(frames=n, blocks=info.blocks, bytes=len(data), sha1=hashlib.sha1(data).hexdigest(), wall_s=walls,
               second_third_s=walls[1:3])
line = json.dumps(out)
print(line)
if len(sys.argv) > 4:
    open(sys.argv[4], "a").write(line + "\n")
