#!/usr/bin/env python3
"""One process of the FLAC writer for the LPC mode's measurements (tools/flac_lpc_profile.sh is the command set):
    python tools/flac_lpc_measure.py <rainy|config3> <max_lpc_order> <renders> [out.json]
renders the program at 44100 Hz stereo, B = 4096, `renders` times into a scratch file and prints one JSON line: the file's
bytes, every render's wall time (the first includes start-up) and which library ran: "in-tree", or the file name (never the
path) of the build that SAU_AMD_LIB names. One
without the _lpc entry points (the parent commit's) takes max_lpc_order 0 only, through sauAmd_render_file_flac."""
import ctypes as C
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import saugns_amd as sa  # noqa: E402
from saugns_amd import voicebank  # noqa: E402
from saugns_amd.api import FlacInfo  # noqa: E402

what, M, reps = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
if what == "rainy":
    prg = sa.Program.from_image(open(os.path.join(ROOT, "tests", "golden", "programs", "examples__rainy_thunder.saup"), "rb").read())
else:
    prg = voicebank.config3(n=1024, seconds=10)
L = sa.lib()
has_lpc = hasattr(L, "sauAmd_render_file_flac_lpc")
if M and not has_lpc:
    sys.exit("this library has no LPC mode")
with tempfile.TemporaryDirectory() as d:
    path = os.path.join(d, "x.flac")
    walls, n, info = [], C.c_uint64(), FlacInfo()
    for _ in range(reps):
        t = time.perf_counter()
        if has_lpc:
            ok = L.sauAmd_render_file_flac_lpc(prg.ptr, 44100, os.fsencode(path), 2, 4096, M, C.byref(n), C.byref(info))
        else:
            ok = L.sauAmd_render_file_flac(prg.ptr, 44100, os.fsencode(path), 2, 4096, C.byref(n), C.byref(info))
        walls.append(round(time.perf_counter() - t, 6))
        if not ok:
            sys.exit("the writer failed: " + sa.api.last_error(L))
    out = dict(program=what, max_lpc_order=M, lib=os.path.basename(os.environ.get("SAU_AMD_LIB") or "") or "in-tree", entry="_lpc" if has_lpc else "plain",
               frames=n.value, blocks=info.blocks, bytes=os.path.getsize(path), wall_s=walls)
line = json.dumps(out)
print(line)
if len(sys.argv) > 4:
    open(sys.argv[4], "a").write(line + "\n")
