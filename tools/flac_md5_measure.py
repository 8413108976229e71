#!/usr/bin/env python3
"""One process of the FLAC encoder for the MD5's measurements ("MD5"; tools/flac_md5_profile.sh is the command set):
    python tools/flac_md5_measure.py writer <0|1> <renders>      sauAmd_render_file_flac of examples__rainy_thunder, 44100 Hz stereo,
                                                                 B = 4096, with sauAmd_set_flac_file_md5 off or on
    python tools/flac_md5_measure.py fed <0|1> <feeds>           a float-fed encoder of 64 rows, B = 256, stereo, 24 bits, with MD5 off
                                                                 or on, fed noise in feeds of the writer's chunk (176400 frames)
and prints one JSON line. A library without MD5 (the parent commit's, through SAU_AMD_LIB) takes 0 only."""
import json
import os
import sys
import tempfile
import time

what, on, reps = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
if what == "fed":
    import torch  # (before the library: a process has room for one HIP runtime)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import saugns_amd as sa  # noqa: E402
from saugns_amd import voicebank  # noqa: E402

L = sa.lib()
if on and not hasattr(L, "sauAmd_Flac_set_md5"):
    sys.exit("this library has no MD5")
out = dict(what=what, md5=on, lib=os.path.basename(os.environ.get("SAU_AMD_LIB") or "") or "in-tree")
if what == "writer":
    prg = sa.Program.from_image(open(os.path.join(ROOT, "tests", "golden", "programs", "examples__rainy_thunder.saup"), "rb").read())
    if on:
        sa.set_flac_file_md5(1)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "x.flac")
        walls = []
        for _ in range(reps):
            t = time.perf_counter()
            n, info = sa.render_file_flac(prg, 44100, path, 2, 4096)
            walls.append(round(time.perf_counter() - t, 6))
        data = open(path, "rb").read()
        out.update(frames=n, bytes=len(data), md5_field=data[26:42].hex(), wall_s=walls)
else:
    ROWS, B, CH, CHUNK = 64, 256, 2, 176400
    b = sa.Batch([voicebank.build_program([voicebank.Op("sin", freq=200.0, time_ms=10)])], 44100)  # (never run: its device is used)
    g = torch.Generator(device="cuda").manual_seed(1)
    rows = (torch.rand((ROWS, CHUNK * CH), generator=g, device="cuda", dtype=torch.float32) - 0.5) * 0.5
    torch.cuda.synchronize()
    e = b.create_flac_f32(ROWS, CH, B, bits=24)
    if on:
        e.set_md5(True)
    walls = []
    for i in range(reps):
        t = time.perf_counter()
        e.feed_f32(rows.data_ptr(), rows.stride(0) * 4, [CHUNK] * ROWS, None, finish=i == reps - 1)
        sizes, _ = e.unread()
        walls.append(round(time.perf_counter() - t, 6))
        if i < reps - 1:
            e.read()
    digest = e.md5()[0].hex() if on else ""
    e.read(reset=True)
    e.close()
    b.close()
    out.update(rows=ROWS, block_frames=B, channels=CH, bits=24, feed_frames=CHUNK, feeds=reps, md5_row0=digest, wall_s=walls)
print(json.dumps(out))
