#!/usr/bin/env python3
"""One process of the quantiser's measurements ("Dither and noise shaping"); run it under
`rocprofv3 --kernel-trace --stats` for the kernels' times, as tools/profile_round.sh runs its commands:
    python tools/dither_measure.py <kernels|writers> [out.jsonl]
kernels: rows of 441000 stereo frames of noise -- dither_shape_kernel (F9) on 1 and on 64 streams, dither_flat_kernel (FLAT) and
a float-fed 16-bit FLAC encoder's flac_quant_kernel<short> on the same 64 rows -- three feeds each, with the wall time of a
feed and its wait. writers: examples__rainy_thunder at 44100 Hz stereo through sauAmd_render_file_flac_dithered (F9) and through
sauAmd_render_file_flac_f32 at 16 bits, B = 4096, M = 0, three renders each. One JSON line per measurement."""
import json
import os
import sys
import tempfile
import time

import torch  # (before the library: torch's wheel brings a HIP runtime of its own)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import saugns_amd as sa  # noqa: E402
from saugns_amd import voicebank as vb  # noqa: E402

FRAMES, REPS = 441000, 3
lines = []


def note(**kw):
    lines.append(json.dumps(kw))
    print(lines[-1], flush=True)


def kernels():
    b = sa.Batch([vb.build_program([vb.Op("sin", freq=200.0, time_ms=10)])], 44100)  # (never run: its device is all that is used)
    g = torch.Generator(device="cuda").manual_seed(1)
    rows = (torch.randn((64, FRAMES * 2), generator=g, device="cuda", dtype=torch.float32) * 0.1).contiguous()
    torch.cuda.synchronize()
    ptr, pitch = rows.data_ptr(), rows.shape[1] * 4

    def timed(what, n, feed, wait):
        walls = []
        for _ in range(REPS):
            t = time.perf_counter()
            feed()
            wait()
            walls.append(round(time.perf_counter() - t, 6))
        note(what=what, streams=n, frames=FRAMES, wall_s=walls, ns_per_frame=round(min(walls) / FRAMES * 1e9, 3))

    for n in (1, 64):
        q = b.create_quantizer(n, 2, sa.dither_preset(sa.DITHER_F9, 1))
        timed("dither_shape_kernel F9", n, lambda: q.feed(ptr, pitch, [FRAMES] * n), lambda: q.stats())
        q.close()
    q = b.create_quantizer(64, 2, sa.dither_preset(sa.DITHER_FLAT, 1))
    timed("dither_flat_kernel FLAT", 64, lambda: q.feed(ptr, pitch, [FRAMES] * 64), lambda: q.stats())
    q.close()
    e = b.create_flac_f32(64, 2, 4096, bits=16)
    timed("flac_quant_kernel<short> and the encoder behind it", 64, lambda: e.feed_f32(ptr, pitch, [FRAMES] * 64, None, finish=True),
          lambda: e.read(reset=True))
    e.close()
    b.close()


def writers():
    prg = sa.Program.from_image(open(os.path.join(ROOT, "tests", "golden", "programs", "examples__rainy_thunder.saup"), "rb").read())
    spec = sa.dither_preset(sa.DITHER_F9, 1)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "x.flac")
        for what, fn in (("render_file_flac_f32 16 bits", lambda: sa.render_file_flac_f32(prg, 44100, path, 2, 4096, 16, 0, 0.5)[0]),
                         ("render_file_flac_dithered F9", lambda: sa.render_file_flac_dithered(prg, 44100, path, spec, 2, 4096, 0, 0.5)[0])):
            walls = []
            for _ in range(REPS):
                t = time.perf_counter()
                n = fn()
                walls.append(round(time.perf_counter() - t, 6))
            note(what=what, frames=n, bytes=os.path.getsize(path), wall_s=walls)


{"kernels": kernels, "writers": writers}[sys.argv[1]]()
if len(sys.argv) > 2:
    open(sys.argv[2], "a").write("\n".join(lines) + "\n")
