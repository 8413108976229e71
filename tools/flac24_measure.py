#!/usr/bin/env python3
"""What a float-fed FLAC feed costs beside the int16 encoder's (profiles/flac24_*):
    python tools/flac24_measure.py <one|batch> <batches> <feeds per batch> [out.jsonl]
`one`: config 3's shape, one row of 1024 voices; `batch`: 64 rows of 16 voices each. 10 s at 44100 Hz stereo, B = 4096: one run
of 441000 frames per batch. Per batch round three batches of the same programs are made: one runs in float and keeps its rows
on the device, one runs in float and fetches them, one runs in int16. The float rows are fed to a 24-bit and to a 16-bit float-fed
encoder, the int16 rows to the int16 encoder, `feeds per batch` times each by turns, every feed a finish, timed by the wall clock
around queue and wait (the wait is the read that fetches the rows' sizes); the streams are reset between feeds, their bytes
not fetched. One JSON line:
every time taken, the encoded bytes and which is least. Under `rocprofv3 --kernel-trace --stats` with 1 1 it gives the kernels'
shares of one such round."""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import saugns_amd as sa  # noqa: E402
from saugns_amd import voicebank  # noqa: E402
from saugns_amd.api import FlacInfo  # noqa: E402

shape, batches, feeds = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
RATE, FRAMES, B = 44100, 441000, 4096
if shape == "one":
    def programs():
        return [voicebank.config3(n=1024, seconds=10)]
else:
    def programs():
        return [voicebank.config3(n=16, seconds=10) for _ in range(64)]


def reset(e):
    """new streams without fetching the bytes: what is unread goes"""
    n, info = (C.c_size_t * e.n_rows)(), (FlacInfo * e.n_rows)()
    if not sa.lib().sauAmd_Flac_read(e._e, None, None, n, info, 1):
        sys.exit("the reset failed: " + sa.api.last_error())


def timed(fn):
    t = time.perf_counter()
    fn()
    return round(time.perf_counter() - t, 6)


out = dict(shape=shape, rate=RATE, frames=FRAMES, B=B, channels=2, run_f32_s=[], run_f32_fetch_s=[], run_s16_s=[], feed24_s=[],
           feed16f_s=[], feed16_s=[])
for _ in range(batches):
    prgs = programs()
    n = len(prgs)
    bf, bh, bi = sa.Batch(prgs, RATE), sa.Batch(prgs, RATE), sa.Batch(prgs, RATE)

    def run_dev(b, f32):
        (b.run_f32 if f32 else b.run)(FRAMES, True, fetch=False)
        b.sync()

    out["run_f32_s"].append(timed(lambda: run_dev(bf, True)))
    out["run_f32_fetch_s"].append(timed(lambda: bh.run_f32(FRAMES, True)))
    out["run_s16_s"].append(timed(lambda: run_dev(bi, False)))
    e24 = bf.create_flac_f32(n, 2, B, bits=24)
    e16f = bf.create_flac_f32(n, 2, B, bits=16)
    e16 = bi.create_flac(n, 2, B)
    fr = [FRAMES] * n

    def feed(e, f32):
        b = bf if f32 else bi
        if f32:
            e.feed_f32(b.device_pcm_f32(0), b.device_pcm_pitch(), fr, None, finish=True)
        else:
            e.feed(b.device_pcm(0), b.device_pcm_pitch(), fr, finish=True)
        return e.unread()[0]

    for _ in range(feeds):
        for key, e, f32 in (("feed24_s", e24, True), ("feed16f_s", e16f, True), ("feed16_s", e16, False)):
            size = []
            out[key].append(timed(lambda: size.append(sum(feed(e, f32)))))
            out[key.replace("_s", "_bytes")] = size[0]
            reset(e)
    out["rows"] = n
    for e in (e24, e16f, e16):
        e.close()
    for b in (bf, bh, bi):
        b.close()
out["float_bytes"] = out["rows"] * FRAMES * 2 * 4
for key in ("run_f32_s", "run_f32_fetch_s", "run_s16_s", "feed24_s", "feed16f_s", "feed16_s"):
    out["best_" + key] = min(out[key])
line = json.dumps(out)
print(line)
if len(sys.argv) > 4:
    open(sys.argv[4], "a").write(line + "\n")
