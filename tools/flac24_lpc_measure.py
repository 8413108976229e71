#!/usr/bin/env python3
"""The 24-bit LPC mode's measurements (DESIGN §4.4 "LPC at 24 bits"; profiles/flac24_lpc_*):
    python tools/flac24_lpc_measure.py sizes [out.jsonl]
    python tools/flac24_lpc_measure.py feed <bits> <max_lpc_order> <feeds> [out.jsonl]
`sizes`: examples__rainy_thunder at 44100 Hz stereo, B = 4096, gain 0.5 through sauAmd_render_file_flac_lpc24 with max_lpc_order
0, 4 and 8: the files' bytes, and how many frames are longer than their M = 0 frame (the frames' sizes are the host
restatement's of the quantised float render, which every file is held against byte for byte).
`feed`: config 3's shape, one row of 1024 voices, 10 s at 44100 Hz stereo, B = 4096, rendered once in float (bits 24: fed to
sauAmd_Batch_create_flac_lpc24's encoder) or in int16 (bits 16: sauAmd_Batch_create_flac_lpc's), `feeds` times, every feed a
finish, timed by the wall clock around queue and wait; the streams are reset between feeds, their bytes not fetched. Under
`rocprofv3 --kernel-trace --stats` it gives the kernels' times of those feeds. One JSON line either way."""
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

mode = sys.argv[1]
RATE, B = 44100, 4096
if mode == "sizes":
    import numpy as np
    prg = sa.Program.from_image(open(os.path.join(ROOT, "tests", "golden", "programs", "examples__rainy_thunder.saup"), "rb").read())
    out = dict(program="examples__rainy_thunder", rate=RATE, channels=2, B=B, gain=0.5, bytes={}, frames=None, wall_s={})
    sizes = {}
    with tempfile.TemporaryDirectory() as d:
        wav = os.path.join(d, "x.wav")
        sa.render_file(prg, RATE, wav, sa.api.SNDFILE_WAV_F32, 2)
        q = sa.flac_quantize(np.frombuffer(open(wav, "rb").read(), "<f4", offset=58), 0.5, 24)
        for M in (0, 4, 8):
            path = os.path.join(d, "m%d.flac" % M)
            t = time.perf_counter()
            n, info = sa.render_file_flac_lpc24(prg, RATE, path, 2, B, max_lpc_order=M, gain=0.5)
            out["wall_s"][str(M)] = round(time.perf_counter() - t, 4)
            data = open(path, "rb").read()
            out["bytes"][str(M)] = len(data)
            out["frames"], out["blocks"] = n, info.blocks
            # the frames' sizes from the host restatement, which the file has to equal byte for byte
            host = [sa.flac_encode_block_lpc24(q[k * B * 2:(k + 1) * B * 2], 2, B, k, M) for k in range(info.blocks)]
            assert len(q) == 2 * n and b"".join(host) == data[42:], "the file is not the host restatement's"
            sizes[M] = [len(f) for f in host]
    out["frames_longer_than_m0"] = {str(M): sum(a > b for a, b in zip(sizes[M], sizes[0])) for M in (4, 8)}
    out["ratio_to_m0"] = {str(M): round(out["bytes"][str(M)] / out["bytes"]["0"], 4) for M in (4, 8)}
    tail = 2
else:
    bits, M, feeds = int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
    FRAMES = 441000
    b = sa.Batch([voicebank.config3(n=1024, seconds=10)], RATE)
    if bits == 24:
        b.run_f32(FRAMES, True, fetch=False)
        # (a library without the _lpc24 entry points -- the parent commit's, through SAU_AMD_LIB -- takes order 0 only)
        e = b.create_flac_lpc24(1, 2, B, M) if hasattr(sa.lib(), "sauAmd_Batch_create_flac_lpc24") or M else b.create_flac_f32(1, 2, B, bits=24)
    else:
        b.run(FRAMES, True, fetch=False)
        e = b.create_flac_lpc(1, 2, B, M)
    b.sync()
    walls, size = [], 0
    for _ in range(feeds):
        t = time.perf_counter()
        if bits == 24:
            e.feed_f32(b.device_pcm_f32(0), b.device_pcm_pitch(), [FRAMES], None, finish=True)
        else:
            e.feed(b.device_pcm(0), b.device_pcm_pitch(), [FRAMES], finish=True)
        size = sum(e.unread()[0])
        walls.append(round(time.perf_counter() - t, 6))
        n, info = (C.c_size_t * 1)(), (FlacInfo * 1)()
        if not sa.lib().sauAmd_Flac_read(e._e, None, None, n, info, 1):
            sys.exit("the reset failed: " + sa.api.last_error())
    e.close()
    b.close()
    out = dict(shape="config3 x 1024", lib=os.path.basename(os.environ.get("SAU_AMD_LIB") or "") or "in-tree", rate=RATE, frames=FRAMES, B=B, channels=2, bits=bits, max_lpc_order=M, feed_s=walls, best_feed_s=min(walls),
               bytes=size)
    tail = 5
line = json.dumps(out)
print(line)
if len(sys.argv) > tail:
    open(sys.argv[tail], "a").write(line + "\n")
