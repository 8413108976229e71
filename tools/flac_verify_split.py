#!/usr/bin/env python3
"""Where flac_decode_kernel's time goes ("Verify"): single frames of one kind each through the kernel's decode form
(tests/hooks_flac_verify: the product's source for gfx950), one workgroup a launch, B = 4096, five launches a kind:
    rocprofv3 --kernel-trace --output-format csv -d DIR -o s -- python tools/flac_verify_split.py [out.jsonl]
The kinds, in launch order (the trace's dispatches are in the same order): per width and channels, a CONSTANT frame (no residual,
no restoration: loading, header, CRCs, the spread and the store), a VERBATIM frame (noise: the same with the most bytes, read by
all threads), FIXED frames (the serial parse and the serial FIXED restoration), LPC frames of order 8 (the same parse, and the
serial LPC restoration, eight multiply-adds a sample). One JSON line says what was launched: kind, subframe types, bytes;
    python tools/flac_verify_split.py --summary DIR/s_kernel_trace.csv out.jsonl > profiles/flac_verify_split_us.csv
makes a line per kind of the trace's durations."""
import csv
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import saugns_amd as sa  # noqa: E402
import flac_verify_cases as fc  # noqa: E402

if len(sys.argv) > 1 and sys.argv[1] == "--summary":  # --summary s_kernel_trace.csv flac_verify_split.jsonl: a CSV line per kind
    tr = [r for r in csv.DictReader(open(sys.argv[2])) if "flac_decode" in r["Kernel_Name"]]
    tr.sort(key=lambda r: int(r["Start_Timestamp"]))
    ns = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in tr]
    kinds = json.loads(open(sys.argv[3]).readline())["launched"]
    assert len(ns) == sum(k["launches"] for k in kinds)
    print("bits,channels,kind,subframes,frame_bytes,launches,min_us,median_us,max_us")
    at = 0
    for k in kinds:
        t = sorted(ns[at:at + k["launches"]])
        at += k["launches"]
        print("%d,%d,%s,%s,%d,%d,%.1f,%.1f,%.1f" % (k["bits"], k["channels"], k["kind"], "+".join(k["types"]), k["bytes"], len(t), t[0] / 1e3,
                                                    t[len(t) // 2] / 1e3, t[-1] / 1e3))
    sys.exit(0)

HOOKS = os.path.join(ROOT, "tests", "hooks_flac_verify")
subprocess.check_call(["make", "-s", "-C", HOOKS])
L = C.CDLL(os.path.join(HOOKS, "libsaugns_amd_flac_verify_hooks.so"))
L.sauAmd_flac_verify_hook_run.restype = C.c_int
L.sauAmd_flac_verify_hook_run.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32] + [C.c_void_p] * 4 + [C.c_size_t] + \
    [C.c_void_p] * 3 + [C.c_size_t] + [C.c_void_p] * 4
sa.lib()
B, REPS = 4096, 5
launched = []
for mode, kinds in (("lpc", ("silence", "noise", "steps", "burst", "sine", "pm")), ("lpc24", ("silence", "noise", "steps", "burst", "sine", "pm"))):
    bits = fc.MODES[mode][0]
    for channels in (1, 2):
        for kind in kinds:
            x = fc.material(mode, kind, B, channels, B)
            fr = fc.encode(sa, mode, x, channels, B, 0)
            types = list(fc.subframe_types(fr, channels, B, bits, 0))
            data = np.frombuffer(fr, np.uint8).copy()
            for _ in range(REPS):
                block0, n_blocks, last_n = np.zeros(1, np.uint64), np.ones(1, np.uint32), np.full(1, B, np.uint32)
                off, ln = np.zeros(1, np.uint32), np.full(1, len(fr), np.uint32)
                status, n, rec = np.zeros(1, np.uint32), np.zeros(1, np.uint32), np.zeros(3, np.uint64)
                samples = np.zeros(B * channels, np.int32)
                ok = L.sauAmd_flac_verify_hook_run(bits, 0, channels, B, 1, block0.ctypes.data, n_blocks.ctypes.data, last_n.ctypes.data,
                                                   data.ctypes.data, len(data), off.ctypes.data, ln.ctypes.data, None, 0, status.ctypes.data,
                                                   n.ctypes.data, samples.ctypes.data, rec.ctypes.data)
                assert ok == 1 and status[0] == 0 and n[0] == B and (samples == x).all(), (mode, kind, channels, status)
            launched.append(dict(bits=bits, channels=channels, kind=kind, types=types, bytes=len(fr), launches=REPS))
line = json.dumps(dict(what="split", B=B, launched=launched))
print(line)
if len(sys.argv) > 1:
    open(sys.argv[1], "a").write(line + "\n")
