"""The FLAC decoder on the device and the encoders' verify mode (include/saugns_amd.h, section "FLAC", paragraph "Verify":
sauAmd_Flac_set_verify, sauAmd_Flac_verify, sauAmd_set_flac_file_verify; kernel: saugns_amd/csrc/k_flac_dec.h over
sau_flac_dec.h's arithmetic).

1, 2: the product's flac_decode_kernel, both forms and both widths, compiled for gfx950 over frames the test supplies
(tests/hooks_flac_verify): the host test's valid, hand-built, corrupted, bit-flipped and truncated frames decode to the host
restatement's status, length and samples (tests/test_flac_verify_sanitize.py is where the shared reader is shown to stay inside
the frame; the `fuzzed` fixture runs it ahead of the hook test); the verify form finds a sample that is off by one LSB, and nothing else.
3: all five kinds of encoder with verify on: every block checked, none bad, the bytes those of the same feeds with verify off.
4: every FLAC file writer with the process-wide switch on: the same file, byte for byte."""
import ctypes as C
import os
import subprocess
import sys
import traceback

import numpy as np
import pytest

import flac_verify_cases as fc
from conftest import load_program
from test_flac_verify_host import _one_of_each_type
from test_flac_verify_sanitize import run_fuzz

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOKS = os.path.join(ROOT, "tests", "hooks_flac_verify")


@pytest.fixture(scope="module")
def vhooks():
    """tests/hooks_flac_verify/libsaugns_amd_flac_verify_hooks.so: flac_decode_kernel as the product's source, for gfx950"""
    subprocess.check_call(["make", "-s", "-C", HOOKS])
    L = C.CDLL(os.path.join(HOOKS, "libsaugns_amd_flac_verify_hooks.so"))
    L.sauAmd_flac_verify_hook_run.restype = C.c_int
    L.sauAmd_flac_verify_hook_run.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32] + [C.c_void_p] * 4 + [C.c_size_t] + \
        [C.c_void_p] * 3 + [C.c_size_t] + [C.c_void_p] * 4
    return L


@pytest.fixture(scope="module")
def fuzzed(sa, tmp_path_factory):
    """the sanitizer program over the same source (host code only, no GPU) has passed before a corrupt frame reaches the kernel:
    it is the evidence that the reader the kernel shares stays inside the frame"""
    run_fuzz(sa, tmp_path_factory.mktemp("flac_verify_fuzz"))


def run_kernel(L, bits, verify, channels, B, rows, frames, expect=None):
    """rows: (block0, n_blocks, last_n) each; frames: the jobs' bytes, row after row; expect: int32 [n_rows, pitch] (verify form)
    -> (status [jobs], n [jobs], samples [jobs, B, channels] or None, rec [n_rows, 3])"""
    jobs = sum(r[1] for r in rows)
    assert jobs == len(frames)
    block0 = np.array([r[0] for r in rows], np.uint64)
    n_blocks = np.array([r[1] for r in rows], np.uint32)
    last_n = np.array([r[2] for r in rows], np.uint32)
    # POISON between the frames: a read outside a frame finds no neighbour's bytes that happen to fit
    parts, off, at = [], [], 0
    for fr in frames:
        off.append(at)
        parts.append(bytes(fr) + b"\xa5" * 3)
        at += len(fr) + 3
    data = np.frombuffer(b"".join(parts) + b"\xa5", np.uint8).copy()
    off = np.array(off, np.uint32)
    ln = np.array([len(fr) for fr in frames], np.uint32)
    status = np.full(jobs, 99, np.uint32)
    n = np.full(jobs, 99, np.uint32)
    samples = None if verify else np.zeros((jobs, B, channels), np.int32)
    rec = np.zeros((len(rows), 3), np.uint64)
    ex = None if expect is None else np.ascontiguousarray(expect, np.int32)
    ok = L.sauAmd_flac_verify_hook_run(bits, 1 if verify else 0, channels, B, len(rows), block0.ctypes.data, n_blocks.ctypes.data,
                                       last_n.ctypes.data, data.ctypes.data, len(data), off.ctypes.data, ln.ctypes.data,
                                       None if ex is None else ex.ctypes.data, 0 if ex is None else ex.shape[1], status.ctypes.data,
                                       n.ctypes.data, None if samples is None else samples.ctypes.data, rec.ctypes.data)
    assert ok == 1, "the hook refused its arguments or a HIP call failed"
    return status, n, samples, rec


def decode_table(sa):
    """(frame, channels, B, bits, number, what): the host test's valid frames (n = 1, 5, B of every kind and mode), the hand-built
    ones, the refusals, and of one frame per subframe type and width every 29th single-bit flip and every 7th prefix"""
    out = []
    for c in fc.valid_cases(sa):
        if c["n"] in (1, 5, c["B"]):
            out.append((c["frame"], c["channels"], c["B"], c["bits"], c["number"], "valid %s %s n %d" % (c["mode"], c["kind"], c["n"])))
    for name, fr, ch, B, bits, number, x in fc.handmade_valid():
        out.append((fr, ch, B, bits, number, name))
    for name, fr, ch, B, bits, number, status in fc.corrupt_cases():
        out.append((fr, ch, B, bits, number, name))
    for (bits, t), c in sorted(_one_of_each_type(sa).items()):
        fr = c["frame"]
        for bit in list(range(0, min(128, 8 * len(fr)))) + list(range(128, 8 * len(fr), 29)):
            m = bytearray(fr)
            m[bit >> 3] ^= 0x80 >> (bit & 7)
            out.append((bytes(m), c["channels"], c["B"], bits, c["number"], "%s %d bits, bit %d flipped" % (t, bits, bit)))
        for cut in list(range(0, len(fr), 7)) + [len(fr) - 1]:
            out.append((fr[:cut], c["channels"], c["B"], bits, c["number"], "%s %d bits, cut at %d" % (t, bits, cut)))
    return out


def test_decode_form_equals_the_host_restatement(sa, fuzzed, vhooks):
    """status and n equal sauAmd_flac_decode_block's for every job, and the samples wherever the status is OK"""
    table = decode_table(sa)
    seen = set()
    for bits in (16, 24):
        for channels in (1, 2):
            for B in fc.BLOCKS:
                jobs = [t for t in table if (t[1], t[2], t[3]) == (channels, B, bits)]
                if not jobs:
                    continue
                rows = [(t[4], 1, B) for t in jobs]  # (a row per frame: its block0 is the expected number)
                status, n, samples, rec = run_kernel(vhooks, bits, False, channels, B, rows, [t[0] for t in jobs])
                for k, (fr, _, _, _, number, what) in enumerate(jobs):
                    st, size, want = sa.flac_decode_block(fr, channels, B, bits, number)
                    assert status[k] == st, (what, fc.NAMES[status[k]] if status[k] < 12 else status[k], fc.NAMES[st])
                    assert n[k] == (len(want) if st == fc.OK else 0), what
                    if st == fc.OK:
                        assert (samples[k, :n[k]] == want).all(), what
                    assert rec[k][0] == 1 and rec[k][1] == (st != fc.OK), what
                    assert st == fc.OK or rec[k][2] == (number << 8 | st), what
                    seen.add(st)
    assert seen == set(range(11)), sorted(seen)  # (every status but MISMATCH, which is the verify form's)


def _streams(sa, mode, channels, B, shape, seed):
    """rows of whole blocks and a short last one -> (rows for run_kernel, the jobs' frames, expect [n_rows, pitch])"""
    bits = fc.MODES[mode][0]
    kinds = fc.kinds_of(mode)
    rows, frames, xs = [], [], []
    for r, (block0, blocks, tail) in enumerate(shape):
        parts = [fc.material(mode, kinds[(seed + r + k) % len(kinds)], B, channels, B) for k in range(blocks)]
        parts.append(fc.material(mode, "noise", tail, channels, B))
        x = np.concatenate(parts)
        for k in range(blocks + 1):
            frames.append(fc.encode(sa, mode, x[k * B * channels:(k + 1) * B * channels], channels, B, block0 + k))
        rows.append((block0, blocks + 1, tail))
        xs.append(x)
    pitch = max(len(x) for x in xs) + 5
    expect = np.full((len(xs), pitch), 0x5a5a5a, np.int32)
    for r, x in enumerate(xs):
        expect[r, :len(x)] = x
    return bits, rows, frames, expect


@pytest.mark.parametrize("mode,channels,B", [("lpc", 1, 256), ("lpc", 2, 256), ("lpc24", 1, 256), ("lpc24", 2, 256), ("encode_block", 2, 4096),
                                             ("s32", 2, 4096)])
def test_verify_form_finds_one_lsb(sa, vhooks, mode, channels, B):
    """frames of the host restatement with the true samples as the expected ones: no bad block; then one expected sample off by
    one LSB at the first, a middle and the last frame of a block, in each channel: exactly those jobs report MISMATCH, and the
    row's record counts them and names the lowest"""
    shape = [(0, 3, 17), (126, 2, 1), (70000, 3, B - 1)]
    bits, rows, frames, expect = _streams(sa, mode, channels, B, shape, seed=channels + B)
    status, n, _, rec = run_kernel(vhooks, bits, True, channels, B, rows, frames, expect)
    want_n = [B] * 3 + [17] + [B] * 2 + [1] + [B] * 3 + [B - 1]
    assert (status == fc.OK).all() and list(n) == want_n
    assert [list(map(int, r)) for r in rec] == [[4, 0, 2**64 - 1], [3, 0, 2**64 - 1], [4, 0, 2**64 - 1]]
    # (row, block of the row, frame of the block, channel, +-1)
    hits = [(0, 1, 0, 0, 1), (0, 3, 16, channels - 1, -1), (1, 2, 0, 0, -1), (2, 0, B // 2 + 3, channels - 1, 1), (2, 2, B - 1, 0, 1),
            (2, 3, B - 2, 0, -1)]
    job0 = [0, 4, 7]
    bad = expect.copy()
    for r, k, i, c, d in hits:
        bad[r, (k * B + i) * channels + c] += d
    status, n, _, rec = run_kernel(vhooks, bits, True, channels, B, rows, frames, bad)
    want = np.zeros(len(frames), np.uint32)
    for r, k, _, _, _ in hits:
        want[job0[r] + k] = fc.MISMATCH
    assert (status == want).all(), (list(status), list(want))
    for r, (block0, blocks, _) in enumerate(rows):
        mine = sorted(k for rr, k, *_ in hits if rr == r)
        assert [int(v) for v in rec[r]] == [blocks, len(mine), ((block0 + mine[0]) << 8) | fc.MISMATCH], (r, rec[r])
    # a frame of the right samples under the wrong plan: another length, another number
    rows2 = [(0, 4, 18)] + rows[1:]
    status, _, _, _ = run_kernel(vhooks, bits, True, channels, B, rows2, frames, np.pad(expect, ((0, 0), (0, 8))))
    assert status[3] == fc.MISMATCH and (np.delete(status, 3) == fc.OK).all()
    rows3 = [(1, 4, 17)] + rows[1:]
    status, _, _, rec = run_kernel(vhooks, bits, True, channels, B, rows3, frames, expect)
    assert (status[:4] == fc.NUMBER).all() and (status[4:] == fc.OK).all() and [int(v) for v in rec[0]] == [4, 4, (1 << 8) | fc.NUMBER]


# ---- 3. through the API: in a process of its own with torch imported first (tests/test_gpu_flac24.py's fixture) -------------

ENCODERS = ("int16", "int16 lpc", "f32 16", "f32 24", "lpc24")


def _make(b, kind, n_rows, ch, B):
    if kind == "int16":
        return b.create_flac(n_rows, ch, B), 16, False
    if kind == "int16 lpc":
        return b.create_flac(n_rows, ch, B, 8), 16, False
    if kind == "f32 16":
        return b.create_flac_f32(n_rows, ch, B, bits=16, max_lpc_order=8), 16, True
    if kind == "f32 24":
        return b.create_flac_f32(n_rows, ch, B, bits=24), 24, True
    return b.create_flac_lpc24(n_rows, ch, B, 8), 24, True


def _refused(fn, *args):
    try:
        fn(*args)
    except RuntimeError as e:
        assert "bad argument" in str(e), str(e)
        return
    raise AssertionError("not refused")


def api_main(torch, sa, b):
    from test_gpu_flac24 import stage, stage16
    rng = np.random.default_rng(4242)
    for kind in ENCODERS:
        for B in (256, 4096):
            for ch in (1, 2):
                lengths = [3 * B + 17, 0, B + B // 2 + 1, 2 * B - 1, 5][:4 if B == 4096 else 5]
                n_rows = len(lengths)
                total = sum(lengths)
                if kind in ("int16", "int16 lpc"):
                    x = [(rng.integers(-3000, 3001, n * ch) + np.round(9000 * np.sin(np.arange(n * ch) / 23.0))).astype(np.int16) for n in lengths]
                else:
                    x = [(0.4 * np.sin(np.arange(n * ch) / 31.0) + rng.uniform(-0.01, 0.01, n * ch)).astype(np.float32) for n in lengths]
                cuts = [sorted(set(rng.integers(0, n + 1, 3).tolist() + [n])) for n in lengths]
                out = {}
                for verify in (False, True):
                    e, bits, f32 = _make(b, kind, n_rows, ch, B)
                    if verify:
                        e.set_verify(True)
                    else:
                        _refused(e.verify)  # (verify is off)
                    for rep in range(2 if verify else 1):
                        keep, cur, data = [], [0] * n_rows, [b""] * n_rows
                        for step in range(4):
                            fr = [(cuts[r][step] if step < len(cuts[r]) else lengths[r]) - cur[r] for r in range(n_rows)]
                            piece = [x[r][cur[r] * ch:(cur[r] + fr[r]) * ch] for r in range(n_rows)]
                            if f32:
                                ptr, pitch = stage(torch, keep, piece)
                                e.feed_f32(ptr, pitch, fr, None, finish=step == 3)
                            else:
                                ptr, pitch = stage16(torch, keep, piece)
                                e.feed(ptr, pitch, fr, finish=step == 3)
                            cur = [cur[r] + fr[r] for r in range(n_rows)]
                            if step == 0 and sum(fr):
                                _refused(e.set_verify, not verify)  # (behind a feed)
                            if step % 2:
                                got, _ = e.read()
                                data = [data[r] + got[r] for r in range(n_rows)]
                        assert cur == lengths
                        rec = e.verify() if verify else None
                        got, info = e.read(reset=True)
                        data = [data[r] + got[r] for r in range(n_rows)]
                        if verify:
                            assert [v["blocks"] for v in rec] == [i["blocks"] for i in info] == [-(-n // B) for n in lengths], (kind, B, ch, rec)
                            assert all(v["bad_blocks"] == 0 and v["first_status"] == 0 for v in rec), (kind, B, ch, rec)
                            zero = e.verify()  # (the record is zero behind the reset, and the setting still holds)
                            assert all(v == dict(blocks=0, bad_blocks=0, first_bad_block=0, first_status=0) for v in zero), zero
                        out[(verify, rep)] = data
                    e.close()
                assert out[(False, 0)] == out[(True, 0)] == out[(True, 1)], (kind, B, ch)
                assert sum(len(d) for d in out[(True, 0)]) > 0 and total > 0
        print("verify api %s ok" % kind)


def torch_main():
    """every kind of encoder on one batch's device; a kind that fails ends the process -- nothing more is started on the device"""
    import torch
    import saugns_amd as sa
    from saugns_amd import voicebank as vb
    b = sa.Batch([vb.build_program([vb.Op("sin", freq=200.0, time_ms=10)])], 44100)  # (never run: its device is all that is used)
    try:
        api_main(torch, sa, b)
    except Exception:
        print("verify api FAILED\n%s" % traceback.format_exc())
    b.close()


TORCH = r"""
import sys
import torch  # (before the library: tests/test_gpu_flac24.py)
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_flac_verify
test_gpu_flac_verify.torch_main()
"""


@pytest.fixture(scope="module")
def torch_run():
    run = subprocess.run([sys.executable, "-c", TORCH, ROOT], capture_output=True, text=True, timeout=600)
    print(run.stdout[-6000:])
    return run


@pytest.mark.parametrize("kind", ENCODERS)
def test_verify_through_the_api(torch_run, kind):
    """B = 256 and 4096, mono and stereo, rows of different lengths (one of them empty) fed in ragged pieces cut at seeded random
    places, a finish that leaves a short block: `blocks` is sauAmd_Flac_read's, no block is bad, the bytes are those of the same
    feeds with verify off, behind a read with reset the record is zero and the setting holds (the second round is verified too);
    set_verify behind a feed and sauAmd_Flac_verify with verify off are refused"""
    assert "verify api %s ok" % kind in torch_run.stdout, (torch_run.returncode, torch_run.stdout[-4000:], torch_run.stderr[-4000:])
    if kind == ENCODERS[-1]:
        assert torch_run.returncode == 0, (torch_run.stdout[-2000:], torch_run.stderr[-4000:])


# ---- 4. the writers --------------------------------------------------------------------------------------------------------

RATE = 8000
FILE_KEY = "devtests__voice-reuse"


def _writers(sa):
    spec = sa.dither_preset(sa.DITHER_E5, 4)
    return [
        ("flac", lambda p, path: sa.render_file_flac(p, RATE, path, 2, 256)),
        ("flac_lpc", lambda p, path: sa.render_file_flac(p, RATE, path, 2, 256, max_lpc_order=8)),
        ("flac_f32 16", lambda p, path: sa.render_file_flac_f32(p, RATE, path, 2, 256, bits=16, max_lpc_order=8, gain=0.5)),
        ("flac_f32 24", lambda p, path: sa.render_file_flac_f32(p, RATE, path, 1, 256, bits=24, gain=0.5)),
        ("flac_lpc24", lambda p, path: sa.render_file_flac_lpc24(p, RATE, path, 2, 256, max_lpc_order=8, gain=0.5)),
        ("flac_loudness", lambda p, path: sa.render_file_flac_loudness(p, RATE, path, 2, 256, bits=24, limited=False)),
        ("flac_loudness limited", lambda p, path: sa.render_file_flac_loudness(p, RATE, path, 2, 256, bits=16, max_lpc_order=8, limited=True)),
        ("flac_dithered", lambda p, path: sa.render_file_flac_dithered(p, RATE, path, spec, 2, 256, max_lpc_order=8)),
    ]


@pytest.mark.parametrize("which", range(8))
def test_writers_verify_and_write_the_same_file(sa, tmp_path, which):
    """with sauAmd_set_flac_file_verify(1) every FLAC writer succeeds and writes the file it writes with the switch off; the
    switch returns its previous value"""
    name, write = _writers(sa)[which]
    prg = load_program(sa, FILE_KEY)
    off, on = str(tmp_path / "off.flac"), str(tmp_path / "on.flac")
    write(prg, off)
    was = sa.set_flac_file_verify(1)
    try:
        assert was == 0 and sa.set_flac_file_verify(1) == 1
        write(prg, on)
    finally:
        assert sa.set_flac_file_verify(was) == 1
    a, b = open(off, "rb").read(), open(on, "rb").read()
    assert len(a) > 42 + 100 and a == b, name
