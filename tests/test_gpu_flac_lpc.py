"""The on-device FLAC encoder's LPC mode (include/saugns_amd.h, section "FLAC", "The LPC mode":
sauAmd_Batch_create_flac_lpc, sauAmd_render_file_flac_lpc; kernels: the <true> builds in saugns_amd/csrc/k_flac.h).

The header fixes the mode's integer sums and the order of its few f64 operations, so what the device delivers is compared
with the numpy restatement (tests/flac_lpc_model.py, held against its own independent decoder in tests/test_flac_lpc_host.py)
BYTE FOR BYTE, a sequence cut into feeds with itself in one piece, and an encoder of order 0 with the one
sauAmd_Batch_create_flac makes."""
import os
import subprocess
import sys
import traceback

import numpy as np
import pytest

import flac_lpc_model as mdl
from conftest import load_program
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATERIAL = mdl.KINDS + ("pm",)
POISON = 0x5a5b  # what lies between the rows: it would show in the bytes


def stage(torch, keep, rows, ch, extra=24):
    """rows: int16 arrays (interleaved) -> device rows at a pitch larger than the longest, POISON between and behind them"""
    width = (max(max(len(r) for r in rows), 8) + 7) // 8 * 8 + extra  # int16 elements; a multiple of 8: 16 bytes
    t = torch.full((len(rows), width), POISON, dtype=torch.int16, device="cuda")
    for r, x in enumerate(rows):
        if len(x):
            t[r, :len(x)] = torch.from_numpy(np.ascontiguousarray(x)).to("cuda")
    torch.cuda.synchronize()
    keep.append(t)  # (alive until the encoder has been read: the feed is asynchronous)
    return t.data_ptr(), width * 2


def material(kind, frames, ch, seed):
    return mdl.pm(frames, ch, seed) if kind == "pm" else mdl.crafted(kind, frames, ch, seed=seed)


def check_row(data, x, ch, B, M, info, what):
    want, sizes = mdl.encode_stream(x, ch, B, M)
    assert len(data) == len(want), (what, len(data), len(want))
    if data != want:
        at = next(i for i in range(len(want)) if data[i] != want[i])
        raise AssertionError((what, "first difference at byte", at, "of", len(want), data[at:at + 8].hex(), want[at:at + 8].hex()))
    got, s2, kinds = mdl.decode_frames(data, ch, B)
    assert s2 == sizes and (got == x).all(), what
    assert info == mdl.info(len(x) // ch, sizes), (what, info, mdl.info(len(x) // ch, sizes))
    assert all(s <= mdl.frame_bound(B, ch) for s in sizes)
    return kinds


# ---- 1. crafted rows in one feed --------------------------------------------------------------------------------------------

def bytes_main(torch, sa, b):
    case, seen = 0, set()
    for B in (256, 4096):
        for ch in (1, 2):
            for M in (1, 8):
                frames = 2 * B + 37
                kinds = [MATERIAL[(case * 3 + r) % len(MATERIAL)] for r in range(3)]
                x = [material(k, frames, ch, case + r) for r, k in enumerate(kinds)]
                keep, out = [], []
                e = b.create_flac(3, ch, B, max_lpc_order=M)
                for _ in range(2):
                    ptr, pitch = stage(torch, keep, x, ch, extra=8 * (1 + case % 3))
                    e.feed(ptr, pitch, [frames] * 3, finish=True)
                    need, info_q = e.unread()
                    data, info = e.read(reset=True)
                    assert need == [len(d) for d in data] and info_q == info
                    out.append(data)
                e.close()
                assert out[0] == out[1], ("called twice", B, ch, M)
                for r in range(3):
                    kd = check_row(out[0][r], x[r], ch, B, M, info[r], ("B", B, "ch", ch, "M", M, kinds[r]))
                    seen.update(k.split("/")[0] for f in kd for k in f)
                case += 1
    print("cases:", case, sorted(seen))
    assert {"lpc1", "constant", "verbatim"} <= seen and any(k.startswith("fixed") for k in seen), seen
    assert any(k.startswith("lpc") and int(k[3:]) >= 5 for k in seen), seen


# ---- 2. feeds -----------------------------------------------------------------------------------------------------------------

def feeds_main(torch, sa, b):
    M = 8
    for B, ch in ((256, 2), (4096, 1)):
        lengths = [5 * B + 37, 0, 4 * B, 3 * B + 1]
        kinds = ["pm", "silence", "anti", "unrelated"]
        x = [material(k, n, ch, r) for r, (k, n) in enumerate(zip(kinds, lengths))]
        pieces = [1, B - 1, B + 1, 2 * B, 6 * B]
        seen = set()
        e = b.create_flac(4, ch, B, max_lpc_order=M)
        keep, got, cur = [], [b""] * 4, [0] * 4
        for i, n in enumerate(pieces):
            last = i == len(pieces) - 1
            fr = [0 if (i + r) % 5 == 4 and not last else min(n, lengths[r] - cur[r]) for r in range(4)]
            ptr, pitch = stage(torch, keep, [x[r][cur[r] * ch:(cur[r] + fr[r]) * ch] for r in range(4)], ch)
            e.feed(ptr, pitch, fr, finish=last)
            for r in range(4):
                cur[r] += fr[r]
            data, info = e.read()  # reads in between: what is complete so far, nothing twice
            for r in range(4):
                got[r] += data[r]
                assert info[r]["frames"] == cur[r] and info[r]["bytes"] == len(got[r])
        assert cur == lengths
        _, info = e.read()
        # in one piece, behind a reset: the same bytes
        e.read(reset=True)
        ptr, pitch = stage(torch, keep, x, ch)
        e.feed(ptr, pitch, lengths, finish=True)
        data, info2 = e.read()
        assert data == got and info2 == info, ("one piece", B, ch)
        e.close()
        for r in range(4):
            kd = check_row(got[r], x[r], ch, B, M, info[r], ("feeds", B, ch, kinds[r]))
            seen.update(k.split("/")[0] for f in kd for k in f)
        print("feeds", B, ch, sorted(seen))
        assert B != 4096 or "lpc8" in seen, seen  # (the mono anti-phase tone's first block: the highest order)


# ---- 3. order 0 by either entry point -------------------------------------------------------------------------------------

def order0_main(torch, sa, b):
    import flac_model
    for B, ch in ((256, 2), (4096, 1)):
        frames = 2 * B + 37
        kinds = ["pm", "sine", "burst"]
        x = [material(k, frames, ch, r) for r, k in enumerate(kinds)]
        keep, out = [], []
        for make in (b.create_flac_lpc, b.create_flac):
            e = make(3, ch, B)
            ptr, pitch = stage(torch, keep, x, ch)
            e.feed(ptr, pitch, [frames] * 3, finish=True)
            out.append(e.read())
            e.close()
        assert out[0] == out[1], ("order 0", B, ch)
        for r in range(3):
            assert out[0][0][r] == flac_model.encode_stream(x[r], ch, B)[0], ("order 0 against the model", B, ch, kinds[r])


SECTIONS = [("bytes", bytes_main), ("feeds", feeds_main), ("order0", order0_main)]


def torch_main():
    """(in a process of its own, torch imported first: see the fixture) every section on one batch's device; a section that fails
    ends the process -- nothing more is started on the device behind a failure"""
    import torch
    import saugns_amd as sa
    from saugns_amd import voicebank as vb
    b = sa.Batch([vb.build_program([vb.Op("sin", freq=200.0, time_ms=10)])], 44100)  # (never run: its device is all that is used)
    for name, fn in SECTIONS:
        try:
            fn(torch, sa, b)
        except Exception:
            print("flac lpc %s FAILED\n%s" % (name, traceback.format_exc()))
            break
        print("flac lpc %s ok" % name)
    b.close()


TORCH = r"""
import sys
import torch  # (before the library: torch's wheel brings a HIP runtime of its own, and a process has room for one -- api.Batch.device_tensor)
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_flac_lpc
test_gpu_flac_lpc.torch_main()
"""


@pytest.fixture(scope="module")
def torch_run():
    """The tests on rows of device memory of the test's own (torch tensors) share one process: torch has to be imported before
    the library is loaded, in this one the library is loaded already, and one import serves them all."""
    return subprocess.run([sys.executable, "-c", TORCH, ROOT], capture_output=True, text=True, timeout=600)


def _section(run, name):
    assert "flac lpc %s ok" % name in run.stdout, (run.returncode, run.stdout[-4000:], run.stderr[-4000:])


def test_crafted_rows(torch_run):
    """3 rows x mono and stereo x B in 256, 4096 x max_lpc_order in 1, 8, 2 B + 37 frames each (two whole blocks of 16 finest
    partitions and the short tail), the rows' contents rotating through flac_model's kinds and pm; the pitch larger than the
    rows with a pattern between them: the bytes equal the model's byte for byte, the model's decoder returns the input, the
    records equal what the model counts, two identical calls give identical bytes, and subframes of every type occur."""
    _section(torch_run, "bytes")


def test_feeds(torch_run):
    """four rows of unequal length, one empty, cut into feeds of 1, B - 1, B + 1, 2 B frames and the rest, some rows given
    nothing in some feeds, with a read behind every feed: the same bytes as in one piece and as the model's (B = 256 stereo,
    B = 4096 mono, max_lpc_order 8)."""
    _section(torch_run, "feeds")


def test_order_0_by_either_entry_point(torch_run):
    """an encoder of max_lpc_order 0 from sauAmd_Batch_create_flac_lpc and one from sauAmd_Batch_create_flac, fed the same rows:
    equal bytes and records, the bytes of flac_model's encoder"""
    _section(torch_run, "order0")
    assert torch_run.returncode == 0, (torch_run.stdout[-2000:], torch_run.stderr[-4000:])


# ---- 4. render_file_flac with max_lpc_order -------------------------------------------------------------------------------

@pytest.mark.parametrize("channels", [1, 2])
def test_render_file_flac_lpc_holds_what_render_file_writes(sa, tmp_path, channels):
    prg = load_program(sa, "devtests__voice-reuse")
    raw, flac, plain = str(tmp_path / "x.raw"), str(tmp_path / "x.flac"), str(tmp_path / "y.flac")
    n = sa.render_file(prg, 8000, raw, sa.api.SNDFILE_RAW, channels)
    frames, info = sa.render_file_flac(prg, 8000, flac, channels, 1024, max_lpc_order=8)
    frames0, _ = sa.render_file_flac(prg, 8000, plain, channels, 1024)
    want = np.fromfile(raw, "<i2")
    data = open(flac, "rb").read()
    assert frames == frames0 == n == info.frames and len(want) == n * channels and np.abs(want.astype(int)).max() > 1000
    h, x, kinds = mdl.decode_file(data)
    assert (h["srate"], h["channels"], h["max_block"]) == (8000, channels, 1024)
    assert (x == want).all()
    assert data[:42] == sa.flac_header(8000, channels, 1024, info)
    d = info.as_dict()
    assert d["blocks"] == (n + 1023) // 1024 and d["bytes"] == len(data) - 42 and d["min_frame_bytes"] <= d["max_frame_bytes"]
    print("FLAC with max_lpc_order 8 / 0: %d / %d bytes; subframes: %s" % (len(data), os.path.getsize(plain),
                                                                         sorted({k.split("/")[0] for f in kinds for k in f})))
    assert len(data) <= os.path.getsize(plain)
    assert data[42:] == mdl.encode_stream(want, channels, 1024, 8)[0]
