"""The on-device FLAC encoder (include/saugns_amd.h, section "FLAC": sauAmd_Batch_create_flac, sauAmd_Flac_feed, sauAmd_Flac_read,
sauAmd_render_file_flac; kernels: saugns_amd/csrc/k_flac.h).

The header fixes the format and every choice in integers, and the bytes are a function of the fed sequence only, so what the
device delivers is compared with the numpy restatement (tests/flac_model.py, held against its own independent decoder in
tests/test_flac_host.py) BYTE FOR BYTE, and a sequence cut into feeds of any lengths with itself in one piece."""
import os
import subprocess
import sys
import traceback

import numpy as np
import pytest

import flac_model as mdl
from conftest import load_program

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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


def check_row(data, x, ch, B, info, what):
    want, sizes = mdl.encode_stream(x, ch, B)
    assert len(data) == len(want), (what, len(data), len(want))
    if data != want:
        at = next(i for i in range(len(want)) if data[i] != want[i])
        raise AssertionError((what, "first difference at byte", at, "of", len(want), data[at:at + 8].hex(), want[at:at + 8].hex()))
    got, s2, _ = mdl.decode_frames(data, ch, B)
    assert s2 == sizes and (got == x).all(), what
    assert info == mdl.info(len(x) // ch, sizes), (what, info, mdl.info(len(x) // ch, sizes))
    assert all(s <= mdl.frame_bound(B, ch) for s in sizes)


# ---- 1. crafted rows in one feed --------------------------------------------------------------------------------------------

def bytes_main(torch, sa, b):
    case = 0
    for B in (256, 1024, 4096):
        for ch in (1, 2):
            frames = 3 * B + 37
            kinds = [mdl.KINDS[(case * 3 + r) % len(mdl.KINDS)] for r in range(3)]
            x = [mdl.crafted(k, frames, ch, seed=case + r) for r, k in enumerate(kinds)]
            keep, out = [], []
            e = b.create_flac(3, ch, B)
            for _ in range(2):
                ptr, pitch = stage(torch, keep, x, ch, extra=8 * (1 + case % 3))
                e.feed(ptr, pitch, [frames] * 3, finish=True)
                need, info_q = e.unread()
                data, info = e.read(reset=True)
                assert need == [len(d) for d in data] and info_q == info
                out.append(data)
            e.close()
            assert out[0] == out[1], ("called twice", B, ch)
            for r in range(3):
                check_row(out[0][r], x[r], ch, B, info[r], ("B", B, "ch", ch, kinds[r]))
            case += 1
    print("cases:", case)


# ---- 2. feeds -----------------------------------------------------------------------------------------------------------------

def feeds_main(torch, sa, b):
    for B, ch in ((256, 2), (1024, 1), (4096, 2)):
        lengths = [5 * B + 37, 0, 4 * B, 3 * B + 1]
        kinds = ["sine", "silence", "burst", "unrelated"]
        x = [mdl.crafted(k, n, ch, seed=r) for r, (k, n) in enumerate(zip(kinds, lengths))]
        pieces = [1, B - 1, B + 1, 2 * B, 6 * B]
        e = b.create_flac(4, ch, B)
        keep, got, cur = [], [b""] * 4, [0] * 4
        for i, n in enumerate(pieces):
            last = i == len(pieces) - 1
            fr = [0 if (i + r) % 5 == 4 and not last else min(n, lengths[r] - cur[r]) for r in range(4)]
            ptr, pitch = stage(torch, keep, [x[r][cur[r] * ch:(cur[r] + fr[r]) * ch] for r in range(4)], ch)
            e.feed(ptr, pitch, fr, finish=last)
            for r in range(4):
                cur[r] += fr[r]
            if i % 2 == 1 or last:  # reads in between: what is complete so far, nothing twice
                data, info = e.read()
                for r in range(4):
                    got[r] += data[r]
                    assert info[r]["frames"] == cur[r] and info[r]["bytes"] == len(got[r])
                    assert info[r]["blocks"] == (cur[r] + (B - 1 if last else 0)) // B
                assert e.unread()[0] == [0] * 4
        assert cur == lengths
        _, info = e.read()
        for r in range(4):
            check_row(got[r], x[r], ch, B, info[r], ("feeds", B, ch, kinds[r]))
        # in one piece, behind a reset: the same bytes
        e.read(reset=True)
        ptr, pitch = stage(torch, keep, x, ch)
        e.feed(ptr, pitch, lengths, finish=True)
        data, info2 = e.read()
        assert data == got and info2 == info, ("one piece", B, ch)
        e.close()


# ---- 3. frame numbers of two and three bytes ---------------------------------------------------------------------------------

def numbers_main(torch, sa, b):
    B = 256
    for blocks, ch in ((130, 2), (2050, 1)):
        frames = blocks * B - 11
        x = np.zeros(frames * ch, np.int16)
        for k in (0, 126, 127, 128, 129, 2046, 2047, 2048, 2049):  # a tone in the blocks around the changes of length
            if k < blocks:
                n = min(B, frames - k * B)
                x[k * B * ch:(k * B + n) * ch] = mdl.crafted("sine", n, ch, seed=k)
        keep = []
        e = b.create_flac(1, ch, B)
        ptr, pitch = stage(torch, keep, [x], ch)
        e.feed(ptr, pitch, [frames], finish=True)
        data, info = e.read()
        e.close()
        check_row(data[0], x, ch, B, info[0], ("blocks", blocks))
        assert info[0]["blocks"] == blocks


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------

def refusals_main(torch, sa, b):
    B, ch = 256, 2
    x = mdl.crafted("sine", 3 * B, ch)
    keep = []
    ptr, pitch = stage(torch, keep, [x, x], ch)
    e = b.create_flac(2, ch, B)

    def refused(fn, *args, **kw):
        try:
            fn(*args, **kw)
        except RuntimeError as err:
            assert "bad argument" in str(err), (args, err)
        else:
            raise AssertionError(("not refused", args, kw))

    host = np.zeros(4096, np.int16)
    hp = (host.ctypes.data + 15) & ~15
    for args in ((ptr + 2, pitch, [8, 8]), (ptr, pitch + 4, [8, 8]), (hp, 4096, [8, 8]), (0, pitch, [8, 8]), (ptr, 512, [3 * B, 8]),
                 (ptr, 1 << 34, [8, 8])):
        refused(e.feed, *args)
    assert e.unread() == ([0, 0], [mdl.info(0, [])] * 2)  # the refused feeds have changed nothing
    e.feed(ptr, pitch, [3 * B, B + 5])
    need, _ = e.unread()
    want = [mdl.encode_stream(x, ch, B)[0], mdl.encode_stream(x[:B * ch], ch, B)[0]]
    assert need == [len(w) for w in want]
    # a short cap: nothing consumed, nothing written (Flac.read holds the buffers against its fill pattern)
    for caps in ([need[0] - 1, need[1]], [need[0], need[1] - 1], [0, 0]):
        refused(e.read, caps=caps)
        assert e.unread()[0] == need
    data, _ = e.read()
    assert data == want and e.unread()[0] == [0, 0]
    # a finish closes the rows: a later feed is refused until a read with reset
    e.feed(ptr, pitch, [0, 0], finish=True)
    data, info = e.read()
    assert data[0] == b"" and data[1] == mdl.encode_stream(x[:(B + 5) * ch], ch, B)[0][len(want[1]):]
    refused(e.feed, ptr, pitch, [B, B])
    refused(e.feed, ptr, pitch, [0, 0], finish=True)
    assert e.read()[1] == info
    e.read(reset=True)
    e.feed(ptr, pitch, [B, 0], finish=True)
    data, info = e.read()
    assert data == [mdl.encode_stream(x[:B * ch], ch, B)[0], b""] and info[1] == mdl.info(0, []) and info[0]["blocks"] == 1
    e.close()
    # the 1 GiB rule with a small crafted limit: a feed counts with its worst case until a read has fetched the sizes
    bound = 15 + ch * (1 + 2 * B)
    os.environ["SAU_AMD_FLAC_UNREAD_MAX"] = str(4 * bound + 100)
    try:
        e = b.create_flac(2, ch, B)
    finally:
        del os.environ["SAU_AMD_FLAC_UNREAD_MAX"]
    refused(e.feed, ptr, pitch, [3 * B, 2 * B])  # five blocks at their bound
    assert e.unread()[0] == [0, 0]
    e.feed(ptr, pitch, [3 * B, B])  # four
    refused(e.feed, ptr, pitch, [B, 0])
    sizes = e.unread()[0]  # now the sizes are known: far below the bound, and the feed goes through
    assert 0 < sum(sizes) < bound
    e.feed(ptr, pitch, [B, 0])
    refused(e.feed, ptr, pitch, [3 * B, 0])
    data, _ = e.read()
    assert data[0] == mdl.encode_stream(np.concatenate([x, x[:B * ch]]), ch, B)[0] and data[1] == want[1]
    e.feed(ptr, pitch, [3 * B, B])  # read: room again
    e.close()


SECTIONS = [("bytes", bytes_main), ("feeds", feeds_main), ("numbers", numbers_main), ("refusals", refusals_main)]


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
            print("flac %s FAILED\n%s" % (name, traceback.format_exc()))
            break
        print("flac %s ok" % name)
    b.close()


TORCH = r"""
import sys
import torch  # (before the library: torch's wheel brings a HIP runtime of its own, and a process has room for one -- api.Batch.device_tensor)
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_flac
test_gpu_flac.torch_main()
"""


@pytest.fixture(scope="module")
def torch_run():
    """The tests on rows of device memory of the test's own (torch tensors) share one process: torch has to be imported before
    the library is loaded, in this one the library is loaded already, and one import serves them all."""
    return subprocess.run([sys.executable, "-c", TORCH, ROOT], capture_output=True, text=True, timeout=600)


def _section(run, name):
    assert "flac %s ok" % name in run.stdout, (run.returncode, run.stdout[-4000:], run.stderr[-4000:])


def test_crafted_rows(torch_run):
    """3 rows x mono and stereo x B in 256, 1024, 4096, 3 B + 37 frames each, the rows' contents rotating through silence,
    full-scale noise, centre, L only, anti-phase, unrelated channels, a sine, the extremes, bursts and steps; the pitch larger
    than the rows with a pattern between them: the bytes equal the model's byte for byte, the model's decoder returns the input,
    the records equal what the model counts, and two identical calls give identical bytes."""
    _section(torch_run, "bytes")


def test_feeds(torch_run):
    """four rows of unequal length, one empty, cut into feeds of 1, B - 1, B + 1, 2 B frames and the rest, some rows given
    nothing in some feeds, with reads in between: the same bytes as in one piece and as the model's."""
    _section(torch_run, "feeds")


def test_frame_numbers_of_two_and_three_bytes(torch_run):
    """130 and 2050 blocks of 256 frames, silence but for the blocks around the numbers whose coding grows"""
    _section(torch_run, "numbers")


def test_refusals(torch_run):
    """bad rows and pitches, a short cap (nothing consumed or written), a feed after a finish, and the rule on unread output
    with a small limit in place of 1 GiB"""
    _section(torch_run, "refusals")
    assert torch_run.returncode == 0, (torch_run.stdout[-2000:], torch_run.stderr[-4000:])


# ---- 5. render_file_flac ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("channels", [1, 2])
def test_render_file_flac_holds_what_render_file_writes(sa, tmp_path, channels):
    prg = load_program(sa, "devtests__voice-reuse")
    raw, flac = str(tmp_path / "x.raw"), str(tmp_path / "x.flac")
    n = sa.render_file(prg, 8000, raw, sa.api.SNDFILE_RAW, channels)
    frames, info = sa.render_file_flac(prg, 8000, flac, channels, 1024)
    want = np.fromfile(raw, "<i2")
    data = open(flac, "rb").read()
    assert frames == n == info.frames and len(want) == n * channels and np.abs(want.astype(int)).max() > 1000
    h, x = mdl.decode_file(data)
    assert (h["srate"], h["channels"], h["max_block"]) == (8000, channels, 1024)
    assert (x == want).all()
    assert data[:42] == sa.flac_header(8000, channels, 1024, info)
    d = info.as_dict()
    assert d["blocks"] == (n + 1023) // 1024 and d["bytes"] == len(data) - 42 and d["min_frame_bytes"] <= d["max_frame_bytes"]
    assert len(data) < os.path.getsize(raw)
    print("FLAC / RAW: %d / %d = %.3f" % (len(data), os.path.getsize(raw), len(data) / os.path.getsize(raw)))
