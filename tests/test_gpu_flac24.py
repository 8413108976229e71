"""The float-fed FLAC encoder on the device, 16 and 24 bits (include/saugns_amd.h, section "FLAC", paragraph "24 bits":
sauAmd_Batch_create_flac_f32, sauAmd_Flac_feed_f32, sauAmd_render_file_flac_f32, sauAmd_render_file_flac_loudness; kernels:
saugns_amd/csrc/k_flac.h -- flac_quant_kernel and the wide analysis, writer and carry kernels).

The bytes are a function of the fed floats, the gains and (B, channels, bits, M) only, so what the device delivers is compared
BYTE FOR BYTE with the library's host restatement (sauAmd_flac_quantize, then sauAmd_flac_encode_block_s32 block by block), which
tests/test_flac24_host.py holds against the numpy model and its independent decoder; the decoder reads the device's streams
here too, and a sequence cut into feeds of any lengths is compared with itself in one piece."""
import os
import subprocess
import sys
import traceback

import numpy as np
import pytest

import flac24_model as mdl
import flac_lpc_model as m16
from conftest import load_program

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = 0.7071  # what lies between the rows: it would show in the bytes


def stage(torch, keep, rows, extra=24, lead=0):
    """rows: float32 arrays (interleaved) -> device rows at a pitch larger than the longest, POISON between, behind and (`lead`
    floats) ahead of them -> (the first row's address, the pitch in bytes)"""
    width = lead + (max(max(len(r) for r in rows), 8) + 3) // 4 * 4 + extra  # floats; a multiple of 4: 16 bytes
    t = torch.full((len(rows), width), POISON, dtype=torch.float32, device="cuda")
    for r, x in enumerate(rows):
        if len(x):
            t[r, lead:lead + len(x)] = torch.from_numpy(np.ascontiguousarray(x)).to("cuda")
    torch.cuda.synchronize()
    keep.append(t)  # (alive until the encoder has been read: the feed is asynchronous)
    assert t.data_ptr() % 16 == 0
    return t.data_ptr() + 4 * lead, width * 4


def stage16(torch, keep, rows, extra=24):
    width = (max(max(len(r) for r in rows), 8) + 7) // 8 * 8 + extra
    t = torch.full((len(rows), width), 0x5a5b, dtype=torch.int16, device="cuda")
    for r, x in enumerate(rows):
        if len(x):
            t[r, :len(x)] = torch.from_numpy(np.ascontiguousarray(x)).to("cuda")
    torch.cuda.synchronize()
    keep.append(t)
    return t.data_ptr(), width * 2


def material(B, ch, blocks, tail, seed):
    """a row of `blocks` whole blocks, each of another crafted kind (tests/flac24_model.py: constant, the rails, L = -R at the
    rails, a quiet sine, noise, one loud partition), and `tail` frames of noise, with floats out of range and NaNs sown in"""
    parts = [mdl.crafted_f32(mdl.KINDS[(seed + k) % len(mdl.KINDS)], B, ch, seed=seed + k, B=B) for k in range(blocks)]
    if tail:
        parts.append(mdl.crafted_f32("noise", tail, ch, seed=seed + 99, B=B))
    x = np.concatenate(parts) if parts else np.zeros(0, np.float32)
    for at, v in ((3, np.nan), (B * ch // 2 + 1, 1.5), (B * ch // 2 + 2, -7.0), (B * ch + 5, np.inf), (B * ch + 6, -np.inf),
                  (len(x) - 1, np.nan), (len(x) - 2, 1.0000001)):
        if 0 <= at < len(x):
            x[at] = v
    return x


def host_stream(sa, x, gain, ch, B, bits, M):
    """the host restatement of a whole row -> (the bytes, the frames' sizes, the quantised samples)"""
    q = sa.flac_quantize(x, gain, bits)
    out, sizes = [], []
    for k in range((len(q) // ch + B - 1) // B):
        f = sa.flac_encode_block_s32(q[k * B * ch:(k + 1) * B * ch], ch, B, k, bits=bits, max_lpc_order=M)
        assert f, ("the host refuses block", k)
        out.append(f)
        sizes.append(len(f))
    return b"".join(out), sizes, q


def info_of(frames, sizes):
    return mdl.info(frames, sizes)


def check_row(sa, data, x, gain, ch, B, bits, M, info, what):
    want, sizes, q = host_stream(sa, x, gain, ch, B, bits, M)
    assert len(data) == len(want), (what, len(data), len(want))
    if data != want:
        at = next(i for i in range(len(want)) if data[i] != want[i])
        raise AssertionError((what, "first difference at byte", at, "of", len(want), data[at:at + 8].hex(), want[at:at + 8].hex()))
    got, s2, _ = (mdl if bits == 24 else m16).decode_frames(data, ch, B)
    assert s2 == sizes and (got.astype(np.int64) == q).all(), what
    assert info == info_of(len(x) // ch, sizes), (what, info, info_of(len(x) // ch, sizes))
    assert all(s <= 15 + ch * (1 + (3 if bits == 24 else 2) * B) for s in sizes)


CONFIGS = [(256, 1, 24, 0), (256, 2, 24, 0), (1024, 1, 24, 0), (1024, 2, 24, 0), (4096, 1, 24, 0), (4096, 2, 24, 0),
           (256, 2, 16, 0), (256, 1, 16, 8), (4096, 1, 16, 0), (4096, 2, 16, 8)]
GAINS = [1.0, 0.5, -0.83]


# ---- 1. crafted rows in one feed --------------------------------------------------------------------------------------------

def bytes_main(torch, sa, b):
    for case, (B, ch, bits, M) in enumerate(CONFIGS):
        x = [material(B, ch, 6, 37, case), np.zeros(0, np.float32), material(B, ch, 2, 5, case + 3)]
        frames = [len(r) // ch for r in x]
        keep, out = [], []
        e = b.create_flac_f32(3, ch, B, bits=bits, max_lpc_order=M)
        for _ in range(2):
            ptr, pitch = stage(torch, keep, x, extra=4 * (1 + case % 3))
            e.feed_f32(ptr, pitch, frames, GAINS, finish=True)
            need, info_q = e.unread()
            data, info = e.read(reset=True)
            assert need == [len(d) for d in data] and info_q == info
            out.append(data)
        e.close()
        assert out[0] == out[1], ("called twice", B, ch, bits, M)
        assert out[0][1] == b"" and info[1] == info_of(0, [])
        for r in (0, 2):
            check_row(sa, out[0][r], x[r], GAINS[r], ch, B, bits, M, info[r], ("B", B, "ch", ch, "bits", bits, "M", M, "row", r))
    print("cases:", len(CONFIGS))


# ---- 2. feeds -----------------------------------------------------------------------------------------------------------------

def cuts_main(torch, sa, b):
    for B, ch, bits, M in ((256, 2, 24, 0), (4096, 1, 24, 0), (1024, 2, 16, 8)):
        lengths = [5 * B + 37, 0, 4 * B, 3 * B + 1]
        gains = [0.9, 1.0, -0.25, 1.75]
        x = [material(B, ch, n // B, n % B, 10 + r) for r, n in enumerate(lengths)]
        pieces = [1, B - 1, B + 1, 3 * B, 6 * B]
        e = b.create_flac_f32(4, ch, B, bits=bits, max_lpc_order=M)
        keep, got, cur = [], [b""] * 4, [0] * 4
        for i, n in enumerate(pieces):
            last = i == len(pieces) - 1
            fr = [0 if (i + r) % 5 == 4 and not last else min(n, lengths[r] - cur[r]) for r in range(4)]
            ptr, pitch = stage(torch, keep, [x[r][cur[r] * ch:(cur[r] + fr[r]) * ch] for r in range(4)])
            e.feed_f32(ptr, pitch, fr, gains, finish=last)
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
            check_row(sa, got[r], x[r], gains[r], ch, B, bits, M, info[r], ("cuts", B, ch, bits, r))
        # in one piece, behind a reset: the same bytes
        e.read(reset=True)
        ptr, pitch = stage(torch, keep, x)
        e.feed_f32(ptr, pitch, lengths, gains, finish=True)
        data, info2 = e.read()
        assert data == got and info2 == info, ("one piece", B, ch, bits)
        e.close()


# ---- 3. float-fed 16 bits against the int16-fed encoder; gains NULL -------------------------------------------------------------

def kinds_main(torch, sa, b):
    for B, ch, M in ((256, 2, 0), (1024, 1, 8), (4096, 2, 8)):
        x = [material(B, ch, 3, 11, 20 + r) for r in range(2)]
        frames = [len(r) // ch for r in x]
        gains = [0.7, -1.0]
        keep = []
        ef = b.create_flac_f32(2, ch, B, bits=16, max_lpc_order=M)
        ptr, pitch = stage(torch, keep, x)
        ef.feed_f32(ptr, pitch, frames, gains, finish=True)
        fdata, finfo = ef.read()
        ef.close()
        ei = b.create_flac(2, ch, B, max_lpc_order=M)
        q = [sa.flac_quantize(x[r], gains[r], 16).astype(np.int16) for r in range(2)]
        ptr, pitch = stage16(torch, keep, q)
        ei.feed(ptr, pitch, frames, finish=True)
        idata, iinfo = ei.read()
        ei.close()
        assert fdata == idata and finfo == iinfo, ("float-fed 16 bits", B, ch, M)
    # gains NULL is 1.0 everywhere
    B, ch = 256, 2
    x = [material(B, ch, 2, 9, 31)]
    keep = []
    e = b.create_flac_f32(1, ch, B, bits=24)
    ptr, pitch = stage(torch, keep, x)
    e.feed_f32(ptr, pitch, [len(x[0]) // ch], None, finish=True)
    data, info = e.read()
    e.close()
    check_row(sa, data[0], x[0], 1.0, ch, B, 24, 0, info[0], "gains NULL")


# ---- 4. rows that are only float-aligned ----------------------------------------------------------------------------------------

def alignment_main(torch, sa, b):
    for B, ch, bits in ((256, 2, 24), (1024, 1, 24), (256, 1, 16)):
        x = [material(B, ch, 3, 37, 40 + r) for r in range(3)]
        x[1] = x[1][:(B + 3) * ch]  # (ends inside a thread's four samples)
        frames = [len(r) // ch for r in x]
        gains = [0.6, 1.0, -0.9]
        got = []
        for lead in (0, 1, 2, 3):
            keep = []
            e = b.create_flac_f32(3, ch, B, bits=bits)
            ptr, pitch = stage(torch, keep, x, lead=lead)
            assert ptr % 16 == 4 * lead
            e.feed_f32(ptr, pitch, frames, gains, finish=True)
            got.append(e.read())
            e.close()
        for lead in (1, 2, 3):
            assert got[lead] == got[0], ("a feed beginning", 4 * lead, "bytes into a row", B, ch, bits)
        for r in range(3):
            check_row(sa, got[0][0][r], x[r], gains[r], ch, B, bits, 0, got[0][1][r], ("aligned", B, ch, bits, r))


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------

def refusals_main(torch, sa, b):
    B, ch = 256, 2
    x = material(B, ch, 3, 0, 50)
    keep = []
    ptr, pitch = stage(torch, keep, [x, x])
    q = sa.flac_quantize(x, 1.0, 16).astype(np.int16)
    ptr16, pitch16 = stage16(torch, keep, [q, q])

    def refused(fn, *args, **kw):
        try:
            fn(*args, **kw)
        except RuntimeError as err:
            assert "bad argument" in str(err), (args, err)
        else:
            raise AssertionError(("not refused", args, kw))

    empty = ([0, 0], [info_of(0, [])] * 2)
    for bits, M in ((24, 1), (24, 8), (20, 0), (0, 0), (16, 9)):
        refused(b.create_flac_f32, 2, ch, B, bits=bits, max_lpc_order=M)
    e = b.create_flac_f32(2, ch, B, bits=24)
    ei = b.create_flac(2, ch, B)
    # cross-kind feeds change nothing
    refused(e.feed, ptr16, pitch16, [8, 8])
    refused(ei.feed_f32, ptr, pitch, [8, 8], [1.0, 1.0])
    assert e.unread() == empty and ei.unread() == empty
    # gains that are not finite; pointers and pitches that are no multiples of 4; host memory; rows beyond their allocation
    for g in ([np.nan, 1.0], [1.0, np.inf], [-np.inf, 1.0]):
        refused(e.feed_f32, ptr, pitch, [8, 8], g)
    host = np.zeros(4096, np.float32)
    for args in ((ptr + 2, pitch, [8, 8]), (ptr + 1, pitch, [8, 8]), (ptr, pitch + 2, [8, 8]), (host.ctypes.data, 4096, [8, 8]),
                 (0, pitch, [8, 8]), (ptr, 512, [3 * B, 8]), (ptr, 1 << 34, [8, 8]), (ptr, pitch, [3 * B + 64, 3 * B + 64])):
        refused(e.feed_f32, *args)
    assert e.unread() == empty
    e.feed_f32(ptr + 4, pitch, [8, 8])  # float alignment is enough
    e.feed_f32(ptr, pitch, [0, 0], finish=True)
    refused(e.feed_f32, ptr, pitch, [B, B])  # closed until a read with reset
    data, _ = e.read(reset=True)
    assert data[0] == data[1] == host_stream(sa, x[1:1 + 8 * ch], 1.0, ch, B, 24, 0)[0]
    e.close()
    ei.close()
    # the 1 GiB rule with a small crafted limit, and the 24-bit bound: four blocks at the 16-bit bound fit, at the 24-bit bound not
    b16, b24 = 15 + ch * (1 + 2 * B), 15 + ch * (1 + 3 * B)
    os.environ["SAU_AMD_FLAC_UNREAD_MAX"] = str(4 * b16 + 100)
    try:
        e24 = b.create_flac_f32(2, ch, B, bits=24)
        e16 = b.create_flac_f32(2, ch, B, bits=16)
    finally:
        del os.environ["SAU_AMD_FLAC_UNREAD_MAX"]
    assert 4 * b16 + 100 < 3 * b24
    refused(e24.feed_f32, ptr, pitch, [3 * B, B])  # four blocks
    refused(e24.feed_f32, ptr, pitch, [3 * B, 0])  # three
    assert e24.unread() == empty
    e16.feed_f32(ptr, pitch, [3 * B, B])  # the 16-bit bound admits the four
    e24.feed_f32(ptr, pitch, [2 * B, 0])  # two blocks at the 24-bit bound fit
    refused(e24.feed_f32, ptr, pitch, [B, 0])  # ... and a third on top of their worst case does not,
    sizes = e24.unread()[0]  # until the sizes are known
    assert 0 < sum(sizes) <= 2 * b24
    data, _ = e24.read()
    assert data[0] == host_stream(sa, x[:2 * B * ch], 1.0, ch, B, 24, 0)[0]
    e24.close()
    e16.close()


SECTIONS = [("bytes", bytes_main), ("cuts", cuts_main), ("kinds", kinds_main), ("alignment", alignment_main), ("refusals", refusals_main)]


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
            print("flac24 %s FAILED\n%s" % (name, traceback.format_exc()))
            break
        print("flac24 %s ok" % name)
    b.close()


TORCH = r"""
import sys
import torch  # (before the library: torch's wheel brings a HIP runtime of its own, and a process has room for one -- api.Batch.device_tensor)
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_flac24
test_gpu_flac24.torch_main()
"""


@pytest.fixture(scope="module")
def torch_run():
    """The tests on rows of device memory of the test's own (torch tensors) share one process: torch has to be imported before
    the library is loaded, in this one the library is loaded already, and one import serves them all."""
    return subprocess.run([sys.executable, "-c", TORCH, ROOT], capture_output=True, text=True, timeout=600)


def _section(run, name):
    assert "flac24 %s ok" % name in run.stdout, (run.returncode, run.stdout[-4000:], run.stderr[-4000:])


def test_device_bytes_equal_the_hosts(torch_run):
    """3 rows per feed -- 6 B + 37 frames, none, 2 B + 5 --, each block another crafted kind, floats out of range and NaNs sown
    in, per-row gains 1, 0.5, -0.83, POISON between the rows; B = 256 (a writer thread's run is one frame), 1024 and 4096 (the LDS
    maximum), mono and stereo at 24 bits, and B = 256 and 4096 at 16 bits with M 0 and 8: the bytes equal the host restatement's,
    the decoder returns sauAmd_flac_quantize of the floats with the row's gain, and two identical calls give identical bytes."""
    _section(torch_run, "bytes")


def test_cuts(torch_run):
    """four rows of unequal length, one empty, distinct gains, cut into feeds of 1, B - 1, B + 1, 3 B frames and the rest, some rows
    given nothing in some feeds, with reads in between: the same bytes as in one piece and as the host's."""
    _section(torch_run, "cuts")


def test_float_fed_16_bits_is_the_int16_encoder(torch_run):
    """the float-fed encoder at 16 bits and the int16-fed one on pcm16 of the same rows: the same bytes and records, M 0 and 8"""
    _section(torch_run, "kinds")


def test_rows_that_are_only_float_aligned(torch_run):
    """a feed beginning 4, 8 and 12 bytes into a 16-byte aligned row gives the bytes of the aligned copy"""
    _section(torch_run, "alignment")


def test_refusals(torch_run):
    """cross-kind feeds, gains that are not finite, misaligned pointers, rows outside an allocation, a feed after a finish, and the
    rule on unread output with the 24-bit bound: a feed the 16-bit bound admits"""
    _section(torch_run, "refusals")
    assert torch_run.returncode == 0, (torch_run.stdout[-2000:], torch_run.stderr[-4000:])


# ---- 6. the file writers ------------------------------------------------------------------------------------------------------

RATE = 8000
FILE_KEY = "devtests__voice-reuse"
WAV_F32, WAV_F32_HEADER = 3, 58


def decode_flac_file(data, bits):
    if bits == 24:
        return mdl.decode_file(data)
    h, x, _ = m16.decode_file(data)
    return h, x.astype(np.int32)


@pytest.mark.parametrize("bits", [16, 24])
@pytest.mark.parametrize("channels", [1, 2])
def test_render_file_flac_f32_holds_the_quantised_floats_of_the_f32_file(sa, tmp_path, channels, bits):
    prg = load_program(sa, FILE_KEY)
    wav, flac = str(tmp_path / "x.wav"), str(tmp_path / "x.flac")
    n = sa.render_file(prg, RATE, wav, WAV_F32, channels)
    M = 8 if bits == 16 and channels == 2 else 0
    frames, info = sa.render_file_flac_f32(prg, RATE, flac, channels, 1024, bits=bits, max_lpc_order=M, gain=0.5)
    x = np.frombuffer(open(wav, "rb").read(), "<f4", offset=WAV_F32_HEADER)
    data = open(flac, "rb").read()
    assert frames == n == info.frames and len(x) == n * channels and np.abs(x).max() > 0.03
    h, got = decode_flac_file(data, bits)
    assert (h["srate"], h["channels"], h["max_block"], h["bps"]) == (RATE, channels, 1024, bits)
    want = sa.flac_quantize(x, 0.5, bits)
    assert (got == want).all() and (want == mdl.quantize(x, 0.5, bits)).all()
    assert data[:42] == sa.flac_header(RATE, channels, 1024, info, bits=bits)
    d = info.as_dict()
    assert d["blocks"] == (n + 1023) // 1024 and d["bytes"] == len(data) - 42 and d["min_frame_bytes"] <= d["max_frame_bytes"]
    print("FLAC %d bits / WAV_F32: %d / %d" % (bits, len(data), os.path.getsize(wav)))


@pytest.mark.parametrize("limited", [False, True])
@pytest.mark.parametrize("channels", [1, 2])
def test_render_file_flac_loudness_holds_the_quantised_floats_of_the_matching_f32_writer(sa, tmp_path, channels, limited):
    prg = load_program(sa, FILE_KEY)
    wav = str(tmp_path / "x.wav")
    # a first look for the program's loudness and true peak: 9 dB up under a ceiling of the true peak as it stands, so the
    # ceiling binds -- it lowers the unlimited writer's gain, and makes the limiter work in the limited one
    _, ld0, _ = sa.render_file_loudness(prg, RATE, wav, WAV_F32, channels, -23.0, 1.0)
    target, ceiling = ld0.integrated + 9.0, float(max(ld0.true_peak))
    if limited:
        n, ld, gain, st = sa.render_file_loudness_limited(prg, RATE, wav, WAV_F32, channels, target, ceiling)
    else:
        n, ld, gain = sa.render_file_loudness(prg, RATE, wav, WAV_F32, channels, target, ceiling)
    x = np.frombuffer(open(wav, "rb").read(), "<f4", offset=WAV_F32_HEADER)
    assert len(x) == n * channels
    for bits in (24, 16):
        flac = str(tmp_path / ("x%d.flac" % bits))
        n2, ld2, gain2, st2, info = sa.render_file_flac_loudness(prg, RATE, flac, channels, 256, bits=bits, target_lufs=target,
                                                                 max_true_peak=ceiling, limited=limited)
        assert n2 == n == info.frames and bytes(ld2) == bytes(ld), (n2, n, info)
        assert np.float32(gain2).view(np.uint32) == np.float32(gain).view(np.uint32), (gain2, gain)
        if limited:
            assert bytes(st2) == bytes(st) and st2.limited > 0
        h, got = decode_flac_file(open(flac, "rb").read(), bits)
        assert (h["frames"], h["channels"], h["bps"]) == (n, channels, bits)
        want = sa.flac_quantize(x, 1.0, bits)
        assert (got == want).all(), (bits, int(np.argmax(got != want)), len(want))
        if limited and bits == 24:
            assert np.abs(got).max() <= int(sa.flac_quantize(np.array([ceiling], np.float32), 1.0, 24)[0])
