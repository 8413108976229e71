"""The MD5 of the unencoded samples, kept on the device by the FLAC encoder (include/saugns_amd.h, section "FLAC", paragraph
"MD5": sauAmd_Flac_set_md5, sauAmd_Flac_md5, sauAmd_set_flac_file_md5; kernels: saugns_amd/csrc/k_md5.h).

The oracle is hashlib.md5 over the samples packed by numpy -- '<i2', or at 24 bits the low three bytes of '<i4' -- of what the
analysis sees: the fed int16 samples, or sauAmd_flac_quantize of the fed floats. With MD5 on an encoder's bytes are those of an
encoder with it off, and a sequence cut into feeds of any lengths has the digest of the sequence in one piece."""
import hashlib
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
POISON = 0.7071  # what lies between the rows: it would show in the digests
EMPTY = "d41d8cd98f00b204e9800998ecf8427e"


def stage(torch, keep, rows, extra=24):
    """rows: float32 arrays (interleaved) -> device rows at a pitch larger than the longest, POISON between and behind them
    -> (the first row's address, the pitch in bytes)"""
    width = (max(max(len(r) for r in rows), 8) + 3) // 4 * 4 + extra  # floats; a multiple of 4: 16 bytes
    t = torch.full((len(rows), width), POISON, dtype=torch.float32, device="cuda")
    for r, x in enumerate(rows):
        if len(x):
            t[r, :len(x)] = torch.from_numpy(np.ascontiguousarray(x)).to("cuda")
    torch.cuda.synchronize()
    keep.append(t)  # (alive until the encoder has been read: the feed is asynchronous)
    assert t.data_ptr() % 16 == 0
    return t.data_ptr(), width * 4


def stage16(torch, keep, rows, extra=24):
    width = (max(max(len(r) for r in rows), 8) + 7) // 8 * 8 + extra
    t = torch.full((len(rows), width), 0x5a5b, dtype=torch.int16, device="cuda")
    for r, x in enumerate(rows):
        if len(x):
            t[r, :len(x)] = torch.from_numpy(np.ascontiguousarray(x)).to("cuda")
    torch.cuda.synchronize()
    keep.append(t)
    return t.data_ptr(), width * 2


def packed(q, bits):
    q = np.asarray(q)
    if bits == 16:
        return q.astype("<i2").tobytes()
    return np.ascontiguousarray(q.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3]).tobytes()


def material(kind, frames, ch, seed):
    """a row of noise with the extremes sown in: int16 samples, or floats with values out of range and NaNs"""
    rng = np.random.default_rng(seed)
    n = frames * ch
    if kind == "int16":
        x = rng.integers(-32768, 32768, n).astype(np.int16)
        for at, v in ((0, -32768), (n - 1, 32767), (n // 2, -1), (n // 3, 0)):
            if 0 <= at < n:
                x[at] = v
        return x
    x = (rng.standard_normal(n) * 0.4).astype(np.float32)
    for at, v in ((0, -1.0), (n - 1, 1.0), (3, np.nan), (n // 2, 1.5), (n // 2 + 1, -7.0), (n // 3, 0.0), (n - 2, 1.0000001)):
        if 0 <= at < n:
            x[at] = v
    return x


class Kind:
    """how a configuration is fed: int16 rows to an int16-fed encoder, or float rows to a float-fed one of `bits`"""

    def __init__(self, sa, torch, B, ch, bits, fed, M):
        self.sa, self.torch, self.B, self.ch, self.bits, self.fed, self.M = sa, torch, B, ch, bits, fed, M

    def create(self, b, n_rows):
        if self.fed == "int16":
            return b.create_flac(n_rows, self.ch, self.B, max_lpc_order=self.M)
        return b.create_flac_f32(n_rows, self.ch, self.B, bits=self.bits, max_lpc_order=self.M)

    def feed(self, e, keep, rows, frames, gains, finish):
        if self.fed == "int16":
            ptr, pitch = stage16(self.torch, keep, rows)
            e.feed(ptr, pitch, frames, finish=finish)
        else:
            ptr, pitch = stage(self.torch, keep, rows)
            e.feed_f32(ptr, pitch, frames, gains, finish=finish)

    def want(self, x, gain):
        """hashlib's digest of what the analysis sees of the row x"""
        q = x if self.fed == "int16" else self.sa.flac_quantize(x, gain, self.bits)
        return hashlib.md5(packed(q, self.bits)).digest()


def tails(B, ch, bits):
    """the frame counts t < B that put B + t frames' last message chunk at 54, 55, 56, 62 and 63 bytes mod 64 and at 2 to 6,
    where a frame's size reaches them (a whole block is 0 mod 64)"""
    size = ch * bits // 8
    out = []
    for want in (54, 55, 56, 62, 63, 2, 3, 4, 5, 6):
        t = next((t for t in range(1, 65) if (t * size) % 64 == want), None)
        if t is not None:
            out.append(t)
    assert all(t < B for t in out) and len(out) >= 2
    return out


# (B, channels, bits, fed as, M)
CONFIGS = [(256, 1, 16, "int16", 0), (256, 2, 16, "int16", 0), (256, 1, 24, "f32", 0), (256, 2, 24, "f32", 0),
           (1024, 1, 16, "f32", 8), (4096, 2, 24, "f32", 0)]
ROWS = 70  # more than a wave's lanes: a lane-per-row kernel crosses a wave's edge, a wave-per-row one has 70 workgroups


# ---- 1. one feed with finish of 70 rows of unequal lengths ----------------------------------------------------------------------

def digests_main(torch, sa, b):
    for case, (B, ch, bits, fed, M) in enumerate(CONFIGS):
        k = Kind(sa, torch, B, ch, bits, fed, M)
        base = [0, 1, B - 1, B, B + 1, 2 * B] + [B + t for t in tails(B, ch, bits)]
        lengths = [base[r % len(base)] + (0 if r < len(base) else B * (r // len(base) % 2)) for r in range(ROWS)]
        assert lengths[:6] == [0, 1, B - 1, B, B + 1, 2 * B] and len(lengths) == ROWS
        x = [material(fed, n, ch, 1000 * case + r) for r, n in enumerate(lengths)]
        gains = [(1.0, 0.5, -0.83)[r % 3] for r in range(ROWS)]
        want = [k.want(x[r], gains[r]) for r in range(ROWS)]
        assert want[0].hex() == EMPTY
        keep, got = [], []
        e_on, e_off = k.create(b, ROWS), k.create(b, ROWS)
        e_on.set_md5(True)
        for _ in range(2):
            k.feed(e_on, keep, x, lengths, gains, True)
            d = e_on.md5()
            data, info = e_on.read(reset=True)
            got.append((d, data, info))
        k.feed(e_off, keep, x, lengths, gains, True)
        plain = e_off.read(reset=True)
        e_on.close()
        e_off.close()
        for r in range(ROWS):
            assert got[0][0][r] == want[r], ("B", B, "ch", ch, "bits", bits, fed, "row", r, "frames", lengths[r],
                                             got[0][0][r].hex(), want[r].hex())
        assert got[0] == got[1], ("called twice", B, ch, bits, fed)
        assert (got[0][1], got[0][2]) == plain, ("the bytes with MD5 on are not those with it off", B, ch, bits, fed)
        assert any(len(d) for d in plain[0])
    print("cases:", len(CONFIGS))


# ---- 2. feeds -----------------------------------------------------------------------------------------------------------------

def cuts_main(torch, sa, b):
    for B, ch, bits, fed, M in ((256, 2, 24, "f32", 0), (1024, 1, 16, "int16", 8), (256, 1, 24, "f32", 0), (4096, 2, 16, "f32", 0)):
        k = Kind(sa, torch, B, ch, bits, fed, M)
        lengths = [5 * B + 37, 0, 4 * B, 3 * B + 1]
        gains = [0.9, 1.0, -0.25, 1.75]
        x = [material(fed, n, ch, 10 + r) for r, n in enumerate(lengths)]
        want = [k.want(x[r], gains[r]) for r in range(4)]
        pieces = [1, B - 1, B + 1, 3 * B, 6 * B]
        e = k.create(b, 4)
        e.set_md5(True)
        keep, got, cur = [], [b""] * 4, [0] * 4
        for i, n in enumerate(pieces):
            last = i == len(pieces) - 1
            fr = [0 if (i + r) % 5 == 4 and not last else min(n, lengths[r] - cur[r]) for r in range(4)]
            k.feed(e, keep, [x[r][cur[r] * ch:(cur[r] + fr[r]) * ch] for r in range(4)], fr, gains, last)
            for r in range(4):
                cur[r] += fr[r]
            if i % 2 == 1 or last:  # reads without reset in between
                data, _ = e.read()
                for r in range(4):
                    got[r] += data[r]
        assert cur == lengths
        cut = e.md5()
        assert cut == want, ("cut into feeds", B, ch, bits, fed, [d.hex() for d in cut], [d.hex() for d in want])
        assert cut[1].hex() == EMPTY
        # in one piece, behind a reset: the same digests and bytes
        e.read(reset=True)
        k.feed(e, keep, x, lengths, gains, True)
        assert e.md5() == want, ("one piece", B, ch, bits, fed)
        data, _ = e.read(reset=True)
        assert data == got
        # other data behind the reset has its own digest: the states were cleared
        y = [material(fed, n, ch, 50 + r) for r, n in enumerate(reversed(lengths))]
        k.feed(e, keep, y, lengths[::-1], gains, True)
        assert e.md5() == [k.want(y[r], gains[r]) for r in range(4)], ("behind a reset", B, ch, bits, fed)
        e.close()


# ---- 3. refusals ----------------------------------------------------------------------------------------------------------------

def refusals_main(torch, sa, b):
    B, ch = 256, 2
    k = Kind(sa, torch, B, ch, 16, "int16", 0)
    x = [material("int16", 2 * B + 9, ch, 70 + r) for r in range(2)]
    keep = []

    def refused(fn, *args, **kw):
        try:
            fn(*args, **kw)
        except RuntimeError as err:
            assert "bad argument" in str(err), (args, err)
        else:
            raise AssertionError(("not refused", fn, args, kw))

    e, plain = k.create(b, 2), k.create(b, 2)
    refused(e.md5)  # MD5 is off
    e.set_md5(False)  # (at the start either value is allowed)
    e.set_md5(True)
    refused(e.md5)  # nothing is finished
    first = [r[:(B + 5) * ch] for r in x]
    k.feed(e, keep, first, [B + 5] * 2, None, False)
    refused(e.set_md5, False)  # fed: not at the start
    refused(e.set_md5, True)
    refused(e.md5)  # still not finished
    k.feed(e, keep, [r[(B + 5) * ch:] for r in x], [B + 4] * 2, None, True)
    assert e.md5() == [k.want(r, 1.0) for r in x]  # ... and the refusals have changed nothing
    refused(e.set_md5, False)  # finished, not reset
    k.feed(plain, keep, x, [2 * B + 9] * 2, None, True)
    refused(plain.md5)  # finished, MD5 off
    data, info = e.read(reset=True)
    assert (data, info) == plain.read(reset=True)
    refused(e.md5)  # behind the reset nothing is finished; the setting has outlived it:
    k.feed(e, keep, x, [0, 0], None, True)
    assert [d.hex() for d in e.md5()] == [EMPTY] * 2
    e.read(reset=True)
    e.set_md5(False)
    k.feed(e, keep, x, [B, B], None, True)
    refused(e.md5)
    e.close()
    plain.close()


SECTIONS = [("digests", digests_main), ("cuts", cuts_main), ("refusals", refusals_main)]


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
            print("flac md5 %s FAILED\n%s" % (name, traceback.format_exc()))
            break
        print("flac md5 %s ok" % name)
    b.close()


TORCH = r"""
import sys
import torch  # (before the library: torch's wheel brings a HIP runtime of its own, and a process has room for one -- api.Batch.device_tensor)
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_flac_md5
test_gpu_flac_md5.torch_main()
"""


@pytest.fixture(scope="module")
def torch_run():
    """The tests on rows of device memory of the test's own (torch tensors) share one process: torch has to be imported before
    the library is loaded, in this one the library is loaded already, and one import serves them all."""
    return subprocess.run([sys.executable, "-c", TORCH, ROOT], capture_output=True, text=True, timeout=600)


def _section(run, name):
    assert "flac md5 %s ok" % name in run.stdout, (run.returncode, run.stdout[-4000:], run.stderr[-4000:])


def test_digests_equal_hashlibs(torch_run):
    """70 rows in one feed with finish -- 0, 1, B - 1, B, B + 1, 2 B frames and B + t for every tail t that ends the message at
    54, 55, 56, 62, 63 or 2 to 6 bytes past a chunk where the frame size reaches it, then the same with a block more --, POISON
    between the rows; int16-fed and float-fed, 16 and 24 bits, mono and stereo, B = 256, 1024 (LPC) and 4096: every digest is
    hashlib's of the samples the analysis sees, the bytes are those of an encoder with MD5 off, and two calls agree."""
    _section(torch_run, "digests")


def test_cuts(torch_run):
    """four rows of unequal length, one empty, cut into feeds of 1, B - 1, B + 1, 3 B frames and the rest, some rows given
    nothing in some feeds, reads in between: the digests of the rows in one piece and hashlib's; behind a read with reset other
    data has its own digest."""
    _section(torch_run, "cuts")


def test_refusals(torch_run):
    """md5() with MD5 off and before a finish, set_md5 after a feed and after a finish: each a bad argument that changes nothing"""
    _section(torch_run, "refusals")
    assert torch_run.returncode == 0, (torch_run.stdout[-2000:], torch_run.stderr[-4000:])


# ---- 4. the file writers ------------------------------------------------------------------------------------------------------

RATE = 8000
FILE_KEY = "devtests__voice-reuse"


def _writers(sa):
    spec = sa.dither_preset(sa.DITHER_E5, 4)

    def limited(prg, path, ch):
        # 9 dB up under a ceiling of the true peak as it stands, so that the limiter works (tests/test_gpu_flac24.py)
        _, ld0, _ = sa.render_file_loudness(prg, RATE, path + ".wav", sa.api.SNDFILE_WAV_F32, ch, -23.0, 1.0)
        return sa.render_file_flac_loudness(prg, RATE, path, ch, 1024, bits=24, target_lufs=ld0.integrated + 9.0,
                                            max_true_peak=float(max(ld0.true_peak)), limited=True)

    return {
        "lpc": (16, lambda prg, path, ch: sa.render_file_flac(prg, RATE, path, ch, 1024, max_lpc_order=8)),
        "f32_16": (16, lambda prg, path, ch: sa.render_file_flac_f32(prg, RATE, path, ch, 1024, bits=16, max_lpc_order=8, gain=0.5)),
        "f32_24": (24, lambda prg, path, ch: sa.render_file_flac_f32(prg, RATE, path, ch, 1024, bits=24, gain=0.5)),
        "limited": (24, limited),
        "dithered": (16, lambda prg, path, ch: sa.render_file_flac_dithered(prg, RATE, path, spec, channels=ch, block_frames=1024,
                                                                            max_lpc_order=8, gain=0.5)),
    }


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("writer", ["lpc", "f32_16", "f32_24", "limited", "dithered"])
def test_file_writers_fill_the_md5_field(sa, tmp_path, writer, channels):
    """with sauAmd_set_flac_file_md5 on, a writer's file differs from the one it writes with the switch off in bytes 26 .. 41
    only, and those are hashlib's digest of the samples the file decodes to"""
    bits, render = _writers(sa)[writer]
    prg = load_program(sa, FILE_KEY)
    off, on = str(tmp_path / "off.flac"), str(tmp_path / "on.flac")
    assert sa.set_flac_file_md5(0) == 0
    render(prg, off, channels)
    try:
        assert sa.set_flac_file_md5(1) == 0
        render(prg, on, channels)
    finally:
        assert sa.set_flac_file_md5(0) == 1
    a, c = open(off, "rb").read(), open(on, "rb").read()
    assert len(a) == len(c) > 42 + 1024 and a[26:42] == bytes(16)
    assert c[:26] == a[:26] and c[42:] == a[42:]
    if bits == 24:
        h, x = mdl.decode_file(a)
    else:
        h, x, _ = m16.decode_file(a)
    assert (h["channels"], h["bps"]) == (channels, bits) and len(x) == h["frames"] * channels and np.abs(x).max() > 100
    assert c[26:42] == hashlib.md5(packed(x, bits)).digest(), (writer, channels, c[26:42].hex())
    assert c[26:42] == sa.flac_md5(np.asarray(x).reshape(-1), bits)
