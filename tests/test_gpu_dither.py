"""The 16-bit quantiser stage on the device (include/saugns_amd.h, section "Dither and noise shaping": sauAmd_Batch_create_quantizer,
sauAmd_Quantizer_feed / _rows / _read / _stats, sauAmd_render_file_dithered, _flac_dithered, _loudness_dithered; kernels:
saugns_amd/csrc/k_dither.h -- dither_flat_kernel and dither_shape_kernel).

The samples are a function of the fed floats, the gains, the spec and the position in the stream only, so what the device
delivers is compared SAMPLE FOR SAMPLE with the library's host restatement (sauAmd_dither_quantize), which
tests/test_dither_host.py holds against the independent model; a sequence cut into feeds of any lengths is compared with itself
in one piece, and the rows go on into the FLAC encoder and the file writers."""
import os
import subprocess
import sys
import tempfile
import traceback

import numpy as np
import pytest

import dither_model as dm
import flac_lpc_model as m16
from conftest import load_program

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = 0.7071  # what lies between the rows: it would show in the samples
KEY = "devtests__voice-reuse"
TILE = 64        # frames of dither_shape_kernel's tile
GAINS = [1.0, 0.5, -0.83]
# a row of no frames, one, around a wave's 64 lanes and the shaped kernel's tile, three tiles + 17, and around the flat kernel's
# run of 1024 samples per block, mono and stereo
LENGTHS = [0, 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 17, 511, 513, 1023, 1025, 2 * 1024 + 52]


def stage(torch, keep, rows, extra=24, lead=0):
    """rows: float32 arrays (interleaved) -> device rows at a pitch larger than the longest, POISON between, behind and (`lead`
    floats) ahead of them -> (the first row's address, the pitch in bytes)"""
    width = lead + (max(max(len(r) for r in rows), 8) + 3) // 4 * 4 + extra  # floats; a multiple of 4: 16 bytes
    t = torch.full((len(rows), width), POISON, dtype=torch.float32, device="cuda")
    for r, x in enumerate(rows):
        if len(x):
            t[r, lead:lead + len(x)] = torch.from_numpy(np.ascontiguousarray(x)).to("cuda")
    torch.cuda.synchronize()
    keep.append(t)  # (alive until the quantiser has been read: the feed is asynchronous)
    assert t.data_ptr() % 16 == 0
    return t.data_ptr() + 4 * lead, width * 4


def material(n, ch, seed):
    """n frames of noise at one of three levels, with NaN, infinities, full scale and floats out of range sown in"""
    rng = np.random.default_rng(1000 + seed)
    x = (rng.standard_normal(n * ch) * [1e-4, 0.02, 0.6][seed % 3]).astype(np.float32)
    for k, v in enumerate((np.nan, np.inf, -np.inf, 1.5, -7.0, 1.0, -1.0, 1.0000001)):
        if len(x) > 8:
            x[(seed * 7 + k * 13) % len(x)] = v
    return x


def specs(sa):
    """none, FLAT, HP1, E5, F9, with dither on and off"""
    out = [("none", sa.Dither(seed=9))]
    for name in ("FLAT", "HP1", "E5", "F9"):
        shape, coef = dm.PRESETS[name]
        out.append((name, sa.dither_preset(shape, 0x0123456789ABCDEF + shape)))
        if coef:
            out.append((name + " without dither", sa.Dither(seed=3, dither=0, coef=coef)))
    return out


def restated(sa, x, ch, gain, spec, row, first=0, history=None):
    return sa.dither_quantize(x, ch, gain, spec, row=row, first_frame=first, history=history)


def expect(sa, rows, ch, gains, spec):
    """the restatement of whole rows from the stream's start -> (samples per row, stats per row)"""
    out, st = [], []
    for r, x in enumerate(rows):
        q, _, cl = restated(sa, x, ch, gains[r], spec, r)
        out.append(q)
        st.append({"frames": len(x) // ch, "clipped": cl})
    return out, st


# ---- 1. against the restatement, and fed twice ---------------------------------------------------------------------------------

def restatement_main(torch, sa, b):
    case = 0
    for n_rows in (1, 3, 33):  # 33 stereo rows are 66 chains: more than one wave's lanes
        for ch in (1, 2):
            for name, spec in specs(sa):
                lengths = [LENGTHS[(case + 3 * r) % len(LENGTHS)] for r in range(n_rows)]
                if n_rows == 1:
                    lengths = [LENGTHS[1 + case % (len(LENGTHS) - 1)]]
                rows = [material(n, ch, case + r) for r, n in enumerate(lengths)]
                gains = [GAINS[(case + r) % 3] for r in range(n_rows)]
                want, want_st = expect(sa, rows, ch, gains, spec)
                q = b.create_quantizer(n_rows, ch, spec)
                keep, outs = [], []
                for again in range(2):
                    lead = (case + again) % 2  # a row start one float past a 16-byte boundary
                    ptr, pitch = stage(torch, keep, rows, extra=4 * (1 + case % 3), lead=lead)
                    assert ptr % 16 == 4 * lead
                    q.feed(ptr, pitch, lengths, gains)
                    assert q.rows() % 16 == 0 and q.pitch() % 256 == 0 and q.pitch() >= max(lengths) * ch * 2
                    got = q.read()
                    st = q.stats(reset=True)
                    for r in range(n_rows):
                        assert np.array_equal(got[r], want[r]), (name, "rows", n_rows, "ch", ch, "row", r, "frames", lengths[r], "feed", again)
                    assert st == want_st, (name, n_rows, ch, st, want_st)
                    outs.append(got)
                assert all(np.array_equal(a, c) for a, c in zip(*outs)), ("fed twice", name, n_rows, ch)
                q.close()
                case += 1
    # gains NULL is 1.0 everywhere
    spec = sa.dither_preset(sa.DITHER_E5, 4)
    rows = [material(130, 2, 77)]
    q = b.create_quantizer(1, 2, spec)
    keep = []
    ptr, pitch = stage(torch, keep, rows)
    q.feed(ptr, pitch, [130], None)
    assert np.array_equal(q.read()[0], restated(sa, rows[0], 2, 1.0, spec, 0)[0])
    q.close()
    print("cases:", case)


# ---- 2. cut independence -------------------------------------------------------------------------------------------------------

def cuts_main(torch, sa, b):
    lengths = [5 * TILE + 9, 3 * TILE + 17, 2 * TILE + 1]
    extra = 40
    for ch, spec in ((2, sa.dither_preset(sa.DITHER_F9, 21)), (1, sa.dither_preset(sa.DITHER_E5, 22)),
                     (2, sa.dither_preset(sa.DITHER_FLAT, 23)), (1, sa.Dither(seed=1, dither=0, coef=[1.0]))):
        rows = [material(n + extra, ch, 200 + r) for r, n in enumerate(lengths)]
        gains = [0.9, -0.25, 1.75]
        runs = []
        for pieces in ((1, TILE - 1, TILE, TILE + 1, 1 << 20), (TILE - 1, 2, 1 << 20), (1 << 20,)):
            q = b.create_quantizer(3, ch, spec)
            keep, got, cur = [], [[] for _ in range(3)], [0] * 3
            for n in pieces:
                fr = [min(n, lengths[r] - cur[r]) for r in range(3)]
                ptr, pitch = stage(torch, keep, [rows[r][cur[r] * ch:(cur[r] + fr[r]) * ch] for r in range(3)])
                q.feed(ptr, pitch, fr, gains)
                for r, part in enumerate(q.read()):
                    got[r].append(part)
                    cur[r] += fr[r]
            assert cur == lengths
            st = q.stats()
            # one more feed behind the cuts: history, counts and positions have all been carried
            ptr, pitch = stage(torch, keep, [rows[r][lengths[r] * ch:] for r in range(3)])
            q.feed(ptr, pitch, [extra] * 3, gains)
            last = q.read()
            runs.append(([np.concatenate(g) for g in got], st, last, q.stats()))
            q.close()
        want, want_st = expect(sa, rows, ch, gains, spec)
        for k, (got, st, last, st2) in enumerate(runs):
            for r in range(3):
                assert np.array_equal(got[r], want[r][:lengths[r] * ch]), ("cut", k, "ch", ch, "row", r)
                assert np.array_equal(last[r], want[r][lengths[r] * ch:]), ("the feed behind cut", k, "ch", ch, "row", r)
            assert st2 == want_st, (k, st2, want_st)
            assert st == runs[-1][1], (k, st, runs[-1][1])


# ---- 3. full scale ----------------------------------------------------------------------------------------------------------------

def full_scale_main(torch, sa, b):
    for ch, name, seed in ((1, "F9", 7), (2, "F9", 7), (2, "FLAT", 5), (1, "FLAT", 5)):
        x = np.ones(2000 * ch, np.float32)
        if ch == 2:
            x[1::2] = -1.0
        want, _, clipped = dm.quantize(x, ch, 1.0, 1, dm.PRESETS[name][1], seed)
        if (ch, name) == (1, "F9"):
            assert clipped == [902, 0]  # (the header's figure)
        assert clipped[0] > 0
        q = b.create_quantizer(1, ch, sa.dither_preset(dm.PRESETS[name][0], seed))
        keep = []
        ptr, pitch = stage(torch, keep, [x])
        q.feed(ptr, pitch, [2000])
        got = q.read()[0]
        assert q.stats() == [{"frames": 2000, "clipped": clipped}], (name, ch, q.stats(), clipped)
        assert np.array_equal(got, want) and got.min() >= -32767 and got.max() == 32767
        q.close()


# ---- 4. into the FLAC encoder ------------------------------------------------------------------------------------------------------

def composition_main(torch, sa, b):
    B = 256
    for ch, spec in ((2, sa.dither_preset(sa.DITHER_F9, 31)), (1, sa.dither_preset(sa.DITHER_FLAT, 32))):
        lengths = [3 * B + 11, B, 2 * B + 100]
        rows = [material(n, ch, 300 + r) * np.float32(0.5) for r, n in enumerate(lengths)]
        want, _ = expect(sa, rows, ch, GAINS, spec)
        q = b.create_quantizer(3, ch, spec)
        e = b.create_flac(3, ch, B, max_lpc_order=8)
        keep = []
        ptr, pitch = stage(torch, keep, rows)
        q.feed(ptr, pitch, lengths, GAINS)
        e.feed(q.rows(), q.pitch(), lengths, finish=True)
        data, info = e.read()
        for r in range(3):
            got, _, _ = m16.decode_frames(data[r], ch, B)
            assert np.array_equal(np.asarray(got, np.int64), want[r].astype(np.int64)), ("composition", ch, r)
            assert info[r]["frames"] == lengths[r]
        e.close()
        q.close()


# ---- 5. the writers ---------------------------------------------------------------------------------------------------------------

HEADER = {"raw": 0, "au": 28, "wav": 44}


def writers_main(torch, sa, b):
    prg = load_program(sa, KEY)
    srate, ch, gain = 8000, 2, 0.37
    fmts = {"raw": sa.SNDFILE_RAW, "au": sa.SNDFILE_AU, "wav": sa.SNDFILE_WAV}
    with tempfile.TemporaryDirectory() as tmp:
        p = lambda name: os.path.join(tmp, name)
        frames = sa.render_file(prg, srate, p("f32.wav"), sa.api.SNDFILE_WAV_F32, ch)
        x = np.frombuffer(open(p("f32.wav"), "rb").read()[58:], "<f4")
        assert len(x) == frames * ch and frames > 0
        for name, spec in (("F9", sa.dither_preset(sa.DITHER_F9, 41)), ("FLAT", sa.dither_preset(sa.DITHER_FLAT, 42)),
                           ("none", sa.Dither(seed=1))):
            want, _, clipped = restated(sa, x, ch, gain, spec, 0)
            if name == "none":
                assert np.array_equal(want.astype(np.int32), sa.flac_quantize(x, gain, 16))
            for ext, fmt in fmts.items():
                assert sa.render_file(prg, srate, p("plain." + ext), fmt, ch) == frames
                n, st = sa.render_file_dithered(prg, srate, p("d." + ext), spec, fmt=fmt, channels=ch, gain=gain)
                assert n == frames and st == {"frames": frames, "clipped": clipped}, (name, ext, n, st)
                plain, got = open(p("plain." + ext), "rb").read(), open(p("d." + ext), "rb").read()
                h = HEADER[ext]
                assert len(got) == len(plain) and got[:h] == plain[:h], (name, ext, "header")
                s = np.frombuffer(got[h:], ">i2" if ext == "au" else "<i2")
                assert np.array_equal(s.astype(np.int16), want), (name, ext, "samples")
            n, info, st = sa.render_file_flac_dithered(prg, srate, p("d.flac"), spec, channels=ch, block_frames=1024, max_lpc_order=8,
                                                       gain=gain)
            data = open(p("d.flac"), "rb").read()
            assert n == frames and info.frames == frames and st == {"frames": frames, "clipped": clipped}
            assert data[:42] == sa.flac_header(srate, ch, 1024, info)
            got, _, _ = m16.decode_frames(data[42:], ch, 1024)
            assert np.array_equal(np.asarray(got, np.int64), want.astype(np.int64)), (name, "flac")
        # the loudness writer: render_file_loudness's gain, the dithered writer's file at that gain
        spec = sa.dither_preset(sa.DITHER_E5, 43)
        n0, ld0, g0 = sa.render_file_loudness(prg, srate, p("l.wav"), sa.SNDFILE_WAV, ch, -30.0, 0.5)
        n1, ld1, g1, st1 = sa.render_file_loudness_dithered(prg, srate, p("ld.wav"), spec, fmt=sa.SNDFILE_WAV, channels=ch,
                                                           target_lufs=-30.0, max_true_peak=0.5)
        assert (n1, g1) == (n0, g0) and bytes(ld1) == bytes(ld0)
        n2, st2 = sa.render_file_dithered(prg, srate, p("d2.wav"), spec, fmt=sa.SNDFILE_WAV, channels=ch, gain=g1)
        assert open(p("ld.wav"), "rb").read() == open(p("d2.wav"), "rb").read() and st1 == st2 and n2 == n1
        assert open(p("ld.wav"), "rb").read() != open(p("l.wav"), "rb").read()  # (dither is in it)


SECTIONS = [("restatement", restatement_main), ("cuts", cuts_main), ("full scale", full_scale_main),
            ("composition", composition_main), ("writers", writers_main)]


def torch_main():
    """(in a process of its own, torch imported first: see the fixture) every section on one batch's device; a section that fails
    ends the process -- nothing more is started on the device behind a failure"""
    import torch
    import saugns_amd as sa
    from saugns_amd import voicebank as vb
    sa.set_piluts(np.fromfile(os.path.join(ROOT, "tests", "golden", "piluts_ref.f32"), dtype="<f4").reshape(12, 2048))
    b = sa.Batch([vb.build_program([vb.Op("sin", freq=200.0, time_ms=10)])], 44100)  # (never run: its device is all that is used)
    for name, fn in SECTIONS:
        try:
            fn(torch, sa, b)
        except Exception:
            print("dither %s FAILED\n%s" % (name, traceback.format_exc()))
            break
        print("dither %s ok" % name)
    b.close()


TORCH = r"""
import sys
import torch  # (before the library: torch's wheel brings a HIP runtime of its own, and a process has room for one -- api.Batch.device_tensor)
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_dither
test_gpu_dither.torch_main()
"""


@pytest.fixture(scope="module")
def torch_run():
    """The tests on rows of device memory of the test's own (torch tensors) share one process: torch has to be imported before
    the library is loaded, in this one the library is loaded already, and one import serves them all."""
    return subprocess.run([sys.executable, "-c", TORCH, ROOT], capture_output=True, text=True, timeout=600)


def _section(run, name):
    assert "dither %s ok" % name in run.stdout, (run.returncode, run.stdout[-4000:], run.stderr[-4000:])


def test_device_equals_the_restatement(torch_run):
    """1, 3 and 33 rows (33 stereo rows are 66 chains: two waves), mono and stereo, rows of 0, 1, 63, 64, 65 frames, three tiles +
    17 and around the flat kernel's 1024 samples, the specs none, FLAT, HP1, E5, F9 with dither on and off, gains 1, 0.5, -0.83,
    every other feed beginning one float past a 16-byte boundary, NaN, infinities and floats out of range sown in, POISON between
    the rows: the samples and the stats equal the host restatement's -- and so do those of the same feed behind a reset."""
    _section(torch_run, "restatement")


def test_cuts(torch_run):
    """three rows cut into feeds of (1, 63, 64, 65, rest), (63, 2, rest) and one piece, shaped and flat, mono and stereo: the
    concatenated samples, the stats and one more feed behind them equal the run in one piece and the restatement."""
    _section(torch_run, "cuts")


def test_full_scale(torch_run):
    """constant full scale, F9 and FLAT: the model's samples and clip counts (902 of 2000 for F9 with seed 7), nothing outside
    -32767 .. 32767."""
    _section(torch_run, "full scale")


def test_rows_go_into_the_flac_encoder(torch_run):
    """the quantiser's device rows fed to an int16-fed encoder at LPC order 8 decode to the restatement's samples"""
    _section(torch_run, "composition")


def test_writers(torch_run):
    """a golden program at 8000 Hz, stereo: the dithered RAW, AU and WAV files have sauAmd_render_file's headers and the
    restatement's samples of the WAV_F32 render times the gain (AU big-endian; spec none: sauAmd_flac_quantize's), the FLAC file
    decodes to them, and the loudness writer has sauAmd_render_file_loudness's gain and the dithered writer's file at that gain."""
    _section(torch_run, "writers")
