"""Float32 sample output (include/saugns_amd.h: sauAmd_Batch_run_f32, sauAmd_Batch_device_pcm_f32, SAU_AMD_SNDFILE_WAV_F32): the mixers
store their f32 accumulator as it stands -- no clamp, no rounding to 15 bits -- in the reference's order and association.

Here the float samples are checked through the oracle's int16 output without a tolerance (tests/test_gpu_f32_oracle.py compares
them with the oracle's float output bit for bit; this is a second, independent route): amp_scale = 0.5 * ampmult /
vo_count multiplies every voice sample BEFORE the ordered sum, so scaling ampmult by 2^k scales every intermediate of the mix
exactly, and for every frame

    quantise(x * 2^k) == oracle PCM rendered with ampmult * 2^k

where x is the device's float output at ampmult and quantise is pcm16() of sau_dev_math.h restated in float32 (NaN -> -1, clip to
+-1, rint(x * 32767), half to even). k = 0 is plain parity; k = 4 and k = 8 pin the float samples at 1/16 and 1/256 of an int16
step; k = 8 also reaches the clamp (0.27 % of the stereo samples, all at +32767 in these 3000 frames)."""
import functools
import re
import struct

import numpy as np
import pytest

from conftest import ORACLE_FORMS, load_program
from saugns_amd import voicebank as vb
from saugns_amd.api import POP_PMOD

pytestmark = pytest.mark.gpu

RATE = 44100


def quantise(x, k=0):
    """pcm16(x * 2^k), all of it in float32"""
    x = np.asarray(x, np.float32) * np.float32(2.0 ** k)
    x = np.where(np.isnan(x), np.float32(-1.0), x)
    x = np.clip(x, np.float32(-1.0), np.float32(1.0)).astype(np.float32)
    return np.rint(x * np.float32(32767.0)).astype(np.int16)


def _same(got, want, what):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert len(got) == len(want), (what, len(got), len(want))
    d = np.flatnonzero(got != want)
    assert len(d) == 0, f"{what}: {len(d)} samples differ, first at {d[0]}: got {got[d[0]:d[0] + 4].tolist()} want {want[d[0]:d[0] + 4].tolist()}"


def _padded(want, k, run_len, ch):
    """run k of the oracle's PCM: the frames it has, zeros behind them"""
    exp = np.zeros(run_len * ch, np.int16)
    part = want[k * run_len * ch:(k + 1) * run_len * ch]
    exp[:len(part)] = part
    return exp


def _render_f32(batch, chunk, stereo):
    """every stream to its end in float runs of `chunk` frames -> list of float32 arrays"""
    ch = 2 if stereo else 1
    outs, alive = [[] for _ in range(batch.n)], [True] * batch.n
    while any(alive):
        pcm, more, lens = batch.run_f32(chunk, stereo)
        for i in range(batch.n):
            if alive[i]:
                outs[i].append(pcm[i, :lens[i] * ch].copy())
                alive[i] = more[i]
    return [np.concatenate(o) for o in outs]


@pytest.fixture(autouse=True)
def forms(oracle):
    oracle.oracle().ora_set_fastmath_forms(ORACLE_FORMS)


# ---- 1. the many-voice mixer ---------------------------------------------------------------------------------------------

BANK_FRAMES = 3000  # (not a multiple of 256)
BANK_AMP = 2.0 ** -6


def _bank300(ampmult):
    """300 rows: one full tile of 256 voices + 44 (a batch of 32 loads and a remainder of 12), pans of their own"""
    voices = vb.config3_voices(300, 1)
    for i, v in enumerate(voices):
        v.pan = vb.Line(vb._num(".2f", ((i * 37) % 100) / 100.0))
    return vb.build_program(voices, ampmult=ampmult)


@functools.lru_cache(maxsize=None)
def _bank300_oracle(k, stereo):
    from oracle import pyoracle as po
    prg = _bank300(BANK_AMP * 2.0 ** k)  # (kept alive through the render)
    want = po.oracle_render(prg.ptr, RATE, stereo, chunk=BANK_FRAMES, max_frames=BANK_FRAMES)
    want.setflags(write=False)
    return want


@pytest.mark.parametrize("stereo", [False, True])
def test_many_voice_mixer_at_three_scales(sa, oracle, stereo):
    """mix_kernel's float form, constant-pan fast path: peak 280 of 32767 at k = 0, 4478 at k = 4 (nothing clamped), and at
    k = 8 a quarter of a percent of the samples clamp"""
    b = sa.Batch([_bank300(BANK_AMP)], RATE)
    pcm, more, lens = b.run_f32(BANK_FRAMES, stereo)
    b.close()
    assert pcm.dtype == np.float32 and lens == [BANK_FRAMES] and more == [True]
    x = pcm[0]
    assert np.abs(x).max() < 0.01  # (far below full scale: what k = 4 and k = 8 resolve is below one int16 step)
    for k in (0, 4, 8):
        _same(quantise(x, k), _bank300_oracle(k, stereo), ("k", k))
    clamped = np.abs(_bank300_oracle(8, stereo).astype(np.int32)) == 32767
    assert 0 < clamped.mean() < 0.02


# ---- 2. no mixing inside the rendering launch ----------------------------------------------------------------------------

INMIX = re.compile(r"inmix: voices (\d+) frames (\d+) chunks (\d+) x (\d+) frames, tiles (\d+) of (\d+)")


def test_a_float_run_leaves_the_mixing_to_the_mixer(sa, oracle, capfd, monkeypatch):
    """test_gpu_inmix.py's bank: the int16 run has tiles mixed by the closed-form launch (the control), the float run of a fresh
    batch has none -- mix_kernel writes every frame -- and quantises to the oracle's PCM"""
    monkeypatch.setenv("SAU_AMD_FK_GRID", "16")
    monkeypatch.setenv("SAU_AMD_INMIX_REPORT", "1")
    voices = vb.config3_voices(96, 4)
    for i, v in enumerate(voices):
        v.pan = vb.Line(vb._num(".2f", ((i * 37) % 100) / 100.0))
    prg = vb.build_program(voices)
    want = oracle.oracle_render(prg.ptr, RATE, True, chunk=176400)
    b = sa.Batch([prg], RATE)
    got = b.run(176400, stereo=True)[0][0]
    b.close()
    _same(got[:len(want)], want, "int16")
    tiles = [int(m.group(5)) for m in INMIX.finditer(capfd.readouterr().err)]
    assert tiles and max(tiles) > 0, "the control: the int16 run's launch mixed nothing itself"
    b = sa.Batch([prg], RATE)
    x = b.run_f32(176400, stereo=True)[0][0]
    b.close()
    _same(quantise(x)[:len(want)], want, "float")
    assert not INMIX.findall(capfd.readouterr().err)


# ---- 3. short rows and pan rows ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("stereo", [False, True])
def test_short_rows_and_pan_rows(sa, oracle, stereo):
    """mix_kernel's other branch: twelve voices of one stream that end at different frame counts (rows shorter than the
    segment) and of which every third has a pan sweep (per-frame pan rows)"""
    voices = []
    for i in range(12):
        ms = 20 + 5 * i  # 882, 1102, 1323, ... frames
        m = vb.Op("sin", freq=vb.Line(float(1 + i % 3), ratio=True), amp=vb._f32(0.6))
        pan = vb.Line(0.1, goal=0.9, shape="lin") if i % 3 == 0 else vb.Line(vb._num(".2f", ((i * 29) % 100) / 100.0))
        voices.append(vb.Op(("sin", "tri")[i % 2], freq=vb._num(".3f", 170.0 + 7.3 * i), time_ms=ms, pan=pan, mods={POP_PMOD: [m]}))
    assert len({ms * RATE // 1000 for ms in range(20, 80, 5)}) == 12
    prg = vb.build_program(voices)
    want = oracle.oracle_render(prg.ptr, RATE, stereo, chunk=4096)
    b = sa.Batch([prg], RATE)
    x = _render_f32(b, 4096, stereo)[0]
    b.close()
    _same(quantise(x), want, "12 voices")
    assert np.abs(x).max() > 0.01


# ---- 4. few-voice streams ------------------------------------------------------------------------------------------------

def _small_scripts():
    prgs = []
    for k, ms in enumerate((61, 67, 73, 79, 90, 95, 101, 107)):  # (2690, 2954, 3219, ... frames: none a multiple of 4)
        a = vb.Op("sin", freq=vb._num(".3f", 150.0 + 11.0 * k), time_ms=ms, pan=vb.Line(vb._num(".2f", (k * 13 % 100) / 100.0)),
                  mods={POP_PMOD: [vb.Op("sin", freq=vb.Line(2.0, ratio=True), amp=vb._f32(0.5))]})
        c = vb.Op("tri", freq=vb._num(".3f", 310.0 + 5.0 * k), time_ms=ms - 10, pan=vb.Line(0.8, goal=0.2) if k == 5 else None)
        # stream 3: a later event at 10 ms = frame 441 -- not a multiple of 4, so the segment behind it is mix_kernel's
        upd = [(10, 0, a, {"amp": vb.Line(0.5)})] if k == 3 else ()
        prgs.append(vb.build_program([a, c], updates=upd))
    return prgs


@pytest.mark.parametrize("stereo", [False, True])
def test_few_voice_streams(sa, oracle, stereo):
    """mix_few_kernel's float form (eight streams of two voices: four frames per thread, 16-byte stores) with stream lengths that
    are no multiple of 4 (the scalar tail), a row shorter than its stream, a pan row, and a segment that begins at frame 441"""
    ch = 2 if stereo else 1
    prgs = _small_scripts()
    run = 6000
    want = [oracle.oracle_render(p.ptr, RATE, stereo, chunk=run) for p in prgs]
    assert all((len(w) // ch) % 4 for w in want) and len({len(w) for w in want}) == 8
    b = sa.Batch(prgs, RATE)
    pcm, more, lens = b.run_f32(run, stereo)
    b.close()
    assert not any(more)
    for s, w in enumerate(want):
        assert lens[s] * ch == len(w), s
        _same(quantise(pcm[s, :len(w)]), w, ("stream", s))


# ---- 5. formats alternating on one batch ---------------------------------------------------------------------------------

@pytest.mark.parametrize("stereo", [False, True])
def test_formats_alternate_on_one_batch(sa, oracle, monkeypatch, stereo):
    """Runs of 4096 frames -- int16, float, float, int16, float -- on a poisoned batch of two streams: a voice that ends inside
    the second run, then a gap in the script (frames 5997 to 11025 of stream 0: nothing sounds), then a voice that begins inside
    the third run. Each run continues where the last one stopped, whatever its format."""
    monkeypatch.setenv("SAU_AMD_POISON", "1")
    ch = 2 if stereo else 1
    run = 4096
    first = vb.Op("sin", freq=220.0, time_ms=136, pan=vb.Line(0.3))
    later = vb.Op("saw", freq=330.0, time_ms=150, pan=vb.Line(0.7),
                  mods={POP_PMOD: [vb.Op("sin", freq=vb.Line(2.0, ratio=True), amp=vb._f32(0.5))]})
    later.start_ms = 250
    prgs = [vb.build_program([first, later]),
            vb.build_program([vb.Op("sin", freq=140.0, time_ms=500, pan=vb.Line(0.2, goal=0.9))])]
    want = [oracle.oracle_render(p.ptr, RATE, stereo, chunk=run, max_frames=5 * run) for p in prgs]
    b = sa.Batch(prgs, RATE)
    for k, f32 in enumerate((False, True, True, False, True)):
        pcm = (b.run_f32 if f32 else b.run)(run, stereo)[0]
        assert pcm.dtype == (np.float32 if f32 else np.int16)
        for s in range(2):
            _same(quantise(pcm[s]) if f32 else pcm[s], _padded(want[s], k, run, ch), ("run", k, "stream", s))
            assert bool(b.device_pcm_f32(s)) == f32 and bool(b.device_pcm(s)) == (not f32)
        assert b.device_pcm_pitch() == (b.device_pcm_f32(1) or b.device_pcm(1)) - (b.device_pcm_f32(0) or b.device_pcm(0))
        if k == 1:  # stream 0's last voice of the moment ends at frame 5997 = 1901 of this run
            silent = pcm[0][1901 * ch:]
            assert silent.dtype == np.float32 and (silent.view(np.uint32) == 0).all()  # +0.0f, not the poison pattern
        if k == 2:  # ... and the next one begins at frame 11025 = 2833 of this run
            silent = pcm[0][:2833 * ch]
            assert (silent.view(np.uint32) == 0).all() and pcm[0][2833 * ch:].any()
    b.close()


# ---- 6. the device view --------------------------------------------------------------------------------------------------

VIEW = r"""
import sys
import numpy as np
import torch  # (before the library: torch's wheel brings a HIP runtime of its own, and a process has room for one -- api.Batch.device_tensor)
sys.path.insert(0, sys.argv[1])
import saugns_amd as sa
from saugns_amd import voicebank as vb

frames = 5000
prgs = [vb.build_program([vb.Op("sin", freq=200.0 + 50.0 * k, time_ms=300, pan=vb.Line(0.25 * k))]) for k in range(3)]
for stereo in (False, True):
    ch = 2 if stereo else 1
    b = sa.Batch(prgs, 44100)
    host = b.run_f32(frames, stereo, fetch=True)[0]
    b.sync()
    t = b.device_tensor(frames, stereo)
    assert t.dtype == torch.float32 and tuple(t.shape) == (3, frames, ch) and t.is_cuda
    assert t.data_ptr() == b.device_pcm_f32(0)
    assert t.stride(0) * 4 == b.device_pcm_pitch()
    got = t.cpu().numpy().reshape(3, frames * ch)
    assert host.any() and (got.view(np.uint32) == host.view(np.uint32)).all()
    host = b.run(frames, stereo, fetch=True)[0]
    b.sync()
    t = b.device_tensor(frames, stereo)
    assert t.dtype == torch.int16 and tuple(t.shape) == (3, frames, ch) and t.is_cuda
    assert t.data_ptr() == b.device_pcm(0) and t.stride(0) * 2 == b.device_pcm_pitch()
    assert host.any() and (t.cpu().numpy().reshape(3, frames * ch) == host).all()
    del t
    b.close()
print("views ok")
"""


def test_device_tensor_aliases_the_rows():
    """Batch.device_tensor after a float run and after an int16 run, mono and stereo, three streams (the pitch): the tensor's bytes
    are the fetched host array's, its data_ptr() is the first row's address. In a process of its own, which is what this test is
    about: torch has to be imported before the library is loaded, and in this one the library is loaded already."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    run = subprocess.run([sys.executable, "-c", VIEW, root], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "views ok" in run.stdout, run.stderr[-3000:]


# ---- 7. float WAV --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("channels", [1, 2])
def test_float_wav(sa, oracle, tmp_path, channels):
    """WAVE_FORMAT_IEEE_FLOAT: `fmt ` of 18 bytes with cbSize 0, `fact` with the frame count, `data`; sizes patched on close"""
    prg = load_program(sa, "examples__tests__panning")
    want = oracle.oracle_render(prg.ptr, RATE, channels == 2, chunk=256 * RATE // 1000)
    frames = len(want) // channels
    path = str(tmp_path / "f32.wav")
    assert sa.render_file(prg, RATE, path, sa.api.SNDFILE_WAV_F32, channels) == frames
    raw = open(path, "rb").read()
    riff, riff_size, wave = struct.unpack_from("<4sI4s", raw, 0)
    assert (riff, wave) == (b"RIFF", b"WAVE") and riff_size == len(raw) - 8
    cid, size = struct.unpack_from("<4sI", raw, 12)
    assert (cid, size) == (b"fmt ", 18)
    tag, ch, rate, byte_rate, align, bits, cb = struct.unpack_from("<HHIIHHH", raw, 20)
    assert (tag, ch, rate, byte_rate, align, bits, cb) == (3, channels, RATE, RATE * 4 * channels, 4 * channels, 32, 0)
    cid, size, n = struct.unpack_from("<4sII", raw, 38)
    assert (cid, size, n) == (b"fact", 4, frames)
    cid, size = struct.unpack_from("<4sI", raw, 50)
    assert (cid, size) == (b"data", frames * channels * 4) and len(raw) == 58 + size
    _same(quantise(np.frombuffer(raw, "<f4", offset=58)), want, "samples")
