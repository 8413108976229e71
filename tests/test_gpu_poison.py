"""Every render here runs with SAU_AMD_POISON: ahead of every engine run the streams' whole PCM rows are filled with 0x5a5a, and
ahead of every segment the voice and pan rows with 0x3ea5a5a5 (about 0.32; engine.h: Backend::poison_run, hip_backend.hip). PCM
rows and voice rows come back from the process-wide pool uncleared, and since round 6 nothing clears the PCM ahead of a run:
every frame is stored by a mixer or cleared by zero_pcm (engine.cpp: Engine::render_segment). Without the fill, a frame that a
later render leaves unwritten would still hold an earlier render's PCM -- usually the right one. With it, such a frame reads
0x5a5a (or the mix of a poisoned row) and differs from the oracle's, to which every render here is compared bit for bit."""
import ctypes as C
import re

import numpy as np
import pytest

from conftest import ORACLE_FORMS
from saugns_amd import voicebank as vb
from saugns_amd.api import POP_AMOD, POP_FMOD, POP_PMOD, POPT_RASEG

pytestmark = pytest.mark.gpu

POISON = 0x5A5A
RATE = 44100


@pytest.fixture(autouse=True)
def poison(monkeypatch, oracle):
    monkeypatch.setenv("SAU_AMD_POISON", "1")
    oracle.oracle().ora_set_fastmath_forms(ORACLE_FORMS)


def _same(got, want, what):
    got = np.asarray(got).reshape(-1)
    assert len(got) == len(want), (what, len(got), len(want))
    d = np.flatnonzero(got != want)
    assert len(d) == 0, f"{what}: {len(d)} samples differ, first at {d[0]}: got {got[d[0]:d[0] + 4].tolist()} want {want[d[0]:d[0] + 4].tolist()}"


def _pm_voice(i, ms):
    m2 = vb.Op("sin", freq=vb.Line(float(2 + i % 3), ratio=True), amp=vb._f32(0.7))
    m1 = vb.Op(("sin", "tri", "sqr")[i % 3], freq=vb.Line(float(1 + i % 5), ratio=True), amp=vb._num(".2f", 0.5 + (i % 7) * 0.1),
               mods={POP_PMOD: [m2]})
    return vb.Op("sin", freq=vb._num(".4f", 110.0 + i * 0.731), time_ms=ms, pan=vb.Line(vb._num(".2f", ((i * 37) % 100) / 100.0)),
                 mods={POP_PMOD: [m1]})


def _fm_voice(i, ms):
    m2 = vb.Op("sin", freq=vb.Line(float(2 + i % 3), ratio=True), amp=vb._f32(0.7))
    m1 = vb.Op("sin", freq=vb.Line(float(1 + i % 5), ratio=True), amp=vb._num(".1f", 20.0 + (i % 7) * 5.0), mods={POP_PMOD: [m2]})
    return vb.Op(("sin", "saw")[i % 2], freq=vb._num(".4f", 140.0 + i * 1.377), time_ms=ms, mods={POP_FMOD: [m1]})


def _r_voice(i, ms):
    rate = vb.Op("sin", freq=0.7 + 0.1 * (i % 5), amp=3.0)
    r = vb.Op(op_type=POPT_RASEG, ras=(("lin", "cos", "sqe")[i % 3], i % 4, 0), seed=77 + 5 * i, freq=9.0 + i % 6, amp=25.0,
              mods={POP_FMOD: [rate]})
    am = vb.Op("sin", freq=2.0 + i % 3, amp=0.3)
    return vb.Op("sin", freq=200.0 + 3.1 * i, time_ms=ms, mods={POP_FMOD: [r], POP_AMOD: [am]})


def _runs(sa, prgs, run_len, stereo, runs=None):
    """A batch run after run of run_len frames: each run's WHOLE buffers (the frames behind a stream's end included)"""
    b = sa.Batch(prgs, RATE)
    out = []
    while True:
        pcm, more, _ = b.run(run_len, stereo=stereo)
        out.append(np.array(pcm, copy=True))
        if (runs is None and not any(more)) or (runs is not None and len(out) == runs):
            break
    b.close()
    return out


def _expect(want, k, run_len, ch):
    """run k of the oracle's PCM: the frames it has, zeros behind them"""
    exp = np.zeros(run_len * ch, np.int16)
    part = want[k * run_len * ch:(k + 1) * run_len * ch]
    exp[:len(part)] = part
    return exp


def _check_runs(sa, oracle, prgs, run_len, stereo, what=""):
    ch = 2 if stereo else 1
    want = [oracle.oracle_render(p.ptr, RATE, stereo, chunk=run_len) for p in prgs]
    runs = _runs(sa, prgs, run_len, stereo)
    assert len(runs) * run_len * ch >= max(len(w) for w in want)
    for k, pcm in enumerate(runs):
        for s, w in enumerate(want):
            _same(pcm[s], _expect(w, k, run_len, ch), (what, "run", k, "stream", s))


@pytest.mark.parametrize("stereo", [False, True])
def test_the_switch_is_live(sa, oracle, stereo):
    """After a run left on the device, each stream's row holds the oracle's PCM up to the run's length, and the frames behind it
    -- never handed out -- still read 0x5a5a (a row is at least the run rounded up to 64 frames, twice for stereo)."""
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    prgs = [vb.build_program([_pm_voice(3 * k + i, 900 + 150 * k) for i in range(3)]) for k in range(4)]
    frames = 44100 + 17  # (not a multiple of 64: a part of the row's last 64 frames lies behind the run)
    ch = 2 if stereo else 1
    b = sa.Batch(prgs, RATE)
    b.run(frames, stereo=stereo, fetch=False)
    b.sync()
    n = ((frames + 63) // 64 * 64) * 2
    for i, p in enumerate(prgs):
        row = np.zeros(n, np.int16)
        assert hip.hipMemcpy(row.ctypes.data, b.device_pcm(i), row.nbytes, 2) == 0
        want = oracle.oracle_render(p.ptr, RATE, stereo, chunk=frames)
        _same(row[:frames * ch], _expect(want, 0, frames, ch), i)
        assert (row[frames * ch:] == POISON).all(), (i, np.flatnonzero(row[frames * ch:] != POISON)[:4])
    b.close()


@pytest.mark.parametrize("stereo", [False, True])
def test_consecutive_runs_of_one_engine(sa, oracle, stereo):
    """Voices that sound through the first run end inside the second: frames that were sound in run 1 are zero in run 2. Two
    identical streams (one zero_pcm span over two rows), streams that end at other frames (spans of their own), one that ends in
    the first run, and runs after every stream has ended."""
    long_ = vb.build_program([_pm_voice(0, 1700), _pm_voice(1, 900), _fm_voice(2, 1250)])
    prgs = [long_, long_, vb.build_program([_pm_voice(3, 1300), _r_voice(4, 600)]), vb.build_program([_pm_voice(5, 400)]),
            vb.build_program([_pm_voice(6 + k, 1550 + 60 * k) for k in range(3)])]
    run_len = 44100
    ch = 2 if stereo else 1
    want = [oracle.oracle_render(p.ptr, RATE, stereo, chunk=run_len) for p in prgs]
    runs = _runs(sa, prgs, run_len, stereo, runs=3)
    for k, pcm in enumerate(runs):
        for s, w in enumerate(want):
            _same(pcm[s], _expect(w, k, run_len, ch), ("run", k, "stream", s))


@pytest.mark.parametrize("run_len", [11289, 66157])
@pytest.mark.parametrize("stereo", [False, True])
def test_a_batch_of_scripts_with_staggered_ends(sa, oracle, run_len, stereo):
    """Ten scripts of different lengths whose voices end one after the other, in runs that divide nothing"""
    prgs = []
    for k in range(10):
        ms = 700 + 230 * k
        voices = [_pm_voice(4 * k + i, ms - 90 * i) for i in range(3)]
        voices.append(_fm_voice(k, ms - 333) if k % 2 else _r_voice(k, ms - 50))
        prgs.append(vb.build_program(voices))
    _check_runs(sa, oracle, prgs, run_len, stereo)


INMIX = re.compile(r"inmix: voices (\d+) frames (\d+) chunks (\d+) x (\d+) frames, tiles (\d+) of (\d+)")


@pytest.mark.parametrize("grid", ["16", "24"])
@pytest.mark.parametrize("stereo", [False, True])
def test_banks_the_launch_mixes_itself(sa, oracle, capfd, monkeypatch, grid, stereo):
    """96 closed-form voices of depth 3 at launches of 16 and 24 workgroups, one run of 4 s: the launch mixing tiles itself (what
    ships; SAU_AMD_INMIX_REPORT says that it did), every frame left to mix_kernel (SAU_AMD_NO_INMIX), and the 12-row build in one
    launch (SAU_AMD_NO_INNER). Then the same voices ending at different frames, in runs of 70001 frames."""
    monkeypatch.setenv("SAU_AMD_FK_GRID", grid)
    monkeypatch.setenv("SAU_AMD_INMIX_REPORT", "1")
    voices = vb.config3_voices(96, 4)
    for i, v in enumerate(voices):
        v.pan = vb.Line(vb._num(".2f", ((i * 29) % 100) / 100.0))
    same = vb.build_program(voices)
    for v, i in zip(voices, range(len(voices))):
        v.time_ms = 4000 - 41 * (i % 29)
    staggered = vb.build_program(voices)
    for leg in ("", "SAU_AMD_NO_INMIX", "SAU_AMD_NO_INNER"):
        if leg:
            monkeypatch.setenv(leg, "1")
        _check_runs(sa, oracle, [same], 176400, stereo, leg)
        tiles = [int(m.group(5)) for m in INMIX.finditer(capfd.readouterr().err)]
        if not leg:
            assert tiles and max(tiles) > 0, "the launch mixed nothing itself"
        if leg == "SAU_AMD_NO_INMIX":
            assert not tiles
        _check_runs(sa, oracle, [staggered], 70001, stereo, (leg, "staggered"))
        if leg == "SAU_AMD_NO_INMIX":
            monkeypatch.delenv(leg)


DUO = re.compile(r"\[sau-amd\] duo (\d):")


@pytest.mark.parametrize("tailmix", [False, True])
def test_duo_banks(sa, oracle, capfd, monkeypatch, tailmix):
    """test_gpu_duo.py's shapes: a bank of both kinds in one engine run (mono and stereo), and twelve small scripts in one batch
    (mix_few_kernel), with the look-back launch mixing the streams' tails itself (SAU_AMD_TAILMIX) and without"""
    monkeypatch.setenv("SAU_AMD_DEBUG_DUO", "1")
    if tailmix:
        monkeypatch.setenv("SAU_AMD_TAILMIX", "1")
    voices = []
    for i in range(48):
        voices += [_pm_voice(2 * i, 3000 - 7 * i), _fm_voice(i, 3000) if i % 3 else _r_voice(i, 2900), _pm_voice(2 * i + 1, 3000)]
    prg = vb.build_program(voices)
    for stereo in (False, True):
        _check_runs(sa, oracle, [prg], 132300, stereo, ("bank", stereo))
    assert 1 in [int(m.group(1)) for m in DUO.finditer(capfd.readouterr().err)], "the joint launch did not run"
    monkeypatch.setenv("SAU_AMD_MORE_ROWS", "0")
    monkeypatch.setenv("SAU_AMD_NO_WIDE_TABS", "1")
    prgs = []
    for k in range(12):
        ms = 2000 + 250 * (k % 5)
        v = [_pm_voice(3 * k, ms), _r_voice(k, ms) if k % 2 else _fm_voice(2 * k, ms), _pm_voice(3 * k + 3, ms - 400)]
        if k % 3 == 0:
            v.append(vb.Op("sin", freq=55.0 + k, time_ms=ms, amp=vb.Line(0.8, goal=0.1, shape="exp")))
        prgs.append(vb.build_program(v))
    _check_runs(sa, oracle, prgs, 66150, False, "small scripts")
    if not tailmix:  # (the look-back launch that mixes tails itself runs apart: hip_backend.hip, duo needs !tail_live_)
        assert 1 in [int(m.group(1)) for m in DUO.finditer(capfd.readouterr().err)], "the joint launch did not run"


def test_feedback_chains_in_chunks(sa, oracle, monkeypatch):
    """A config-5-like bank of feedback voices of different lengths, with the segments' chains in three chunks that the mixer
    follows (SAU_AMD_CHAIN_CHUNKS=3), beside an R-feedback voice"""
    monkeypatch.setenv("SAU_AMD_CHAIN_CHUNKS", "3")
    voices = vb.config5_voices(48, 2)
    for i, v in enumerate(voices):
        v.time_ms = 2000 - 53 * (i % 11)
    r = vb.Op(op_type=POPT_RASEG, ras=("cos", 1, 0), seed=91, freq=7.0, amp=30.0)
    voices.append(vb.Op("sin", freq=vb.Line(180.0, goal=260.0, shape="exp"), time_ms=1700, pm_a=0.4, mods={POP_FMOD: [r]}))
    prg = vb.build_program(voices)
    for stereo in (False, True):
        _check_runs(sa, oracle, [prg], 50021, stereo, stereo)


def test_block_loop_voices(sa, oracle, monkeypatch):
    """The block loop (render_kernel): voices whose modulators run out of time inside a segment, and the whole batch with the
    time-parallel path off (SAU_AMD_NO_FAST)"""
    voices = []
    for i in range(24):
        m = vb.Op("sin", freq=vb.Line(float(1 + i % 4), ratio=True), amp=vb._f32(0.6), time_ms=300 + 37 * i)
        voices.append(vb.Op(("sin", "tri")[i % 2], freq=vb._num(".3f", 180.0 + 5.3 * i), time_ms=1500 - 20 * i,
                            pan=vb.Line(vb._num(".2f", ((i * 13) % 100) / 100.0)), mods={POP_PMOD: [m]}))
    prgs = [vb.build_program(voices), vb.build_program([_pm_voice(k, 800 + 90 * k) for k in range(6)])]
    for leg in ("", "SAU_AMD_NO_FAST"):
        if leg:
            monkeypatch.setenv(leg, "1")
        for stereo in (False, True):
            _check_runs(sa, oracle, prgs, 23001, stereo, (leg, stereo))


CALLS = [[(11289, False)] * 3 + [(11289, True)] * 4 + [(5000, False)] * 3 + [(1746, True)],
         [(1746, True), (1746, True), (300, False), (300, False), (300, True), (11289, False), (5000, True)]]


def _render_calls(create, run, destroy, prg, calls):
    """(frames, stereo) call after call, the last one until the script ends -> every call's whole buffer, one after the other
    (the frames behind the script's end included)"""
    g = create(prg, RATE)
    assert g
    n, out, k = C.c_size_t(), [], 0
    while True:
        size, stereo = calls[min(k, len(calls) - 1)]
        k += 1
        buf = np.zeros(size * (2 if stereo else 1), np.int16)
        more = run(g, buf.ctypes.data, size, stereo, C.byref(n))
        out.append(buf.copy())
        if not more:
            break
    destroy(g)
    return np.concatenate(out)


@pytest.mark.parametrize("depth", ["1", "2"])
def test_dropin_generator_with_read_ahead(sa, oracle, monkeypatch, depth):
    """The drop-in generator's read-ahead (its runs' PCM fetched asynchronously, one or two runs ahead) behind a host that
    changes its call size and channel layout in mid-stream (the snapshot rewind)"""
    import saugns_amd.api as api
    monkeypatch.setenv("SAU_AMD_READAHEAD_DEPTH", depth)
    lib, ora = api.lib(), oracle.oracle()
    prgs = [vb.build_program([_pm_voice(k, 1200 + 170 * k) for k in range(5)] + [_fm_voice(1, 900)]), vb.config5(n=5, seconds=2)]
    for k, prg in enumerate(prgs):
        for calls in CALLS:
            want = _render_calls(ora.ora_create, ora.ora_run, ora.ora_destroy, prg.ptr, calls)
            got = _render_calls(lib.sau_create_Generator, lib.sauGenerator_run, lib.sau_destroy_Generator, prg.ptr, calls)
            _same(got, want, (k, calls[:3]))


@pytest.mark.parametrize("channels", [1, 2])
def test_files(sa, oracle, monkeypatch, tmp_path, channels):
    """sauAmd_render_file, AU (byte-swapped PCM) and WAV, over a bank the launch mixes itself: byte for byte the restated writer's
    over the oracle's PCM"""
    monkeypatch.setenv("SAU_AMD_FK_GRID", "16")
    voices = vb.config3_voices(96, 3)
    for i, v in enumerate(voices):
        v.time_ms = 3000 - 29 * (i % 17)
        v.pan = vb.Line(vb._num(".2f", ((i * 29) % 100) / 100.0))
    prg = vb.build_program(voices)
    pcm = oracle.oracle_render(prg.ptr, RATE, channels == 2)
    for fmt, name in ((sa.api.SNDFILE_AU, "au"), (sa.api.SNDFILE_WAV, "wav")):
        path = str(tmp_path / f"bank.{name}")
        assert sa.render_file(prg, RATE, path, fmt, channels) == len(pcm) // channels
        assert open(path, "rb").read() == oracle.oracle_sndfile_bytes(fmt, channels, RATE, pcm), name
