"""On-device BS.1770 loudness and true peak, and the loudness-normalised file writer (include/saugns_amd.h: sauAmdLoudness,
sauAmd_Batch_set_loudness, sauAmd_Batch_loudness, sauAmd_Batch_loudness_hops, sauAmd_Batch_measure_loudness_rows,
sauAmd_render_file_loudness; kernels: saugns_amd/csrc/k_loudness.h).

The header fixes the order of every operation, so what the device measures is compared with the Python restatement
(tests/loudness_model.py) fed the same rows in the same run lengths BIT FOR BIT: hop energies, true peak, counts; integrated
and momentary loudness must equal sauAmd_loudness_gate of the same hops, which tests/test_loudness_host.py compares with its
own restatement without a GPU."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import loudness_model as lm
from conftest import ORACLE_FORMS, load_program
from test_loudness_host import CHUNK_ACCURACY

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# launch_plan.h, mirrored (tests/test_loudness_host.py reads the header and fails when the model's copies no longer match
# it): a workgroup of loud_chunk_kernel owns 64 chunks of 256 frames, one of truepeak_kernel 256 frames
LOUD_WG_FRAMES = 64 * lm.LOUD_CHUNK


def bits32(v):
    return int(np.float32(v).view(np.uint32))


def bits64(v):
    return int(np.float64(v).view(np.uint64))


def check_record(sa, got, meter, what):
    """got: api.Loudness; meter: the restatement fed the same frames"""
    hops = meter.hops()
    assert int(got.frames) == meter.pos, (what, "frames", int(got.frames), meter.pos)
    want_tp = meter.true_peak()
    for c in range(2):
        assert bits32(got.true_peak[c]) == bits32(want_tp[c]), (what, "true_peak", c, float(got.true_peak[c]), float(want_tp[c]))
    gated = sa.loudness_gate(hops, meter.hop, meter.ch)
    assert (int(got.blocks), int(got.gated_blocks)) == (int(gated.blocks), int(gated.gated_blocks)), (what, got, gated)
    assert int(got.blocks) == max(len(hops) - 3, 0)
    for k in ("integrated", "momentary_max"):
        assert bits64(getattr(got, k)) == bits64(getattr(gated, k)), (what, k, got, gated)


def check_hops(got, meter, what):
    want = meter.hops()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    d = np.flatnonzero(got.view(np.uint64).reshape(-1) != want.view(np.uint64).reshape(-1))
    assert len(d) == 0, (what, "hop energies", len(d), d[:4], got.reshape(-1)[d[:4]], want.reshape(-1)[d[:4]])


# ---- 1. crafted rows and known signals through measure_loudness_rows ----------------------------------------------------

def crafted_frames(hop):
    n = [1, 31, 32, 33, 255, 256, 257, 511, 513, hop - 1, hop, hop + 1, 4 * hop - 1, 4 * hop, 4 * hop + 1, 10 * hop + 77,
         lm.TP_TILE - 1, lm.TP_TILE + 1, LOUD_WG_FRAMES - 1, LOUD_WG_FRAMES + 1, LOUD_WG_FRAMES + 257]
    return sorted(set(n))


def crafted_values(rng, n_rows, frames, ch, case):
    """seeded noise plus DC, a NaN, a +inf and a -inf planted (and at the row's two ends in turn); the last row zeros"""
    x = (rng.standard_normal((n_rows, frames * ch)) * 0.3 + 0.05).astype(np.float32)
    planted = [np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf), np.float32(-3.0), np.float32(-0.0)]
    for r in range(n_rows):
        at = rng.permutation(frames * ch)[:len(planted)]
        for k, i in enumerate(at):
            x[r, i] = planted[(k + r + case) % len(planted)]
        if frames * ch > 8:
            x[r, -1] = planted[(case + r) % len(planted)]
            x[r, 0] = planted[(case + r + 1) % len(planted)]
    x[n_rows - 1] = 0.0
    return x


def rows_main():
    """(in a process of its own, torch imported first: see test_rows)"""
    import torch
    import saugns_amd as sa
    from saugns_amd import voicebank as vb
    b = sa.Batch([vb.build_program([vb.Op("sin", freq=200.0, time_ms=10)])], 44100)  # (never run: its device is all that is used)
    taps = sa.truepeak_taps()
    rng = np.random.default_rng(20261018)
    cases = 0
    for rate in (8000, 11025):
        hop = rate // 10
        f = sa.loudness_filter(rate)
        for ch in (1, 2):
            for frames in crafted_frames(hop):
                n_rows = 3
                x = crafted_values(rng, n_rows, frames, ch, cases)
                pitch_el = (frames * ch * 4 + 15) // 16 * 4 + 4 * (1 + cases % 3)  # larger than the row
                # what lies between the rows would show in every sum if a kernel read it
                t = torch.full((n_rows, pitch_el), 1e30, dtype=torch.float32, device="cuda")
                t[:, :frames * ch] = torch.from_numpy(x).to("cuda")
                torch.cuda.synchronize()
                got, hops = b.measure_loudness_rows(t.data_ptr(), pitch_el * 4, n_rows, frames, ch, rate)
                again, hops2 = b.measure_loudness_rows(t.data_ptr(), pitch_el * 4, n_rows, frames, ch, rate)
                assert len(got) == n_rows and hops.shape == (n_rows, frames // hop, 2)
                for r in range(n_rows):
                    what = ("rate", rate, "ch", ch, "frames", frames, "row", r)
                    m = lm.Meter(f, taps, hop, ch)
                    m.run(x[r])
                    check_hops(hops[r], m, what)
                    check_record(sa, got[r], m, what)
                    assert bytes(got[r]) == bytes(again[r]) and hops.tobytes() == hops2.tobytes(), (what, "measured twice")
                    if ch == 1:
                        assert got[r].true_peak[1] == 0 and not hops[r][:, 1].any()
                z = got[n_rows - 1]  # the row of zeros
                assert list(z.true_peak) == [0, 0] and z.integrated == -math.inf and z.gated_blocks == 0 and not hops[n_rows - 1].any()
                cases += 1
    # frames == 0: empty records; refusals: a misaligned address, an odd pitch, three channels, a low rate, host memory
    t = torch.zeros((2, 64), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for ld in b.measure_loudness_rows(t.data_ptr(), 256, 2, 0, 2, 8000)[0]:
        assert ld.frames == 0 and ld.blocks == 0 and ld.integrated == -math.inf and list(ld.true_peak) == [0, 0]
    host = np.zeros(1024, np.float32)
    refused = 0
    for args in ((t.view(-1)[1:].data_ptr(), 256, 1, 8, 1, 8000), (t.data_ptr(), 260, 2, 8, 1, 8000), (t.data_ptr(), 256, 2, 8, 3, 8000),
                 (t.data_ptr(), 256, 2, 8, 1, 2559), (t.data_ptr(), 16, 2, 8, 1, 8000), ((host.ctypes.data + 15) & ~15, 256, 2, 8, 1, 8000),
                 (t.data_ptr(), 1 << 20, 60000, 8, 1, 8000)):
        try:
            b.measure_loudness_rows(*args)
        except RuntimeError as e:
            assert "bad argument" in str(e), e
            refused += 1
    assert refused == 7
    # a sine at a quarter of the rate sampled at 45 degrees: every sample is +-0.7071, the signal between them reaches 1
    # (faded in and out over 256 frames: a tone switched on at full level has an overshoot of its own between the samples)
    for rate in (8000, 44100):
        n = rate // 2
        x = np.sin(2.0 * math.pi * np.arange(n) / 4.0 + math.pi / 4.0)
        ramp = 0.5 - 0.5 * np.cos(math.pi * (np.arange(256) + 0.5) / 256.0)
        x[:256] *= ramp
        x[-256:] *= ramp[::-1]
        x = x.astype(np.float32)
        t = torch.from_numpy(np.concatenate([x, np.zeros(-n % 4, np.float32)])).to("cuda")
        torch.cuda.synchronize()
        ld = b.measure_loudness_rows(t.data_ptr(), len(t) * 4, 1, n, 1, rate)[0][0]
        lv = b.measure_rows(t.data_ptr(), len(t) * 4, 1, True, n, 1)[0]
        assert 0.99 <= ld.true_peak[0] <= 1.01, (rate, ld)
        assert abs(lv.peak[0] - 0.70710678) < 1e-6, (rate, lv)
    # stereo 1 kHz at -23 dBFS for 3 s: -23.0 LUFS (EBU Tech 3341, case 1)
    for rate in (8000, 44100):
        n = 3 * rate
        s = (10.0 ** (-23.0 / 20.0) * np.sin(2.0 * math.pi * 1000.0 * np.arange(n) / rate)).astype(np.float32)
        t = torch.from_numpy(np.repeat(s, 2)).to("cuda")
        torch.cuda.synchronize()
        ld = b.measure_loudness_rows(t.data_ptr(), len(t) * 4, 1, n, 2, rate)[0][0]
        assert ld.frames == n and ld.blocks == 27 and ld.gated_blocks == 27
        assert abs(ld.integrated - -23.0) <= 0.1 and abs(ld.momentary_max - -23.0) <= 0.1, (rate, ld)
    b.close()
    print("loudness rows ok:", cases, "cases")


ROWS = r"""
import sys
import torch  # (before the library: torch's wheel brings a HIP runtime of its own, and a process has room for one -- api.Batch.device_tensor)
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_loudness
test_gpu_loudness.rows_main()
"""


def test_rows():
    """measure_loudness_rows on torch tensors, mono and stereo, at 8000 Hz (hop 800) and 11025 Hz (hop 1102: not a tenth of
    the rate): frame counts on both sides of the chunk, the true-peak tile and history, a chunk kernel's workgroup, one hop and
    one block; seeded noise plus DC with a NaN and both infinities planted, a row of zeros, a pitch larger than the row --
    hop energies, true peak and counts equal the restatement bit for bit. Then the two known signals. In a process of its
    own: torch has to be imported before the library is loaded, and in this one the library is loaded already."""
    run = subprocess.run([sys.executable, "-c", ROWS, ROOT], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "loudness rows ok" in run.stdout, (run.stdout[-2000:], run.stderr[-4000:])


# ---- 2. a batch of golden programs of unequal length ---------------------------------------------------------------------

RATE = 8000
KEYS = ["examples__sounds__wooddrum", "examples__sounds__errorsignal", "examples__tests__panning"]
RUNS = [1, 255, 800, 3, 4097]  # then 11289 until every stream has ended


@pytest.fixture(autouse=True)
def forms(oracle):
    oracle.oracle().ora_set_fastmath_forms(ORACLE_FORMS)


def _run_to_the_end(b, stereo, runs, meters=None, loudness=True):
    """float runs of the given lengths, then of 11289 frames, until every stream has ended -> per stream the fetched frames of
    every run (and the meters fed them)"""
    ch = 2 if stereo else 1
    out = [[] for _ in range(b.n)]
    alive, k, inside = [True] * b.n, 0, 0
    while any(alive):
        n = runs[k] if k < len(runs) else 11289
        pcm, more, lens = b.run_f32(n, stereo)
        for s in range(b.n):
            x = pcm[s, :lens[s] * ch].copy()
            out[s].append(x)
            if meters:
                meters[s].run(x)
            if alive[s] and not more[s] and 0 < lens[s] < n:
                inside += 1
            alive[s] = more[s]
        k += 1
    return out, inside


@pytest.mark.parametrize("stereo", [False, True])
def test_a_batch_equals_the_restatement_run_by_run(sa, stereo):
    ch = 2 if stereo else 1
    hop = RATE // 10
    prgs = [load_program(sa, k) for k in KEYS]
    f, taps = sa.loudness_filter(RATE), sa.truepeak_taps()
    meters = [lm.Meter(f, taps, hop, ch) for _ in prgs]
    b = sa.Batch(prgs, RATE)
    b.set_loudness(True)
    fresh = [bytes(r) for r in b.loudness()]
    rows, inside = _run_to_the_end(b, stereo, RUNS, meters)
    assert inside >= 1  # a stream ended inside a run
    assert len({m.pos for m in meters}) == len(prgs) and all(m.pos > 4 * hop for m in meters)
    got = b.loudness()
    for s in range(len(prgs)):
        check_hops(b.loudness_hops(s), meters[s], ("stream", s))
        check_record(sa, got[s], meters[s], ("stream", s))
        assert got[s].true_peak[0] > 0 and (got[s].true_peak[1] > 0) == stereo
        assert got[s].integrated > -70.0
    assert [bytes(r) for r in b.loudness()] == [bytes(r) for r in got]  # (reading changes nothing)
    # one long run per stream: other chunk boundaries, the same energies within the chunked method's accuracy
    b2 = sa.Batch(prgs, RATE)
    b2.set_loudness(True)
    longest = max(m.pos for m in meters)
    b2.run_f32(longest, stereo, fetch=False)
    for s in range(len(prgs)):
        x = np.concatenate(rows[s]).astype(np.float64)
        one, many = b2.loudness_hops(s), b.loudness_hops(s)
        assert one.shape == many.shape
        for c in range(ch):
            ssq = float((lm.clean(x[c::ch]) ** 2).sum())
            assert np.abs(one[:, c] - many[:, c]).max() <= CHUNK_ACCURACY * ssq, (s, c)
    got2 = b2.loudness()
    for s in range(len(prgs)):
        assert got2[s].frames == got[s].frames and abs(got2[s].integrated - got[s].integrated) < 1e-9
        assert bits32(got2[s].true_peak[0]) == bits32(got[s].true_peak[0])  # (the run lengths do not come into the peak)
    b2.close()
    # after a reset the records are a fresh batch's, and the next measurement starts from zero state at frame 0
    b.loudness(reset=True)
    assert [bytes(r) for r in b.loudness()] == fresh and len(b.loudness_hops(0)) == 0
    b.close()


def test_off_means_off_and_refusals_leave_the_batch_where_it_stood(sa):
    prgs = [load_program(sa, k) for k in KEYS[:2]]
    runs = [5000, 3000]

    def render(loud):
        b = sa.Batch(prgs, RATE)
        b.set_metering(True)
        if loud:
            b.set_loudness(True)
            with pytest.raises(RuntimeError, match="bad argument"):
                b.run(100, True)
            with pytest.raises(RuntimeError, match="bad argument"):
                b.run_decimated(2, 100, True)
        rows, _ = _run_to_the_end(b, True, runs, loudness=loud)
        if loud:
            with pytest.raises(RuntimeError, match="bad argument"):
                b.run(100, True)
            with pytest.raises(RuntimeError, match="bad argument"):
                b.run_f32(100, False)  # the other channel layout than the record's
            assert all(r.frames == sum(len(x) for x in rows[s]) // 2 for s, r in enumerate(b.loudness()))
        else:
            assert all(r.frames == 0 and r.blocks == 0 for r in b.loudness())
        lv = [bytes(r) for r in b.levels()]
        b.close()
        return [np.concatenate(r) for r in rows], lv

    on, lv_on = render(True)
    off, lv_off = render(False)
    assert lv_on == lv_off
    for a, c in zip(on, off):
        assert len(a) == len(c) > 0 and a.tobytes() == c.tobytes()


def test_a_refused_run_in_the_middle_does_not_move_the_batch(sa):
    prg = load_program(sa, KEYS[1])
    ref = sa.Batch([prg], RATE)
    want = np.concatenate(_run_to_the_end(ref, False, [3000], loudness=False)[0][0])
    ref.close()
    b = sa.Batch([prg], RATE)
    b.set_loudness(True)
    first = b.run_f32(3000, False)[0][0]
    for bad in (lambda: b.run(500, False), lambda: b.run_decimated(4, 500, False)):
        with pytest.raises(RuntimeError, match="bad argument"):
            bad()
    rest = np.concatenate(_run_to_the_end(b, False, [])[0][0])  # continues at frame 3000
    got = np.concatenate([first, rest])
    assert b.loudness()[0].frames == len(want)
    b.close()
    assert got.tobytes() == want.tobytes()


# ---- 3. the loudness-normalised writer ---------------------------------------------------------------------------------

HEADER = {0: 0, 1: 28, 2: 44, 3: 58}  # RAW, AU, WAV, WAV_F32
FILE_KEY = "examples__tests__panning"


def quantise(x):
    """pcm16(x), all of it in float32"""
    x = np.asarray(x, np.float32)
    x = np.where(np.isnan(x), np.float32(-1.0), x)
    x = np.clip(x, np.float32(-1.0), np.float32(1.0)).astype(np.float32)
    return np.rint(x * np.float32(32767.0)).astype(np.int16)


def _float_render(sa, prg, rate, stereo):
    """the program in float runs on the file writer's lattice, loudness on -> (samples, the record)"""
    ch = 2 if stereo else 1
    call = 256 * rate // 1000
    chunk = 176400 // call * call
    b = sa.Batch([prg], rate)
    b.set_call_len(call)
    b.set_loudness(True)
    out, more = [], True
    while more:
        pcm, m, lens = b.run_f32(chunk, stereo)
        out.append(pcm[0, :lens[0] * ch].copy())
        more = m[0]
    ld = b.loudness()[0]
    b.close()
    return np.concatenate(out), ld


@pytest.mark.parametrize("channels", [1, 2])
def test_loudness_normalised_files(sa, tmp_path, channels):
    rate = 12000
    prg = load_program(sa, FILE_KEY)
    x, ld = _float_render(sa, prg, rate, channels == 2)
    frames = len(x) // channels
    assert ld.frames == frames and ld.integrated > -70.0
    tp = np.float32(max(ld.true_peak))
    assert tp > 0
    # two cases picked from the record: a target 6 dB down under a ceiling far above what that gain reaches, and a target
    # 6 dB up under a ceiling of the true peak as it stands -- the ceiling binds and the gain is exactly 1
    for target, ceiling, binds in ((ld.integrated - 6.0, float(tp), False), (ld.integrated + 6.0, float(tp), True)):
        gain = np.float32(10.0 ** ((target - ld.integrated) / 20.0))
        took_ceiling = bool(tp * gain > np.float32(ceiling))
        if took_ceiling:
            gain = np.float32(ceiling) / tp
        assert took_ceiling == binds
        y = x * gain
        assert y.dtype == np.float32
        for fmt, dtype, want in ((2, "<i2", quantise(y)), (1, ">i2", quantise(y)), (3, "<f4", y)):
            path = str(tmp_path / ("t%d%d" % (fmt, binds)))
            n, got, g = sa.render_file_loudness(prg, rate, path, fmt, channels, target, ceiling)
            assert n == frames and bytes(got) == bytes(ld)
            assert bits32(g) == bits32(gain), (g, gain)
            raw = open(path, "rb").read()
            data = np.frombuffer(raw, dtype, offset=HEADER[fmt])
            assert len(data) == frames * channels
            if fmt == 3:
                d = np.flatnonzero(data.view(np.uint32) != want.view(np.uint32))
            else:
                d = np.flatnonzero(data.astype(np.int16) != want)
            assert len(d) == 0, (target, fmt, len(d), d[:4], data[d[:4]], want[d[:4]])
        if binds:
            assert bits32(gain) == bits32(1.0)
        else:
            assert abs(float(gain) - 10.0 ** (-6.0 / 20.0)) < 1e-6


def test_a_silent_program_is_written_with_gain_1(sa, tmp_path):
    from saugns_amd import voicebank as vb
    prg = vb.build_program([vb.Op("sin", freq=200.0, amp=vb._f32(0.0), time_ms=900)])
    path = str(tmp_path / "silent.wav")
    n, ld, g = sa.render_file_loudness(prg, 8000, path, 2, 2, -16.0, 0.9)
    assert n == 7200 and ld.frames == 7200 and ld.blocks == 6 and ld.gated_blocks == 0 and ld.integrated == -math.inf
    assert g == 1.0 and list(ld.true_peak) == [0, 0]
    assert not any(np.frombuffer(open(path, "rb").read(), "<i2", offset=44) != 0)
