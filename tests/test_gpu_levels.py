"""On-device level metering and the normalised file writer (include/saugns_amd.h: sauAmdLevels, sauAmd_Batch_set_metering,
sauAmd_Batch_levels, sauAmd_Batch_measure_rows, sauAmd_render_file_normalized; kernels: saugns_amd/csrc/k_levels.h).

What is measured is counted again on the host with numpy, under the header's rules: peak, the counts and the frames must be
EQUAL; an int16 measurement's sum of squares too (integers on the device, one division on the host); a float measurement's
sum of squares must lie within n * 2^-52 * S of math.fsum over the exact float64 squares -- n the samples of the channel, S
the sum: every term is exact and non-negative, so any order of additions errs by at most (n - 1) * 2^-53 * S, and the bound is
twice that."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ORACLE_FORMS, load_program
from saugns_amd import voicebank as vb
from saugns_amd.api import POP_PMOD

pytestmark = pytest.mark.gpu

RATE = 44100
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# launch_plan.h (plan_levels), mirrored: the samples the 256 lanes of a workgroup take with one 16-byte load each -- float and
# int16 rows -- and the consecutive samples of a row that one workgroup owns. tests/test_levels_host.py reads the header and
# fails when these no longer match it.
LEVELS_SWEEP_F32 = 1024
LEVELS_SWEEP_S16 = 2048
LEVELS_WG_SAMPLES = 16384


def quantise(x, k=0):
    """pcm16(x * 2^k), all of it in float32"""
    x = np.asarray(x, np.float32) * np.float32(2.0 ** k)
    x = np.where(np.isnan(x), np.float32(-1.0), x)
    x = np.clip(x, np.float32(-1.0), np.float32(1.0)).astype(np.float32)
    return np.rint(x * np.float32(32767.0)).astype(np.int16)


def count_levels(samples, ch, frames):
    """The header's rules on the host -> dict like Levels.as_dict(), with sum_sq exact (fsum) and `n` per channel"""
    samples = np.asarray(samples).reshape(-1)[:frames * ch]
    out = {"frames": frames, "peak": [np.float32(0), np.float32(0)], "sum_sq": [0.0, 0.0], "over": [0, 0], "full_scale": [0, 0],
           "nonfinite": [0, 0], "n": [0, 0]}
    for c in range(ch):
        x = samples[c::ch]
        out["n"][c] = len(x)
        if len(x) == 0:
            continue
        if x.dtype == np.float32:
            fin = np.isfinite(x)
            xf = x[fin]
            out["peak"][c] = np.abs(xf).max() if len(xf) else np.float32(0)
            out["sum_sq"][c] = math.fsum((xf.astype(np.float64) ** 2).tolist())
            with np.errstate(invalid="ignore"):
                out["over"][c] = int(np.count_nonzero(~(np.abs(x) <= np.float32(1.0))))
            out["full_scale"][c] = int(np.count_nonzero(np.abs(quantise(x).astype(np.int32)) == 32767))
            out["nonfinite"][c] = int(np.count_nonzero(~fin))
        else:
            assert x.dtype == np.int16
            a = np.abs(x.astype(np.int64))
            out["peak"][c] = np.float32(a.max()) / np.float32(32767.0)
            out["sum_sq"][c] = float(int((a * a).sum())) / 32767.0 ** 2
            out["over"][c] = int(np.count_nonzero(a == 32768))
            out["full_scale"][c] = int(np.count_nonzero(a >= 32767))
    return out


def add_levels(total, part):
    """accumulate one run's count into a running one (what the device's records do run after run)"""
    if total is None:
        return part
    t = dict(total)
    t["frames"] = total["frames"] + part["frames"]
    t["peak"] = [max(np.float32(a), np.float32(b)) for a, b in zip(total["peak"], part["peak"])]
    for k in ("sum_sq", "over", "full_scale", "nonfinite", "n"):
        t[k] = [a + b for a, b in zip(total[k], part[k])]
    return t


def check_levels(got, want, what, exact_sum, slack=0):
    """got: api.Levels. exact_sum: an int16 measurement (sum_sq equal); else the float bound of this file's docstring, with
    `slack` further roundings of the total allowed for (records that join several runs)."""
    assert int(got.frames) == want["frames"], (what, "frames", int(got.frames), want["frames"])
    for c in range(2):
        for k in ("over", "full_scale", "nonfinite"):
            assert int(getattr(got, k)[c]) == want[k][c], (what, k, c, int(getattr(got, k)[c]), want[k][c])
        gp, wp = np.float32(got.peak[c]), np.float32(want["peak"][c])
        assert gp.view(np.uint32) == wp.view(np.uint32), (what, "peak", c, float(gp), float(wp))
        g, S = float(got.sum_sq[c]), want["sum_sq"][c]
        if exact_sum:
            assert g == S, (what, "sum_sq", c, g, S)
        else:
            assert abs(g - S) <= (want["n"][c] + slack) * 2.0 ** -52 * S, (what, "sum_sq", c, g, S, want["n"][c])


def _raw(lv):
    return bytes(lv)


# ---- 1. crafted rows through measure_rows --------------------------------------------------------------------------------

def smallest_full_scale():
    """the smallest float32 whose pcm16() is 32767 (bit patterns of positive floats are ordered: bisect them)"""
    lo, hi = int(np.float32(0.9999).view(np.uint32)), int(np.float32(1.0).view(np.uint32))
    assert quantise(np.uint32(lo).view(np.float32)) < 32767 and quantise(np.uint32(hi).view(np.float32)) == 32767
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if quantise(np.uint32(mid).view(np.float32)) == 32767:
            hi = mid
        else:
            lo = mid
    return np.uint32(hi).view(np.float32)


def crafted_frames(ch):
    """frame counts: small and odd ones, around 256 and 1024, and around each of plan_levels' constants -- which are in
    samples, so for a stereo row also around half of each"""
    n = [1, 2, 3, 5, 7, 8, 9, 255, 256, 257, 1023, 4097]
    for c in (LEVELS_SWEEP_F32, LEVELS_SWEEP_S16, LEVELS_WG_SAMPLES):
        n += [c - 1, c, c + 1, 3 * c + 7]
        if ch == 2:
            n += [c // 2 - 1, c // 2, c // 2 + 1]
    return sorted(set(n))


def crafted_values(rng, n_rows, samples, f32, case):
    """a seeded normal x 0.7 with the values planted that the rules turn on"""
    x = rng.standard_normal((n_rows, samples)) * 0.7
    if f32:
        x = x.astype(np.float32)
        one = np.float32(1.0)
        planted = [np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf), np.float32(-0.0), one, -one,
                   np.nextafter(one, np.float32(0)), np.nextafter(one, np.float32(2)), smallest_full_scale(),
                   -smallest_full_scale(), np.nextafter(smallest_full_scale(), np.float32(0)), np.float32(1e-40), np.float32(-3.0)]
    else:
        x = np.clip(np.rint(x * 32767.0 * 0.45), -32768, 32767).astype(np.int16)
        planted = [np.int16(32767), np.int16(-32767), np.int16(-32768), np.int16(32766), np.int16(0), np.int16(-1)]
    planted = planted[case % len(planted):] + planted[:case % len(planted)]  # (short rows take turns with the values)
    for r in range(n_rows):
        at = rng.permutation(samples)[:len(planted)]
        for k, i in enumerate(at):
            x[r, i] = planted[(k + r) % len(planted)]
        # the last sample (the scalar tail), the first, and both sides of a workgroup's boundary
        x[r, samples - 1] = planted[(case + r) % len(planted)]
        for k, i in enumerate((0, LEVELS_WG_SAMPLES - 1, LEVELS_WG_SAMPLES, LEVELS_WG_SAMPLES + 1)):
            if i < samples - 1 and samples > 16:
                x[r, i] = planted[(case + r + k + 1) % len(planted)]
    return x


def crafted_rows_main():
    """(in a process of its own, torch imported first: see test_crafted_rows)"""
    import torch
    import saugns_amd as sa
    b = sa.Batch([vb.build_program([vb.Op("sin", freq=200.0, time_ms=10)])], RATE)  # (never run: measure_rows needs its device only)
    rng = np.random.default_rng(20261017)
    cases = 0
    for f32 in (True, False):
        size = 4 if f32 else 2
        for ch in (1, 2):
            for n_rows in (1, 3):
                for frames in crafted_frames(ch):
                    samples = frames * ch
                    x = crafted_values(rng, n_rows, samples, f32, cases)
                    pitch_el = (samples * size + 15) // 16 * 16 // size + 16 // size * (1 + cases % 3)  # larger than the row
                    # what lies between the rows would show in every count if a kernel read it
                    t = torch.full((n_rows, pitch_el), float("nan") if f32 else -32768, dtype=torch.float32 if f32 else torch.int16,
                                   device="cuda")
                    t[:, :samples] = torch.from_numpy(x).to("cuda")
                    torch.cuda.synchronize()
                    assert t.data_ptr() % 16 == 0 and (pitch_el * size) % 16 == 0
                    got = b.measure_rows(t.data_ptr(), pitch_el * size, n_rows, f32, frames, ch)
                    again = b.measure_rows(t.data_ptr(), pitch_el * size, n_rows, f32, frames, ch)
                    assert len(got) == n_rows
                    for r in range(n_rows):
                        what = ("f32" if f32 else "s16", "ch", ch, "rows", n_rows, "frames", frames, "row", r)
                        check_levels(got[r], count_levels(x[r], ch, frames), what, exact_sum=not f32)
                        assert _raw(got[r]) == _raw(again[r]), (what, "measured twice")
                        if ch == 1:
                            assert got[r].peak[1] == 0 and got[r].sum_sq[1] == 0 and got[r].full_scale[1] == 0
                    cases += 1
    # frames == 0: zeroed records; refusals: a misaligned address, an odd pitch, three channels, host memory
    t = torch.zeros((2, 64), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for lv in b.measure_rows(t.data_ptr(), 256, 2, True, 0, 2):
        assert _raw(lv) == bytes(80)
    refused = 0
    for args in ((t.view(-1)[1:].data_ptr(), 256, 1, True, 8, 1), (t.data_ptr(), 260, 2, True, 8, 1), (t.data_ptr(), 256, 2, True, 8, 3),
                 (t.data_ptr() + 8, 256, 1, False, 8, 1), (t.data_ptr(), 200, 2, False, 8, 2)):
        try:
            b.measure_rows(*args)
        except RuntimeError as e:
            assert "bad argument" in str(e), e
            refused += 1
    assert refused == 5
    host = np.zeros(1024, np.float32)
    try:
        b.measure_rows((host.ctypes.data + 15) & ~15, 256, 2, True, 8, 1)
        raise AssertionError("host memory was measured")
    except RuntimeError as e:
        assert "bad argument" in str(e), e
    try:  # rows that reach beyond their allocation
        b.measure_rows(t.data_ptr(), 1 << 20, 60000, True, 8, 1)
        raise AssertionError("rows beyond the allocation were measured")
    except RuntimeError as e:
        assert "bad argument" in str(e), e
    # the batch's own rows, after the caller's own processing, through the device view
    b2 = sa.Batch([vb.build_program([vb.Op("sin", freq=200.0 + 50.0 * k, time_ms=300, pan=vb.Line(0.25 * k))]) for k in range(3)], RATE)
    b2.run_f32(5000, True, fetch=False)
    b2.sync()
    view = b2.device_tensor(5000, True)
    view *= 1.5
    torch.cuda.synchronize()
    got = b2.measure_rows(view.data_ptr(), b2.device_pcm_pitch(), 3, True, 5000, 2)
    host = view.cpu().numpy().reshape(3, -1)
    for r in range(3):
        check_levels(got[r], count_levels(host[r], 2, 5000), ("device view", r), exact_sum=False)
    assert all(lv.frames == 0 for lv in b2.levels())  # (the batch's own records are untouched)
    del view
    b2.close()
    b.close()
    print("crafted rows ok:", cases, "cases")


CRAFTED = r"""
import sys
import torch  # (before the library: torch's wheel brings a HIP runtime of its own, and a process has room for one -- api.Batch.device_tensor)
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_levels
test_gpu_levels.crafted_rows_main()
"""


def test_crafted_rows():
    """measure_rows on torch tensors: float32 and int16, mono and stereo, 1 and 3 rows with a pitch larger than the row, frame
    counts on both sides of everything the kernel's loop turns on, every value planted that a rule turns on; the same tensor
    measured twice gives the same bits; misaligned rows, an odd pitch, host memory are refused. In a process of its own: torch
    has to be imported before the library is loaded, and in this one the library is loaded already."""
    run = subprocess.run([sys.executable, "-c", CRAFTED, ROOT], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "crafted rows ok" in run.stdout, (run.stdout[-2000:], run.stderr[-4000:])


# ---- 2. batch metering equals the host's count ---------------------------------------------------------------------------

BANK_FRAMES = 3000  # (not a multiple of anything of the kernel's)


def _bank40(ampmult):
    voices = vb.config3_voices(40, 1)
    for i, v in enumerate(voices):
        v.pan = vb.Line(vb._num(".2f", ((i * 37) % 100) / 100.0))
    return vb.build_program(voices, ampmult=ampmult)


@pytest.fixture(autouse=True)
def forms(oracle):
    oracle.oracle().ora_set_fastmath_forms(ORACLE_FORMS)


def _metered_run(sa, prg, f32, stereo, fetch=True):
    b = sa.Batch([prg], RATE)
    b.set_metering(True)
    pcm = (b.run_f32 if f32 else b.run)(BANK_FRAMES, stereo, fetch=fetch)[0]
    lv = b.levels()[0]
    b.close()
    return pcm, lv


@pytest.mark.parametrize("f32", [True, False])
@pytest.mark.parametrize("stereo", [False, True])
def test_a_metered_run_equals_the_hosts_count(sa, stereo, f32):
    ch = 2 if stereo else 1
    prg = _bank40(1.0)
    pcm, lv = _metered_run(sa, prg, f32, stereo)
    assert pcm[0].any()
    check_levels(lv, count_levels(pcm[0], ch, BANK_FRAMES), ("bank", f32, stereo), exact_sum=not f32)
    assert lv.peak[0] > 0 and (lv.peak[1] > 0) == stereo
    none, lv2 = _metered_run(sa, prg, f32, stereo, fetch=False)  # PCM left on the device: the same record
    assert none is None and _raw(lv2) == _raw(lv)


@pytest.mark.parametrize("stereo", [False, True])
def test_full_scale_of_a_float_run_is_what_an_int16_run_puts_on_the_rail(sa, oracle, stereo):
    ch = 2 if stereo else 1
    _, quiet = _metered_run(sa, _bank40(1.0), True, stereo, fetch=False)
    peak = max(quiet.peak)
    assert 0 < peak < 1
    prg = _bank40(float(np.float32(1.04 / peak)))  # the loudest samples now pass +-1 by a few percent
    x, hot = _metered_run(sa, prg, True, stereo)
    n_over = sum(hot.over)
    assert 0 < n_over <= 0.05 * BANK_FRAMES * ch, (n_over, list(hot.peak))
    check_levels(hot, count_levels(x[0], ch, BANK_FRAMES), ("hot bank", stereo), exact_sum=False)
    pcm, rail = _metered_run(sa, prg, False, stereo)
    assert list(rail.full_scale) == list(hot.full_scale) and sum(rail.full_scale) >= n_over
    want = oracle.oracle_render(prg.ptr, RATE, stereo, chunk=BANK_FRAMES, max_frames=BANK_FRAMES)
    for c in range(ch):
        assert int(np.count_nonzero(np.abs(want[c::ch].astype(np.int32)) == 32767)) == hot.full_scale[c], c
    assert (pcm[0] == want).all()


# ---- 3. accumulation, stream ends, reset ---------------------------------------------------------------------------------

def _ending_streams(sa):
    """streams for consecutive runs of 5000 frames at 12000 Hz: one that ends inside the first run, one inside the third, one
    inside the fourth, and a script whose events leave segments with nothing sounding"""
    def v(i, ms):
        m = vb.Op("sin", freq=vb.Line(float(1 + i % 3), ratio=True), amp=vb._f32(0.5))
        return vb.Op(("sin", "tri", "sqr")[i % 3], freq=vb._num(".3f", 150.0 + 31.7 * i), time_ms=ms,
                     pan=vb.Line(vb._num(".2f", ((i * 37) % 100) / 100.0)), mods={POP_PMOD: [m]})
    return [vb.build_program([v(5, 400)]), vb.build_program([v(0, 900), v(1, 500)]), vb.build_program([v(3, 1300), v(4, 600)]),
            load_program(sa, "devtests__voice-reuse")]


@pytest.mark.parametrize("stereo", [False, True])
def test_records_accumulate_over_runs_of_both_formats(sa, stereo):
    ch = 2 if stereo else 1
    R, srate = 5000, 12000
    prgs = _ending_streams(sa)
    b = sa.Batch(prgs, srate)
    b.set_metering(True)
    total = [None] * len(prgs)
    ended_at = [None] * len(prgs)
    for k in range(4):
        f32 = k % 2 == 1
        pcm, more, lens = (b.run_f32 if f32 else b.run)(R, stereo)
        for s in range(len(prgs)):
            total[s] = add_levels(total[s], count_levels(pcm[s], ch, lens[s]))
            if not more[s] and ended_at[s] is None:
                ended_at[s] = k
        lv = b.levels()
        for s in range(len(prgs)):
            # (sum_sq: the device joins its int16 and float totals with one division and one addition more than the host)
            check_levels(lv[s], total[s], ("run", k, "stream", s), exact_sum=k == 0, slack=8)
    assert ended_at[0] == 0 and ended_at[1] == 2 and ended_at[2] == 3, ended_at
    assert total[0]["frames"] == 4800 and total[1]["frames"] == 10800 and total[2]["frames"] == 15600
    before = [_raw(x) for x in b.levels()]
    pcm, more, lens = b.run(R, stereo)  # a stream that has ended adds nothing
    after = b.levels(reset=True)
    for s in range(len(prgs)):
        if ended_at[s] is not None:
            assert lens[s] == 0 and _raw(after[s]) == before[s], s
    assert all(_raw(x) == bytes(80) for x in b.levels())
    pcm, more, lens = b.run_f32(R, stereo)  # ... and the records begin again from zero
    lv = b.levels()
    for s in range(len(prgs)):
        check_levels(lv[s], count_levels(pcm[s], ch, lens[s]), ("after the reset", s), exact_sum=False)
    b.close()


# ---- 4. metering changes nothing -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("stereo", [False, True])
def test_metering_changes_no_sample(sa, stereo):
    prgs = _ending_streams(sa)
    out = {}
    for on in (False, True):
        b = sa.Batch(prgs, 12000)
        b.set_metering(on)
        runs = []
        for k in range(4):
            pcm, more, lens = (b.run_f32 if k % 2 else b.run)(5000, stereo)
            runs.append((pcm.tobytes(), more, lens))
        lv = b.levels()
        assert all((x.frames > 0) == on for x in lv)
        if not on:
            assert all(_raw(x) == bytes(80) for x in lv)
        out[on] = runs
        b.close()
    assert out[False] == out[True]


# ---- 5. normalised files -------------------------------------------------------------------------------------------------

HEADER = {0: 0, 1: 28, 2: 44, 3: 58}  # RAW, AU, WAV, WAV_F32
CALL = 256 * RATE // 1000
CHUNK = 176400 // CALL * CALL  # sauAmd_render_file's frames per device run


def _file_program():
    """4.2 s, so that the writer makes two device runs (its two host slots both carry a chunk)"""
    def v(i, ms, amp):
        m = vb.Op("sin", freq=vb.Line(float(1 + i % 3), ratio=True), amp=vb._f32(0.5))
        return vb.Op(("sin", "saw", "tri")[i % 3], freq=vb._num(".3f", 170.0 + 41.3 * i), time_ms=ms, amp=vb._f32(amp),
                     pan=vb.Line(vb._num(".2f", 0.15 + 0.3 * i)), mods={POP_PMOD: [m]})
    return vb.build_program([v(0, 4200, 0.9), v(1, 2500, 0.7), v(2, 3900, 0.8)])


def _metered_float_render(sa, prg, stereo):
    """the program in float runs on the file writer's lattice -> (samples, the metered record)"""
    ch = 2 if stereo else 1
    b = sa.Batch([prg], RATE)
    b.set_call_len(CALL)
    b.set_metering(True)
    out, more = [], True
    while more:
        pcm, m, lens = b.run_f32(CHUNK, stereo)
        out.append(pcm[0, :lens[0] * ch].copy())
        more = m[0]
    lv = b.levels()[0]
    b.close()
    return np.concatenate(out), lv


@pytest.mark.parametrize("channels", [1, 2])
def test_normalised_files(sa, tmp_path, channels):
    stereo = channels == 2
    prg = _file_program()
    x, lv = _metered_float_render(sa, prg, stereo)
    frames = len(x) // channels
    assert frames > CHUNK and lv.frames == frames
    peak = np.float32(max(lv.peak))
    assert peak > 0
    # a target equal to the measured peak: the gain is exactly 1.0f and every file is sauAmd_render_file's, byte for byte
    for fmt in (0, 1, 2, 3):
        plain, norm = str(tmp_path / ("plain%d" % fmt)), str(tmp_path / ("norm%d" % fmt))
        assert sa.render_file(prg, RATE, plain, fmt, channels) == frames
        n, got = sa.render_file_normalized(prg, RATE, norm, fmt, channels, float(peak))
        assert n == frames and _raw(got) == _raw(lv), fmt
        a, b = open(plain, "rb").read(), open(norm, "rb").read()
        assert len(a) == HEADER[fmt] + frames * channels * (4 if fmt == 3 else 2)
        assert a == b, (fmt, len(a), len(b))
    # other targets: the int16 formats hold pcm16(x * gain), rounded once after the gain; the float one x * gain
    for target in (0.5, 1.0):
        gain = np.float32(target) / peak
        y = x * gain
        assert y.dtype == np.float32
        for fmt, dtype, want in ((2, "<i2", quantise(y)), (1, ">i2", quantise(y)), (0, "<i2", quantise(y)), (3, "<f4", y)):
            path = str(tmp_path / ("t%d" % fmt))
            n, got = sa.render_file_normalized(prg, RATE, path, fmt, channels, target)
            assert n == frames and _raw(got) == _raw(lv)
            raw = open(path, "rb").read()
            data = np.frombuffer(raw, dtype, offset=HEADER[fmt])
            assert len(data) == frames * channels
            if fmt == 3:
                d = np.flatnonzero(data.view(np.uint32) != want.view(np.uint32))
            else:
                d = np.flatnonzero(data.astype(np.int16) != want)
            assert len(d) == 0, (target, fmt, len(d), d[:4], data[d[:4]], want[d[:4]])
        if target == 1.0:  # the loudest sample is on the rail, and nothing was clamped on the way
            q = quantise(y).astype(np.int32)
            assert np.abs(q).max() == 32767


def test_a_silent_program_is_written_with_gain_1(sa, tmp_path):
    prg = vb.build_program([vb.Op("sin", freq=200.0, amp=vb._f32(0.0), time_ms=100)])
    for fmt in (2, 3):
        path = str(tmp_path / ("silent%d" % fmt))
        n, lv = sa.render_file_normalized(prg, RATE, path, fmt, 2, 0.5)
        assert n == 4410 and lv.frames == 4410 and list(lv.peak) == [0, 0] and list(lv.sum_sq) == [0, 0]
        raw = open(path, "rb").read()
        assert len(raw) == HEADER[fmt] + n * 2 * (4 if fmt == 3 else 2)
        # (zeros of either sign in the float file: 0 * 1.0f)
        assert not any(np.frombuffer(raw, "<f4" if fmt == 3 else "<i2", offset=HEADER[fmt]) != 0)
