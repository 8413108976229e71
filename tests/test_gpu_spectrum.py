"""The on-device spectrum meter (include/saugns_amd.h, section "Spectrum": sauAmd_Batch_spectrum_rows, sauAmd_Batch_create_spectrum,
sauAmd_Spectrum_feed, sauAmd_Spectrum_read, sauAmd_render_spectrum; kernels: saugns_amd/csrc/k_spectrum.h).

The header fixes every operation and its order, and the sums are a function of the fed sequence only, so what the device
delivers -- sums, segment counts, spectrograms -- is compared with the Python restatement (tests/spectrum_model.py, itself held
against numpy.fft in tests/test_spectrum_host.py) BIT FOR BIT, and a sequence cut into feeds of any lengths with itself in one
piece."""
import ctypes as C
import math
import os
import subprocess
import sys
import traceback

import numpy as np
import pytest

import spectrum_model as mdl
from conftest import ORACLE_FORMS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANTED = [np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf), np.float32(-0.0)]


def same_bits(got, want, what):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    d = np.flatnonzero(got.view(u) != want.view(u))
    assert len(d) == 0, (what, len(d), "of", len(got), "first at", d[:4], got[d[:4]], want[d[:4]])


def crafted_values(rng, n_rows, frames, ch, case, zero_last=True):
    """seeded noise with a NaN, both infinities and a -0.0 planted (and at the row's two ends in turn); the last row zeros"""
    x = (rng.standard_normal((n_rows, frames * ch)) * 0.35).astype(np.float32)
    for r in range(n_rows):
        at = rng.permutation(frames * ch)[:len(PLANTED)]
        for k, i in enumerate(at):
            x[r, i] = PLANTED[(k + r + case) % len(PLANTED)]
        x[r, -1] = PLANTED[(case + r) % len(PLANTED)]
        x[r, 0] = PLANTED[(case + r + 1) % len(PLANTED)]
    if zero_last:
        x[n_rows - 1] = 0.0
    return x


_tables = {}


def tables(sa, L):
    if L not in _tables:
        _tables[L] = (sa.spectrum_window(L), sa.spectrum_twiddles(L))
    return _tables[L]


def raw_rows(b, ptr, pitch, n_rows, frames, ch, L, hop, power, segs, gram, cap):
    """sauAmd_Batch_spectrum_rows as it stands: the caller's arrays, the caller's capacity"""
    return b._L.sauAmd_Batch_spectrum_rows(b._b, ptr, pitch, n_rows, frames, ch, L, hop,
                                           power.ctypes.data_as(C.POINTER(C.c_double)) if power is not None else None,
                                           segs.ctypes.data_as(C.POINTER(C.c_uint64)) if segs is not None else None,
                                           gram.ctypes.data_as(C.POINTER(C.c_float)) if gram is not None else None, cap)


# ---- 1. crafted rows through spectrum_rows (in a process of its own, torch imported first) -----------------------------------

def _rows_case(torch, sa, b, rng, L, hop, ch, frames, n_rows, case):
    N, bins = 1 << L, (1 << L) // 2 + 1
    w, tw = tables(sa, L)
    x = crafted_values(rng, n_rows, frames, ch, case)
    pitch_el = (frames * ch * 4 + 15) // 16 * 4 + 4 * (1 + case % 3)  # larger than the row
    t = torch.full((n_rows, pitch_el), 1e30, dtype=torch.float32, device="cuda")  # what lies between the rows would show in the sums
    t[:, :frames * ch] = torch.from_numpy(x).to("cuda")
    torch.cuda.synchronize()
    S = mdl.segments(frames, N, hop)
    need = n_rows * ch * S * bins
    out = []
    for _ in range(2):
        power, segs = np.full((n_rows, ch, bins), 7.0), np.full(n_rows, 77, np.uint64)
        gram = np.full(need + 64, 7.0, np.float32)
        assert raw_rows(b, t.data_ptr(), pitch_el * 4, n_rows, frames, ch, L, hop, power, segs, gram, need), sa.api.last_error(b._L)
        out.append((power, segs, gram))
    what = ("L", L, "hop", hop, "ch", ch, "frames", frames)
    assert all(a.tobytes() == c.tobytes() for a, c in zip(out[0], out[1])), (what, "called twice")
    power, segs, gram = out[0]
    assert (gram[need:] == 7.0).all(), (what, "a store beyond the spectrogram's [S]")
    gram = gram[:need].reshape(n_rows, ch, S, bins)
    for r in range(n_rows):
        p, S_m, g = mdl.measure(x[r], w, tw, L, hop, ch)
        assert int(segs[r]) == S_m == S, (what, r, segs[r], S_m)
        same_bits(power[r], p, what + ("row", r, "sums"))
        same_bits(gram[r], g, what + ("row", r, "spectrogram"))
    assert not power[n_rows - 1].any() and not gram[n_rows - 1].any()  # the row of zeros
    if S:
        assert power[0].max() > 0.0
    else:
        assert not power.any()
    return S


def rows_main(torch, sa, b):
    rng = np.random.default_rng(20261019)
    L, N = 8, 256
    cases = 0
    for hop in (32, 100, 256):
        for ch in (1, 2):
            for frames in (N - 1, N, N + hop - 1, N + hop, N + 15 * hop, N + 16 * hop, N + 33 * hop + 7):
                _rows_case(torch, sa, b, rng, L, hop, ch, frames, 3, cases)
                cases += 1
    assert _rows_case(torch, sa, b, rng, 11, 1024, 2, 2048 + 18 * 1024, 2, cases) == 19
    assert _rows_case(torch, sa, b, rng, 12, 512, 1, 4096 + 34 * 512 + 5, 2, cases + 1) == 35
    # frames == 0: zero sums; then the refusals
    t = torch.full((2, 1024), 0.25, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    p, s = b.spectrum_rows(t.data_ptr(), 4096, 2, 0, 2, 8, 64)
    assert s == [0, 0] and not p.any()
    host = np.zeros(4096, np.float32)
    hp = (host.ctypes.data + 15) & ~15
    bins, S = 129, (512 - 256) // 64 + 1
    need = 2 * 2 * S * bins
    names = ("ptr", "pitch", "n_rows", "frames", "channels", "log2n", "hop", "power", "segs", "gram", "cap")
    power, segs, gram = np.full((2, 2, bins), 7.0), np.full(2, 77, np.uint64), np.full(need, 7.0, np.float32)
    ok = dict(zip(names, (t.data_ptr(), 4096, 2, 512, 2, 8, 64, power, segs, gram, need)))

    def but(**kw):
        a = dict(ok)
        a.update(kw)
        return tuple(a[k] for k in names)

    bad = [but(ptr=t.view(-1)[1:].data_ptr()), but(pitch=4100), but(ptr=hp), but(ptr=0), but(pitch=2048),  # (a pitch below the row)
           but(pitch=1 << 20, n_rows=60000),  # (rows that run out of their allocation)
           but(channels=3), but(channels=0), but(log2n=7), but(log2n=13), but(hop=31), but(hop=257), but(hop=0), but(n_rows=0),
           but(power=None), but(segs=None), but(cap=need - 1)]
    for args in bad:
        assert not raw_rows(b, *args), ("not refused", args[:7], args[10])
        assert "bad argument" in sa.api.last_error(b._L), (args[:7], sa.api.last_error(b._L))
    assert (power == 7.0).all() and (segs == 77).all() and (gram == 7.0).all()  # a refused call has written nothing
    assert raw_rows(b, *but())  # (and the arguments they were varied from are good ones)
    assert (segs == S).all() and (power != 7.0).all() and (gram != 7.0).all()
    m = b.create_spectrum(2, 2, 8, 64)
    for args in ((t.view(-1)[1:].data_ptr(), 4096, [8, 8]), (t.data_ptr(), 4100, [8, 8]), (hp, 4096, [8, 8]), (0, 4096, [8, 8]),
                 (t.data_ptr(), 2048, [512, 8]), (t.data_ptr(), 1 << 34, [8, 512])):
        try:
            m.feed(*args)
        except RuntimeError as e:
            assert "bad argument" in str(e), (args, e)
        else:
            raise AssertionError(("not refused", args))
    p, s = m.read()
    assert s == [0, 0] and not p.any()  # the refused feeds have changed nothing
    m.close()
    print("cases:", cases + 2)


# ---- 2. feeds ------------------------------------------------------------------------------------------------------------------

def feeds_main(torch, sa, b):
    rng = np.random.default_rng(77)
    L, hop, N = 8, 100, 256
    w, tw = tables(sa, L)
    lengths = [5003, 3333, 4100]
    pieces = [1, 7, 99, 100, 101, 255, 256, 257, 1600, 0, 3, 1000, 5000, 5000, 5000]
    for ch in (2, 1):
        x = [crafted_values(rng, 1, n, ch, r, zero_last=False)[0] for r, n in enumerate(lengths)]
        want = [mdl.measure(x[r], w, tw, L, hop, ch) for r in range(3)]
        assert [v[1] for v in want] == [mdl.segments(n, N, hop) for n in lengths] == [48, 31, 39]  # whole groups, and not
        keep = []

        def stage(slices):
            width = (max(max(len(s) for s in slices), 4) + 3) // 4 * 4 + 4
            t = torch.full((3, width), 1e30, dtype=torch.float32, device="cuda")
            for r, s in enumerate(slices):
                if len(s):
                    t[r, :len(s)] = torch.from_numpy(s).to("cuda")
            torch.cuda.synchronize()
            keep.append(t)  # (alive until the meter has been read: the feed is asynchronous)
            return t.data_ptr(), width * 4

        # spectrum_rows of the whole, row by row (the rows differ in length)
        for r in range(3):
            ptr, pitch = stage([x[r], x[r][:0], x[r][:0]])
            p, s = b.spectrum_rows(ptr, pitch, 1, lengths[r], ch, L, hop)
            assert s == [want[r][1]]
            same_bits(p[0], want[r][0], ("rows call", ch, r))
        m = b.create_spectrum(3, ch, L, hop)
        # in one piece
        ptr, pitch = stage(x)
        m.feed(ptr, pitch, lengths)
        one, s_one = m.read()
        again, s_again = m.read(reset=True)  # a read changes nothing; the reset comes behind it
        assert s_one == s_again == [v[1] for v in want] and one.tobytes() == again.tobytes()
        for r in range(3):
            same_bits(one[r], want[r][0], ("one piece", ch, r))
        fresh, s_fresh = m.read()
        assert s_fresh == [0, 0, 0] and not fresh.any()
        # in pieces, some rows given nothing in some feeds, a read in the middle
        cur = [0, 0, 0]
        models = [mdl.Meter(w, tw, L, hop, ch) for _ in range(3)]
        for i, n in enumerate(pieces):
            fr = [0 if (i + r) % 4 == 3 else min(n, lengths[r] - cur[r]) for r in range(3)]
            sl = [x[r][cur[r] * ch:(cur[r] + fr[r]) * ch] for r in range(3)]
            ptr, pitch = stage(sl)
            m.feed(ptr, pitch, fr)
            for r in range(3):
                models[r].feed(sl[r])
                cur[r] += fr[r]
            if i in (5, 8, 11):  # a read in the middle, without reset
                mid, s_mid = m.read()
                for r in range(3):
                    pm, sm = models[r].read()
                    assert s_mid[r] == sm
                    same_bits(mid[r], pm, ("middle", ch, i, r))
        assert cur == lengths
        got, s_got = m.read(reset=True)
        assert s_got == s_one and got.tobytes() == one.tobytes()
        # behind the reset: a fresh record
        ptr, pitch = stage([v[:1000 * ch] for v in x])
        m.feed(ptr, pitch, [1000, 0, 999])
        short, s_short = m.read()
        for r, n in enumerate([1000, 0, 999]):
            p, s, _ = mdl.measure(x[r][:n * ch], w, tw, L, hop, ch)
            assert s_short[r] == s
            same_bits(short[r], p, ("behind the reset", ch, r))
        m.close()
        del keep[:]


# ---- 5. what the numbers mean ------------------------------------------------------------------------------------------------

def sine_main(torch, sa, b):
    """a float sine on a bin centre, L = 11, one segment: its bin holds the maximum, and every bin more than four away lies at
    least 150 dB below it. That is a condition on the input: the restatement holds it with 13 dB to spare (54.2 dB at the peak,
    -109.4 dB at most elsewhere: the float32 samples' rounding), and the device equals the restatement."""
    L, N, k0 = 11, 2048, 200
    w, tw = tables(sa, L)
    x = np.sin(2.0 * math.pi * k0 * np.arange(N) / N).astype(np.float32)
    t = torch.from_numpy(x).to("cuda").reshape(1, N)
    torch.cuda.synchronize()
    p, s = b.spectrum_rows(t.data_ptr(), N * 4, 1, N, 1, L, N)
    want, S, _ = mdl.measure(x, w, tw, L, N, 1)
    assert s == [1] and S == 1
    same_bits(p[0], want, "sine")
    p = p[0, 0]
    far = np.abs(np.arange(N // 2 + 1) - k0) > 4
    with np.errstate(divide="ignore"):
        db = 10.0 * np.log10(p)
    print("sine: %.1f dB at the peak, %.1f dB at most elsewhere" % (db[k0], db[far].max()))
    assert p.argmax() == k0 and abs(db[k0] - 54.2) < 0.1
    assert db[far].max() <= db[k0] - 150.0


SECTIONS = [("rows", rows_main), ("feeds", feeds_main), ("sine", sine_main)]


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
            print("spectrum %s FAILED\n%s" % (name, traceback.format_exc()))
            break
        print("spectrum %s ok" % name)
    b.close()


TORCH = r"""
import sys
import torch  # (before the library: torch's wheel brings a HIP runtime of its own, and a process has room for one -- api.Batch.device_tensor)
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_spectrum
test_gpu_spectrum.torch_main()
"""


@pytest.fixture(scope="module")
def torch_run():
    """The three tests on rows of device memory of the test's own (torch tensors) share one process: torch has to be imported
    before the library is loaded, in this one the library is loaded already, and one import serves them all."""
    run = subprocess.run([sys.executable, "-c", TORCH, ROOT], capture_output=True, text=True, timeout=600)
    return run


def _section(run, name):
    assert "spectrum %s ok" % name in run.stdout, (run.returncode, run.stdout[-4000:], run.stderr[-4000:])


def test_rows(torch_run):
    """spectrum_rows on torch tensors at L = 8 with hop 32, 100 and 256, mono and stereo, three rows of which the last is zeros:
    frame counts on both sides of the first segment, the second, a group's end and three groups; seeded noise with a NaN, both
    infinities and a -0.0 planted, the two ends included, pitches larger than the rows with 1e30 between them -- sums, segment
    counts and spectrograms equal the restatement bit for bit, a call made twice gives identical bytes, and nothing is written
    behind the spectrogram's [S]. One case each at L = 11 (19 segments) and L = 12 (hop N / 8, 35 segments). Then the refusals,
    none of which writes anything."""
    _section(torch_run, "rows")


def test_feeds(torch_run):
    """three rows of different lengths, L = 8, hop 100, stereo and mono: fed in one piece and in pieces of 1, 7, 99, 100, 101,
    255, 256, 257, 1600, 0, 3, .. frames with some rows given nothing in some feeds -- the reads equal each other, spectrum_rows
    of the whole and the restatement bit for bit; a read in the middle changes nothing; a read with reset starts a fresh
    record."""
    _section(torch_run, "feeds")


def test_a_sine_on_a_bin_centre(torch_run):
    _section(torch_run, "sine")
    assert torch_run.returncode == 0, (torch_run.stdout[-2000:], torch_run.stderr[-4000:])


# ---- 3. a batch of two programs of unequal length, fed run by run ----------------------------------------------------------------

RATE = 8000


@pytest.fixture(autouse=True)
def forms(oracle):
    oracle.oracle().ora_set_fastmath_forms(ORACLE_FORMS)


def _programs():
    """two voices of different lengths; the second is silent for its first 200 ms (those of tests/test_gpu_limiter.py)"""
    from saugns_amd import voicebank as vb
    one = vb.Op("sin", freq=440.0, amp=vb.Line(2.4, goal=0.3), time_ms=900, pan=-0.4)
    late = vb.Op("saw", freq=97.0, amp=vb.Line(0.1, goal=2.5), time_ms=500, pan=0.7)
    late.start_ms = 200
    return [vb.build_program([one]), vb.build_program([late])]


@pytest.mark.parametrize("stereo", [False, True])
def test_a_batch_fed_run_by_run(sa, stereo):
    ch = 2 if stereo else 1
    L, hop = 8, 100
    w, tw = tables(sa, L)
    prgs = _programs()
    results = []
    for metering in (False, True):
        b = sa.Batch(prgs, RATE)
        if metering:
            b.set_metering(True)
        m = b.create_spectrum(2, ch, L, hop)
        rows, more = [[], []], [True, True]
        for n in [1, 7, 255, 256, 257, 1000, 3001] + [1777] * 8:
            if not any(more):
                break
            pcm, more, lens = b.run_f32(n, stereo)
            m.feed(b.device_pcm_f32(0), b.device_pcm_pitch(), lens)
            for s in range(2):
                rows[s].append(pcm[s, :lens[s] * ch].copy())
        assert not any(more)
        got, segs = m.read()
        m.close()
        b.close()
        x = [np.concatenate(r) for r in rows]
        assert len(x[0]) != len(x[1]) and not x[1][:(RATE // 5 - 8) * ch].any() and np.abs(x[1]).max() > 1.0
        for s in range(2):
            p, S, _ = mdl.measure(x[s], w, tw, L, hop, ch)
            assert segs[s] == S > 16
            same_bits(got[s], p, ("stream", s, "metering", metering))
        results.append((got.tobytes(), segs))
    assert results[0] == results[1]  # level metering beside it changes nothing


# ---- 4. render_spectrum ------------------------------------------------------------------------------------------------------------

def _short_program():
    from saugns_amd import voicebank as vb
    a = vb.Op("saw", freq=311.0, amp=vb.Line(0.8, goal=0.2), time_ms=700, pan=-0.5)
    c = vb.Op("sqr", freq=1237.0, amp=0.3, time_ms=450, pan=0.6)
    c.start_ms = 100
    return vb.build_program([a, c])


@pytest.mark.parametrize("factor", [1, 2])
@pytest.mark.parametrize("channels", [1, 2])
def test_render_spectrum_measures_what_the_file_holds(sa, tmp_path, channels, factor):
    L, hop = 9, 256
    w, tw = tables(sa, L)
    prg = _short_program()
    path = str(tmp_path / "x.wav")
    if factor == 1:
        n = sa.render_file(prg, RATE, path, sa.api.SNDFILE_WAV_F32, channels)
    else:
        n = sa.render_file_oversampled(prg, RATE, factor, path, sa.api.SNDFILE_WAV_F32, channels)
    x = np.frombuffer(open(path, "rb").read(), "<f4", offset=58).astype(np.float32)
    assert len(x) == n * channels and 0 < n < RATE and np.abs(x).max() > 0.1
    want, S, _ = mdl.measure(x, w, tw, L, hop, channels)
    got, segs, frames = sa.render_spectrum(prg, RATE, factor, channels, L, hop)
    assert frames == n and segs == S == (n - 512) // hop + 1 > 16
    same_bits(got, want, ("render_spectrum", channels, factor))
