"""The on-device look-ahead true-peak limiter and the loudness writer that uses it (include/saugns_amd.h, section "Limiter":
sauAmd_Batch_limit_rows, sauAmd_Batch_run_limited_f32, sauAmd_Batch_limiter_stats, sauAmd_render_file_loudness_limited;
kernels: saugns_amd/csrc/k_limiter.h).

The header fixes every operation and its order, and the output is a function of the input sequence only, so what the device
delivers -- rows, files, statistics -- is compared with the Python restatement (tests/limiter_model.py) BIT FOR BIT, and a
sequence cut into runs of any lengths with itself in one piece."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import limiter_model as mdl
from conftest import ORACLE_FORMS, load_program

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = [(2.0, 0.8912509), (1.0, 0.5)]


def same_bits(got, want, what):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    u = {2: np.uint16, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    d = np.flatnonzero(got.view(u) != want.view(u))
    assert len(d) == 0, (what, len(d), "of", len(got), "first at", d[:4], got[d[:4]], want[d[:4]])


def same_stats(got, G, what):
    frames, limited, min_gain = mdl.stats(G)
    assert (int(got.frames), int(got.limited)) == (frames, limited), (what, got, frames, limited, min_gain)
    assert np.float64(got.min_gain).view(np.uint64) == np.float64(min_gain).view(np.uint64), (what, got, min_gain)


# ---- 1. crafted rows through limit_rows ---------------------------------------------------------------------------------

def crafted_frames(rate):
    A, D, T = mdl.lookahead(rate), mdl.latency(rate), mdl.LIM_TILE
    return sorted({1, 2, 15, 16, 17, 31, 32, 33, D - 1, D, D + 1, 2 * A, 2 * A + 1, 4 * A + 31, 4 * A + 33, T - 1, T, T + 1, 2 * T + 3})


def crafted_values(rng, n_rows, frames, ch, case):
    """seeded noise with a NaN, both infinities, a -0.0 and a 3.0 planted (and at the row's two ends in turn); the last row
    zeros"""
    x = (rng.standard_normal((n_rows, frames * ch)) * 0.35).astype(np.float32)
    planted = [np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf), np.float32(-0.0), np.float32(3.0)]
    for r in range(n_rows):
        at = rng.permutation(frames * ch)[:len(planted)]
        for k, i in enumerate(at):
            x[r, i] = planted[(k + r + case) % len(planted)]
        if frames * ch > 8:
            x[r, -1] = planted[(case + r) % len(planted)]
            x[r, 0] = planted[(case + r + 1) % len(planted)]
    x[n_rows - 1] = 0.0
    return x


def _rows_case(torch, sa, b, taps, rng, rate, ch, frames, n_rows, case):
    g0, c = PARAMS[case % 2]
    win = sa.limiter_window(rate)
    x = crafted_values(rng, n_rows, frames, ch, case)
    pitch_el = (frames * ch * 4 + 15) // 16 * 4 + 4 * (1 + case % 3)  # larger than the row
    out_el = pitch_el + 4 * (case % 2)
    # what lies between the rows would reach the envelope of the last frames if a kernel read it
    t = torch.full((n_rows, pitch_el), 1e30, dtype=torch.float32, device="cuda")
    t[:, :frames * ch] = torch.from_numpy(x).to("cuda")
    o = torch.full((n_rows, out_el), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    st = b.limit_rows(t.data_ptr(), pitch_el * 4, n_rows, frames, ch, rate, g0, c, o.data_ptr(), out_el * 4)
    got = o.cpu().numpy().copy()
    o.fill_(7.0)
    torch.cuda.synchronize()
    st2 = b.limit_rows(t.data_ptr(), pitch_el * 4, n_rows, frames, ch, rate, g0, c, o.data_ptr(), out_el * 4)
    again = o.cpu().numpy()
    assert got.tobytes() == again.tobytes() and [bytes(s) for s in st] == [bytes(s) for s in st2], (rate, ch, frames, "called twice")
    assert (got[:, frames * ch:] == 7.0).all(), (rate, ch, frames, "a store beyond the rows' frames")
    assert len(st) == n_rows
    for r in range(n_rows):
        what = ("rate", rate, "ch", ch, "frames", frames, "row", r, "g0", g0, "c", c)
        y, G = mdl.limit(x[r].reshape(frames, ch), rate, g0, c, taps, win)
        same_bits(got[r, :frames * ch], y, what)
        same_stats(st[r], G, what)
        assert np.abs(got[r, :frames * ch]).max() <= np.float32(c)
    z = st[n_rows - 1]  # the row of zeros
    assert (z.frames, z.limited, z.min_gain) == (frames, 0, 1.0) and not got[n_rows - 1, :frames * ch].any()
    return st


def rows_main():
    """(in a process of its own, torch imported first: see test_rows)"""
    import torch
    import saugns_amd as sa
    from saugns_amd import voicebank as vb
    b = sa.Batch([vb.build_program([vb.Op("sin", freq=200.0, time_ms=10)])], 44100)  # (never run: its device is all that is used)
    taps = sa.truepeak_taps()
    rng = np.random.default_rng(20261019)
    cases, limited = 0, 0
    for rate in (3200, 8000):
        for ch in (1, 2):
            for frames in crafted_frames(rate):
                st = _rows_case(torch, sa, b, taps, rng, rate, ch, frames, 3, cases)
                limited += sum(int(s.limited) for s in st)
                cases += 1
    assert limited > 1000
    # the largest look-ahead: A = 1024, a halo of 4128 frames, more than the rows are long
    _rows_case(torch, sa, b, taps, rng, 204800, 2, 3 * 1024 + 5, 2, cases)
    # frames == 0: empty records; the refusals
    t = torch.zeros((2, 64), dtype=torch.float32, device="cuda")
    o = torch.zeros((2, 64), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for s in b.limit_rows(t.data_ptr(), 256, 2, 0, 2, 8000, 1.0, 0.5, o.data_ptr(), 256):
        assert (s.frames, s.limited, s.min_gain) == (0, 0, 1.0)
    host = np.zeros(1024, np.float32)
    hp = (host.ctypes.data + 15) & ~15
    ok = (t.data_ptr(), 256, 2, 8, 1, 8000, 1.0, 0.5, o.data_ptr(), 256)

    def but(**kw):
        names = ("ptr", "pitch", "n_rows", "frames", "channels", "srate", "pre_gain", "ceiling", "out_ptr", "out_pitch")
        a = dict(zip(names, ok))
        a.update(kw)
        return tuple(a[k] for k in names)

    bad = [but(ptr=t.view(-1)[1:].data_ptr()), but(pitch=260), but(out_ptr=o.view(-1)[1:].data_ptr()), but(out_pitch=260),
           but(channels=3), but(ptr=hp), but(out_ptr=hp), but(srate=0),
           but(out_ptr=t.data_ptr()), but(out_ptr=t.view(-1)[4:].data_ptr(), n_rows=1), but(out_ptr=t.view(-1)[64:].data_ptr()),
           but(pitch=16), but(pitch=1 << 20, n_rows=60000)]
    for v in (0.0, -1.0, math.nan, math.inf):
        bad += [but(pre_gain=v), but(ceiling=v)]
    for args in bad:
        try:
            b.limit_rows(*args)
        except RuntimeError as e:
            assert "bad argument" in str(e), (args, e)
        else:
            raise AssertionError(("not refused", args))
    assert not o.cpu().numpy().any()  # a refused call has written nothing
    b.limit_rows(*ok)  # (and the arguments they were varied from are good ones)
    b.close()
    print("limiter rows ok:", cases, "cases")


ROWS = r"""
import sys
import torch  # (before the library: torch's wheel brings a HIP runtime of its own, and a process has room for one -- api.Batch.device_tensor)
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_limiter
test_gpu_limiter.rows_main()
"""


def test_rows():
    """limit_rows on torch tensors at 3200 Hz (A = 16) and 8000 Hz (A = 40), mono and stereo, three rows: frame counts on both
    sides of the interpolator's reach, the delay, the hold, the history and the tile; seeded noise with a NaN, both infinities,
    a -0.0 and a 3.0 planted, the two ends included, a row of zeros, pitches larger than the rows with 1e30 between the input
    rows -- output rows and statistics equal the restatement bit for bit, and a call made twice gives identical bytes. One
    case at 204800 Hz (A = 1024) covers the largest halo. Then the refusals. In a process of its own: torch has to be imported
    before the library is loaded, and in this one the library is loaded already."""
    run = subprocess.run([sys.executable, "-c", ROWS, ROOT], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "limiter rows ok" in run.stdout, (run.stdout[-2000:], run.stderr[-4000:])


# ---- 2. a batch of two programs of unequal length, in one piece and in pieces ------------------------------------------

RATE = 8000


@pytest.fixture(autouse=True)
def forms(oracle):
    oracle.oracle().ora_set_fastmath_forms(ORACLE_FORMS)


def _programs():
    """two voices over the ceiling, of different lengths; the second is silent for its first 200 ms"""
    from saugns_amd import voicebank as vb
    one = vb.Op("sin", freq=440.0, amp=vb.Line(2.4, goal=0.3), time_ms=900, pan=-0.4)
    late = vb.Op("saw", freq=97.0, amp=vb.Line(0.1, goal=2.5), time_ms=500, pan=0.7)
    late.start_ms = 200
    return [vb.build_program([one]), vb.build_program([late])]


def _pieces(longest):
    A, D = mdl.lookahead(RATE), mdl.latency(RATE)
    runs = [1, 7, A, D, D + 1, mdl.LIM_TILE + 1, 2 * mdl.LIM_TILE - 1]
    while sum(runs) < longest + 3:  # the run that crosses the longest stream's end, then only tails
        runs.append(1777)
    return runs + [A, 1, D + 37]


def _limited(b, g0, c, runs, stereo):
    """limited runs of the given lengths -> per stream the fetched rows end to end, and the float runs' out_len summed"""
    ch = 2 if stereo else 1
    out, lens = [[] for _ in range(b.n)], [0] * b.n
    for n in runs:
        pcm, more, ln = b.run_limited(g0, c, n, stereo)
        assert pcm.shape == (b.n, n * ch)
        for s in range(b.n):
            out[s].append(pcm[s].copy())
            lens[s] += ln[s]
            assert more[s] or ln[s] <= n
    return [np.concatenate(o) for o in out], lens


@pytest.mark.parametrize("stereo", [False, True])
def test_a_batch_in_pieces_equals_itself_in_one_piece_and_the_restatement(sa, stereo):
    ch = 2 if stereo else 1
    g0, c = 1.0, 0.5
    taps, win = sa.truepeak_taps(), sa.limiter_window(RATE)
    D = mdl.latency(RATE)
    prgs = _programs()
    twin = sa.Batch(prgs, RATE)
    pcm, more, lens = twin.run_f32(3 * RATE, stereo)
    twin.close()
    assert not any(more) and len(set(lens)) == 2 and min(lens) > 4 * D
    x = [pcm[s, :lens[s] * ch].reshape(-1, ch).copy() for s in range(2)]
    assert not x[1][:RATE // 5 - 8].any() and np.abs(x[1]).max() > c and np.abs(x[0]).max() > c
    runs = _pieces(max(lens))
    total = sum(runs)
    assert total >= max(lens) + D  # every frame of every stream is delivered
    want = [mdl.limit_delayed(x[s], total, RATE, g0, c, taps, win) for s in range(2)]
    for what, rr in (("one piece", [total]), ("pieces", runs)):
        b = sa.Batch(prgs, RATE)
        fresh = b.limiter_stats()
        assert [(s.frames, s.limited, s.min_gain) for s in fresh] == [(0, 0, 1.0)] * 2
        rows, got_lens = _limited(b, g0, c, rr, stereo)
        assert got_lens == lens
        assert b.device_limited_f32(0) and b.device_limited_pitch() % 256 == 0 and b.device_limited_pitch() >= rr[-1] * ch * 4
        st = b.limiter_stats(reset=True)
        for s in range(2):
            same_bits(rows[s], want[s][0], (what, "stream", s))
            same_stats(st[s], want[s][1], (what, "stream", s))
            assert st[s].limited > 0 and np.abs(rows[s]).max() <= np.float32(c)
            assert not rows[s][(D + lens[s] + D) * ch:].any()  # behind the tail: silence
        assert [(s.frames, s.limited, s.min_gain) for s in b.limiter_stats()] == [(0, 0, 1.0)] * 2  # after the reset
        b.close()


def test_another_ceiling_starts_from_zero_history(sa):
    taps, win = sa.truepeak_taps(), sa.limiter_window(RATE)
    prgs = _programs()
    twin = sa.Batch(prgs, RATE)
    pcm, _, lens = twin.run_f32(3 * RATE, False)
    twin.close()
    n1, n2 = 1500, 2000
    b = sa.Batch(prgs, RATE)
    first, _ = _limited(b, 1.0, 0.5, [1000, n1 - 1000], False)
    second, _ = _limited(b, 1.0, 0.25, [700, n2 - 700], False)
    b.close()
    for s in range(2):
        x = pcm[s, :lens[s]]
        same_bits(first[s], mdl.limit_delayed(x, n1, RATE, 1.0, 0.5, taps, win)[0], ("first ceiling", s))
        same_bits(second[s], mdl.limit_delayed(x[n1:], n2, RATE, 1.0, 0.25, taps, win)[0], ("second ceiling", s))


def test_a_limited_run_is_refused_while_loudness_is_on_and_the_batch_stands(sa):
    prgs = _programs()
    twin = sa.Batch(prgs, RATE)
    want = twin.run_f32(2500, True)[0]
    twin.close()
    b = sa.Batch(prgs, RATE)
    first = b.run_f32(1000, True)[0]
    b.set_loudness(True)
    for fetch in (True, False):
        with pytest.raises(RuntimeError, match="bad argument"):
            b.run_limited(1.0, 0.5, 300, True, fetch=fetch)
    for g0, c in ((0.0, 0.5), (1.0, math.nan), (math.inf, 0.5), (1.0, -1.0)):
        with pytest.raises(RuntimeError, match="bad argument"):
            b.run_limited(g0, c, 300, True)
    rest = b.run_f32(1500, True)[0]  # continues at frame 1000
    assert b.loudness()[0].frames == 1500  # (metering went on at frame 1000; the refused runs have added nothing)
    b.close()
    assert np.concatenate([first, rest], axis=1).tobytes() == want.tobytes()


# ---- 3. the writer ---------------------------------------------------------------------------------------------------------

HEADER = {0: 0, 1: 28, 2: 44, 3: 58}  # RAW, AU, WAV, WAV_F32
FILE_KEY = "devtests__voice-reuse"


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
def test_limited_loudness_files(sa, tmp_path, channels):
    prg = load_program(sa, FILE_KEY)
    x, ld = _float_render(sa, prg, RATE, channels == 2)
    frames = len(x) // channels
    assert ld.frames == frames and ld.integrated > -70.0
    tp = float(max(ld.true_peak))
    # 9 dB up under a ceiling of the true peak as it stands: the ceiling binds, and the gain is not lowered for it
    target, ceiling = ld.integrated + 9.0, tp
    gain = np.float32(10.0 ** ((target - ld.integrated) / 20.0))
    assert np.float32(tp) * gain > np.float32(ceiling)
    taps, win = sa.truepeak_taps(), sa.limiter_window(RATE)
    y, G = mdl.limit(x.reshape(frames, channels), RATE, gain, ceiling, taps, win)
    y = y.reshape(-1)
    assert (G < 1.0).any()
    plain = sa.render_file(prg, RATE, str(tmp_path / "plain.wav"), 2, channels)
    for fmt, dtype, want in ((2, "<i2", mdl.pcm16(y)), (1, ">i2", mdl.pcm16(y)), (3, "<f4", y)):
        path = str(tmp_path / ("t%d" % fmt))
        n, got, g, st = sa.render_file_loudness_limited(prg, RATE, path, fmt, channels, target, ceiling)
        assert n == frames == plain and bytes(got) == bytes(ld)
        assert np.float32(g).view(np.uint32) == gain.view(np.uint32), (g, gain)
        assert st.limited > 0 and st.min_gain < 1.0 and st.frames >= frames + mdl.latency(RATE)
        data = np.frombuffer(open(path, "rb").read(), dtype, offset=HEADER[fmt])
        assert len(data) == frames * channels
        same_bits(data.astype(dtype[1:]), want, ("format", fmt))
        if fmt == 3:
            assert np.abs(data).max() <= np.float32(ceiling)
