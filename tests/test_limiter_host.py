"""The look-ahead true-peak limiter without a GPU (include/saugns_amd.h, section "Limiter": sauAmd_limiter_window,
sauAmd_limiter_latency, sauAmd_Batch_run_limited_f32, sauAmd_Batch_limit_rows, sauAmd_render_file_loudness_limited): the
smoothing window and the constants against the header's formulas, the refusals over the sequential test executor
(tests/seqexec keeps engine.h's refusing defaults) -- the writer's before a file exists -- and the properties the header
states of the arithmetic, checked on its Python restatement (tests/limiter_model.py), which tests/test_gpu_limiter.py
compares with the device bit for bit."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import limiter_model as mdl
import loudness_model as lm
from conftest import ORACLE_FORMS, ROOT, load_program, max_diff

KEY = "devtests__voice-reuse"


@pytest.fixture(scope="module")
def limiter_hooks(sa, hooks):
    """tests/hooks_limiter/libsaugns_amd_limiter_hooks.so: the product's object files (the `hooks` fixture has built them) +
    the limited writer over an injected backend"""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "hooks_limiter")])
    return sa.api.use_limiter_hooks(os.path.join(ROOT, "tests", "hooks_limiter", "libsaugns_amd_limiter_hooks.so"))


def test_the_statistics_structure_is_24_bytes(sa):
    S = sa.api.LimiterStats
    assert C.sizeof(S) == 24
    assert [getattr(S, f).offset for f in ("frames", "limited", "min_gain")] == [0, 8, 16]


def test_the_constants_the_model_mirrors_are_the_headers():
    hdr = open(os.path.join(ROOT, "saugns_amd", "csrc", "launch_plan.h")).read()
    eng = open(os.path.join(ROOT, "saugns_amd", "csrc", "engine.h")).read()
    assert re.search(r"LIM_A_MIN = 16, LIM_A_MAX = 1024;", eng)
    assert re.search(r"LIM_THREADS = 256, LIM_PER_LANE = 2, LIM_TILE = LIM_THREADS \* LIM_PER_LANE;", hdr)
    assert re.search(r"LIM_ENV_TILE = LIM_THREADS;", hdr)
    assert (mdl.LIM_A_MIN, mdl.LIM_A_MAX, mdl.LIM_THREADS, mdl.LIM_PER_LANE, mdl.LIM_TILE, mdl.LIM_ENV_TILE) == (16, 1024, 256, 2, 512, 256)


RATES = [(1, 16), (3199, 16), (3200, 16), (8000, 40), (44100, 220), (204800, 1024), (4294967295, 1024)]


@pytest.mark.parametrize("fs,A", RATES)
def test_lookahead_and_delay(sa, fs, A):
    assert mdl.lookahead(fs) == A and mdl.latency(fs) == 2 * A + 16
    assert sa.limiter_latency(fs) == 2 * A + 16
    assert sa.lib().sauAmd_limiter_window(fs, None, 0) == 2 * A + 1


def test_rate_0_has_no_limiter(sa):
    assert sa.limiter_latency(0) == 0 and len(sa.limiter_window(0)) == 0


@pytest.mark.parametrize("fs", [3200, 8000, 44100, 204800])
def test_the_window_matches_the_formula(sa, fs):
    h = sa.limiter_window(fs)
    A = mdl.lookahead(fs)
    assert len(h) == 2 * A + 1
    assert np.abs(h - mdl.window_formula(fs)).max() <= 1e-15
    assert (h == h[::-1]).all()  # exactly symmetric
    S = 0.0
    for v in h.tolist():
        S += v
    assert abs(S - 1.0) <= 1e-14
    assert (h > 0).all() and h.argmax() == A


def test_the_window_call_writes_nothing_into_a_short_buffer(sa):
    L = sa.lib()
    buf = np.full(100, 7.0)
    p = buf.ctypes.data_as(C.POINTER(C.c_double))
    assert L.sauAmd_limiter_window(8000, p, 80) == 81 and (buf == 7.0).all()
    assert L.sauAmd_limiter_window(8000, p, 81) == 81 and (buf[:81] != 7.0).all() and (buf[81:] == 7.0).all()


# ---- refusals over the sequential executor ---------------------------------------------------------------------------

def test_limited_runs_are_refused_and_the_int16_render_after_them_starts_at_frame_0(sa, oracle, seqexec):
    oracle.oracle().ora_set_fastmath_forms(ORACLE_FORMS)
    prg = load_program(sa, KEY)
    want = oracle.oracle_render(prg.ptr, 12000, True, chunk=5000)
    b = sa.Batch([prg], 12000, backend=seqexec.seq_backend_create(1016))
    for fetch in (True, False):
        with pytest.raises(RuntimeError, match="this backend has no limiter"):
            b.run_limited(1.0, 0.5, 1000, stereo=True, fetch=fetch)
    assert "this backend has no limiter" in sa.api.last_error()
    for g0, c in ((0.0, 0.5), (-1.0, 0.5), (math.nan, 0.5), (math.inf, 0.5), (1.0, 0.0), (1.0, -1.0), (1.0, math.nan), (1.0, math.inf)):
        with pytest.raises(RuntimeError, match="bad argument"):  # whatever the backend
            b.run_limited(g0, c, 1000)
    rows = np.zeros(256, np.float32)  # (host memory: the refusal comes before anything reads it)
    p = (rows.ctypes.data + 15) & ~15
    with pytest.raises(RuntimeError, match="this backend has no limiter"):
        b.limit_rows(p, 64, 1, 8, 1, 8000, 1.0, 0.5, p + 512, 64)
    for args in ((p + 4, 64, 1, 8, 1, 8000, 1.0, 0.5, p + 512, 64), (p, 68, 1, 8, 1, 8000, 1.0, 0.5, p + 512, 64),
                 (p, 64, 1, 8, 3, 8000, 1.0, 0.5, p + 512, 64), (p, 64, 1, 8, 1, 0, 1.0, 0.5, p + 512, 64),
                 (p, 64, 1, 8, 1, 8000, 0.0, 0.5, p + 512, 64), (p, 64, 1, 8, 1, 8000, 1.0, math.nan, p + 512, 64),
                 (p, 64, 1, 8, 1, 8000, 1.0, 0.5, p + 516, 64), (p, 64, 1, 8, 1, 8000, 1.0, 0.5, p + 512, 72)):
        with pytest.raises(RuntimeError, match="bad argument"):
            b.limit_rows(*args)
    st = b.limiter_stats()  # no limited sequence has begun: empty records, and no backend asked
    assert len(st) == 1 and (st[0].frames, st[0].limited, st[0].min_gain) == (0, 0, 1.0)
    assert not b.device_limited_f32(0) and b.device_limited_pitch() == 0
    got = b.render(stereo=True, chunk=5000)[0]  # every refused call has rendered nothing
    b.close()
    assert max_diff(got, want) == 0


@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
def test_the_limited_writer_over_a_backend_without_it_makes_no_file(sa, seqexec, limiter_hooks, tmp_path, fmt):
    prg = load_program(sa, KEY)
    path = str(tmp_path / "lim.out")
    with pytest.raises(RuntimeError, match="this backend has no"):
        sa.render_file_loudness_limited(prg, 12000, path, fmt, 2, -23.0, 1.0, backend=seqexec.seq_backend_create(1016))
    assert "this backend has no" in sa.api.last_error()
    assert not os.path.exists(path)


BAD = [(math.nan, 1.0, 12000), (math.inf, 1.0, 12000), (-math.inf, 1.0, 12000), (-23.0, 0.0, 12000), (-23.0, -1.0, 12000),
       (-23.0, math.nan, 12000), (-23.0, math.inf, 12000), (-23.0, 1.0, 2559)]


@pytest.mark.parametrize("target,ceiling,srate", BAD)
def test_the_limited_writers_bad_arguments_make_no_file(sa, seqexec, limiter_hooks, tmp_path, target, ceiling, srate):
    prg = load_program(sa, KEY)
    path = str(tmp_path / "lim.wav")
    # over the executor, and through the product's own entry point: the arguments are looked at before any backend is made,
    # so this is the same refusal with and without a GPU
    with pytest.raises(RuntimeError, match="bad argument"):
        sa.render_file_loudness_limited(prg, srate, path, sa.api.SNDFILE_WAV, 1, target, ceiling, backend=seqexec.seq_backend_create(1016))
    assert not os.path.exists(path)
    with pytest.raises(RuntimeError, match="bad argument"):
        sa.render_file_loudness_limited(prg, srate, path, sa.api.SNDFILE_WAV, 1, target, ceiling)
    assert "bad argument" in sa.api.last_error()
    assert not os.path.exists(path)
    for fmt, channels in ((4, 1), (-1, 1), (2, 0), (2, 3)):
        with pytest.raises(RuntimeError, match="bad argument"):
            sa.render_file_loudness_limited(prg, 12000, path, fmt, channels, -23.0, 1.0)
        assert not os.path.exists(path)


# ---- the properties the header states, on the restatement ------------------------------------------------------------

N = 3000
SIGNALS = ["noise", "quarter-rate sine", "50 Hz sine", "burst"]
PARAMS = [(2.0, 0.8912509), (1.0, 0.5)]
# The true peak of the limited output against the ceiling, in dB: not bounded by the arithmetic (a gain that varies in time
# moves the peaks between the samples). Measured with this test's twenty-four cases (DESIGN.md 4.4 has the table); the bound
# is the issue's: five times the worst value a prototype of this arithmetic gave on the twelve mono cases, because such cases
# are a sample and not a bound.
TRUE_PEAK_GAP_DB = 0.05


def signal(name, fs, ch):
    t = np.arange(N)
    if name == "noise":
        x = np.random.default_rng(fs).standard_normal((N, ch)) * 0.4
    elif name == "quarter-rate sine":
        x = np.sin(2.0 * math.pi * t / 4.0 + math.pi / 4.0)
        ramp = 0.5 - 0.5 * np.cos(math.pi * (np.arange(256) + 0.5) / 256.0)
        x[:256] *= ramp
        x[-256:] *= ramp[::-1]
        x = np.repeat(x[:, None], ch, axis=1) * ([1.0, 0.5][:ch])
    elif name == "50 Hz sine":
        x = np.repeat(np.sin(2.0 * math.pi * 50.0 * t / fs)[:, None], ch, axis=1) * ([0.9, -0.7][:ch])
    else:  # a 40-frame burst, 20 times over a quiet tone
        x = 0.05 * np.sin(2.0 * math.pi * t / 16.0)
        x[1500:1540] *= 20.0
        x = np.repeat(x[:, None], ch, axis=1)
    return x.astype(np.float32)


@pytest.mark.parametrize("g0,c", PARAMS)
@pytest.mark.parametrize("name", SIGNALS)
@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("fs", [3200, 8000, 44100])
def test_the_restatement_has_the_headers_properties(sa, fs, ch, name, g0, c):
    x = signal(name, fs, ch)
    taps, win = sa.truepeak_taps(), sa.limiter_window(fs)
    y, G = mdl.limit(x, fs, g0, c, taps, win)
    c32, g32 = np.float32(c), np.float32(g0)
    assert y.dtype == np.float32 and y.shape == x.shape and (G > 0).all() and (G <= 1.0).all()
    assert np.abs(y).max() <= c32  # exactly: no sample passes the ceiling
    assert (G < 1.0).any(), "the case does not reach the ceiling"
    same = G == 1.0  # untouched passages: the pre-gain alone, rounded once
    want = (x.astype(np.float64) * float(g32)).astype(np.float32)
    assert (y[same].view(np.uint32) == want[same].view(np.uint32)).all()
    if g0 == 1.0:
        assert (y[same].view(np.uint32) == x[same].view(np.uint32)).all()
    # the true peak of the output against the ceiling
    m = lm.Meter(sa.loudness_filter(fs), taps, fs // 10, ch)
    m.run(y)
    tp = float(max(m.true_peak()))
    gap = 20.0 * math.log10(tp / float(c32))
    print("true peak over the ceiling: %d Hz, %d ch, %s, g0 %g, c %g: %+.5f dB, min gain %.4f (%.1f dB)"
          % (fs, ch, name, g0, c, gap, G.min(), 20.0 * math.log10(G.min())))
    assert gap <= TRUE_PEAK_GAP_DB, (fs, ch, name, g0, c, gap)


def test_cutting_the_sequence_does_not_change_the_restatements_delayed_form(sa):
    """limit_delayed, what a sequence of runs delivers, is the time-aligned form shifted by D -- the identity the GPU tests
    lean on when they compare a batch's rows with the model"""
    fs, g0, c = 8000, 2.0, 0.5
    x = signal("noise", fs, 2)[:700]
    taps, win = sa.truepeak_taps(), sa.limiter_window(fs)
    D = mdl.latency(fs)
    y, G = mdl.limit(x, fs, g0, c, taps, win)
    for total in (D + 700, D + 300, 50):
        row, Gd = mdl.limit_delayed(x, total, fs, g0, c, taps, win)
        assert len(row) == total and not row[:min(D, total)].any()
        m = max(total - D, 0)
        assert row[D:].tobytes() == y[:m].tobytes() and Gd[D:].tobytes() == G[:m].tobytes()
