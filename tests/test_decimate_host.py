"""Oversampled rendering without a GPU (include/saugns_amd.h: sauAmd_decimator_taps, sauAmd_decimator_latency,
sauAmd_Batch_run_decimated_f32, sauAmd_render_file_oversampled): the filter's taps against the header's formula built again
in numpy and against its stated response, and the refusals -- the sequential test executor (tests/seqexec) keeps engine.h's
default bodies of the decimation calls, which refuse with a text; a refusal renders nothing, and the file writer's refusals
come before a file exists."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ORACLE_FORMS, ROOT, load_program, max_diff

KEY = "devtests__voice-reuse"
H = 32
BETA = 10.06


@pytest.fixture(scope="module")
def oversample_hooks(sa, hooks):
    """tests/hooks_oversample/libsaugns_amd_oversample_hooks.so: the product's object files (the `hooks` fixture has built
    them) + the oversampled writer over an injected backend"""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "hooks_oversample")])
    return sa.api.use_oversample_hooks(os.path.join(ROOT, "tests", "hooks_oversample", "libsaugns_amd_oversample_hooks.so"))


def i0(x):
    """the power series, until a term no longer changes the sum"""
    total, term, k = 1.0, 1.0, 1
    while True:
        term *= (x * x / 4.0) / (k * k)
        if total + term == total:
            return total
        total += term
        k += 1


def numpy_taps(K):
    C, L = H * K, 2 * H * K + 1
    n = np.arange(C + 1, dtype=np.float64)
    t = (n - C) / K
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = np.where(t == 0.0, 1.0, np.sin(np.pi * t) / (np.pi * t))
    w = np.array([i0(BETA * np.sqrt(max(0.0, 1.0 - ((k - C) / C) ** 2))) for k in range(C + 1)]) / i0(BETA)
    g = np.zeros(L)
    g[:C + 1] = sinc * w
    g[C + 1:] = g[:C][::-1]
    S = 0.0
    for v in g:  # ascending n
        S += v
    return g / S


@pytest.mark.parametrize("K", [2, 4, 8])
def test_the_taps_are_the_headers_formula(sa, K):
    h = sa.decimator_taps(K)
    L = 2 * H * K + 1
    assert h.dtype == np.float64 and len(h) == L
    assert sa.decimator_latency(K) == H
    want = numpy_taps(K)
    assert np.abs(h - want).max() <= 1e-13
    assert (h == h[::-1]).all()  # exactly symmetric
    assert abs(float(np.sum(h)) - 1.0) <= 1e-14
    # the response: the filter runs at K times the output rate fs_out, so f / fs_out = bin * K / N
    N = 1 << 18
    gain = np.abs(np.fft.rfft(h, N))
    f = np.arange(len(gain)) * K / N  # in units of fs_out
    with np.errstate(divide="ignore"):
        db = 20.0 * np.log10(gain)
    assert np.abs(db[f <= 0.45]).max() <= 2e-4
    assert db[f >= 0.55].max() <= -98.0


def test_the_taps_call_writes_nothing_into_a_short_buffer(sa):
    import ctypes as C
    L = sa.lib()
    buf = np.full(600, 7.0)
    p = buf.ctypes.data_as(C.POINTER(C.c_double))
    assert L.sauAmd_decimator_taps(4, p, 256) == 257 and (buf == 7.0).all()
    assert L.sauAmd_decimator_taps(4, p, 257) == 257 and (buf[:257] != 7.0).all() and (buf[257:] == 7.0).all()


@pytest.mark.parametrize("K", [0, 1, 3, 16, -2])
def test_other_factors_have_no_filter(sa, K):
    assert len(sa.decimator_taps(K)) == 0
    assert sa.decimator_latency(K) == 0


def test_a_decimated_run_is_refused_and_the_int16_render_after_it_starts_at_frame_0(sa, oracle, seqexec):
    oracle.oracle().ora_set_fastmath_forms(ORACLE_FORMS)
    prg = load_program(sa, KEY)
    want = oracle.oracle_render(prg.ptr, 12000, True, chunk=5000)
    b = sa.Batch([prg], 12000, backend=seqexec.seq_backend_create(1016))
    for fetch in (True, False):
        with pytest.raises(RuntimeError, match="this backend has no decimator"):
            b.run_decimated(4, 1000, stereo=True, fetch=fetch)
    assert "this backend has no decimator" in sa.api.last_error()
    for K in (0, 3, 16):  # a bad factor is a bad argument whatever the backend
        with pytest.raises(RuntimeError, match="bad argument"):
            b.run_decimated(K, 1000)
    with pytest.raises(RuntimeError, match="bad argument"):
        b.run_decimated(8, 1 << 29)  # buf_len * factor beyond 32 bits
    assert not b.device_decimated_f32(0) and b.device_decimated_pitch() == 0
    got = b.render(stereo=True, chunk=5000)[0]
    b.close()
    assert max_diff(got, want) == 0


@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
def test_the_oversampled_writer_over_a_backend_without_a_decimator_makes_no_file(sa, seqexec, oversample_hooks, tmp_path, fmt):
    prg = load_program(sa, KEY)
    path = str(tmp_path / "over.out")
    with pytest.raises(RuntimeError, match="this backend has no"):
        sa.render_file_oversampled(prg, 6000, 4, path, fmt, 2, backend=seqexec.seq_backend_create(1016))
    assert "this backend has no" in sa.api.last_error()
    assert not os.path.exists(path)


@pytest.mark.parametrize("factor,fmt,channels", [(0, 2, 1), (1, 2, 1), (3, 2, 1), (16, 2, 1), (4, 4, 1), (4, -1, 1), (4, 2, 0), (4, 2, 3)])
def test_a_bad_factor_format_or_channel_count_makes_no_file(sa, seqexec, oversample_hooks, tmp_path, factor, fmt, channels):
    prg = load_program(sa, KEY)
    path = str(tmp_path / "over.wav")
    # over the executor, and through the product's own entry point: the arguments are looked at before any backend is made,
    # so this is the same refusal with and without a GPU
    with pytest.raises(RuntimeError, match="bad argument"):
        sa.render_file_oversampled(prg, 6000, factor, path, fmt, channels, backend=seqexec.seq_backend_create(1016))
    assert not os.path.exists(path)
    with pytest.raises(RuntimeError, match="bad argument"):
        sa.render_file_oversampled(prg, 6000, factor, path, fmt, channels)
    assert "bad argument" in sa.api.last_error()
    assert not os.path.exists(path)


def test_plan_decimate_constants_are_what_the_gpu_tests_mirror():
    """tests/test_gpu_decimate.py names the tile of launch_plan.h's plan_decimate (output frames per workgroup) to put a run
    past it and off its multiples: it is read here from the header it comes from."""
    hdr = open(os.path.join(ROOT, "saugns_amd", "csrc", "launch_plan.h")).read()
    assert re.search(r"DECIM_THREADS = 64, DECIM_PER_LANE = 4;", hdr)
    assert re.search(r"DECIM_TILE = 256;", hdr)
    import test_gpu_decimate as g
    assert g.DECIM_TILE == 256 and g.DECIM_TILE < 300 and 300 % g.DECIM_TILE != 0
    # tests/test_gpu_decimate_rows.py sizes its runs by the tile, by the history (2 * DECIM_HALF output frames) and by the
    # carry kernel's reach (four floats a thread): the same header, and engine.h for the half-length
    assert re.search(r"DECIM_CARRY_THREADS = 256;", hdr)
    assert re.search(r"DECIM_HALF = \(uint32_t\)sauengine::DECIM_HALF;", hdr)
    eng = open(os.path.join(ROOT, "saugns_amd", "csrc", "engine.h")).read()
    assert re.search(r"constexpr size_t DECIM_HALF = 32;", eng)
    import test_gpu_decimate_rows as r
    assert (r.DECIM_TILE, r.DECIM_HALF, r.DECIM_CARRY_THREADS) == (256, 32, 256) and r.H == g.H == H == r.DECIM_HALF
    assert 2 * r.DECIM_HALF * 8 * 2 == 4 * r.DECIM_CARRY_THREADS  # K = 8 stereo fills the carry kernel to its last thread
    for n in (r.DECIM_TILE - 1, r.DECIM_TILE, r.DECIM_TILE + 1, 2 * r.DECIM_TILE, 2 * r.DECIM_HALF - 1, 2 * r.DECIM_HALF, 2 * r.DECIM_HALF + 1):
        assert n in r.RUNS
