"""The spectrum meter without a GPU (include/saugns_amd.h, section "Spectrum": sauAmd_spectrum_window, sauAmd_spectrum_twiddles,
sauAmd_Batch_create_spectrum, sauAmd_Batch_spectrum_rows, sauAmd_render_spectrum): the tables against the header's formulas,
the library's host restatement of one segment (tables.cpp: spectrum_segment) against the numpy restatement
(tests/spectrum_model.py) bit for bit, the restatement itself against numpy.fft, the refusals over the sequential test
executor (tests/seqexec keeps engine.h's refusing defaults) and those that need no device, and the launch plan of a feed
(launch_plan.h: plan_spectrum_row, plan_spectrum). tests/test_gpu_spectrum.py compares the device with the restatement."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import spectrum_model as mdl
from conftest import ORACLE_FORMS, ROOT, load_program, max_diff

KEY = "devtests__voice-reuse"


@pytest.fixture(scope="module")
def spectrum_hooks(sa, hooks):
    """tests/hooks_spectrum/libsaugns_amd_spectrum_hooks.so: the product's object files (the `hooks` fixture has built them) +
    the spectrum writer over an injected backend, the host's one segment, the launch plan"""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "hooks_spectrum")])
    return sa.api.use_spectrum_hooks(os.path.join(ROOT, "tests", "hooks_spectrum", "libsaugns_amd_spectrum_hooks.so"))


# ---- tables ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", [8, 9, 10, 11, 12])
def test_the_tables_match_the_formulas(sa, L):
    """within 2^-52 absolute: libm's cos and sin are good to one unit in the last place and every value is at most 1"""
    N = 1 << L
    w, tw = sa.spectrum_window(L), sa.spectrum_twiddles(L)
    assert w.shape == (N,) and tw.shape == (N // 2, 2) and w.dtype == tw.dtype == np.float64
    assert w[0] == 0.0
    want_w = np.array([0.5 - 0.5 * math.cos(2.0 * math.pi * j / N) for j in range(N)])
    want_c = np.array([math.cos(2.0 * math.pi * k / N) for k in range(N // 2)])
    want_d = np.array([-math.sin(2.0 * math.pi * k / N) for k in range(N // 2)])
    assert np.abs(w - want_w).max() <= 2.0 ** -52
    assert np.abs(tw[:, 0] - want_c).max() <= 2.0 ** -52 and np.abs(tw[:, 1] - want_d).max() <= 2.0 ** -52
    assert tw[0, 0] == 1.0 and tw[0, 1] == 0.0


@pytest.mark.parametrize("L", [7, 13, 0])
def test_other_sizes_have_no_tables(sa, L):
    lib = sa.lib()
    assert lib.sauAmd_spectrum_window(L, None, 0) == 0 and lib.sauAmd_spectrum_twiddles(L, None, 0) == 0
    assert len(sa.spectrum_window(L)) == 0 and len(sa.spectrum_twiddles(L)) == 0


def test_the_table_calls_write_nothing_into_a_short_buffer(sa):
    lib = sa.lib()
    for call in (lib.sauAmd_spectrum_window, lib.sauAmd_spectrum_twiddles):
        buf = np.full(300, 7.0)
        p = buf.ctypes.data_as(C.POINTER(C.c_double))
        assert call(8, p, 255) == 256 and (buf == 7.0).all()
        assert call(8, p, 256) == 256 and (buf[1:256] != 7.0).all() and (buf[256:] == 7.0).all()


# ---- one segment: the library's host code and the restatement -------------------------------------------------------------

def crafted(rng, n, scale=0.5):
    """seeded noise with a NaN, both infinities and a -0.0 planted"""
    x = (rng.standard_normal(n) * scale).astype(np.float32)
    at = rng.permutation(n)[:4]
    x[at[0]], x[at[1]], x[at[2]], x[at[3]] = np.nan, np.inf, -np.inf, -0.0
    return x


@pytest.mark.parametrize("L", [8, 9, 12])
@pytest.mark.parametrize("stride", [1, 2])
def test_the_hosts_segment_equals_the_restatement_bit_for_bit(sa, spectrum_hooks, L, stride):
    N = 1 << L
    w, tw = sa.spectrum_window(L), sa.spectrum_twiddles(L)
    x = crafted(np.random.default_rng(1000 + L), N * stride)
    got = np.full(N // 2 + 2, 7.0)
    assert spectrum_hooks.sauAmd_spectrum_segment(L, x.ctypes.data, stride, got.ctypes.data_as(C.POINTER(C.c_double)))
    want = mdl.segment_power(mdl.clean(x[::stride]), w, tw, L)
    assert got[-1] == 7.0 and got[:-1].tobytes() == want.tobytes()
    assert want.max() > 1.0 and np.isfinite(want).all()
    assert not spectrum_hooks.sauAmd_spectrum_segment(7, x.ctypes.data, stride, got.ctypes.data_as(C.POINTER(C.c_double)))


@pytest.mark.parametrize("L", [8, 9, 10, 11, 12])
def test_the_restatement_is_a_power_spectrum(sa, L):
    """The restatement is the yardstick of the GPU tests, so it is held against numpy.fft.rfft of w * x in f64 here:
    max_k |p[k] - q[k]| <= 8 L 2^-53 sum_k q[k] (a radix-2 transform's rounding error grows as L u). Measured with this
    test's input, max_k |p - q| in units of 2^-53 sum_k q: L = 8: 0.168, L = 9: 0.062, L = 10: 0.061, L = 11: 0.030,
    L = 12: 0.021 (in units of 2^-53 of the largest bin alone: 3.82, 2.63, 4.86, 3.53, 6.21) -- the bound of 8 L has more than
    a hundredfold margin."""
    N = 1 << L
    w, tw = sa.spectrum_window(L), sa.spectrum_twiddles(L)
    x = (np.random.default_rng(L).standard_normal(N) * 0.5).astype(np.float32)
    p = mdl.segment_power(x, w, tw, L)
    q = np.abs(np.fft.rfft(w * x.astype(np.float64))) ** 2
    dev = float(np.abs(p - q).max())
    print("L = %d: max |p - q| = %.3f x 2^-53 sum q = %.2f x 2^-53 max q" % (L, dev / (2.0 ** -53 * q.sum()), dev / (2.0 ** -53 * q.max())))
    assert dev <= 8 * L * 2.0 ** -53 * q.sum()


def test_the_restatement_does_not_depend_on_the_feeds(sa):
    L, hop, ch = 8, 100, 2
    w, tw = sa.spectrum_window(L), sa.spectrum_twiddles(L)
    x = crafted(np.random.default_rng(5), 5003 * ch).reshape(-1, ch)
    whole, S, gram = mdl.measure(x, w, tw, L, hop, ch)
    assert S == mdl.segments(5003, 256, hop) == 48 and gram.shape == (ch, S, 129)
    m = mdl.Meter(w, tw, L, hop, ch)
    at = 0
    for n in [1, 7, 99, 100, 101, 255, 256, 257, 1600, 0, 3, 2324]:
        before = m.read()
        assert before[0].tobytes() == m.read()[0].tobytes()  # a read changes nothing
        m.feed(x[at:at + n])
        at += n
    assert at == len(x)
    p, S2 = m.read()
    assert S2 == S and p.tobytes() == whole.tobytes()
    # 48 segments are three complete groups: the total alone; one frame less than the 49th segment needs changes nothing
    one, S3, _ = mdl.measure(x[:256 + 47 * hop], w, tw, L, hop, ch)
    assert S3 == 48 and one.tobytes() == whole.tobytes()


# ---- refusals over the sequential executor ---------------------------------------------------------------------------

def test_a_meter_is_refused_and_the_render_after_it_starts_at_frame_0(sa, oracle, seqexec):
    oracle.oracle().ora_set_fastmath_forms(ORACLE_FORMS)
    prg = load_program(sa, KEY)
    want = oracle.oracle_render(prg.ptr, 12000, True, chunk=5000)
    b = sa.Batch([prg], 12000, backend=seqexec.seq_backend_create(1016))
    with pytest.raises(RuntimeError, match="this backend has no spectrum meter"):
        b.create_spectrum(1, 2, 9, 256)
    assert "this backend has no spectrum meter" in sa.api.last_error()
    for n_rows, ch, L, hop in ((0, 1, 9, 256), (1, 0, 9, 256), (1, 3, 9, 256), (1, 1, 7, 64), (1, 1, 13, 4096), (1, 1, 9, 0), (1, 1, 9, 63),
                               (1, 1, 9, 513)):
        with pytest.raises(RuntimeError, match="bad argument"):  # whatever the backend
            b.create_spectrum(n_rows, ch, L, hop)
    rows = np.zeros(2048, np.float32)  # (host memory: the refusal comes before anything reads it)
    p = (rows.ctypes.data + 15) & ~15
    with pytest.raises(RuntimeError, match="this backend has no spectrum meter"):
        b.spectrum_rows(p, 4096, 1, 600, 1, 9, 256)
    for args in ((p + 4, 4096, 1, 600, 1, 9, 256), (p, 4100, 1, 600, 1, 9, 256), (p, 4096, 0, 600, 1, 9, 256), (p, 4096, 1, 600, 3, 9, 256),
                 (p, 4096, 1, 600, 1, 7, 64), (p, 4096, 1, 600, 1, 9, 63), (0, 4096, 1, 600, 1, 9, 256)):
        with pytest.raises(RuntimeError, match="bad argument"):
            b.spectrum_rows(*args)
    got = b.render(stereo=True, chunk=5000)[0]  # every refused call has rendered nothing
    b.close()
    assert max_diff(got, want) == 0


@pytest.mark.parametrize("factor", [1, 2])
def test_render_spectrum_over_a_backend_without_it_is_refused(sa, seqexec, spectrum_hooks, factor):
    prg = load_program(sa, KEY)
    with pytest.raises(RuntimeError, match="this backend has no"):
        sa.render_spectrum(prg, 12000, factor, 2, 9, 256, backend=seqexec.seq_backend_create(1016))
    assert "this backend has no" in sa.api.last_error()


# ---- refusals that need no device ------------------------------------------------------------------------------------------

BAD = [dict(log2n=7, hop=64), dict(log2n=13, hop=4096), dict(hop=0), dict(hop=512 // 8 - 1), dict(hop=512 + 1), dict(channels=3),
       dict(channels=0), dict(factor=3), dict(factor=0), dict(factor=-2), dict(srate=0), dict(srate=1 << 31, factor=2)]


@pytest.mark.parametrize("bad", BAD, ids=[",".join("%s=%s" % kv for kv in b.items()) for b in BAD])
def test_render_spectrum_refuses_bad_arguments_before_it_touches_a_device(sa, seqexec, spectrum_hooks, bad):
    """through the product's own entry point the arguments are looked at before any backend is made, so this is the same
    refusal with and without a GPU; over the executor likewise"""
    prg = load_program(sa, KEY)
    a = dict(srate=8000, factor=1, channels=1, log2n=9, hop=256)
    a.update(bad)
    with pytest.raises(RuntimeError, match="bad argument"):
        sa.render_spectrum(prg, a["srate"], a["factor"], a["channels"], a["log2n"], a["hop"])
    assert "bad argument" in sa.api.last_error()
    with pytest.raises(RuntimeError, match="bad argument"):
        sa.render_spectrum(prg, a["srate"], a["factor"], a["channels"], a["log2n"], a["hop"], backend=seqexec.seq_backend_create(1016))


def test_render_spectrum_refuses_null_pointers(sa):
    prg = load_program(sa, KEY)
    lib = sa.lib()
    power, segs = np.zeros(257), C.c_uint64()
    pp = power.ctypes.data_as(C.POINTER(C.c_double))
    assert not lib.sauAmd_render_spectrum(None, 8000, 1, 1, 9, 256, pp, C.byref(segs), None) and "bad argument" in sa.api.last_error(lib)
    assert not lib.sauAmd_render_spectrum(prg.ptr, 8000, 1, 1, 9, 256, None, C.byref(segs), None) and "bad argument" in sa.api.last_error(lib)
    assert not lib.sauAmd_render_spectrum(prg.ptr, 8000, 1, 1, 9, 256, pp, None, None) and "bad argument" in sa.api.last_error(lib)
    lib.sauAmd_Spectrum_destroy(None)  # allowed


# ---- the launch plan ----------------------------------------------------------------------------------------------------

def plan(hooks_lib, L, hop, ch, pos, frames):
    n = len(pos)
    rows = (C.c_uint64 * (8 * n))()
    out = (C.c_uint64 * 8)()
    ok = hooks_lib.sauAmd_spectrum_plan(L, hop, ch, n, (C.c_uint64 * n)(*pos), (C.c_uint32 * n)(*frames), rows, out)
    names = ("seg0", "n_seg", "pend", "pend_next", "acc_cnt", "n_groups", "n_complete")
    return ok, [dict(zip(names, rows[8 * r:8 * r + 7])) for r in range(n)], dict(zip(("N", "bins", "max_groups", "lds_bytes", "pend_pitch",
                                                                                    "sum_pitch", "scratch", "rows"), out))


@pytest.mark.parametrize("L,hop", [(8, 32), (8, 100), (8, 256), (11, 1024), (12, 512)])
def test_the_plan_of_a_feed(spectrum_hooks, L, hop):
    N = 1 << L
    ends = [N - 1, N, N + hop - 1, N + hop, N + 15 * hop, N + 16 * hop, N + 33 * hop + 7]
    want_S = [0, 1, 1, 2, 16, 17, 34]
    assert [mdl.segments(P, N, hop) for P in ends] == want_S
    # from an empty record, and from positions an earlier feed has left: on both sides of a segment's and a group's end
    starts = [0, 1, N - 1, N, N + 1, N + hop - 1, N + hop, N + 14 * hop + 3, N + 15 * hop - 1, N + 15 * hop, N + 16 * hop]
    cases = [(p0, P - p0) for P in ends for p0 in starts if p0 <= P]
    ok, rows, out = plan(spectrum_hooks, L, hop, 2, [c[0] for c in cases], [c[1] for c in cases])
    assert ok == 1
    for (p0, fr), r in zip(cases, rows):
        s0, s1 = mdl.segments(p0, N, hop), mdl.segments(p0 + fr, N, hop)
        g0 = s0 // 16
        touched = sorted({s // 16 for s in range(s0, s1)})
        assert r["seg0"] == s0 and r["n_seg"] == s1 - s0, (p0, fr, r)
        assert r["pend"] == p0 - s0 * hop < N and r["pend_next"] == p0 + fr - s1 * hop < N, (p0, fr, r)
        assert r["acc_cnt"] == s0 % 16 and r["n_groups"] == len(touched), (p0, fr, r)
        assert touched == list(range(g0, g0 + len(touched)))
        assert r["n_complete"] == len([g for g in touched if 16 * g + 16 <= s1]), (p0, fr, r)
    assert out["N"] == N and out["bins"] == N // 2 + 1 and out["lds_bytes"] == 16 * N <= 65536
    assert out["max_groups"] == max(r["n_groups"] for r in rows) == 3
    assert out["pend_pitch"] == 2 * N and out["sum_pitch"] == 2 * (N // 2 + 1) and out["rows"] == len(cases)
    assert out["scratch"] == len(cases) * 2 * 3 * (N // 2 + 1)


def test_the_plan_refuses_what_the_header_refuses(spectrum_hooks):
    for L, hop, ch in ((7, 64, 1), (13, 4096, 1), (9, 63, 1), (9, 513, 1), (9, 0, 1), (9, 256, 0), (9, 256, 3)):
        assert plan(spectrum_hooks, L, hop, ch, [0], [1000])[0] == 0
    assert plan(spectrum_hooks, 9, 64, 2, [0], [1000])[0] == 1 and plan(spectrum_hooks, 9, 512, 1, [0], [1000])[0] == 1
    # a feed whose groups' sums would pass 2^27 doubles is refused: 2^32 - 1 frames at hop 32 are 8.4e6 groups of 129 bins
    assert plan(spectrum_hooks, 8, 32, 1, [0], [0xffffffff])[0] == 0
    assert plan(spectrum_hooks, 8, 32, 1, [0], [1 << 24])[0] == 1
    assert plan(spectrum_hooks, 8, 32, 1, [0] * 65536, [0] * 65536)[0] == 0  # more rows than a grid has
