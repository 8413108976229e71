"""BS.1770 loudness and true peak without a GPU (include/saugns_amd.h: sauAmdLoudness, sauAmd_loudness_filter,
sauAmd_truepeak_taps, sauAmd_loudness_gate, sauAmd_Batch_set_loudness, sauAmd_render_file_loudness): the coefficients and taps
against the header's formulas, the filter's response claims, the host gating against a Python restatement
(tests/loudness_model.py) bit for bit, the refusals over the sequential test executor (tests/seqexec keeps engine.h's
refusing defaults) -- each before a file exists -- and the accuracy of the chunked evaluation itself."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import loudness_model as lm
from conftest import ORACLE_FORMS, ROOT, load_program, max_diff

KEY = "devtests__voice-reuse"
RATES = [8000, 44100, 48000, 384000]


@pytest.fixture(scope="module")
def loudness_hooks(sa, hooks):
    """tests/hooks_loudness/libsaugns_amd_loudness_hooks.so: the product's object files (the `hooks` fixture has built them) +
    the loudness-normalised writer over an injected backend"""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "hooks_loudness")])
    return sa.api.use_loudness_hooks(os.path.join(ROOT, "tests", "hooks_loudness", "libsaugns_amd_loudness_hooks.so"))


def test_the_loudness_structure_is_48_bytes(sa):
    L = sa.api.Loudness
    assert C.sizeof(L) == 48
    assert [getattr(L, f).offset for f in ("frames", "blocks", "gated_blocks", "integrated", "momentary_max", "true_peak")] == \
        [0, 8, 16, 24, 32, 40]


def test_the_constants_the_model_mirrors_are_the_headers():
    hdr = open(os.path.join(ROOT, "saugns_amd", "csrc", "launch_plan.h")).read()
    assert re.search(r"LOUD_CHUNK = 256;", hdr)
    assert re.search(r"TP_THREADS = 64, TP_PER_LANE = 4, TP_TILE = TP_THREADS \* TP_PER_LANE;", hdr)
    assert (lm.LOUD_CHUNK, lm.TP_TILE) == (256, 256)


@pytest.mark.parametrize("fs", RATES)
def test_the_coefficients_match_the_formulas(sa, fs):
    got = sa.loudness_filter(fs)
    want = lm.filter_formula(fs)
    assert got is not None and np.abs(got - np.array(want)).max() <= 1e-13, (fs, list(got), want)
    assert list(got[5:8]) == [1.0, -2.0, 1.0]


def test_at_48000_they_are_the_bs1770_table(sa):
    got = sa.loudness_filter(48000)
    table = [1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
             1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621]
    assert np.abs(got - np.array(table)).max() <= 1e-12, list(got)


def test_no_coefficients_below_2560(sa):
    assert sa.loudness_filter(2559) is None
    assert sa.loudness_filter(2560) is not None


def test_the_true_peak_taps_match_the_formula(sa):
    L = sa.lib()
    assert L.sauAmd_truepeak_taps(None, 0) == 129
    few = np.full(128, 7.0)
    assert L.sauAmd_truepeak_taps(few.ctypes.data_as(C.POINTER(C.c_double)), 128) == 129 and (few == 7.0).all()
    g = sa.truepeak_taps()
    assert len(g) == 129 and g[64] == 1.0 and (g == g[::-1]).all()
    assert np.abs(g - lm.taps_formula()).max() <= 1e-13


def test_the_interpolators_response_claims(sa):
    """at the 4x rate the filter passes to 0.45 of the input rate within 0.02 dB and stops from 0.55 of it below -53 dB
    (gain 4: the taps are not normalised, each of the four phases sums to about 1)"""
    g = sa.truepeak_taps()
    n = np.arange(129)

    def db(f_of_rate):  # f as a fraction of the INPUT rate
        w = 2.0 * math.pi * np.asarray(f_of_rate)[:, None] / 4.0
        h = np.abs((g[None, :] * np.exp(-1j * w * n[None, :])).sum(axis=1)) / 4.0
        return 20.0 * np.log10(np.maximum(h, 1e-300))

    assert np.abs(db(np.linspace(0.0, 0.45, 2001))).max() <= 0.02
    assert db(np.linspace(0.55, 2.0, 8001)).max() <= -53.0


def test_a_full_scale_997_hz_sine_reads_minus_3_01_lufs(sa):
    fs, hop = 48000, 4800
    x = np.sin(2.0 * math.pi * 997.0 * np.arange(fs) / fs).astype(np.float32)
    hops = np.zeros((fs // hop, 2))
    hops[:, 0] = lm.sequential_hops(sa.loudness_filter(fs), x, hop)
    assert abs(sa.loudness_gate(hops, hop, 1).integrated - -3.0103) <= 2e-3


def _level(lufs, hop, channels=1):
    """a hop's energy per channel such that a block of four such hops reads `lufs`"""
    return 10.0 ** ((lufs + 0.691) / 10.0) * hop / channels


def gate_cases():
    hop = 800
    rng = np.random.default_rng(1770)
    loud, quiet = _level(-20.0, hop), _level(-45.0, hop)
    cases = {
        "no hops": np.zeros((0, 2)),
        "three hops": np.full((3, 2), loud),
        "four hops": np.full((4, 2), loud),
        "all zero": np.zeros((12, 2)),
        # twenty loud hops, then twenty 25 dB below: the relative gate cuts the quiet blocks
        "a level step": np.concatenate([np.full((20, 2), loud), np.full((20, 2), quiet)]),
        "around the absolute gate": np.concatenate([np.full((8, 2), _level(-71.0, hop)), np.full((8, 2), _level(-69.0, hop))]),
        "only below the absolute gate": np.full((9, 2), _level(-71.0, hop)),
        "noise": rng.random((37, 2)) * loud,
    }
    return hop, cases


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("name", list(gate_cases()[1]))
def test_the_gating_equals_the_restatement(sa, name, channels):
    hop, cases = gate_cases()
    hops = cases[name].copy()
    if channels == 2:  # two thirds and one third of it: the blocks read what the mono ones do
        hops[:, 0] *= 2.0 / 3.0
        hops[:, 1] = hops[:, 0] * 0.5
    got = sa.loudness_gate(hops, hop, channels)
    want = lm.gate(hops, hop, channels)
    assert (got.blocks, got.gated_blocks) == (want["blocks"], want["gated_blocks"]), (name, got, want)
    for k in ("integrated", "momentary_max"):
        assert np.float64(getattr(got, k)).view(np.uint64) == np.float64(want[k]).view(np.uint64), (name, k, got, want)
    assert got.frames == len(hops) * hop and list(got.true_peak) == [0.0, 0.0]
    if name in ("no hops", "three hops"):
        assert got.blocks == 0 and got.integrated == -math.inf and got.momentary_max == -math.inf
    if name == "all zero":
        assert got.blocks == 9 and got.gated_blocks == 0 and got.integrated == -math.inf
    if name == "a level step":
        assert got.blocks == 37 and 17 <= got.gated_blocks <= 20 and abs(got.integrated - -20.0) < 0.5
    if name == "around the absolute gate":
        # blocks wholly at -71 fall to the absolute gate; the mixed ones and those at -69 stay
        assert got.blocks == 13 and 5 <= got.gated_blocks <= 8, got
    if name == "only below the absolute gate":
        assert got.blocks == 6 and got.gated_blocks == 0 and got.integrated == -math.inf and abs(got.momentary_max - -71.0) < 1e-9


def test_the_gate_refuses_bad_arguments(sa):
    hops = np.zeros((4, 2))
    for hop, ch in ((0, 1), (800, 0), (800, 3)):
        with pytest.raises(RuntimeError, match="bad argument"):
            sa.loudness_gate(hops, hop, ch)


def test_loudness_is_refused_and_the_int16_render_after_it_starts_at_frame_0(sa, oracle, seqexec):
    oracle.oracle().ora_set_fastmath_forms(ORACLE_FORMS)
    prg = load_program(sa, KEY)
    want = oracle.oracle_render(prg.ptr, 12000, True, chunk=5000)
    b = sa.Batch([prg], 12000, backend=seqexec.seq_backend_create(1016))
    with pytest.raises(RuntimeError, match="loudness"):
        b.set_loudness(True)
    assert "this backend" in sa.api.last_error()
    rows = np.zeros(64, np.float32)  # (host memory: the refusal comes before anything reads it)
    with pytest.raises(RuntimeError, match="loudness"):
        b.measure_loudness_rows((rows.ctypes.data + 15) & ~15, 64, 1, 8, 1, 8000)
    b.set_loudness(False)  # always succeeds
    ld = b.loudness()  # never on: empty records, and no backend asked
    assert len(ld) == 1 and ld[0].frames == 0 and ld[0].blocks == 0 and ld[0].integrated == -math.inf
    assert len(b.loudness_hops(0)) == 0
    got = b.render(stereo=True, chunk=5000)[0]
    b.close()
    assert max_diff(got, want) == 0


def test_loudness_below_2560_hz_is_refused(sa, oracle, seqexec):
    oracle.oracle().ora_set_fastmath_forms(ORACLE_FORMS)
    prg = load_program(sa, KEY)
    want = oracle.oracle_render(prg.ptr, 2000, False, chunk=700)
    b = sa.Batch([prg], 2000, backend=seqexec.seq_backend_create(1016))
    with pytest.raises(RuntimeError, match="bad argument"):
        b.set_loudness(True)
    got = b.render(stereo=False, chunk=700)[0]
    b.close()
    assert max_diff(got, want) == 0


@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
def test_the_loudness_writer_over_a_backend_without_it_makes_no_file(sa, seqexec, loudness_hooks, tmp_path, fmt):
    prg = load_program(sa, KEY)
    path = str(tmp_path / "loud.out")
    with pytest.raises(RuntimeError, match="this backend has no"):
        sa.render_file_loudness(prg, 12000, path, fmt, 2, -23.0, 1.0, backend=seqexec.seq_backend_create(1016))
    assert "this backend has no" in sa.api.last_error()
    assert not os.path.exists(path)


BAD = [(math.nan, 1.0, 12000), (math.inf, 1.0, 12000), (-math.inf, 1.0, 12000), (-23.0, 0.0, 12000), (-23.0, -1.0, 12000),
       (-23.0, math.nan, 12000), (-23.0, math.inf, 12000), (-23.0, 1.0, 2559)]


@pytest.mark.parametrize("target,ceiling,srate", BAD)
def test_the_loudness_writers_bad_arguments_make_no_file(sa, oracle, seqexec, loudness_hooks, tmp_path, target, ceiling, srate):
    prg = load_program(sa, KEY)
    path = str(tmp_path / "loud.wav")
    # over the executor, and through the product's own entry point: the arguments are looked at before any backend is made,
    # so this is the same refusal with and without a GPU
    with pytest.raises(RuntimeError, match="bad argument"):
        sa.render_file_loudness(prg, srate, path, sa.api.SNDFILE_WAV, 1, target, ceiling, backend=seqexec.seq_backend_create(1016))
    assert not os.path.exists(path)
    with pytest.raises(RuntimeError, match="bad argument"):
        sa.render_file_loudness(prg, srate, path, sa.api.SNDFILE_WAV, 1, target, ceiling)
    assert "bad argument" in sa.api.last_error()
    assert not os.path.exists(path)
    for fmt, channels in ((4, 1), (-1, 1), (2, 0), (2, 3)):
        with pytest.raises(RuntimeError, match="bad argument"):
            sa.render_file_loudness(prg, 12000, path, fmt, channels, -23.0, 1.0)
        assert not os.path.exists(path)


# The chunked evaluation against the plain sequential one, on noise with a DC offset: the largest difference of a hop's
# energy as a fraction of the row's sum of x * x. Measured with this test's inputs: 8000 Hz 1.5e-16,
# 44100 Hz 3.2e-15, 384000 Hz 2.7e-13 -- the high-pass's pole pair moves towards the unit circle as the rate grows, and what
# the map M rounds away grows with it. The bound is 64 times the largest of them: room for other inputs and seeds.
CHUNK_ACCURACY = 64 * 2.7e-13


@pytest.mark.parametrize("fs", [8000, 44100, 384000])
def test_the_chunked_method_is_as_accurate_as_the_sequential_one(sa, fs):
    hop, n = fs // 10, 20000 if fs < 100000 else 2 * (fs // 10) + 777
    rng = np.random.default_rng(fs)
    x = (rng.standard_normal(n) * 0.25 + 0.1).astype(np.float32)
    f = sa.loudness_filter(fs)
    m = lm.Meter(f, sa.truepeak_taps(), hop, 1)
    m.run(x)
    got, want = m.hops()[:, 0], lm.sequential_hops(f, x, hop)
    assert len(got) == len(want) == n // hop
    ratio = np.abs(got - want).max() / float((x.astype(np.float64) ** 2).sum())
    print("chunked against sequential at", fs, "Hz:", ratio, "of the sum of x * x")
    assert ratio <= CHUNK_ACCURACY, (fs, ratio)
