"""Dither and noise shaping without a GPU (include/saugns_amd.h, section "Dither and noise shaping"): the header's known
answers on the independent model (tests/dither_model.py) and on the library's host restatement (tables.cpp, built from
sau_dither.h as the kernels are), the restatement against the model on random rows, cut independence, the anchor to the existing
rounding, every refusal that needs no device, and what dither is for -- a tone below half an LSB that a bare rounding erases
-- as conditions on fixed seeds. tests/test_gpu_dither.py compares the device with the host restatement."""
import hashlib
import os

import numpy as np
import pytest

import dither_model as dm
from conftest import load_program

KEY = "devtests__voice-reuse"
SHAPES = ["FLAT", "HP1", "E3", "E5", "F9"]


def ramp(n):
    k = np.arange(n)
    return ((((37 * k) % 101) - 50) / 65536).astype(np.float32)


def lib_spec(sa, dither, coef, seed):
    return sa.Dither(seed=seed, dither=dither, coef=coef)


def sown(rng, n, ch):
    """random samples around full scale with NaN, infinities and out-of-range values sown in"""
    x = (rng.standard_normal(n * ch) * rng.choice([1e-4, 0.01, 0.5])).astype(np.float32)
    for v in (np.nan, np.inf, -np.inf, 3.5, -7.25, 1.0, -1.0):
        x[rng.integers(0, x.size, 3)] = v
    return x


# ---- known answers -----------------------------------------------------------------------------------------------------------

def test_hash_known_answers():
    assert dm.hash_z(0, 0, 0) == 0xE220A8397B1DCDAF
    sr = dm.row_seed(0x0123456789ABCDEF, 2)
    assert sr == 0xA48DD9CD2CD1A7F5
    assert dm.hash_z(sr, 5, 1) == 0xFC6B0CE94FE76F9F
    assert dm.tpdf_int(sr, 5, 1) == 1252133
    assert dm.tpdf_array(sr, 5, 1, 1)[0] == 1252133 / 2.0 ** 24


FIRST12 = {"E5": [-25, -6, 11, -18, -5, 21, -18, 5, 22, -11, 9, -23],
           "F9": [-25, -6, 10, -16, -8, 26, -25, 13, 14, -4, 4, -19]}


@pytest.mark.parametrize("shape", ["E5", "F9"])
def test_first_samples_known_answers(sa, shape):
    x = ramp(12)
    got, _, _ = dm.quantize(x, 1, 1.0, 1, dm.PRESETS[shape][1], 1)
    assert got.tolist() == FIRST12[shape]
    out, _, cl = sa.dither_quantize(x, 1, 1.0, sa.dither_preset(dm.PRESETS[shape][0], 1))
    assert out.tolist() == FIRST12[shape] and cl == [0, 0]


def test_long_run_known_answer(sa):
    """n < 4096, gain -0.83, F9 with TPDF, seed 7, row 3, channel 1"""
    x = np.zeros((4096, 2), np.float32)
    x[:, 1] = ramp(4096)
    for out, hist, cl in (dm.quantize(x, 2, -0.83, 1, dm.PRESETS["F9"][1], 7, row=3),
                          sa.dither_quantize(x, 2, -0.83, sa.dither_preset(sa.DITHER_F9, 7), row=3)):
        ch1 = np.asarray(out).reshape(-1, 2)[:, 1].astype("<i2")
        assert hashlib.sha256(ch1.tobytes()).hexdigest().startswith("5d0d773724199efa")
        assert list(cl) == [0, 0]
        assert float(hist[1][0]).hex() == "-0x1.e710125a95b20p-2"


def test_presets(sa):
    for name in SHAPES:
        shape, coef = dm.PRESETS[name]
        d = sa.dither_preset(shape, 99).as_dict()
        assert d == {"seed": 99, "dither": 1, "taps": len(coef), "coef": coef}
    for bad in (-1, 5, 100):
        with pytest.raises(ValueError):
            sa.dither_preset(bad, 0)
    # the noise transfer function 1 - sum(coef[j] z^-(j+1)) of E5: its gain at DC and at Nyquist
    c = dm.PRESETS["E5"][1]
    assert abs(abs(1 - sum(c)) - 0.148) < 1e-3
    assert abs(abs(1 - sum(v * (-1) ** (j + 1) for j, v in enumerate(c))) - 9.36) < 1e-2


# ---- the restatement against the model ------------------------------------------------------------------------------------------

def specs(rng):
    out = [(0, []), (0, dm.PRESETS["E5"][1])] + [(1, dm.PRESETS[s][1]) for s in SHAPES]
    c = rng.uniform(-1, 1, 9)
    out.append((1, (c * (63.0 / np.abs(c).sum())).tolist()))  # nine random taps inside the bound
    return out


@pytest.mark.parametrize("ch", [1, 2])
def test_restatement_equals_model(sa, ch):
    rng = np.random.default_rng(5 + ch)
    n = 700
    for k, (dither, coef) in enumerate(specs(rng)):
        for gain in (1.0, 0.5, -0.83):
            x = sown(rng, n, ch)
            seed, row, first = int(rng.integers(0, 2 ** 63)), int(rng.integers(0, 65535)), int(rng.integers(0, 2 ** 40))
            hist = rng.uniform(-1.4, 1.4, (ch, 9))
            want, wh, wc = dm.quantize(x, ch, gain, dither, coef, seed, row=row, first=first, history=hist)
            got, gh, gc = sa.dither_quantize(x, ch, gain, lib_spec(sa, dither, coef, seed), row=row, first_frame=first, history=hist)
            assert np.array_equal(got, want), (k, gain)
            assert np.array_equal(gh, np.array(wh)), (k, gain)
            assert gc == wc, (k, gain)
            assert np.abs(got.astype(np.int32)).max() <= 32767


def test_full_scale_clips_as_the_header_says(sa):
    """constant full scale with F9 (seed 7, row 0): the clamp changes 902 of 2000 samples"""
    x = np.ones(2000, np.float32)
    want, _, wc = dm.quantize(x, 1, 1.0, 1, dm.PRESETS["F9"][1], 7)
    got, _, gc = sa.dither_quantize(x, 1, 1.0, sa.dither_preset(sa.DITHER_F9, 7))
    assert np.array_equal(got, want) and gc == wc == [902, 0]
    assert got.max() == 32767


def test_pieces_equal_one_piece(sa):
    rng = np.random.default_rng(11)
    ch, n = 2, 400
    x = sown(rng, n, ch)
    for dither, coef in specs(rng):
        spec = lib_spec(sa, dither, coef, 3)
        whole, wh, wc = sa.dither_quantize(x, ch, 0.5, spec, row=7, first_frame=1000)
        parts, hist, clips, at = [], None, [0, 0], 0
        for ln in (1, 63, 64, 65, n - 193):
            o, hist, c = sa.dither_quantize(x[at * ch:(at + ln) * ch], ch, 0.5, spec, row=7, first_frame=1000 + at, history=hist)
            parts.append(o)
            clips = [clips[0] + c[0], clips[1] + c[1]]
            at += ln
        assert at == n
        assert np.array_equal(np.concatenate(parts), whole)
        assert np.array_equal(hist, wh) and clips == wc


def test_no_dither_no_taps_is_the_existing_rounding(sa):
    rng = np.random.default_rng(2)
    x = np.concatenate([sown(rng, 4000, 1), (np.arange(-40000, 40000, 7) / 32767.0 + 0.5 / 32767.0).astype(np.float32)])
    spec = sa.Dither(seed=5)
    for gain in (1.0, 0.5, -0.83, 3.0):
        got, hist, cl = sa.dither_quantize(x, 1, gain, spec, history=np.full((1, 9), 0.25))
        assert np.array_equal(got.astype(np.int32), sa.flac_quantize(x, gain, 16))
        assert cl == [0, 0] and (hist == 0.25).all()
        assert np.array_equal(got, dm.quantize(x, 1, gain, 0, [], 5)[0])


# ---- refusals -----------------------------------------------------------------------------------------------------------------

def bad_specs(sa):
    nan = sa.Dither(seed=1, dither=1, coef=[0.5, float("nan")])
    inf = sa.Dither(seed=1, dither=1, coef=[float("inf")])
    big = sa.Dither(seed=1, dither=1, coef=[32.0, -32.5])
    d2 = sa.Dither(seed=1, dither=2)
    t10 = sa.Dither(seed=1, dither=1, coef=[0.1] * 9)
    t10.taps = 10
    return {"dither 2": d2, "taps 10": t10, "a NaN coefficient": nan, "an infinite coefficient": inf, "a sum above 64": big}


def test_invalid_specs_are_refused(sa):
    x = np.zeros(8, np.float32)
    for what, spec in bad_specs(sa).items():
        assert not dm.spec_valid(spec.dither, [spec.coef[j] for j in range(min(spec.taps, 9))] + [0.0] * max(spec.taps - 9, 0)), what
        with pytest.raises(ValueError):
            sa.dither_quantize(x, 1, 1.0, spec)
    ok = sa.Dither(seed=1, dither=1, coef=[32.0, -32.0])  # the bound itself is allowed
    sa.dither_quantize(x, 1, 1.0, ok)
    unused = sa.Dither(seed=1, dither=1, coef=[0.5])
    unused.coef[5] = float("nan")  # (an unused coefficient is not looked at)
    sa.dither_quantize(x, 1, 1.0, unused)
    for gain in (float("nan"), float("inf")):
        with pytest.raises(ValueError):
            sa.dither_quantize(x, 1, gain, ok)
    with pytest.raises(ValueError):
        sa.dither_quantize(x, 3, 1.0, ok)


def test_writers_refuse_before_any_file(sa, tmp_path):
    prg = load_program(sa, KEY)
    good = sa.dither_preset(sa.DITHER_E5, 1)
    path = str(tmp_path / "never")

    def refused(call):
        with pytest.raises(RuntimeError, match="bad argument"):
            call()
        assert not os.path.exists(path)

    for spec in bad_specs(sa).values():
        refused(lambda: sa.render_file_dithered(prg, 8000, path, spec, fmt=sa.SNDFILE_WAV, channels=2))
        refused(lambda: sa.render_file_flac_dithered(prg, 8000, path, spec, channels=2))
        refused(lambda: sa.render_file_loudness_dithered(prg, 8000, path, spec, channels=2))
    wav_f32 = sa.api.SNDFILE_WAV_F32
    refused(lambda: sa.render_file_dithered(prg, 8000, path, good, fmt=wav_f32, channels=2))
    refused(lambda: sa.render_file_loudness_dithered(prg, 8000, path, good, fmt=wav_f32, channels=2))
    refused(lambda: sa.render_file_dithered(prg, 8000, path, good, channels=3))
    refused(lambda: sa.render_file_dithered(prg, 8000, path, good, gain=float("nan")))
    refused(lambda: sa.render_file_flac_dithered(prg, 8000, path, good, gain=float("inf")))
    refused(lambda: sa.render_file_flac_dithered(prg, 8000, path, good, block_frames=300))
    refused(lambda: sa.render_file_flac_dithered(prg, 0, path, good))


# ---- what it is for: a 1 kHz sine of 0.4 LSB at 44.1 kHz, 65536 frames, seed 1 (the model) ---------------------------------------

N, RATE, AMP = 65536, 44100.0, 0.4
_tone = {}


def tone():
    if "x" not in _tone:
        ph = 2 * np.pi * 1000.0 * np.arange(N) / RATE
        _tone["s"], _tone["c"] = np.sin(ph), np.cos(ph)
        _tone["x"] = (AMP * _tone["s"] / 32767.0).astype(np.float32)
    return _tone


def quantized(name):
    if name not in _tone:
        t = tone()
        dither, coef = (0, []) if name == "none" else (1, dm.PRESETS[name][1])
        _tone[name] = dm.quantize(t["x"], 1, 1.0, dither, coef, 1)[0].astype(np.float64)
    return _tone[name]


def low_band_error_power(name):
    """the mean power of (output - input, in LSB) below 4 kHz"""
    t = tone()
    err = quantized(name) - t["x"].astype(np.float64) * 32767.0
    spec = np.abs(np.fft.rfft(err)) ** 2
    k = int(4000.0 / RATE * N)
    return spec[:k].sum() * 2 / N ** 2


def test_bare_rounding_erases_the_tone():
    assert not quantized("none").any()


def test_flat_dither_keeps_the_tone():
    t = tone()
    q = quantized("FLAT")
    amp = 2 * np.hypot(q @ t["s"], q @ t["c"]) / N
    assert abs(amp - AMP) <= 0.05 * AMP, amp
    mse = np.mean((q - t["x"].astype(np.float64) * 32767.0) ** 2)
    assert abs(mse - 0.25) <= 0.05 * 0.25, mse


@pytest.mark.parametrize("shape", ["E5", "F9"])
def test_shaping_moves_the_noise_out_of_the_low_band(shape):
    flat, shaped = low_band_error_power("FLAT"), low_band_error_power(shape)
    assert shaped <= flat / 10, (shaped, flat)
