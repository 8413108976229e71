"""Oversampled rendering on the device (include/saugns_amd.h: sauAmd_Batch_run_decimated_f32, sauAmd_Batch_device_decimated_f32,
sauAmd_render_file_oversampled; kernels: saugns_amd/csrc/k_decimate.h).

The reference is numpy applied to a SECOND batch's run_f32 output at srate * K -- tests/test_gpu_f32.py pins that float path to
the oracle -- rendered in the same runs (a run is one call of the reference's block lattice), and it is the header's loop as it
stands: float64, the taps the library exports, ascending j, acc = acc + h[j] * x64[m * K - j], then .astype(float32). numpy
neither fuses the multiply into the add nor reorders the sum, so the comparison is by BYTES. The reference is asserted to
hold no non-zero subnormal, so no denormal mode can come into it -- subnormal, non-finite and full-scale samples, poison behind
a stream's end and every kernel instantiation are tests/test_gpu_decimate_rows.py's, on rows of its own."""
import functools
import struct

import numpy as np
import pytest

from conftest import ORACLE_FORMS, load_program
from test_gpu_levels import check_levels, count_levels, quantise

pytestmark = pytest.mark.gpu

RATE = 6000  # the output rate
H = 32
DECIM_TILE = 256  # launch_plan.h (plan_decimate), mirrored: tests/test_decimate_host.py reads the header
KEYS = ["devtests__voice-reuse", "devtests__pm-addremaddrem"]  # 4 s; 2 s with a PM chain
THIRD = "examples__tests__vibrato-pm"  # 2.1 s


def decimate_ref(sa, x_hi, K, ch, n_out, allow_subnormal=False):
    """the header's loop over x_hi (float32, interleaved, from the start of the sequence; +0 before it and behind its end)
    -> n_out frames as float32. allow_subnormal: the caller feeds crafted rows and compares subnormal results too
    (tests/test_gpu_decimate_rows.py); everyone else's reference holds none."""
    h = sa.decimator_taps(K)
    L = len(h)
    x = np.asarray(x_hi, np.float32).reshape(-1, ch)
    xp = np.zeros((L - 1 + n_out * K, ch), np.float64)  # xp[L - 1 + i] = x[i]
    n = min(len(x), n_out * K)
    xp[L - 1:L - 1 + n] = x[:n]
    acc = np.zeros((n_out, ch), np.float64)
    for j in range(L):
        acc = acc + h[j] * xp[L - 1 - j:L - 1 - j + n_out * K:K]
    y = acc.astype(np.float32)
    if not allow_subnormal:
        tiny = np.abs(y) < np.finfo(np.float32).tiny
        assert not (tiny & (y != 0)).any(), "the reference holds a non-zero subnormal"
    return y.reshape(-1)


def _same_bytes(got, want, what):
    got, want = np.ascontiguousarray(got).reshape(-1), np.ascontiguousarray(want).reshape(-1)
    assert got.dtype == want.dtype and len(got) == len(want), (what, got.dtype, want.dtype, len(got), len(want))
    g, w = got.view(np.uint8).reshape(len(got), -1), want.view(np.uint8).reshape(len(want), -1)
    d = np.flatnonzero((g != w).any(axis=1))
    assert len(d) == 0, f"{what}: {len(d)} samples differ, first at {d[0]}: got {got[d[0]:d[0] + 4].tolist()} want {want[d[0]:d[0] + 4].tolist()}"


def run_lengths(first, then, total):
    """output frames per run: `first`, then `then` over and over until `total` frames are covered"""
    out, n = list(first), sum(first)
    while n < total:
        out.append(then)
        n += then
    return out


def high_rate(sa, prgs, K, stereo, lens_out):
    """a second batch's float runs of lens_out[r] * K frames each -> per stream: the valid frames end to end (float32,
    interleaved), the per-run out_len and more"""
    ch = 2 if stereo else 1
    b = sa.Batch(prgs, RATE * K)
    xs, lens, mores = [[] for _ in prgs], [], []
    for n in lens_out:
        pcm, more, ln = b.run_f32(n * K, stereo)
        for i in range(b.n):
            xs[i].append(pcm[i, :ln[i] * ch].copy())
        lens.append(ln)
        mores.append(more)
    b.close()
    return [np.concatenate(x) for x in xs], lens, mores


@pytest.fixture(autouse=True)
def forms(oracle):
    oracle.oracle().ora_set_fastmath_forms(ORACLE_FORMS)


# ---- (a) one sequence of runs: shorter than the history, longer than a tile and off its multiples, the tail --------------

@pytest.mark.parametrize("stereo", [False, True])
@pytest.mark.parametrize("K", [2, 4, 8])
@pytest.mark.parametrize("key", KEYS)
def test_a_sequence_of_decimated_runs_is_the_reference_frame_for_frame(sa, key, K, stereo):
    ch = 2 if stereo else 1
    prg = load_program(sa, key)
    total = {KEYS[0]: 4 * RATE, KEYS[1]: 2 * RATE}[key]
    # 37, 1 and 5 frames are runs shorter than the history (64 output frames); 300 is more than one tile and not a multiple
    plan = run_lengths([37, 1, 5, 300, 5], 4099, total)
    assert 300 > DECIM_TILE and 300 % DECIM_TILE and max(37, 1, 5) < 2 * H
    x_hi, lens_hi, mores_hi = high_rate(sa, [prg], K, stereo, plan)
    assert not mores_hi[-1][0] and -(-len(x_hi[0]) // (K * ch)) == total
    plan = plan + [2 * H + 6]  # one run after the end: the rest of the tail
    want = decimate_ref(sa, x_hi[0], K, ch, sum(plan))
    b = sa.Batch([prg], RATE * K)
    got, pos = [], 0
    for r, n in enumerate(plan):
        y, more, ln = b.run_decimated(K, n, stereo)
        assert y.dtype == np.float32 and y.shape == (1, n * ch)
        if r < len(lens_hi):
            assert more == mores_hi[r] and ln == [-(-lens_hi[r][0] // K)], (r, more, ln, lens_hi[r])
        else:
            assert more == [False] and ln == [0]
        got.append(y[0])
        pos += n
    b.close()
    got = np.concatenate(got)
    _same_bytes(got, want, (key, K, stereo))


# ---- (b) three streams of different lengths: the zero extension goes by each stream's frame count ------------------------

def test_streams_that_end_inside_a_run_are_zero_extended_and_still_deliver_their_tails(sa):
    K, stereo, ch = 4, True, 2
    prgs = [load_program(sa, k) for k in (KEYS[0], KEYS[1], THIRD)]
    ends = [4 * RATE, 2 * RATE, 12600]  # output frames
    # a long first run, then short ones: stream 1 ends 300 frames into the third run and stream 2 200 frames into the fourth,
    # at frames where the run before left signal in the rows
    plan = run_lengths([11000, 700, 700, 700, 700], 5000, ends[0])
    x_hi, lens_hi, mores_hi = high_rate(sa, prgs, K, stereo, plan)
    assert [len(x) for x in x_hi] == [e * K * ch for e in ends]
    assert lens_hi[2][1] == 300 * K and lens_hi[3][2] == 200 * K and lens_hi[2][0] == 700 * K
    plan = plan + [100]
    want = [decimate_ref(sa, x, K, ch, sum(plan)) for x in x_hi]
    b = sa.Batch(prgs, RATE * K)
    got = [[] for _ in prgs]
    for r, n in enumerate(plan):
        y, more, ln = b.run_decimated(K, n, stereo)
        if r < len(lens_hi):
            assert more == mores_hi[r] and ln == [-(-v // K) for v in lens_hi[r]]
        else:
            assert more == [False] * 3 and ln == [0] * 3
        for i in range(3):
            got[i].append(y[i])
    b.close()
    for i in range(3):
        _same_bytes(np.concatenate(got[i]), want[i], ("stream", i))
    # the ended streams' tails were there to deliver: the H frames behind stream 1's end are not all zero
    assert np.abs(want[1][ends[1] * ch:(ends[1] + H) * ch]).max() > 0


# ---- (c) the history belongs to one sequence ------------------------------------------------------------------------------

def test_the_history_starts_from_zero_after_a_float_run_and_after_a_change_of_factor(sa):
    stereo, ch = False, 1
    prg = load_program(sa, KEYS[0])
    # the batch's rate is 24000: runs of 500 x 4, 100 (float), 300 x 4, 300 x 2 and 40 x 4 (stereo) frames
    hi = [2000, 100, 1200, 600]
    ref = sa.Batch([prg], RATE * 4)
    x = [ref.run_f32(n, stereo)[0][0] for n in hi]
    x.append(ref.run_f32(160, True)[0][0])
    ref.close()
    b = sa.Batch([prg], RATE * 4)
    y0 = b.run_decimated(4, 500, stereo)[0][0]
    _same_bytes(y0, decimate_ref(sa, x[0], 4, ch, 500), "first sequence")
    f = b.run_f32(100, stereo)[0][0]
    _same_bytes(f, x[1], "the interposed float run")
    y1 = b.run_decimated(4, 300, stereo)[0][0]
    _same_bytes(y1, decimate_ref(sa, x[2], 4, ch, 300), "after a float run")
    assert y1.tobytes() != decimate_ref(sa, np.concatenate([x[0], x[1], x[2]]), 4, ch, 825)[525:].tobytes()  # (a history would show)
    y2 = b.run_decimated(2, 300, stereo)[0][0]
    _same_bytes(y2, decimate_ref(sa, x[3], 2, ch, 300), "after a change of factor")
    y3 = b.run_decimated(4, 40, True)[0][0]
    _same_bytes(y3, decimate_ref(sa, x[4], 4, 2, 40), "after a change of channel layout")
    b.close()


# ---- (d) the decimated rows, measured where they are ----------------------------------------------------------------------

def test_decimated_device_rows_measure_as_the_fetched_rows_do(sa):
    prgs = [load_program(sa, k) for k in KEYS]
    for stereo in (False, True):
        ch = 2 if stereo else 1
        b = sa.Batch(prgs, RATE * 2)
        n = 1111
        y = b.run_decimated(2, n, stereo)[0]
        b.sync()
        ptr, pitch = b.device_decimated_f32(0), b.device_decimated_pitch()
        assert ptr and ptr % 16 == 0 and pitch % 256 == 0 and pitch >= n * ch * 4
        assert b.device_decimated_f32(1) == ptr + pitch
        lv = b.measure_rows(ptr, pitch, 2, True, n, ch)
        for i in range(2):
            assert np.abs(y[i]).max() > 0
            check_levels(lv[i], count_levels(y[i], ch, n), ("row", i, stereo), exact_sum=False)
        b.close()


# ---- (e) the oversampled file writer ---------------------------------------------------------------------------------------

HEADER = {0: 0, 1: 28, 2: 44, 3: 58}  # RAW, AU, WAV, WAV_F32


@functools.lru_cache(maxsize=None)
def _file_reference(factor, channels):
    """sauAmd_render_file at RATE * factor as float WAV -> its samples decimated on the host, H frames dropped,
    ceil(N / factor) kept"""
    import tempfile
    import saugns_amd as sa
    prg = load_program(sa, KEYS[1])
    with tempfile.TemporaryDirectory() as t:
        n_hi = sa.render_file(prg, RATE * factor, t + "/hi.wav", sa.api.SNDFILE_WAV_F32, channels)
        x = np.frombuffer(open(t + "/hi.wav", "rb").read()[HEADER[3]:], "<f4")
    assert len(x) == n_hi * channels and n_hi == 2 * RATE * factor
    keep = -(-n_hi // factor)
    y = decimate_ref(sa, x, factor, channels, keep + H)[H * channels:]
    y.setflags(write=False)
    return keep, y


# factor 4 stereo in every format (ids as before); factors 2 and 8 mono in the int16 formats with a header: the big-endian one
# (AU) and the little-endian one (WAV) -- decimate_kernel<2 and 8, int16_t, 1> with and without swap_bytes
@pytest.mark.parametrize("factor,channels,fmt", [
    pytest.param(4, 2, 0, id="0"), pytest.param(4, 2, 1, id="1"), pytest.param(4, 2, 2, id="2"), pytest.param(4, 2, 3, id="3"),
    pytest.param(2, 1, 1, id="x2-mono-au"), pytest.param(2, 1, 2, id="x2-mono-wav"),
    pytest.param(8, 1, 1, id="x8-mono-au"), pytest.param(8, 1, 2, id="x8-mono-wav")])
def test_oversampled_files(sa, tmp_path, factor, channels, fmt):
    keep, y = _file_reference(factor, channels)
    prg = load_program(sa, KEYS[1])
    path = str(tmp_path / "over.out")
    assert sa.render_file_oversampled(prg, RATE, factor, path, fmt, channels) == keep
    raw = open(path, "rb").read()
    head, data = raw[:HEADER[fmt]], raw[HEADER[fmt]:]
    if fmt == 3:
        want = y.astype("<f4").tobytes()
    else:
        want = quantise(y).astype(">i2" if fmt == 1 else "<i2").tobytes()
    assert len(data) == len(want) == keep * channels * (4 if fmt == 3 else 2)
    assert data == want
    if fmt == 1:
        assert head[:4] == b".snd" and struct.unpack(">I", head[16:20])[0] == RATE and struct.unpack(">I", head[8:12])[0] == keep
    elif fmt in (2, 3):
        assert head[:4] == b"RIFF" and struct.unpack("<I", head[24:28])[0] == RATE
        assert struct.unpack("<I", head[-4:])[0] == len(data)


# ---- (f) a batch that never decimates renders as before -------------------------------------------------------------------

def test_without_a_decimated_run_int16_and_float_renders_equal_the_oracles(sa, oracle):
    prg = load_program(sa, KEYS[0])
    want = oracle.oracle_render(prg.ptr, 12000, True, chunk=5000)
    b = sa.Batch([prg], 12000)
    assert not b.device_decimated_f32(0) and b.device_decimated_pitch() == 0
    got = b.render(stereo=True, chunk=5000)[0]
    b.close()
    assert len(got) == len(want) and (got == want).all()
    b = sa.Batch([prg], 12000)
    outs, more = [], [True]
    while more[0]:
        pcm, more, lens = b.run_f32(5000, True)
        outs.append(pcm[0, :lens[0] * 2])
    assert not b.device_decimated_f32(0)
    b.close()
    x = np.concatenate(outs)
    assert len(x) == len(want) and (quantise(x) == want).all()
