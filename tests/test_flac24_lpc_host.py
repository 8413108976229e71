"""The LPC mode of the 24-bit FLAC encoder without a GPU (include/saugns_amd.h, section "FLAC", paragraph "LPC at 24 bits":
sauAmd_flac_encode_block_lpc24 and the refusals of the other three _lpc24 entry points): the numpy restatement of that
paragraph (tests/flac24_lpc_model.py) against its own independent decoder, the library's host restatement (tables.cpp, built
from sau_flac.h as the kernels are) against the model byte for byte, step 5b's shared function (sau_flac.h: flac_lpc_guard)
through tests/hooks_flac24_lpc against the model on vectors that fire it and vectors that do not, a stream on which it takes an
order away, and the committed golden stream. The entry points that take `bits` keep refusing (24, M > 0).
tests/test_gpu_flac24_lpc.py compares the device with the host restatement."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import flac24_lpc_model as mdl
import flac_lpc_model as l16
import test_flac_lpc_steps_host as steps
from conftest import GOLDEN, ROOT, load_program

KEY = "devtests__voice-reuse"
GOLDEN_FLAC = os.path.join(GOLDEN, mdl.GOLDEN_NAME)
BLOCKS = (256, 1024, 4096)
POLES = (0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85)


def guard_hooks_lib():
    """tests/hooks_flac24_lpc/libsaugns_amd_flac24_lpc_hooks.so: sau_flac.h's flac_lpc_guard on the host and for gfx950"""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "hooks_flac24_lpc")])
    L = C.CDLL(os.path.join(ROOT, "tests", "hooks_flac24_lpc", "libsaugns_amd_flac24_lpc_hooks.so"))
    for f in (L.sauAmd_kat_flac_lpc_guard_host, L.sauAmd_kat_flac_lpc_guard_device):
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    return L


@pytest.fixture(scope="module")
def guard_hooks():
    return guard_hooks_lib()


# ---- the cases -------------------------------------------------------------------------------------------------------------

_cases = {}


def cases(B):
    """[(tag, channels, M, frame number, int32 samples of one block)], the same on every call: float PM material at every M in both
    channel counts, ar(p) * 1200 for p = 1 .. 8 at M = 8 (and stereo pairs of them), flac24_model's crafted kinds -- the rails
    among them, whose side channel is +-16777214 --, short last blocks and n <= 4"""
    if B in _cases:
        return _cases[B]
    out = []
    for ch in (1, 2):
        x = mdl.pm(2 * B, ch, seed=1)[B * ch:]  # (the second block: no phase of the voice starts at 0)
        for M in range(1, 9):
            out.append(("pm", ch, M, M + 126, x))
    for p in range(1, 9):
        out.append(("ar%d" % p, 1, 8, p, mdl.rows(mdl.ar(p, B, p))))
    for p in (2, 5, 8):
        out.append(("ar%d+%d" % (p, 9 - p), 2, 8, 2047 + p, mdl.rows(mdl.ar(p, B, p), mdl.ar(9 - p, B, 20 + p))))
        out.append(("ar%d at M=%d" % (p, p - 1), 1, p - 1, 70000, mdl.rows(mdl.ar(p, B, p))))
    for i, kind in enumerate(mdl.KINDS):
        for ch in (1, 2):
            out.append((kind, ch, 8, i, mdl.crafted(kind, B, ch, seed=i, B=B)))
            out.append((kind + "/M3", ch, 3, i, mdl.crafted(kind, B, ch, seed=i, B=B)))
    for n in (1, 2, 3, 4, 5, 255, B - 1):
        for ch in (1, 2):
            out.append(("short%d" % n, ch, 8, (1 << 31) - 1, mdl.pm(n, ch, seed=2)))
    _cases[B] = out
    return out


_model = {}


def model_frame(B, i):
    """the model's frame and choices of cases(B)[i], computed once"""
    if (B, i) not in _model:
        tag, ch, M, number, x = cases(B)[i]
        _model[(B, i)] = mdl.encode_block(x, ch, B, number, M, with_choice=True)
    return _model[(B, i)]


# ---- the model ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", BLOCKS)
def test_the_model_decodes_what_it_encodes(B):
    kinds_seen = set()
    for i, (tag, ch, M, number, x) in enumerate(cases(B)):
        frame, (assign, an, _) = model_frame(B, i)
        got, end, kd = mdl.decode_frame(frame, 0, ch, B, number)
        assert end == len(frame) and (got.reshape(-1) == x).all(), (tag, ch, M)
        assert [k.split("/")[0].rstrip("0123456789") for k in kd] == [a["type"] for a in an], (tag, kd)
        assert len(frame) <= mdl.frame_bound(len(x) // ch, ch)
        kinds_seen |= {a["type"] for a in an}
        if tag.startswith("short"):
            assert all(a["type"] != "lpc" for a in an)  # whole blocks only
    assert kinds_seen == {"constant", "verbatim", "fixed", "lpc"}


def test_the_all_pole_material_makes_the_model_choose_every_order():
    """at B = 256 with M = 8, ar(p) * 1200 is coded with order p, for p = 1 .. 8"""
    chosen = {}
    for i, (tag, ch, M, number, x) in enumerate(cases(256)):
        if tag.startswith("ar") and ch == 1 and M == 8:
            _, (_, an, _) = model_frame(256, i)
            assert an[0]["type"] == "lpc", tag
            chosen[tag] = an[0]["order"]
    assert chosen == {"ar%d" % p: p for p in range(1, 9)}


def test_the_pm_material_is_a_quarter_shorter():
    """what the mode is for: the float PM voice at 24 bits, B = 1024 stereo, four blocks, every subframe of the first an LPC one"""
    x = mdl.pm(4096, 2, seed=1)
    b0, b8 = (len(mdl.encode_stream(x, 2, 1024, M)[0]) for M in (0, 8))
    assert b8 < 0.75 * b0, (b0, b8)
    _, (_, an, _) = mdl.encode_block(x[:2048], 2, 1024, 0, 8, with_choice=True)
    assert all(a["type"] == "lpc" for a in an)


def test_the_decoder_refuses_what_the_paragraph_excludes():
    B = 256
    x = mdl.pm(B + 9, 2, seed=1)
    data, sizes = mdl.encode_stream(x, 2, B, 8)
    _, _, kinds = mdl.decode_frames(data, 2, B)
    assert all(k.startswith("lpc") for k in kinds[0]), kinds

    def broken(at, xor):
        b = bytearray(data)
        b[at] ^= xor
        return bytes(b)

    for what, d in (("sync", broken(1, 0x01)), ("the sample size code", broken(3, 0x04)), ("CRC-8", broken(4, 0x01)),
                    ("CRC-16", broken(sizes[0] - 1, 0x80)), ("a body bit", broken(sizes[0] // 2, 0x10)),
                    ("cut short", data[:-1]), ("bytes behind", data + b"\0")):
        with pytest.raises((mdl.Bad, ValueError, IndexError)):
            mdl.decode_frames(d, 2, B)
    # a 16-bit LPC stream is no 24-bit one, and the other way round
    with pytest.raises(mdl.Bad):
        mdl.decode_frames(l16.encode_stream(l16.pm(B, 2, seed=1), 2, B, 8)[0], 2, B)
    with pytest.raises(l16.Bad):
        l16.decode_frames(data, 2, B)


# ---- the library's host restatement -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", BLOCKS)
def test_the_hosts_block_equals_the_model_byte_for_byte_and_is_never_longer(sa, B):
    for i, (tag, ch, M, number, x) in enumerate(cases(B)):
        frame, _ = model_frame(B, i)
        got = sa.flac_encode_block_lpc24(x, ch, B, number, M)
        assert got == frame, (tag, ch, M, number, len(got), len(frame))
        plain = sa.flac_encode_block_s32(x, ch, B, number, bits=24)
        assert plain and len(got) <= len(plain), (tag, ch, M)
        assert sa.flac_encode_block_lpc24(x, ch, B, number, 0) == plain, (tag, ch)
        assert sa.flac_encode_block_s32(x, ch, B, number, bits=24, max_lpc_order=M) == b"", (tag, ch, M)  # that one keeps refusing
    x = mdl.pm(4096, 2, seed=1)
    assert sa.flac_encode_block_lpc24(x, 2, 0, 7, 8) == mdl.encode_block(x, 2, 4096, 7, 8)  # 0 means 4096
    # samples the quantiser never makes: -2^23 is inside the format
    x = mdl.rows(np.where(np.arange(256) % 7 < 3, mdl.S24_MIN, mdl.S24_MAX).astype(np.int64))
    assert sa.flac_encode_block_lpc24(x, 1, 256, 1, 8) == mdl.encode_block(x, 1, 256, 1, 8)


def test_a_short_cap_writes_nothing_and_bad_arguments_give_0(sa):
    lib = sa.lib()
    x = mdl.pm(300, 2, seed=1)
    want = mdl.encode_block(x[:512], 2, 256, 3, 8)
    buf = np.full(len(want) + 16, 0xa5, np.uint8)
    f = lib.sauAmd_flac_encode_block_lpc24
    assert f(x.ctypes.data, 256, 2, 256, 3, 8, buf.ctypes.data, len(want) - 1) == len(want)
    assert (buf == 0xa5).all()
    assert f(x.ctypes.data, 256, 2, 256, 3, 8, None, 1 << 20) == len(want)
    assert f(x.ctypes.data, 256, 2, 256, 3, 8, buf.ctypes.data, len(want)) == len(want)
    assert bytes(buf[:len(want)]) == want and (buf[len(want):] == 0xa5).all()
    p = x.ctypes.data
    for args in ((None, 256, 2, 256, 3, 8), (p, 0, 2, 256, 3, 8), (p, 257, 2, 256, 3, 8), (p, 256, 0, 256, 3, 8), (p, 256, 3, 256, 3, 8),
                 (p, 256, 2, 255, 3, 8), (p, 256, 2, 8192, 3, 8), (p, 256, 2, 256, 1 << 31, 8), (p, 256, 2, 256, 3, 9),
                 (p, 256, 2, 256, 3, 0xffffffff)):
        assert f(*args, buf.ctypes.data, len(buf)) == 0, args
    for bad in (8388608, -8388609, 1 << 30, -(1 << 31)):
        y = x.copy()
        y[77] = bad
        assert f(y.ctypes.data, 256, 2, 256, 3, 8, buf.ctypes.data, len(buf)) == 0, bad


def test_the_golden_stream_decodes_and_encodes_to_itself(sa):
    """the PM voice, 3 * 256 + 100 stereo frames at 44100 Hz in blocks of 256, 24 bits, M = 8, made by the model: for anyone with
    a decoder"""
    data = open(GOLDEN_FLAC, "rb").read()
    assert len(data) < 8192
    h, x, kinds = mdl.decode_file(data)
    assert (h["srate"], h["channels"], h["max_block"], h["frames"], h["bps"]) == (44100, 2, 256, 868, 24)
    assert (x == mdl.golden_samples()).all()
    assert all(k.startswith("lpc") for kd in kinds[:3] for k in kd) and not any(k.startswith("lpc") for k in kinds[3])
    frames, sizes = mdl.encode_stream(x, 2, 256, 8)
    assert mdl.header(44100, 2, 256, 868, min(sizes), max(sizes)) + frames == data
    host = b"".join(sa.flac_encode_block_lpc24(x[k * 512:(k + 1) * 512], 2, 256, k, 8) for k in range(4))
    assert sa.flac_header(44100, 2, 256, mdl.info(868, sizes), bits=24) + host == data


# ---- step 5b -------------------------------------------------------------------------------------------------------------------

def pole_autocorrelation(p):
    """R[0 .. 8] of the impulse response of 1 / (1 - p z^-1)^8, scaled to R[0] = 2^60"""
    h = np.zeros(4096)  # (the response has died away long before: 0.85^4096)
    h[0] = 1.0
    for _ in range(8):
        for i in range(1, len(h)):
            h[i] += p * h[i - 1]
    R = [float((h[l:] * h[:len(h) - l]).sum()) for l in range(9)]
    return [int(v * (2.0 ** 60 / R[0])) for v in R]


def guard_inputs(R, M):
    """steps 3 to 5 of the model for one autocorrelation -> (mask, q [64] as (m - 1) * 8 + j, shift [8])"""
    _, mask, cands, _, _, _ = l16.levinson(R, M)
    q, shift = np.zeros(64, np.int16), np.zeros(8, np.uint8)
    for m, (qq, sh) in cands.items():
        q[(m - 1) * 8:(m - 1) * 8 + m] = qq
        shift[m - 1] = sh
    return mask, q, shift


def run_guard(fn, items):
    """fn: sauAmd_kat_flac_lpc_guard_host or _device over [(mask, q, shift, bps)] -> the masks"""
    n = len(items)
    mask = np.array([it[0] for it in items], np.uint32)
    q = np.stack([it[1] for it in items]).astype(np.int16)
    shift = np.stack([it[2] for it in items]).astype(np.uint8)
    bps = np.array([it[3] for it in items], np.uint32)
    out = np.full(n, 0xa5a5a5a5, np.uint32)
    assert fn(mask.ctypes.data, q.ctypes.data, shift.ctypes.data, bps.ctypes.data, n, out.ctypes.data) == 1
    return [int(v) for v in out]


_guard_items = None


def guard_items():
    """[(mask, q, shift, bps)] and the model's answers: the pole vectors at both bps, then test_flac_lpc_steps_host's vectors at
    both bps -- the side that spares"""
    global _guard_items
    if _guard_items is None:
        items = []
        for p in POLES:
            mask, q, shift = guard_inputs(pole_autocorrelation(p), 8)
            items += [(mask, q, shift, 24), (mask, q, shift, 25)]
        n_pole = len(items)
        for (_, R, M), res in zip(steps.vectors(), steps.model_results()):
            q, shift = np.zeros(64, np.int16), np.zeros(8, np.uint8)
            for m, (qq, sh) in res[2].items():
                q[(m - 1) * 8:(m - 1) * 8 + m] = qq
                shift[m - 1] = sh
            items += [(res[1], q, shift, 24), (res[1], q, shift, 25)]
        want = [mdl.guard_mask(*it) for it in items]
        _guard_items = (items, want, n_pole)
    return _guard_items


def test_the_guard_vectors_fire_and_spare_at_both_widths():
    """which orders step 5b takes from the pole vectors: none up to p = 0.65; 7 and 8 at bps 25 from p = 0.7 on (sums of |c| of 65
    and 68.8 at p = 0.7); order 8 at bps 24 too at p = 0.85 (157.1), and nothing else there (order 7: 108.7 < 128)"""
    items, want, n_pole = guard_items()
    taken = {}
    for k, p in enumerate(POLES):
        assert items[2 * k][0] == 0xff  # all eight orders are candidates of steps 3 to 5
        for j, bps in enumerate((24, 25)):
            taken[(p, bps)] = [m for m in range(1, 9) if not want[2 * k + j] >> (m - 1) & 1]
    for p in (0.5, 0.55, 0.6, 0.65):
        assert taken[(p, 24)] == [] and taken[(p, 25)] == [], p
    for p in (0.7, 0.75, 0.8):
        assert taken[(p, 24)] == [] and taken[(p, 25)] == [7, 8], p
    assert taken[(0.85, 24)] == [8] and taken[(0.85, 25)] == [7, 8]
    # the sums themselves, from q and the shift: where the guard's line lies
    mask, q, shift = guard_inputs(pole_autocorrelation(0.7), 8)
    sums = [sum(abs(int(v)) for v in q[(m - 1) * 8:(m - 1) * 8 + m]) / 2.0 ** int(shift[m - 1]) for m in range(1, 9)]
    assert 48 < sums[5] < 49 and 64 < sums[6] < 66 and 68 < sums[7] < 70, sums
    # test_flac_lpc_steps_host's vectors never fire it: their largest sum of |c| is below 32
    assert all(w == it[0] for w, it in zip(want[n_pole:], items[n_pole:]))
    assert any(it[0] for it in items[n_pole:])


def test_the_hosts_guard_equals_the_model(guard_hooks):
    items, want, _ = guard_items()
    assert run_guard(guard_hooks.sauAmd_kat_flac_lpc_guard_host, items) == want
    # a mask bit that is not set stays unset, whatever q and the shift hold
    mask, q, shift = guard_inputs(pole_autocorrelation(0.85), 8)
    assert run_guard(guard_hooks.sauAmd_kat_flac_lpc_guard_host, [(0x55, q, shift, 25), (0, q, shift, 24)]) == [0x15, 0]


def test_a_stream_that_trips_the_guard(sa):
    """B = 256, L = s and R = -s with s the response of 1 / (1 - 0.7 z^-1)^8 from frame 64 on at full scale: the side channel's
    order 8 (a sum of |c| of 91.6) goes, L and R keep theirs"""
    x = mdl.guard_stream()
    assert int(np.abs(x).max()) == 8388607
    s = x[0::2].astype(np.int64)
    for sig, bps, left in ((s, 24, list(range(1, 9))), (-s, 24, list(range(1, 9))), (2 * s, 25, list(range(1, 8)))):
        cands = l16.orders(mdl.autocorrelation(sig, 256, 8), 8)
        assert sorted(cands) == list(range(1, 9)) and sorted(mdl.guard(cands, bps)) == left
        q, sh = cands[8]
        assert 91 < sum(abs(v) for v in q) / 2.0 ** sh < 92
    stat = {}
    frame, _ = mdl.encode_block(x, 2, 256, 0, 8, with_choice=True, stat=stat)
    assert stat["guarded"] == [(25, 8)]
    assert sa.flac_encode_block_lpc24(x, 2, 256, 0, 8) == frame
    got, _, _ = mdl.decode_frame(frame, 0, 2, 256, 0)
    assert (got.reshape(-1) == x).all()


# ---- refusals that need no device ----------------------------------------------------------------------------------------------

def test_an_lpc24_encoder_is_refused_by_a_backend_without_one(sa, seqexec):
    prg = load_program(sa, KEY)
    b = sa.Batch([prg], 12000, backend=seqexec.seq_backend_create(1016))
    with pytest.raises(RuntimeError, match="this backend has no float-fed FLAC encoder"):  # M = 0 is create_flac_f32 at 24 bits
        b.create_flac_lpc24(1, 2, 1024, 0)
    for M in (1, 8):
        with pytest.raises(RuntimeError, match="no LPC mode at 24 bits"):
            b.create_flac_lpc24(1, 2, 1024, M)
    for n_rows, ch, B, M in ((0, 1, 256, 8), (65536, 1, 256, 8), (1, 0, 256, 8), (1, 3, 256, 8), (1, 1, 255, 8), (1, 1, 8192, 8),
                             (1, 1, 256, 9), (1, 1, 256, -1)):
        with pytest.raises(RuntimeError, match="bad argument"):  # whatever the backend
            b.create_flac_lpc24(n_rows, ch, B, M)
    for M in (1, 8):  # the entry point that takes `bits` keeps refusing
        with pytest.raises(RuntimeError, match="bad argument"):
            b.create_flac_f32(1, 1, 256, bits=24, max_lpc_order=M)
    b.close()
    lib = sa.lib()
    assert not lib.sauAmd_Batch_create_flac_lpc24(None, 1, 1, 256, 8) and "bad argument" in sa.api.last_error(lib)


BAD_WRITER_ARGS = (dict(srate=0), dict(srate=655351), dict(channels=0), dict(channels=3), dict(block_frames=100), dict(block_frames=8192),
                   dict(max_lpc_order=9), dict(max_lpc_order=-1))


def test_render_file_flac_lpc24_refuses_before_there_is_a_file(sa, tmp_path):
    prg = load_program(sa, KEY)
    path = str(tmp_path / "x.flac")
    for bad in BAD_WRITER_ARGS + (dict(gain=float("nan")), dict(gain=float("inf")), dict(gain=-float("inf"))):
        a = dict(srate=8000, channels=1, block_frames=256, max_lpc_order=8, gain=0.5)
        a.update(bad)
        srate = a.pop("srate")
        with pytest.raises(RuntimeError, match="bad argument"):  # the arguments are looked at before any device
            sa.render_file_flac_lpc24(prg, srate, path, **a)
        assert not os.path.exists(path), bad
    lib = sa.lib()
    assert not lib.sauAmd_render_file_flac_lpc24(None, 8000, os.fsencode(path), 1, 256, 8, 1.0, None, None) and "bad argument" in sa.api.last_error(lib)
    assert not lib.sauAmd_render_file_flac_lpc24(prg.ptr, 8000, None, 1, 256, 8, 1.0, None, None) and "bad argument" in sa.api.last_error(lib)
    for M in (1, 8):  # the writer that takes `bits` keeps refusing
        with pytest.raises(RuntimeError, match="bad argument"):
            sa.render_file_flac_f32(prg, 8000, path, 1, 256, bits=24, max_lpc_order=M)
    assert not os.path.exists(path)


@pytest.mark.parametrize("limited", [False, True])
def test_render_file_flac_loudness_lpc24_refuses_before_there_is_a_file(sa, tmp_path, limited):
    prg = load_program(sa, KEY)
    path = str(tmp_path / "x.flac")
    for bad in BAD_WRITER_ARGS + (dict(srate=100), dict(target_lufs=float("nan")), dict(target_lufs=float("inf")), dict(max_true_peak=0.0),
                                  dict(max_true_peak=-1.0), dict(max_true_peak=float("nan")), dict(max_true_peak=float("inf"))):
        a = dict(srate=8000, channels=1, block_frames=256, max_lpc_order=8, target_lufs=-20.0, max_true_peak=0.9)
        a.update(bad)
        srate = a.pop("srate")
        with pytest.raises(RuntimeError, match="bad argument"):
            sa.render_file_flac_loudness_lpc24(prg, srate, path, limited=limited, **a)
        assert not os.path.exists(path), bad
    lib = sa.lib()
    assert not lib.sauAmd_render_file_flac_loudness_lpc24(None, 8000, os.fsencode(path), 1, 256, 8, -20.0, 1.0, int(limited),
                                                          None, None, None, None, None) and "bad argument" in sa.api.last_error(lib)
    for M in (1, 8):
        with pytest.raises(RuntimeError, match="bad argument"):
            sa.render_file_flac_loudness(prg, 8000, path, 1, 256, bits=24, max_lpc_order=M, limited=limited)
    assert not os.path.exists(path)
