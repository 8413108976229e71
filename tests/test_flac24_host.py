"""The 24-bit and float-fed FLAC encoder without a GPU (include/saugns_amd.h, section "FLAC", paragraph "24 bits":
sauAmd_flac_quantize, sauAmd_flac_header_bits, sauAmd_flac_encode_block_s32, sauAmd_render_file_flac_f32,
sauAmd_render_file_flac_loudness): the numpy restatement of that paragraph (tests/flac24_model.py) against its own independent
decoder, the library's host restatement (tables.cpp, built from sau_flac.h and sau_dev_math.h as the kernels are) against the
model -- the quantiser value for value, a frame byte for byte --, the header against hand-packed bytes, the committed golden
stream, the launch plan at 24 bits, and every refusal that needs no device, the writers' over the sequential test executor
(tests/seqexec keeps engine.h's refusing defaults). tests/test_gpu_flac24.py compares the device with the host restatement."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import flac24_model as mdl
import flac_lpc_model as lpc16
from conftest import GOLDEN, ROOT, load_program

KEY = "devtests__voice-reuse"
GOLDEN_FLAC = os.path.join(GOLDEN, mdl.GOLDEN_NAME)
NUMBERS = [0, 127, 128, 2047, 2048, 65535, 65536, (1 << 31) - 1]


@pytest.fixture(scope="module")
def flac24_hooks(sa, hooks):
    """tests/hooks_flac24/libsaugns_amd_flac24_hooks.so: the product's object files (the `hooks` fixture has built them) + the
    float-fed FLAC writers over injected backends and the encoder's launch plan at a sample width"""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "hooks_flac24")])
    return sa.api.use_flac24_hooks(os.path.join(ROOT, "tests", "hooks_flac24", "libsaugns_amd_flac24_hooks.so"))


def lengths(B):
    return [1, 4, 5, 255, B]


_cases = {}


def cases(B):
    """(kind, channels, n, frame number, samples, the model's frame, its choices): computed once per B"""
    if B not in _cases:
        out = []
        for ch in (1, 2):
            for i, kind in enumerate(mdl.KINDS):
                for j, n in enumerate(lengths(B)):
                    x = mdl.crafted(kind, n, ch, seed=i, B=B)
                    number = NUMBERS[(i + j) % len(NUMBERS)]
                    frame, choice = mdl.encode_block(x, ch, B, number, with_choice=True)
                    out.append((kind, ch, n, number, x, frame, choice))
        _cases[B] = out
    return _cases[B]


# ---- the quantiser ---------------------------------------------------------------------------------------------------------

def f32_next(x, up):
    return np.nextafter(np.float32(x), np.float32(np.inf if up else -np.inf), dtype=np.float32)


def ties16():
    """float32 y whose f32 product y * 32767 is exactly j + 0.5, for even and for odd j (the 16-bit quantiser's ties)"""
    out = {0: [], 1: []}
    for j in range(0, 16384):
        y = np.float32((j + 0.5) / 32767.0)
        if np.float32(y * np.float32(32767)) == j + 0.5:
            out[j & 1].append(y)
    assert len(out[0]) > 100 and len(out[1]) > 100
    return np.array(out[0][:200] + out[1][:200], np.float32)


def quantiser_inputs():
    """+-0, +-1, +-(1 + ulp), +-inf, NaN, the ties, subnormals, and a spread of ordinary values. A 24-bit tie needs
    y * 8388607 = j + 0.5 with y a float, and 8388607 is odd, so y = q / 2 with q odd: inside the clamp only y = +-0.5, whose
    product 4194303.5 lies below an even integer. The other parity exists for the 16-bit quantiser only (ties16: the product is
    rounded to f32 first), and is taken there."""
    one_up = f32_next(1.0, True)
    near = [f32_next(0.5, True), f32_next(0.5, False), -f32_next(0.5, True), -f32_next(0.5, False)]
    sub = [np.float32(1e-45), np.float32(-1e-45), np.float32(1e-40), np.float32(-5.8e-39)]
    rng = np.random.default_rng(24)
    spread = rng.uniform(-1.2, 1.2, 4000).astype(np.float32)
    special = np.array([0.0, -0.0, 1.0, -1.0, one_up, -one_up, np.inf, -np.inf, np.nan, 0.5, -0.5] + near + sub, np.float32)
    t = ties16()
    return np.concatenate([special, t, -t, spread])


def test_the_quantiser_against_the_model(sa):
    x = quantiser_inputs()
    for bits in (24, 16):
        for gain in (1.0, 0.5, -1.0, 0.9999999, 3.0, 0.0, 2.0 ** 125, 1e39):  # (1e39 overflows to inf as a float)
            got = sa.flac_quantize(x, gain, bits)
            with np.errstate(over="ignore"):
                want = mdl.quantize(x, np.float32(gain), bits)
            bad = got != want
            assert not bad.any(), (bits, gain, x[bad][:8], got[bad][:8], want[bad][:8])
    up = f32_next(1.0, True)
    q = sa.flac_quantize(np.array([0.0, -0.0, 1.0, -1.0, up, -up, np.inf, -np.inf, np.nan], np.float32), 1.0, 24)
    assert q.tolist() == [0, 0, 8388607, -8388607, 8388607, -8388607, 8388607, -8388607, -8388607]
    # ties go to even: 0.5 * 8388607 = 4194303.5, and 16383.5 at 16 bits
    assert sa.flac_quantize(np.array([0.5, -0.5], np.float32), 1.0, 24).tolist() == [4194304, -4194304]
    assert sa.flac_quantize(np.array([0.5, -0.5], np.float32), 1.0, 16).tolist() == [16384, -16384]
    t = ties16()
    got = sa.flac_quantize(t, 1.0, 16)
    lo = np.floor((t * np.float32(32767)).astype(np.float32).astype(np.float64))  # the products are j + 0.5 exactly
    want = np.where(lo % 2 == 0, lo, lo + 1)
    assert (got == want).all() and (want == lo).any() and (want == lo + 1).any()  # both parities of j: down and up
    # a gain that overflows to inf: inf * 0 is a NaN -> -1; inf * x clamps to the sign's rail
    assert sa.flac_quantize(np.array([0.0, 1e-30, -1e-30], np.float32), np.inf, 24).tolist() == [-8388607, 8388607, -8388607]
    # subnormals are not flushed: 1e-40 * 2^125 is an ordinary value
    one = sa.flac_quantize(np.array([1e-40], np.float32), 2.0 ** 125, 24).tolist()
    assert one == mdl.quantize(np.array([1e-40], np.float32), 2.0 ** 125).tolist() and one != [0]
    assert np.abs(sa.flac_quantize(x, 7.0, 24)).max() == 8388607  # never -2^23
    for bits in (0, 8, 15, 17, 23, 25, 32, -24):
        assert sa.flac_quantize(x, 1.0, bits) is None
    lib = sa.lib()
    assert not lib.sauAmd_flac_quantize(None, 4, 1.0, 24, None)
    assert lib.sauAmd_flac_quantize(None, 0, 1.0, 24, None)  # nothing to do


def test_the_gain_is_one_f32_multiply(sa):
    """x * gain is rounded to f32 before the clamp and the scaling: gains that are no powers of two, on values near the ties"""
    x = np.array([1.5, -1.5, 0.75, 0.25, 1.0, 3.0, 0.1], np.float32)
    for gain in (np.float32(1) / np.float32(3), np.float32(2) / np.float32(3), np.float32(2), np.float32(0.5), np.float32(0.1)):
        for bits in (16, 24):
            assert (sa.flac_quantize(x, gain, bits) == mdl.quantize(x, gain, bits)).all(), (gain, bits)


# ---- the model ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [256, 4096])
def test_the_model_decodes_what_it_encodes_and_chooses_what_the_inputs_are_crafted_for(B):
    seen = set()
    for kind, ch, n, number, x, frame, (assign, an) in cases(B):
        got, end, kd = mdl.decode_frame(frame, 0, ch, B, number)
        assert end == len(frame) and (got.reshape(-1) == x).all(), (kind, ch, n)
        assert len(frame) <= mdl.frame_bound(n, ch)
        assert [k[0] for k in kd] == [a["type"] for a in an]
        seen.add(assign)
        ks = [k for a in an if a["type"] == "fixed" for k in a["ks"]]
        if kind == "constant" or n == 1:
            assert all(a["type"] == "constant" for a in an), (kind, ch, n, an)
        if kind == "rails" and n >= 255:
            assert all(a["type"] == "verbatim" for a in an) and len(frame) > 3 * n * ch, (ch, n, an)
        if kind == "anti_rails" and ch == 2 and n >= 4:  # the mid is constant 0, the side +-16777214: all 25 bits, verbatim
            assert assign == "MS" and an[0] == dict(type="constant", bits=8 + 24) and an[1] == dict(type="verbatim", bits=8 + 25 * n), (n, an)
            assert sorted(set((x[0::2].astype(np.int64) - x[1::2]).tolist())) == [-16777214, 16777214]
        if kind == "quiet_sine" and n >= 255:
            assert ks and max(ks) <= 14, (ch, n, ks)
        if kind == "noise" and n >= 255:  # a parameter capped at 14 could not code this
            assert ks and max(ks) >= 15 and all(a["type"] == "fixed" for a in an), (ch, n, an)
        if kind == "one_loud" and n == B:
            for a in an:
                if a["type"] == "fixed":
                    assert a["p"] == 4 and min(a["ks"]) == 0 and max(a["ks"]) >= 20, a
            assert any(a["type"] == "fixed" for a in an)
    assert seen >= {"mono", "LR", "MS"}


def test_the_decoder_refuses_what_the_paragraph_excludes():
    B = 256
    x = mdl.crafted("noise", B + 9, 2)
    data, sizes = mdl.encode_stream(x, 2, B)
    mdl.decode_frames(data, 2, B)

    def broken(at, xor):
        b = bytearray(data)
        b[at] ^= xor
        return bytes(b)

    for what, d in (("sync", broken(1, 0x01)), ("the sample size code", broken(3, 0x04)), ("CRC-8", broken(4, 0x01)),
                    ("CRC-16", broken(sizes[0] - 1, 0x80)), ("a body bit", broken(sizes[0] // 2, 0x10)),
                    ("cut short", data[:-1]), ("bytes behind", data + b"\0")):
        with pytest.raises((mdl.Bad, ValueError, IndexError)):
            mdl.decode_frames(d, 2, B)
    import flac_model as m16  # a 16-bit stream is no 24-bit one, and the other way round
    with pytest.raises(mdl.Bad):
        mdl.decode_frames(m16.encode_stream(m16.crafted("sine", B, 2), 2, B)[0], 2, B)
    with pytest.raises(m16.Bad):
        m16.decode_frames(data, 2, B)


# ---- the library's host restatement -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [256, 4096])
def test_the_hosts_block_equals_the_model_byte_for_byte(sa, B):
    for kind, ch, n, number, x, frame, _ in cases(B):
        got = sa.flac_encode_block_s32(x, ch, B, number, bits=24)
        assert got == frame, (kind, ch, n, number, len(got), len(frame))
        assert len(got) <= 15 + ch * (1 + 3 * n)
    x = mdl.crafted("noise", 4096, 2)
    assert sa.flac_encode_block_s32(x, 2, 0, 7) == mdl.encode_block(x, 2, 4096, 7)  # 0 means 4096
    # samples the quantiser never makes: -2^23 and 2^23 - 1 are inside the format
    x = np.array([-8388608, 8388607] * 128, np.int32)
    assert sa.flac_encode_block_s32(x, 2, 256, 1) == mdl.encode_block(x, 2, 256, 1)
    got, _, _ = mdl.decode_frame(sa.flac_encode_block_s32(x, 2, 256, 1), 0, 2, 256, 1)
    assert (got.reshape(-1) == x).all()


@pytest.mark.parametrize("M", [0, 8])
def test_16_bits_is_the_int16_encoders_frame(sa, M):
    for B, n, ch, kind in ((256, 256, 2, "sine"), (256, 100, 1, "burst"), (4096, 4096, 2, "unrelated"), (1024, 1024, 1, "steps")):
        import flac_model as m16
        x = m16.crafted(kind, n, ch, seed=3)
        want = sa.flac_encode_block(x, ch, B, 5, max_lpc_order=M)
        assert want and sa.flac_encode_block_s32(x.astype(np.int32), ch, B, 5, bits=16, max_lpc_order=M) == want
        assert want == lpc16.encode_block(x, ch, B, 5, M)
    x = np.array([32768, 0, 0, 0], np.int32)
    assert sa.flac_encode_block_s32(x, 1, 256, 0, bits=16, max_lpc_order=M) == b""  # beyond int16
    x = np.array([-32769, 0, 0, 0], np.int32)
    assert sa.flac_encode_block_s32(x, 2, 256, 0, bits=16, max_lpc_order=M) == b""


def test_a_short_cap_writes_nothing_and_bad_arguments_give_0(sa):
    lib = sa.lib()
    x = mdl.crafted("noise", 300, 2)
    want = mdl.encode_block(x[:512], 2, 256, 3)
    buf = np.full(len(want) + 16, 0xa5, np.uint8)
    f = lib.sauAmd_flac_encode_block_s32
    assert f(x.ctypes.data, 256, 2, 256, 3, 24, 0, buf.ctypes.data, len(want) - 1) == len(want)
    assert (buf == 0xa5).all()
    assert f(x.ctypes.data, 256, 2, 256, 3, 24, 0, None, 1 << 20) == len(want)
    assert f(x.ctypes.data, 256, 2, 256, 3, 24, 0, buf.ctypes.data, len(want)) == len(want)
    assert bytes(buf[:len(want)]) == want and (buf[len(want):] == 0xa5).all()
    p = x.ctypes.data
    for args in ((None, 256, 2, 256, 3, 24, 0), (p, 0, 2, 256, 3, 24, 0), (p, 257, 2, 256, 3, 24, 0), (p, 256, 0, 256, 3, 24, 0),
                 (p, 256, 3, 256, 3, 24, 0), (p, 256, 2, 255, 3, 24, 0), (p, 256, 2, 8192, 3, 24, 0), (p, 256, 2, 256, 1 << 31, 24, 0),
                 (p, 256, 2, 256, 3, 24, 1), (p, 256, 2, 256, 3, 24, 8), (p, 256, 2, 256, 3, 24, 9), (p, 256, 2, 256, 3, 16, 9),
                 (p, 256, 2, 256, 3, 20, 0), (p, 256, 2, 256, 3, 32, 0), (p, 256, 2, 256, 3, 0, 0),
                 (p, 256, 2, 256, 3, 16, 0)):  # (the last: these samples do not fit int16)
        assert f(*args, buf.ctypes.data, len(buf)) == 0, args
    for bad in (8388608, -8388609, 1 << 30, -(1 << 31)):
        y = x.copy()
        y[77] = bad
        assert f(y.ctypes.data, 256, 2, 256, 3, 24, 0, buf.ctypes.data, len(buf)) == 0, bad


def test_the_header_against_hand_packed_bytes(sa):
    info = dict(frames=0x9_8765_4321, blocks=3, bytes=99, min_frame_bytes=0x0e, max_frame_bytes=0x123456)
    got = sa.flac_header(44100, 2, 1024, info, bits=24)
    want = bytes.fromhex("664c6143" "80000022" "0400" "0400" "00000e" "123456"
                         # 44100 = 0x0ac44 in 20 bits, 001 (channels - 1), 10111 (bits - 1 = 23), then 36 bits of frames
                         "0ac44" "37" "987654321") + bytes(16)
    assert len(want) == 42 and got == want
    assert got == mdl.header(44100, 2, 1024, info["frames"], 0x0e, 0x123456)
    h = mdl.parse_header(got)
    assert (h["srate"], h["channels"], h["bps"], h["frames"], h["min_block"], h["max_block"]) == (44100, 2, 24, info["frames"], 1024, 1024)
    assert sa.flac_header(44100, 2, 1024, info, bits=16) == sa.flac_header(44100, 2, 1024, info)
    assert sa.flac_header(655350, 1, 0, bits=24) == mdl.header(655350, 1, 4096)  # 0 means 4096; no record: an empty one
    for args in ((0, 1, 256), (655351, 1, 256), (8000, 0, 256), (8000, 3, 256), (8000, 1, 100), (8000, 1, 8192)):
        assert sa.flac_header(*args, bits=24) == b"", args
    for bits in (0, 8, 15, 17, 20, 23, 25, 32):
        assert sa.flac_header(8000, 1, 256, bits=bits) == b"", bits
    lib = sa.lib()
    buf = np.full(64, 0xa5, np.uint8)
    assert lib.sauAmd_flac_header_bits(8000, 1, 256, 24, None, buf.ctypes.data, 41) == 42 and (buf == 0xa5).all()
    assert lib.sauAmd_flac_header_bits(8000, 1, 256, 24, None, None, 0) == 42
    assert lib.sauAmd_flac_header_bits(8000, 1, 256, 24, None, buf.ctypes.data, 42) == 42 and (buf[42:] == 0xa5).all()


def test_the_golden_stream_decodes_and_encodes_to_itself(sa):
    """noise in +-0.25 left and a sine right, 3 * 256 + 100 stereo frames at 44100 Hz in blocks of 256, 24 bits, made by the model:
    for anyone with a decoder"""
    data = open(GOLDEN_FLAC, "rb").read()
    assert len(data) < 32768
    h, x = mdl.decode_file(data)
    assert (h["srate"], h["channels"], h["max_block"], h["frames"], h["bps"]) == (44100, 2, 256, 868, 24)
    assert (x == mdl.golden_samples()).all()
    frames, sizes = mdl.encode_stream(x, 2, 256)
    assert mdl.header(44100, 2, 256, 868, min(sizes), max(sizes)) + frames == data
    host = b"".join(sa.flac_encode_block_s32(x[k * 512:(k + 1) * 512], 2, 256, k) for k in range(4))
    assert sa.flac_header(44100, 2, 256, mdl.info(868, sizes), bits=24) + host == data


# ---- the launch plan at 24 bits ----------------------------------------------------------------------------------------------

def plan(hooks_lib, B, ch, bits, pos, frames, finish):
    n = len(pos)
    out = (C.c_uint64 * 8)()
    ok = hooks_lib.sauAmd_flac_plan_bits(B, ch, bits, n, (C.c_uint64 * n)(*pos), (C.c_uint32 * n)(*frames), 1 if finish else 0, out)
    return ok, dict(zip(("B", "jobs", "analyze_threads", "analyze_lds", "write_lds", "pend_pitch", "worst", "out_bytes"), out))


@pytest.mark.parametrize("B", [256, 1024, 4096])
@pytest.mark.parametrize("ch", [1, 2])
def test_the_plan_at_24_bits(flac24_hooks, B, ch):
    ok, out = plan(flac24_hooks, B, ch, 24, [0, B - 1], [3 * B + 37, B + 2], True)
    assert ok == 1
    sizes = [[B, B, B, 37], [B, B, 1]]  # (the second row stood at B - 1: it completes the blocks 0 and 1 and a tail of 1)
    assert out["jobs"] == 7 and out["worst"] == sum(15 + ch * (1 + 3 * n) for s in sizes for n in s)
    assert out["analyze_threads"] == (256 if ch == 2 else 64) and out["pend_pitch"] == B * ch
    assert out["analyze_lds"] == 4 * ch * (B + B // 32)  # L and R apart, a word per sample
    assert out["write_lds"] == out["analyze_lds"] + 4 * ((15 + ch * (1 + 3 * B)) // 4 + 2)
    # (+ the kernels' static LDS: s_fine [4][16 * 31] of 8 bytes, the nodes, the candidates' records)
    assert out["write_lds"] + 256 <= 65536 and out["analyze_lds"] + 4 * 16 * 31 * 8 + 4 * 32 * 9 + 4 * 44 <= 65536
    ok16, out16 = plan(flac24_hooks, B, ch, 16, [0, B - 1], [3 * B + 37, B + 2], True)
    assert ok16 == 1 and out16["analyze_lds"] == 4 * (B + B // 32) and out16["worst"] == sum(15 + ch * (1 + 2 * n) for s in sizes for n in s)
    assert plan(flac24_hooks, B, ch, 20, [0], [B], True)[0] == 0


def test_the_1_gib_rule_uses_the_24_bit_bound(flac24_hooks):
    """2^21 mono blocks of 256 frames are 2^21 * 528 bytes at the 16-bit bound and 2^21 * 784 at the 24-bit one"""
    assert plan(flac24_hooks, 256, 1, 24, [0], [(1 << 30) // 784 * 256], False)[0] == 1
    assert plan(flac24_hooks, 256, 1, 24, [0], [((1 << 30) // 784 + 1) * 256], False)[0] == 0
    assert plan(flac24_hooks, 256, 1, 16, [0], [((1 << 30) // 784 + 1) * 256], False)[0] == 1  # the 16-bit bound still admits it


# ---- refusals over the sequential executor -------------------------------------------------------------------------------

def test_a_float_fed_encoder_is_refused_by_a_backend_without_one(sa, seqexec):
    prg = load_program(sa, KEY)
    b = sa.Batch([prg], 12000, backend=seqexec.seq_backend_create(1016))
    for bits, M in ((24, 0), (16, 0), (16, 8)):
        with pytest.raises(RuntimeError, match="this backend has no float-fed FLAC encoder"):
            b.create_flac_f32(1, 2, 1024, bits=bits, max_lpc_order=M)
    for n_rows, ch, B, bits, M in ((0, 1, 256, 24, 0), (65536, 1, 256, 24, 0), (1, 0, 256, 24, 0), (1, 3, 256, 24, 0), (1, 1, 255, 24, 0),
                                   (1, 1, 8192, 24, 0), (1, 1, 256, 20, 0), (1, 1, 256, 0, 0), (1, 1, 256, 32, 0), (1, 1, 256, 24, 1),
                                   (1, 1, 256, 24, 8), (1, 1, 256, 16, 9), (1, 1, 256, 24, 9)):
        with pytest.raises(RuntimeError, match="bad argument"):  # whatever the backend
            b.create_flac_f32(n_rows, ch, B, bits=bits, max_lpc_order=M)
    b.close()
    lib = sa.lib()
    assert not lib.sauAmd_Flac_feed_f32(None, None, 0, None, None, 0) and "bad argument" in sa.api.last_error(lib)


BAD_WRITER_ARGS = (dict(srate=0), dict(srate=655351), dict(channels=0), dict(channels=3), dict(block_frames=100), dict(block_frames=8192),
                   dict(bits=0), dict(bits=20), dict(bits=32), dict(bits=24, max_lpc_order=1), dict(bits=24, max_lpc_order=8),
                   dict(bits=16, max_lpc_order=9))


def test_render_file_flac_f32_refuses_before_there_is_a_file(sa, seqexec, flac24_hooks, tmp_path):
    prg = load_program(sa, KEY)
    path = str(tmp_path / "x.flac")
    # the sequential executor has no float output, and no float-fed encoder either: the first of the two is what it says
    with pytest.raises(RuntimeError, match="float|FLAC encoder"):
        sa.render_file_flac_f32(prg, 8000, path, 2, 1024, bits=24, backend=seqexec.seq_backend_create(1016))
    assert not os.path.exists(path)
    for bad in BAD_WRITER_ARGS + (dict(gain=float("nan")), dict(gain=float("inf")), dict(gain=-float("inf"))):
        a = dict(srate=8000, channels=1, block_frames=256, bits=24, max_lpc_order=0, gain=0.5)
        a.update(bad)
        srate = a.pop("srate")
        with pytest.raises(RuntimeError, match="bad argument"):
            sa.render_file_flac_f32(prg, srate, path, backend=seqexec.seq_backend_create(1016), **a)
        with pytest.raises(RuntimeError, match="bad argument"):  # the product's own entry point looks at them before any device
            sa.render_file_flac_f32(prg, srate, path, **a)
        assert not os.path.exists(path), bad
    lib = sa.lib()
    assert not lib.sauAmd_render_file_flac_f32(None, 8000, os.fsencode(path), 1, 256, 24, 0, 1.0, None, None) and "bad argument" in sa.api.last_error(lib)
    assert not lib.sauAmd_render_file_flac_f32(prg.ptr, 8000, None, 1, 256, 24, 0, 1.0, None, None) and "bad argument" in sa.api.last_error(lib)


@pytest.mark.parametrize("limited", [False, True])
def test_render_file_flac_loudness_refuses_before_there_is_a_file(sa, seqexec, flac24_hooks, tmp_path, limited):
    prg = load_program(sa, KEY)
    path = str(tmp_path / "x.flac")
    with pytest.raises(RuntimeError, match="float|loudness"):  # pass 1 needs float output and the loudness meter
        sa.render_file_flac_loudness(prg, 8000, path, 2, 1024, bits=24, limited=limited,
                                     backends=(seqexec.seq_backend_create(1016), seqexec.seq_backend_create(1016)))
    assert not os.path.exists(path)
    for bad in BAD_WRITER_ARGS + (dict(srate=100), dict(target_lufs=float("nan")), dict(target_lufs=float("inf")), dict(max_true_peak=0.0),
                                  dict(max_true_peak=-1.0), dict(max_true_peak=float("nan")), dict(max_true_peak=float("inf"))):
        a = dict(srate=8000, channels=1, block_frames=256, bits=24, max_lpc_order=0, target_lufs=-20.0, max_true_peak=0.9)
        a.update(bad)
        srate = a.pop("srate")
        with pytest.raises(RuntimeError, match="bad argument"):
            sa.render_file_flac_loudness(prg, srate, path, limited=limited,
                                         backends=(seqexec.seq_backend_create(1016), seqexec.seq_backend_create(1016)), **a)
        with pytest.raises(RuntimeError, match="bad argument"):
            sa.render_file_flac_loudness(prg, srate, path, limited=limited, **a)
        assert not os.path.exists(path), bad
    lib = sa.lib()
    assert not lib.sauAmd_render_file_flac_loudness(None, 8000, os.fsencode(path), 1, 256, 24, 0, -20.0, 1.0, int(limited),
                                                    None, None, None, None, None) and "bad argument" in sa.api.last_error(lib)
