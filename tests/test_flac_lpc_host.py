"""The FLAC encoder's LPC mode without a GPU (include/saugns_amd.h, section "FLAC", "The LPC mode":
sauAmd_flac_encode_block_lpc, and the refusals of sauAmd_Batch_create_flac_lpc and sauAmd_render_file_flac_lpc): the library's
host restatement (tables.cpp, built from sau_flac.h as the kernels are) against the numpy restatement of the header's text
(tests/flac_lpc_model.py) byte for byte, every frame through the model's independent decoder, the invariants the scheme
promises -- M = 0 is today's encoder, no frame grows -- and the committed golden stream. tests/test_gpu_flac_lpc.py compares
the device with the model."""
import os

import numpy as np
import pytest

import flac_lpc_model as mdl
from conftest import GOLDEN, load_program

KEY = "devtests__voice-reuse"
GOLDEN_FLAC = os.path.join(GOLDEN, "flac_lpc_pm_stereo_b256.flac")
ORDERS = (1, 5, 8)

_cases = {}


def cases(B):
    """(name, channels, n, frame number, samples): every kind of flac_model.KINDS, pm, the side of +-65535 and the quiet sine,
    mono and stereo, a whole block and a short one"""
    if B not in _cases:
        out = []
        numbers = [0, 127, 128, 2047, 2048, 65535, 65536, (1 << 31) - 1]
        i = 0
        for ch in (1, 2):
            for n in (B, B - 1 if B == 256 else 1000):
                mats = [(k, mdl.crafted(k, n, ch, seed=j)) for j, k in enumerate(mdl.KINDS)]
                mats.append(("pm", mdl.pm(n, ch, seed=2)))
                mats.append(("quiet", mdl.quiet_sine(n, ch)))
                if ch == 2:
                    mats.append(("side", mdl.side_extremes(n)))
                for name, x in mats:
                    out.append((name, ch, n, numbers[i % len(numbers)], x))
                    i += 1
        _cases[B] = out
    return _cases[B]


def encode(sa, x, ch, B, number, M):
    return sa.flac_encode_block(x, ch, B, number, max_lpc_order=M)


@pytest.mark.parametrize("B", [256, 4096])
@pytest.mark.parametrize("M", ORDERS)
def test_the_hosts_lpc_block_equals_the_model_and_decodes(sa, B, M):
    kinds = set()
    for name, ch, n, number, x in cases(B):
        want, (_, an) = mdl.encode_block(x, ch, B, number, M, with_choice=True)
        got = encode(sa, x, ch, B, number, M)
        assert got == want, (name, ch, n, M, len(got), len(want), [a["type"] for a in an])
        back, end, kd = mdl.decode_frame(got, 0, ch, B, number)
        assert end == len(got) and (back.reshape(-1) == x).all(), (name, ch, n, M)
        assert len(got) <= mdl.frame_bound(n, ch)
        kinds.update(k.split("/")[0] for k in kd)
        if n != B:
            assert not any(k.startswith("lpc") for k in kd)
        for a in an:
            if a["type"] == "lpc":
                assert 1 <= a["order"] <= M and 0 <= a["shift"] <= 15 and all(-2048 <= q <= 2047 for q in a["q"])
    assert {"constant", "verbatim"} <= kinds and any(k.startswith("fixed") for k in kinds), kinds
    orders = {int(k[3:]) for k in kinds if k.startswith("lpc")}
    assert orders and max(orders) <= M and (M == 1 or max(orders) > 1), kinds


def test_the_highest_order_is_reached(sa):
    x = mdl.crafted("anti", 4096, 1, seed=2)
    want, (_, an) = mdl.encode_block(x, 1, 4096, 9, 8, with_choice=True)
    assert an[0]["type"] == "lpc" and an[0]["order"] == 8
    got = encode(sa, x, 1, 4096, 9, 8)
    assert got == want and (mdl.decode_frame(got, 0, 1, 4096, 9)[0].reshape(-1) == x).all()


@pytest.mark.parametrize("B", [256, 4096])
def test_order_0_is_todays_encoder_and_no_frame_grows(sa, B):
    for name, ch, n, number, x in cases(B):
        base = sa.flac_encode_block(x, ch, B, number)
        assert encode(sa, x, ch, B, number, 0) == base, (name, ch, n)
        assert mdl.encode_block(x, ch, B, number, 0) == base
        for M in range(1, 9):
            got = encode(sa, x, ch, B, number, M)
            assert 0 < len(got) <= len(base), (name, ch, n, M, len(got), len(base))
            if name == "noise" or n != B:
                assert got == base, (name, ch, n, M)


def test_pm_at_4096_is_all_lpc_and_shorter(sa):
    B, M = 4096, 8
    for ch in (1, 2):
        x = mdl.pm(2 * B + 100, ch, seed=3)
        a = b"".join(encode(sa, x[k * B * ch:(k + 1) * B * ch], ch, B, k, M) for k in range(3))
        b = b"".join(sa.flac_encode_block(x[k * B * ch:(k + 1) * B * ch], ch, B, k) for k in range(3))
        back, sizes, kinds = mdl.decode_frames(a, ch, B)
        assert (back == x).all()
        assert all(k.startswith("lpc") for kd in kinds[:2] for k in kd), kinds
        assert not any(k.startswith("lpc") for k in kinds[2]), kinds
        assert len(a) < len(b)
        print("pm, %d channel(s): %.2f bits per sample with LPC, %.2f without" % (ch, 8 * len(a) / len(x), 8 * len(b) / len(x)))


def test_bad_arguments_are_refused(sa, seqexec, tmp_path):
    lib = sa.lib()
    x = mdl.pm(256, 2)
    buf = np.full(4096, 0xa5, np.uint8)
    want = mdl.encode_block(x, 2, 256, 3, 8)
    assert lib.sauAmd_flac_encode_block_lpc(x.ctypes.data, 256, 2, 256, 3, 8, buf.ctypes.data, len(want) - 1) == len(want)
    assert (buf == 0xa5).all()  # a short cap writes nothing
    assert lib.sauAmd_flac_encode_block_lpc(x.ctypes.data, 256, 2, 256, 3, 8, None, 0) == len(want)
    assert lib.sauAmd_flac_encode_block_lpc(x.ctypes.data, 256, 2, 256, 3, 8, buf.ctypes.data, len(buf)) == len(want)
    assert bytes(buf[:len(want)]) == want and (buf[len(want):] == 0xa5).all()
    for args in ((x.ctypes.data, 256, 2, 256, 3, 9), (x.ctypes.data, 256, 2, 256, 3, 0xffffffff), (None, 256, 2, 256, 3, 8),
                 (x.ctypes.data, 0, 2, 256, 3, 8), (x.ctypes.data, 257, 2, 256, 3, 8), (x.ctypes.data, 256, 3, 256, 3, 8),
                 (x.ctypes.data, 256, 2, 255, 3, 8), (x.ctypes.data, 256, 2, 256, 1 << 31, 8)):
        assert lib.sauAmd_flac_encode_block_lpc(*args, buf.ctypes.data, len(buf)) == 0, args
    assert sa.flac_encode_block(x, 2, 256, 3, max_lpc_order=9) == b""
    prg = load_program(sa, KEY)
    b = sa.Batch([prg], 12000, backend=seqexec.seq_backend_create(1016))
    with pytest.raises(RuntimeError, match="bad argument"):
        b.create_flac(1, 2, 1024, max_lpc_order=9)
    with pytest.raises(RuntimeError, match="bad argument"):
        b.create_flac(0, 2, 1024, max_lpc_order=8)
    with pytest.raises(RuntimeError, match="FLAC encoder"):  # engine.h's default refuses M > 0, and forwards M = 0 to create_flac
        b.create_flac(1, 2, 1024, max_lpc_order=8)
    with pytest.raises(RuntimeError, match="this backend has no FLAC encoder"):
        b.create_flac(1, 2, 1024, max_lpc_order=0)
    b.close()
    path = str(tmp_path / "x.flac")
    for a in (dict(max_lpc_order=9), dict(max_lpc_order=8, srate=0), dict(max_lpc_order=8, channels=3), dict(max_lpc_order=1, block_frames=100)):
        kw = dict(srate=8000, channels=1, block_frames=256)
        kw.update(a)
        with pytest.raises(RuntimeError, match="bad argument"):  # looked at before any device or file
            sa.render_file_flac(prg, kw["srate"], path, kw["channels"], kw["block_frames"], max_lpc_order=kw["max_lpc_order"])
        assert not os.path.exists(path)
    assert not lib.sauAmd_render_file_flac_lpc(None, 8000, os.fsencode(path), 1, 256, 8, None, None) and "bad argument" in sa.api.last_error(lib)
    assert not lib.sauAmd_render_file_flac_lpc(prg.ptr, 8000, None, 1, 256, 8, None, None) and "bad argument" in sa.api.last_error(lib)
    assert not os.path.exists(path)


def test_the_decoder_refuses_what_the_lpc_mode_excludes():
    """the model's own decoder only (no code of the library runs here): a frame with one field changed and the CRC-16 made
    right again is refused by the check that field belongs to, not by a parser that lost its way"""
    B = 256
    x = mdl.pm(B, 1)
    frame, (_, an) = mdl.encode_block(x, 1, B, 0, 8, with_choice=True)
    assert an[0]["type"] == "lpc"
    m = an[0]["order"]
    mdl.decode_frame(frame, 0, 1, B, 0)
    head = 8 * 6  # sync and codes, the number, the CRC-8
    at = head + 8 + 16 * m  # the precision code

    def with_bits(pos, width, value):
        v = int.from_bytes(frame[:-2], "big")
        total = 8 * (len(frame) - 2)
        v &= ~(((1 << width) - 1) << (total - pos - width))
        v |= value << (total - pos - width)
        body = v.to_bytes(len(frame) - 2, "big")
        return body + mdl.crc16(body).to_bytes(2, "big")

    assert with_bits(at, 4, 0b1011) == frame
    for what, d in (("coefficient precision code", with_bits(at, 4, 0b1010)), ("coefficient precision code", with_bits(at, 4, 0b1111)),
                    ("LPC shift -1", with_bits(at + 4, 5, 0b11111)), ("LPC shift -16", with_bits(at + 4, 5, 16)),
                    ("LPC order 9", with_bits(head, 8, (0b100000 | 8) << 1)), ("LPC order 32", with_bits(head, 8, 0b111111 << 1)),
                    ("subframe type 16", with_bits(head, 8, 0b010000 << 1))):
        with pytest.raises(mdl.Bad, match="^%s$" % what):
            mdl.decode_frame(d, 0, 1, B, 0)


def test_the_golden_lpc_stream_decodes_and_encodes_to_itself(sa):
    """868 stereo frames of pm at 44100 Hz in blocks of 256 with max_lpc_order 8, made by the model: for anyone with a decoder"""
    data = open(GOLDEN_FLAC, "rb").read()
    assert len(data) <= 8192
    h, x, kinds = mdl.decode_file(data)
    assert (h["srate"], h["channels"], h["max_block"], h["frames"]) == (44100, 2, 256, 868)
    assert np.abs(x.astype(int) - mdl.pm(868, 2, seed=1)).max() <= 1  # (the material, whatever the last bit of a sine here)
    assert all(k.startswith("lpc") for kd in kinds[:3] for k in kd), kinds
    frames, sizes = mdl.encode_stream(x, 2, 256, 8)
    assert mdl.header(44100, 2, 256, 868, min(sizes), max(sizes)) + frames == data
    host = b"".join(encode(sa, x[k * 512:(k + 1) * 512], 2, 256, k, 8) for k in range(4))
    assert sa.flac_header(44100, 2, 256, mdl.info(868, sizes)) + host == data
