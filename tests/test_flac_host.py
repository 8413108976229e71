"""The FLAC encoder without a GPU (include/saugns_amd.h, section "FLAC": sauAmd_flac_header, sauAmd_flac_encode_block,
sauAmd_render_file_flac): the numpy restatement of that section (tests/flac_model.py) against its own independent decoder, the
library's host restatement (tables.cpp: flac_encode_block, built from sau_flac.h as the kernels are) against the model byte for
byte, the header against hand-packed bytes, the committed golden stream, the launch plan of a feed (launch_plan.h:
plan_flac_row, plan_flac) and the refusals over the sequential test executor (tests/seqexec keeps engine.h's refusing
default). tests/test_gpu_flac.py compares the device with the model."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import flac_model as mdl
from conftest import GOLDEN, ROOT, load_program

KEY = "devtests__voice-reuse"
GOLDEN_FLAC = os.path.join(GOLDEN, "flac_sine_stereo_b256.flac")


@pytest.fixture(scope="module")
def flac_hooks(sa, hooks):
    """tests/hooks_flac/libsaugns_amd_flac_hooks.so: the product's object files (the `hooks` fixture has built them) + the FLAC
    writer over an injected backend and the encoder's launch plan"""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "hooks_flac")])
    return sa.api.use_flac_hooks(os.path.join(ROOT, "tests", "hooks_flac", "libsaugns_amd_flac_hooks.so"))


def lengths(B):
    return [1, 3, 4, 5, B - 1, B]


_cases = {}


def cases(B):
    """(kind, channels, n, frame number, samples, the model's frame, its choices): computed once per B"""
    if B not in _cases:
        out = []
        numbers = [0, 127, 128, 2047, 2048, 65535, 65536, (1 << 31) - 1]
        for ch in (1, 2):
            for i, kind in enumerate(mdl.KINDS):
                for j, n in enumerate(lengths(B)):
                    x = mdl.crafted(kind, n, ch, seed=i)
                    number = numbers[(i + j) % len(numbers)]
                    frame, choice = mdl.encode_block(x, ch, B, number, with_choice=True)
                    out.append((kind, ch, n, number, x, frame, choice))
        _cases[B] = out
    return _cases[B]


# ---- the model ---------------------------------------------------------------------------------------------------------------

def test_the_crc_check_values():
    assert mdl.crc8(b"123456789") == 0xF4 and mdl.crc16(b"123456789") == 0xFEE8
    assert mdl.crc8(b"") == 0 and mdl.crc16(b"") == 0


def test_the_frame_numbers_coding():
    want = {0: "00", 127: "7f", 128: "c280", 2047: "dfbf", 2048: "e0a080", 65535: "efbfbf", 65536: "f0908080",
            0x1fffff: "f7bfbfbf", 0x200000: "f888808080", 0x3ffffff: "fbbfbfbfbf", 0x4000000: "fc8480808080",
            (1 << 31) - 1: "fdbfbfbfbfbf"}
    for v, h in want.items():
        assert mdl.utf8(v).hex() == h, (v, mdl.utf8(v).hex())
        if v < 0x110000 and not 0xd800 <= v < 0xe000:
            assert chr(v).encode("utf-8") == mdl.utf8(v)  # where UTF-8 proper reaches, it is UTF-8


@pytest.mark.parametrize("B", mdl.BLOCKS)
def test_the_model_decodes_what_it_encodes(B):
    kinds, assigns = set(), set()
    for kind, ch, n, number, x, frame, (assign, an) in cases(B):
        got, end, kd = mdl.decode_frame(frame, 0, ch, B, number)
        assert end == len(frame) and (got.reshape(-1) == x).all(), (kind, ch, n)
        assert len(frame) <= mdl.frame_bound(n, ch)
        assigns.add(assign)
        kinds.update(a["type"] + str(a.get("order", "")) for a in an)
        if n == 1 or kind == "silence":
            assert all(a["type"] == "constant" for a in an)
        if kind == "noise" and n == B:
            assert all(a["type"] == "verbatim" for a in an) and len(frame) > 2 * n * ch
    assert assigns == {"mono", "LR", "LS", "SR", "MS"}
    assert kinds >= {"constant", "verbatim", "fixed0", "fixed1", "fixed2", "fixed3", "fixed4"}, kinds


def test_crafted_inputs_choose_what_they_are_crafted_for():
    B = 1024

    def choice(kind, ch=2, n=B):
        return mdl.encode_block(mdl.crafted(kind, n, ch, seed=2), ch, B, 0, with_choice=True)[1]

    assert choice("silence") == ("LR", [dict(type="constant", bits=24)] * 2)
    assert choice("noise")[0] == "LR" and [a["type"] for a in choice("noise")[1]] == ["verbatim"] * 2
    a, an = choice("centre")  # L == R: the side is constant, and L + S comes before S + R and M + S on the tie
    assert a == "LS" and an[0]["type"] == "fixed" and an[1] == dict(type="constant", bits=25)
    a, an = choice("l_only")  # R is constant: L + R costs what L + S costs, and comes first
    assert a == "LR" and an[0]["type"] == "fixed" and an[1] == dict(type="constant", bits=24)
    a, an = choice("anti")  # R == -L: the mid is constant (0)
    assert a == "MS" and an[0] == dict(type="constant", bits=24) and an[1]["type"] == "fixed"
    assert choice("unrelated")[0] == "LR"
    a, an = choice("extremes")  # L - R = +-65535 needs all 17 bits; L + R = -1: the mid is constant
    assert a == "MS" and an[0] == dict(type="constant", bits=24) and an[1] == dict(type="verbatim", bits=8 + 17 * B)
    x = mdl.crafted("extremes", 6, 2)
    assert sorted(set((x[0::2].astype(int) - x[1::2]).tolist())) == [-65535, 65535]
    got, _, _ = mdl.decode_frame(mdl.encode_block(x, 2, B, 5), 0, 2, B, 5)
    assert (got.reshape(-1) == x).all()
    assert {a.get("p") for k in ("burst", "steps", "sine") for a in choice(k)[1]} >= {0, 4}  # partitioned and not


def test_the_decoder_refuses_what_the_section_excludes():
    B = 256
    x = mdl.crafted("sine", B + 9, 2)
    data, sizes = mdl.encode_stream(x, 2, B)
    mdl.decode_frames(data, 2, B)

    def broken(at, xor):
        b = bytearray(data)
        b[at] ^= xor
        return bytes(b)

    for what, d in (("sync", broken(1, 0x01)), ("CRC-8", broken(4, 0x01)), ("CRC-16", broken(sizes[0] - 1, 0x80)),
                    ("a body bit", broken(sizes[0] // 2, 0x10)), ("the second frame's number", broken(sizes[0] + 4, 0x01)),
                    ("cut short", data[:-1]), ("bytes behind", data + b"\0")):
        with pytest.raises((mdl.Bad, ValueError, IndexError)):
            mdl.decode_frames(d, 2, B)
    with pytest.raises(mdl.Bad):
        mdl.decode_frames(data, 2, B, first=1)


# ---- the library's host restatement -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", mdl.BLOCKS)
def test_the_hosts_block_equals_the_model_byte_for_byte(sa, B):
    for kind, ch, n, number, x, frame, _ in cases(B):
        got = sa.flac_encode_block(x, ch, B, number)
        assert got == frame, (kind, ch, n, number, len(got), len(frame))
        assert len(got) <= 15 + ch * (1 + 2 * n)
    x = mdl.crafted("sine", 4096, 2)
    assert sa.flac_encode_block(x, 2, 0, 7) == mdl.encode_block(x, 2, 4096, 7)  # 0 means 4096


def test_a_short_cap_writes_nothing_and_bad_arguments_give_0(sa):
    lib = sa.lib()
    x = mdl.crafted("sine", 300, 2)
    want = mdl.encode_block(x[:512], 2, 256, 3)
    buf = np.full(len(want) + 16, 0xa5, np.uint8)
    assert lib.sauAmd_flac_encode_block(x.ctypes.data, 256, 2, 256, 3, buf.ctypes.data, len(want) - 1) == len(want)
    assert (buf == 0xa5).all()
    assert lib.sauAmd_flac_encode_block(x.ctypes.data, 256, 2, 256, 3, None, 1 << 20) == len(want)
    assert lib.sauAmd_flac_encode_block(x.ctypes.data, 256, 2, 256, 3, buf.ctypes.data, len(want)) == len(want)
    assert bytes(buf[:len(want)]) == want and (buf[len(want):] == 0xa5).all()
    for args in ((None, 256, 2, 256, 3), (x.ctypes.data, 0, 2, 256, 3), (x.ctypes.data, 257, 2, 256, 3), (x.ctypes.data, 256, 0, 256, 3),
                 (x.ctypes.data, 256, 3, 256, 3), (x.ctypes.data, 256, 2, 255, 3), (x.ctypes.data, 256, 2, 8192, 3),
                 (x.ctypes.data, 256, 2, 128, 3), (x.ctypes.data, 256, 2, 256, 1 << 31)):
        assert lib.sauAmd_flac_encode_block(*args, buf.ctypes.data, len(buf)) == 0, args


def test_the_header_against_hand_packed_bytes(sa):
    info = dict(frames=0x9_8765_4321, blocks=3, bytes=99, min_frame_bytes=0x0e, max_frame_bytes=0x123456)
    got = sa.flac_header(44100, 2, 1024, info)
    want = bytes.fromhex("664c6143" "80000022" "0400" "0400" "00000e" "123456"
                         # 44100 = 0x0ac44 in 20 bits, 001 (channels - 1), 01111 (bits - 1), then 36 bits of frames
                         "0ac44" "2f" "987654321") + bytes(16)
    assert len(want) == 42 and got == want
    assert got == mdl.header(44100, 2, 1024, info["frames"], 0x0e, 0x123456)
    h = mdl.parse_header(got)
    assert (h["srate"], h["channels"], h["bps"], h["frames"], h["min_block"], h["max_block"]) == (44100, 2, 16, info["frames"], 1024, 1024)
    assert sa.flac_header(655350, 1, 0) == mdl.header(655350, 1, 4096)  # 0 means 4096; no record: an empty one
    for args in ((0, 1, 256), (655351, 1, 256), (8000, 0, 256), (8000, 3, 256), (8000, 1, 100), (8000, 1, 8192)):
        assert sa.flac_header(*args) == b"", args
    lib = sa.lib()
    buf = np.full(64, 0xa5, np.uint8)
    assert lib.sauAmd_flac_header(8000, 1, 256, None, buf.ctypes.data, 41) == 42 and (buf == 0xa5).all()
    assert lib.sauAmd_flac_header(8000, 1, 256, None, None, 0) == 42
    assert lib.sauAmd_flac_header(8000, 1, 256, None, buf.ctypes.data, 42) == 42 and (buf[42:] == 0xa5).all()


def test_the_golden_stream_decodes_and_encodes_to_itself(sa):
    """a stereo sine of 3 * 256 + 100 frames at 44100 Hz in blocks of 256, made by the model: for anyone with a decoder"""
    data = open(GOLDEN_FLAC, "rb").read()
    assert len(data) <= 4096
    h, x = mdl.decode_file(data)
    assert (h["srate"], h["channels"], h["max_block"], h["frames"]) == (44100, 2, 256, 868)
    assert (x == mdl.crafted("sine", 868, 2, seed=1)).all()
    frames, sizes = mdl.encode_stream(x, 2, 256)
    assert mdl.header(44100, 2, 256, 868, min(sizes), max(sizes)) + frames == data
    host = b"".join(sa.flac_encode_block(x[k * 512:(k + 1) * 512], 2, 256, k) for k in range(4))
    assert sa.flac_header(44100, 2, 256, mdl.info(868, sizes)) + host == data


# ---- the launch plan ----------------------------------------------------------------------------------------------------

def plan(hooks_lib, B, ch, pos, frames, finish):
    n = len(pos)
    rows = (C.c_uint64 * (8 * n))()
    out = (C.c_uint64 * 8)()
    ok = hooks_lib.sauAmd_flac_plan(B, ch, n, (C.c_uint64 * n)(*pos), (C.c_uint32 * n)(*frames), 1 if finish else 0, rows, out)
    names = ("block0", "n_blocks", "last_n", "pend", "pend_next", "job0", "out_off", "worst")
    return ok, [dict(zip(names, rows[8 * r:8 * r + 8])) for r in range(n)], dict(zip(("B", "jobs", "analyze_threads", "analyze_lds",
                                                                                    "write_lds", "pend_pitch", "worst", "out_bytes"), out))


@pytest.mark.parametrize("B", [256, 1024, 4096])
@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("finish", [False, True])
def test_the_plan_of_a_feed(flac_hooks, B, ch, finish):
    starts = [0, 1, B - 1, B, B + 1, 3 * B + 37]
    feeds = [0, 1, B - 1, B, B + 1, 2 * B, 3 * B + 37]
    case = [(p0, fr) for p0 in starts for fr in feeds]
    ok, rows, out = plan(flac_hooks, B, ch, [c[0] for c in case], [c[1] for c in case], finish)
    assert ok == 1
    jobs = off = worst = 0
    for (p0, fr), r in zip(case, rows):
        end = p0 + fr
        blocks = list(range(p0 // B, end // B)) + ([end // B] if finish and end % B else [])
        sizes = [min(B, end - k * B) for k in blocks]
        assert r["block0"] == p0 // B and r["n_blocks"] == len(blocks), (p0, fr, r)
        assert r["last_n"] == (sizes[-1] if blocks else B), (p0, fr, r)
        assert r["pend"] == p0 % B and r["pend_next"] == (0 if finish else end % B), (p0, fr, r)
        assert r["pend"] + fr == sum(sizes) + (end % B if not finish else 0), (p0, fr, r)  # nothing is lost, nothing read twice
        assert r["job0"] == jobs and r["out_off"] == off and off % 16 == 0, (p0, fr, r)
        assert r["worst"] == sum(15 + ch * (1 + 2 * n) for n in sizes), (p0, fr, r)
        jobs += len(blocks)
        worst += r["worst"]
        off += (r["worst"] + 15) // 16 * 16
    assert out["B"] == B and out["jobs"] == jobs and out["worst"] == worst and out["out_bytes"] == off
    assert out["analyze_threads"] == (256 if ch == 2 else 64) and out["pend_pitch"] == B * ch
    assert out["analyze_lds"] == 4 * (B + B // 32)
    assert out["write_lds"] == out["analyze_lds"] + 4 * ((15 + ch * (1 + 2 * B)) // 4 + 2)
    assert out["write_lds"] + 64 <= 65536 and out["analyze_lds"] + 10240 <= 65536  # (+ the kernels' static LDS)


def test_the_plan_refuses_what_the_header_refuses(flac_hooks):
    for B, ch in ((100, 1), (8192, 1), (256, 0), (256, 3)):
        assert plan(flac_hooks, B, ch, [0], [1000], True)[0] == 0
    assert plan(flac_hooks, 0, 2, [0], [10000], True)[2]["B"] == 4096
    assert plan(flac_hooks, 256, 1, [0] * 65536, [0] * 65536, True)[0] == 0  # more rows than an encoder has
    assert plan(flac_hooks, 256, 1, [0] * 65535, [0] * 65535, True)[0] == 1
    # block numbers stay below 2^31 - 1: the last allowed block, and one more
    top = ((1 << 31) - 2) * 256
    assert plan(flac_hooks, 256, 1, [top], [256], False)[0] == 1 and plan(flac_hooks, 256, 1, [top], [257], True)[0] == 0
    # the 1 GiB rule on the arguments alone: 2^21 mono blocks of 256 frames are 2^21 * 528 bytes at their bound
    assert plan(flac_hooks, 256, 1, [0], [(1 << 30) // 528 * 256], False)[0] == 1
    assert plan(flac_hooks, 256, 1, [0], [((1 << 30) // 528 + 1) * 256], False)[0] == 0
    assert plan(flac_hooks, 256, 1, [0, 0], [(1 << 30) // 528 * 256, 256], False)[0] == 0  # ... summed over the rows


# ---- refusals over the sequential executor -------------------------------------------------------------------------------

def test_an_encoder_is_refused_by_a_backend_without_one(sa, seqexec):
    prg = load_program(sa, KEY)
    b = sa.Batch([prg], 12000, backend=seqexec.seq_backend_create(1016))
    with pytest.raises(RuntimeError, match="this backend has no FLAC encoder"):
        b.create_flac(1, 2, 1024)
    for n_rows, ch, B in ((0, 1, 256), (65536, 1, 256), (1, 0, 256), (1, 3, 256), (1, 1, 255), (1, 1, 8192)):
        with pytest.raises(RuntimeError, match="bad argument"):  # whatever the backend
            b.create_flac(n_rows, ch, B)
    b.close()
    sa.lib().sauAmd_Flac_destroy(None)  # allowed


def test_render_file_flac_over_a_backend_without_an_encoder_leaves_no_file(sa, seqexec, flac_hooks, tmp_path):
    prg = load_program(sa, KEY)
    path = str(tmp_path / "x.flac")
    with pytest.raises(RuntimeError, match="this backend has no FLAC encoder"):
        sa.render_file_flac(prg, 8000, path, 2, 1024, backend=seqexec.seq_backend_create(1016))
    assert "this backend has no FLAC encoder" in sa.api.last_error()
    assert not os.path.exists(path)
    for bad in (dict(srate=0), dict(srate=655351), dict(channels=0), dict(channels=3), dict(block_frames=100), dict(block_frames=8192)):
        a = dict(srate=8000, channels=1, block_frames=256)
        a.update(bad)
        with pytest.raises(RuntimeError, match="bad argument"):
            sa.render_file_flac(prg, a["srate"], path, a["channels"], a["block_frames"], backend=seqexec.seq_backend_create(1016))
        with pytest.raises(RuntimeError, match="bad argument"):  # the product's own entry point looks at them before any device
            sa.render_file_flac(prg, a["srate"], path, a["channels"], a["block_frames"])
        assert not os.path.exists(path)
    lib = sa.lib()
    assert not lib.sauAmd_render_file_flac(None, 8000, os.fsencode(path), 1, 256, None, None) and "bad argument" in sa.api.last_error(lib)
    assert not lib.sauAmd_render_file_flac(prg.ptr, 8000, None, 1, 256, None, None) and "bad argument" in sa.api.last_error(lib)
