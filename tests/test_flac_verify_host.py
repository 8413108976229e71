"""The FLAC decoder on the host (include/saugns_amd.h, section "FLAC", paragraph "Verify": sauAmd_flac_decode_block; the arithmetic
is saugns_amd/csrc/sau_flac_dec.h's, which the device's flac_decode_kernel runs too): round trips of every encoder mode against
the Python models' decoders, the golden files, single-bit flips, the crafted refusals and truncation. No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import flac_verify_cases as fc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _kind(k):
    """a model's word on a subframe as "constant", "verbatim", "fixed<o>/p<p>" or "lpc<o>/p<p>" (flac24_model gives tuples)"""
    if isinstance(k, str):
        return k
    return k[0] if k[0] in ("constant", "verbatim") else "%s%d/p%d" % (k[0], k[1], k[2])


def _decode(sa, c):
    return sa.flac_decode_block(c["frame"], c["channels"], c["B"], c["bits"], c["number"])


@pytest.mark.parametrize("mode", list(fc.MODES))
def test_round_trip(sa, mode):
    """every kind, channels 1 and 2, B 256 and 4096, n in {1, 2, 4, 5, 255, B}: the decoder returns the input, consumes exactly the
    encoder's size and agrees with the mode's model; the set holds every subframe type, every assignment, partition orders 0 and 4"""
    bits, M, model = fc.MODES[mode]
    cases = [c for c in fc.valid_cases(sa) if c["mode"] == mode]
    assert {(c["kind"], c["channels"], c["B"], c["n"]) for c in cases} >= {
        (k, ch, B, n) for k in fc.kinds_of(mode) for ch in (1, 2) for B in fc.BLOCKS for n in fc.LENGTHS(B)}
    kinds, assigns = set(), set()
    for c in cases:
        st, size, out = _decode(sa, c)
        what = (mode, c["kind"], c["channels"], c["B"], c["n"])
        assert st == fc.OK, (what, fc.NAMES[st] if st < 12 else st)
        assert size == len(c["frame"]), what
        assert out.shape == (c["n"], c["channels"]) and (out.reshape(-1) == c["x"]).all(), what
        want, end, kd = model.decode_frame(c["frame"], 0, c["channels"], c["B"], c["number"])
        assert end == size and (np.asarray(want).reshape(-1) == out.reshape(-1)).all(), what
        kinds.update(_kind(k) for k in kd)
        assigns.add(c["frame"][3] >> 4)
    types = {k.split("/")[0] for k in kinds}
    assert {"constant", "verbatim", "fixed0", "fixed1", "fixed2", "fixed3", "fixed4"} <= types, types
    assert assigns == {0, 1, 8, 9, 10}, assigns
    assert any(k.endswith("/p0") for k in kinds) and any(k.endswith("/p4") for k in kinds), kinds
    if M:
        assert any(t.startswith("lpc") for t in types), types


def test_lpc_at_shift_15(sa):
    """the encoders' material does not reach a shift of 15 in a subframe that is taken (the largest coefficient would have to be
    below 1/16), so valid frames with it are built bit by bit: both widths and sums, against the models' decoders"""
    for name, fr, ch, B, bits, number, x in fc.handmade_valid():
        st, size, out = sa.flac_decode_block(fr, ch, B, bits, number)
        assert st == fc.OK and size == len(fr) and (out.reshape(-1) == x).all(), name
        want, end, kd = (fc.m16l if bits == 16 else fc.m24l).decode_frame(fr, 0, ch, B, number)
        assert end == size and (np.asarray(want).reshape(-1) == x).all() and kd == ["lpc1/p0"], name


@pytest.mark.parametrize("name,model,bits", [("flac_sine_stereo_b256.flac", fc.m16, 16), ("flac_lpc_pm_stereo_b256.flac", fc.m16l, 16),
                                             (fc.m24.GOLDEN_NAME, fc.m24, 24), (fc.m24l.GOLDEN_NAME, fc.m24l, 24)])
def test_golden_files(sa, name, model, bits):
    """the four golden files decode frame by frame to the models' samples"""
    data = open(os.path.join(GOLDEN, name), "rb").read()
    h = model.parse_header(data)
    ch, B = h["channels"], h["max_block"]
    assert h["bps"] == bits
    want = model.decode_frames(data[42:], ch, B)[0]
    at, k, got = 42, 0, []
    while at < len(data):
        st, size, out = sa.flac_decode_block(data[at:], ch, B, bits, k)
        assert st == fc.OK and size, (name, k, st)
        got.append(out)
        at, k = at + size, k + 1
    assert at == len(data) and k == -(-h["frames"] // B)
    got = np.concatenate(got).reshape(-1)
    assert len(got) == h["frames"] * ch and (got == np.asarray(want).reshape(-1)).all()


def _one_of_each_type(sa):
    """one B = 256 whole frame per (width, subframe type): (type, case)"""
    picked = {}
    for c in fc.valid_cases(sa):
        if c["B"] != 256 or c["n"] != 256:
            continue
        for k in fc.subframe_types(c["frame"], c["channels"], c["B"], c["bits"], c["number"]):
            t = k.split("/")[0].rstrip("012345678")
            if (c["bits"], t) not in picked or len(c["frame"]) < len(picked[(c["bits"], t)]["frame"]):
                picked[(c["bits"], t)] = c
    assert set(picked) == {(b, t) for b in (16, 24) for t in ("constant", "verbatim", "fixed", "lpc")}, sorted(picked)
    return picked


def test_single_bit_flips(sa):
    """one B = 256 frame of each subframe type and width with every single bit flipped: never OK (CRC-16 sees every such error)"""
    L = sa.lib()
    for (bits, t), c in sorted(_one_of_each_type(sa).items()):
        fr = c["frame"]
        buf = (C.c_uint8 * len(fr)).from_buffer_copy(fr)
        out = np.zeros(256 * c["channels"], np.int32)
        n, st = C.c_uint32(0), C.c_int(-1)
        seen = set()
        for bit in range(8 * len(fr)):
            buf[bit >> 3] ^= 0x80 >> (bit & 7)
            size = L.sauAmd_flac_decode_block(buf, len(fr), c["channels"], 256, bits, c["number"], out.ctypes.data, 256, C.byref(n), C.byref(st))
            buf[bit >> 3] ^= 0x80 >> (bit & 7)
            assert st.value != fc.OK and size == 0, (bits, t, bit)
            seen.add(st.value)
        assert bytes(buf) == fr
        assert fc.CRC16 in seen and fc.SYNC in seen, (bits, t, sorted(seen))


def test_crafted_refusals(sa):
    """each corruption of the table, its CRCs made right again, gives exactly its status"""
    cases = fc.corrupt_cases()
    wanted = ("wrong frame number", "escape parameter", "the other width's method (16 bits)", "partition order 1 on a short block",
              "wasted-bits flag", "LPC precision 11", "non-zero padding", "left/side whose R leaves the bits (16 bits)", "CRC-8 off by one",
              "CRC-16 off by one", "block size code 0111 carrying n == B")
    for w in wanted:
        assert any(name.startswith(w) for name, *_ in cases), w
    assert {c[6] for c in cases} == set(range(12)) - {fc.LENGTH, fc.MISMATCH}
    for name, fr, ch, B, bits, number, status in cases:
        st, size, out = sa.flac_decode_block(fr, ch, B, bits, number)
        assert st == status, (name, fc.NAMES[st] if st < 12 else st, fc.NAMES[status])
        assert (size == len(fr)) if status == fc.OK else (size == 0 and out is None), name


def test_truncation(sa):
    """every proper prefix of a valid frame gives LENGTH: short and whole blocks of every type at both widths, and a long frame"""
    frames = [c for c in _one_of_each_type(sa).values()]
    frames += [c for c in fc.valid_cases(sa) if c["n"] == 5 and c["channels"] == 2 and c["kind"] == "noise"]
    for c in frames:
        fr = c["frame"]
        for cut in range(len(fr)):
            st, size, _ = sa.flac_decode_block(fr[:cut], c["channels"], c["B"], c["bits"], c["number"])
            assert st == fc.LENGTH and size == 0, (c["mode"], c["kind"], cut, st)
    big = max((c for c in fc.valid_cases(sa) if c["B"] == 4096), key=lambda c: len(c["frame"]))
    for cut in list(range(0, len(big["frame"]), 97)) + [len(big["frame"]) - 1]:
        assert sa.flac_decode_block(big["frame"][:cut], big["channels"], 4096, big["bits"], big["number"])[0] == fc.LENGTH, cut


def test_arguments(sa):
    """a bad argument or too little room gives 0 with BAD_ARGUMENT, outside the list of a frame's statuses"""
    c = next(c for c in fc.valid_cases(sa) if c["n"] == 255 and c["channels"] == 2 and c["bits"] == 16)
    fr = c["frame"]
    assert sa.flac_decode_block(fr, 2, 256, 16, c["number"], cap_frames=254)[0] == fc.BAD_ARGUMENT
    assert sa.flac_decode_block(fr, 2, 256, 16, c["number"], cap_frames=255)[0] == fc.OK
    assert sa.flac_decode_block(fr, 3, 256, 16, c["number"])[0] == fc.BAD_ARGUMENT
    assert sa.flac_decode_block(fr, 2, 300, 16, c["number"])[0] == fc.BAD_ARGUMENT
    assert sa.flac_decode_block(fr, 2, 256, 20, c["number"])[0] == fc.BAD_ARGUMENT
    assert sa.flac_decode_block(fr, 2, 256, 16, 1 << 31)[0] == fc.BAD_ARGUMENT
    assert sa.flac_decode_block(b"", 2, 256, 16, 0)[0] == fc.LENGTH
    L = sa.lib()
    buf = (C.c_uint8 * len(fr)).from_buffer_copy(fr)
    n = C.c_uint32(7)
    assert L.sauAmd_flac_decode_block(buf, len(fr), 2, 256, 16, c["number"], None, 0, C.byref(n), None) == 0
    assert fc.BAD_ARGUMENT not in range(12)
    # the package's names for the statuses are the header's
    assert tuple(sa.FLAC_DEC_NAMES) == fc.NAMES and sa.FLAC_DEC_BAD_ARGUMENT == fc.BAD_ARGUMENT
    assert [getattr(sa, "FLAC_DEC_" + n) for n in fc.NAMES] == list(range(12))
