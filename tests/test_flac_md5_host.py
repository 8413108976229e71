"""The MD5 of a FLAC stream's unencoded samples on the host (include/saugns_amd.h, section "FLAC", paragraph "MD5":
sauAmd_flac_md5, sauAmd_flac_header_md5; the arithmetic is saugns_amd/csrc/sau_md5.h's, which the device's flac_md5_kernel uses
too). The oracle is hashlib.md5 over the samples packed by numpy: little-endian, 2 bytes per sample at 16 bits, the low 3 of 4
at 24 bits."""
import hashlib

import numpy as np
import pytest

EMPTY = "d41d8cd98f00b204e9800998ecf8427e"


def packed(x, bits):
    x = np.asarray(x, np.int64)
    if bits == 16:
        return x.astype("<i2").tobytes()
    return np.ascontiguousarray(x.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3]).tobytes()


def lengths(bits):
    """every sample count that puts the byte length mod 64 at 0, 1 to 3 samples past a boundary, at 54 / 55 / 56 and at 62 / 63
    where the sample size reaches them, and the counts around one, two and three chunks"""
    size = bits // 8
    want = {0, 54, 55, 56, 62, 63, size, 2 * size, 3 * size}
    out = {n for n in range(0, 3 * 64 // size + 70) if (n * size) % 64 in want}
    for chunks in (1, 2, 3):
        mid = chunks * 64 // size
        out.update(range(max(mid - 2, 0), mid + 3))
    return sorted(out)


def test_known_answers(sa):
    x = np.frombuffer(b"message digest", "<i2")
    assert len(x) == 7
    assert sa.flac_md5(x, 16).hex() == "f96b697d7cb7938d525a2f31aaf161d0"
    assert sa.flac_md5(np.zeros(0, np.int32), 16).hex() == EMPTY
    assert sa.flac_md5(np.zeros(0, np.int32), 24).hex() == EMPTY
    # RFC 1321's other suite members that are whole samples at 3 bytes: "abc"
    assert sa.flac_md5([int.from_bytes(b"abc", "little")], 24).hex() == "900150983cd24fb0d6963f7d28e17f72"


@pytest.mark.parametrize("bits", [16, 24])
def test_against_hashlib(sa, bits):
    """the issue's counts are among them: 18, 61, 40 and 21 samples at 24 bits (54, 183, 120, 63 bytes); 27, 28 and 31 at 16"""
    ns = lengths(bits)
    assert set({16: (27, 28, 31, 32, 33, 34, 35), 24: (18, 61, 40, 21, 64, 65, 66, 67)}[bits]) <= set(ns)
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    rng = np.random.default_rng(bits)
    for n in ns:
        x = rng.integers(lo, hi + 1, n).astype(np.int32)
        for at, v in ((0, lo), (n - 1, hi), (n // 2, -1), (n // 3, 0)):  # the extremes, all ones and zero
            if 0 <= at < n:
                x[at] = v
        got = sa.flac_md5(x, bits)
        assert got is not None and got.hex() == hashlib.md5(packed(x, bits)).hexdigest(), (bits, n)
    # a long one: many chunks, and both channels of a stereo stream are just the interleaved samples
    x = rng.integers(lo, hi + 1, 2 * 4096 + 6).astype(np.int32)
    assert sa.flac_md5(x, bits).hex() == hashlib.md5(packed(x, bits)).hexdigest()
    assert sa.flac_md5(x.reshape(-1, 2), bits) == sa.flac_md5(x, bits)


def test_header_with_md5(sa):
    d = bytes(range(1, 17))
    info = {"frames": 12345, "blocks": 13, "bytes": 999, "min_frame_bytes": 14, "max_frame_bytes": 2100}
    for bits in (16, 24):
        for ch in (1, 2):
            plain = sa.flac_header(44100, ch, 1024, info, bits=bits)
            got = sa.flac_header(44100, ch, 1024, info, bits=bits, md5=d)
            assert len(plain) == len(got) == 42 and plain[26:42] == bytes(16)
            assert got[:26] == plain[:26] and got[26:42] == d
    assert sa.flac_header(44100, 2, 1024, info, md5=d) == sa.flac_header(44100, 2, 1024, info, bits=16, md5=d)
    assert sa.flac_header(44100, 2, 1024, info, md5=d)[:26] == sa.flac_header(44100, 2, 1024, info)[:26]
    # md5 NULL means zeros: sauAmd_flac_header_bits's bytes
    L = sa.lib()
    out = (sa.api.C.c_uint8 * 42)()
    assert L.sauAmd_flac_header_md5(44100, 2, 1024, 24, None, None, out, 42) == 42
    assert bytes(out) == sa.flac_header(44100, 2, 1024, None, bits=24)
    # what the plain header refuses is refused here too
    assert sa.flac_header(44100, 2, 1024, info, bits=20, md5=d) == b""
    assert sa.flac_header(44100, 3, 1024, info, bits=16, md5=d) == b""
    assert sa.flac_header(44100, 2, 300, info, bits=16, md5=d) == b""
    with pytest.raises(ValueError):
        sa.flac_header(44100, 2, 1024, info, md5=b"short")


def test_refusals(sa):
    x = np.arange(-4, 4, dtype=np.int32)
    for bits in (0, 8, 15, 17, 20, 32, -16):
        assert sa.flac_md5(x, bits) is None, bits
    for bits, bad in ((16, 32768), (16, -32769), (24, 1 << 23), (24, -(1 << 23) - 1)):
        for at in (0, 3, 7):
            y = x.copy()
            y[at] = bad
            assert sa.flac_md5(y, bits) is None, (bits, bad, at)
        y[at] = bad - 1 if bad > 0 else bad + 1
        assert sa.flac_md5(y, bits) is not None


def test_the_file_switch_is_off_and_returns_the_previous_value(sa):
    assert sa.set_flac_file_md5(0) == 0  # the initial value
    try:
        assert sa.set_flac_file_md5(1) == 0
        assert sa.set_flac_file_md5(5) == 1
        assert sa.set_flac_file_md5(0) == 1
    finally:
        sa.set_flac_file_md5(0)
