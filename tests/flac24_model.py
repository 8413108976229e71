"""The 24-bit FLAC format of include/saugns_amd.h, section "FLAC", paragraph "24 bits", restated in numpy from that text alone:
the quantiser, the encoder's choices (bps 24 and 25, Rice parameters 0 .. 30 in five bits, residual coding method 01) and an
independent decoder written from RFC 9639 -- sample size code 110, method 01, the side channel in 25 bits. The decoder verifies
both CRCs, the frame numbers, every reserved bit, that no parameter is the escape 11111 and that every frame ends where the
next begins; it shares nothing with the encoder but the two CRC routines and the frame number's coding, which come from
tests/flac_model.py and are held against their check values there."""
import numpy as np

from flac_model import crc8, crc16, utf8

BLOCKS = (256, 512, 1024, 2048, 4096)
ASSIGN = {0: "mono", 1: "LR", 8: "LS", 9: "SR", 10: "MS"}
S24_MIN, S24_MAX = -(1 << 23), (1 << 23) - 1
NK = 31  # Rice parameters 0 .. 30


class Bad(Exception):
    pass


def block_frames(b):
    return 4096 if b == 0 else (b if b in BLOCKS else 0)


def frame_bound(n, channels):
    return 15 + channels * (1 + 3 * n)


# ---- the quantiser ---------------------------------------------------------------------------------------------------------

def quantize(x, gain=1.0, bits=24):
    """float32 samples -> int32: y = x * gain in f32; a NaN becomes -1; clamped to [-1, 1]; bits 24: the nearest integer to
    (double)y * 8388607, ties to even (the product is exact); bits 16: the nearest integer to the f32 product y * 32767"""
    x = np.asarray(x, np.float32)
    with np.errstate(all="ignore"):
        y = (x * np.float32(gain)).astype(np.float32)
    y = np.where(np.isnan(y), np.float32(-1), y)
    y = np.minimum(np.maximum(y, np.float32(-1)), np.float32(1)).astype(np.float32)
    if bits == 24:
        return np.rint(y.astype(np.float64) * 8388607.0).astype(np.int32)
    assert bits == 16
    return np.rint((y * np.float32(32767)).astype(np.float32)).astype(np.int32)


# ---- the encoder -----------------------------------------------------------------------------------------------------------

def header(srate, channels, B, frames=0, min_frame=0, max_frame=0, bits=24):
    B = block_frames(B)
    v = (B << 128) | (B << 112) | (min_frame << 88) | (max_frame << 64) | (srate << 44) | ((channels - 1) << 41) | ((bits - 1) << 36) | frames
    return b"fLaC" + bytes([0x80, 0, 0, 34]) + v.to_bytes(18, "big") + bytes(16)


def _residual(s, o):
    r = s.astype(np.int64)
    for _ in range(o):
        r = r[1:] - r[:-1]
    return r


def _zigzag(r):
    return np.where(r >= 0, 2 * r, -2 * r - 1)


def _best_k(u):
    best = None
    for k in range(NK):
        cost = int((u >> k).sum()) + (1 + k) * len(u)
        if best is None or cost < best[0]:
            best = (cost, k)
    return best


def analyze(s, bps, B):
    """one channel candidate of a block -> dict(type, bits, order, p, ks)"""
    n = len(s)
    s = s.astype(np.int64)
    if (s == s[0]).all():
        return dict(type="constant", bits=8 + bps)
    o = 0
    if n > 4:
        sums = [int(np.abs(_residual(s, k)[4 - k:]).sum()) for k in range(5)]
        o = sums.index(min(sums))
    u = _zigzag(_residual(s, o))
    assert int(u.max()) < 1 << 30
    best = None
    for p in range((4 if n == B else 0) + 1):
        plen = n >> p
        parts = [_best_k(u[(j * plen - o if j else 0):(j + 1) * plen - o]) for j in range(1 << p)]
        cost = sum(5 + c for c, _ in parts)
        if best is None or cost < best[0]:
            best = (cost, p, [k for _, k in parts])
    fixed, verbatim = 8 + bps * o + 6 + best[0], 8 + bps * n
    if verbatim <= fixed:
        return dict(type="verbatim", bits=verbatim)
    return dict(type="fixed", bits=fixed, order=o, p=best[1], ks=best[2])


def _put(bits, pos, value, width):
    for i in range(width):
        bits[pos + i] = (value >> (width - 1 - i)) & 1
    return pos + width


def _put_many(bits, pos, values, width):
    at = pos + width * np.arange(len(values))
    for i in range(width):
        bits[at + i] = (values >> (width - 1 - i)) & 1
    return pos + width * len(values)


def _write_sub(bits, pos, s, bps, a):
    s = s.astype(np.int64)
    mask = (1 << bps) - 1
    if a["type"] == "constant":
        pos = _put(bits, pos, 0, 8)
        return _put(bits, pos, int(s[0]) & mask, bps)
    if a["type"] == "verbatim":
        pos = _put(bits, pos, 0b00000010, 8)
        return _put_many(bits, pos, s & mask, bps)
    o, p, n = a["order"], a["p"], len(s)
    pos = _put(bits, pos, (0b001000 | o) << 1, 8)
    pos = _put_many(bits, pos, s[:o] & mask, bps)
    pos = _put(bits, pos, 0b010000 | p, 6)  # method 01, the partition order
    u = _zigzag(_residual(s, o))
    plen = n >> p
    for j in range(1 << p):
        k = a["ks"][j]
        pos = _put(bits, pos, k, 5)
        v = u[(j * plen - o if j else 0):(j + 1) * plen - o]
        q = v >> k
        lens = q + 1 + k
        start = pos + np.concatenate(([0], np.cumsum(lens)[:-1]))
        bits[start + q] = 1
        for i in range(k):
            bits[start + q + 1 + i] = (v >> (k - 1 - i)) & 1
        pos += int(lens.sum())
    return pos


def encode_block(x, channels, B, number, with_choice=False):
    """x: int32 [n * channels] interleaved, every sample in -2^23 .. 2^23 - 1 -> the frame's bytes"""
    B = block_frames(B)
    x = np.asarray(x, np.int64).reshape(-1, channels)
    n = len(x)
    assert 1 <= n <= B and x.min() >= S24_MIN and x.max() <= S24_MAX
    if channels == 1:
        subs, assign = [(x[:, 0], 24)], 0
        an = [analyze(x[:, 0], 24, B)]
    else:
        L, R = x[:, 0], x[:, 1]
        cand = {"L": (L, 24), "R": (R, 24), "M": ((L + R) >> 1, 24), "S": (L - R, 25)}
        A = {k: analyze(v[0], v[1], B) for k, v in cand.items()}
        pairs = [("L", "R", 1), ("L", "S", 8), ("S", "R", 9), ("M", "S", 10)]
        costs = [A[a]["bits"] + A[b]["bits"] for a, b, _ in pairs]
        a, b, assign = pairs[costs.index(min(costs))]
        subs, an = [cand[a], cand[b]], [A[a], A[b]]
    code = 8 + BLOCKS.index(B) if n == B else 7
    head = bytes([0xff, 0xf8, code << 4, (assign << 4) | 0b1100]) + utf8(number)  # sample size 110, one bit 0
    if n != B:
        head += (n - 1).to_bytes(2, "big")
    head += bytes([crc8(head)])
    total = 8 * len(head) + sum(a["bits"] for a in an)
    bits = np.zeros((total + 7) // 8 * 8, np.uint8)
    pos = 8 * len(head)
    for (s, bps), a in zip(subs, an):
        end = _write_sub(bits, pos, s, bps, a)
        assert end == pos + a["bits"], (end, pos, a)
        pos = end
    body = head + np.packbits(bits[8 * len(head):]).tobytes()
    frame = body + crc16(body).to_bytes(2, "big")
    assert len(frame) <= frame_bound(n, channels)
    if with_choice:
        return frame, (ASSIGN[assign], an)
    return frame


def encode_stream(x, channels, B, finish=True):
    """the frames of one row (no header) -> (bytes, the frames' sizes)"""
    B = block_frames(B)
    x = np.asarray(x, np.int64).reshape(-1, channels)
    sizes, out = [], []
    for k in range((len(x) + B - 1) // B if finish else len(x) // B):
        f = encode_block(x[k * B:(k + 1) * B].reshape(-1), channels, B, k)
        out.append(f)
        sizes.append(len(f))
    return b"".join(out), sizes


def info(frames, sizes):
    return dict(frames=frames, blocks=len(sizes), bytes=sum(sizes), min_frame_bytes=min(sizes) if sizes else 0,
                max_frame_bytes=max(sizes) if sizes else 0)


# ---- the decoder (RFC 9639; what the section excludes is refused) -----------------------------------------------------------

def parse_header(data):
    if data[:4] != b"fLaC" or bytes(data[4:8]) != bytes([0x80, 0, 0, 34]) or len(data) < 42:
        raise Bad("not the 42 header bytes")
    v = int.from_bytes(data[8:26], "big")
    return dict(min_block=v >> 128, max_block=(v >> 112) & 0xffff, min_frame=(v >> 88) & 0xffffff, max_frame=(v >> 64) & 0xffffff,
                srate=(v >> 44) & 0xfffff, channels=((v >> 41) & 7) + 1, bps=((v >> 36) & 31) + 1, frames=v & ((1 << 36) - 1),
                md5=bytes(data[26:42]))


def _signed(v, bits):
    return v - (1 << bits) if v >> (bits - 1) else v


_PRED = ((), (1,), (2, -1), (3, -3, 1), (4, -6, 4, -1))


def decode_frame(data, at, channels, B, number):
    """one frame from data[at:] -> (int64 [n, channels], the position behind it, per subframe (kind, order, p, ks))"""
    d = data
    if d[at] != 0xff or d[at + 1] != 0xf8:
        raise Bad("no sync code (or a reserved bit, or a variable block size) at %d" % at)
    code, rate = d[at + 2] >> 4, d[at + 2] & 15
    assign, size, zero = d[at + 3] >> 4, (d[at + 3] >> 1) & 7, d[at + 3] & 1
    if rate != 0 or size != 0b110 or zero != 0:
        raise Bad("sample rate code, sample size (not 110) or the reserved bit")
    if assign not in ASSIGN or (assign == 0) != (channels == 1):
        raise Bad("channel assignment %d" % assign)
    p = at + 4
    lead = d[p]
    if lead < 0x80:
        num, ulen = lead, 1
    else:
        ulen = 8 - (lead ^ 0xff).bit_length()
        if not 2 <= ulen <= 6:
            raise Bad("frame number's lead byte")
        num = lead & (0x7f >> ulen)
        for i in range(1, ulen):
            if d[p + i] >> 6 != 0b10:
                raise Bad("frame number's continuation byte")
            num = (num << 6) | (d[p + i] & 0x3f)
        if utf8(num) != bytes(d[p:p + ulen]):
            raise Bad("frame number not in its shortest form")
    p += ulen
    if num != number:
        raise Bad("frame number %d, not %d" % (num, number))
    if code == 7:
        n = int.from_bytes(d[p:p + 2], "big") + 1
        p += 2
        if n == B:
            raise Bad("a whole block with the code 0111")
    elif 8 <= code <= 12 and 256 << (code - 8) == B:
        n = B
    else:
        raise Bad("block size code %d" % code)
    if n > B:
        raise Bad("a block longer than B")
    if crc8(d[at:p]) != d[p]:
        raise Bad("CRC-8")
    p += 1
    chunk = d[p:p + frame_bound(n, channels) - (p - at)]
    s = format(int.from_bytes(chunk, "big"), "0%db" % (8 * len(chunk)))
    pos = 0

    def take(w):
        nonlocal pos
        v = int(s[pos:pos + w], 2)
        pos += w
        return v

    subs, kinds = [], []
    for c in range(channels):
        bps = 25 if (assign, c) in ((8, 1), (9, 0), (10, 1)) else 24
        if take(1) != 0:
            raise Bad("subframe padding bit")
        t = take(6)
        if take(1) != 0:
            raise Bad("wasted bits flag")
        if t == 0:
            v = np.full(n, _signed(take(bps), bps), np.int64)
            kinds.append(("constant", 0, 0, []))
        elif t == 1:
            v = np.array([_signed(int(s[pos + bps * i:pos + bps * (i + 1)], 2), bps) for i in range(n)], np.int64)
            pos += bps * n
            kinds.append(("verbatim", 0, 0, []))
        elif 0b001000 <= t <= 0b001100:
            o = t & 7
            v = [_signed(take(bps), bps) for _ in range(o)]
            if take(2) != 1:
                raise Bad("residual coding method (not 01)")
            po = take(4)
            if po and (n >> po) << po != n:
                raise Bad("partition order")
            ks = []
            coef = _PRED[o]
            for j in range(1 << po):
                k = take(5)
                if k == 31:
                    raise Bad("Rice parameter 31 (the escape)")
                ks.append(k)
                for _ in range((n >> po) - (o if j == 0 else 0)):
                    one = s.index("1", pos)
                    u = ((one - pos) << k) | (int(s[one + 1:one + 1 + k], 2) if k else 0)
                    pos = one + 1 + k
                    r = (u >> 1) if not u & 1 else -((u + 1) >> 1)
                    i = len(v)
                    v.append(r + sum(cf * v[i - 1 - m] for m, cf in enumerate(coef)))
            v = np.array(v, np.int64)
            kinds.append(("fixed", o, po, ks))
        else:
            raise Bad("subframe type %d" % t)
        if len(v) != n:
            raise Bad("subframe length")
        if v.min() < -(1 << (bps - 1)) or v.max() >= 1 << (bps - 1):
            raise Bad("a subframe's sample beyond its bps")
        subs.append(v)
    pad = (-pos) % 8
    if pad and take(pad) != 0:
        raise Bad("padding bits")
    end = p + pos // 8
    if crc16(d[at:end]) != int.from_bytes(d[end:end + 2], "big"):
        raise Bad("CRC-16")
    if channels == 1:
        out = subs[0][:, None]
    else:
        a, b = subs
        if assign == 1:
            L, R = a, b
        elif assign == 8:
            L, R = a, a - b
        elif assign == 9:
            L, R = a + b, b
        else:
            m = (a << 1) | (b & 1)
            L, R = (m + b) >> 1, (m - b) >> 1
        out = np.stack([L, R], 1)
    if out.min() < S24_MIN or out.max() > S24_MAX:
        raise Bad("a sample beyond 24 bits")
    return out, end + 2, kinds


def decode_frames(data, channels, B, first=0):
    """frames back to back, numbered from `first` -> (int32 [frames * channels], the frames' sizes, their subframes' kinds)"""
    B = block_frames(B)
    data = bytes(data)
    at, k, out, sizes, kinds = 0, first, [], [], []
    while at < len(data):
        if out and len(out[-1]) != B:
            raise Bad("a short block that is not the last")
        x, end, kd = decode_frame(data, at, channels, B, k)
        out.append(x)
        sizes.append(end - at)
        kinds.append(kd)
        at, k = end, k + 1
    if at != len(data):
        raise Bad("bytes behind the last frame")
    x = np.concatenate(out).astype(np.int32).reshape(-1) if out else np.zeros(0, np.int32)
    return x, sizes, kinds


def decode_file(data):
    """a whole 24-bit file -> (header dict, int32 [frames * channels]); STREAMINFO is held against the frames"""
    data = bytes(data)
    h = parse_header(data)
    if h["min_block"] != h["max_block"] or h["bps"] != 24 or h["md5"] != bytes(16):
        raise Bad("STREAMINFO")
    x, sizes, _ = decode_frames(data[42:], h["channels"], h["max_block"])
    if len(x) != h["frames"] * h["channels"]:
        raise Bad("total samples")
    if (h["min_frame"], h["max_frame"]) != ((min(sizes), max(sizes)) if sizes else (0, 0)):
        raise Bad("frame sizes")
    return h, x


# ---- crafted material ------------------------------------------------------------------------------------------------------

KINDS = ("constant", "rails", "anti_rails", "quiet_sine", "noise", "one_loud")


def crafted_f32(kind, frames, channels, seed=0, B=4096):
    """float32 [frames * channels] whose pcm24 values are: a constant; +-8388607 by turns (VERBATIM); L = -R at the rails (a side
    of +-16777214: all 25 bits); a sine of amplitude 2^-10 (every parameter <= 14); uniform noise in +-0.25 (parameters >= 15);
    a block silent in 15 of its 16 partitions of B / 16 frames and full-scale noise in one (p = 4, parameters far apart)"""
    rng = np.random.default_rng(2400 + seed)
    t = np.arange(frames)
    if kind == "constant":
        L, R = np.full(frames, 0.3712), np.full(frames, -0.0051)
    elif kind == "rails":
        L = np.where(t % 2 == 0, 1.0, -1.0)
        R = np.where(t % 3 == 0, -1.0, 1.0)
    elif kind == "anti_rails":
        L = np.where(t % 2 == 0, 1.0, -1.0)
        R = -L
    elif kind == "quiet_sine":
        L = 2.0 ** -10 * np.sin(2 * np.pi * 440 * t / 44100 + seed)
        R = 0.7 * L
    elif kind == "noise":
        L, R = rng.uniform(-0.25, 0.25, frames), rng.uniform(-0.25, 0.25, frames)
    elif kind == "one_loud":
        loud = (t // (B // 16)) % 16 == 5
        L = np.where(loud, rng.uniform(-1, 1, frames), 0.0)
        R = np.where((t // (B // 16)) % 16 == 11, rng.uniform(-1, 1, frames), 0.0)
    else:
        raise ValueError(kind)
    x = np.stack([L, R], 1) if channels == 2 else L[:, None]
    return x.astype(np.float32).reshape(-1)


def crafted(kind, frames, channels, seed=0, B=4096):
    """crafted_f32 through the quantiser: int32 [frames * channels]"""
    return quantize(crafted_f32(kind, frames, channels, seed, B), 1.0, 24)


def golden_samples():
    """the golden stream's samples: 3 * 256 + 100 stereo frames, noise in +-0.25 left, a sine of amplitude 0.5 right"""
    n = 3 * 256 + 100
    L = crafted_f32("noise", n, 1, seed=7)
    R = (0.5 * np.sin(2 * np.pi * 440 * np.arange(n) / 44100)).astype(np.float32)
    return quantize(np.stack([L, R], 1).reshape(-1), 1.0, 24)


GOLDEN_NAME = "flac24_noise_sine_stereo_b256.flac"

if __name__ == "__main__":  # python tests/flac24_model.py: (re)make the golden stream
    import os
    _x = golden_samples()
    _frames, _sizes = encode_stream(_x, 2, 256)
    _path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN_NAME)
    open(_path, "wb").write(header(44100, 2, 256, len(_x) // 2, min(_sizes), max(_sizes)) + _frames)
    print(_path, 42 + len(_frames), "bytes")
