"""The FLAC encoder of include/saugns_amd.h, section "FLAC", restated in numpy from that section alone, and an independent
decoder of the subset it states. The decoder verifies both CRCs, the frame numbers, every reserved bit, k <= 14 and that every
frame ends where the next begins; it shares nothing with the encoder but the two CRC routines, which the tests hold against
their check values. No third-party decoder has read these streams: tests/golden/flac_sine_stereo_b256.flac is there for anyone
who has one."""
import numpy as np

BLOCKS = (256, 512, 1024, 2048, 4096)
ASSIGN = {0: "mono", 1: "LR", 8: "LS", 9: "SR", 10: "MS"}


def block_frames(b):
    return 4096 if b == 0 else (b if b in BLOCKS else 0)


def frame_bound(n, channels):
    return 15 + channels * (1 + 2 * n)


# ---- CRCs ------------------------------------------------------------------------------------------------------------------

def _table(poly, width):
    top, mask = 1 << (width - 1), (1 << width) - 1
    t = []
    for b in range(256):
        c = b << (width - 8)
        for _ in range(8):
            c = ((c << 1) ^ poly) & mask if c & top else (c << 1) & mask
        t.append(c)
    return t


_T8, _T16 = _table(0x07, 8), _table(0x8005, 16)


def crc8(data):
    c = 0
    for b in bytes(data):
        c = _T8[c ^ b]
    return c


def crc16(data):
    c = 0
    for b in bytes(data):
        c = ((c << 8) & 0xffff) ^ _T16[(c >> 8) ^ b]
    return c


def utf8(v):
    """the extended UTF-8 coding of a frame number below 2^31"""
    assert 0 <= v < 1 << 31
    if v < 0x80:
        return bytes([v])
    n = 2 if v < 0x800 else 3 if v < 0x10000 else 4 if v < 0x200000 else 5 if v < 0x4000000 else 6
    lead = ((0xff << (8 - n)) & 0xff) | (v >> (6 * (n - 1)))
    return bytes([lead] + [0x80 | ((v >> (6 * i)) & 0x3f) for i in range(n - 2, -1, -1)])


# ---- the encoder -----------------------------------------------------------------------------------------------------------

def header(srate, channels, B, frames=0, min_frame=0, max_frame=0):
    B = block_frames(B)
    v = (B << 128) | (B << 112) | (min_frame << 88) | (max_frame << 64) | (srate << 44) | ((channels - 1) << 41) | (15 << 36) | frames
    return b"fLaC" + bytes([0x80, 0, 0, 34]) + v.to_bytes(18, "big") + bytes(16)


def _residual(s, o):
    """order o's residuals for i = o .. n-1, as int64"""
    s = s.astype(np.int64)
    r = s
    for _ in range(o):
        r = r[1:] - r[:-1]
    return r


def _zigzag(r):
    return np.where(r >= 0, 2 * r, -2 * r - 1)


def _best_k(u):
    """(cost, k) of one partition's zigzagged residuals"""
    best = None
    for k in range(15):
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
    u = _zigzag(_residual(s, o))  # u[i - o] belongs to frame i
    best = None
    for p in range((4 if n == B else 0) + 1):
        plen = n >> p
        parts = [_best_k(u[(j * plen - o if j else 0):(j + 1) * plen - o]) for j in range(1 << p)]
        cost = sum(4 + c for c, _ in parts)
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
    """values (int64 array, already masked to `width` bits) back to back from pos"""
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
    pos = _put(bits, pos, p, 6)
    u = _zigzag(_residual(s, o))
    plen = n >> p
    for j in range(1 << p):
        k = a["ks"][j]
        pos = _put(bits, pos, k, 4)
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
    """x: int16 [n * channels] interleaved -> the frame's bytes"""
    B = block_frames(B)
    x = np.asarray(x, np.int16).reshape(-1, channels).astype(np.int64)
    n = len(x)
    assert 1 <= n <= B
    if channels == 1:
        subs, assign = [(x[:, 0], 16)], 0
        an = [analyze(x[:, 0], 16, B)]
    else:
        L, R = x[:, 0], x[:, 1]
        cand = {"L": (L, 16), "R": (R, 16), "M": ((L + R) >> 1, 16), "S": (L - R, 17)}
        A = {k: analyze(v[0], v[1], B) for k, v in cand.items()}
        pairs = [("L", "R", 1), ("L", "S", 8), ("S", "R", 9), ("M", "S", 10)]
        costs = [A[a]["bits"] + A[b]["bits"] for a, b, _ in pairs]
        a, b, assign = pairs[costs.index(min(costs))]
        subs, an = [cand[a], cand[b]], [A[a], A[b]]
    code = 8 + BLOCKS.index(B) if n == B else 7
    head = bytes([0xff, 0xf8, code << 4, (assign << 4) | 0b1000]) + utf8(number)
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
    """the frames of one row (no header) -> (bytes, the frames' sizes). Without `finish` the frames behind the last complete
    block stay out."""
    B = block_frames(B)
    x = np.asarray(x, np.int16).reshape(-1, channels)
    sizes, out = [], []
    for k in range((len(x) + B - 1) // B if finish else len(x) // B):
        f = encode_block(x[k * B:(k + 1) * B].reshape(-1), channels, B, k)
        out.append(f)
        sizes.append(len(f))
    return b"".join(out), sizes


def info(frames, sizes):
    return dict(frames=frames, blocks=len(sizes), bytes=sum(sizes), min_frame_bytes=min(sizes) if sizes else 0,
                max_frame_bytes=max(sizes) if sizes else 0)


# ---- the decoder -----------------------------------------------------------------------------------------------------------

class Bad(Exception):
    pass


def parse_header(data):
    if data[:4] != b"fLaC" or bytes(data[4:8]) != bytes([0x80, 0, 0, 34]) or len(data) < 42:
        raise Bad("not the 42 header bytes")
    v = int.from_bytes(data[8:26], "big")
    h = dict(min_block=v >> 128, max_block=(v >> 112) & 0xffff, min_frame=(v >> 88) & 0xffffff, max_frame=(v >> 64) & 0xffffff,
             srate=(v >> 44) & 0xfffff, channels=((v >> 41) & 7) + 1, bps=((v >> 36) & 31) + 1, frames=v & ((1 << 36) - 1),
             md5=bytes(data[26:42]))
    return h


def _signed(v, bits):
    return v - (1 << bits) if v >> (bits - 1) else v


def decode_frame(data, at, channels, B, number):
    """one frame from data[at:] -> (int64 [n, channels], the position behind it, the kinds of its subframes)"""
    d = data
    if d[at] != 0xff or d[at + 1] != 0xf8:
        raise Bad("no sync code (or a reserved bit, or a variable block size) at %d" % at)
    code, rate = d[at + 2] >> 4, d[at + 2] & 15
    assign, size, zero = d[at + 3] >> 4, (d[at + 3] >> 1) & 7, d[at + 3] & 1
    if rate != 0 or size != 0b100 or zero != 0:
        raise Bad("sample rate code, sample size or the reserved bit")
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
    nbytes_max = frame_bound(n, channels) - (p - at)
    s = format(int.from_bytes(d[p:p + nbytes_max], "big"), "0%db" % (8 * len(d[p:p + nbytes_max])))
    pos = 0

    def take(w):
        nonlocal pos
        v = int(s[pos:pos + w], 2)
        pos += w
        return v

    subs, kinds = [], []
    for c in range(channels):
        bps = 17 if (assign, c) in ((8, 1), (9, 0), (10, 1)) else 16
        if take(1) != 0:
            raise Bad("subframe padding bit")
        t = take(6)
        if take(1) != 0:
            raise Bad("wasted bits flag")
        if t == 0:
            v = np.full(n, _signed(take(bps), bps), np.int64)
            kinds.append("constant")
        elif t == 1:
            v = np.array([_signed(int(s[pos + bps * i:pos + bps * (i + 1)], 2), bps) for i in range(n)], np.int64)
            pos += bps * n
            kinds.append("verbatim")
        elif 0b001000 <= t <= 0b001100:
            o = t & 7
            v = [_signed(take(bps), bps) for _ in range(o)]
            if take(2) != 0:
                raise Bad("residual coding method")
            po = take(4)
            if (n >> po) << po != n and po:
                raise Bad("partition order")
            for j in range(1 << po):
                k = take(4)
                if k > 14:
                    raise Bad("Rice parameter 15 (the escape)")
                for _ in range((n >> po) - (o if j == 0 else 0)):
                    one = s.index("1", pos)
                    u = ((one - pos) << k) | (int(s[one + 1:one + 1 + k], 2) if k else 0)
                    pos = one + 1 + k
                    r = (u >> 1) if not u & 1 else -((u + 1) >> 1)
                    i = len(v)
                    pred = [0, v[i - 1] if o > 0 else 0, 2 * v[i - 1] - v[i - 2] if o > 1 else 0,
                            3 * v[i - 1] - 3 * v[i - 2] + v[i - 3] if o > 2 else 0,
                            4 * v[i - 1] - 6 * v[i - 2] + 4 * v[i - 3] - v[i - 4] if o > 3 else 0][o]
                    v.append(r + pred)
            v = np.array(v, np.int64)
            kinds.append("fixed%d/p%d" % (o, po))
        else:
            raise Bad("subframe type %d" % t)
        if len(v) != n:
            raise Bad("subframe length")
        subs.append(v)
    pad = (-pos) % 8
    if take(pad) != 0 if pad else False:
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
    if out.min() < -32768 or out.max() > 32767:
        raise Bad("a sample beyond 16 bits")
    return out, end + 2, kinds


def decode_frames(data, channels, B, first=0):
    """frames back to back, numbered from `first` -> (int16 [frames * channels], the frames' sizes, their subframes' kinds).
    Every block but the last has B frames; the data ends with its last frame."""
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
    x = np.concatenate(out).astype(np.int16).reshape(-1) if out else np.zeros(0, np.int16)
    return x, sizes, kinds


def decode_file(data):
    """a whole file -> (header dict, int16 [frames * channels]); STREAMINFO is held against the frames"""
    data = bytes(data)
    h = parse_header(data)
    if h["min_block"] != h["max_block"] or h["bps"] != 16 or h["md5"] != bytes(16):
        raise Bad("STREAMINFO")
    x, sizes, _ = decode_frames(data[42:], h["channels"], h["max_block"])
    if len(x) != h["frames"] * h["channels"]:
        raise Bad("total samples")
    if (h["min_frame"], h["max_frame"]) != ((min(sizes), max(sizes)) if sizes else (0, 0)):
        raise Bad("frame sizes")
    return h, x


# ---- crafted material ------------------------------------------------------------------------------------------------------

KINDS = ("silence", "noise", "centre", "l_only", "anti", "unrelated", "sine", "extremes", "burst", "steps")


def crafted(kind, frames, channels, seed=0):
    """int16 [frames * channels]: silence; full-scale noise; a centre-panned tone (L == R); L only; anti-phase (R == -L);
    unrelated channels (a tone and a slower one); a sine; the extremes that make a side of +-65535; bursts (a few quiet values, then
    loud noise, by turns of 100 frames: partitions with different parameters); steps (a staircase and a ramp: orders 0 and 1)"""
    rng = np.random.default_rng(1000 + seed)
    t = np.arange(frames)
    tone = np.round(12000 * np.sin(2 * np.pi * 440 * t / 44100 + seed)).astype(np.int64)
    if kind == "silence":
        L = R = np.zeros(frames, np.int64)
    elif kind == "noise":
        L, R = rng.integers(-32768, 32768, frames), rng.integers(-32768, 32768, frames)
    elif kind == "centre":
        L = R = tone
    elif kind == "l_only":
        L, R = tone, np.zeros(frames, np.int64)
    elif kind == "anti":
        L, R = tone, -tone
    elif kind == "unrelated":
        L, R = tone, np.round(9000 * np.sin(2 * np.pi * 97 * t / 44100) + rng.integers(-40, 41, frames)).astype(np.int64)
    elif kind == "sine":
        L, R = tone, np.round(0.7 * tone).astype(np.int64)
    elif kind == "extremes":
        L = np.where(t % 2 == 0, 32767, -32768)
        R = np.where(t % 2 == 0, -32768, 32767)
    elif kind == "burst":
        loud = (t // 100) % 2 == 1
        L = np.where(loud, rng.integers(-9000, 9001, frames), rng.integers(-3, 4, frames))
        R = np.where(loud, rng.integers(-2, 3, frames), rng.integers(-700, 701, frames))
    elif kind == "steps":
        L, R = (t // 61) * 977 % 20001 - 10000, (t * 7) % 30011 - 15000
    else:
        raise ValueError(kind)
    x = np.stack([L, R], 1) if channels == 2 else L[:, None]
    return x.astype(np.int16).reshape(-1)


if __name__ == "__main__":  # python tests/flac_model.py: (re)make the golden stream
    import os
    _x = crafted("sine", 868, 2, seed=1)
    _frames, _sizes = encode_stream(_x, 2, 256)
    _path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flac_sine_stereo_b256.flac")
    open(_path, "wb").write(header(44100, 2, 256, 868, min(_sizes), max(_sizes)) + _frames)
    print(_path, 42 + len(_frames), "bytes")
