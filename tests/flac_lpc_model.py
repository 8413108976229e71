"""The LPC mode of the FLAC encoder (include/saugns_amd.h, section "FLAC", "The LPC mode") restated in numpy from that text
alone, on top of tests/flac_model.py (whose CRCs, frame-number coding, FIXED analysis, bit helpers and crafted material it
uses), and an independent decoder of CONSTANT, VERBATIM, FIXED and LPC subframes. The decoder's LPC branch follows RFC 9639's
wording in Python integers and shares nothing with the encoder; like flac_model's it verifies both CRCs, the frame numbers,
every reserved bit, k <= 14, and for LPC the precision code 1011, a shift in 0 .. 15 and an order <= 8. No third-party decoder
has read these streams: tests/golden/flac_lpc_pm_stereo_b256.flac is there for anyone who has one."""
import math
import struct
from fractions import Fraction

import numpy as np

import flac_model as fm
from flac_model import (ASSIGN, BLOCKS, KINDS, Bad, analyze, block_frames, crafted, crc8, crc16, frame_bound, header, info,  # noqa: F401
                        parse_header, utf8)
from flac_model import _best_k, _put, _put_many, _residual, _signed, _zigzag

MAX_ORDER = 8
PRECISION = 12


# ---- the material ----------------------------------------------------------------------------------------------------------

def pm(frames, channels, seed=0):
    """int16 [frames * channels]: a PM voice (220 Hz modulated by 330 Hz, index 2) plus a 3111 Hz partial at 44100 Hz; the right
    channel is the same at 0.6 of the amplitude with every phase moved by `seed`"""
    t = np.arange(frames)

    def voice(ph):
        return (9000 * np.sin(2 * np.pi * 220 * t / 44100 + ph + 2 * np.sin(2 * np.pi * 330 * t / 44100 + ph))
                + 4000 * np.sin(2 * np.pi * 3111 * t / 44100 + ph))

    L = np.round(voice(0.0)).astype(np.int64)
    R = np.round(0.6 * voice(float(seed))).astype(np.int64)
    x = np.stack([L, R], 1) if channels == 2 else L[:, None]
    return x.astype(np.int16).reshape(-1)


def side_extremes(frames):
    """stereo int16 whose side channel alternates between -65535 and +65535: the largest values a 17-bit candidate has"""
    t = np.arange(frames)
    L = np.where(t % 2 == 1, 32767, -32768)
    R = np.where(t % 2 == 1, -32768, 32767)
    return np.stack([L, R], 1).astype(np.int16).reshape(-1)


def quiet_sine(frames, channels):
    """a sine of amplitude 3"""
    t = np.arange(frames)
    L = np.round(3 * np.sin(2 * np.pi * 440 * t / 44100)).astype(np.int64)
    R = np.round(3 * np.sin(2 * np.pi * 440 * t / 44100 + 1.0)).astype(np.int64)
    x = np.stack([L, R], 1) if channels == 2 else L[:, None]
    return x.astype(np.int16).reshape(-1)


def ar(p, frames, seed):
    """int64 [frames]: an all-pole process of order p -- the reflection coefficients (0.92 for even m, -0.85 for odd m) * (1 - 0.03 m),
    m = 0 .. p-1, stepped up to the direct form, driven by unit Gaussian noise, the first 64 frames discarded, scaled to a peak of
    6000 and rounded. Its best predictor has exactly p taps: the material that makes the encoder choose every order."""
    a = []
    for m in range(p):
        k = (0.92 if m % 2 == 0 else -0.85) * (1 - 0.03 * m)
        a = [a[j] + k * a[m - 1 - j] for j in range(m)] + [k]
    e = np.random.default_rng(seed).standard_normal(frames + 64)
    y = np.zeros(frames + 64)
    for i in range(len(y)):
        y[i] = e[i] - sum(a[j] * y[i - 1 - j] for j in range(min(p, i)))
    y = y[64:]
    return np.round(y * (6000 / np.abs(y).max())).astype(np.int64)


def impulse(frames, B):
    """int64 [frames]: zeros and one sample of 1000 in the middle of every block: R[1 ..] = 0, no candidate order"""
    s = np.zeros(frames, np.int64)
    s[B // 2::B] = 1000
    return s


def pair(frames, B):
    """int64 [frames]: two samples of 1000 two frames apart in every block: R[1] = 0 and R[2] != 0, so order 1 is no candidate (its
    cmax is 0) and order 2 is one"""
    s = impulse(frames, B)
    s[B // 2 + 2::B] = 1000
    return s


def edge(frames, B, v):
    """int64 [frames]: zeros but the first sample of every block, v -- where the window is smallest: W[0] is 1 at B = 4096 and 7 at
    B = 1024, so ws[0] = (v W[0]) >> 3 is 0 for v = +7 resp. +1 (a block that is not constant with R[0] == 0) and -1 for v = -1 at
    B = 4096 (R[0] = 1)"""
    s = np.zeros(frames, np.int64)
    s[::B] = v
    return s


def rows(L, R=None):
    """int16 [frames * channels], interleaved, of one or two int64 channels"""
    x = L[:, None] if R is None else np.stack([L, R], 1)
    assert x.min() >= -32768 and x.max() <= 32767
    return x.astype(np.int16).reshape(-1)


# ---- the encoder: steps 1 .. 9 -------------------------------------------------------------------------------------------

def window(B):
    lg = B.bit_length() - 1
    j = np.arange(B, dtype=np.int64)
    return (B * B - (2 * j + 1 - B) ** 2) >> (2 * lg - 12)


def _bits(x):
    return struct.unpack(">Q", struct.pack(">d", x))[0]


def autocorrelation(s, B, M):
    ws = (s.astype(np.int64) * window(B)) >> 3
    n = len(s)
    return [int((ws[l:] * ws[:n - l]).sum()) for l in range(M + 1)]


def _muladd(x, y, z, fused):
    """x * y + z: the product rounded before the sum as the header has it, or (fused) the whole as one correctly rounded operation,
    which is what a fused multiply-add instruction gives"""
    if not fused or not all(map(math.isfinite, (x, y, z))):
        return x * y + z
    exact = Fraction(x) * Fraction(y) + Fraction(z)
    if exact == 0:
        return x * y + z  # (the sign of an exact zero is the sum's)
    try:
        return float(exact)  # (an int / int division: correctly rounded)
    except OverflowError:
        return math.copysign(math.inf, exact)


def levinson(R, M, fused=False):
    """steps 3 .. 5 for one autocorrelation R[0 .. M] (more values are not read) -> (g, the mask of the candidate orders with bit
    m - 1 for order m, {m: (q[0 .. m-1], shift)}, the bit patterns of a[0 .. M-1] as they stand when the loop ends, the i at which
    the recursion stopped or None, what happened on the way: dict(stop: that i, cmax_zero: the orders skipped because cmax is 0
    or subnormal, shift15: those whose shift was above 15, qmax: those with a q clamped to +2047, qmin: those with a q at -2048
    -- the clamp's other end: |c 2^shift| < 2048 and E >= -0.5 keep floor(E + 0.5) from passing it)).
    fused=True does every `z + x * y` of steps 4 and 5 (1.0 - k * k and E + c[j] * 2^shift among them) as one rounded operation:
    what a build that contracts products into sums computes. Nothing but tests/test_flac_lpc_steps_host.py's proof that its
    inputs tell the two apart uses it."""
    g = 0
    while (R[0] >> g) >= 1 << 53:
        g += 1
    r = [float(v >> g) for v in R[:M + 1]]
    assert all(int(v) == w >> g for v, w in zip(r, R))
    a = [0.0] * M
    err = r[0]
    out, mask, stop = {}, 0, None
    seen = dict(stop=None, cmax_zero=[], shift15=[], qmax=[], qmin=[])
    for i in range(M):
        acc = r[i + 1]
        for j in range(i):
            acc = _muladd(a[j], r[i - j], acc, fused)
        k = -acc / err
        a[i] = k
        for j in range(i // 2):
            t, u = a[j], a[i - 1 - j]
            a[j] = _muladd(k, u, t, fused)
            a[i - 1 - j] = _muladd(k, t, u, fused)
        if i % 2 == 1:
            t = a[i // 2]
            a[i // 2] = _muladd(k, t, t, fused)
        err = err * _muladd(-k, k, 1.0, fused)
        if not err > 0.0 or math.isinf(err):
            stop = seen["stop"] = i
            break
        m = i + 1
        c = [-a[j] for j in range(m)]
        cmax = 0.0
        for v in c:
            if abs(v) > cmax:
                cmax = abs(v)
        field = (_bits(cmax) >> 52) & 0x7ff
        if field == 0 or field == 0x7ff:  # 0 or subnormal; not finite
            if field == 0:
                seen["cmax_zero"].append(m)
            continue
        e = field - 1022  # 2^(e-1) <= cmax < 2^e
        shift = PRECISION - 1 - e
        if shift > 15:
            seen["shift15"].append(m)
            shift = 15
        if shift < 0:
            continue
        E, q = 0.0, []
        for j in range(m):
            E = _muladd(c[j], float(1 << shift), E, fused)
            v = int(math.floor(E + 0.5))
            if v > 2047 and m not in seen["qmax"]:
                seen["qmax"].append(m)
            if v <= -2048 and m not in seen["qmin"]:
                seen["qmin"].append(m)
            v = max(-2048, min(2047, v))
            q.append(v)
            E = E - float(v)
        out[m] = (q, shift)
        mask |= 1 << i
    return g, mask, out, [_bits(v) for v in a], stop, seen


def orders(R, M):
    """steps 3 .. 5: {m: (q[0 .. m-1], shift)} of the candidate orders"""
    return levinson(R, M)[2]


def lpc_residual(s, q, shift):
    """step 6, for i = m .. n-1"""
    s = s.astype(np.int64)
    m, n = len(q), len(s)
    acc = np.zeros(n - m, np.int64)
    for j in range(m):
        acc += q[j] * s[m - 1 - j:n - 1 - j]
    assert np.abs(acc).max(initial=0) < 1 << 30
    r = s[m:] - (acc >> shift)
    assert np.abs(r).max(initial=0) < 1 << 31
    return r


def analyze_lpc(s, bps, B, M):
    """one channel candidate of a block -> dict(type, bits, ...) with type "lpc": order, p, ks, q, shift"""
    a = analyze(s, bps, B)
    n = len(s)
    if M == 0 or n != B or a["type"] == "constant":
        return a
    R = autocorrelation(s, B, M)
    if R[0] == 0:
        return a
    cands = orders(R, M)
    best = None
    for m in sorted(cands):
        q, shift = cands[m]
        A = int(np.abs(lpc_residual(s, q, shift)[M - m:]).sum())
        est = min((1 + k) * (n - M) + ((2 * A) >> k) for k in range(15)) + m * (bps + PRECISION)
        if best is None or est < best[0]:
            best = (est, m)
    if best is None:
        return a
    m = best[1]
    q, shift = cands[m]
    u = _zigzag(lpc_residual(s, q, shift))
    bestp = None
    for p in range(5):
        plen = n >> p
        parts = [_best_k(u[(j * plen - m if j else 0):(j + 1) * plen - m]) for j in range(1 << p)]
        cost = sum(4 + c for c, _ in parts)
        if bestp is None or cost < bestp[0]:
            bestp = (cost, p, [k for _, k in parts])
    lpc = 8 + bps * m + 4 + 5 + PRECISION * m + 6 + bestp[0]
    verbatim = 8 + bps * n
    fixed = a["bits"] if a["type"] == "fixed" else None  # (None: VERBATIM <= FIXED)
    if fixed is None and verbatim <= lpc:
        return a  # VERBATIM is <= both others
    if fixed is not None and fixed <= lpc:
        return a  # FIXED (it is below VERBATIM)
    return dict(type="lpc", bits=lpc, order=m, p=bestp[1], ks=bestp[2], q=q, shift=shift)


def _write_sub(bits, pos, s, bps, a):
    if a["type"] != "lpc":
        return fm._write_sub(bits, pos, s, bps, a)
    s = s.astype(np.int64)
    mask = (1 << bps) - 1
    m, p, n = a["order"], a["p"], len(s)
    pos = _put(bits, pos, (0b100000 | (m - 1)) << 1, 8)
    pos = _put_many(bits, pos, s[:m] & mask, bps)
    pos = _put(bits, pos, PRECISION - 1, 4)
    pos = _put(bits, pos, a["shift"] & 31, 5)
    for v in a["q"]:
        pos = _put(bits, pos, v & 0xfff, PRECISION)
    pos = _put(bits, pos, p, 6)
    u = _zigzag(lpc_residual(s, a["q"], a["shift"]))
    plen = n >> p
    for j in range(1 << p):
        k = a["ks"][j]
        pos = _put(bits, pos, k, 4)
        v = u[(j * plen - m if j else 0):(j + 1) * plen - m]
        q = v >> k
        lens = q + 1 + k
        start = pos + np.concatenate(([0], np.cumsum(lens)[:-1]))
        bits[start + q] = 1
        for i in range(k):
            bits[start + q + 1 + i] = (v >> (k - 1 - i)) & 1
        pos += int(lens.sum())
    return pos


def encode_block(x, channels, B, number, M, with_choice=False):
    """x: int16 [n * channels] interleaved -> the frame's bytes with max_lpc_order M"""
    assert 0 <= M <= MAX_ORDER
    B = block_frames(B)
    x = np.asarray(x, np.int16).reshape(-1, channels).astype(np.int64)
    n = len(x)
    assert 1 <= n <= B
    if channels == 1:
        subs, assign = [(x[:, 0], 16)], 0
        an = [analyze_lpc(x[:, 0], 16, B, M)]
    else:
        L, R = x[:, 0], x[:, 1]
        cand = {"L": (L, 16), "R": (R, 16), "M": ((L + R) >> 1, 16), "S": (L - R, 17)}
        A = {k: analyze_lpc(v[0], v[1], B, M) for k, v in cand.items()}
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


def encode_stream(x, channels, B, M, finish=True):
    """the frames of one row (no header) -> (bytes, the frames' sizes)"""
    B = block_frames(B)
    x = np.asarray(x, np.int16).reshape(-1, channels)
    sizes, out = [], []
    for k in range((len(x) + B - 1) // B if finish else len(x) // B):
        f = encode_block(x[k * B:(k + 1) * B].reshape(-1), channels, B, k, M)
        out.append(f)
        sizes.append(len(f))
    return b"".join(out), sizes


# ---- the decoder -----------------------------------------------------------------------------------------------------------

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

    def residuals(v, o, predict):
        """the coded residual section behind `o` warm-up samples; predict(v, i) is the prediction of sample i"""
        nonlocal pos
        if take(2) != 0:
            raise Bad("residual coding method")
        po = take(4)
        if (n >> po) << po != n and po:
            raise Bad("partition order")
        if (n >> po) < o:
            raise Bad("a first partition shorter than the order")
        for j in range(1 << po):
            k = take(4)
            if k > 14:
                raise Bad("Rice parameter 15 (the escape)")
            for _ in range((n >> po) - (o if j == 0 else 0)):
                one = s.index("1", pos)
                u = ((one - pos) << k) | (int(s[one + 1:one + 1 + k], 2) if k else 0)
                pos = one + 1 + k
                r = (u >> 1) if not u & 1 else -((u + 1) >> 1)
                v.append(r + predict(v, len(v)))
        return po

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
            po = residuals(v, o, lambda v, i: [0, v[i - 1] if o > 0 else 0, 2 * v[i - 1] - v[i - 2] if o > 1 else 0,
                                               3 * v[i - 1] - 3 * v[i - 2] + v[i - 3] if o > 2 else 0,
                                               4 * v[i - 1] - 6 * v[i - 2] + 4 * v[i - 3] - v[i - 4] if o > 3 else 0][o])
            v = np.array(v, np.int64)
            kinds.append("fixed%d/p%d" % (o, po))
        elif t >= 0b100000:
            # RFC 9639, 9.2.6: the order is the low five bits plus one; the unencoded warm-up samples; the predictor
            # coefficient precision minus one in four bits (1111 is forbidden); the right shift needed as a signed five-bit
            # number that must not be negative; the coefficients, signed, of that precision; the residual. A sample is
            # predicted from the ones before it, the first coefficient times the most recent one, the sum shifted right
            # (arithmetically) by the shift.
            o = (t & 31) + 1
            if o > MAX_ORDER:
                raise Bad("LPC order %d" % o)
            if o > n:
                raise Bad("an LPC order above the block's length")
            v = [_signed(take(bps), bps) for _ in range(o)]
            if take(4) != 0b1011:
                raise Bad("coefficient precision code")
            shift = _signed(take(5), 5)
            if not 0 <= shift <= 15:
                raise Bad("LPC shift %d" % shift)
            coef = [_signed(take(12), 12) for _ in range(o)]
            po = residuals(v, o, lambda v, i: sum(coef[j] * v[i - 1 - j] for j in range(o)) >> shift)
            v = np.array(v, np.int64)
            kinds.append("lpc%d/p%d" % (o, po))
        else:
            raise Bad("subframe type %d" % t)
        if len(v) != n:
            raise Bad("subframe length")
        if v.min() < -(1 << (bps - 1)) or v.max() >= 1 << (bps - 1):
            raise Bad("a sample beyond the subframe's bits")
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
    """frames back to back, numbered from `first` -> (int16 [frames * channels], the frames' sizes, their subframes' kinds)"""
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
    """a whole file -> (header dict, int16 [frames * channels], the kinds); STREAMINFO is held against the frames"""
    data = bytes(data)
    h = parse_header(data)
    if h["min_block"] != h["max_block"] or h["bps"] != 16 or h["md5"] != bytes(16):
        raise Bad("STREAMINFO")
    x, sizes, kinds = decode_frames(data[42:], h["channels"], h["max_block"])
    if len(x) != h["frames"] * h["channels"]:
        raise Bad("total samples")
    if (h["min_frame"], h["max_frame"]) != ((min(sizes), max(sizes)) if sizes else (0, 0)):
        raise Bad("frame sizes")
    return h, x, kinds


if __name__ == "__main__":  # python tests/flac_lpc_model.py: (re)make the golden stream
    import os
    _x = pm(868, 2, seed=1)
    _frames, _sizes = encode_stream(_x, 2, 256, 8)
    _path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flac_lpc_pm_stereo_b256.flac")
    open(_path, "wb").write(header(44100, 2, 256, 868, min(_sizes), max(_sizes)) + _frames)
    print(_path, 42 + len(_frames), "bytes")
