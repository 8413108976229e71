"""The LPC mode at 24 bits (include/saugns_amd.h, section "FLAC", paragraph "LPC at 24 bits") restated in numpy from that text
alone. It sits on tests/flac24_model.py (the FIXED analysis, the bit helpers, the quantiser, the crafted material) and on
tests/flac_lpc_model.py's levinson (steps 3 to 5 do not depend on the width); what the paragraph changes is written out here:
the window product >> 11, step 5b, the 64-bit coefficient sum, k = 0 .. 30 in five bits and method 01. The decoder of LPC
subframes is independent of the encoder: Python integers after RFC 9639, both CRCs, method 01, k <= 30, the precision code
1011, a shift in 0 .. 15, an order <= 8, and every residual inside int32. No third-party decoder has read these streams:
tests/golden/flac24_lpc_pm_stereo_b256.flac is there for anyone who has one."""
import numpy as np

import flac24_model as f24
import flac_lpc_model as l16
from flac24_model import (ASSIGN, BLOCKS, KINDS, NK, S24_MAX, S24_MIN, Bad, block_frames, crafted, crafted_f32, frame_bound,  # noqa: F401
                          header, info, parse_header, quantize)
from flac24_model import _best_k, _put, _put_many, _signed, _zigzag
from flac_model import crc8, crc16, utf8

MAX_ORDER = 8
PRECISION = 12
GOLDEN_NAME = "flac24_lpc_pm_stereo_b256.flac"


# ---- the material ----------------------------------------------------------------------------------------------------------

def pm_f32(frames, channels, seed=0):
    """float32 [frames * channels]: flac_lpc_model.pm's voice as floats -- a PM voice (220 Hz modulated by 330 Hz, index 2) of
    amplitude 0.27 plus a 3111 Hz partial of 0.12 at 44100 Hz; the right channel is the same at 0.6 of the amplitude with every
    phase moved by `seed`"""
    t = np.arange(frames)

    def voice(ph):
        return (0.27 * np.sin(2 * np.pi * 220 * t / 44100 + ph + 2 * np.sin(2 * np.pi * 330 * t / 44100 + ph))
                + 0.12 * np.sin(2 * np.pi * 3111 * t / 44100 + ph))

    L = voice(0.0)
    R = 0.6 * voice(float(seed))
    x = np.stack([L, R], 1) if channels == 2 else L[:, None]
    return x.astype(np.float32).reshape(-1)


def pm(frames, channels, seed=0):
    """pm_f32 through the quantiser: int32 [frames * channels]"""
    return quantize(pm_f32(frames, channels, seed), 1.0, 24)


def ar(p, frames, seed):
    """int64 [frames]: flac_lpc_model.ar(p) * 1200, a peak of 7200000: the material that makes the encoder choose order p"""
    return l16.ar(p, frames, seed) * 1200


def octuple_pole(p, frames, start=0, peak=S24_MAX):
    """int64 [frames]: the impulse response of 1 / (1 - p z^-1)^8 from frame `start` on, scaled to `peak` and rounded. Its
    predictor is (1 - p z^-1)^8 itself: the sum of |c[j]| is (1 + p)^8 - 1."""
    h = np.zeros(frames)
    h[start] = 1.0
    for _ in range(8):
        for i in range(1, frames):
            h[i] += p * h[i - 1]
    return np.round(h * (peak / np.abs(h).max())).astype(np.int64)


def guard_stream(frames=256):
    """int32 [frames * 2], B = 256: L = s and R = -s with s = octuple_pole(0.7) from frame 64 on. The side channel S = 2 s takes 25
    bits, where step 5b fires at half the sum: S loses order 8, L and R keep it."""
    s = octuple_pole(0.7, frames, start=64)
    return np.stack([s, -s], 1).astype(np.int32).reshape(-1)


def rows(L, R=None):
    """int32 [frames * channels], interleaved, of one or two int64 channels"""
    x = L[:, None] if R is None else np.stack([L, R], 1)
    assert x.min() >= S24_MIN and x.max() <= S24_MAX
    return x.astype(np.int32).reshape(-1)


# ---- the encoder -----------------------------------------------------------------------------------------------------------

def autocorrelation(s, B, M):
    """steps 1 and 2: the product s W in 64 bits, >> 11"""
    ws = (s.astype(np.int64) * l16.window(B)) >> 11
    assert np.abs(ws).max(initial=0) < 1 << 25
    n = len(s)
    return [int((ws[l:] * ws[:n - l]).sum()) for l in range(M + 1)]


def guard(cands, bps):
    """step 5b: {m: (q, shift)} without the orders with (S << (bps - 1)) >> shift >= 2^30, S the sum of |q[j]|"""
    return {m: (q, sh) for m, (q, sh) in cands.items() if ((sum(abs(int(v)) for v in q) << (bps - 1)) >> sh) < 1 << 30}


def guard_mask(mask, q, shift, bps):
    """step 5b on the shared function's arguments: the mask, q[(m - 1) * 8 + j], shift[m - 1]"""
    for m in range(1, MAX_ORDER + 1):
        if mask >> (m - 1) & 1:
            S = sum(abs(int(q[(m - 1) * 8 + j])) for j in range(m))
            if (S << (bps - 1)) >> int(shift[m - 1]) >= 1 << 30:
                mask &= ~(1 << (m - 1))
    return mask


def lpc_residual(s, q, shift):
    """step 6, for i = m .. n-1, in Python-sized integers held against the paragraph's bounds"""
    s = s.astype(np.int64)
    m, n = len(q), len(s)
    acc = np.zeros(n - m, np.int64)
    for j in range(m):
        acc += int(q[j]) * s[m - 1 - j:n - 1 - j]
    assert np.abs(acc).max(initial=0) < 1 << 39
    r = s[m:] - (acc >> shift)
    assert np.abs(r).max(initial=0) < 1 << 31
    return r


def analyze_lpc(s, bps, B, M, stat=None):
    """one channel candidate of a block -> dict(type, bits, ...) with type "lpc": order, p, ks, q, shift. stat (a dict): what
    step 5b took out, stat["guarded"] a list of (bps, order)."""
    a = f24.analyze(s, bps, B)
    n = len(s)
    if M == 0 or n != B or a["type"] == "constant":
        return a
    R = autocorrelation(s, B, M)
    if R[0] == 0:
        return a
    all_cands = l16.orders(R, M)
    cands = guard(all_cands, bps)
    if stat is not None:
        stat.setdefault("guarded", []).extend((bps, m) for m in sorted(set(all_cands) - set(cands)))
    best = None
    for m in sorted(cands):
        q, shift = cands[m]
        A = int(np.abs(lpc_residual(s, q, shift)[M - m:]).sum())
        est = min((1 + k) * (n - M) + ((2 * A) >> k) for k in range(NK)) + m * (bps + PRECISION)
        if best is None or est < best[0]:
            best = (est, m)
    if best is None:
        return a
    m = best[1]
    q, shift = cands[m]
    u = _zigzag(lpc_residual(s, q, shift))
    assert int(u.max(initial=0)) < 1 << 32
    bestp = None
    for p in range(5):
        plen = n >> p
        parts = [_best_k(u[(j * plen - m if j else 0):(j + 1) * plen - m]) for j in range(1 << p)]
        cost = sum(5 + c for c, _ in parts)
        if bestp is None or cost < bestp[0]:
            bestp = (cost, p, [k for _, k in parts])
    lpc = 8 + bps * m + 4 + 5 + PRECISION * m + 6 + bestp[0]
    verbatim = 8 + bps * n
    fixed = a["bits"] if a["type"] == "fixed" else None  # (None: VERBATIM <= FIXED)
    if fixed is None and verbatim <= lpc:
        return a
    if fixed is not None and fixed <= lpc:
        return a
    return dict(type="lpc", bits=lpc, order=m, p=bestp[1], ks=bestp[2], q=q, shift=shift)


def _write_sub(bits, pos, s, bps, a):
    if a["type"] != "lpc":
        return f24._write_sub(bits, pos, s, bps, a)
    s = s.astype(np.int64)
    mask = (1 << bps) - 1
    m, p, n = a["order"], a["p"], len(s)
    pos = _put(bits, pos, (0b100000 | (m - 1)) << 1, 8)
    pos = _put_many(bits, pos, s[:m] & mask, bps)
    pos = _put(bits, pos, PRECISION - 1, 4)
    pos = _put(bits, pos, a["shift"] & 31, 5)
    for v in a["q"]:
        pos = _put(bits, pos, v & 0xfff, PRECISION)
    pos = _put(bits, pos, 0b010000 | p, 6)  # method 01, the partition order
    u = _zigzag(lpc_residual(s, a["q"], a["shift"]))
    plen = n >> p
    for j in range(1 << p):
        k = a["ks"][j]
        pos = _put(bits, pos, k, 5)
        v = u[(j * plen - m if j else 0):(j + 1) * plen - m]
        q = v >> k
        lens = q + 1 + k
        start = pos + np.concatenate(([0], np.cumsum(lens)[:-1]))
        bits[start + q] = 1
        for i in range(k):
            bits[start + q + 1 + i] = (v >> (k - 1 - i)) & 1
        pos += int(lens.sum())
    return pos


def encode_block(x, channels, B, number, M, with_choice=False, stat=None):
    """x: int32 [n * channels] interleaved, every sample in -2^23 .. 2^23 - 1 -> the frame's bytes with max_lpc_order M"""
    assert 0 <= M <= MAX_ORDER
    B = block_frames(B)
    x = np.asarray(x, np.int64).reshape(-1, channels)
    n = len(x)
    assert 1 <= n <= B and x.min() >= S24_MIN and x.max() <= S24_MAX
    if channels == 1:
        subs, assign = [(x[:, 0], 24)], 0
        an = [analyze_lpc(x[:, 0], 24, B, M, stat)]
        A = {"L": an[0]}
    else:
        L, R = x[:, 0], x[:, 1]
        cand = {"L": (L, 24), "R": (R, 24), "M": ((L + R) >> 1, 24), "S": (L - R, 25)}
        A = {k: analyze_lpc(v[0], v[1], B, M, stat) for k, v in cand.items()}
        pairs = [("L", "R", 1), ("L", "S", 8), ("S", "R", 9), ("M", "S", 10)]
        costs = [A[a]["bits"] + A[b]["bits"] for a, b, _ in pairs]
        a, b, assign = pairs[costs.index(min(costs))]
        subs, an = [cand[a], cand[b]], [A[a], A[b]]
    code = 8 + BLOCKS.index(B) if n == B else 7
    head = bytes([0xff, 0xf8, code << 4, (assign << 4) | 0b1100]) + utf8(number)
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
        return frame, (ASSIGN[assign], an, A)
    return frame


def encode_stream(x, channels, B, M, finish=True):
    """the frames of one row (no header) -> (bytes, the frames' sizes)"""
    B = block_frames(B)
    x = np.asarray(x, np.int64).reshape(-1, channels)
    sizes, out = [], []
    for k in range((len(x) + B - 1) // B if finish else len(x) // B):
        f = encode_block(x[k * B:(k + 1) * B].reshape(-1), channels, B, k, M)
        out.append(f)
        sizes.append(len(f))
    return b"".join(out), sizes


# ---- the decoder (RFC 9639; what the section excludes is refused) -----------------------------------------------------------

def decode_frame(data, at, channels, B, number):
    """one frame from data[at:] -> (int64 [n, channels], the position behind it, the kinds of its subframes: "constant",
    "verbatim", "fixed<o>/p<p>", "lpc<o>/p<p>")"""
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

    def residuals(v, o, predict):
        """the coded residual section behind `o` warm-up samples; predict(v, i) is the prediction of sample i"""
        nonlocal pos
        if take(2) != 1:
            raise Bad("residual coding method (not 01)")
        po = take(4)
        if po and (n >> po) << po != n:
            raise Bad("partition order")
        if (n >> po) < o:
            raise Bad("a first partition shorter than the order")
        for j in range(1 << po):
            k = take(5)
            if k > 30:
                raise Bad("Rice parameter 31 (the escape)")
            for _ in range((n >> po) - (o if j == 0 else 0)):
                one = s.index("1", pos)
                u = ((one - pos) << k) | (int(s[one + 1:one + 1 + k], 2) if k else 0)
                pos = one + 1 + k
                r = (u >> 1) if not u & 1 else -((u + 1) >> 1)
                if not -(1 << 31) <= r < 1 << 31:
                    raise Bad("a residual beyond int32")
                v.append(r + predict(v, len(v)))
        return po

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
            kinds.append("constant")
        elif t == 1:
            v = np.array([_signed(int(s[pos + bps * i:pos + bps * (i + 1)], 2), bps) for i in range(n)], np.int64)
            pos += bps * n
            kinds.append("verbatim")
        elif 0b001000 <= t <= 0b001100:
            o = t & 7
            coef = f24._PRED[o]
            v = [_signed(take(bps), bps) for _ in range(o)]
            po = residuals(v, o, lambda v, i: sum(cf * v[i - 1 - m] for m, cf in enumerate(coef)))
            v = np.array(v, np.int64)
            kinds.append("fixed%d/p%d" % (o, po))
        elif t >= 0b100000:
            # RFC 9639, 9.2.6: the order is the low five bits plus one; the unencoded warm-up samples; the predictor coefficient
            # precision minus one in four bits; the right shift as a signed five-bit number that must not be negative; the
            # coefficients, signed, of that precision; the residual. A sample is predicted from the ones before it, the first
            # coefficient times the most recent one, the sum shifted right (arithmetically) by the shift.
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


def decode_file(data, md5=None):
    """a whole 24-bit file -> (header dict, int32 [frames * channels], the kinds); STREAMINFO is held against the frames, its MD5
    field against `md5` (None: zeros)"""
    data = bytes(data)
    h = parse_header(data)
    if h["min_block"] != h["max_block"] or h["bps"] != 24 or h["md5"] != (bytes(16) if md5 is None else md5):
        raise Bad("STREAMINFO")
    x, sizes, kinds = decode_frames(data[42:], h["channels"], h["max_block"])
    if len(x) != h["frames"] * h["channels"]:
        raise Bad("total samples")
    if (h["min_frame"], h["max_frame"]) != ((min(sizes), max(sizes)) if sizes else (0, 0)):
        raise Bad("frame sizes")
    return h, x, kinds


def lpc_orders_seen(kinds):
    """the LPC orders among decode_frames' kinds"""
    return {int(k[3]) for kd in kinds for k in kd if k.startswith("lpc")}


def golden_samples():
    """the golden stream's samples: 3 * 256 + 100 stereo frames of the PM voice"""
    return pm(3 * 256 + 100, 2, seed=1)


if __name__ == "__main__":  # python tests/flac24_lpc_model.py: (re)make the golden stream
    import os
    _x = golden_samples()
    _frames, _sizes = encode_stream(_x, 2, 256, 8)
    _path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN_NAME)
    open(_path, "wb").write(header(44100, 2, 256, len(_x) // 2, min(_sizes), max(_sizes)) + _frames)
    print(_path, 42 + len(_frames), "bytes")
