"""The decoder's test material, shared by tests/test_flac_verify_host.py, tests/test_flac_verify_sanitize.py and
tests/test_gpu_flac_verify.py: frames that the library's host restatements of the encoders make of the models' crafted material,
frames built bit by bit here (a valid LPC frame at shift 15, and the refusals, each with its CRCs recomputed by flac_model's crc8
and crc16), and the names of the statuses. Nothing here runs a GPU."""
import functools

import numpy as np

import flac24_lpc_model as m24l
import flac24_model as m24
import flac_lpc_model as m16l
import flac_model as m16

OK, LENGTH, SYNC, HEADER, NUMBER, CRC8, SUBFRAME, RESIDUAL, PADDING, CRC16, RANGE, MISMATCH = range(12)
BAD_ARGUMENT = 255
NAMES = ("OK", "LENGTH", "SYNC", "HEADER", "NUMBER", "CRC8", "SUBFRAME", "RESIDUAL", "PADDING", "CRC16", "RANGE", "MISMATCH")

# mode -> (bits, max_lpc_order, the model whose decode_frame reads its frames)
MODES = {"encode_block": (16, 0, m16), "lpc": (16, 8, m16l), "s32": (24, 0, m24), "lpc24": (24, 8, m24l)}
BLOCKS = (256, 4096)
LENGTHS = lambda B: (1, 2, 4, 5, 255, B)  # noqa: E731


def material(mode, kind, n, channels, B):
    """interleaved samples [n * channels] (int16 values at 16 bits, int32 at 24) of `kind` for a mode"""
    bits = MODES[mode][0]
    if kind in m16.KINDS:
        x = m16.crafted(kind, n, channels, seed=3).astype(np.int32)
        return x if bits == 16 else x * 256  # (-32768 becomes -2^23, the least a 24-bit sample may be)
    if kind == "pm":
        return m16l.pm(n, channels, seed=1).astype(np.int32) if bits == 16 else np.asarray(m24l.pm(n, channels, seed=1), np.int32)
    if kind == "ar8":
        s = m16l.ar(8, n + 8, 5)[:n] if n > 8 else np.arange(n, dtype=np.int64) * 37 - 50
        s = s if bits == 16 else s * 1200
        return (np.stack([s, -s // 2], 1) if channels == 2 else s[:, None]).astype(np.int32).reshape(-1)
    if kind == "side_extremes":  # (16 bits, stereo: a side of +-65535)
        return m16l.side_extremes(n).astype(np.int32)
    return np.asarray(m24.crafted(kind[3:], n, channels, seed=3, B=B), np.int32)  # "24:<kind>": the 24-bit model's extremes


def kinds_of(mode):
    bits, M, _ = MODES[mode]
    k = list(m16.KINDS)
    if bits == 24:
        k += ["24:" + x for x in m24.KINDS]
    if M:
        k += ["pm", "ar8"]
    return k


def encode(sa, mode, x, channels, B, number):
    bits, M, _ = MODES[mode]
    if mode == "encode_block":
        return sa.flac_encode_block(np.asarray(x, np.int16), channels, B, number)
    if mode == "lpc":
        return sa.flac_encode_block(np.asarray(x, np.int16), channels, B, number, M)
    if mode == "s32":
        return sa.flac_encode_block_s32(x, channels, B, number, 24, 0)
    return sa.flac_encode_block_lpc24(x, channels, B, number, M)


_valid = {}


def valid_cases(sa):
    """every (mode, kind, channels, B, n): dicts with the frame, its parameters and the samples it was made of"""
    if _valid:
        return _valid["v"]
    out = []
    for mode in MODES:
        bits = MODES[mode][0]
        kinds = kinds_of(mode) + (["side_extremes"] if bits == 16 else [])
        for kind in kinds:
            for channels in (1, 2):
                if kind == "side_extremes" and channels == 1:
                    continue
                for B in BLOCKS:
                    for n in LENGTHS(B):
                        number = (len(out) * 2654435761) % (1 << 31) if len(out) % 3 == 0 else len(out)  # (every length of the number's coding)
                        x = material(mode, kind, n, channels, B)
                        fr = encode(sa, mode, x, channels, B, number)
                        assert fr, (mode, kind, channels, B, n)
                        out.append(dict(mode=mode, kind=kind, channels=channels, B=B, n=n, bits=bits, number=number, frame=fr, x=x))
    _valid["v"] = out
    return out


# ---- frames built bit by bit ---------------------------------------------------------------------------------------------

class Bits:
    def __init__(self):
        self.b = []

    def put(self, v, w):
        v &= (1 << w) - 1
        self.b += [(v >> (w - 1 - i)) & 1 for i in range(w)]
        return self

    def __len__(self):
        return len(self.b)


def rice(bw, r, k):
    u = 2 * r if r >= 0 else -2 * r - 1
    bw.put(0, u >> k) if u >> k else None
    bw.put(1, 1)
    bw.put(u, k) if k else None


def build(channels, bits, B, n, number, body, assign=None, code=None, pad=0, crc8_add=0, crc16_add=0, raw_n=None):
    """a frame from its header fields and the subframes' bits (a Bits). code: the block size code (the right one when None); raw_n:
    the 16 bits behind a code 0111 (n - 1 when None); pad: the value of the padding bits; crc*_add: added to the right CRC."""
    if assign is None:
        assign = 0 if channels == 1 else 1
    if code is None:
        code = 8 + (256, 512, 1024, 2048, 4096).index(B) if n == B else 7
    head = bytes([0xff, 0xf8, code << 4, (assign << 4) | ((6 if bits == 24 else 4) << 1)]) + m16.utf8(number)
    if code == 7:
        head += ((n - 1) if raw_n is None else raw_n).to_bytes(2, "big")
    head += bytes([(m16.crc8(head) + crc8_add) & 0xff])
    b = list(body.b)
    padding = (-len(b)) % 8
    b += [(pad >> (padding - 1 - i)) & 1 for i in range(padding)]
    body_bytes = np.packbits(np.array(b, np.uint8)).tobytes() if b else b""
    fr = head + body_bytes
    return fr + ((m16.crc16(fr) + crc16_add) & 0xffff).to_bytes(2, "big")


def sub_fixed0(bw, bps, samples, k, method, kw, p=0, wasted=0):
    """a FIXED subframe of order 0 with one partition of parameter k"""
    bw.put(0, 1).put(0b001000, 6).put(wasted, 1).put(method, 2).put(p, 4).put(k, kw)
    for s in samples:
        rice(bw, int(s), k if k < (1 << kw) - 1 else 0)
    return bw


def sub_lpc1(bw, bps, samples, q, shift, k, method, kw, precision=11):
    """an LPC subframe of order 1: coefficient q, `shift`, one partition of parameter k"""
    s = [int(v) for v in samples]
    bw.put(0, 1).put(0b100000, 6).put(0, 1).put(s[0], bps).put(precision, 4).put(shift, 5).put(q, 12).put(method, 2).put(0, 4).put(k, kw)
    for i in range(1, len(s)):
        rice(bw, s[i] - ((q * s[i - 1]) >> shift), k)
    return bw


def handmade_valid():
    """frames no encoder here makes but the format above allows: (name, frame, channels, B, bits, number, samples)"""
    out = []
    for bits, method, kw, k, amp in ((16, 0, 4, 11, 3000), (24, 1, 5, 17, 100000)):
        for B in (256, 4096):
            t = np.arange(B)
            s = np.round(amp * np.sin(2 * np.pi * t / 97.0)).astype(np.int64)
            body = sub_lpc1(Bits(), bits, s, 2047, 15, k, method, kw)
            out.append(("lpc1 at shift 15, %d bits, B %d" % (bits, B), build(1, bits, B, B, 5, body), 1, B, bits, 5, s.astype(np.int32)))
    return out


def corrupt_cases():
    """(name, frame, channels, B, bits, expected frame number, status): each refusal of the issue's table, at both widths where the
    width matters, and a few more of every status"""
    out = []
    s4 = [3, -2, 0, 5]  # (33 or 34 bits of subframe: both widths have padding bits)

    def add(name, status, fr, channels=1, B=256, bits=16, number=9):
        out.append((name, fr, channels, B, bits, number, status))

    for bits, method, kw in ((16, 0, 4), (24, 1, 5)):
        w = " (%d bits)" % bits
        good = lambda **kv: sub_fixed0(Bits(), bits, s4, kv.pop("k", 2), kv.pop("method", method), kw, **kv)  # noqa: E731
        add("a well-formed short frame" + w, OK, build(1, bits, 256, 4, 9, good()), bits=bits)
        add("wrong frame number" + w, NUMBER, build(1, bits, 256, 4, 10, good()), bits=bits)
        add("escape parameter" + w, RESIDUAL, build(1, bits, 256, 4, 9, good(k=(1 << kw) - 1)), bits=bits)
        add("the other width's method" + w, RESIDUAL, build(1, bits, 256, 4, 9, good(method=1 - method)), bits=bits)
        add("partition order 1 on a short block" + w, RESIDUAL, build(1, bits, 256, 4, 9, good(p=1)), bits=bits)
        add("partition order 5 on a whole block" + w, RESIDUAL,
            build(1, bits, 256, 256, 9, sub_fixed0(Bits(), bits, [0] * 256, 0, method, kw, p=5)), bits=bits)
        add("wasted-bits flag" + w, SUBFRAME, build(1, bits, 256, 4, 9, good(wasted=1)), bits=bits)
        add("subframe padding bit" + w, SUBFRAME, build(1, bits, 256, 4, 9, Bits().put(1, 1).put(0, 7).put(0, bits)), bits=bits)
        add("reserved subframe type" + w, SUBFRAME, build(1, bits, 256, 4, 9, Bits().put(0, 1).put(0b000010, 6).put(0, 1).put(0, bits)), bits=bits)
        add("FIXED order 5" + w, SUBFRAME, build(1, bits, 256, 256, 9, Bits().put(0, 1).put(0b001101, 6).put(0, 1).put(0, 5 * bits)), bits=bits)
        add("LPC order 9" + w, SUBFRAME, build(1, bits, 256, 256, 9, Bits().put(0, 1).put(0b101000, 6).put(0, 1).put(0, 9 * bits)), bits=bits)
        ramp = np.arange(256) * 3
        add("LPC precision 11" + w, SUBFRAME, build(1, bits, 256, 256, 9, sub_lpc1(Bits(), bits, ramp, 1024, 10, 3, method, kw, precision=10)), bits=bits)
        add("LPC shift -1" + w, SUBFRAME, build(1, bits, 256, 256, 9, sub_lpc1(Bits(), bits, ramp, 1024, 31, 3, method, kw)), bits=bits)
        add("LPC in a short block" + w, SUBFRAME, build(1, bits, 256, 4, 9, sub_lpc1(Bits(), bits, s4, 1024, 10, 3, method, kw)), bits=bits)
        add("a well-formed LPC frame" + w, OK, build(1, bits, 256, 256, 9, sub_lpc1(Bits(), bits, ramp, 1024, 10, 3, method, kw)), bits=bits)
        assert len(good()) % 8, "the short frame has padding bits"
        add("non-zero padding" + w, PADDING, build(1, bits, 256, 4, 9, good(), pad=1), bits=bits)
        add("CRC-8 off by one" + w, CRC8, build(1, bits, 256, 4, 9, good(), crc8_add=1), bits=bits)
        add("CRC-16 off by one" + w, CRC16, build(1, bits, 256, 4, 9, good(), crc16_add=1), bits=bits)
        add("block size code 0111 carrying n == B" + w, HEADER,
            build(1, bits, 256, 256, 9, sub_fixed0(Bits(), bits, [0] * 256, 0, method, kw), code=7), bits=bits)
        add("block size code of another B" + w, HEADER, build(1, bits, 256, 256, 9, Bits().put(0, 8 + bits), code=9), bits=bits)
        add("the other width's sample size code" + w, HEADER, build(1, 40 - bits, 256, 4, 9, good()), bits=bits)
        add("mono frame for a stereo stream" + w, HEADER, build(1, bits, 256, 4, 9, good()), channels=2, bits=bits)
        add("channel assignment 2" + w, HEADER, build(2, bits, 256, 4, 9, good(), assign=2), channels=2, bits=bits)
        lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
        const = lambda v, bps: Bits().put(0, 8).put(v, bps)  # noqa: E731
        both = lambda a, b: Bits().put(0, 8).put(a[0], a[1]).put(0, 8).put(b[0], b[1])  # noqa: E731
        add("left/side whose R leaves the bits" + w, RANGE, build(2, bits, 256, 4, 9, both((hi, bits), (-(1 << bits), bits + 1)), assign=8), channels=2, bits=bits)
        add("side/right whose L leaves the bits" + w, RANGE, build(2, bits, 256, 4, 9, both(((1 << bits) - 1, bits + 1), (hi, bits)), assign=9), channels=2, bits=bits)
        add("mid/side whose L leaves the bits" + w, RANGE, build(2, bits, 256, 4, 9, both((hi, bits), ((1 << bits) - 2, bits + 1)), assign=10), channels=2, bits=bits)
        add("left/side at the rails" + w, OK, build(2, bits, 256, 4, 9, both((hi, bits), (hi - lo, bits + 1)), assign=8), channels=2, bits=bits)
        add("a constant frame" + w, OK, build(1, bits, 256, 4, 9, const(lo, bits)), bits=bits)
        fr = build(1, bits, 256, 4, 9, good())
        add("no sync code" + w, SYNC, bytes([0xff, 0xf9]) + fr[2:], bits=bits)
        add("sample rate code 1001" + w, HEADER, _recrc(fr[:2] + bytes([fr[2] | 9]) + fr[3:], 8), bits=bits)
        add("reserved header bit" + w, HEADER, _recrc(fr[:3] + bytes([fr[3] | 1]) + fr[4:], 8), bits=bits)
        add("frame number's lead byte 10xxxxxx" + w, NUMBER, _recrc(fr[:4] + bytes([0x89]) + fr[5:], 8), bits=bits)
        long9 = bytes([0xff, 0xf8, 0x70, (6 if bits == 24 else 4) << 1, 0xc0, 0x89, 0, 3])
        long9 += bytes([m16.crc8(long9)])
        body = np.packbits(np.array(good().b + [0] * ((-len(good())) % 8), np.uint8)).tobytes()
        add("frame number 9 in two bytes" + w, NUMBER, long9 + body + m16.crc16(long9 + body).to_bytes(2, "big"), bits=bits)
    return out


def _recrc(fr, head):
    """fr with the CRC-8 behind its first `head` - 1 bytes and the CRC-16 at its end made right again"""
    fr = fr[:head - 1] + bytes([m16.crc8(fr[:head - 1])]) + fr[head:-2]
    return fr + m16.crc16(fr).to_bytes(2, "big")


@functools.lru_cache(None)
def subframe_types(frame, channels, B, bits, number):
    """the kinds of a valid frame's subframes by the width's LPC model, e.g. ("fixed2/p4", "lpc7/p0")"""
    model = m16l if bits == 16 else m24l
    return tuple(model.decode_frame(frame, 0, channels, B, number)[2])
