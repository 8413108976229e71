"""An independent model of the 16-bit quantiser (include/saugns_amd.h, section "Dither and noise shaping"), written from the
header's text with Python integers and floats and numpy -- not from sau_dither.h. Python floats are IEEE doubles and nothing
here can contract a product into a sum, so every step rounds where the text says it does."""
import math

import numpy as np

M64 = (1 << 64) - 1
PRESETS = {
    "FLAT": (0, []),
    "HP1": (1, [1.0]),
    "E3": (2, [1.623, -0.982, 0.109]),
    "E5": (3, [2.033, -2.165, 1.959, -1.590, 0.6149]),
    "F9": (4, [2.412, -3.370, 3.937, -4.174, 3.353, -2.205, 1.281, -0.569, 0.0847]),
}


def row_seed(seed, r):
    return (seed + 0xD1B54A32D192ED03 * r) & M64


def hash_z(seed_r, i, c):
    """splitmix64's output at the counter 2 i + c + 1, in Python integers"""
    z = (seed_r + 0x9E3779B97F4A7C15 * (2 * i + c + 1)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def tpdf_int(seed_r, i, c):
    z = hash_z(seed_r, i, c)
    return (z >> 40) - ((z >> 16) & 0xFFFFFF)


def tpdf_array(seed_r, first, n, c):
    """d for frames first .. first + n of one channel, as float64 (every value is exact in float32 too)"""
    with np.errstate(over="ignore"):
        k = (np.uint64(2) * (np.uint64(first & M64) + np.arange(n, dtype=np.uint64)) + np.uint64(c + 1))
        z = np.uint64(seed_r) + np.uint64(0x9E3779B97F4A7C15) * k
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    a = (z >> np.uint64(40)).astype(np.int64)
    b = ((z >> np.uint64(16)) & np.uint64(0xFFFFFF)).astype(np.int64)
    return (a - b).astype(np.float64) * 2.0 ** -24


def spec_valid(dither, coef):
    if dither not in (0, 1) or len(coef) > 9:
        return False
    if any(not math.isfinite(c) for c in coef):
        return False
    return sum(abs(c) for c in coef) <= 64


def scaled(x, gain):
    """y = x * gain in float32, a NaN -> -1, clamped to [-1, 1]"""
    with np.errstate(all="ignore"):
        y = np.asarray(x, np.float32) * np.float32(gain)
    y = np.where(np.isnan(y), np.float32(-1), y)
    return np.clip(y, np.float32(-1), np.float32(1)).astype(np.float32)


def quantize(x, channels, gain, dither, coef, seed, row=0, first=0, history=None):
    """-> (int16 samples, the history [channels][9] behind them -- history[c][0] the last error --, [clipped per channel])"""
    assert spec_valid(dither, coef) and channels in (1, 2)
    x = np.asarray(x, np.float32).reshape(-1, channels)
    n, T = x.shape[0], len(coef)
    out = np.zeros((n, channels), np.int16)
    hist = [[0.0] * 9 for _ in range(channels)] if history is None else [list(map(float, h)) for h in history]
    clipped = [0, 0]
    if not dither and not T:  # the existing rounding: float32 product, then to the nearest, ties to even
        y = scaled(x, gain)
        return np.rint(y * np.float32(32767)).astype(np.int16).reshape(-1), hist, clipped
    sr = row_seed(seed, row)
    for c in range(channels):
        s = scaled(x[:, c], gain).astype(np.float64) * 32767.0
        d = tpdf_array(sr, first, n, c) if dither else np.zeros(n)
        if not T:
            q = np.rint(s + d)
            clipped[c] = int(np.count_nonzero(np.abs(q) > 32767))
            out[:, c] = np.clip(q, -32767, 32767).astype(np.int16)
            continue
        e = hist[c]
        sl, dl = s.tolist(), d.tolist()
        col = [0] * n
        for i in range(n):
            t = 0.0
            for j in range(T - 1, 0, -1):
                t = t + coef[j] * e[j]
            w = (sl[i] - t) - coef[0] * e[0]
            q = float(round(w + dl[i]))  # round(): to the nearest, ties to even
            e = [q - w] + e[:8]
            if q > 32767.0 or q < -32767.0:
                clipped[c] += 1
                q = 32767.0 if q > 0 else -32767.0
            col[i] = int(q)
        out[:, c] = np.array(col, np.int16)
        hist[c] = e
    return out.reshape(-1), hist, clipped


def preset(name, seed):
    return dict(dither=1, coef=list(PRESETS[name][1]), seed=seed)
