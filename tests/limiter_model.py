"""The arithmetic contract of include/saugns_amd.h's section "Limiter", restated in numpy: interpolated points, linked envelope,
required gain, hold, smoothing window, gain and output -- every operation an IEEE one in the header's order (numpy's elementwise
products and sums are separate, rounded operations: nothing is fused; the sums run over a Python loop of taps, one accumulator
per output value), so the device's results can be compared bit for bit. Shared by tests/test_limiter_host.py and
tests/test_gpu_limiter.py."""
import math

import numpy as np

import loudness_model as lm

LIM_A_MIN, LIM_A_MAX = 16, 1024        # engine.h
LIM_THREADS, LIM_PER_LANE = 256, 2     # launch_plan.h
LIM_TILE = LIM_THREADS * LIM_PER_LANE  # launch_plan.h
LIM_ENV_TILE = LIM_THREADS             # launch_plan.h


def lookahead(fs):
    """A = min(max(fs / 200, 16), 1024) frames"""
    return min(max(int(fs) // 200, LIM_A_MIN), LIM_A_MAX)


def latency(fs):
    """D = 2 A + 16 frames"""
    return 2 * lookahead(fs) + 16


def window_formula(fs):
    """h[j] = u[j] / S, u[j] = 1 + cos(pi (j - A) / (A + 1)), S the ascending sum, in Python floats"""
    A = lookahead(fs)
    u = [1.0 + math.cos(math.pi * (j - A) / (A + 1)) for j in range(2 * A + 1)]
    S = 0.0
    for v in u:
        S += v
    return np.array([v / S for v in u])


def pcm16(y):
    """the kernels' pcm16(y), all of it in float32"""
    y = np.asarray(y, np.float32)
    y = np.where(np.isnan(y), np.float32(-1.0), y)
    y = np.clip(y, np.float32(-1.0), np.float32(1.0)).astype(np.float32)
    return np.rint(y * np.float32(32767.0)).astype(np.int16)


def _abs_bits(v32):
    return np.asarray(v32, np.float32).view(np.uint32) & np.uint32(0x7fffffff)


def limit(x, fs, g0, c, taps, window):
    """x: float32 [frames, ch] (or [frames]: mono), zero before its first and behind its last frame; taps: sauAmd_truepeak_taps;
    window: sauAmd_limiter_window(fs) -> (y float32 [frames, ch], G float64 [frames]), time-aligned: y[i] belongs to x[i]"""
    x = np.asarray(x, np.float32)
    x = x.reshape(len(x), -1)
    n, ch = x.shape
    A = lookahead(fs)
    g = np.asarray(taps, np.float64)
    h = np.asarray(window, np.float64)
    assert len(h) == 2 * A + 1 and len(g) == 129
    g0, c = float(np.float32(g0)), float(np.float32(c))
    xc = lm.clean(x)
    # frame k of the sequence lies at xp[k + off]
    off = 2 * A + 32
    xp = np.zeros((n + 4 * A + 64, ch))
    xp[off:off + n] = xc
    lo, K = -2 * A, n + 4 * A  # s and r are needed for k = lo .. lo + K - 1
    # 1. the points w[m][p][ch] for m = lo + 15 .. lo + 15 + K, folded to the largest finite |w| of each m, as bits
    m0, M = lo + 15, K + 1
    wm = np.zeros(M, np.uint32)
    for cc in range(ch):
        for p in (1, 2, 3):
            acc = np.zeros(M)
            for q in range(32):
                a = m0 - q + off
                acc = acc + g[4 * q + p] * xp[a:a + M, cc]
            with np.errstate(over="ignore"):
                b = _abs_bits(acc.astype(np.float32))
            wm = np.maximum(wm, np.where(b < np.uint32(0x7f800000), b, np.uint32(0)))
    # 2. the envelope, channels linked
    e = np.maximum(wm[:K], wm[1:K + 1])
    for cc in range(ch):
        e = np.maximum(e, _abs_bits(xp[lo + off:lo + off + K, cc].astype(np.float32)))
    # 3. the required gain
    E = e.view(np.float32).astype(np.float64) * g0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(E <= c, 1.0, c / E)
    s = 1.0 - r
    # 4. the hold: d[k] for k = -A .. n + A - 1 at dd[k + A]
    dd = s[0:n + 2 * A].copy()
    for j in range(1, 2 * A + 1):
        dd = np.maximum(dd, s[j:j + n + 2 * A])
    # 6. the gain
    acc = np.zeros(n)
    for j in range(2 * A + 1):
        acc = acc + h[j] * dd[j:j + n]
    G = np.minimum(1.0 - acc, r[2 * A:2 * A + n])
    # 7. the output
    y = ((xc * g0) * G[:, None]).astype(np.float32)
    return y, G


def stats(G):
    """-> (frames, limited, min_gain) of the delivered frames' gains"""
    G = np.asarray(G, np.float64)
    return len(G), int((G < 1.0).sum()), float(G.min()) if len(G) else 1.0


def limit_delayed(x, total, fs, g0, c, taps, window):
    """what a sequence of limited runs delivers over `total` frames for a stream whose float samples are x: the limiter's
    output delayed by D, the input zero-extended -> (row float32 [total, ch], G [total])"""
    x = np.asarray(x, np.float32)
    x = x.reshape(len(x), -1)
    D = latency(fs)
    xd = np.zeros((total + D, x.shape[1]), np.float32)  # position n looks ahead to x[n]: the first `total` frames of x count
    m = min(len(x), total)
    xd[D:D + m] = x[:m]
    y, G = limit(xd, fs, g0, c, taps, window)
    return y[:total], G[:total]
