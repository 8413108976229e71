"""The arithmetic contract of include/saugns_amd.h's loudness section, restated in Python: K-weighting coefficients, the chunked
recurrence, hop energies, the 4x true-peak interpolator and the BS.1770 gating -- every operation an IEEE f64 one in the
header's order (numpy's elementwise products and sums are separate, rounded operations: nothing is fused), so the device's
results can be compared bit for bit. Shared by tests/test_loudness_host.py and tests/test_gpu_loudness.py."""
import math

import numpy as np

LOUD_CHUNK = 256  # launch_plan.h
TP_TILE = 256     # launch_plan.h: TP_THREADS * TP_PER_LANE


def filter_formula(fs):
    """the ten coefficients by the header's formulas, in Python floats"""
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / fs)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    s1 = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0,
          2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / fs)
    a0 = 1.0 + K / Q + K * K
    return s1 + [1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]


def _i0(x):
    q, s, t = x * x * 0.25, 1.0, 1.0
    for k in range(1, 1000):
        t *= q / (k * k)
        if s + t == s:
            break
        s += t
    return s


def taps_formula():
    """g[n], n = 0 .. 128: K = 4, C = 64, beta = 5.0, not normalised"""
    K, Cn, beta = 4, 64, 5.0
    g = [0.0] * (2 * Cn + 1)
    for n in range(Cn + 1):
        d = float(n - Cn)
        t, r = d / K, d / Cn
        sinc = 1.0 if n == Cn else math.sin(math.pi * t) / (math.pi * t)
        g[n] = sinc * _i0(beta * math.sqrt(max(1.0 - r * r, 0.0))) / _i0(beta)
    for n in range(Cn):
        g[2 * Cn - n] = g[n]
    return np.array(g)


def step(st, f, x):
    """one frame on st = [s1, s2, t1, t2] (Python floats) -> y"""
    u = f[0] * x + st[0]
    st[0] = (f[1] * x - f[3] * u) + st[1]
    st[1] = f[2] * x - f[4] * u
    y = f[5] * u + st[2]
    st[2] = (f[6] * u - f[8] * y) + st[3]
    st[3] = f[7] * u - f[9] * y
    return y


def chunk_map(f):
    """M[r][k]: the state after 256 frames of zero input from the k-th unit state"""
    M = [[0.0] * 4 for _ in range(4)]
    for k in range(4):
        st = [0.0] * 4
        st[k] = 1.0
        for _ in range(LOUD_CHUNK):
            step(st, f, 0.0)
        for r in range(4):
            M[r][k] = st[r]
    return M


def clean(x):
    """float32 samples as f64, a NaN or +-inf as +0.0"""
    x = np.asarray(x, np.float32)
    return np.where(np.isfinite(x), x, np.float32(0.0)).astype(np.float64)


def _chunks_pass(f, X, valid, S, fb=None):
    """all chunks at once, frame by frame: X, valid [nch, 256]; S [nch, 4] start states -> end states (and, with fb [nch],
    the sums of y * y over the frames below and from fb)"""
    s1, s2, t1, t2 = (S[:, k].copy() for k in range(4))
    a0 = np.zeros(len(X))
    a1 = np.zeros(len(X))
    for j in range(X.shape[1]):
        x, v = X[:, j], valid[:, j]
        u = f[0] * x + s1
        n1 = (f[1] * x - f[3] * u) + s2
        n2 = f[2] * x - f[4] * u
        y = f[5] * u + t1
        m1 = (f[6] * u - f[8] * y) + t2
        m2 = f[7] * u - f[9] * y
        s1, s2, t1, t2 = np.where(v, n1, s1), np.where(v, n2, s2), np.where(v, m1, t1), np.where(v, m2, t2)
        if fb is not None:
            yy = y * y
            a0 = np.where(v & (j < fb), a0 + yy, a0)
            a1 = np.where(v & (j >= fb), a1 + yy, a1)
    return np.stack([s1, s2, t1, t2], axis=1), a0, a1


class Meter:
    """one stream's record under the contract: run(x) for every metered run in order, then hops() / true_peak()"""

    def __init__(self, f, taps, hop, channels):
        self.f = [float(v) for v in f]
        self.g = np.asarray(taps, np.float64)
        self.M = chunk_map(self.f)
        self.hop, self.ch = int(hop), int(channels)
        self.reset()

    def reset(self):
        self.pos = 0
        self.state = np.zeros((self.ch, 4))
        self.E = []  # [hop] -> [ch] running sums
        self.hist = np.zeros((31, self.ch))
        self.peak = [np.float32(0.0)] * self.ch

    def _e(self, h):
        while len(self.E) <= h:
            self.E.append([0.0] * self.ch)
        return self.E[h]

    def run(self, x):
        """x: float32 [frames, ch] (or [frames] on mono): the stream's frames of one run"""
        x = np.asarray(x, np.float32).reshape(-1, self.ch)
        n = len(x)
        if n == 0:
            return
        xc = clean(x)
        nch = (n + LOUD_CHUNK - 1) // LOUD_CHUNK
        idx = np.arange(nch * LOUD_CHUNK).reshape(nch, LOUD_CHUNK)
        valid = idx < n
        fb = np.array([min(self.hop - (self.pos + c * LOUD_CHUNK) % self.hop, LOUD_CHUNK) for c in range(nch)])
        for c in range(self.ch):
            X = np.zeros(nch * LOUD_CHUNK)
            X[:n] = xc[:, c]
            X = X.reshape(nch, LOUD_CHUNK)
            z, _, _ = _chunks_pass(self.f, X, valid, np.zeros((nch, 4)))
            S = np.zeros((nch, 4))
            S[0] = self.state[c]
            for k in range(nch - 1):  # behind every full chunk
                for r in range(4):
                    M = self.M[r]
                    S[k + 1, r] = ((((0.0 + M[0] * S[k, 0]) + M[1] * S[k, 1]) + M[2] * S[k, 2]) + M[3] * S[k, 3]) + z[k, r]
            end, a0, a1 = _chunks_pass(self.f, X, valid, S, fb)
            self.state[c] = end[nch - 1]
            for k in range(nch):
                cnt = min(LOUD_CHUNK, n - k * LOUD_CHUNK)
                h = (self.pos + k * LOUD_CHUNK) // self.hop
                self._e(h)[c] = self._e(h)[c] + float(a0[k])
                if cnt > fb[k]:
                    self._e(h + 1)[c] = self._e(h + 1)[c] + float(a1[k])
            # true peak of the run's frames
            xe = np.concatenate([self.hist[:, c], xc[:, c]])
            pk = self.peak[c]
            ax = np.abs(xc[:, c].astype(np.float32)).max()
            pk = max(pk, ax)
            for p in (1, 2, 3):
                acc = np.zeros(n)
                for q in range(32):
                    acc = acc + self.g[4 * q + p] * xe[31 - q:31 - q + n]
                pk = self._fold(pk, acc)
            self.peak[c] = pk
        self.hist = np.concatenate([self.hist, xc])[-31:]
        self.pos += n

    @staticmethod
    def _fold(pk, acc):
        with np.errstate(over="ignore"):
            w = np.abs(acc.astype(np.float32))
        w = w[np.isfinite(w)]
        return max(pk, w.max()) if len(w) else pk

    def hops(self):
        """the complete hops, float64 [n, 2] ([.., 1] is 0 on mono)"""
        n = self.pos // self.hop
        out = np.zeros((n, 2))
        for h in range(n):
            out[h, :self.ch] = self._e(h)
        return out

    def true_peak(self):
        """[2] float32: the record's peaks with the positions behind the last frame covered (on a copy)"""
        out = [np.float32(0.0), np.float32(0.0)]
        for c in range(self.ch):
            pk = self.peak[c]
            if self.pos:
                xe = np.concatenate([self.hist[:, c], np.zeros(31)])
                for p in (1, 2, 3):
                    acc = np.zeros(31)
                    for q in range(32):
                        acc = acc + self.g[4 * q + p] * xe[31 - q:62 - q]
                    pk = self._fold(pk, acc)
            out[c] = np.float32(pk)
        return out


def sequential_hops(f, x, hop):
    """plain frame-by-frame evaluation of one channel (no chunks): the complete hops' energies"""
    f = [float(v) for v in f]
    st = [0.0] * 4
    xs = clean(x).tolist()
    out = []
    for h in range(len(xs) // hop):
        acc = 0.0
        for v in xs[h * hop:(h + 1) * hop]:
            y = step(st, f, v)
            acc = acc + y * y
        out.append(acc)
    return np.array(out)


def lufs(z):
    return -0.691 + 10.0 * math.log10(z) if z > 0.0 else -math.inf


def gate(hops, hop, channels):
    """-> dict(blocks, gated_blocks, integrated, momentary_max) of complete hops [n][2]"""
    hops = np.asarray(hops, np.float64).reshape(-1, 2)
    nb = max(len(hops) - 3, 0)
    zs = []
    for j in range(nb):
        z = 0.0
        for c in range(channels):
            z = z + (((float(hops[j, c]) + float(hops[j + 1, c])) + float(hops[j + 2, c])) + float(hops[j + 3, c])) / (4.0 * hop)
        zs.append(z)
    ls = [lufs(z) for z in zs]
    out = {"blocks": nb, "gated_blocks": 0, "integrated": -math.inf, "momentary_max": max(ls) if ls else -math.inf}
    ab = [z for z, l in zip(zs, ls) if l > -70.0]
    if ab:
        s = 0.0
        for z in ab:
            s += z
        rel = lufs(s / len(ab)) - 10.0
        both = [z for z, l in zip(zs, ls) if l > -70.0 and l > rel]
        if both:
            s = 0.0
            for z in both:
                s += z
            out["gated_blocks"] = len(both)
            out["integrated"] = lufs(s / len(both))
    return out
