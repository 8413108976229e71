"""The spectrum meter's arithmetic (include/saugns_amd.h, section "Spectrum") restated in numpy, operation for operation: every
numpy operation below is one IEEE operation per element, rounded on its own -- a product, then the sum or difference -- and a
stage of the radix-2 transform is one gather, the butterflies and one scatter. Window and twiddles are arguments: the tables
the library returns (sauAmd_spectrum_window, sauAmd_spectrum_twiddles), so no comparison depends on two libm's agreeing.
tests/test_spectrum_host.py holds this restatement against numpy.fft and against the library's host code;
tests/test_gpu_spectrum.py compares the device with it bit for bit."""
import numpy as np

GROUP = 16  # segments per group (saugns_amd/csrc/engine.h: SPEC_GROUP)
L_MIN, L_MAX = 8, 12


def clean(x):
    """a NaN or +-inf counts as +0.0f (a -0.0f stays what it is)"""
    x = np.asarray(x, np.float32)
    return np.where(np.isfinite(x), x, np.float32(0.0)).astype(np.float32)


def segments(P, N, hop):
    """S(P): the complete segments of P frames"""
    return 0 if P < N else (P - N) // hop + 1


def bit_reversal(L):
    j = np.arange(1 << L)
    r = np.zeros_like(j)
    for b in range(L):
        r |= ((j >> b) & 1) << (L - 1 - b)
    return r


def segment_power(x, w, tw, L):
    """x: float32 [..., N], cleaned -> p: float64 [..., N/2 + 1], one segment per leading index"""
    N = 1 << L
    assert x.shape[-1] == N and w.shape == (N,) and tw.shape == (N // 2, 2)
    prod = w * x.astype(np.float64)
    re = np.empty_like(prod)
    re[..., bit_reversal(L)] = prod  # re[rev(j)] = w[j] * x[j]
    im = np.zeros_like(re)
    for t in range(1, L + 1):
        m = 1 << t
        h, st = m // 2, N // m
        k0, j = np.meshgrid(np.arange(0, N, m), np.arange(h), indexing="ij")
        a = (k0 + j).ravel()
        b = a + h
        c, d = tw[(j * st).ravel(), 0], tw[(j * st).ravel(), 1]
        rb, ib = re[..., b], im[..., b]
        tr = c * rb - d * ib
        ti = c * ib + d * rb
        ur, ui = re[..., a], im[..., a]
        re[..., a] = ur + tr
        im[..., a] = ui + ti
        re[..., b] = ur - tr
        im[..., b] = ui - ti
    re, im = re[..., :N // 2 + 1], im[..., :N // 2 + 1]
    return re * re + im * im


class Meter:
    """one record: a row of `channels` interleaved channels that is fed frames"""

    def __init__(self, w, tw, L, hop, channels):
        self.w, self.tw, self.L, self.N, self.hop, self.ch = w, tw, L, 1 << L, hop, channels
        assert L_MIN <= L <= L_MAX and self.N // 8 <= hop <= self.N and channels in (1, 2)
        self.reset()

    def reset(self):
        bins = self.N // 2 + 1
        self.P, self.S, self.cnt = 0, 0, 0
        self.buf = np.zeros((0, self.ch), np.float32)  # the frames from S * hop on: pending
        self.acc = np.zeros((self.ch, bins))
        self.total = np.zeros((self.ch, bins))
        self.gram = []  # every segment's p, float64 [ch, bins]

    def feed(self, x):
        x = clean(x).reshape(-1, self.ch)
        self.buf = np.concatenate([self.buf, x])
        self.P += len(x)
        n = segments(self.P, self.N, self.hop) - self.S
        if n <= 0:
            return
        at = np.arange(n)[:, None] * self.hop + np.arange(self.N)[None, :]
        p = segment_power(np.moveaxis(self.buf[at], 2, 1), self.w, self.tw, self.L)  # [n, ch, bins]
        for i in range(n):
            self.acc = self.acc + p[i]  # (from +0.0: the first sum is exact)
            self.cnt += 1
            self.gram.append(p[i])
            if self.cnt == GROUP:  # a complete group goes into the total
                self.total = self.total + self.acc
                self.acc = np.zeros_like(self.acc)
                self.cnt = 0
        self.S += n
        self.buf = self.buf[n * self.hop:]
        assert len(self.buf) < self.N

    def read(self):
        """-> (sums [ch, bins], S): the group at hand is added into the copy"""
        return (self.total + self.acc if self.cnt else self.total.copy()), self.S

    def spectrogram(self):
        """float32 [ch, S, bins]"""
        bins = self.N // 2 + 1
        if not self.gram:
            return np.zeros((self.ch, 0, bins), np.float32)
        with np.errstate(over="ignore"):
            return np.moveaxis(np.stack(self.gram), 0, 1).astype(np.float32)


def measure(x, w, tw, L, hop, channels):
    """the whole of x ([frames * channels] or [frames, channels]) in one feed -> (sums, S, spectrogram)"""
    m = Meter(w, tw, L, hop, channels)
    m.feed(x)
    p, S = m.read()
    return p, S, m.spectrogram()
