"""The decimating FIR (saugns_amd/csrc/k_decimate.h: decimate_kernel, decimate_carry_kernel) on rows the test writes itself,
through tests/hooks_decimate: a HIP backend of the hook's own, a batch over it, and Backend::begin_decimation / decimate /
fetch_decimated_async called beside the engine on host rows copied over the batch's float rows. tests/test_gpu_decimate.py
reaches the kernels through rendered programs only -- smooth, finite, round lengths; here every one of the twelve
decimate_kernel<K, OutT, CH> runs over noise, over-range noise, constant full scale, subnormals, NaN and infinities, with
NaN poison behind every stream's end, in runs around the history's length and the tile's multiples, with frame counts of
every residue mod 4.

The reference is tests/test_gpu_decimate.py's decimate_ref -- the header's f64 loop with the exported taps, rounded once
to float -- over the runs end to end, each zero-extended from frames_hi[s] to n_hi; int16 is test_gpu_levels.quantise of it.
The comparison is by BYTES, subnormal results included (the header's contract lists no exception). A float the reference
has as NaN need only be NaN on the device (x86 and the GPU differ in a generated NaN's sign and payload)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_program
from test_gpu_decimate import H, KEYS, decimate_ref
from test_gpu_levels import quantise

pytestmark = pytest.mark.gpu

# launch_plan.h and engine.h, mirrored: tests/test_decimate_host.py reads the headers
DECIM_TILE = 256           # output frames of one workgroup of decimate_kernel
DECIM_HALF = 32            # H: the history is 2 * H output frames' worth of input
DECIM_CARRY_THREADS = 256  # decimate_carry_kernel: four floats a thread -- K = 8 stereo's 1024 history floats fill it
RATE = 6000
N_STREAMS = 5
NOISE, LOUD, RAILS, TINY, NONFINITE = range(N_STREAMS)  # what stream s holds

# output frames per run: shorter than, as long as and longer than the history (2 * H = 64); a tile less one, a tile, a tile and
# one, two whole tiles (with buf_len on a tile's multiple the kernel's `m >= P.buf_len` never holds); then the tails
RUNS = [1, 3, 63, 64, 65, 255, 256, 257, 512, 2 * H + 6]
# frames_hi[s] of every run, by name (frames_hi): full n_hi, zero 0, one 1, m1 n_hi - 1, m3 n_hi - 3, r1 / r3 a count from the
# middle of the run with frames_hi * ch = 1 / 3 mod 4 in mono (stereo: an odd count, 2 mod 4). The runs of 1, 3 and 63 frames
# hold partial and zero counts: decimate_carry_kernel's old history, input and zero in one short run. The NONFINITE stream is
# full where its NaN and infinities are sown (the runs of 255, 256 and 512).
SCHEDULE = [
    # NOISE   LOUD    RAILS   TINY    NONFINITE
    ["full", "zero", "one",  "full", "one"],    # 1
    ["m1",   "r1",   "zero", "m3",   "full"],   # 3
    ["r3",   "m3",   "m1",   "zero", "r1"],     # 63
    ["zero", "full", "r3",   "r1",   "m1"],     # 64
    ["m3",   "one",  "full", "r3",   "zero"],   # 65
    ["full", "r3",   "full", "m1",   "full"],   # 255
    ["r1",   "full", "full", "full", "full"],   # 256
    ["one",  "m1",   "r1",   "m3",   "r3"],     # 257
    ["full", "m3",   "m3",   "full", "full"],   # 512
    ["m1",   "full", "zero", "r1",   "one"],    # 2H + 6
]
SOWN = {5: np.nan, 6: np.inf, 8: -np.inf}  # run -> what the middle of the NONFINITE stream's run holds


def frames_hi(name, n_hi):
    mid = (n_hi // 2) & ~3
    f = {"full": n_hi, "zero": 0, "one": 1, "m1": n_hi - 1, "m3": n_hi - 3, "r1": mid + 1, "r3": mid + 3}[name]
    return f if 0 <= f <= n_hi else 1  # (the one-frame run at K = 2 has no room for 3 frames)


def material(K, ch, n_out, seed):
    """per stream: n_out * K frames of ch channels, float32"""
    rng = np.random.default_rng(seed)
    n = n_out * K
    x = np.zeros((N_STREAMS, n, ch), np.float32)
    x[NOISE] = rng.normal(0.0, 0.3, (n, ch))
    x[LOUD] = rng.normal(0.0, 1.5, (n, ch))
    x[RAILS, :, 0] = 1.0
    x[RAILS, :, ch - 1] = 1.0 if ch == 1 else -1.0
    x[TINY] = (rng.normal(0.0, 1.0, (n, ch)) * 1e-39).astype(np.float32)
    x[NONFINITE] = rng.normal(0.0, 0.3, (n, ch))
    return x


def sequence(K, ch, runs=RUNS, schedule=SCHEDULE, sown=SOWN, seed=1):
    """-> [(n, frames[N_STREAMS], rows[N_STREAMS, n * K * ch] with NaN behind frames[s] * ch)], and per stream what the
    filter is to see: the runs end to end, +0 behind frames[s]"""
    x = material(K, ch, sum(runs), seed + 16 * K + ch)
    L = 2 * H * K + 1
    out, seen, pos = [], np.zeros_like(x), 0
    for r, n in enumerate(runs):
        n_hi = n * K
        if r in sown:  # mid-run: more than L frames from the run's ends, and from the other two
            assert n_hi > 2 * L + 8 and schedule[r][NONFINITE] == "full"
            x[NONFINITE, pos + n_hi // 2 + r, r % ch] = sown[r]
        fr = [frames_hi(schedule[r][s], n_hi) for s in range(N_STREAMS)]
        rows = x[:, pos:pos + n_hi].copy()
        for s in range(N_STREAMS):
            seen[s, pos:pos + fr[s]] = rows[s, :fr[s]]
            rows[s, fr[s]:] = np.nan  # poison: "whatever the row holds" behind the stream's end
        out.append((n, fr, rows.reshape(N_STREAMS, n_hi * ch)))
        pos += n_hi
    return out, seen


def check_schedule(K, ch, seq):
    """the sequence holds what it is there for"""
    res = {(f * ch) % 4 for n, fr, _ in seq for f in fr if f}
    assert res >= ({1, 3} if ch == 1 else {2}), (K, ch, res)  # the masks of x.y / x.z / x.w: all three, and x.w alone
    short = [(n, f) for n, fr, _ in seq for f in fr if n < 2 * DECIM_HALF]  # shift < hist_floats
    assert any(0 < f < n * K for n, f in short) and any(f == 0 for n, f in short) and any(f == n * K for n, f in short)
    assert 2 * DECIM_HALF * K * ch <= 4 * DECIM_CARRY_THREADS
    lens = [n for n, _, _ in seq]
    assert {DECIM_TILE - 1, DECIM_TILE, DECIM_TILE + 1, 2 * DECIM_TILE, 2 * DECIM_HALF - 1, 2 * DECIM_HALF, 2 * DECIM_HALF + 1} <= set(lens)
    assert lens[-1] == 2 * H + 6


def window_meets(mask, K, n_out):
    """mask [n_hi, ch] -> [n_out, ch]: output m's L-tap window x[m * K - (L - 1) .. m * K] holds a marked sample"""
    L = 2 * H * K + 1
    c = np.concatenate([np.zeros((1, mask.shape[1]), np.int64), np.cumsum(mask, axis=0)])
    hi = np.arange(n_out) * K + 1
    return (c[hi] - c[np.maximum(hi - L, 0)]) > 0


def reference(sa, K, ch, seq, seen):
    """-> [N_STREAMS, n_out * ch] float32, with the material asserted present: a case cannot pass by not containing it"""
    n_out = sum(n for n, _, _ in seq)
    with np.errstate(invalid="ignore"):  # (inf - inf in the NONFINITE stream is meant)
        want = np.stack([decimate_ref(sa, seen[s].reshape(-1), K, ch, n_out, allow_subnormal=True) for s in range(N_STREAMS)])
    y = want.reshape(N_STREAMS, n_out, ch)
    tiny = np.finfo(np.float32).tiny
    for s in (NOISE, LOUD, RAILS, TINY):
        assert np.isfinite(seen[s]).all() and np.isfinite(y[s]).all()
    assert np.abs(y[NOISE]).max() > 0.1
    q = quantise(want[LOUD])
    assert y[LOUD].max() > 1.0 and y[LOUD].min() < -1.0 and (q == 32767).any() and (q == -32767).any()
    for c in range(ch):  # constant full scale: the f64 sum lands within an ulp of the rail
        assert abs(seen[RAILS][:, c]).max() == 1.0 and np.abs(np.abs(y[RAILS][:, c]) - 1.0).min() <= 2.0 ** -23
    assert ch == 1 or (seen[RAILS][:, 1].min() == -1.0 and seen[RAILS][:, 0].max() == 1.0)
    assert (np.abs(seen[TINY]) < tiny).all() and (seen[TINY] != 0).any()
    sub = (np.abs(y[TINY]) < tiny) & (y[TINY] != 0)
    assert sub.sum() > n_out * ch // 2, "the reference's float output holds non-zero subnormals"
    x = seen[NONFINITE]
    assert np.isnan(x).sum() == 1 and (x == np.inf).sum() == 1 and (x == -np.inf).sum() == 1
    nan_w = window_meets(np.isnan(x), K, n_out)
    pinf_w, ninf_w = window_meets(x == np.inf, K, n_out), window_meets(x == -np.inf, K, n_out)
    assert nan_w.any() and pinf_w.any() and ninf_w.any()
    # exactly the windows that meet the NaN, or both infinities (sown at least L apart: there is none), give NaN; a window
    # that meets one infinity gives an infinity
    assert (np.isnan(y[NONFINITE]) == (nan_w | (pinf_w & ninf_w))).all()
    assert np.isinf(y[NONFINITE][(pinf_w | ninf_w) & ~nan_w]).all()
    return want


def same_samples(got, want, what):
    """by bytes; where a float reference is NaN the device's need only be NaN"""
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if want.dtype == np.float32:
        nan = np.isnan(want)
        assert np.isnan(got[nan]).all(), f"{what}: {int((~np.isnan(got[nan])).sum())} of {int(nan.sum())} NaN samples are not NaN"
        g, w = got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]
    else:
        g, w = got.view(np.uint16), want.view(np.uint16)
    d = np.flatnonzero(g != w)
    assert len(d) == 0, f"{what}: {len(d)} samples differ, first at {d[0]}: got {got.reshape(-1)[d[0]:d[0] + 4].tolist()} want {want.reshape(-1)[d[0]:d[0] + 4].tolist()}"


@pytest.fixture(scope="module")
def decimate_hooks(sa, hooks):
    """tests/hooks_decimate/libsaugns_amd_decimate_hooks.so: the product's object files (the `hooks` fixture has built them)
    + the decimator over rows of the test's own"""
    d = os.path.join(ROOT, "tests", "hooks_decimate")
    subprocess.check_call(["make", "-s", "-C", d])
    L = C.CDLL(os.path.join(d, "libsaugns_amd_decimate_hooks.so"))
    L.sauAmd_last_error.restype = C.c_char_p
    L.sauAmd_decimate_rows_create.restype = C.c_void_p
    L.sauAmd_decimate_rows_create.argtypes = [C.POINTER(C.c_void_p), C.c_size_t, C.c_uint32]
    L.sauAmd_decimate_rows_destroy.argtypes = [C.c_void_p]
    L.sauAmd_decimate_rows_prime.restype = C.c_bool
    L.sauAmd_decimate_rows_prime.argtypes = [C.c_void_p, C.c_size_t, C.c_int]
    L.sauAmd_decimate_rows_begin.restype = C.c_bool
    L.sauAmd_decimate_rows_begin.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.sauAmd_decimate_rows_run.restype = C.c_bool
    L.sauAmd_decimate_rows_run.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int,
                                           C.c_void_p, C.c_size_t]
    return L


class Rows:
    """a batch of N_STREAMS streams whose float rows hold n_hi_max frames, stereo or mono; closed after the test"""

    def __init__(self, L, sa, srate, n_hi_max):
        self.L = L
        self._prgs = [load_program(sa, KEYS[0]) for _ in range(N_STREAMS)]  # (any program: its samples are overwritten)
        arr = (C.c_void_p * N_STREAMS)(*[p.ptr for p in self._prgs])
        self.h = L.sauAmd_decimate_rows_create(arr, N_STREAMS, srate)
        assert self.h, L.sauAmd_last_error().decode()
        assert L.sauAmd_decimate_rows_prime(self.h, n_hi_max, 1), L.sauAmd_last_error().decode()

    def begin(self, K, ch):
        assert self.L.sauAmd_decimate_rows_begin(self.h, K, ch - 1), self.L.sauAmd_last_error().decode()

    def run(self, rows, frames, n, K, ch, out):
        """out: "f4", "<i2" or ">i2" -> [N_STREAMS, n * ch] of float32 or (as the file would hold them) int16"""
        rows = np.ascontiguousarray(rows, np.float32)
        assert rows.shape == (N_STREAMS, n * K * ch)
        fr = np.asarray(frames, np.uint32)
        got = np.zeros((N_STREAMS, n * ch), np.float32 if out == "f4" else np.int16)
        ok = self.L.sauAmd_decimate_rows_run(self.h, rows.ctypes.data, rows.shape[1], fr.ctypes.data, n, K, ch - 1, out == "f4", out == ">i2",
                                             got.ctypes.data, got.strides[0])
        assert ok, self.L.sauAmd_last_error().decode()
        return got

    def close(self):
        if self.h:
            self.L.sauAmd_decimate_rows_destroy(self.h)
            self.h = None


def as_written(want, out):
    """the float reference as the device rows hold it, in the host's view of their bytes"""
    if out == "f4":
        return want
    q = quantise(want)  # (NaN -> -32767, as pcm16 has it)
    return q if out == "<i2" else q.byteswap()


# ---- every instantiation, over every material, run length and stream end ---------------------------------------------------

@pytest.mark.parametrize("out", ["f4", "<i2", ">i2"])
@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("K", [2, 4, 8])
def test_crafted_rows_decimate_to_the_reference_byte_for_byte(sa, decimate_hooks, K, ch, out):
    seq, seen = sequence(K, ch)
    check_schedule(K, ch, seq)
    want = as_written(reference(sa, K, ch, seq, seen), out)
    b = Rows(decimate_hooks, sa, RATE * K, max(RUNS) * K)
    try:
        b.begin(K, ch)
        got = np.concatenate([b.run(rows, fr, n, K, ch, out) for n, fr, rows in seq], axis=1)
    finally:
        b.close()
    print(f"ran decimate_kernel<{K}, {'float' if out == 'f4' else 'int16_t'}, {ch}>" + (" swap_bytes" if out == ">i2" else ""))
    for s, name in enumerate(["noise", "noise at 1.5", "full scale", "subnormal", "non-finite"]):
        if out == "f4" and s != NONFINITE:  # the poison behind a stream's end reached no sum
            assert np.isfinite(got[s]).all(), (name, K, ch, int((~np.isfinite(got[s])).sum()))
        same_samples(got[s], want[s], (name, K, ch, out))


# ---- a new sequence forgets -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K,ch,K2,ch2", [(2, 1, 8, 2), (8, 2, 4, 1), (4, 1, 2, 2)])
def test_begin_decimation_zeroes_the_history_whatever_the_last_sequence_was(sa, decimate_hooks, K, ch, K2, ch2):
    runs, sched = [65, 65], [["full"] * N_STREAMS] * 2
    first, _ = sequence(K, ch, runs[:1], sched, {}, seed=7)
    then, seen = sequence(K2, ch2, runs, sched, {}, seed=8)
    alone = [decimate_ref(sa, seen[s, :65 * K2].reshape(-1), K2, ch2, 65, allow_subnormal=True) for s in range(N_STREAMS)]
    again = [decimate_ref(sa, seen[s, 65 * K2:].reshape(-1), K2, ch2, 65, allow_subnormal=True) for s in range(N_STREAMS)]
    carried = [decimate_ref(sa, seen[s].reshape(-1), K2, ch2, 130, allow_subnormal=True)[65 * ch2:] for s in range(N_STREAMS)]
    b = Rows(decimate_hooks, sa, RATE * 8, 65 * 8)
    try:
        b.begin(K, ch)
        n, fr, rows = first[0]
        b.run(rows, fr, n, K, ch, "f4")
        b.begin(K2, ch2)  # another factor and layout
        n, fr, rows = then[0]
        got = b.run(rows, fr, n, K2, ch2, "f4")
        b.begin(K2, ch2)  # the same factor and layout: a new sequence all the same
        n, fr, rows = then[1]
        got2 = b.run(rows, fr, n, K2, ch2, "f4")
    finally:
        b.close()
    for s in range(N_STREAMS):
        same_samples(got[s], alone[s], ("after another factor and layout", s))
        same_samples(got2[s], again[s], ("after the same factor and layout", s))
        assert again[s].tobytes() != carried[s].tobytes()  # (a history kept would show)
