"""Steps 3 to 5 of the FLAC encoder's LPC mode (include/saugns_amd.h, section "FLAC", "The LPC mode"; sau_flac.h:
flac_lpc_f64_shift, flac_lpc_orders) as a known-answer probe, without a GPU: the serial run of binary64 operations in the middle
of "the bytes are a function of the fed sequence only".

The stream tests cannot see that arithmetic: the 12-bit quantisation swallows a last-bit difference in the recursion almost
always, so a build that fuses a product into a sum still gives the same bytes on everything they feed. The recursion's work
array a[] shows it at once. So the probe (tests/hooks: sauAmd_kat_flac_lpc_orders_host here, its _device twin in
tests/test_gpu_flac_lpc_steps.py) hands the shared function autocorrelations and compares g, the candidate mask, q and shift of
every candidate order and a[]'s BIT PATTERNS with tests/flac_lpc_model.py's levinson(). The vectors are proved fit for it by the
model alone: they reach every branch of the steps, and levinson(fused=True) -- every z + x * y as one rounded operation --
differs from levinson() in a[]'s bits on nearly all of them.

The module also holds what tests/test_gpu_flac_lpc_steps.py feeds the product kernels (stream_cases, degenerate_cases), each
with a census by the model of what it reaches."""
import ctypes as C
import os
import re

import numpy as np

import flac_lpc_model as mdl
from conftest import ROOT

A_FILL, Q_FILL, SHIFT_FILL, WORD_FILL = 0x5a5a5a5a5a5a5a5a, 0x5a5b, 0xa5, 0xdeadbeef


# ---- the probe's vectors ---------------------------------------------------------------------------------------------------

def _step_up(k):
    """reflection coefficients k[0 .. 7] -> the autocorrelation r[0 .. 8] with r[0] = 1 whose Levinson-Durbin recursion returns them"""
    r, a, err = [1.0], [], 1.0
    for i, ki in enumerate(k):
        r.append(-ki * err - sum(a[j] * r[i - j] for j in range(i)))
        a = [a[j] + ki * a[i - 1 - j] for j in range(i)] + [ki]
        err *= 1.0 - ki * ki
    return r


def _degenerate():
    """autocorrelations at the edges of steps 3 to 5; each also scaled by a few powers of two"""
    out = []

    def scaled(R, shifts):
        for s in shifts:
            out.append([v << s for v in R])

    scaled([1] * 9, (0, 1, 20, 53, 61))                                    # all equal: k = -1, err = 0, a stop at i = 0
    scaled([3] * 9, (0, 30))
    scaled([(-1) ** l for l in range(9)], (0, 1, 20, 53, 61))              # alternating sign: k = +1
    scaled([7 * (-1) ** l for l in range(9)], (0, 30))
    scaled([1 << 40, (1 << 40) - 1] + [1 << (40 - l) for l in range(1, 8)], (0, 10, 20))  # a stop behind order 1
    scaled([5, 3, -5, 1, 0, 2, -4, 5, 5], (0, 10, 30, 57))                 # |R[2]| = R[0]: k beyond 1 at i = 1
    scaled([1] + [0] * 8, (0, 10, 52, 60))                                 # [x, 0, 0, ...] ([1, 0, ...] among them): k = -0.0 throughout
    scaled([(1 << 52) + 1] + [0] * 8, (0, 9))
    scaled([2, 0, 1, 0, 0, 0, 0, 0, 0], (0, 39, 59))                       # [x, 0, y, 0, ...]: order 1 skipped, order 2 a candidate
    scaled([1000, 0, -999, 0, 1, 0, -1, 0, 1], (0, 20, 50))
    for r0 in ((1 << 53) - 1, 1 << 53, (1 << 53) + 1, (1 << 62) - 1):      # g = 0, 1, 1, 9; odd negative R[l] under the shift
        out.append([r0] + [-((r0 >> l) | 1) for l in range(1, 9)])
        out.append([r0] + [-((r0 // (2 * l + 1)) | 1) for l in range(1, 9)])
    scaled([1 << 40, 1, -2, 3, -1, 0, 2, -3, 1], (0, 10, 21))              # near-white: coefficients near 2^-40, the shift clamped to 15
    scaled([1 << 30, 100, -70, 30, 0, -20, 10, 5, -1], (0, 25))
    for s in (30, 45, 53, 61):                                             # k = +-(1 - 2^-20) at i = 0: q at both ends
        r0 = 1 << s
        r1 = r0 - (r0 >> 20)
        out.append([r0, -r1] + [(-1) ** l * (r0 - l * (r0 >> 19)) for l in range(2, 9)])
        out.append([r0, r1] + [r0 - l * (r0 >> 19) for l in range(2, 9)])
    return out


_vectors = None


def vectors():
    """[(tag, R[0 .. 8], M)], the same on every call: "sig" -- autocorrelations (mdl.autocorrelation) of int16 sines in noise at
    B = 256 and 4096 --, "rc" -- eight drawn reflection coefficients stepped up to r[0 .. 8], scaled by 2^30 .. 2^61 and truncated --
    and "deg", the degenerate ones; M in 1 .. 8, mostly high: M = 1 has no multiply-add that reaches a[]"""
    global _vectors
    if _vectors is not None:
        return _vectors
    rng = np.random.default_rng(20240611)
    out = []

    def draw_m():
        return int(rng.choice(np.arange(1, 9), p=[.01, .03, .06, .1, .1, .1, .2, .4]))

    for i in range(600):
        B = (256, 4096)[i % 2]
        amp, freq, sigma = (float(np.exp(rng.uniform(np.log(lo), np.log(hi)))) for lo, hi in ((10, 30000), (20, 8000), (0.5, 300)))
        t = np.arange(B)
        s = amp * np.sin(2 * np.pi * freq * t / 44100 + rng.uniform(0, 2 * np.pi)) + sigma * rng.standard_normal(B)
        s = np.clip(np.round(s), -32768, 32767).astype(np.int64)
        R = mdl.autocorrelation(s, B, 8)
        assert R[0] > 0
        out.append(("sig", R, draw_m()))
    n = 0
    while n < 600:
        k = rng.uniform(-1, 1, 8) * (0.3, 0.9, 0.999, 0.999999)[int(rng.integers(4))]
        scale = 2.0 ** rng.uniform(30, 61)
        R = [int(v * scale) for v in _step_up([float(v) for v in k])]
        if all(abs(v) <= R[0] for v in R):
            out.append(("rc", R, draw_m()))
            n += 1
    for R in _degenerate():
        assert len(R) == 9 and 0 < R[0] < 1 << 62 and all(abs(v) <= R[0] for v in R), R
        for M in (1, 2, 3, 5, 8):
            out.append(("deg", R, M))
    _vectors = out
    return out


_model = None


def model_results():
    """levinson() of every vector, once"""
    global _model
    if _model is None:
        _model = [mdl.levinson(R, M) for _, R, M in vectors()]
    return _model


# ---- the probe ---------------------------------------------------------------------------------------------------------------

def run_probe(fn, vecs):
    """fn: sauAmd_kat_flac_lpc_orders_host or _device -> (g, mask, q [n][8][8], shift [n][8], a_bits [n][8]) with the outputs filled
    with a pattern beforehand"""
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32] + [C.c_void_p] * 5
    n = len(vecs)
    R = np.array([v[1] for v in vecs], np.int64).reshape(n, 9)
    M = np.array([v[2] for v in vecs], np.uint32)
    g = np.full(n, WORD_FILL, np.uint32)
    mask = np.full(n, WORD_FILL, np.uint32)
    q = np.full((n, 8, 8), Q_FILL, np.int16)
    shift = np.full((n, 8), SHIFT_FILL, np.uint8)
    a = np.full((n, 8), A_FILL, np.uint64)
    assert fn(R.ctypes.data, M.ctypes.data, n, g.ctypes.data, mask.ctypes.data, q.ctypes.data, shift.ctypes.data, a.ctypes.data) == 1
    return g, mask, q, shift, a


def check_probe(got, vecs, want, who):
    """g, the mask, a[0 .. M-1] bit for bit, q and shift of every candidate order; entries of orders outside the mask are not looked
    at, a[M ..] keeps the pattern"""
    g, mask, q, shift, a = got
    bad = []
    for v, ((tag, R, M), (wg, wmask, wout, wa, _, _)) in enumerate(zip(vecs, want)):
        what = None
        if int(g[v]) != wg:
            what = ("g", int(g[v]), wg)
        elif int(mask[v]) != wmask:
            what = ("mask", int(mask[v]), wmask)
        elif [int(x) for x in a[v, :M]] != wa:
            what = ("a", [hex(int(x)) for x in a[v, :M]], [hex(x) for x in wa])
        elif any(int(x) != A_FILL for x in a[v, M:]):
            what = ("a beyond M", [hex(int(x)) for x in a[v]])
        else:
            for m, (wq, wshift) in wout.items():
                if [int(x) for x in q[v, m - 1, :m]] != wq or int(shift[v, m - 1]) != wshift:
                    what = ("order", m, [int(x) for x in q[v, m - 1, :m]], int(shift[v, m - 1]), wq, wshift)
                    break
        if what:
            bad.append((v, tag, R, M) + what)
    assert not bad, (who, len(bad), "of", len(vecs), "vectors differ; the first:", bad[0])


def test_the_vectors_reach_every_branch_and_tell_fused_arithmetic_apart():
    """by the model alone: what the probe's vectors reach, and that a[]'s bits would show a fused multiply-add"""
    vecs, res = vectors(), model_results()
    assert 1400 <= len(vecs) <= 1700
    assert sum(t == "sig" for t, _, _ in vecs) >= 300 and sum(t == "rc" for t, _, _ in vecs) >= 300
    assert {M for _, _, M in vecs} == set(range(1, 9))
    gs = {r[0] for r in res}
    assert {0, 1, 9} <= gs, gs
    stop0 = sum(r[4] == 0 for r in res)
    stop_kept = sum(r[4] is not None and r[4] >= 1 and r[1] != 0 for r in res)
    hole = sum(any(any(m2 > m for m2 in r[2]) for m in r[5]["cmax_zero"]) for r in res)
    shift15 = sum(bool(r[5]["shift15"]) for r in res)
    qmax = sum(bool(r[5]["qmax"]) for r in res)
    qmin = sum(bool(r[5]["qmin"]) for r in res)
    none = sum(r[1] == 0 for r in res)
    print("vectors: %d; g: %s; stop at i = 0: %d; stop at i >= 1 with lower orders kept: %d; cmax zero below a candidate: %d; "
          "shift clamped to 15: %d; q clamped at +2047: %d; q at -2048: %d; no candidate at all: %d"
          % (len(vecs), sorted(gs), stop0, stop_kept, hole, shift15, qmax, qmin, none))
    assert stop0 and stop_kept and hole and shift15 and qmax and qmin and none
    for r in res:
        for m in r[5]["cmax_zero"]:
            assert not r[1] & (1 << (m - 1))
    assert any(r[1] & 2 and not r[1] & 1 for r in res)  # a mask with a hole
    for tag in ("sig", "rc"):
        idx = [i for i, v in enumerate(vecs) if v[0] == tag]
        differ = sum(mdl.levinson(vecs[i][1], vecs[i][2], fused=True)[3] != res[i][3] for i in idx)
        print("fused arithmetic changes a[]'s bits on %d of %d %s vectors" % (differ, len(idx), tag))
        assert differ >= 0.9 * len(idx), (tag, differ, len(idx))


def test_orders_is_levinson():
    for _, R, M in vectors()[::7]:
        g, mask, out, a, stop, seen = mdl.levinson(R, M)
        assert mdl.orders(R, M) == out and mask == sum(1 << (m - 1) for m in out) and len(a) == M
        assert (stop is None) == (seen["stop"] is None) and (stop is None or 0 <= stop < M)


def test_the_host_probe_equals_the_model(hooks):
    vecs = vectors()
    check_probe(run_probe(hooks.sauAmd_kat_flac_lpc_orders_host, vecs), vecs, model_results(), "host")


def test_the_probe_is_compiled_with_the_products_flags():
    """the probe holds the shared function as the product's build compiles it only if tests/hooks/Makefile's FLAGS carry every flag
    of saugns_amd/build.py's (-ffp-contract=off above all)"""
    make = open(os.path.join(ROOT, "tests", "hooks", "Makefile")).read()
    line = re.search(r"^FLAGS\s*:?=\s*(.*)$", make, re.M).group(1).split()
    build = open(os.path.join(ROOT, "saugns_amd", "build.py")).read()
    flags = re.findall(r'"([^"]+)"', re.search(r"^FLAGS\s*=\s*\[(.*?)\]", build, re.M | re.S).group(1))
    assert "-ffp-contract=off" in flags and "--offload-arch=gfx950" in flags and len(flags) >= 5, flags
    assert set(flags) <= set(line), (flags, line)
    for obj in ("test_hooks.o", "kat_kernels.o"):
        rule = re.search(r"^%s:((?:.*\\\n)*.*)\n\t(.*)$" % re.escape(obj), make, re.M)
        assert "sau_flac.h" in rule.group(1) and "$(FLAGS)" in rule.group(2), rule.group(0)


# ---- what the stream tests on the device feed, with the model's census of it ----------------------------------------------

def stream_cases():
    """[(B, channels, M, [(name, int16 row)] * 3)]: every block size, at B = 256 every M in 1 .. 8 (mono and stereo by turns), at
    the other sizes one mono and one stereo encoder with M = 8 and one of 3, 5, 6, 7; rows of 2 B + 37 frames: all-pole
    processes of orders spread over 1 .. M (stereo: the right channel another seed's), then pm and the extremes"""
    plan = [(256, 1 + (M + 1) % 2, M) for M in range(1, 9)]
    plan += [(512, 1, 8), (512, 2, 3), (1024, 1, 5), (1024, 2, 8), (2048, 1, 8), (2048, 2, 6), (4096, 1, 7), (4096, 2, 8)]
    out = []
    for case, (B, ch, M) in enumerate(plan):
        frames = 2 * B + 37
        ps = [M] + ([1 + (case + M // 2) % (M - 1)] if M >= 3 else [1] if M == 2 else [])
        rows = []
        for r, p in enumerate(ps):
            L = mdl.ar(p, frames, 10 * case + r)
            rows.append(("ar%d" % p, mdl.rows(L, mdl.ar(p, frames, 10 * case + r + 5) if ch == 2 else None)))
        fill = [("pm", mdl.pm(frames, ch, case)), ("extremes", mdl.crafted("extremes", frames, ch))]
        if case % 2:
            fill.reverse()
        rows += fill[:3 - len(rows)]
        out.append((B, ch, M, rows))
    return out


def degenerate_cases():
    """[(B, channels, [(name, int16 row)])] with max_lpc_order 8: blocks in which steps 3 to 5 find nothing or not everything --
    impulse (no candidate order: the kernel's m == 0 path), pair (order 1 skipped below a candidate order 2), the edge blocks that
    exist at this B (R[0] == 0 in a block that is not constant; R[0] = 1), and a block without a candidate followed by one that
    chooses order 8. Stereo: the right channel is the left one negated (M constant, S twice L), another seed's process in the last row"""
    out = []
    for B in (256, 1024, 4096):
        frames = 2 * B + 37
        for ch in (1, 2):
            mats = [("impulse", mdl.impulse(frames, B)), ("pair", mdl.pair(frames, B))]
            if B == 1024:
                mats.append(("edge+1", mdl.edge(frames, B, 1)))
            if B == 4096:
                mats += [("edge+7", mdl.edge(frames, B, 7)), ("edge-1", mdl.edge(frames, B, -1))]
            rows = [(name, mdl.rows(s, -s if ch == 2 else None)) for name, s in mats]
            L = np.concatenate([mdl.impulse(B, B), mdl.ar(8, B + 37, B)])
            R = np.concatenate([-mdl.impulse(B, B), mdl.ar(8, B + 37, B + 1)])
            rows.append(("impulse,ar8", mdl.rows(L, R if ch == 2 else None)))
            out.append((B, ch, rows))
    return out


def feed_case():
    """(B, channels, M, [(name, int16 row)]) of the feeds-in-pieces section: rows of 5 B + 37, 0, 4 B and 3 B + 1 frames"""
    B = 512
    n = [5 * B + 37, 0, 4 * B, 3 * B + 1]
    return B, 2, 5, [("ar5", mdl.rows(mdl.ar(5, n[0], 1), mdl.ar(5, n[0], 2))), ("empty", np.zeros(0, np.int16)),
                     ("pair", mdl.rows(mdl.pair(n[2], B), -mdl.pair(n[2], B))), ("ar2", mdl.rows(mdl.ar(2, n[3], 3), mdl.ar(2, n[3], 4)))]


def lpc_orders_chosen(x, ch, B, M):
    """the orders of the LPC subframes the model's encoder chooses for the whole blocks of a row"""
    seen = set()
    for k in range(len(x) // ch // B):
        _, (_, an) = mdl.encode_block(x[k * B * ch:(k + 1) * B * ch], ch, B, k, M, with_choice=True)
        seen.update(a["order"] for a in an if a["type"] == "lpc")
    return seen


def test_census_of_the_all_pole_material():
    """at every B, with M = 8, the model chooses LPC of exactly order p for ar(p): three seeds, two blocks each"""
    for B in mdl.BLOCKS:
        for p in range(1, 9):
            for seed in range(3):
                s = mdl.ar(p, 2 * B, seed)
                for b in range(2):
                    a = mdl.analyze_lpc(s[b * B:(b + 1) * B], 16, B, 8)
                    assert a["type"] == "lpc" and a["order"] == p, (B, p, seed, b, a["type"], a.get("order"))


def test_census_of_the_stream_cases():
    """what the device's stream test asserts of the decoded kinds holds for the model: at B = 256 every order 1 .. 8 is chosen, at
    every other B an order <= 3 and an order >= 5"""
    seen = {}
    for B, ch, M, rows in stream_cases():
        assert len(rows) == 3 and all(len(x) == (2 * B + 37) * ch for _, x in rows)
        for _, x in rows:
            seen.setdefault(B, set()).update(lpc_orders_chosen(x, ch, B, M))
    print("LPC orders the model chooses per B:", {B: sorted(s) for B, s in seen.items()})
    assert sorted(seen) == list(mdl.BLOCKS)
    assert seen[256] == set(range(1, 9)), seen[256]
    for B in mdl.BLOCKS[1:]:
        assert min(seen[B]) <= 3 and max(seen[B]) >= 5, (B, seen[B])
    assert {M for B, _, M, _ in stream_cases() if B == 256} == set(range(1, 9))
    assert all({ch for b, ch, _, _ in stream_cases() if b == B} == {1, 2} for B in mdl.BLOCKS)


def test_census_of_the_feed_case():
    B, ch, M, rows = feed_case()
    assert [len(x) // ch for _, x in rows] == [5 * B + 37, 0, 4 * B, 3 * B + 1]
    seen = {name: lpc_orders_chosen(x, ch, B, M) for name, x in rows}
    assert 5 in seen["ar5"] and 2 in seen["ar2"] and not seen["empty"], seen


def test_census_of_the_degenerate_blocks():
    """by the model: what each degenerate block is there for"""
    M = 8
    for B in (256, 1024, 4096):
        s = mdl.impulse(B, B)
        R = mdl.autocorrelation(s, B, M)
        assert R[0] > 0 and not any(R[1:]) and mdl.levinson(R, M)[1] == 0
        assert mdl.analyze_lpc(s, 16, B, M)["type"] != "lpc" and mdl.analyze(s, 16, B)["type"] != "constant"
        R = mdl.autocorrelation(mdl.pair(B, B), B, M)
        g, mask, out, _, _, seen = mdl.levinson(R, M)
        assert R[1] == 0 and R[2] != 0 and not mask & 1 and mask & 2 and 1 in seen["cmax_zero"], (B, R, mask)
    for B, v in ((4096, 7), (1024, 1)):
        s = mdl.edge(B, B, v)
        assert mdl.window(B)[0] * v >> 3 == 0 and mdl.autocorrelation(s, B, M)[0] == 0 and mdl.analyze(s, 16, B)["type"] != "constant"
    s = mdl.edge(4096, 4096, -1)
    assert int(mdl.window(4096)[0]) == 1 and (mdl.window(4096) * s >> 3)[0] == -1
    R = mdl.autocorrelation(s, 4096, M)
    g, mask, out, _, stop, seen = mdl.levinson(R, M)
    assert R == [1] + [0] * 8 and mask == 0 and stop is None and seen["cmax_zero"] == list(range(1, 9))
    for B, ch, rows in degenerate_cases():
        names = [n for n, _ in rows]
        assert names[:2] == ["impulse", "pair"] and names[-1] == "impulse,ar8" and len(rows) == {256: 3, 1024: 4, 4096: 5}[B]
        for name, x in rows:
            chosen = lpc_orders_chosen(x, ch, B, M)
            if name == "impulse" or name.startswith("edge"):
                assert not chosen, (B, ch, name, chosen)
            if name == "impulse,ar8":
                _, (_, an) = mdl.encode_block(x[:B * ch], ch, B, 0, M, with_choice=True)
                assert all(a["type"] != "lpc" for a in an)
                assert 8 in chosen, (B, ch, chosen)
