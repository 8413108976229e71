"""The oracle's float entry (oracle/sau_oracle.c: ora_run_f32, the mix accumulator stored as it stands) held from both sides before
tests/test_gpu_f32_oracle.py makes it the yardstick of the device's float rows:

  a. quantise(float oracle) == int16 oracle on the programs the GPU parity tests render (the float entry is the int16 one with its
     last step taken out, and a plain store never departs from the reference's `+=` into a cleared buffer);
  b. quantise(float oracle * 2^k) == the compiled reference's PCM of the same voices at ampmult * 2^k for k = -12 .. 8: amp_scale
     multiplies every voice sample before the ordered sum, so the scaling is exact while nothing under- or overflows -- which is
     asserted on the float samples, not assumed. At k = -12 no reference sample is clamped: the samples beyond +-1, which the
     int16 comparisons see as +-32767 only, are checked to 1/8 of an int16 step of their own scale;
  c. the edge programs of the GPU tests reach what they are for: subnormal sums, sums beyond +-1, infinities and NaN.

The program lists are functions here and tests/test_gpu_f32_oracle.py imports them."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_lanemajor_ops as tl
import test_gpu_range_guards as tg
import test_gpu_units as tu
from conftest import ORACLE_FORMS, load_program, ref_tables
from saugns_amd import voicebank as vb
from saugns_amd.api import POP_PMOD
from test_gpu_f32 import quantise

RATE = 44100
CORPUS_CALL, CORPUS_CALLS = 11289, 12
SCALES = (-12, -6, 0, 4, 8)


# ---- the programs ----------------------------------------------------------------------------------------------------------

def random_graph(seed, ampmult=1.0):
    """test_gpu_units.py::test_random_operator_graphs' program `seed` -> (program, stereo, its cut-up render's call size)"""
    rng = np.random.default_rng(1000 + seed)
    voices = [tu._random_voice(rng) for _ in range(int(rng.integers(1, 4)))]
    return vb.build_program(voices, ampmult=ampmult), bool(seed & 1), int(rng.integers(700, 3000))


def later_event_graph(seed, ampmult=1.0):
    """test_gpu_units.py::test_random_graphs_with_later_events' (and, from seed 100, ..._in_other_kernel_configurations')
    program `seed` -> (program, stereo, the small call size)"""
    rng = np.random.default_rng(5000 + seed)
    voices = [tu._random_voice(rng) for _ in range(int(rng.integers(1, 4)))]
    tu._random_starts(rng, voices)
    ups = tu._random_updates(rng, voices)
    return vb.build_program(voices, updates=ups, ampmult=ampmult), bool(seed & 1), int(rng.integers(700, 3000))


WHOLE = 4000000  # (the call size of the renders in one run)

# (amplitude a, ampmult) -> what the sums of edge_program are at 44100 Hz
EDGES = {"subnormal": (1e-38, 1.0), "subnormal scaled": (1e-30, 2.0 ** -40), "subnormal ampmult": (1.0, 2.0 ** -140),
         "over range": (3e38, 1.0), "infinite": (1e30, 1e30)}


def edge_program(a, ampmult):
    """a 50 ms sine under PM whose amplitude line falls from `a` to 0 at pan 0.3, beside a 40 ms saw of amplitude `a` whose pan
    sweeps from -0.9 to 0.9"""
    m = vb.Op("sin", freq=vb.Line(2.0, ratio=True), amp=vb._f32(0.5))
    one = vb.Op("sin", freq=220.0, amp=vb.Line(vb._f32(a), goal=0.0, shape="lin"), time_ms=50, pan=vb.Line(0.3),
                mods={POP_PMOD: [m]})
    two = vb.Op("saw", freq=330.0, amp=vb._f32(a), time_ms=40, pan=vb.Line(-0.9, goal=0.9, shape="lin"))
    return vb.build_program([one, two], ampmult=ampmult)


def classes(x):
    """-> counts of a float32 array's samples by kind"""
    x = np.asarray(x, np.float32).reshape(-1)
    b = x.view(np.uint32)
    return {"n": len(x), "subnormal": int((((b & 0x7f800000) == 0) & ((b & 0x007fffff) != 0)).sum()),
            "over": int((np.abs(x) > 1).sum()), "inf": int(np.isinf(x).sum()), "nan": int(np.isnan(x).sum())}


# ---- a. against the int16 oracle -------------------------------------------------------------------------------------------

@pytest.fixture(autouse=True)
def forms(oracle):
    oracle.oracle().ora_set_fastmath_forms(ORACLE_FORMS)


def _both(oracle, prg, rate, stereo, chunk, what, max_frames=0):
    """quantise(float oracle) == int16 oracle -> (float samples, int16 samples)"""
    x = oracle.oracle_render_f32(prg.ptr, rate, stereo, chunk=chunk, max_frames=max_frames)
    want = oracle.oracle_render(prg.ptr, rate, stereo, chunk=chunk, max_frames=max_frames)
    assert x.dtype == np.float32 and len(x) == len(want), (what, len(x), len(want))
    d = np.flatnonzero(quantise(x) != want)
    assert len(d) == 0, f"{what}: {len(d)} samples differ, first at {d[0]}: float {x[d[0]]!r} int16 {want[d[0]]}"
    return x, want


def test_float_oracle_quantises_to_the_int16_oracle_on_the_corpus(oracle, sa, index):
    keys = sorted(index["corpus"])
    assert len(keys) >= 90
    for key in keys:
        prg = load_program(sa, key)
        # (stereo and mono at the corpus rate, and mono at 8000 Hz as tests/test_gpu_f32_oracle.py renders it)
        for stereo, rate in ((True, index["corpus_rate"]), (False, index["corpus_rate"]), (False, 8000)):
            _both(oracle, prg, rate, stereo, CORPUS_CALL, (key, stereo, rate), max_frames=CORPUS_CALL * CORPUS_CALLS)


def test_float_oracle_quantises_to_the_int16_oracle_on_the_random_graphs(oracle):
    """... of which a quarter of the samples lie beyond +-1 (measured: 26 %); at least a tenth is asserted"""
    n = over = 0
    for seed in range(64):
        prg, stereo, chunk = random_graph(seed)
        for c in (4000, chunk):  # (check()'s call size and check_runs')
            x, _ = _both(oracle, prg, RATE, stereo, c, ("random", seed, c))
        n, over = n + len(x), over + int((np.abs(x) > 1).sum())
    assert over > n // 10, (over, n)
    for seed in range(48):
        prg, stereo, chunk = later_event_graph(seed)
        for c in (WHOLE, chunk):
            _both(oracle, prg, RATE, stereo, c, ("later events", seed, c))


def test_float_oracle_quantises_to_the_int16_oracle_on_the_extreme_programs(oracle):
    kinds = {"over": 0, "inf": 0, "nan": 0}
    for seed in tu.EXTREME_SEEDS:
        prg, rate, call = tu.extreme_program(seed)
        for stereo in (False, True):
            x, _ = _both(oracle, prg, rate, stereo, call, ("extreme", seed, stereo))
            c = classes(x)
            for k in kinds:
                kinds[k] += c[k]
    assert kinds["over"] > 0 and kinds["nan"] > 0, kinds  # (612 and 10687: feedback that runs to infinity)


def test_float_oracle_quantises_to_the_int16_oracle_on_the_lane_major_and_guard_programs(oracle):
    for name, (voices, ups) in tl.lanemajor_programs().items():
        prg = vb.build_program(voices, updates=ups)
        _both(oracle, prg, RATE, True, 70001, name, max_frames=70001)
    for name, voices in tg.guard_programs().items():
        prg = vb.build_program(voices)
        for stereo in (False, True):
            _both(oracle, prg, RATE, stereo, tg.CHUNK, name)


def test_silence_is_positive_zero_in_every_call(oracle):
    """the gap before a later voice and the frames behind the script's end are +0.0f in every call's buffer, whatever the call
    before left there (calls of 500 frames: the gap, frames 441 to 882, spans two of them). No sample here is a -0.0f: an
    accumulator that starts at +0.0f cannot become one by the mixer's additions (x + y is -0 only where both are), so the
    plain store and the reference's `+=` into a cleared buffer agree on that too."""
    one = vb.Op("sin", freq=441.0, amp=0.5, time_ms=10, pan=vb.Line(0.25))
    two = vb.Op("saw", freq=330.0, amp=0.5, time_ms=10, pan=vb.Line(0.75))
    two.start_ms = 20
    prg = vb.build_program([one, two])
    for stereo in (True, False):
        ch = 2 if stereo else 1
        calls = oracle.oracle_calls_f32(prg.ptr, RATE, stereo, chunk=500)
        assert [(m, n) for _, m, n in calls] == [(True, 500), (True, 500), (False, 323)]
        b = np.concatenate([c[0] for c in calls]).view(np.uint32)
        assert (b[441 * ch:882 * ch] == 0).all() and (b[1323 * ch:] == 0).all()
        assert b[:441 * ch].any() and b[882 * ch:1323 * ch].any() and not (b == 0x80000000).any()
        _both(oracle, prg, RATE, stereo, 500, "gap")


# ---- b. against the compiled reference -------------------------------------------------------------------------------------

def _normal_or_zero(x):
    c = classes(x)
    return c["subnormal"] == 0 and c["inf"] == 0 and c["nan"] == 0


@pytest.mark.parametrize("events", [False, True])
def test_scaled_float_oracle_vs_reference(oracle, sa, tables, events):
    """quantise(x * 2^k) == the compiled reference at ampmult * 2^k, on the reference's own wave tables"""
    if not oracle.have_ref():
        pytest.skip("compiled reference not present")
    with ref_tables(sa, oracle, tables):
        oracle.oracle().ora_set_fastmath_forms(2)
        make = later_event_graph if events else random_graph
        over = total = 0
        for seed in range(48 if events else 64):
            prg, stereo, chunk = make(seed)
            x = oracle.oracle_render_f32(prg.ptr, RATE, stereo, chunk=chunk)
            assert _normal_or_zero(x), (seed, classes(x))
            over, total = over + int((np.abs(x) > 1).sum()), total + len(x)
            for k in SCALES:
                scaled = x * np.float32(2.0 ** k)
                assert _normal_or_zero(scaled), (seed, k, classes(scaled))  # (the scaling is exact: nothing under- or overflows)
                prg_k, _, _ = make(seed, ampmult=2.0 ** k)
                ref = oracle.ref_render(prg_k.ptr, RATE, stereo, chunk=chunk)
                assert len(ref) == len(x), (seed, k, len(ref), len(x))
                d = np.flatnonzero(quantise(x, k) != ref)
                assert len(d) == 0, f"seed {seed} k {k}: {len(d)} samples differ, first at {d[0]}: float {x[d[0]]!r} reference {ref[d[0]]}"
                if k == -12:
                    assert np.abs(ref.astype(np.int32)).max() < 32767, (seed, "a reference sample is clamped at k = -12")
        assert over > total // 10, (over, total)  # (the samples beyond +-1 that k = -12 brings into range)


# ---- c. the edge programs --------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def edge_counts(name):
    """-> the counts of the edge program's float samples, stereo and mono together"""
    from oracle import pyoracle as po
    prg = edge_program(*EDGES[name])
    x = np.concatenate([po.oracle_render_f32(prg.ptr, RATE, stereo, chunk=4096) for stereo in (True, False)])
    return classes(x), x


def test_edge_programs_reach_what_they_are_for(oracle):
    """measured on x86-64: (1e-38, 1) all 6615 samples subnormal, (1e-30, 2^-40) 6572, (1, 2^-140) 6558; (3e38, 1) all beyond 1
    and none infinite; (1e30, 1e30) 877 infinities, of both signs, and 5738 NaN. Lower bounds are asserted."""
    for name in ("subnormal", "subnormal scaled", "subnormal ampmult"):
        c, _ = edge_counts(name)
        assert c["n"] == 6615 and c["subnormal"] > 6000 and c["inf"] == c["nan"] == c["over"] == 0, (name, c)
    c, _ = edge_counts("over range")
    assert c["n"] == 6615 and c["over"] > 6000 and c["inf"] == 0 and c["nan"] == 0, c
    c, x = edge_counts("infinite")
    assert c["n"] == 6615 and c["inf"] > 500 and c["nan"] > 4000, c
    pos, neg = int((x == np.inf).sum()), int((x == -np.inf).sum())
    assert pos > 0 and neg > 0, (pos, neg)


def test_every_nan_of_this_host_carries_the_sign_bit(oracle):
    """x86's default NaN (inf - inf, 0 * inf) is 0xFFC00000; a GPU's need not be, which is why tests/test_gpu_f32_oracle.py asks of
    the device only a NaN where the oracle has one. Recorded here so that the rule is seen to be needed."""
    import platform
    if platform.machine() not in ("x86_64", "AMD64"):
        pytest.skip("the default NaN of another architecture")
    n = 0
    _, x = edge_counts("infinite")
    progs = [x]
    for seed in (612, 10687):
        prg, rate, call = tu.extreme_program(seed)
        progs.append(oracle.oracle_render_f32(prg.ptr, rate, True, chunk=call))
    for x in progs:
        nan = x[np.isnan(x)].view(np.uint32)
        n += len(nan)
        assert ((nan >> 31) == 1).all(), hex(int(nan[(nan >> 31) == 0][0]))
    assert n > 5000, n
