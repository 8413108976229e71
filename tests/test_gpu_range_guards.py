"""The kernels' short rounding forms on both sides of their guards, rendered.

Phase offsets and increments are rounded by short forms that are exact only inside a range (k_common.h: rint32w_p31_small for
|p| < 2^20, rint32w_small for |x| < 2^51); a guard sends a lane or a whole wave to the general form (sau_dev_math.h: rint32w,
rint32w_p31) when a value is outside it. tests/test_gpu_units.py checks each form on every f32 bit pattern; here programs drive
the values across each guard inside a row group -- waves whose lanes straddle it -- and across the points where the short forms
really are wrong (2^20 for offsets, 2^51 for increments), under every route that holds a guard. Every render equals the oracle's
and the compiled reference's bit for bit, and every test shows that its route ran (kernel times, SAU_AMD_DEBUG_DUO).

guard_programs() is shared with tests/test_oracle.py, which pins the oracle to the compiled reference on the same programs."""
import re

import numpy as np
import pytest

from conftest import need_ref, ref_tables, ORACLE_FORMS
from saugns_amd import voicebank as vb
from saugns_amd.api import POP_FMOD, POP_FPMOD, POP_PMOD, POPT_RASEG

RATE = 44100
CHUNK = 5000  # (both sides make calls of this size: the reference build's loop tails fall where its blocks end)
M20 = float(2 ** 20)


def _pm_voice(mod_hz, fpm=False, wave="sin"):
    """a 440 Hz carrier phase-modulated by a sine whose amplitude ramps 0.9 * 2^20 -> 1.1 * 2^20: the offsets cross 2^20"""
    mods = {POP_PMOD: [vb.Op("sin", freq=mod_hz, time_ms=300, amp=vb.Line(0.9 * M20, goal=1.1 * M20))]}
    if fpm:
        mods[POP_FPMOD] = [vb.Op("sin", freq=5.0, time_ms=300, amp=0.3)]
    return vb.Op(wave, freq=440.0, time_ms=300, mods=mods)


def _inc_voices():
    """carriers whose coeff * f (coeff = 2^32 / 44100) crosses 2^50 (f = 1.16e10) and 2^51 (f = 2.3e10): ramps across one and both,
    and a 1.2e10 carrier whose FM swings 0.05e10 .. 2.35e10 and back. (Above 2^51 one increment in 16 is a multiple of 2^32, a
    repeated phase: the ramps stay short enough there for the repair pass, not the block loop.)"""
    return [vb.Op("sin", freq=vb.Line(1e10, goal=3e10), time_ms=300),
            vb.Op("tri", freq=vb.Line(1e10, goal=1.4e10, shape="exp"), time_ms=300),
            vb.Op("saw", freq=vb.Line(2.2e10, goal=2.5e10), time_ms=300),
            vb.Op("sin", freq=1.2e10, time_ms=300, mods={POP_FMOD: [vb.Op("sin", freq=7.0, time_ms=300, amp=1.15e10)]})]


def _fb_voices():
    """W self-modulation (chain_kernel, the block loop's feedback path): amounts that cross chain_batch's 2^14 switch, that make
    |fb_s * amount| pass 2^20, and a constant one above it -- on sin, saw and sqr -- beside plain feedback voices, so that the
    chain waves mix small and large lanes; and feedback voices whose increments cross 2^50 and 2^51 (the feeders' guards: an
    `exp` glide takes the straight-line feeder, a `lin` ramp the general one)"""
    voices = []
    for w in ("sin", "saw", "sqr"):
        for a in (vb.Line(1e4, goal=3e4), vb.Line(1e5, goal=float(2 ** 22)), 3e6):
            voices.append(vb.Op(w, freq=220.0 + 10 * len(voices), time_ms=300, pm_a=a, amp=0.5))
        voices.append(vb.Op(w, freq=150.0 + 10 * len(voices), time_ms=300, pm_a=0.5, amp=0.5))
    voices.append(vb.Op("sin", freq=vb.Line(1e10, goal=3e10, shape="exp"), time_ms=300, pm_a=0.5, amp=0.5))
    voices.append(vb.Op("saw", freq=vb.Line(3e10, goal=1e10, shape="exp"), time_ms=300, pm_a=vb.Line(0.2, goal=0.9), amp=0.5))
    voices.append(vb.Op("sin", freq=vb.Line(1e10, goal=3e10, shape="lin"), time_ms=300, pm_a=vb.Line(0.3, goal=0.7, shape="cos"),
                        amp=0.5))
    return voices


def _rfb_voices():
    """R self-modulation (rchain_kernel): feedback offsets of up to 2e10 cycles, both signs -- the reference's floorf wraps at
    2^31 (sau_dev_math.h: floor_i32_ref) -- over several line shapes and functions"""
    kinds = (("lin", 0), ("cos", 1), ("sqe", 2), ("xpe", 3), ("smo", 4), ("sah", 5), ("uwh", 0), ("nhl", 2))
    voices = []
    for k, (line, func) in enumerate(kinds):
        sign = -1.0 if k % 2 else 1.0
        voices.append(vb.Op(op_type=POPT_RASEG, ras=(line, func, (0, 9, 25)[k % 3]), seed=31 + 7 * k, freq=110.0 + 37 * k, time_ms=300,
                            amp=0.5, pm_a=vb.Line(sign * 1e9, goal=sign * 2e10, shape=("lin", "exp", "cos")[k % 3])))
    return voices


def guard_programs():
    """name -> voices of each program (build with voicebank.build_program)"""
    return {
        "pm": [_pm_voice(3.0), _pm_voice(2000.0, wave="tri"), _pm_voice(3.0, fpm=True, wave="saw")],
        "inc": _inc_voices(),
        "fb": _fb_voices(),
        "rfb": _rfb_voices(),
    }



def _bank():
    """the duo tests' PM and FM voices (tests/test_gpu_duo.py) with the PM and increment programs' voices among them"""
    import test_gpu_duo as td
    voices = []
    for i in range(24):
        voices += [td._pm_voice(i, 300), td._fm_voice(i, 300)]
        if i % 8 == 0:
            g = guard_programs()  # (new operators each time: a voice's operators are its own)
            voices += g["pm"] + g["inc"]
    return voices


class _Routes:
    """One program rendered under kernel settings in turn, each compared with the oracle's PCM -- and with the compiled
    reference's, which the oracle's must equal -- on the reference's own wave tables."""

    def __init__(self, sa, oracle, tables, monkeypatch, voices):
        need_ref(oracle)
        self.sa, self.mp = sa, monkeypatch
        self.prg = vb.build_program(voices)
        self._tabs = ref_tables(sa, oracle, tables)
        self._tabs.__enter__()
        oracle.oracle().ora_set_fastmath_forms(ORACLE_FORMS)
        self.want = oracle.oracle_render(self.prg.ptr, RATE, False, chunk=CHUNK)
        if ORACLE_FORMS == 2:  # (the product's default: the reference build's loop tails, tests/conftest.py)
            ref = oracle.ref_render(self.prg.ptr, RATE, False, chunk=CHUNK)
            assert len(ref) == len(self.want) and (ref == self.want).all(), "the oracle is not the compiled reference here"

    def close(self):
        self._tabs.__exit__(None, None, None)

    def render(self, **env):
        """-> timing_ex() of the render under `env` (SAU_AMD_<name>: value), after checking its PCM"""
        for k, v in env.items():
            self.mp.setenv("SAU_AMD_" + k, str(v))
        try:
            b = self.sa.Batch([self.prg], RATE)
            b.set_timing(2)
            got = b.render(stereo=False, chunk=CHUNK)[0]
            t = b.timing_ex()
            b.close()
        finally:
            for k in env:
                self.mp.delenv("SAU_AMD_" + k, raising=False)
        d = np.nonzero(got[:len(self.want)] != self.want[:len(got)])[0]
        assert len(got) == len(self.want) and len(d) == 0, (env, len(got), len(self.want), len(d), d[:6].tolist())
        return t


@pytest.fixture()
def routes(sa, oracle, tables, monkeypatch):
    made = []

    def make(voices):
        r = _Routes(sa, oracle, tables, monkeypatch, voices)
        made.append(r)
        return r
    yield make
    for r in made:
        r.close()


CLOSED_FORM = [{}, {"NO_INNER": 1}, {"MORE_ROWS": 0}, {"MORE_ROWS": 10}, {"NO_WIDE_TABS": 1},
               {"FAST_ROWS": 2}, {"FAST_ROWS": 5}, {"FAST_ROWS": 6}]


@pytest.mark.gpu
def test_pm_offsets_across_2_20_in_the_closed_form(routes):
    """PM offsets that cross 2^20 cycles slowly (a 3 Hz modulator), in most row groups (2 kHz) and beside an FPM modulator: the
    common path's wave-wide fallback and the general path's choice of rint32w_p31, at every closed-form build; then the block
    loop. The time-parallel renders leave nothing to the block loop."""
    r = routes(guard_programs()["pm"])
    for env in CLOSED_FORM:
        t = r.render(**env)
        assert t["block_ms"] < 1.0 and t["fast_ms"] > 0, (env, t)
    assert r.render(NO_FAST=1)["block_ms"] > 0


@pytest.mark.gpu
def test_increments_across_2_50_and_2_51_in_the_running_sums(routes):
    """Swept and frequency-modulated carriers whose increments cross the short form's guard (2^50) and the point where it is wrong
    (2^51), both ways: the single pass with look-back (one test per wave), the several passes (one per lane), and the block loop."""
    r = routes(guard_programs()["inc"])
    t = r.render(LOOK_MIN_VOICES=1)
    assert t["block_ms"] < 1.0 and t["fast_ms"] > 0, t
    t = r.render(NO_LOOKBACK=1)
    assert t["block_ms"] < 1.0 and t["fast_ms"] > 0, t
    assert r.render(NO_FAST=1)["block_ms"] > 0


LINE_DUO = re.compile(r"\[sau-amd\] duo (\d):")


@pytest.mark.gpu
def test_pm_and_increment_voices_in_a_bank(routes, capfd, monkeypatch):
    """The PM and increment voices among the duo tests' plain PM and FM voices: closed-form and look-back waves in one launch
    (duo_kernel, said by SAU_AMD_DEBUG_DUO), the two launches apart, and the several-pass form."""
    r = routes(_bank())
    capfd.readouterr()
    monkeypatch.setenv("SAU_AMD_DEBUG_DUO", "1")
    t = r.render()
    assert t["block_ms"] < 1.0, t
    duos = [int(m.group(1)) for m in LINE_DUO.finditer(capfd.readouterr().err)]
    assert 1 in duos, "the joint launch did not run"
    t = r.render(NO_DUO=1)
    assert t["block_ms"] < 1.0, t
    assert 1 not in [int(m.group(1)) for m in LINE_DUO.finditer(capfd.readouterr().err)]
    t = r.render(NO_LOOKBACK=1)
    assert t["block_ms"] < 1.0, t


@pytest.mark.gpu
def test_w_feedback_across_its_switches(routes):
    """W self-modulation across chain_batch's 2^14 switch and the per-sample 2^20 test of its general instances, with increments
    across 2^50 / 2^51 from both feeders: chain_kernel fed by its own lines, fed through rows (SAU_AMD_NO_CHAIN_INLINE: the
    increments then come from the several-pass rows), without early chains, and the block loop's feedback path."""
    r = routes(guard_programs()["fb"])
    loop = r.render(NO_CHAIN=1)
    assert loop["block_ms"] > 0
    for env in ({}, {"NO_CHAIN_INLINE": 1}, {"NO_EARLY_CHAINS": 1}):
        # (chain_kernel runs beside the time-parallel launches, whose measured time then holds the chains' serial steps; with
        #  SAU_AMD_NO_CHAIN those launches have nothing of these voices)
        t = r.render(**env)
        assert t["fast_ms"] > 2 * loop["fast_ms"], (env, t, loop)
    assert r.render(NO_CHAIN=1, NO_FAST=1)["block_ms"] > 0


@pytest.mark.gpu
def test_r_feedback_offsets_past_2_31_cycles(routes):
    """R self-modulation of up to 2e10 cycles, both signs: rchain_kernel and the block loop wrap floorf's conversion at 2^31 as the
    reference's build does."""
    r = routes(guard_programs()["rfb"])
    t = r.render()
    assert t["block_ms"] < 1.0, t
    assert r.render(NO_CHAIN=1)["block_ms"] > 0
