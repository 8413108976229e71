"""The inner launch of the 12-row closed-form build in the lane-major form (k_fast_group_lm.h: lane l, register k holds the group's
frame 12 l + k) against the oracle, bit for bit, with the row-major form (SAU_AMD_NO_LANEMAJOR) as the control. SAU_AMD_INNER_REPORT
says which form the inner launch took -- each render here must have taken it, in the form asked for. Every render runs with
SAU_AMD_POISON (tests/test_gpu_poison.py): a frame of a voice row or a pan row that the new mapping fails to store reads about 0.32
and shows in the PCM."""
import re

import numpy as np
import pytest

from conftest import ORACLE_FORMS
from saugns_amd import voicebank as vb
from saugns_amd.api import POP_PMOD

pytestmark = pytest.mark.gpu

RATE = 44100
INNER = re.compile(r"\[sau-amd\] inner: (lane-major|row-major)")


@pytest.fixture(autouse=True)
def switches(monkeypatch, oracle):
    monkeypatch.setenv("SAU_AMD_POISON", "1")
    monkeypatch.setenv("SAU_AMD_INNER_REPORT", "1")
    oracle.oracle().ora_set_fastmath_forms(ORACLE_FORMS)


def _both_forms(sa, oracle, capfd, monkeypatch, prg, stereo, chunk, what):
    want = oracle.oracle_render(prg.ptr, RATE, stereo, chunk=chunk)
    for form in ("lane-major", "row-major"):
        if form == "row-major":
            monkeypatch.setenv("SAU_AMD_NO_LANEMAJOR", "1")
        else:
            monkeypatch.delenv("SAU_AMD_NO_LANEMAJOR", raising=False)
        capfd.readouterr()
        batch = sa.Batch([prg], RATE)
        got = np.asarray(batch.render(stereo=stereo, chunk=chunk)[0]).reshape(-1)
        batch.close()
        forms = set(INNER.findall(capfd.readouterr().err))
        assert forms == {form}, (what, form, "the inner launch ran as", forms)
        assert len(got) == len(want), (what, form, len(got), len(want))
        d = np.flatnonzero(got != want)
        assert len(d) == 0, (f"{what} ({form}): {len(d)} samples differ, first at {d[0]}: "
                             f"got {got[d[0]:d[0] + 4].tolist()} want {want[d[0]:d[0] + 4].tolist()}")


@pytest.mark.parametrize("stereo", [False, True])
def test_config3_at_reduced_size(sa, oracle, capfd, monkeypatch, stereo):
    """BASELINE config 3's voices, 96 of them for 4 s with pans of their own and ends at different frames, in one run and in runs
    that cut the voices' groups elsewhere"""
    voices = vb.config3_voices(96, 4)
    for i, v in enumerate(voices):
        v.time_ms = 4000 - 37 * (i % 23)
        v.pan = vb.Line(vb._num(".2f", ((i * 29) % 100) / 100.0))
    prg = vb.build_program(voices)
    for chunk in (176400, 70001):
        _both_forms(sa, oracle, capfd, monkeypatch, prg, stereo, chunk, ("config 3", chunk))


def _drawn_voice(rng, depth, ms):
    """a carrier over a PM chain `depth` operators deep (1: none), sines throughout (one wave table: what lets a bank take the
    12-row build), ratios, amplitudes and pans drawn"""
    op = None
    for d in range(depth - 1):
        op = vb.Op("sin", freq=vb.Line(float(rng.integers(1, 6)), ratio=True), amp=vb._num(".2f", rng.uniform(0.1, 0.9)),
                   mods={POP_PMOD: [op]} if op else None)
    return vb.Op("sin", freq=vb._num(".3f", rng.uniform(60.0, 900.0)), time_ms=ms,
                 pan=vb.Line(vb._num(".2f", rng.uniform(0.0, 1.0))), mods={POP_PMOD: [op]} if op else None)


@pytest.mark.parametrize("seed", range(6))
def test_drawn_closed_form_banks(sa, oracle, capfd, monkeypatch, seed):
    """Banks drawn at random: 80 to 160 voices of nesting depth 1 to 4 side by side (so lead-ins of several lengths: groups that
    start on a multiple of four frames and groups that do not; deeper chains need more block buffers than LDS holds at 12 rows,
    and never reach this launch), 3 to 5 s, mono or stereo, runs that end short of the script or cut it elsewhere"""
    rng = np.random.default_rng(7700 + seed)
    n, seconds = int(rng.integers(80, 161)), int(rng.integers(3, 6))
    stereo = bool(seed % 2)
    voices = [_drawn_voice(rng, int(rng.integers(1, 5)), seconds * 1000 - int(rng.integers(0, 400))) for _ in range(n)]
    prg = vb.build_program(voices)
    chunk = int(seconds * RATE + rng.integers(-5000, 3000)) if seed < 3 else 66157
    _both_forms(sa, oracle, capfd, monkeypatch, prg, stereo, chunk, ("drawn", seed, n, seconds))


@pytest.mark.parametrize("stereo", [False, True])
def test_phase_steps_of_zero(sa, oracle, capfd, monkeypatch, stereo):
    """Carriers (and middle modulators) of frequency 0 under PM too small to move the phase every frame: the phase step is zero on
    runs of one to thousands of frames, and the differentiator holds its output (wosc.h:251-252) -- runs inside a lane, runs that
    cross from lane to lane, runs that reach back to the group's first defined frame (the repair pass, or the block loop)"""
    voices = []
    for i in range(96):
        # (2^-31 of a cycle is one phase step: amplitudes of 2^-31 * 20 .. 20000 step the phase every 1000th .. every frame)
        a = vb._f32(2.0 ** -31 * 20.0 * 10.0 ** ((i % 7) / 2.0))
        m2 = vb.Op("sin", freq=vb._num(".2f", 0.5 + (i % 5)), amp=a)
        if i % 3 == 0:
            m1 = vb.Op("sin", freq=0.0, amp=vb._num(".2f", 0.3 + (i % 4) * 0.1), mods={POP_PMOD: [m2]})
            mods = {POP_PMOD: [vb.Op("sin", freq=vb.Line(float(1 + i % 3), ratio=True), amp=0.5, mods={POP_PMOD: [m1]})]}
            freq = vb._num(".3f", 110.0 + 3.3 * i)
        else:
            mods = {POP_PMOD: [m2]} if i % 3 == 1 else {POP_PMOD: [vb.Op("sin", freq=3.0, amp=vb._f32(a * 0.5), mods={POP_PMOD: [m2]})]}
            freq = 0.0
        voices.append(vb.Op("sin", freq=freq, time_ms=4000 - 29 * (i % 17),
                            pan=vb.Line(vb._num(".2f", ((i * 13) % 100) / 100.0)), mods=mods))
    prg = vb.build_program(voices)
    for chunk in (176400, 70001):
        _both_forms(sa, oracle, capfd, monkeypatch, prg, stereo, chunk, ("holds", chunk))
