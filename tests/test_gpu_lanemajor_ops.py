"""Every branch of the lane-major row-group evaluation (k_fast_group_lm.h) that a segment can reach, against the oracle, bit for
bit, with the row-major form as the control -- tests/test_gpu_lanemajor.py's discipline on programs that leave its sine-over-small-PM
ground: PM across 2^20 cycles (the wave-wide fallback to rint32w_p31), frequency-scaled PM, N operators, the A operator and
oscillators that stand still, amplitude modulator lists and layered lists, the discontinuous waves, later events that cut
segments of many lengths, other sample rates, and the hand-off of hold runs to the repair pass and to the block loop.

What reaches the inner launch (hip_backend.hip): a closed-form-only segment of one wave table and one block buffer. A voice with
an R operator, with red noise or with a ramp ever given to one of its operators makes its segment one that may need running sums
(engine.cpp: static_block, goal_seen), and such a segment takes the builds with running sums, never the inner launch. So the R
branch and the ramps of k_fast_group_lm.h run only where SAU_AMD_NO_SEQ turns those builds off (a test switch): the legs marked
NO_SEQ below. The range ends of `r[...]` lists (ST_LERP, SF_WAVE_ENV), pan modulators (ST_VOICE, the pan row), PM beside
frequency-scaled PM and a table outside LDS need a second block buffer or are excluded by the launch's own conditions: DESIGN.md 5
has the table.

Every render runs with SAU_AMD_POISON; SAU_AMD_INNER_REPORT says, per closed-form segment, which form the inner launch took or
that the segment went without it; kernel times (set_timing(2)) say whether anything was left to the block loop.

lanemajor_programs() is shared with tests/test_oracle.py, which pins the oracle to the compiled reference on the same programs."""
import re

import numpy as np
import pytest

from conftest import ORACLE_FORMS
from saugns_amd import voicebank as vb
from saugns_amd.api import POP_AMOD, POP_FMOD, POP_FPMOD, POP_PMOD, POP_RAMOD, POPT_AMP, POPT_NOISE, POPT_RASEG

RATE = 44100
M20 = float(2 ** 20)
INNER = re.compile(r"\[sau-amd\] inner: (lane-major|row-major|none)")
# a segment without the inner launch says what kept it from it: rows per pass (12 is the launch's build), wide tables, tasks per voice
NONE = re.compile(r"\[sau-amd\] inner: none \(rows (\d+), wide (\d), chunks (\d+)\)")
# ramp shapes of an amplitude line (`cub` is a line shape like the others here: only R's `cub` segments have a build of their own)
SHAPES = "cos lin sah exp log xpe lge sqe cub smo".split()
# ... of which a `cub` ramp in progress keeps its voice in the block loop while the reference build's loop tails are reproduced
# (k_analyze.h: which samples take the tail form depends on where the reference's blocks end)
SHAPES_CLOSED = [x for x in SHAPES if x != "cub"]


def _shapes(ramps):
    """ramps: "closed" -- the shapes a closed form serves; "cub" -- every shape, `cub` among them"""
    return SHAPES if ramps == "cub" else SHAPES_CLOSED
# R oscillators: (line shape, function, flags) -- tests/test_oracle.py::test_r_oscillator_options_vs_reference's grid without `cub`;
# the flags hold both settings of the half-shape bit (sau_dev_ops.h: rate2x)
RAS = [(line, func, flags) for k, line in enumerate("cos lin sah exp log xpe lge sqe smo ncl nhl uwh".split())
       for func, flags in (((k) % 6, (0, 1, 2, 4, 8, 16, 9, 25, 31)[k % 9]), ((k + 3) % 6, (31, 25, 9, 16, 8, 4, 2, 1, 0)[k % 9]))]
NOISES_CLOSED = (0, 1, 2, 3, 5, 6)  # wh gw bw tw vi bv: a function of the frame's index (red noise, 4, is a running sum)


def _sin(freq, amp, ratio=True, **kw):
    return vb.Op(kw.pop("wave", "sin"), freq=vb.Line(float(freq), ratio=ratio), amp=amp, **kw)


def _carrier(i, ms, mods=None, wave="sin", **kw):
    """voice i's carrier: frequencies, pans and ends of its own"""
    return vb.Op(wave, freq=vb._num(".3f", 97.0 + 7.31 * i), time_ms=ms - 31 * (i % 19),
                 pan=vb.Line(vb._num(".2f", ((i * 37) % 100) / 100.0)), mods=mods, **kw)


def _small_pm(i, wave="sin", phase=0.0):
    """config 3's kind of chain, one or two modulators deep"""
    m = _sin(2 + i % 3, vb._num(".2f", 0.3 + (i % 5) * 0.1), wave=wave, phase=phase)
    if i % 2:
        m = _sin(1 + i % 4, vb._num(".2f", 0.5 + (i % 7) * 0.1), wave=wave, phase=phase, mods={POP_PMOD: [m]})
    return {POP_PMOD: [m]}


def big_pm_bank(n=96, ms=3000, ramps=False):
    """PM offsets across 2^20 cycles (tests/test_gpu_range_guards.py::_pm_voice's amplitudes, 0.9 to 1.1 times 2^20): under a
    modulator of 2 to 5 Hz some 768-frame groups lie wholly below 2^20, some straddle it and some lie wholly above; under one of
    2 kHz most groups cross; at 0.9 * 2^20 none does. A third of the voices have small PM, so waves take both paths in one launch;
    some have the large offsets one level down, on a modulator. ramps: the amplitudes as ramps from 0.9 to 1.1 times 2^20, which
    only a NO_SEQ leg takes to the inner launch."""
    voices = []
    for i in range(n):
        a = M20 * (0.9, 1.0, 1.05, 1.1)[(i // 3) % 4]
        if ramps:
            a = vb.Line(0.9 * M20, goal=1.1 * M20, shape=_shapes(ramps)[i % len(_shapes(ramps))])
        if i % 3 == 0:
            mods = _small_pm(i)
        elif i % 3 == 1:
            mods = {POP_PMOD: [_sin((2.0, 3.0, 5.0, 2000.0)[(i // 12) % 4], a, ratio=False)]}
        else:
            inner = _sin((3.0, 2000.0)[(i // 6) % 2], a, ratio=False)
            mods = {POP_PMOD: [_sin(2, 0.6, mods={POP_PMOD: [inner]})]}
        voices.append(_carrier(i, ms, mods))
    return voices


def fpm_bank(n=96, ms=3000):
    """frequency-scaled PM alone (pm_offset32(false, true, ...) with the operator's own frequency): small, and with
    amplitude x frequency at 0.9 to 1.1 times 2^20, on carriers and one level down"""
    voices = []
    for i in range(n):
        c = _carrier(i, ms)
        f = c.freq.v0
        if i % 3 == 0:
            c.mods = {POP_FPMOD: [_sin(1 + i % 3, vb._num(".3f", 0.002 * (1 + i % 5)))]}
        elif i % 3 == 1:
            c.mods = {POP_FPMOD: [_sin((2.0, 5.0, 2000.0)[(i // 3) % 3], vb._f32(M20 * (0.9, 1.02, 1.1)[(i // 9) % 3] / f), ratio=False)]}
        else:
            m = _sin(2, 0.5, mods={POP_FPMOD: [_sin(3.0, vb._f32(M20 * (0.95, 1.08)[(i // 3) % 2] / (2 * f)), ratio=False)]})
            c.mods = {POP_PMOD: [m]}
        voices.append(c)
    return voices


def noise_bank(n=84, ms=3000, red=False):
    """N operators of every type that is a function of the frame's index (NZ_vi and NZ_bv read index n - 1 too), as phase
    modulators, amplitude modulators, below a sine modulator and layered behind one, beside plain sine chains.
    red: one voice's noise is red noise, a running sum -- the negative control."""
    voices = []
    for i in range(n):
        nz = NOISES_CLOSED[i % 6] if not (red and i == 17) else 4
        N = vb.Op(amp=vb._num(".2f", 0.05 + 0.05 * (i % 4)), op_type=POPT_NOISE, noise=nz, seed=(0, 1, 0x9e3779b9, 77)[(i // 6) % 4] + i)
        kind = (i // 6) % 5
        if kind == 0:
            mods = {POP_PMOD: [N]}
        elif kind == 1:
            mods = {POP_AMOD: [N]}
        elif kind == 2:
            mods = {POP_PMOD: [_sin(2, 0.5, mods={POP_PMOD: [N]})]}
        elif kind == 3:
            mods = {POP_PMOD: [_sin(1 + i % 3, 0.4), N]}
        else:
            mods = _small_pm(i)
        voices.append(_carrier(i, ms, mods))
    return voices


def _A(amp, **kw):
    return vb.Op(amp=amp, op_type=POPT_AMP, **kw)


def amp_op_bank(n=84, ms=3000, ramps=False):
    """The A operator (tests/test_gpu_units.py::amp_operator_cases, the roles that need one block buffer) as phase modulator,
    amplitude modulator, frequency-scaled phase modulator, alone and layered beside a sine, with an amplitude list of its own;
    and W operators of frequency 0 without modulators, whose output stands still: they share the A operator's branch, with
    the value held in place of A's 1 (k_decode.h). ramps: the A operators' amplitudes ramp (a NO_SEQ leg)."""
    voices = []
    for i in range(n):
        a = vb._num(".2f", 0.15 + 0.1 * (i % 6))
        amp = vb.Line(0.0, goal=a * 2, shape=_shapes(ramps)[i % len(_shapes(ramps))]) if ramps else a
        kind = i % 7
        if kind == 0:
            mods = {POP_PMOD: [_A(amp)]}
        elif kind == 1:
            mods = {POP_AMOD: [_A(amp)]}
        elif kind == 2:
            mods = {POP_PMOD: [_A(amp), _sin(3.0, 0.5, ratio=False)]}
        elif kind == 3:
            mods = {POP_AMOD: [_sin(7.0, 0.2, ratio=False), _A(amp)]}
        elif kind == 4:
            mods = {POP_FPMOD: [_A(vb._num(".4f", 0.001 * (1 + i % 4)))]}
        elif kind == 5:
            mods = {POP_PMOD: [_A(amp, mods={POP_AMOD: [_sin(11.0, 0.3, ratio=False)]})]}
        else:
            still = vb.Op("sin", freq=0.0, amp=vb._num(".2f", 0.2 + 0.1 * (i % 5)), phase=vb._num(".3f", (0.11 * i) % 1.0))
            mods = {POP_PMOD: [still]} if (i // 7) % 2 else {POP_PMOD: [_sin(2, 0.5, mods={POP_PMOD: [still]})]}
        voices.append(_carrier(i, ms, mods))
    return voices


def still_bank(n=80, ms=3000):
    """W operators of frequency 0 without modulators -- their output stands still, and the step becomes a constant source
    with the held value where the A operator has its 1 (k_decode.h) -- as phase modulators at initial phases of their own,
    directly and one level down, beside plain sine chains"""
    voices = []
    for i in range(n):
        still = vb.Op("sin", freq=0.0, amp=vb._num(".2f", 0.2 + 0.1 * (i % 5)), phase=vb._num(".3f", (0.11 * i + 0.05) % 1.0))
        mods = ({POP_PMOD: [still]}, {POP_PMOD: [_sin(2, 0.5, mods={POP_PMOD: [still]})]}, _small_pm(i))[i % 3]
        voices.append(_carrier(i, ms, mods))
    return voices


def amod_bank(n=90, ms=3000, ramps=False):
    """Amplitude modulator lists (the operator reads its amplitudes from a block: amp_off) of one, two and three members, on
    carriers and on modulators, and phase modulator lists of two and three members (SF_LAYER: each member after the first is
    added onto the block the ones before have written, out_off). ramps: the operators' amplitudes are ramps of every shape, with
    goals reached after a modulator's second and never reached on a carrier (a NO_SEQ leg)."""
    voices = []
    for i in range(n):
        lf = lambda k: _sin(vb._num(".2f", 2.5 + 1.7 * k + 0.3 * (i % 5)), vb._num(".2f", 0.1 + 0.05 * ((i + k) % 4)), ratio=False)
        shapes = _shapes(ramps)
        shape = shapes[i % len(shapes)]
        ma = vb.Line(0.1, goal=0.8, shape=shape) if ramps else 0.5
        ca = vb.Line(0.9, goal=0.2, shape=shapes[(i + 3) % len(shapes)]) if ramps else vb._num(".2f", 0.4 + 0.1 * (i % 5))
        kind = i % 6
        if kind == 0:
            mods = {POP_AMOD: [lf(0)]}
        elif kind == 1:
            mods = {POP_AMOD: [lf(0), lf(1)]}
        elif kind == 2:
            mods = {POP_AMOD: [lf(0), lf(1), lf(2)]}
        elif kind == 3:
            mods = {POP_PMOD: [_sin(1 + i % 3, ma), _sin(2 + i % 2, 0.3)]}
        elif kind == 4:
            mods = {POP_PMOD: [_sin(1, ma), _sin(3, 0.2), _sin(5.0, 0.3, ratio=False)]}
        else:
            mods = {POP_PMOD: [_sin(2, ma, mods={POP_AMOD: [lf(0), lf(1)]})]}
        voices.append(_carrier(i, ms, mods, amp=ca))
    return voices


def wave_bank(wave, n=96, ms=3000):
    """config 3's kind of bank with every operator `wave` and initial phases of their own"""
    return [_carrier(i, ms, _small_pm(i, wave, vb._num(".3f", (0.173 * i) % 1.0)), wave, phase=vb._num(".3f", (0.071 * i) % 1.0))
            for i in range(n)]


def r_bank(n=96, ms=3000):
    """R operators of many line shapes, functions and flags (both settings of the half-shape bit) as phase modulators -- plain
    and with PM of their own from a sine -- and as carriers under a sine's PM, beside sine chains (a NO_SEQ leg)"""
    voices = []
    for i in range(n):
        ras = RAS[i % len(RAS)]
        kind = (i // len(RAS)) % 4
        R = lambda **kw: vb.Op(op_type=POPT_RASEG, ras=ras, seed=12345 + 7 * i, **kw)
        if kind == 0:
            v = _carrier(i, ms, {POP_PMOD: [R(freq=vb.Line(float(1 + i % 3), ratio=True), amp=0.6)]})
        elif kind == 1:
            v = _carrier(i, ms, {POP_PMOD: [R(freq=vb.Line(2.0, ratio=True), amp=0.5, mods={POP_PMOD: [_sin(0.5, 0.4)]})]})
        elif kind == 2:
            c = _carrier(i, ms)
            v = R(freq=c.freq, time_ms=c.time_ms, pan=c.pan, amp=0.8, mods={POP_PMOD: [_sin(2, 0.3)]})
        else:
            v = _carrier(i, ms, _small_pm(i))
        voices.append(v)
    return voices


def mixed_bank(n=96, ms=3000):
    """voices of the default-path banks side by side (the sample-rate legs)"""
    banks = [big_pm_bank(n, ms), fpm_bank(n, ms), noise_bank(n, ms), amp_op_bank(n, ms), amod_bank(n, ms)]
    return [banks[i % 5][i] for i in range(n)]


def events_bank(n=96, ms=4000):
    """-> (voices, updates): sine PM chains with later events on different voices at different times: new amplitudes, new
    frequencies (one value for another), new phases and new modulator lists. Every event ends the segment for the whole bank:
    long segments, segments of some tens of milliseconds, and bursts of events 3 to 20 ms apart, whose segments hold fewer than
    three tasks of row groups -- too short for the inner launch. The times are placed so that for every group length in use
    (768 frames less a lead-in of up to 8) one segment ends 2 to 7 frames after one of its group boundaries."""
    voices = [_carrier(i, ms, _small_pm(i)) for i in range(n)]
    for v in voices:
        v.time_ms = ms  # (events need their voices alive)
    fr = lambda t: int(round(t * RATE / 1000.0))
    times, t = [], 150
    for gf in range(760, 768):  # a segment from the event before that ends just past a group boundary
        u = t + 120
        while not 2 <= (fr(u) - fr(t)) % gf <= 7:
            u += 1
        times.append(u)
        t = u
    for k in range(4):  # bursts: segments of 3 .. 20 ms
        t += 180
        times += [t, t + 3, t + 10, t + 30]
        t += 30
    assert t < ms - 100, t
    ups = []
    for k, at in enumerate(times):
        vi = (k * 17) % n
        carr = voices[vi]
        m = carr.mods[POP_PMOD][0]
        what = k % 5
        if what == 0:
            ups.append((at, vi, m, {"amp": vb.Line(vb._num(".2f", 0.2 + 0.1 * (k % 6)))}))
        elif what == 1:
            ups.append((at, vi, carr, {"freq": vb.Line(vb._num(".2f", 150.0 + 11.0 * k))}))
        elif what == 2:
            ups.append((at, vi, m, {"freq": vb.Line(float(1 + k % 4), ratio=True), "phase": vb._num(".3f", (0.13 * k) % 1.0)}))
        elif what == 3:
            ups.append((at, vi, carr, {"phase": vb._num(".3f", (0.29 * k) % 1.0), "amp": vb.Line(vb._num(".2f", 0.5 + 0.05 * (k % 8)))}))
        else:
            ups.append((at, vi, carr, {"mods": {POP_PMOD: []}} if k % 2 else {"mods": {POP_PMOD: [m]}}))
    return voices, ups


def zero_step_bank(n=96, ms=4000):
    """tests/test_gpu_lanemajor.py::test_phase_steps_of_zero's voices"""
    voices = []
    for i in range(n):
        a = vb._f32(2.0 ** -31 * 20.0 * 10.0 ** ((i % 7) / 2.0))
        m2 = vb.Op("sin", freq=vb._num(".2f", 0.5 + (i % 5)), amp=a)
        if i % 3 == 0:
            m1 = vb.Op("sin", freq=0.0, amp=vb._num(".2f", 0.3 + (i % 4) * 0.1), mods={POP_PMOD: [m2]})
            mods = {POP_PMOD: [vb.Op("sin", freq=vb.Line(float(1 + i % 3), ratio=True), amp=0.5, mods={POP_PMOD: [m1]})]}
            freq = vb._num(".3f", 110.0 + 3.3 * i)
        else:
            mods = {POP_PMOD: [m2]} if i % 3 == 1 else {POP_PMOD: [vb.Op("sin", freq=3.0, amp=vb._f32(a * 0.5), mods={POP_PMOD: [m2]})]}
            freq = 0.0
        voices.append(vb.Op("sin", freq=freq, time_ms=ms - 29 * (i % 17),
                            pan=vb.Line(vb._num(".2f", ((i * 13) % 100) / 100.0)), mods=mods))
    return voices


def many_holds_bank(n=80, ms=3000):
    """Carriers of frequency 0 whose PM moves the phase by about one step in two or three frames for most of the time: a
    repeated phase on the first defined frame of every second or third of a voice's 170 row groups in a 3 s segment, each a note
    for the repair pass -- far more than the 15 a voice may leave (FAST_MAX_REPAIR): these voices go to the block loop."""
    voices = []
    for i in range(n):
        hz = 0.5 + 0.25 * (i % 5)
        steps = (0.35 + 0.05 * (i % 4)) * RATE / (2 * np.pi * hz)  # amplitude in phase steps: at most 0.35 .. 0.5 steps a frame
        voices.append(_carrier(i, ms, {POP_PMOD: [_sin(hz, vb._f32(steps * 2.0 ** -31), ratio=False)]}))
        voices[-1].freq = vb.Line(0.0)
    return voices


def far_holds_bank(n=96, ms=3000):
    """Carriers of frequency 0 under a slow sine's PM of about 10^5 phase steps: the phase moves by several steps a frame except
    around the modulator's two to four peaks in the segment. With a = amplitude x (radians per frame)^2 = 1/2000 (1/1000 for
    every third voice), the phase stands for 2 sqrt(2 / a) = 126 (89) frames at a peak, and repeats now and then only within
    1 / a frames of it -- five (two or three) row groups, about half of them noted for the repair pass: some ten notes a voice,
    below the 15 it may leave (FAST_MAX_REPAIR). Where the run at the peak covers a group's first defined frame and goes on for
    more than the 32 frames the pass stores -- one peak in eight (fourteen) -- the group is one for held_far, and the voice goes
    to the block loop on its account alone. 96 voices with frequencies and phases of their own: a few dozen such groups."""
    voices = []
    for i in range(n):
        hz = (0.35, 0.5, 0.65)[i % 3]
        w = 2 * np.pi * hz / RATE
        steps = 1.0 / ((1000.0 if i % 3 == 2 else 2000.0) * w * w)
        m = _sin(hz, vb._f32(steps * 2.0 ** -31), ratio=False, phase=vb._num(".3f", (0.137 * i) % 1.0))
        voices.append(_carrier(i, ms, {POP_PMOD: [m]}))
        voices[-1].freq = vb.Line(0.0)
    return voices


def not_inner_banks(ms=3000):
    """name -> voices of banks that must not take the inner launch: one voice with two block buffers (an `r[...]` list with a
    second amplitude) among one-buffer voices; two wave tables; a modulator with a frequency ramp (its phases are a running sum);
    red noise (another running sum)"""
    two = [_carrier(i, ms, _small_pm(i)) for i in range(80)]
    two[41] = _carrier(41, ms, {POP_RAMOD: [_sin(4.0, 1.0, ratio=False)]}, amp=0.3, amp2=0.9)
    waves = [_carrier(i, ms, _small_pm(i, "tri" if i == 57 else "sin")) for i in range(80)]
    ramp = [_carrier(i, ms, _small_pm(i)) for i in range(80)]
    ramp[23] = _carrier(23, ms, {POP_PMOD: [vb.Op("sin", freq=vb.Line(2.0, goal=3.0, ratio=True), amp=0.5)]})
    return {"two buffers": two, "two waves": waves, "frequency ramp": ramp, "red noise": noise_bank(84, ms, red=True)}


def _banks():
    """name -> function that makes (voices, later events)"""
    plain = lambda fn, **kw: (lambda: (fn(**kw), ()))
    banks = {
        "big pm": plain(big_pm_bank), "big pm ramps": plain(big_pm_bank, ramps="closed"), "fpm": plain(fpm_bank),
        "noise": plain(noise_bank), "amp op": plain(amp_op_bank), "still": plain(still_bank), "amp op ramps": plain(amp_op_bank, ramps="closed"),
        "amod": plain(amod_bank), "amod ramps": plain(amod_bank, ramps="closed"), "amod ramps cub": plain(amod_bank, ramps="cub"),
        "r": plain(r_bank), "mixed": plain(mixed_bank),
        "events": events_bank, "zero steps": plain(zero_step_bank), "many holds": plain(many_holds_bank),
        "far holds": plain(far_holds_bank),
    }
    for w in ("tri", "saw", "sqr"):
        banks["wave " + w] = plain(wave_bank, wave=w)
    for name in ("two buffers", "two waves", "frequency ramp", "red noise"):
        banks["not inner: " + name] = (lambda name=name: (not_inner_banks()[name], ()))
    return banks


def lanemajor_programs():
    """name -> (voices, later events) of every program rendered here (build with voicebank.build_program)"""
    return {name: make() for name, make in _banks().items()}


# ---- the GPU side -------------------------------------------------------------------------------------------------------

@pytest.fixture()
def switches(monkeypatch, oracle):
    monkeypatch.setenv("SAU_AMD_POISON", "1")
    monkeypatch.setenv("SAU_AMD_INNER_REPORT", "1")
    oracle.oracle().ora_set_fastmath_forms(ORACLE_FORMS)


def _length(prg, rate):
    return int(prg._prg.duration_ms * rate // 1000) + 1


# (stereo, frames per run: the whole script in one run, and runs that cut the groups elsewhere)
LEGS = ((False, None), (True, 70001), (True, None), (False, 70001))


def _both_forms(sa, oracle, capfd, monkeypatch, prg, what, rate=RATE, legs=LEGS, inner="all", loop=False):
    """Render `prg` in the lane-major and the row-major form, each leg against the oracle. inner: "all" -- every closed-form
    segment took the inner launch, in the form asked for; "some" -- some did and some went without it; "none" -- no segment took
    it, and each says that it lacked the 12-row build on wide tables. loop: whether the block loop had work (False: it must have had none, True: it must have had some, None: not looked at).
    -> the report's lines of the last render"""
    lines, log = [], []
    try:
        for stereo, chunk in legs:
            chunk = chunk or _length(prg, rate)
            want = oracle.oracle_render(prg.ptr, rate, stereo, chunk=chunk)
            assert len(want) > 0 and np.abs(want.astype(np.int32)).max() > 0, what
            for form in ("lane-major", "row-major"):
                if form == "row-major":
                    monkeypatch.setenv("SAU_AMD_NO_LANEMAJOR", "1")
                else:
                    monkeypatch.delenv("SAU_AMD_NO_LANEMAJOR", raising=False)
                capfd.readouterr()
                batch = sa.Batch([prg], rate)
                batch.set_timing(2)
                got = np.asarray(batch.render(stereo=stereo, chunk=chunk)[0]).reshape(-1)
                t = batch.timing_ex()
                batch.close()
                err = capfd.readouterr().err
                lines = INNER.findall(err)
                log.append("%s %s %s %d %s block_ms %.3f fast_ms %.3f" % (what, form, "stereo" if stereo else "mono", chunk,
                           {k: lines.count(k) for k in sorted(set(lines))}, t["block_ms"], t["fast_ms"]))
                if inner == "all":
                    assert set(lines) == {form}, (what, form, "the inner launch ran as", lines)
                elif inner == "some":
                    assert set(lines) == {form, "none"}, (what, form, "the inner launch ran as", lines)
                else:
                    why = NONE.findall(err)
                    assert lines and set(lines) == {"none"} and len(why) == len(lines), (what, form, lines)
                    assert all(rows != "12" or wide == "0" for rows, wide, _ in why), (what, form, why)
                assert len(got) == len(want), (what, form, len(got), len(want))
                d = np.flatnonzero(got != want)
                assert len(d) == 0, (f"{what} ({form}, {'stereo' if stereo else 'mono'}, {chunk}): {len(d)} samples differ, first at "
                                     f"{d[0]}: got {got[d[0]:d[0] + 4].tolist()} want {want[d[0]:d[0] + 4].tolist()}")
                if loop is False:
                    assert t["block_ms"] < 1.0 and t["fast_ms"] > 0, (what, form, t)
                elif loop:
                    assert t["block_ms"] > 0 and t["fast_ms"] > 0, (what, form, t)
    finally:
        print("\n".join(log))  # (every figure, shown with a failure or under -rA)
    return lines


def _prg(name):
    voices, ups = _banks()[name]()
    return vb.build_program(voices, updates=ups)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["big pm", "fpm", "noise", "amp op", "still", "amod", "wave tri", "wave saw", "wave sqr"])
def test_banks_on_the_default_path(sa, oracle, capfd, monkeypatch, switches, name):
    """Banks that reach the inner launch as the product runs them: PM across 2^20 cycles on the common and the general path,
    frequency-scaled PM below and across 2^20, N operators, the A operator and oscillators that stand still, amplitude lists and
    layered lists, and config 3's kind of bank on each discontinuous wave. Nothing is left to the block loop."""
    _both_forms(sa, oracle, capfd, monkeypatch, _prg(name), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["r", "amod ramps", "amp op ramps", "big pm ramps", "amod ramps cub"])
def test_banks_with_the_running_sum_builds_off(sa, oracle, capfd, monkeypatch, switches, name):
    """NO_SEQ legs: R operators and amplitude ramps make their segment one that may need running sums, which by default takes
    the builds that have them; with SAU_AMD_NO_SEQ the closed-form build takes the segment, and these voices -- whose phases
    are closed forms all the same -- are rendered by the inner launch: its R branch (both rate2x settings, with and without
    PM), its amplitude ramps of every shape but `cub` on oscillators, A operators and amplitude lines under a list (goals
    reached after a modulator's second, not reached on a carrier), the PM amplitudes of tests/test_gpu_range_guards.py as
    ramps across 2^20. Nothing of these is left to the block loop. "amod ramps cub": a tenth of the bank's ramps are `cub`
    ones, and a `cub` ramp in progress keeps its voice in the block loop by design while the reference build's loop tails are
    reproduced (k_analyze.h: the tail form's samples depend on where the reference's blocks end) -- measured: 5.3 ms of block
    loop beside the inner launch, which renders the other voices; the bank asserts that both ran."""
    monkeypatch.setenv("SAU_AMD_NO_SEQ", "1")
    _both_forms(sa, oracle, capfd, monkeypatch, _prg(name), name, loop=name.endswith("cub"))


@pytest.mark.gpu
@pytest.mark.parametrize("rate", [8000, 48000, 96000])
def test_a_mixed_bank_at_other_sample_rates(sa, oracle, capfd, monkeypatch, switches, rate):
    """voices of the default-path banks side by side at 8, 48 and 96 kHz (44.1 kHz: the banks themselves)"""
    _both_forms(sa, oracle, capfd, monkeypatch, _prg("mixed"), ("mixed", rate), rate=rate)


@pytest.mark.gpu
def test_later_events_cut_segments_of_many_lengths(sa, oracle, capfd, monkeypatch, switches):
    """events_bank: amplitude, frequency, phase and modulator-list events on different voices; the segments between them are
    closed-form ones of one table and one buffer throughout -- the long ones take the inner launch, the bursts' segments hold
    fewer than three tasks and go without it (the report has both kinds of line), and eight segments end 2 to 7 frames past a
    group boundary of some lead-in length."""
    lines = _both_forms(sa, oracle, capfd, monkeypatch, _prg("events"), "events", inner="some")
    assert lines.count("none") >= 6, lines


@pytest.mark.gpu
def test_hold_runs_handed_to_the_repair_pass_and_to_the_block_loop(sa, oracle, capfd, monkeypatch, switches):
    """Phase steps of zero that reach back to a group's first defined frame: without the repair pass (SAU_AMD_NO_REPAIR) every
    noted group of test_gpu_lanemajor.py's zero-step bank sends its voice to the block loop; voices with more than
    FAST_MAX_REPAIR noted groups go there with the pass on; and so do voices with a few noted groups of which one holds for
    longer than the pass stores (held_far). All exact, all with work for the block loop."""
    monkeypatch.setenv("SAU_AMD_NO_REPAIR", "1")
    _both_forms(sa, oracle, capfd, monkeypatch, _prg("zero steps"), "zero steps, no repair", loop=True)
    monkeypatch.delenv("SAU_AMD_NO_REPAIR")
    _both_forms(sa, oracle, capfd, monkeypatch, _prg("many holds"), "many holds", loop=True)
    _both_forms(sa, oracle, capfd, monkeypatch, _prg("far holds"), "far holds", loop=True)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["two buffers", "two waves", "frequency ramp", "red noise"])
def test_banks_that_must_not_take_the_inner_launch(sa, oracle, capfd, monkeypatch, switches, name):
    """Negative controls -- the report's assertion can fail: one voice with a second block buffer, one voice on another wave
    table, one modulator with a frequency ramp or one red-noise operator among voices that would take the inner launch, and the
    report has no line of it (exact all the same)."""
    _both_forms(sa, oracle, capfd, monkeypatch, _prg("not inner: " + name), name, legs=LEGS[:1], inner="none", loop=None)
