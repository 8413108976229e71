"""The lane-major inner launch with its block buffer in registers (k_fast_group_lm.h: `blk`, T values per lane, where the
row-major form keeps the block in LDS): banks that produce and consume the block in the ways a one-buffer segment can, against
the oracle, bit for bit, under SAU_AMD_POISON, in the lane-major and the row-major form (SAU_AMD_NO_LANEMAJOR), mono and stereo,
at 44.1 kHz. SAU_AMD_INNER_REPORT is asserted in every leg.

  - voices of chain depth 1, 2, 3 and 4 interleaved voice by voice: neighbouring waves run different step counts, each against
    its own registers; at the shortest lengths that take the launch and at one many groups longer, whole and in 70001-frame runs
  - a PM list of two modulators on one operator (the second is layered onto the first through the block: read-modify-write of
    `blk` in one step), alone and under a further PM level
  - the block in one role after another: an amplitude list on a phase modulator (the list's sum is consumed as amplitude, the
    product written back is the next operator's PM) and a frequency-scaled phase modulator over a PM chain
  - an amplitude list whose modulator has a PM chain of its own: the amplitude line waits in one block while the chain runs
    through another, so the plan has two buffers (plan.cpp; tests/test_inner_plan.py asserts the count) and the segment cannot
    take this launch -- rendered all the same, as a control
  - negative controls: `p[...]` beside `p.f[...]` on one operator and an `a.r[...]` list need two or three buffers; such a
    segment does not take the lane-major launch (launch_plan.h: plan_closed_form; tests/test_inner_plan.py has the rule on the
    CPU), and its PCM equals the oracle's all the same

regblock_programs() is shared with tests/test_inner_plan.py, which asks the planner about the same banks without a GPU."""
import re

import numpy as np
import pytest

from conftest import ORACLE_FORMS
from saugns_amd import voicebank as vb
from saugns_amd.api import POP_AMOD, POP_FPMOD, POP_PMOD, POP_RAMOD

RATE = 44100
INNER = re.compile(r"\[sau-amd\] inner: (lane-major|row-major|none)")
# The planner counts a segment's row groups as 720 frames each (launch_plan.h: row_groups at 12 rows) and gives the inner launch
# to segments of three tasks or more: 1441 frames are the least. 33 ms are 1456 frames -- the launch runs and finds no group
# between a voice's first and last; 50 ms are 2206 frames, three groups of 768 less the lead-in: one group each for the launch.
SHORT_MS = (33, 50)
LONG_MS = 2000  # 88201 frames: 116 groups a voice, two runs of 70001


def _sin(freq, amp, ratio=True, **kw):
    return vb.Op("sin", freq=vb.Line(float(freq), ratio=ratio), amp=amp, **kw)


def _carrier(i, ms, mods=None, spread=True, **kw):
    """voice i's carrier: a frequency and a pan of its own, and (spread) an end of its own"""
    return vb.Op("sin", freq=vb._num(".3f", 101.0 + 6.17 * i), time_ms=ms - (29 * (i % 17) if spread else 0),
                 pan=vb.Line(vb._num(".2f", ((i * 41) % 100) / 100.0)), mods=mods, **kw)


def depth_bank(ms, n=96):
    """voice i: a carrier over a PM chain of i mod 4 further operators -- depth 1 (no modulator), 2, 3, 4, voice by voice"""
    voices = []
    for i in range(n):
        op = None
        for d in range(i % 4):
            op = _sin(1 + (i + d) % 4, vb._num(".2f", 0.25 + 0.1 * ((i + 2 * d) % 6)), mods={POP_PMOD: [op]} if op else None)
        voices.append(_carrier(i, ms, {POP_PMOD: [op]} if op else None, spread=ms > 1000))
    return voices


def pm_pair_bank(ms=LONG_MS, n=88):
    """PM lists of two modulators on one operator: on the carrier; on a modulator, under the carrier's PM; on the carrier with
    a chain under the list's first member; and two levels down"""
    voices = []
    for i in range(n):
        a = _sin(1 + i % 3, vb._num(".2f", 0.3 + 0.1 * (i % 5)))
        b = _sin(vb._num(".2f", 2.5 + 0.7 * (i % 4)), vb._num(".2f", 0.15 + 0.05 * (i % 6)), ratio=False)
        kind = i % 4
        if kind == 0:
            mods = {POP_PMOD: [a, b]}
        elif kind == 1:
            mods = {POP_PMOD: [_sin(2, 0.5, mods={POP_PMOD: [a, b]})]}
        elif kind == 2:
            a.mods = {POP_PMOD: [_sin(3, 0.4)]}
            mods = {POP_PMOD: [a, b]}
        else:
            mods = {POP_PMOD: [_sin(1, 0.6, mods={POP_PMOD: [_sin(2, 0.4, mods={POP_PMOD: [a, b]})]})]}
        voices.append(_carrier(i, ms, mods))
    return voices


def roles_bank(ms=LONG_MS, n=84):
    """the one block as amplitude and as PM in turn: a phase modulator with an amplitude list of one or two members (the line and
    the members' samples summed in the block, read as the modulator's amplitude, its output written over them and read as the
    carrier's PM), the same one level down, and a frequency-scaled phase modulator over a PM chain"""
    voices = []
    for i in range(n):
        lf = lambda k: _sin(vb._num(".2f", 2.5 + 1.3 * k + 0.4 * (i % 5)), vb._num(".2f", 0.1 + 0.05 * ((i + k) % 4)), ratio=False)
        m = _sin(1 + i % 3, vb._num(".2f", 0.3 + 0.1 * (i % 4)), mods={POP_AMOD: [lf(0), lf(1)] if i % 2 else [lf(0)]})
        kind = i % 3
        if kind == 0:
            mods = {POP_PMOD: [m]}
        elif kind == 1:
            mods = {POP_PMOD: [_sin(2, 0.5, mods={POP_PMOD: [m]})]}
        else:
            mods = {POP_FPMOD: [_sin(2, vb._num(".4f", 0.001 * (1 + i % 4)), mods={POP_PMOD: [_sin(3, 0.4)]})]}
        voices.append(_carrier(i, ms, mods))
    return voices


def amod_over_pm_bank(ms=LONG_MS, n=80):
    """amplitude lists whose member has a PM chain of its own, one and two operators deep, on carriers and on a modulator; every
    fourth voice a plain chain. Two block buffers: the list's amplitude line is held while the chain is evaluated."""
    voices = []
    for i in range(n):
        chain = _sin(1 + i % 3, vb._num(".2f", 0.3 + 0.1 * (i % 4)))
        if i % 2:
            chain = _sin(2, 0.5, mods={POP_PMOD: [chain]})
        lf = _sin(vb._num(".2f", 3.0 + 0.9 * (i % 5)), vb._num(".2f", 0.2 + 0.05 * (i % 4)), ratio=False, mods={POP_PMOD: [chain]})
        kind = i % 4
        if kind in (0, 1):
            mods = {POP_AMOD: [lf]}
        elif kind == 2:
            mods = {POP_PMOD: [_sin(2, 0.5, mods={POP_AMOD: [lf]})]}
        else:
            mods = {POP_PMOD: [chain]}
        voices.append(_carrier(i, ms, mods, amp=vb._num(".2f", 0.4 + 0.1 * (i % 5))))
    return voices


def pm_beside_fpm_bank(ms=LONG_MS, n=80):
    """negative control: one voice with `p[...]` beside `p.f[...]` on its carrier among one-buffer voices"""
    voices = depth_bank(ms, n)
    voices[37] = _carrier(37, ms, {POP_PMOD: [_sin(2, 0.4)], POP_FPMOD: [_sin(3, 0.002)]})
    return voices


def range_amod_bank(ms=LONG_MS, n=80):
    """negative control: one voice with an `a.r[...]` list among one-buffer voices"""
    voices = depth_bank(ms, n)
    voices[52] = _carrier(52, ms, {POP_RAMOD: [_sin(4.0, 1.0, ratio=False)]}, amp=0.3, amp2=0.9)
    return voices


def regblock_programs():
    """name -> (voices, whether the segment takes the lane-major launch)"""
    banks = {"depth %d ms" % ms: (depth_bank(ms), True) for ms in SHORT_MS + (LONG_MS,)}
    banks["pm pair"] = (pm_pair_bank(), True)
    banks["roles"] = (roles_bank(), True)
    banks["amod over pm"] = (amod_over_pm_bank(), False)
    banks["pm beside fpm"] = (pm_beside_fpm_bank(), False)
    banks["range amod"] = (range_amod_bank(), False)
    return banks


# ---- the GPU side -------------------------------------------------------------------------------------------------------

@pytest.fixture()
def switches(monkeypatch, oracle):
    monkeypatch.setenv("SAU_AMD_POISON", "1")
    monkeypatch.setenv("SAU_AMD_INNER_REPORT", "1")
    oracle.oracle().ora_set_fastmath_forms(ORACLE_FORMS)


def _both_forms(sa, oracle, capfd, monkeypatch, prg, what, chunks=(None,), lane_major=True):
    """`prg` mono and stereo, each in the lane-major and the row-major form, against the oracle. lane_major: every segment took
    the inner launch in the form asked for; False: no segment's report says lane-major, whatever was asked for."""
    log = []
    length = int(prg._prg.duration_ms * RATE // 1000) + 1
    try:
        for chunk in chunks:
            chunk = chunk or length
            for stereo in (False, True):
                want = oracle.oracle_render(prg.ptr, RATE, stereo, chunk=chunk)
                assert len(want) > 0 and np.abs(want.astype(np.int32)).max() > 0, what
                for form in ("lane-major", "row-major"):
                    if form == "row-major":
                        monkeypatch.setenv("SAU_AMD_NO_LANEMAJOR", "1")
                    else:
                        monkeypatch.delenv("SAU_AMD_NO_LANEMAJOR", raising=False)
                    capfd.readouterr()
                    batch = sa.Batch([prg], RATE)
                    batch.set_timing(2)
                    got = np.asarray(batch.render(stereo=stereo, chunk=chunk)[0]).reshape(-1)
                    t = batch.timing_ex()
                    batch.close()
                    lines = INNER.findall(capfd.readouterr().err)
                    log.append("%s %s %s %d %s block_ms %.3f fast_ms %.3f" % (what, form, "stereo" if stereo else "mono", chunk,
                               {k: lines.count(k) for k in sorted(set(lines))}, t["block_ms"], t["fast_ms"]))
                    if lane_major:
                        assert set(lines) == {form}, (what, form, "the inner launch ran as", lines)
                        assert t["block_ms"] < 1.0 and t["fast_ms"] > 0, (what, form, t)  # (nothing went to the block loop)
                    else:
                        assert lines and "lane-major" not in lines, (what, form, "the inner launch ran as", lines)
                    assert len(got) == len(want), (what, form, len(got), len(want))
                    d = np.flatnonzero(got != want)
                    assert len(d) == 0, (f"{what} ({form}, {'stereo' if stereo else 'mono'}, {chunk}): {len(d)} samples differ, "
                                         f"first at {d[0]}: got {got[d[0]:d[0] + 4].tolist()} want {want[d[0]:d[0] + 4].tolist()}")
    finally:
        print("\n".join(log))  # (every figure, shown with a failure or under -rA)


def _prg(name):
    return vb.build_program(regblock_programs()[name][0])


@pytest.mark.gpu
@pytest.mark.parametrize("ms", SHORT_MS)
def test_chain_depths_side_by_side_at_the_shortest_lengths(sa, oracle, capfd, monkeypatch, switches, ms):
    """Depth 1 to 4 voice by voice in segments of three tasks of row groups, the least the launch takes: at 1456 frames it runs
    and has no group of its own, at 2206 one group a voice."""
    _both_forms(sa, oracle, capfd, monkeypatch, _prg("depth %d ms" % ms), ("depths", ms))


@pytest.mark.gpu
def test_chain_depths_side_by_side(sa, oracle, capfd, monkeypatch, switches):
    """... and over 116 groups a voice, ends at different frames, in one run and in runs of 70001 frames"""
    _both_forms(sa, oracle, capfd, monkeypatch, _prg("depth %d ms" % LONG_MS), "depths", chunks=(None, 70001))


@pytest.mark.gpu
def test_two_phase_modulators_on_one_operator(sa, oracle, capfd, monkeypatch, switches):
    """The list's second member adds its samples onto the first's in the block (SF_LAYER: `blk` read and written in one step):
    on a carrier, under a further PM level and two, and with a chain under the first member."""
    _both_forms(sa, oracle, capfd, monkeypatch, _prg("pm pair"), "pm pair")


@pytest.mark.gpu
def test_the_block_as_amplitude_and_as_pm_in_turn(sa, oracle, capfd, monkeypatch, switches):
    """An amplitude list on a phase modulator: the registers hold the list's sum, are read as amplitude, take the modulator's
    output and are read as PM by the next step; and a chain's output read as frequency-scaled PM."""
    _both_forms(sa, oracle, capfd, monkeypatch, _prg("roles"), "roles")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["pm beside fpm", "range amod", "amod over pm"])
def test_segments_of_two_buffers_do_not_take_the_lane_major_launch(sa, oracle, capfd, monkeypatch, switches, name):
    """Negative controls: one voice that needs a second block (PM beside frequency-scaled PM; a range list's blend) among voices
    that would take the launch, and a bank of amplitude lists over PM chains (two buffers a voice). The report has no
    lane-major line, asked for or not, and the PCM is the oracle's."""
    _both_forms(sa, oracle, capfd, monkeypatch, _prg(name), name, lane_major=False)
