"""The wave-only instantiation of the lane-major inner launch (k_fast_voice.h: fast_kernel's WONLY; k_fast_group_lm.h; DESIGN.md
4.1): banks of wave oscillators with constant amplitude, the only thing it holds, against the oracle bit for bit, int16 (mono
and stereo) and float, under SAU_AMD_POISON. SAU_AMD_INNER_REPORT's line ends in `, wonly` where the instantiation ran, and
every leg asserts it. Banks of 80 to 96 voices and 2 to 4 s: over a hundred row groups a voice, a dozen tasks or more. On a
full grid such a bank's tasks go out in fixed strides and the mixer does all the mixing; leg 0 runs the launch on 16 workgroups
(SAU_AMD_FK_GRID, as tests/test_gpu_inmix.py does), where the tasks come from the XCDs' queues and the launch mixes tiles itself.

Legs that take it:
  0  the launch that mixes: config 3's own voices (one depth, so every voice's row groups are cut at the same frames and
     premix_kernel lets the launch mix), 96 of them x 4 s with pans of their own, on 16 workgroups. SAU_AMD_INMIX_REPORT says the
     launch mixed tiles (tiles > 0, both guards 0), the inner report says `, wonly`; mono and stereo int16 against the oracle,
     and the whole length in float, mono and stereo (a float run's launch mixes nothing: mix_kernel_f32 writes every frame)
  1  PM chains 0 to 4 modulators deep, voice by voice (neighbouring waves run different step counts; the voices without a
     modulator have an unmodulated carrier and nothing else), ends at different frames, whole and in runs of 70001 frames. A
     group starts at frame cg (768 - H) - H, H the chain's lead-in: with H odd no multiple of four (dword stores), with H a
     multiple of four every group (16-byte stores) -- depths 0 to 4 hold both.
  2  a modulator of zero increment under PM of its own (every phase step of it is its PM's), a modulator of zero increment
     and no PM (its output stands still: the constant source of k_decode.h), and PM of amplitude 2^21 (|pm| >= 2^20: the general
     path's wrapping offsets) -- tests/test_gpu_inner_issue.py's exits bank and tests/test_gpu_lanemajor_ops.py's still bank
  3  phase steps of zero on defined frames (tests/test_gpu_lanemajor.py's zero-step bank): holds, and the notes for the repair
     pass
  4  the same as 1 with SAU_AMD_NO_INNER_WONLY: the general instantiation, no `, wonly`

Legs that must not: the depth bank with ONE voice changed -- an amplitude ramp on a carrier or on a modulator, an amplitude
modulator, a layered operator (a second phase modulator), an N, an R or an A operator, a line (a pan modulator: a line step and
ST_VOICE). No segment's report says `, wonly` (tests/test_inner_wonly_plan.py has the rule on the CPU), the PCM is the oracle's,
and -- where the bank still takes the lane-major launch -- nothing goes to the block loop. With SAU_AMD_NO_SEQ the ramp and the R
bank reach the lane-major launch too, in the general instantiation.

The kernel's guard: SAU_AMD_INNER_WONLY_FORCE (a test switch) gives the instantiation to every lane-major segment. The odd
voice's step is not of the shape, its wave says so in one scalar test, the voice goes to the block loop (its kernel time shows
it) and the PCM is still the oracle's. The A operator is the exception: its step is the constant source the instantiation keeps
for W operators that stand still, so the forced launch renders it itself -- the host all the same does not flag a bank with one."""
import re

import numpy as np
import pytest

from conftest import ORACLE_FORMS
from saugns_amd import voicebank as vb
from saugns_amd.api import POP_PMOD
from test_gpu_f32_oracle import check_batch
from test_gpu_inner_issue import exits_bank
from test_gpu_lanemajor_ops import still_bank, zero_step_bank
from test_gpu_lanemajor_regblock import RATE, _carrier, _sin
from test_inner_wonly_plan import ODD, odd_bank

MS = 2000
REPORT = re.compile(r"\[sau-amd\] inner: (lane-major|row-major|none)[^\n]*?, (\d+) voices(?:, (\d+) tables(, tab0|, wonly)?)?")
# which odd banks still take the lane-major launch as the product runs them (one buffer, no running sums)
ODD_LANE_MAJOR = {"amplitude modulator", "layered operator", "noise operator", "A operator"}
ODD_NO_SEQ = {"amplitude ramp", "modulator's amplitude ramp", "R operator"}
# Whether the block loop had a voice to render, from its kernel time: with nothing on its list the launch returns at once (a few
# microseconds), and one voice of 88200 frames, rendered by a single workgroup block after block, takes a millisecond or more:
# 0.5 ms, the lower of the bounds the other lane-major tests draw between the two, leaves the idle launch a factor of fifty.
BLOCK_IDLE_MS = 0.5
INMIX = re.compile(r"inmix: voices (\d+) frames (\d+) chunks (\d+) x (\d+) frames, tiles (\d+) of (\d+), chunks mixed whole (\d+), guard (\d+) (\d+)")


def deep_bank(ms=MS, n=95):
    """voice i: a carrier over a PM chain of i mod 5 operators -- none (an unmodulated carrier) to four"""
    voices = []
    for i in range(n):
        op = None
        for d in range(i % 5):
            op = _sin(1 + (i + d) % 4, vb._num(".2f", 0.25 + 0.1 * ((i + 2 * d) % 6)), mods={POP_PMOD: [op]} if op else None)
        voices.append(_carrier(i, ms, {POP_PMOD: [op]} if op else None))
    return voices


@pytest.fixture()
def switches(monkeypatch, oracle):
    monkeypatch.setenv("SAU_AMD_POISON", "1")
    monkeypatch.setenv("SAU_AMD_INNER_REPORT", "1")
    oracle.oracle().ora_set_fastmath_forms(ORACLE_FORMS)


_WANT = {}  # (key, stereo, chunk) -> the oracle's PCM: computed once, shared by the legs of a bank, never written to


def _render(sa, oracle, capfd, key, prg, stereo, chunk=None):
    """-> (the report's lines, block_ms) of one int16 render of `prg`, compared with the oracle's"""
    length = int(prg._prg.duration_ms * RATE // 1000) + 1
    chunk = chunk or length
    if (key, stereo, chunk) not in _WANT:
        want = oracle.oracle_render(prg.ptr, RATE, stereo, chunk=chunk)
        want.setflags(write=False)
        _WANT[(key, stereo, chunk)] = want
    want = _WANT[(key, stereo, chunk)]
    assert len(want) > 0 and np.abs(want.astype(np.int32)).max() > 0, key
    capfd.readouterr()
    batch = sa.Batch([prg], RATE)
    batch.set_timing(2)
    got = np.asarray(batch.render(stereo=stereo, chunk=chunk)[0]).reshape(-1)
    t = batch.timing_ex()
    batch.close()
    lines = REPORT.findall(capfd.readouterr().err)
    print(key, "stereo" if stereo else "mono", chunk, sorted(set(lines)), "block_ms %.3f fast_ms %.3f" % (t["block_ms"], t["fast_ms"]))
    assert len(got) == len(want), (key, len(got), len(want))
    d = np.flatnonzero(got != want)
    assert len(d) == 0, (f"{key} ({'stereo' if stereo else 'mono'}, {chunk}): {len(d)} samples differ, first at {d[0]}: "
                         f"got {got[d[0]:d[0] + 4].tolist()} want {want[d[0]:d[0] + 4].tolist()}")
    return lines, t


def _took_it(lines, key):
    assert lines and {(f, n, w) for f, _, n, w in lines} == {("lane-major", "1", ", wonly")}, (key, lines)


def _float_leg(sa, oracle, capfd, key, prg, want_wonly, whole=False):
    """the first run of 70001 stereo float frames against the float oracle -- whole: every run of the script's length, stereo and
    mono -- and what the report says of it"""
    for stereo in ((True, False) if whole else (True,)):
        capfd.readouterr()
        check_batch(sa, oracle, [prg], RATE, stereo, 70001, key, max_calls=0 if whole else 1)
        lines = REPORT.findall(capfd.readouterr().err)
        assert lines and all((w == ", wonly") == want_wonly for _, _, _, w in lines), (key, stereo, lines)


@pytest.mark.gpu
def test_the_launch_that_mixes_its_own_tiles(sa, oracle, capfd, monkeypatch, switches):
    monkeypatch.setenv("SAU_AMD_FK_GRID", "16")
    monkeypatch.setenv("SAU_AMD_INMIX_REPORT", "1")
    voices = vb.config3_voices(96, 4)
    for i, v in enumerate(voices):
        v.pan = vb.Line(vb._num(".2f", ((i * 37) % 100) / 100.0))
    prg = vb.build_program(voices)
    for stereo in (False, True):
        want = oracle.oracle_render(prg.ptr, RATE, stereo, chunk=176400)
        capfd.readouterr()
        batch = sa.Batch([prg], RATE)
        got = np.array(batch.run(176400, stereo=stereo)[0][0], copy=True).reshape(-1)[:len(want)]
        batch.close()
        err = capfd.readouterr().err
        lines = REPORT.findall(err)
        mixed = [tuple(int(x) for x in m.groups()) for m in INMIX.finditer(err)]
        print("stereo" if stereo else "mono", lines, mixed)
        _took_it(lines, "mixing")
        assert mixed and mixed[0][0] == 96 and mixed[0][4] > 0 and mixed[0][7] == 0 and mixed[0][8] == 0, mixed
        d = np.flatnonzero(got != want)
        assert len(got) == len(want) and len(d) == 0, (stereo, len(d), d[:4])
    monkeypatch.delenv("SAU_AMD_INMIX_REPORT")
    _float_leg(sa, oracle, capfd, "mixing f32", prg, True, whole=True)


@pytest.mark.gpu
def test_chains_of_every_depth_side_by_side(sa, oracle, capfd, switches):
    prg = vb.build_program(deep_bank())
    for stereo, chunk in ((False, None), (True, None), (True, 70001)):
        lines, t = _render(sa, oracle, capfd, "deep", prg, stereo, chunk)
        _took_it(lines, "deep")
        assert t["block_ms"] < BLOCK_IDLE_MS and t["fast_ms"] > 0, ("deep", t)  # (nothing went to the block loop)
    _float_leg(sa, oracle, capfd, "deep f32", prg, True)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["exits", "still"])
def test_zero_increments_and_big_offsets(sa, oracle, capfd, switches, name):
    prg = vb.build_program(exits_bank(MS) if name == "exits" else still_bank(80, MS))
    for stereo in (False, True):
        lines, t = _render(sa, oracle, capfd, name, prg, stereo)
        _took_it(lines, name)
        assert t["block_ms"] < BLOCK_IDLE_MS and t["fast_ms"] > 0, (name, t)
    _float_leg(sa, oracle, capfd, name + " f32", prg, True)


@pytest.mark.gpu
def test_phase_steps_of_zero_hold_and_are_repaired(sa, oracle, capfd, switches):
    prg = vb.build_program(zero_step_bank(96, 2500))
    for stereo in (False, True):
        lines, _ = _render(sa, oracle, capfd, "zero steps", prg, stereo)
        _took_it(lines, "zero steps")
    _float_leg(sa, oracle, capfd, "zero steps f32", prg, True)


@pytest.mark.gpu
def test_the_switch_restores_the_general_instantiation(sa, oracle, capfd, monkeypatch, switches):
    monkeypatch.setenv("SAU_AMD_NO_INNER_WONLY", "1")
    prg = vb.build_program(deep_bank())
    for stereo in (False, True):
        lines, t = _render(sa, oracle, capfd, "deep", prg, stereo)
        assert lines and {(f, n, w) for f, _, n, w in lines} == {("lane-major", "1", "")}, lines
        assert t["block_ms"] < BLOCK_IDLE_MS and t["fast_ms"] > 0, t


@pytest.mark.gpu
@pytest.mark.parametrize("name", ODD)
def test_one_odd_voice_keeps_its_bank_from_it(sa, oracle, capfd, monkeypatch, switches, name):
    prg = vb.build_program(odd_bank(name, MS))
    for stereo in (False, True):
        lines, t = _render(sa, oracle, capfd, name, prg, stereo)
        assert lines and all(w != ", wonly" for _, _, _, w in lines), (name, lines)
        if name in ODD_LANE_MAJOR:
            assert {f for f, _, _, _ in lines} == {"lane-major"}, (name, lines)
            assert t["block_ms"] < BLOCK_IDLE_MS and t["fast_ms"] > 0, (name, t)
        else:
            assert "lane-major" not in {f for f, _, _, _ in lines}, (name, lines)
    if name in ODD_LANE_MAJOR:
        _float_leg(sa, oracle, capfd, name + " f32", prg, False)
    if name in ODD_NO_SEQ:  # (the closed-form build takes the segment: the lane-major launch, in the general instantiation)
        monkeypatch.setenv("SAU_AMD_NO_SEQ", "1")
        lines, t = _render(sa, oracle, capfd, name, prg, True)
        assert lines and {(f, w) for f, _, _, w in lines} == {("lane-major", "")}, (name, lines)
        assert t["block_ms"] < BLOCK_IDLE_MS and t["fast_ms"] > 0, (name, t)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(ODD_LANE_MAJOR))
def test_the_kernels_guard_sends_an_odd_voice_to_the_block_loop(sa, oracle, capfd, monkeypatch, switches, name):
    monkeypatch.setenv("SAU_AMD_INNER_WONLY_FORCE", "1")
    prg = vb.build_program(odd_bank(name, MS))
    for stereo in (False, True):
        lines, t = _render(sa, oracle, capfd, name, prg, stereo)
        _took_it(lines, name)
        if name == "A operator":  # (the constant source the instantiation keeps for W operators that stand still serves it)
            assert t["block_ms"] < BLOCK_IDLE_MS and t["fast_ms"] > 0, (name, t)
        else:
            assert t["block_ms"] > BLOCK_IDLE_MS and t["fast_ms"] > 0, (name, t)


@pytest.mark.gpu
def test_the_guard_on_ramps_and_r_operators(sa, oracle, capfd, monkeypatch, switches):
    """... and on the shapes that reach the lane-major launch only with the running-sum builds off"""
    monkeypatch.setenv("SAU_AMD_INNER_WONLY_FORCE", "1")
    monkeypatch.setenv("SAU_AMD_NO_SEQ", "1")
    for name in sorted(ODD_NO_SEQ):
        prg = vb.build_program(odd_bank(name, MS))
        lines, t = _render(sa, oracle, capfd, name, prg, True)
        _took_it(lines, name)
        assert t["block_ms"] > BLOCK_IDLE_MS and t["fast_ms"] > 0, (name, t)
