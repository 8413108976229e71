"""The wave-only instantiation of the lane-major inner launch on the host's side, without a GPU:

  - SegmentDesc.wave_only (engine.cpp) -- "every active voice's operators are wave oscillators with constant amplitude" -- is
    never true of a segment whose decoded steps and operators do not have that shape. The steps and the operators' state are the
    sequential executor's own (tests/seqexec, taken into tests/hooks_inner_wonly with a look at every segment it is handed);
    the segments are drawn from the banks the GPU tests render, among them programs with later events, ramps, noise, R and A
    operators, amplitude lists, layered lists and pan ramps, run whole and in pieces.
  - the planner (launch_plan.h: plan_closed_form) gives FastPlan.inner_wonly exactly to lane-major segments with the flag, and
    SAU_AMD_NO_INNER_WONLY takes it away; the mixing point is the lane-major launch's either way.
  - the plan cache's key (plan.cpp: voice_plan_shape) differs wherever a voice's share of the flag does.
"""
import ctypes as C
import os
import subprocess

import pytest

from conftest import ROOT
from saugns_amd import voicebank as vb
from saugns_amd.api import POP_AMOD, POP_CAMOD, POP_PMOD
from test_gpu_lanemajor_ops import lanemajor_programs
from test_gpu_lanemajor_regblock import LONG_MS, RATE, _carrier, _sin, depth_bank, regblock_programs
from test_launch_plan import MI355X, SEG, segment_of

OUT = ("inner", "inner_wonly", "inner_tab0", "inmix_flags", "n_tabs")
COUNTS = ("segments", "flagged", "flagged_with_shape", "with_shape", "last_flag", "last_shape")
INNER_NONE, INNER_ROW_MAJOR, INNER_LANE_MAJOR = 0, 1, 2


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    """The planner reads the switches from the environment: none set but what a test sets."""
    for name in list(os.environ):
        if name.startswith("SAU_AMD_"):
            monkeypatch.delenv(name)


@pytest.fixture(scope="module")
def wonly_hooks(hooks):
    """tests/hooks_inner_wonly/libsaugns_amd_inner_wonly_hooks.so: the product's object files (the `hooks` fixture has built
    them) + the sequential executor + the hooks"""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "hooks_inner_wonly")])
    L = C.CDLL(os.path.join(ROOT, "tests", "hooks_inner_wonly", "libsaugns_amd_inner_wonly_hooks.so"))
    L.wonly_backend_create.restype = C.c_void_p
    L.wonly_backend_create.argtypes = [C.c_uint32]
    L.wonly_backend_counts.argtypes = [C.c_void_p, C.c_int]
    L.sauAmd_inner_wonly_plan.restype = C.c_int
    L.sauAmd_inner_wonly_plan.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
    L.sauAmd_wonly_key_probe.restype = C.c_int
    L.sauAmd_wonly_key_probe.argtypes = [C.c_uint32, C.c_void_p]
    return L


def _counts(L, reset=True):
    out = (C.c_uint32 * len(COUNTS))()
    L.wonly_backend_counts(out, 1 if reset else 0)
    return dict(zip(COUNTS, list(out)))


def _run(sa, L, prg, runs):
    """`prg` through the executor in runs of the given lengths -> the counts over its segments"""
    _counts(L)
    b = sa.Batch([prg], RATE, backend=L.wonly_backend_create(256))
    for n in runs:
        b.run(n, stereo=False, fetch=False)
    b.close()
    return _counts(L)


def wonly_plan(L, seg, wave_only):
    row_stride = (seg["len"] + 63) & ~63
    vals = [int(seg[k]) for k in SEG] + [MI355X["lds"], MI355X["cus"], row_stride, 2 * row_stride, 0, seg["len"],
                                         -(-seg["n_voices"] // seg["n_streams"]), 1 if wave_only else 0]
    a = (C.c_uint32 * len(vals))(*vals)
    out = (C.c_uint32 * len(OUT))()
    assert L.sauAmd_inner_wonly_plan(a, len(vals), out, len(OUT)) == len(OUT)
    return dict(zip(OUT, list(out)))


def odd_voices(ms=LONG_MS):
    """name -> a voice that keeps its bank from the wave-only instantiation (tests/test_gpu_inner_wonly.py renders them)"""
    from saugns_amd.api import POPT_AMP, POPT_NOISE, POPT_RASEG
    return {
        "amplitude ramp": _carrier(5, ms, {POP_PMOD: [_sin(2, 0.5)]}, amp=vb.Line(0.9, goal=0.2, shape="lin")),
        "modulator's amplitude ramp": _carrier(5, ms, {POP_PMOD: [vb.Op("sin", freq=vb.Line(2.0, ratio=True),
                                                                        amp=vb.Line(0.2, goal=0.7, shape="exp"))]}),
        "amplitude modulator": _carrier(5, ms, {POP_AMOD: [_sin(4.0, 0.3, ratio=False)]}, amp=0.6),
        "layered operator": _carrier(5, ms, {POP_PMOD: [_sin(2, 0.4), _sin(3, 0.2)]}),
        "noise operator": _carrier(5, ms, {POP_PMOD: [vb.Op(amp=0.1, op_type=POPT_NOISE, noise=0, seed=7)]}),
        "R operator": _carrier(5, ms, {POP_PMOD: [vb.Op(op_type=POPT_RASEG, ras=("lin", 0, 0), seed=99,
                                                       freq=vb.Line(2.0, ratio=True), amp=0.5)]}),
        "A operator": _carrier(5, ms, {POP_PMOD: [vb.Op(amp=0.3, op_type=POPT_AMP)]}),
        "line": _carrier(5, ms, {POP_PMOD: [_sin(2, 0.5)], POP_CAMOD: [_sin(3.0, 0.2, ratio=False)]}),
    }


def odd_bank(name, ms=LONG_MS, n=80):
    voices = depth_bank(ms, n)
    voices[5] = odd_voices(ms)[name]
    return voices


ODD = ("amplitude ramp", "modulator's amplitude ramp", "amplitude modulator", "layered operator", "noise operator",
       "R operator", "A operator", "line")


def test_plain_chains_have_the_flag_and_the_shape(sa, wonly_hooks):
    """depth 1 to 4 PM chains of sines, config 3's own voices: flagged, and the steps agree"""
    for voices in (depth_bank(LONG_MS), vb.config3_voices(64, 2)):
        c = _run(sa, wonly_hooks, vb.build_program(voices), (4096,))
        assert c["segments"] >= 1 and c["flagged"] == c["segments"] == c["flagged_with_shape"], c


@pytest.mark.parametrize("name", ODD)
def test_one_odd_voice_takes_the_flag_from_its_bank(sa, wonly_hooks, name):
    c = _run(sa, wonly_hooks, vb.build_program(odd_bank(name)), (4096, 4096))
    assert c["segments"] >= 2 and c["flagged"] == 0 and c["with_shape"] == 0, (name, c)


def test_the_flag_implies_the_shape_on_every_segment_drawn(sa, wonly_hooks):
    """Every program of the lane-major tests -- events that change amplitudes, frequencies, phases and lists, ramps of every
    shape, noise, A and R operators, amplitude lists, oscillators that stand still -- over its first segments, and the program
    with later events to its end: wherever the host sets the flag, the executor's steps and operators have the shape. Both
    sides occur, so the assertion is not empty."""
    total = dict.fromkeys(COUNTS, 0)
    programs = {name: vb.build_program(v, updates=u) for name, (v, u) in lanemajor_programs().items()}
    programs.update({"regblock " + name: vb.build_program(v) for name, (v, _) in regblock_programs().items()})
    for name, prg in programs.items():
        length = int(prg._prg.duration_ms * RATE // 1000) + 1
        # (the executor renders what it is handed: two short runs a program, and the one with later events to its end)
        runs = (30011,) * (length // 30011 + 1) if name == "events" else (4096, 3001)
        c = _run(sa, wonly_hooks, prg, runs)
        assert c["flagged"] == c["flagged_with_shape"], (name, c)
        for k in COUNTS[:4]:
            total[k] += c[k]
    assert total["flagged"] > 0 and total["segments"] > total["with_shape"] > 0, total
    print(total)


def test_a_ramp_once_given_keeps_the_flag_away_for_good(sa, wonly_hooks):
    """An event gives one modulator an amplitude sweep: flagged before it, and not after -- sticky per operator, as for the
    running-sum builds (the host does not follow a sweep to its end)."""
    voices = depth_bank(LONG_MS, 64)
    for v in voices:
        v.time_ms = LONG_MS
    m = voices[1].mods[POP_PMOD][0]
    ups = [(500, 1, m, {"amp": vb.Line(0.3, goal=0.6, shape="lin", state=False)})]
    prg = vb.build_program(voices, updates=ups)
    before = _run(sa, wonly_hooks, prg, (RATE // 2,))
    assert before["flagged"] == before["segments"] >= 1 and before["flagged_with_shape"] == before["flagged"], before
    _counts(wonly_hooks)
    b = sa.Batch([prg], RATE, backend=wonly_hooks.wonly_backend_create(256))
    b.run(RATE // 2, stereo=False, fetch=False)
    _counts(wonly_hooks)
    b.run(RATE, stereo=False, fetch=False)
    after = _counts(wonly_hooks)
    b.close()
    assert after["segments"] >= 1 and after["flagged"] == 0, after


@pytest.fixture(scope="module")
def segments(sa, seqexec):
    def seg_of(voices):
        prg = vb.build_program(voices)
        seg = segment_of(sa, seqexec, prg)
        seg["len"] = int(prg._prg.duration_ms * RATE // 1000) + 1
        return seg
    return {"depths": seg_of(depth_bank(LONG_MS)), "two buffers": seg_of(regblock_programs()["range amod"][0])}


def test_the_planner_gives_the_instantiation_to_lane_major_segments_with_the_flag(wonly_hooks, segments, monkeypatch):
    seg = segments["depths"]
    p = wonly_plan(wonly_hooks, seg, True)
    assert p["inner"] == INNER_LANE_MAJOR and p["inner_wonly"] == 1, p
    q = wonly_plan(wonly_hooks, seg, False)
    assert q["inner"] == INNER_LANE_MAJOR and q["inner_wonly"] == 0, q
    assert {k: v for k, v in p.items() if k != "inner_wonly"} == {k: v for k, v in q.items() if k != "inner_wonly"}
    # not without the lane-major launch: two buffers, too few tasks, the row-major form
    assert wonly_plan(wonly_hooks, segments["two buffers"], True)["inner_wonly"] == 0
    p = wonly_plan(wonly_hooks, dict(seg, len=1440), True)
    assert p["inner"] == INNER_NONE and p["inner_wonly"] == 0, p
    monkeypatch.setenv("SAU_AMD_NO_LANEMAJOR", "1")
    p = wonly_plan(wonly_hooks, seg, True)
    assert p["inner"] == INNER_ROW_MAJOR and p["inner_wonly"] == 0, p


def test_the_switch_restores_the_general_instantiation(wonly_hooks, segments, monkeypatch):
    seg = dict(segments["depths"], len=441000, n_voices=1024)
    on = wonly_plan(wonly_hooks, seg, True)
    assert on["inner"] == INNER_LANE_MAJOR and on["inner_wonly"] == 1 and on["inmix_flags"] & 32, on
    monkeypatch.setenv("SAU_AMD_NO_INNER_WONLY", "1")
    off = wonly_plan(wonly_hooks, seg, True)
    assert off["inner"] == INNER_LANE_MAJOR and off["inner_wonly"] == 0, off
    assert off["inmix_flags"] == wonly_plan(wonly_hooks, seg, False)["inmix_flags"], off


def test_forcing_the_flag_is_a_test_switch_of_its_own(wonly_hooks, segments, monkeypatch):
    """SAU_AMD_INNER_WONLY_FORCE (tests/test_gpu_inner_wonly.py: the kernel's guard) sets it on every lane-major segment"""
    monkeypatch.setenv("SAU_AMD_INNER_WONLY_FORCE", "1")
    assert wonly_plan(wonly_hooks, segments["depths"], False)["inner_wonly"] == 1
    assert wonly_plan(wonly_hooks, segments["two buffers"], False)["inner_wonly"] == 0


def test_the_plan_caches_key_changes_when_the_flag_does(wonly_hooks):
    """Voices that share a key share a compiled plan and with it the plan's share of the flag: the key must tell apart whatever
    the flag tells apart. A W carrier over one modulator, the modulator chosen nine ways (tests/hooks_inner_wonly)."""
    def probe(what):
        out = (C.c_ulonglong * 3)()
        assert wonly_hooks.sauAmd_wonly_key_probe(what, out) == 3, what
        return out[0], out[1]
    plain = probe(0)
    assert plain[1] == 1 and probe(0) == plain  # (the same voice: the same key)
    keys = {plain[0]}
    for what in range(1, 9):
        key, flag = probe(what)
        assert flag == 0, what
        assert key != plain[0], what
        keys.add(key)
    assert len(keys) == 9
