"""The round-10 forms of the lane-major inner launch's wave oscillator (k_fast_group_lm.h, k_fast_voice.h: FK_LM_ONE_PHASE_SET,
FK_LM_TAB0, FK_LM_AHEAD): a sample's differentiator right behind its polynomial, the instantiation for launches of
one table, and the table gathers issued a pair of samples ahead. Integer identities and instruction order only, so every leg is
compared with the oracle bit for bit, mono and stereo, under SAU_AMD_POISON, and every leg asserts the SAU_AMD_INNER_REPORT line,
which since round 10 ends in the launch's table count and `, tab0` where the one-table instantiation ran.

By default (a) and (c) are on and (b) is off (within noise on config 3). Every leg runs in three builds: the default one -- the
one phase set and the ordered gathers in the form that adds the table's base; a library with all three macros at 0, the forms
before round 10; and a library with FK_LM_TAB0=1 beside the defaults, the one-table instantiation. The two libraries are built by
`python saugns_amd/build.py --variant` in the set-up; where one cannot be built, its legs are skipped.

  1  depth_bank, 96 voices, 50 ms: one inner group a voice, the least that runs the loop
  2  the same bank at 2000 ms, whole and in runs of 70001 frames: chain depths 1-4 voice by voice, so the unmodulated branch and
     the PM branch run in neighbouring waves
  3  the same bank on one wave that is not the sine: a single table that is not table 0 of the set -- still the one-table launch
  4  voices on two different waves: two tables. This leg checks the planner's refusal only, and runs none of the inner kernel:
     two wide tables leave an MI355X's 160 KiB of LDS no room for the 12-row build, so the report is `inner: none` in every build
     (tests/test_inner_tab0_plan.py has the rule for budgets where the launch fits: lane-major, never the one-table form). The
     form that adds the table's base with the round-10 forms runs in legs 1, 2, 3 and 5 of the default build.
  5  a zero-frequency modulator (every phase step of it is zero) and a phase modulator of amplitude 2^21 (|pm| >= 2^20): the two
     exits that leave the common path after the phases are final, for the general path
"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ORACLE_FORMS, ROOT
from saugns_amd import voicebank as vb
from saugns_amd.api import POP_PMOD
from test_gpu_lanemajor_regblock import LONG_MS, RATE, _carrier, _sin, depth_bank

REPORT = re.compile(r"\[sau-amd\] inner: (lane-major|row-major|none)[^\n]*?, (\d+) voices(?:, (\d+) tables(, tab0)?)?")
VARIANTS = {"parent": ("r10parent", ("FK_LM_ONE_PHASE_SET=0", "FK_LM_TAB0=0", "FK_LM_AHEAD=0")),
            "tab0": ("r10tab0", ("FK_LM_TAB0=1",))}


def _rewave(op, wave):
    op.wave = wave(op) if callable(wave) else wave
    for ops in op.mods.values():
        for m in ops:
            _rewave(m, wave)
    return op


def one_wave_bank(ms, wave):
    return [_rewave(op, wave) for op in depth_bank(ms)]


def two_wave_bank(ms):
    """voice i's operators: the sine where i is even, the parabola where it is odd -- two tables staged, every voice one"""
    return [_rewave(op, "par" if i % 2 else "sin") for i, op in enumerate(depth_bank(ms))]


def exits_bank(ms):
    """depth_bank with, every eighth voice, a 0 Hz modulator under the carrier (constant phase: every step of it is zero, and
    its output holds), and every eighth other voice a modulator of amplitude 2^21 (|pm| >= 2^20: the wrapping form of the offset)"""
    voices = depth_bank(ms)
    for i in range(0, len(voices), 8):
        voices[i] = _carrier(i, ms, {POP_PMOD: [_sin(0.0, 0.5, ratio=False, phase=0.13)]})
        voices[i + 4] = _carrier(i + 4, ms, {POP_PMOD: [_sin(2, float(1 << 21))]})
    return voices


@pytest.fixture(scope="module")
def variant_libs(sa, tables):
    """build -> saugns_amd/variants/lib_<name>.so loaded, or the reason it is not there. Stale ones (a source is newer) are rebuilt,
    side by side."""
    csrc = os.path.join(ROOT, "saugns_amd", "csrc")
    deps = [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".h", ".hip", ".cpp"))] + \
        [os.path.join(ROOT, "saugns_amd", "build.py")]
    paths = {b: os.path.join(ROOT, "saugns_amd", "variants", "lib_%s.so" % n) for b, (n, _) in VARIANTS.items()}
    stale = [b for b, p in paths.items() if not os.path.exists(p) or any(os.path.getmtime(d) > os.path.getmtime(p) for d in deps)]
    if stale:
        sa.build()  # (once, ahead of the variants: each of them starts with it)
    procs = {b: subprocess.Popen([sys.executable, os.path.join(ROOT, "saugns_amd", "build.py"), "--variant", VARIANTS[b][0]] +
                                 list(VARIANTS[b][1]), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for b in stale}
    libs = {}
    for b, p in paths.items():
        out = procs[b].communicate()[0] if b in procs else ""
        if (b in procs and procs[b].returncode != 0) or not os.path.exists(p):
            libs[b] = "the variant library %s could not be built: %s" % (VARIANTS[b][0], out[-400:])
            continue
        libs[b] = sa.api._declare(C.CDLL(p))
        libs[b].sauAmd_set_piluts(np.ascontiguousarray(tables, dtype=np.float32).ctypes.data)
    return libs


@pytest.fixture()
def switches(monkeypatch, oracle):
    monkeypatch.setenv("SAU_AMD_POISON", "1")
    monkeypatch.setenv("SAU_AMD_INNER_REPORT", "1")
    oracle.oracle().ora_set_fastmath_forms(ORACLE_FORMS)


_WANT = {}  # (leg, stereo, chunk) -> the oracle's PCM: computed once, shared by the two builds' legs, never written to


def _leg(sa, oracle, capfd, monkeypatch, build, lib, key, voices, chunks=(None,), tables=1):
    """`voices` mono and stereo against the oracle; every segment's report: lane-major, `tables` tables, and the one-table
    instantiation exactly where the build has it and the launch has one table"""
    if lib is not None:
        monkeypatch.setattr(sa.api, "_lib", lib)
    prg = vb.build_program(voices)
    length = int(prg._prg.duration_ms * RATE // 1000) + 1
    log = []
    try:
        for chunk in chunks:
            chunk = chunk or length
            for stereo in (False, True):
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
                log.append("%s %s %s %d %s block_ms %.3f fast_ms %.3f" % (key, build, "stereo" if stereo else "mono", chunk,
                           sorted(set(lines)), t["block_ms"], t["fast_ms"]))
                tab0 = ", tab0" if build == "tab0" and tables == 1 else ""
                if tables == 1:
                    assert lines and {(f, n, t0) for f, _, n, t0 in lines} == {("lane-major", "1", tab0)}, (key, build, lines)
                else:  # (no inner launch on this LDS: the planner's refusal; were there one, never the one-table form)
                    assert lines and all(t0 == "" and (f == "none" or n == str(tables)) for f, _, n, t0 in lines), (key, build, lines)
                assert len(got) == len(want), (key, build, len(got), len(want))
                d = np.flatnonzero(got != want)
                assert len(d) == 0, (f"{key} ({build}, {'stereo' if stereo else 'mono'}, {chunk}): {len(d)} samples differ, "
                                     f"first at {d[0]}: got {got[d[0]:d[0] + 4].tolist()} want {want[d[0]:d[0] + 4].tolist()}")
    finally:
        prg = None  # (freed by the library that made it)
        print("\n".join(log))  # (every figure, shown with a failure or under -rA)


def _variant(request, build):
    if build == "default":
        return None
    lib = request.getfixturevalue("variant_libs")[build]
    if isinstance(lib, str):
        pytest.skip(lib)
    return lib


BUILDS = pytest.mark.parametrize("build", ["default", "parent", "tab0"])


@pytest.mark.gpu
@BUILDS
def test_one_inner_group_a_voice(sa, oracle, capfd, monkeypatch, switches, request, build):
    _leg(sa, oracle, capfd, monkeypatch, build, _variant(request, build), "depths 50 ms", depth_bank(50))


@pytest.mark.gpu
@BUILDS
def test_chain_depths_side_by_side_whole_and_in_runs(sa, oracle, capfd, monkeypatch, switches, request, build):
    _leg(sa, oracle, capfd, monkeypatch, build, _variant(request, build), "depths", depth_bank(LONG_MS), chunks=(None, 70001))


@pytest.mark.gpu
@BUILDS
def test_one_table_that_is_not_the_sets_first(sa, oracle, capfd, monkeypatch, switches, request, build):
    """every operator on the parabola: wave 7 of the set, the launch's table 0"""
    _leg(sa, oracle, capfd, monkeypatch, build, _variant(request, build), "par", one_wave_bank(LONG_MS, "par"))


@pytest.mark.gpu
@BUILDS
def test_two_tables_take_no_inner_launch_on_this_lds(sa, oracle, capfd, monkeypatch, switches, request, build):
    _leg(sa, oracle, capfd, monkeypatch, build, _variant(request, build), "sin + par", two_wave_bank(LONG_MS), tables=2)


@pytest.mark.gpu
@BUILDS
def test_zero_steps_and_big_offsets_leave_for_the_general_path(sa, oracle, capfd, monkeypatch, switches, request, build):
    _leg(sa, oracle, capfd, monkeypatch, build, _variant(request, build), "exits", exits_bank(LONG_MS))
