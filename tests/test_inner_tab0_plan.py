"""Which instantiation of the lane-major inner launch the planner gives a closed-form segment (saugns_amd/csrc/launch_plan.h:
plan_closed_form, FastPlan.inner_tab0), without a GPU: the one whose table address is the index alone (k_fast_voice.h: fk_entry's
TAB0) exactly for lane-major segments that stage ONE table -- whichever wave it is -- and never for two tables or more, the
row-major form or a segment without the inner launch. Through a hook library of its own, tests/hooks_inner_issue
(sauAmd_inner_tab0_plan); segments as in tests/test_inner_plan.py, on the banks tests/test_gpu_inner_issue.py renders on a GPU."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import ROOT
from saugns_amd import voicebank as vb
from test_gpu_inner_issue import _rewave, one_wave_bank, two_wave_bank
from test_gpu_lanemajor_regblock import LONG_MS, RATE, depth_bank, regblock_programs
from test_launch_plan import MI355X, SEG, segment_of

OUT = ("inner", "n_tabs", "inner_tab0", "n_fast", "rows", "inmix_flags")
INNER_NONE, INNER_ROW_MAJOR, INNER_LANE_MAJOR = 0, 1, 2


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    """The planner reads the switches from the environment: none set but what a test sets."""
    for name in list(os.environ):
        if name.startswith("SAU_AMD_"):
            monkeypatch.delenv(name)


@pytest.fixture(scope="module")
def tab0_hooks(hooks):
    """tests/hooks_inner_issue/libsaugns_amd_inner_issue_hooks.so: the product's object files (the `hooks` fixture has built
    them) + the hook"""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "hooks_inner_issue")])
    L = C.CDLL(os.path.join(ROOT, "tests", "hooks_inner_issue", "libsaugns_amd_inner_issue_hooks.so"))
    L.sauAmd_inner_tab0_plan.restype = C.c_int
    L.sauAmd_inner_tab0_plan.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
    return L


def tab0_plan(tab0_hooks, seg):
    row_stride = (seg["len"] + 63) & ~63
    vals = [int(seg[k]) for k in SEG] + [MI355X["lds"], MI355X["cus"], row_stride, 2 * row_stride, 0, seg["len"],
                                         -(-seg["n_voices"] // seg["n_streams"])]
    a = (C.c_uint32 * len(vals))(*vals)
    out = (C.c_uint32 * len(OUT))()
    assert tab0_hooks.sauAmd_inner_tab0_plan(a, len(vals), out, len(OUT)) == len(OUT)
    return dict(zip(OUT, list(out)))


def _segment(sa, seqexec, voices):
    prg = vb.build_program(voices)
    seg = segment_of(sa, seqexec, prg)
    seg["len"] = int(prg._prg.duration_ms * RATE // 1000) + 1
    return seg


@pytest.fixture(scope="module")
def segments(sa, seqexec):
    segs = {name: _segment(sa, seqexec, voices) for name, (voices, _) in regblock_programs().items()}
    segs["par"] = _segment(sa, seqexec, one_wave_bank(LONG_MS, "par"))
    segs["sin + par"] = _segment(sa, seqexec, two_wave_bank(LONG_MS))
    segs["three waves"] = _segment(sa, seqexec, [_rewave(op, ("sin", "tri", "saw")[i % 3]) for i, op in enumerate(depth_bank(LONG_MS))])
    return segs


def test_the_flag_is_set_exactly_for_lane_major_segments_of_one_table(tab0_hooks, segments, monkeypatch):
    """On an MI355X's LDS and on a budget that holds several wide tables beside 12 rows (SAU_AMD_LDS_LIMIT, a test switch)"""
    seen = set()
    for limit in (None, 512 * 1024):
        if limit:
            monkeypatch.setenv("SAU_AMD_LDS_LIMIT", str(limit))
        for name, seg in segments.items():
            p = tab0_plan(tab0_hooks, seg)
            assert p["inner_tab0"] == (1 if p["inner"] == INNER_LANE_MAJOR and p["n_tabs"] == 1 else 0), (name, limit, p)
            seen.add((p["inner"] == INNER_LANE_MAJOR, min(p["n_tabs"], 2), p["inner_tab0"]))
    # the banks cover the flag set, lane-major launches without it, and segments that are not lane-major
    assert (True, 1, 1) in seen and (True, 2, 0) in seen and any(not lm for lm, _, _ in seen), seen


def test_one_table_of_any_wave_two_tables_never(tab0_hooks, segments, monkeypatch):
    for name in ("depth %d ms" % LONG_MS, "par"):
        p = tab0_plan(tab0_hooks, segments[name])
        assert p["inner"] == INNER_LANE_MAJOR and p["n_tabs"] == 1 and p["inner_tab0"] == 1 and p["rows"] == 12, (name, p)
    # two wide tables leave an MI355X's 160 KiB no room for the 12-row build's edge launch: no inner launch at all
    p = tab0_plan(tab0_hooks, segments["sin + par"])
    assert p["inner"] == INNER_NONE and p["n_tabs"] == 2 and p["inner_tab0"] == 0, p
    # where they fit, the lane-major launch takes the form that adds the table's base: the table count is the rule, not the sizes
    monkeypatch.setenv("SAU_AMD_LDS_LIMIT", str(512 * 1024))
    for name, n in (("sin + par", 2), ("three waves", 3)):
        p = tab0_plan(tab0_hooks, segments[name])
        assert p["inner"] == INNER_LANE_MAJOR and p["n_tabs"] == n and p["inner_tab0"] == 0 and p["rows"] == 12, (name, p)
    p = tab0_plan(tab0_hooks, segments["par"])
    assert p["inner"] == INNER_LANE_MAJOR and p["n_tabs"] == 1 and p["inner_tab0"] == 1, p


def test_the_lane_major_launch_mixes_later_into_a_chunk(tab0_hooks, segments, monkeypatch):
    """With its round-10 forms its tasks are shorter, so the tasks that mix the chunk before start 15 sixteenths into a chunk
    (Tuning.inmix_at_lm), the other launches 13 (inmix_at); SAU_AMD_INMIX_AT sets both. inmix_flags bits 8-11, bit 5: the launch
    mixes. At config 3's step length and voice count: the launch mixes where its tasks come from the XCDs' queues."""
    seg = dict(segments["depth %d ms" % LONG_MS], len=441000, n_voices=1024)
    p = tab0_plan(tab0_hooks, seg)
    assert p["inner"] == INNER_LANE_MAJOR and p["inmix_flags"] & 32 and (p["inmix_flags"] >> 8) & 15 == 15, p
    monkeypatch.setenv("SAU_AMD_NO_LANEMAJOR", "1")
    p = tab0_plan(tab0_hooks, seg)
    assert p["inner"] == INNER_ROW_MAJOR and p["inmix_flags"] & 32 and (p["inmix_flags"] >> 8) & 15 == 13, p
    monkeypatch.delenv("SAU_AMD_NO_LANEMAJOR")
    monkeypatch.setenv("SAU_AMD_INMIX_AT", "11")
    assert (tab0_plan(tab0_hooks, seg)["inmix_flags"] >> 8) & 15 == 11


def test_not_for_the_row_major_form_nor_without_the_inner_launch(tab0_hooks, segments, monkeypatch):
    seg = segments["depth %d ms" % LONG_MS]
    assert tab0_plan(tab0_hooks, dict(seg, len=1440))["inner_tab0"] == 0  # (two tasks of row groups: no inner launch)
    monkeypatch.setenv("SAU_AMD_NO_LANEMAJOR", "1")
    p = tab0_plan(tab0_hooks, seg)
    assert p["inner"] == INNER_ROW_MAJOR and p["n_tabs"] == 1 and p["inner_tab0"] == 0, p
