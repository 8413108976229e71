"""The inner launch of a closed-form segment as the planner decides it (saugns_amd/csrc/launch_plan.h: plan_closed_form,
FastPlan::inner_lds), without a GPU. The lane-major form keeps its block buffer in registers, so it is given only to segments
whose voices share exactly ONE buffer, and its launch asks for the table blocks' LDS and nothing else.
Through a hook library of its own, tests/hooks_plan (sauAmd_inner_plan); segments come from the sequential test backend, as in
tests/test_launch_plan.py, on the banks tests/test_gpu_lanemajor_regblock.py renders on a GPU."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import ROOT
from saugns_amd import voicebank as vb
from test_gpu_lanemajor_regblock import RATE, regblock_programs
from test_launch_plan import MI355X, SEG, segment_of

OUT = ("use_fast", "main_build", "rows", "wide_cf", "n_fast", "n_tabs", "inner", "dyn_chunks", "inner_lds", "lds_12_wide",
       "tab_bytes_wide", "lds_limit")
INNER_NONE, INNER_ROW_MAJOR, INNER_LANE_MAJOR = 0, 1, 2


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    """The planner reads the switches from the environment: none set but what a test sets."""
    for name in list(os.environ):
        if name.startswith("SAU_AMD_"):
            monkeypatch.delenv(name)


@pytest.fixture(scope="module")
def plan_hooks(hooks):
    """tests/hooks_plan/libsaugns_amd_plan_hooks.so: the product's object files (the `hooks` fixture has built them) + the hook"""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "hooks_plan")])
    L = C.CDLL(os.path.join(ROOT, "tests", "hooks_plan", "libsaugns_amd_plan_hooks.so"))
    L.sauAmd_inner_plan.restype = C.c_int
    L.sauAmd_inner_plan.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
    return L


def inner_plan(plan_hooks, seg):
    row_stride = (seg["len"] + 63) & ~63
    vals = [int(seg[k]) for k in SEG] + [MI355X["lds"], MI355X["cus"], row_stride, 2 * row_stride, 0, seg["len"],
                                         -(-seg["n_voices"] // seg["n_streams"])]
    a = (C.c_uint32 * len(vals))(*vals)
    out = (C.c_uint32 * len(OUT))()
    assert plan_hooks.sauAmd_inner_plan(a, len(vals), out, len(OUT)) == len(OUT)
    return dict(zip(OUT, list(out)))


@pytest.fixture(scope="module")
def segments(sa, seqexec):
    """name -> (the bank's segment at its script's length, whether it is to take the lane-major launch)"""
    segs = {}
    for name, (voices, lm) in regblock_programs().items():
        prg = vb.build_program(voices)
        seg = segment_of(sa, seqexec, prg)
        seg["len"] = int(prg._prg.duration_ms * RATE // 1000) + 1
        segs[name] = (seg, lm)
    return segs


def test_one_buffer_banks_take_the_lane_major_launch_on_the_tables_lds_alone(plan_hooks, segments):
    """The banks the GPU test renders through the lane-major launch: one buffer, one table, 12 rows -- and the launch's LDS is the
    64 KiB table block, where the same build with its block buffers in LDS asks for 16 waves x 3 KiB more (and the steps' words)."""
    for name, (seg, lm) in segments.items():
        if not lm:
            continue
        p = inner_plan(plan_hooks, seg)
        assert seg["n_fast"] == 1 and p["n_fast"] == 1 and p["n_tabs"] == 1, (name, seg, p)
        assert p["use_fast"] and p["main_build"] == 0 and p["rows"] == 12 and p["wide_cf"] and p["dyn_chunks"] >= 3, (name, p)
        assert p["inner"] == INNER_LANE_MAJOR, (name, p)
        assert p["inner_lds"] == p["n_tabs"] * p["tab_bytes_wide"] == 65536, (name, p)
        assert p["lds_12_wide"] >= p["inner_lds"] + 16 * 12 * 64 * 4, (name, p)


def test_the_shortest_segment_of_the_launch(plan_hooks, segments):
    """three tasks of row groups, 720 frames each as the planner counts them: 1441 frames take the launch, 1440 do not"""
    seg, _ = segments["depth 33 ms"]
    assert inner_plan(plan_hooks, dict(seg, len=1441))["inner"] == INNER_LANE_MAJOR
    p = inner_plan(plan_hooks, dict(seg, len=1440))
    assert p["inner"] == INNER_NONE and p["dyn_chunks"] == 2, p


def test_banks_of_two_or_three_buffers_do_not(plan_hooks, segments):
    """`p[...]` beside `p.f[...]` on one operator, an `a.r[...]` list, an amplitude list whose member has a PM chain of its own:
    more than one buffer, and on an MI355X's LDS no 12 rows"""
    for name, (seg, lm) in segments.items():
        if lm:
            continue
        p = inner_plan(plan_hooks, seg)
        assert seg["n_fast"] in (2, 3) and p["n_fast"] == seg["n_fast"], (name, seg, p)
        assert p["use_fast"] and p["inner"] != INNER_LANE_MAJOR, (name, p)


@pytest.mark.parametrize("n_fast", [1, 2, 3])
def test_exactly_one_buffer_is_the_rule_not_the_sizes(plan_hooks, segments, monkeypatch, n_fast):
    """With an LDS budget that holds 12 rows of three buffers beside the table (SAU_AMD_LDS_LIMIT, a test switch), a segment of
    two or three buffers takes the 12-row build's inner launch in the row-major form, buffers in LDS; one buffer: lane-major."""
    monkeypatch.setenv("SAU_AMD_LDS_LIMIT", str(256 * 1024))
    seg, _ = segments["depth 2000 ms"]
    p = inner_plan(plan_hooks, dict(seg, n_fast=n_fast, n_fast_full=max(n_fast, seg["n_fast_full"])))
    assert p["lds_limit"] == 256 * 1024 and p["rows"] == 12 and p["wide_cf"] and p["n_fast"] == n_fast, p
    if n_fast == 1:
        assert p["inner"] == INNER_LANE_MAJOR and p["inner_lds"] == 65536, p
    else:
        assert p["inner"] == INNER_ROW_MAJOR and p["inner_lds"] == p["lds_12_wide"] >= 65536 + 16 * n_fast * 12 * 64 * 4, p


def test_the_row_major_form_keeps_its_buffers_in_lds(plan_hooks, segments, monkeypatch):
    """SAU_AMD_NO_LANEMAJOR: the same segment's inner launch in the row-major form asks for the 12-row wide build's LDS"""
    monkeypatch.setenv("SAU_AMD_NO_LANEMAJOR", "1")
    seg, _ = segments["pm pair"]
    p = inner_plan(plan_hooks, seg)
    assert p["inner"] == INNER_ROW_MAJOR and p["inner_lds"] == p["lds_12_wide"] > 65536 + 16 * 12 * 64 * 4, p
