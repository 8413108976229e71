"""The HIP backend's launch planner (saugns_amd/csrc/launch_plan.h) without a GPU: which builds the bench workloads take,
how rows per pass degrade as LDS runs out, the feedback chains' chunk boundaries, the closed-form launches' tasks.
Everything goes through one hook, sauAmd_launch_plan (tests/hooks/test_hooks.cpp)."""
import ctypes as C

import pytest

from conftest import load_program

# a segment's scalars, in the order of tests/seqexec's seq_backend_last_segment
SEG = ("n_main", "n_fast", "n_fast_full", "may_scan", "serial", "len", "n_voices", "n_streams", "n_slots", "sum_levels", "max_ops",
       "max_steps", "n_pan_rows", "wave_mask", "maybe_block", "maybe_cub", "n_chain_rows", "n_inc_rows", "n_look_rows", "n_may_scan",
       "n_chain_slots", "chain_rows_padded", "stereo", "pcm_offset")
PER_VOICE = ("n_voices", "n_pan_rows", "n_chain_rows", "n_inc_rows", "n_look_rows", "n_may_scan", "n_chain_slots")
# what the hook returns for a segment
PLAN = ("bl_ok", "W", "T", "V", "HB", "bl_lds", "bl_tabs", "bl_grid",
        "use_fast", "main_build", "rows", "rows_multi", "rows_cf", "rows_lean", "lean_on", "n_tabs", "wide_cf", "wide_look",
        "cub_ok", "look_split", "scan", "look", "look_wpv", "look_inside", "look_words_real", "chains", "n_chunks", "short_last",
        "duo", "tailmix", "queues", "inmix", "inner", "dyn_chunks", "dyn_static", "dyn_small", "div_m", "div_s",
        "grid", "grid_cf", "grid_look", "pass_grid", "max_lds", "lds_limit", "mixer", "cf_dyn_chunks", "cf_dyn_static",
        "groups", "task_groups", "dyn_min_tasks", "n_want", "fk_grid")
INNER_LANE_MAJOR = 2
MI355X = dict(lds=160 * 1024, cus=256)  # LDS per CU, CUs: grid 256, eight XCDs


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    """The planner reads the switches from the environment: none set but what a test sets."""
    import os
    for name in list(os.environ):
        if name.startswith("SAU_AMD_"):
            monkeypatch.delenv(name)


def call(hooks, what, values, n_out):
    fn = hooks.sauAmd_launch_plan
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
    a = (C.c_uint32 * len(values))(*values)
    out = (C.c_uint32 * n_out)()
    n = fn(what, a, len(values), out, n_out)
    assert n >= 0, "sauAmd_launch_plan refused its arguments"
    return list(out[:n])


def plan(hooks, seg, lds=MI355X["lds"], cus=MI355X["cus"], f32=False):
    """The plan of segment `seg` (a dict over SEG) as one stream of the batch per `n_streams`, written in full."""
    row_stride = (seg["len"] + 63) & ~63
    vals = [int(seg[k]) for k in SEG] + [lds, cus, row_stride, 2 * row_stride, int(f32), seg["len"],
                                         -(-seg["n_voices"] // seg["n_streams"])]
    return dict(zip(PLAN, call(hooks, 0, vals, len(PLAN))))


def segment_of(sa, seqexec, prg, frames=512):
    """The scalars of the segment the engine cuts for `prg` at frame 0, through the sequential test backend."""
    b = sa.Batch([prg], 44100, backend=seqexec.seq_backend_create(256))
    b.run(frames, stereo=False, fetch=False)
    out = (C.c_uint32 * len(SEG))()
    seqexec.seq_backend_last_segment(out)
    return dict(zip(SEG, list(out)))


def scaled(seg, n_voices, n_streams, frames):
    """The same bank at the workload's size: per-voice counts grow with the voices."""
    s = dict(seg)
    for k in PER_VOICE:
        s[k] = seg[k] * n_voices // seg["n_voices"]
    s["n_chain_slots"] = (s["n_chain_slots"] + 63) & ~63
    s["n_streams"] = n_streams
    s["len"] = frames
    return s


@pytest.fixture(scope="module")
def workloads(sa, seqexec):
    """The five bench workloads' segments: shapes from a short, few-voice instance of the same bank, sizes the workload's own."""
    from saugns_amd import voicebank as vb
    few = 8
    return {
        "config3": scaled(segment_of(sa, seqexec, vb.config3(n=few, seconds=1)), 1024, 1, 441000),
        "config2": scaled(segment_of(sa, seqexec, vb.config2(n=few, seconds=1)), 256, 1, 441000),
        "fm": scaled(segment_of(sa, seqexec, vb.config3_fm(n=few, seconds=1)), 1024, 1, 441000),
        "config5": scaled(segment_of(sa, seqexec, vb.config5(n=few, seconds=1)), 4096, 1, 441000),
        # 64 renders of rainy_thunder.sau per batch, a stream each
        "config4": (lambda s: scaled(s, 64 * s["n_voices"], 64, 441000))(segment_of(sa, seqexec, load_program(sa, "config4_seed0"))),
    }


# ---- (a) the bench workloads take the documented builds ----

def test_config3_plan(hooks, workloads):
    p = plan(hooks, workloads["config3"])
    assert p["use_fast"] and p["main_build"] == 0 and p["rows"] == 12 and p["wide_cf"]
    assert p["inner"] == INNER_LANE_MAJOR and p["queues"] and p["inmix"]
    assert not p["scan"] and not p["chains"] and not p["duo"]


def test_config3_float_run_does_not_mix_in_the_launch(hooks, workloads):
    p = plan(hooks, workloads["config3"], f32=True)
    assert p["rows"] == 12 and p["inner"] == INNER_LANE_MAJOR and p["queues"] and not p["inmix"]


def test_config2_plan(hooks, workloads):
    p = plan(hooks, workloads["config2"])
    assert p["use_fast"] and p["main_build"] == 0 and p["rows"] == 8 and not p["wide_cf"]
    assert p["queues"] and not p["inmix"] and p["inner"] == 0


def test_config4_plan(hooks, workloads):
    p = plan(hooks, workloads["config4"])
    assert p["use_fast"] and p["main_build"] == 2 and p["rows"] == 8 and p["rows_cf"] == 8 and p["duo"]
    assert not p["wide_cf"] and not p["wide_look"] and p["look_words_real"]


def test_fm_bank_plan(hooks, workloads):
    p = plan(hooks, workloads["fm"])
    assert p["use_fast"] and p["main_build"] == 2 and p["rows"] == 8 and p["wide_look"] and not p["duo"]


def test_config5_plan(hooks, workloads):
    p = plan(hooks, workloads["config5"])
    assert p["use_fast"] and p["chains"] and p["lean_on"] and p["rows_lean"] == 6
    assert p["n_chunks"] > 1 and p["pass_grid"] <= p["grid"]


# ---- (b) degradation: rows per pass as LDS runs out ----

ROWS_ANY = {2, 4, 5, 6, 8}          # fast_kernel<T, 0> and <T, 2>
ROWS_WIDE = {6, 8, 10, 12}          # the closed-form build with wide table blocks


@pytest.mark.parametrize("lds", [160 * 1024, 65536])
@pytest.mark.parametrize("n_tables", [1, 12])
def test_rows_per_pass_only_go_down(hooks, workloads, lds, n_tables):
    base = dict(workloads["config3"], wave_mask=(1 << n_tables) - 1)
    last, was_fast = None, True
    for n_fast in range(1, 13):
        seg = dict(base, n_fast=n_fast, n_fast_full=n_fast)
        p = plan(hooks, seg, lds=lds)
        steps = min(seg["max_steps"], 64)
        two_rows_fit = 16 * (n_fast * 64 * 2 * 4 + steps * 8) + 1024 <= lds
        assert bool(p["use_fast"]) == two_rows_fit, (n_fast, p)
        assert was_fast or not p["use_fast"], "the path came back with more buffers"
        was_fast = bool(p["use_fast"])
        if not p["use_fast"]:
            continue
        assert p["rows"] in (ROWS_WIDE if p["wide_cf"] else ROWS_ANY), p
        assert last is None or p["rows"] <= last, (n_fast, p["rows"], last)
        last = p["rows"]
        assert p["max_lds"] <= p["lds_limit"] == lds, p


@pytest.mark.parametrize("lds", [160 * 1024, 65536])
def test_split_segment_rows_only_go_down(hooks, workloads, lds):
    """... and of a segment with look-back voices: both launches' rows, the full build's never above 4"""
    last = None
    for n_fast in range(1, 13):
        seg = dict(workloads["fm"], n_fast=n_fast, n_fast_full=n_fast + 1)
        p = plan(hooks, seg, lds=lds)
        if not p["use_fast"]:
            continue
        assert p["main_build"] == 2 and p["rows"] in ROWS_ANY and p["rows_multi"] in {2, 4}
        assert p["rows_cf"] in (ROWS_WIDE if p["wide_cf"] else ROWS_ANY)
        assert last is None or (p["rows"] <= last[0] and p["rows_cf"] <= last[1]), (n_fast, p, last)
        last = (p["rows"], p["rows_cf"])
        assert p["max_lds"] <= lds, p


# ---- (c) chain_chunk_bounds ----

@pytest.mark.parametrize("length,chunks_env", [(4095, None), (16384, None), (8 * 4096 + 1, None), (81930, "20"), (441000, None),
                                               (8 * 4096, None), (65536, None), (16 * 16384 + 5000, None)])
def test_chain_chunk_bounds(hooks, monkeypatch, length, chunks_env):
    if chunks_env:
        monkeypatch.setenv("SAU_AMD_CHAIN_CHUNKS", chunks_env)  # (81930 frames in 20 chunks: ADVICE r05's empty chunks)
    out = call(hooks, 1, [length], 40)
    n, short_last, cb = out[0], out[1], out[2:]
    assert len(cb) == n + 1 and 1 <= n <= 33
    assert cb[0] == 0 and cb[-1] == length
    assert all(b > a for a, b in zip(cb, cb[1:])), cb
    assert all(b % 256 == 0 for b in cb[1:-1]), cb
    if not chunks_env:
        # the short last chunk: where the frames make 4 to 31 chunks of their own and the segment is longer than 8 x 4096
        by_frames = min(32, -(-length // 16384))
        while by_frames > 1 and length // by_frames < 4096:
            by_frames -= 1
        want_short = 4 <= by_frames < 32 and length > 8 * 4096
        assert bool(short_last) == want_short
        if want_short:
            assert cb[-2] == (length - 4096) & ~255
    else:
        assert not short_last


# ---- (d) tasks ----

@pytest.mark.parametrize("n_voices", [1, 3, 16, 64, 256, 1024, 4096])
@pytest.mark.parametrize("length", [4410, 44100, 441000])
def test_tasks_go_through_the_queues_when_there_are_enough(hooks, workloads, n_voices, length):
    p = plan(hooks, scaled(workloads["config3"], n_voices, 1, length))
    assert p["use_fast"] and p["main_build"] == 0
    k_dyn = -(-p["groups"] // p["task_groups"])
    waves = p["grid"] * 16
    assert bool(p["dyn_static"]) == (n_voices * k_dyn < p["dyn_min_tasks"] * waves), p
    if p["dyn_static"]:
        assert p["dyn_chunks"] == max(1, min(waves // n_voices, p["groups"]))
    else:
        assert p["dyn_chunks"] == k_dyn and p["dyn_small"] == 0


@pytest.mark.parametrize("d", [1, 3, 64, 1000, 1024, 4096])
def test_magic_divisor(hooks, d):
    """q / n_voices by the kernels' udiv_magic (k_fast_voice.h: exact for every 32-bit q) with the divisor words the host prepares"""
    import random
    rnd = random.Random(d)
    top = 2 ** 32 - 1
    qs = list(range(0, 3000)) + [top - i for i in range(3000)] + [k * d + e for k in (1, 7, 4095, top // d) for e in (-1, 0, 1)
                                                                   if 0 <= k * d + e <= top]
    qs += [rnd.randrange(0, top + 1) for _ in range(3000)]
    got = call(hooks, 2, [d] + qs, len(qs))
    assert got == [q // d for q in qs]
