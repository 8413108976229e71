"""The final mixer on a stream of its own (saugns_amd/csrc/mix_overlap.h, launch_plan.h: plan_mix_overlap), without a GPU.

A segment's last mixer launch runs on a side stream beside the next segment's set-up launches; a host-only tracker tells the
backend where its main stream has to wait. tests/hooks_overlap plays drawn sequences of backend operations on that tracker, in
the order HipBackendImpl makes its calls, and logs what either stream would do. Here the log is replayed in a model of two
in-order streams: every launch takes a drawn time, a mixer starts when the main stream has reached its fork and the mixer
before it has ended, and a wait holds the main stream until its mixer has ended. For every pair (mixer k, later operation on
the main stream) that meets on a set's records, a block of rows or the PCM, the mixer must have ended before the operation
starts. And in the steady sequence of BASELINE config 3 -- segment after segment, each with a launch that writes PCM itself
and a final mixer -- there is exactly one wait per segment, in front of the first PCM writer (alternate rows) or the first
writer of rows (shared rows): any more would lose the overlap without a test noticing.

The same sequences go through overlap_driver_san, the interpreter as a program of its own built with
-fsanitize=address,undefined: same log, no finding."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HOOKS = os.path.join(ROOT, "tests", "hooks_overlap")
OP_SEGMENT, OP_ENTRY, OP_REFUSE, OP_SWITCHES = 0, 1, 2, 3
LOG_WAIT, LOG_RECORDS, LOG_ROWS, LOG_PCM, LOG_ALL, LOG_MIXER, LOG_SEGMENT = 1, 2, 3, 4, 5, 6, 7
W_RECORDS, W_POISON, W_ROWS, W_PCM, W_MIXER_MAIN, W_ENTRY = 1, 2, 3, 4, 5, 6
OFF, SHARED, ALTERNATE = 0, 1, 2
MIXER, INMIX, POISON, INNER, OTHER_PCM, DRAIN = 1, 2, 4, 8, 16, 32  # OP_SEGMENT's flags
CONFIG3 = MIXER | INMIX | INNER  # a segment of BASELINE config 3: edge and inner launches, the inner one mixing tiles itself
ENTRIES = ("fetch", "sync", "order_after", "save_state", "load_state", "format change", "zero_pcm", "metering")


@pytest.fixture(scope="module")
def hooks():
    path = os.path.join(HOOKS, "libsaugns_amd_overlap_hooks.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-s", "-C", HOOKS, "libsaugns_amd_overlap_hooks.so"])
    lib = ctypes.CDLL(path)
    lib.sauAmd_overlap_play.restype = ctypes.c_longlong
    lib.sauAmd_overlap_play.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]
    lib.sauAmd_overlap_plan.restype = ctypes.c_int
    lib.sauAmd_overlap_plan.argtypes = [ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    return lib


def play(lib, ops):
    ops = np.ascontiguousarray(ops, dtype=np.int64).reshape(-1, 6)
    log = np.zeros(3 * 16 * len(ops) + 3, dtype=np.int64)  # (a segment logs ten entries at most)
    n = lib.sauAmd_overlap_play(ops.ctypes.data, len(ops), log.ctypes.data, log.size)
    assert 0 <= n * 3 <= log.size, n
    return log[: 3 * n].reshape(-1, 3)


def draw_ops(rng, n):
    """Segments with and without a PCM writer among their launches (the closed-form launch's own mixing, which is what puts the
    final mixer on the side stream; another launch's), with and without a final mixer, poisoned or not, in one launch or in
    edge and inner groups, of rows below and above the cap; either mode and the serial order (the switches change in mid-sequence, which no backend does: a
    superset of what one sees); the second block refused; every kind of joining entry point."""
    ops = []
    for i in range(n):
        r = rng.random()
        if r < 0.70:
            flags = ((MIXER if rng.random() < 0.85 else 0) | (INMIX if rng.random() < 0.6 else 0) | (POISON if rng.random() < 0.2 else 0) |
                     (INNER if rng.random() < 0.7 else 0) | (OTHER_PCM if rng.random() < 0.2 else 0) | (DRAIN if rng.random() < 0.1 else 0))
            ops.append([OP_SEGMENT, flags, int(rng.choice([1, 100, 1800, 5000])), 0, 0, 0])
        elif r < 0.90:
            ops.append([OP_ENTRY, int(rng.integers(0, len(ENTRIES))), 0, 0, 0, 0])
        elif r < 0.93:
            # (a refusal is for good: only late in the sequence, so that both modes get their share of it)
            ops.append([OP_REFUSE, 0, 0, 0, 0, 0] if i > 0.8 * n else [OP_ENTRY, 0, 0, 0, 0, 0])
        else:
            ops.append([OP_SWITCHES, int(rng.random() < 0.2), int(rng.random() < 0.3), int(rng.choice([0, 64, 4096])), 0, 0])
    return ops


def check_log(log, rng):
    """The model: two in-order streams. Returns (mixers, waits)."""
    t_main = 0.0       # when the main stream's last operation ends
    side_free = 0.0    # when the side stream's last mixer ends
    mixers = {}        # ticket -> (set, block, end)
    running = {}       # ... those that have not ended by t_main (the main stream's time never goes back)
    for kind, x, y in log.tolist():
        if kind == LOG_SEGMENT:
            continue
        if kind == LOG_WAIT:
            assert x in mixers, f"a wait for ticket {x}, which no mixer has"
            t_main = max(t_main, mixers[x][2])
            continue
        if kind == LOG_MIXER:
            assert x == len(mixers) + 1, "tickets count the mixers in launch order"
            # (long mixers, so that a missing wait shows: the main stream's operations below are short)
            start = max(t_main, side_free)
            side_free = start + float(rng.choice([0.5, 50.0, 5000.0]))
            mixers[x] = running[x] = (y & 1, y >> 1, side_free)
            continue
        start = t_main
        running = {t: m for t, m in running.items() if m[2] > start}
        for t, (mset, mblock, end) in running.items():
            meets = (kind == LOG_RECORDS and mset == x) or (kind == LOG_ROWS and mblock == x) or kind in (LOG_PCM, LOG_ALL)
            assert not meets or end <= start, (
                f"mixer {t} (set {mset}, block {mblock}) still runs at {start} (ends {end}) when the main stream "
                f"{ {LOG_RECORDS: 'writes records of set', LOG_ROWS: 'writes rows of block', LOG_PCM: 'touches PCM', LOG_ALL: 'enters'}[kind] } {x} {y}")
        t_main = start + float(rng.uniform(0.1, 2.0))
    return mixers


@pytest.mark.parametrize("seed", range(6))
def test_drawn_sequences_keep_every_hazard_apart(hooks, seed):
    rng = np.random.default_rng(7300 + seed)
    ops = draw_ops(rng, 4000)
    log = play(hooks, ops)
    mixers = check_log(log, rng)
    modes = set(log[log[:, 0] == LOG_SEGMENT][:, 1].tolist())
    assert modes == {OFF, SHARED, ALTERNATE} and len(mixers) > 500, (modes, len(mixers))
    # segment n uses set n mod 2, whatever happens between the segments
    sets = log[log[:, 0] == LOG_SEGMENT][:, 2]
    assert (sets == np.arange(len(sets)) % 2).all()
    # a block of rows of its own only in alternate mode, and only for set 1
    for kind, x, y in log[log[:, 0] == LOG_MIXER].tolist():
        assert (y >> 1) in (0, y & 1)


@pytest.mark.parametrize("shared", [0, 1])
def test_a_join_inside_the_mixers_launch_does_not_cover_that_mixer(hooks, shared):
    """The timing pool may drain -- a join -- after the mixer's ticket is known and before its done event is recorded. The
    tracker hears of the mixer only once that event is there, so the join takes nothing for waited-for that it has not waited
    for: the next segment still waits for this mixer, and so does an entry point right behind it."""
    seg = [OP_SEGMENT, CONFIG3 | DRAIN, 100, 0, 0, 0]
    log = play(hooks, [[OP_SWITCHES, 0, shared, 4096, 0, 0]] + [seg] * 8 + [[OP_ENTRY, 0, 0, 0, 0, 0]])
    check_log(log, np.random.default_rng(4))
    waits = log[log[:, 0] == LOG_WAIT]
    # every mixer is waited for exactly once: 1 .. 7 by the segment after it (the drain's join in between finds the one
    # before already joined), 8 by the entry point
    assert waits[:, 1].tolist() == list(range(1, 9)), waits
    assert waits[:-1, 2].tolist() == [W_ROWS if shared else W_PCM] * 7 and waits[-1, 2] == W_ENTRY


def test_a_refused_second_block_means_shared_rows_for_good(hooks):
    seg = [OP_SEGMENT, CONFIG3, 100, 0, 0, 0]
    log = play(hooks, [seg, [OP_REFUSE, 0, 0, 0, 0, 0]] + [seg] * 6)
    modes = log[log[:, 0] == LOG_SEGMENT][:, 1].tolist()
    assert modes == [ALTERNATE] + [SHARED] * 6, modes
    assert all((y >> 1) == 0 for y in log[log[:, 0] == LOG_MIXER][:, 2].tolist())
    check_log(log, np.random.default_rng(1))


@pytest.mark.parametrize("mode", [ALTERNATE, SHARED])
def test_the_steady_config3_sequence_waits_once_per_segment(hooks, mode):
    """Segment after segment of config 3: no wait in the first, then one per segment -- in front of the inner launch (the first
    PCM writer) with rows of its own, in front of the edge launch (the first writer of rows) with shared rows."""
    ops = [[OP_SWITCHES, 0, 1 if mode == SHARED else 0, 4096, 0, 0]] + [[OP_SEGMENT, CONFIG3, 1810, 0, 0, 0]] * 40
    log = play(hooks, ops)
    check_log(log, np.random.default_rng(2))
    segs = np.flatnonzero(log[:, 0] == LOG_SEGMENT)
    assert len(segs) == 40 and (log[segs, 1] == mode).all()
    for i, at in enumerate(segs):
        part = log[at: segs[i + 1] if i + 1 < len(segs) else len(log)]
        waits = part[part[:, 0] == LOG_WAIT]
        if i == 0:
            assert len(waits) == 0
            continue
        assert len(waits) == 1, (i, waits)
        assert waits[0, 1] == i and waits[0, 2] == (W_PCM if mode == ALTERNATE else W_ROWS), (i, waits)
        # ... and the mixer it waits for is the previous segment's: everything before the wait ran beside it
        k = int(np.flatnonzero(part[:, 0] == LOG_WAIT)[0])
        assert part[k + 1, 0] == (LOG_PCM if mode == ALTERNATE else LOG_ROWS)
    assert (log[log[:, 0] == LOG_MIXER][:, 1] == np.arange(1, 41)).all()


def test_the_serial_order_launches_no_side_mixer_and_waits_for_nothing(hooks):
    log = play(hooks, [[OP_SWITCHES, 1, 0, 4096, 0, 0]] + [[OP_SEGMENT, CONFIG3, 100, 0, 0, 0], [OP_ENTRY, 0, 0, 0, 0, 0]] * 20)
    assert not (log[:, 0] == LOG_MIXER).any() and not (log[:, 0] == LOG_WAIT).any()


def test_segments_whose_launch_does_not_mix_keep_the_serial_order(hooks):
    """No launch of the segment writes PCM ahead of its mixer: nothing would join the last segment's mixer before the rendering
    launches (measured slower on every such workload, launch_plan.h), so their mixers stay on the main stream -- and a
    segment of config 3's kind between them still waits for its predecessor's."""
    plain, other = [OP_SEGMENT, MIXER | INNER, 100, 0, 0, 0], [OP_SEGMENT, MIXER | OTHER_PCM, 100, 0, 0, 0]
    log = play(hooks, [plain, other] * 10)
    assert (log[log[:, 0] == LOG_SEGMENT][:, 1] == OFF).all() and not (log[:, 0] == LOG_MIXER).any()
    log = play(hooks, [[OP_SEGMENT, CONFIG3, 100, 0, 0, 0], plain, other] * 10)
    check_log(log, np.random.default_rng(3))
    assert log[log[:, 0] == LOG_SEGMENT][:, 1].tolist() == [ALTERNATE, OFF, OFF] * 10
    assert (log[:, 0] == LOG_MIXER).sum() == 10 and (log[:, 0] == LOG_WAIT).sum() == 10


def test_the_planner_rule_and_its_switches(hooks, monkeypatch):
    """plan_mix_overlap: on for every segment whose closed-form launch mixes tiles itself and which has a final mixer launch;
    rows of their own up to the cap, which admits config 3's 1.81 GB block by default, where the launch is split into edge and
    inner groups."""
    for name in ("SAU_AMD_NO_MIX_OVERLAP", "SAU_AMD_MIX_OVERLAP_SHARED", "SAU_AMD_MIX_OVERLAP_MB", "SAU_AMD_MIX_OVERLAP_FAIL"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("SAU_AMD_TUNE", "1")
    config3 = 1024 * 441024 * 4

    def plan(max_write, rows, refused, inmix=1, inner=1):
        return hooks.sauAmd_overlap_plan(max_write, rows, refused, inmix, inner)

    assert plan(441000, config3, 0) == ALTERNATE
    assert plan(441000, config3 * 5 // 4, 0) == ALTERNATE  # (what the pool rounds the block to)
    assert plan(0, config3, 0) == OFF  # no frame to write: no final mixer
    assert plan(441000, config3, 0, inmix=0) == OFF  # nothing would join the mixer ahead of the rendering launches
    assert plan(441000, config3, 0, inner=0) == SHARED  # one launch: no edge groups to run beside the mixer
    assert plan(441000, config3, 1) == SHARED  # the second block was refused
    assert plan(441000, 5 << 30, 0) == SHARED  # beyond the cap
    monkeypatch.setenv("SAU_AMD_MIX_OVERLAP_MB", "1024")
    assert plan(441000, config3, 0) == SHARED and plan(441000, 1 << 29, 0) == ALTERNATE
    monkeypatch.setenv("SAU_AMD_MIX_OVERLAP_SHARED", "1")
    assert plan(441000, 1 << 20, 0) == SHARED
    monkeypatch.setenv("SAU_AMD_NO_MIX_OVERLAP", "1")
    assert plan(441000, 1 << 20, 0) == OFF
    monkeypatch.delenv("SAU_AMD_TUNE")
    assert plan(441000, 1 << 20, 0) == ALTERNATE  # (the switches count only under SAU_AMD_TUNE)


def test_the_same_sequences_in_a_program_built_with_sanitizers(hooks, tmp_path):
    """overlap_driver_san (address and undefined-behaviour sanitizers, every finding fatal) plays the sequences of the drawn
    test and gives the library's logs."""
    subprocess.check_call(["make", "-s", "-C", HOOKS, "overlap_driver_san"])
    exe = os.path.join(HOOKS, "overlap_driver_san")
    for seed in range(3):
        ops = np.asarray(draw_ops(np.random.default_rng(7300 + seed), 4000), dtype=np.int64)
        src, dst = tmp_path / f"ops{seed}.bin", tmp_path / f"log{seed}.bin"
        ops.tofile(src)
        out = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and not out.stderr, (out.returncode, out.stderr[-2000:])
        assert (np.fromfile(dst, dtype=np.int64).reshape(-1, 3) == play(hooks, ops)).all()
