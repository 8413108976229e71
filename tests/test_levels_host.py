"""Level metering and the normalised file writer over a backend that has neither (include/saugns_amd.h: sauAmd_Batch_set_metering,
sauAmd_Batch_measure_rows, sauAmd_render_file_normalized): the sequential test executor (tests/seqexec) keeps engine.h's default
bodies of the metering calls, which refuse with a text, as it does for float output. A refusal changes nothing, and the file
writer's refusals -- of such a backend, of a bad target peak -- come before a file exists."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import ORACLE_FORMS, ROOT, load_program, max_diff

KEY = "devtests__voice-reuse"


@pytest.fixture(scope="module")
def file_hooks(sa, hooks):
    """tests/hooks_levels/libsaugns_amd_file_hooks.so: the product's object files (the `hooks` fixture has built them) + the
    normalised writer over an injected backend"""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "hooks_levels")])
    return sa.api.use_file_hooks(os.path.join(ROOT, "tests", "hooks_levels", "libsaugns_amd_file_hooks.so"))


def test_the_levels_structure_is_80_bytes(sa):
    L = sa.api.Levels
    assert C.sizeof(L) == 80
    assert [getattr(L, f).offset for f in ("frames", "peak", "sum_sq", "over", "full_scale", "nonfinite")] == [0, 8, 16, 32, 48, 64]


def test_metering_is_refused_and_the_int16_render_after_it_starts_at_frame_0(sa, oracle, seqexec):
    oracle.oracle().ora_set_fastmath_forms(ORACLE_FORMS)
    prg = load_program(sa, KEY)
    want = oracle.oracle_render(prg.ptr, 12000, True, chunk=5000)
    b = sa.Batch([prg], 12000, backend=seqexec.seq_backend_create(1016))
    with pytest.raises(RuntimeError, match="metering"):
        b.set_metering(True)
    assert "this backend" in sa.api.last_error()
    rows = np.zeros(64, np.float32)  # (host memory: the refusal comes before anything reads it)
    ptr = (rows.ctypes.data + 15) & ~15
    for f32 in (True, False):
        with pytest.raises(RuntimeError, match="metering"):
            b.measure_rows(ptr, 64, 1, f32, 8, 1)
    assert "this backend" in sa.api.last_error()
    b.set_metering(False)  # always succeeds
    lv = b.levels()  # never on: zeros, and no backend asked
    assert len(lv) == 1 and bytes(lv[0]) == bytes(80)
    got = b.render(stereo=True, chunk=5000)[0]
    assert bytes(b.levels(reset=True)[0]) == bytes(80)
    b.close()
    assert max_diff(got, want) == 0


@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
def test_the_normalised_writer_over_a_backend_without_metering_makes_no_file(sa, seqexec, file_hooks, tmp_path, fmt):
    prg = load_program(sa, KEY)
    path = str(tmp_path / "norm.out")
    with pytest.raises(RuntimeError, match="this backend has no"):
        sa.render_file_normalized(prg, 12000, path, fmt, 2, 0.5, backend=seqexec.seq_backend_create(1016))
    assert "this backend has no" in sa.api.last_error()
    assert not os.path.exists(path)


@pytest.mark.parametrize("target", [0.0, -1.0, math.nan, math.inf, -math.inf])
def test_a_bad_target_peak_makes_no_file(sa, seqexec, file_hooks, tmp_path, target):
    prg = load_program(sa, KEY)
    path = str(tmp_path / "norm.wav")
    # over the executor, and through the product's own entry point: the argument is looked at before any backend is made,
    # so this is the same refusal with and without a GPU
    with pytest.raises(RuntimeError, match="bad argument"):
        sa.render_file_normalized(prg, 12000, path, sa.api.SNDFILE_WAV, 1, target, backend=seqexec.seq_backend_create(1016))
    assert not os.path.exists(path)
    with pytest.raises(RuntimeError, match="bad argument"):
        sa.render_file_normalized(prg, 12000, path, sa.api.SNDFILE_WAV, 1, target)
    assert "bad argument" in sa.api.last_error()
    assert not os.path.exists(path)


def test_the_normalised_writer_keeps_render_files_argument_checks(sa, tmp_path):
    prg = load_program(sa, KEY)
    path = str(tmp_path / "norm.wav")
    for fmt, channels in ((4, 1), (-1, 1), (2, 0), (2, 3)):
        with pytest.raises(RuntimeError, match="bad argument"):
            sa.render_file_normalized(prg, 12000, path, fmt, channels, 0.5)
        assert not os.path.exists(path)


def test_plan_levels_constants_are_what_the_gpu_tests_mirror():
    """tests/test_gpu_levels.py names the two constants of launch_plan.h's plan_levels (samples per sweep, samples per
    workgroup) to place its frame counts on both sides of them: they are read here from the header they come from."""
    import re
    hdr = open(os.path.join(ROOT, "saugns_amd", "csrc", "launch_plan.h")).read()
    assert re.search(r"LEVELS_THREADS = 256;", hdr)
    assert re.search(r"LEVELS_SWEEP_F32 = LEVELS_THREADS \* 4, LEVELS_SWEEP_S16 = LEVELS_THREADS \* 8;", hdr)
    assert re.search(r"LEVELS_WG_SAMPLES = 16384;", hdr)
    import test_gpu_levels as g
    assert (g.LEVELS_SWEEP_F32, g.LEVELS_SWEEP_S16, g.LEVELS_WG_SAMPLES) == (1024, 2048, 16384)
