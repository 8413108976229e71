"""Float32 sample output over a backend that has none (include/saugns_amd.h: sauAmd_Batch_run_f32, SAU_AMD_SNDFILE_WAV_F32):
the sequential test executor (tests/seqexec) keeps engine.h's default bodies of the float calls, which refuse with a text.
A refused float run renders nothing and leaves the engine where it was."""
import os

import numpy as np
import pytest

from conftest import ORACLE_FORMS, load_program, max_diff

KEY = "devtests__voice-reuse"


def test_run_f32_is_refused_and_the_int16_render_after_it_starts_at_frame_0(sa, oracle, seqexec):
    oracle.oracle().ora_set_fastmath_forms(ORACLE_FORMS)
    prg = load_program(sa, KEY)
    want = oracle.oracle_render(prg.ptr, 12000, True, chunk=5000)
    b = sa.Batch([prg], 12000, backend=seqexec.seq_backend_create(1016))
    for fetch in (True, False):
        with pytest.raises(RuntimeError, match="float32"):
            b.run_f32(5000, stereo=True, fetch=fetch)
    assert "this backend" in sa.api.last_error()
    assert not b.device_pcm_f32(0)
    got = b.render(stereo=True, chunk=5000)[0]
    b.close()
    assert max_diff(got, want) == 0


@pytest.mark.parametrize("channels", [1, 2])
def test_float_wav_over_a_backend_without_float_output_fails_cleanly(sa, seqexec, tmp_path, capfd, channels):
    prg = load_program(sa, KEY)
    path = str(tmp_path / "f32.wav")
    with pytest.raises(RuntimeError):
        sa.render_file(prg, 12000, path, sa.api.SNDFILE_WAV_F32, channels, backend=seqexec.seq_backend_create(1016))
    assert "float32" in capfd.readouterr().err  # (the output stage reports on stderr, like the reference's)
    # the int16 writer over the same executor is what it was
    n = sa.render_file(prg, 12000, path, sa.api.SNDFILE_WAV, channels, backend=seqexec.seq_backend_create(1016))
    assert n > 0 and os.path.getsize(path) == 44 + n * channels * 2


def test_a_format_of_4_is_a_bad_argument(sa, seqexec, tmp_path, capfd):
    prg = load_program(sa, KEY)
    path = str(tmp_path / "none.wav")
    with pytest.raises(RuntimeError):
        sa.render_file(prg, 12000, path, 4, 1, backend=seqexec.seq_backend_create(1016))
    assert "bad argument" in capfd.readouterr().err
    assert not os.path.exists(path)
    assert sa.api.SNDFILE_WAV_F32 == 3
