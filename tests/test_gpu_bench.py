"""bench.py's --dump-outputs on the device: what it writes is the PCM of the last timed step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


@pytest.mark.gpu
def test_bench_dump_outputs_is_the_last_timed_steps_pcm(tmp_path, sa):
    frames, steps, warmup, voices = 44100, 2, 1, 16
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--voices", str(voices),
                          "--frames", str(frames), "--steps", str(steps), "--warmup", str(warmup),
                          "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    line = json.loads([x for x in out.stdout.splitlines() if x.startswith("{")][-1])
    assert line["steps"] == steps and line["ms_per_step"] > 0
    got = np.load(tmp_path / "pcm.npy")
    assert got.dtype == np.float32 and got.shape == (frames,)
    # the same program through the batch API: bench.py's first step, the warm-up, the timed steps -- the last one fetched
    from saugns_amd import voicebank
    seconds = frames * (steps + warmup + 1000 + 2) // 44100 + 2  # (bench.py sizes config 3's script for --sustain 1000)
    batch = sa.Batch([voicebank.config3(n=voices, seconds=seconds)], 44100)
    try:
        for _ in range(1 + warmup + steps - 1):
            batch.run(frames, stereo=False, fetch=False)
        want = batch.run(frames, stereo=False)[0][0]
    finally:
        batch.close()
    assert np.abs(want).max() > 0
    assert np.array_equal(got, want.astype(np.float32))
