"""A segment's final mixer on a stream of its own, beside the next segment's set-up launches (saugns_amd/csrc/mix_overlap.h,
hip_backend.hip: launch_mixer): the PCM is what it was -- the oracle's, or the serial order's (SAU_AMD_NO_MIX_OVERLAP) -- in
either mode, and SAU_AMD_OVERLAP_REPORT tells where each segment's mixer ran, on which set of records, and where the main
stream waited for which mixer: a test that would pass on the serial order as well says nothing.

The shapes are tests/test_gpu_inmix.py's smallest at which the closed-form launch still mixes tiles itself: 96 config-3
voices, launches of 16 workgroups, runs of 176400 frames, rows and PCM poisoned ahead of every run."""
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ORACLE_FORMS, ROOT

pytestmark = pytest.mark.gpu

RUN = 176400
LINE = re.compile(r"overlap: mode (\w+) set (\d) block (\d) mixer (\w+) ticket (\d+) waits(.*)")
INMIX = re.compile(r"inmix: voices (\d+) frames (\d+) chunks (\d+) x (\d+) frames, tiles (\d+) of")
MODES = {"alternate": {}, "shared": {"SAU_AMD_MIX_OVERLAP_SHARED": "1"}, "off": {"SAU_AMD_NO_MIX_OVERLAP": "1"}}


def _reports(capfd):
    """[(mode, set, block, mixer, ticket, [(where, ticket, done|busy), ...]), ...], one per segment; and the stderr itself"""
    err = capfd.readouterr().err
    out = []
    for m in LINE.finditer(err):
        waits = [tuple(w.split(":")) for w in m.group(6).split() if w != "-"]
        out.append((m.group(1), int(m.group(2)), int(m.group(3)), m.group(4), int(m.group(5)), [(w, int(t), d) for w, t, d in waits]))
    return out, err


def _env(monkeypatch, mode, poison=True, **more):
    for name in ("SAU_AMD_NO_MIX_OVERLAP", "SAU_AMD_MIX_OVERLAP_SHARED", "SAU_AMD_MIX_OVERLAP_FAIL", "SAU_AMD_MIX_OVERLAP_MB"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("SAU_AMD_FK_GRID", "16")
    monkeypatch.setenv("SAU_AMD_OVERLAP_REPORT", "1")
    if poison:
        monkeypatch.setenv("SAU_AMD_POISON", "1")
    else:
        monkeypatch.delenv("SAU_AMD_POISON", raising=False)
    for k, v in {**MODES[mode], **more}.items():
        monkeypatch.setenv(k, v)


@pytest.fixture(scope="module")
def bank(oracle):
    """96 config-3 voices x 12 s with pans of their own, and the oracle's PCM of the three 4 s runs (mono)"""
    from saugns_amd import voicebank as vb
    oracle.oracle().ora_set_fastmath_forms(ORACLE_FORMS)
    voices = vb.config3_voices(96, 12)
    for i, v in enumerate(voices):
        v.pan = vb.Line(vb._num(".2f", ((i * 37) % 100) / 100.0))
    prg = vb.build_program(voices)
    want = oracle.oracle_render(prg.ptr, 44100, False, chunk=RUN)
    assert len(want) == 3 * RUN
    return prg, want


def _check_sides(reps, mode, n):
    """n segments, each with its mixer on the side stream, sets alternating, tickets counting up"""
    assert len(reps) == n, reps
    for i, (m, s, b, mixer, ticket, waits) in enumerate(reps):
        assert (m, s, mixer, ticket) == (mode, i % 2, "side", i + 1), (i, reps[i])
        assert b == (s if mode == "alternate" else 0), (i, reps[i])


@pytest.mark.parametrize("mode", ["alternate", "shared", "off"])
def test_three_runs_fetched_run_by_run(sa, bank, capfd, monkeypatch, mode):
    """Each run's PCM is the oracle's. With the overlap on every mixer runs on the side stream from the first run on, the set
    alternates, and the run's fetch is what waits for it; with it off no mixer leaves the main stream and nothing waits."""
    prg, want = bank
    _env(monkeypatch, mode, SAU_AMD_INMIX_REPORT="1")
    batch = sa.Batch([prg], 44100)
    for r in range(3):
        got = batch.run(RUN, stereo=False)[0][0]
        assert (np.asarray(got) == want[r * RUN:(r + 1) * RUN]).all(), (mode, r)
    batch.close()
    reps, err = _reports(capfd)
    tiles = [int(m.group(5)) for m in INMIX.finditer(err)]
    assert len(tiles) == 3 and min(tiles) > 0, tiles  # (the launch mixed tiles itself: the mixer had control words to read)
    if mode == "off":
        assert [(m, mixer, t, w) for m, s, b, mixer, t, w in reps] == [("off", "main", 0, [])] * 3, reps
        assert [s for m, s, b, mixer, t, w in reps] == [0, 1, 0]
        return
    _check_sides(reps, mode, 3)
    assert reps[0][5] == [] and [w[:2] for w in reps[1][5]] == [("fetch_pcm", 1)] and [w[:2] for w in reps[2][5]] == [("fetch_pcm", 2)], reps


@pytest.mark.parametrize("poison", [True, False])
@pytest.mark.parametrize("mode", ["alternate", "shared"])
def test_runs_that_nobody_fetches_overlap_the_next_run(sa, bank, capfd, monkeypatch, mode, poison):
    """Only the last of three runs is fetched: its PCM is the oracle's third run. Each run waits once for the mixer of the run
    before and for nothing else: in front of the inner launch (the first PCM writer) with rows of its own, in front of the edge
    launch (the first writer of rows) with shared rows -- or, poisoned, where the run's PCM is poisoned first."""
    prg, want = bank
    _env(monkeypatch, mode, poison=poison)
    batch = sa.Batch([prg], 44100)
    batch.run(RUN, stereo=False, fetch=False)
    batch.run(RUN, stereo=False, fetch=False)
    got = batch.run(RUN, stereo=False)[0][0]
    batch.close()
    assert (np.asarray(got) == want[2 * RUN:]).all()
    reps, _ = _reports(capfd)
    _check_sides(reps, mode, 3)
    where = "poison_run" if poison else "pcm" if mode == "alternate" else "rows"
    assert reps[0][5] == [], reps
    for i in (1, 2):
        assert [w[:2] for w in reps[i][5]] == [(where, i)], (i, reps)


VIEW = r"""
import sys
import numpy as np
import torch  # (before the library: torch's wheel brings a HIP runtime of its own, and a process has room for one -- api.Batch.device_tensor)
sys.path.insert(0, sys.argv[1])
import saugns_amd as sa
from saugns_amd import voicebank as vb
sa.set_piluts(np.fromfile(sys.argv[1] + "/tests/golden/piluts_ref.f32", dtype="<f4").reshape(12, 2048))
voices = vb.config3_voices(96, 12)
for i, v in enumerate(voices):
    v.pan = vb.Line(vb._num(".2f", ((i * 37) % 100) / 100.0))
batch = sa.Batch([vb.build_program(voices)], 44100)
for _ in range(3):
    batch.run(176400, stereo=False, fetch=False)
batch.sync()
np.save(sys.argv[2], batch.device_tensor(176400, False).cpu().numpy().reshape(-1))
batch.close()
print("view ok")
"""


def test_the_last_run_through_the_device_view(bank, tmp_path, monkeypatch):
    """No run is fetched; after sync() the rows on the device, read through Batch.device_tensor, are the oracle's third run. In
    a process of its own: torch has to be imported before the library is loaded, and in this one the library is loaded already."""
    prg, want = bank
    _env(monkeypatch, "alternate")
    out = str(tmp_path / "last.npy")
    run = subprocess.run([sys.executable, "-c", VIEW, ROOT, out], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "view ok" in run.stdout, run.stderr[-3000:]
    assert (np.load(out) == want[2 * RUN:]).all()


CONSUMER = r"""
import sys
import numpy as np
import torch  # (before the library: torch's wheel brings a HIP runtime of its own, and a process has room for one -- api.Batch.device_tensor)
sys.path.insert(0, sys.argv[1])
import saugns_amd as sa
from saugns_amd import voicebank as vb
sa.set_piluts(np.fromfile(sys.argv[1] + "/tests/golden/piluts_ref.f32", dtype="<f4").reshape(12, 2048))
voices = vb.config3_voices(96, 12)
for i, v in enumerate(voices):
    v.pan = vb.Line(vb._num(".2f", ((i * 37) % 100) / 100.0))
batch = sa.Batch([vb.build_program(voices)], 44100)
outs = []
for r in range(3):
    batch.run(176400, stereo=False, fetch=False)
    # the contract (include/saugns_amd.h): the stream is asked for again after the run whose rows are read on the device
    stream = torch.cuda.ExternalStream(batch._L.sauAmd_Batch_stream(batch._b))
    rows = batch.device_tensor(176400, False)
    with torch.cuda.stream(stream):
        outs.append(rows.clone())  # a consumer's kernel on the batch's stream: no sync() in between
torch.cuda.synchronize()
np.save(sys.argv[2], torch.cat([o.reshape(-1) for o in outs]).cpu().numpy())
batch.close()
print("consumer ok")
"""


def test_a_consumer_ordered_on_the_batchs_stream_sees_the_finished_rows(bank, tmp_path, monkeypatch):
    """The device-side contract: a kernel of the caller's on the stream sauAmd_Batch_stream hands out AFTER a run reads that
    run's finished rows, without a host-side wait -- the call joins the run's mixer, which is on the side stream, onto the stream
    it returns. Three unfetched runs, each copied by a consumer on the stream while the next run is issued behind it: the
    oracle's PCM. In a process of its own, for torch (which is the consumer) has to be imported before the library."""
    prg, want = bank
    _env(monkeypatch, "alternate", poison=False)
    out = str(tmp_path / "rows.npy")
    run = subprocess.run([sys.executable, "-c", CONSUMER, ROOT, out], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "consumer ok" in run.stdout, run.stderr[-3000:]
    assert (np.load(out) == want).all()
    lines = [m for m in LINE.finditer(run.stderr)]
    assert [m.group(4) for m in lines] == ["side"] * 3 and "stream_handle:1:" in lines[1].group(6) and "stream_handle:2:" in lines[2].group(6), run.stderr[-2000:]


@pytest.mark.parametrize("stereo", [False, True])
@pytest.mark.parametrize("mode", ["alternate", "shared"])
def test_a_run_of_several_segments(sa, oracle, capfd, monkeypatch, mode, stereo):
    """Later events cut one run of 12 s into three segments (4 s each: shorter ones have too few tasks for the launch to mix tiles
    itself, and keep the serial order), each with its own PCM offset, on the run's one block of rows (and, with rows
    of its own, the second): the oracle's PCM, mono and stereo. With shared rows each segment from the second on waits once, in
    front of its first writer of rows, for the mixer of the segment before; with rows of its own a segment waits where it first
    touches PCM or a set's records, for no mixer twice."""
    from saugns_amd import voicebank as vb
    oracle.oracle().ora_set_fastmath_forms(ORACLE_FORMS)
    voices = vb.config3_voices(96, 12)
    for i, v in enumerate(voices):
        v.pan = vb.Line(vb._num(".2f", ((i * 29) % 100) / 100.0))
    ups = [(4000, 3, voices[3], {"amp": vb.Line(0.5)}), (8000, 40, voices[40], {"amp": vb.Line(0.25)})]
    prg = vb.build_program(voices, updates=ups)
    want = oracle.oracle_render(prg.ptr, 44100, stereo, chunk=3 * RUN)
    _env(monkeypatch, mode, poison=False)
    batch = sa.Batch([prg], 44100)
    got = batch.run(3 * RUN, stereo=stereo)[0][0]
    batch.close()
    assert (np.asarray(got).reshape(-1)[:len(want)] == want).all()
    reps, _ = _reports(capfd)
    assert len(reps) == 3 and [r[1] for r in reps] == [0, 1, 0] and sum(r[3] == "side" for r in reps) >= 2, reps
    seen, tickets = [], 0
    for i, (m, st, b, mixer, ticket, waits) in enumerate(reps):
        assert (m, mixer) in ((mode, "side"), ("off", "main")) and b == (st if m == "alternate" else 0), (i, reps)
        # (nothing but the tracker's own points waits inside a run, never for a mixer twice, never for one not yet launched)
        assert all(w in ("pcm", "rows", "records", "mixer") and t <= tickets for w, t, d in waits), (i, reps)
        seen += [t for w, t, d in waits]
        if i and reps[i - 1][3] == "side" and mode == "shared" and mixer == "side":
            # the segment's first writer of rows waits for the mixer of the segment before, which reads them
            assert [w[:2] for w in waits] == [("rows", tickets)], (i, reps)
        if mixer == "side":
            tickets += 1
            assert ticket == tickets, (i, reps)
    assert len(seen) == len(set(seen)), reps


def test_a_refused_second_block_means_shared_rows(sa, bank, capfd, monkeypatch):
    """SAU_AMD_MIX_OVERLAP_FAIL: the second block of rows is not to be had when the second run asks for it -- shared rows from
    there on, the same PCM."""
    prg, want = bank
    _env(monkeypatch, "alternate", SAU_AMD_MIX_OVERLAP_FAIL="1")
    batch = sa.Batch([prg], 44100)
    for r in range(3):
        got = batch.run(RUN, stereo=False)[0][0]
        assert (np.asarray(got) == want[r * RUN:(r + 1) * RUN]).all(), r
    batch.close()
    reps, _ = _reports(capfd)
    assert [(m, s, b, mixer) for m, s, b, mixer, t, w in reps] == [("alternate", 0, 0, "side"), ("shared", 1, 0, "side"), ("shared", 0, 0, "side")], reps


def test_voices_the_block_loop_renders(sa, oracle, capfd, monkeypatch):
    """Nonzero guard words: the segment's mixer mixes every frame, whatever the launches mixed. (i) tests/test_gpu_inmix.py's bank
    of voices of two depths: premix_kernel says that the launch cannot mix (guard[1] != 0), and the mixer -- on the side stream,
    reading the guard of its segment's set while the next run's analyze_kernel clears the other set's -- takes all of it. (ii) that
    file's voices with a line the host took for one value (SAU_AMD_LEAN_IDS_LIE): decode_kernel sends them to the block loop
    (guard[0] != 0); running-sum voices, whose launches do not mix, so the serial order. Three runs each, only the later ones
    fetched: the oracle's PCM."""
    from saugns_amd import voicebank as vb
    oracle.oracle().ora_set_fastmath_forms(ORACLE_FORMS)
    voices = vb.config3_voices(64, 12) + [vb.Op("sin", freq=vb._num(".4f", 55.0 * (1 + i)), time_ms=12000) for i in range(32)]
    prg = vb.build_program(voices)
    want = oracle.oracle_render(prg.ptr, 44100, False, chunk=RUN)
    for mode in ("alternate", "shared"):
        _env(monkeypatch, mode, poison=False, SAU_AMD_INMIX_REPORT="1")
        batch = sa.Batch([prg], 44100)
        batch.run(RUN, stereo=False, fetch=False)
        got = [batch.run(RUN, stereo=False)[0][0].copy() for _ in range(2)]
        batch.close()
        assert (np.concatenate(got) == want[RUN:]).all(), mode
        reps, err = _reports(capfd)
        _check_sides(reps, mode, 3)
        guards = [int(g) for g in re.findall(r"inmix: .* guard \d+ (\d+)", err)]
        assert len(guards) == 3 and all(guards), (guards, err[-2000:])

    def voice(i):
        m3 = vb.Op("sin", freq=vb.Line(3.0, ratio=True), amp=vb._f32(0.4))
        m2 = vb.Op("sin", freq=vb.Line(2.0, goal=5.0, ratio=True), amp=vb._f32(0.7), mods={vb.POP_PMOD: [m3]})
        m1 = vb.Op("sin", freq=vb.Line(1.0, ratio=True), amp=20.0 + i, amp2=vb.Line(40.0), mods={vb.POP_PMOD: [m2]})
        return vb.Op("sin", freq=vb._num(".2f", 110.0 + 3.7 * i), freq2=vb.Line(vb._num(".2f", 220.0 + i), goal=330.0), time_ms=1500,
                     mods={vb.POP_FMOD: [m1]})

    prg = vb.build_program([voice(i) for i in range(24)])
    want = oracle.oracle_render(prg.ptr, 44100, False, chunk=22050)
    assert len(want) == 3 * 22050
    _env(monkeypatch, "alternate", SAU_AMD_LEAN_IDS_LIE="1")
    batch = sa.Batch([prg], 44100)
    batch.run(22050, stereo=False, fetch=False)
    got = [batch.run(22050, stereo=False)[0][0].copy() for _ in range(2)]
    batch.close()
    assert (np.concatenate(got) == want[22050:]).all()
    reps, _ = _reports(capfd)
    assert [(r[0], r[3]) for r in reps] == [("off", "main")] * 3, reps


def test_a_side_stream_mixer_behind_a_block_loop_with_work(sa, oracle, capfd, monkeypatch):
    """guard[0] != 0 read by a mixer on the side stream: tests/test_gpu_lanemajor_ops.py's bank of phase steps of zero, which takes
    the edge and inner launches, with the repair pass off (SAU_AMD_NO_REPAIR) -- every noted group sends its voice to the block
    loop, whose work list is counted in the guard's first word, in the segment's set. The mixer mixes every frame while the next
    run's analyze_kernel clears the other set's word. Three runs, the first unfetched: the oracle's PCM."""
    from saugns_amd import voicebank as vb
    from test_gpu_lanemajor_ops import zero_step_bank
    oracle.oracle().ora_set_fastmath_forms(ORACLE_FORMS)
    prg = vb.build_program(zero_step_bank(96, 12000))
    want = oracle.oracle_render(prg.ptr, 44100, True, chunk=RUN)
    for mode in ("alternate", "shared"):
        _env(monkeypatch, mode, poison=False, SAU_AMD_INMIX_REPORT="1", SAU_AMD_NO_REPAIR="1")
        batch = sa.Batch([prg], 44100)
        batch.run(RUN, stereo=True, fetch=False)
        got = [batch.run(RUN, stereo=True)[0][0].copy() for _ in range(2)]
        batch.close()
        assert (np.concatenate(got) == want[2 * RUN:]).all(), mode
        reps, err = _reports(capfd)
        _check_sides(reps, mode, 3)
        guards = [int(g) for g in re.findall(r"inmix: .* guard (\d+) \d+", err)]
        assert len(guards) == 3 and guards[0] and guards[1], (guards, err[-2000:])


def _levels_and_pcm(sa, prg, monkeypatch, mode):
    _env(monkeypatch, mode)
    batch = sa.Batch([prg], 44100)
    batch.set_metering(True)
    a = batch.run(RUN, stereo=True)[0].copy()
    la = [l.as_dict() for l in batch.levels(reset=True)]
    b = batch.run_f32(RUN, stereo=True)[0].copy()
    lb = [l.as_dict() for l in batch.levels(reset=True)]
    batch.run(RUN, stereo=True, fetch=False)
    lc = [l.as_dict() for l in batch.levels()]
    batch.close()
    return a, la, b, lb, lc


def test_metering_and_a_float_run_after_an_int16_run(sa, bank, capfd, monkeypatch):
    """One batch, metering on: an int16 run (its mixer on the side stream), a float run (set_format re-sizes the rows' samples; no
    launch mixes floats, so the serial order), an int16 run nobody fetches. measure_streams is what waits for the first run's mixer
    and reads the finished PCM: levels and PCM equal the serial order's."""
    prg, _ = bank
    on = _levels_and_pcm(sa, prg, monkeypatch, "alternate")
    reps, _ = _reports(capfd)
    assert [r[3] for r in reps] == ["side", "main", "side"] and reps[0][5] == [], reps
    assert [w[:2] for w in reps[1][5]] == [("measure_streams", 1)], reps
    off = _levels_and_pcm(sa, prg, monkeypatch, "off")
    assert on[0].any() and (on[0] == off[0]).all() and (on[2].view(np.uint32) == off[2].view(np.uint32)).all()
    assert on[1] == off[1] and on[3] == off[3] and on[4] == off[4]
    assert on[4][0]["frames"] == RUN


def test_two_batches_one_ordered_after_the_other(sa, bank, capfd, monkeypatch):
    """order_after joins the first batch's pending mixer before its event is recorded -- the report of the first batch's next
    segment shows that wait, for the unfetched run's ticket -- so that "everything issued for the first batch" includes its
    mixer: the second batch's PCM is the oracle's, and the first's, fetched afterwards by a run of its own, too."""
    prg, want = bank
    _env(monkeypatch, "alternate", poison=False)
    a, b = sa.Batch([prg], 44100), sa.Batch([prg], 44100)
    a.run(RUN, stereo=False, fetch=False)
    b.order_after(a)
    got_b = b.run(RUN, stereo=False)[0][0]
    got_a = a.run(RUN, stereo=False)[0][0]
    a.close()
    b.close()
    assert (np.asarray(got_b) == want[:RUN]).all() and (np.asarray(got_a) == want[RUN:2 * RUN]).all()
    reps, _ = _reports(capfd)
    # a's first run, b's run, a's second run: the one wait for a's first mixer is order_after's, not the second run's own
    assert [(r[3], r[4]) for r in reps] == [("side", 1), ("side", 1), ("side", 2)], reps
    assert reps[0][5] == [] and reps[1][5] == [] and [w[:2] for w in reps[2][5]] == [("order_after", 1)], reps


def _two_runs(sa, prgs, frames, monkeypatch, mode):
    _env(monkeypatch, mode)
    batch = sa.Batch(prgs, 44100)
    batch.run(frames, stereo=False, fetch=False)
    pcm = batch.run(frames, stereo=False)[0].copy()
    batch.close()
    return pcm


def test_many_streams_of_a_few_voices_and_a_feedback_bank(sa, capfd, monkeypatch):
    """mix_few_kernel (16 streams x 4 voices) and the early mixers of a feedback bank (config 5's voices, chains in chunks), two
    runs each, the first unfetched. No launch of theirs mixes tiles itself, so plan_mix_overlap leaves them on the serial order
    (beside their rendering launches the mixer measured slower): every mixer on the main stream, the PCM the same with the
    switches as without."""
    from saugns_amd import voicebank as vb
    few = [vb.build_program([vb.Op("sin", freq=110.0 + 13.0 * s + 3.1 * v, time_ms=2000) for v in range(4)]) for s in range(16)]
    feedback = [vb.build_program(vb.config5_voices(64, 2))]
    for prgs, frames in ((few, 30000), (feedback, 44100)):
        off = _two_runs(sa, prgs, frames, monkeypatch, "off")
        capfd.readouterr()
        assert off.any()
        for mode in ("alternate", "shared"):
            on = _two_runs(sa, prgs, frames, monkeypatch, mode)
            reps, _ = _reports(capfd)
            assert reps and all((r[0], r[3], r[5]) == ("off", "main", []) for r in reps), reps
            assert (on == off).all(), mode
