"""The device's float rows (include/saugns_amd.h: sauAmd_Batch_run_f32, "the mixer's f32 accumulator stored as it stands") against
the oracle's float output (oracle/sau_oracle.c: ora_run_f32), bit for bit: every sample's 32 bits, where the int16 parity tests see
15 of the 24 significant ones, only a sign on the quarter of the random programs' samples that lie beyond +-1, and nothing of a
subnormal sum. tests/test_oracle_f32.py holds the float oracle itself from both sides -- against the int16 oracle and, scaled by
powers of two, against the compiled reference -- and makes the programs.

One rule of comparison (same_bits): equal bit patterns wherever the oracle's sample is not a NaN; where it is one, the device's is
a NaN too -- sign and payload are free there (x86 makes 0xFFC00000 of inf - inf, and a GPU need not). Both sides make calls of
the same size; every call's whole buffer, `more` and out_len are compared until the stream has ended."""
import os
import struct

import numpy as np
import pytest

import test_gpu_f32 as tf
import test_gpu_lanemajor_ops as tl
import test_gpu_range_guards as tg
import test_gpu_duo as td
import test_gpu_units as tu
import test_oracle_f32 as to
from conftest import ORACLE_FORMS, load_program
from saugns_amd import voicebank as vb
from test_gpu_f32 import quantise

pytestmark = pytest.mark.gpu

RATE = 44100


@pytest.fixture(autouse=True)
def forms(oracle):
    oracle.oracle().ora_set_fastmath_forms(ORACLE_FORMS)


def same_bits(got, want, what):
    """got: the device's float32 samples, want: the oracle's"""
    got, want = np.asarray(got, np.float32).reshape(-1), np.asarray(want, np.float32).reshape(-1)
    assert len(got) == len(want), (what, len(got), len(want))
    nan = np.isnan(want)
    g, w = got.view(np.uint32), want.view(np.uint32)
    bad = np.where(nan, ~np.isnan(got), g != w)
    d = np.flatnonzero(bad)
    if len(d):
        seen = int((quantise(got[d]) != quantise(want[d])).sum())
        raise AssertionError(f"{what}: {len(d)} of {len(got)} samples differ, first at sample {d[0]}: device {int(g[d[0]]):#010x} "
                             f"({got[d[0]]!r}) oracle {int(w[d[0]]):#010x} ({want[d[0]]!r}); {seen} of them differ after quantise() too")


def check_batch(sa, oracle, prgs, rate, stereo, chunk, what, max_calls=0, call_len=0):
    """`prgs` as the streams of one batch in float runs of `chunk` frames against the oracle's calls of `chunk` frames -- or, with
    call_len, each run of chunk frames against the oracle's calls of call_len frames (sauAmd_Batch_set_call_len)
    -> per stream the device's samples of [0, out_len) of every run, concatenated"""
    ch = 2 if stereo else 1
    per_run = chunk // call_len if call_len else 1
    assert not call_len or chunk % call_len == 0
    want = []
    for p in prgs:
        calls = oracle.oracle_calls_f32(p.ptr, rate, stereo, chunk=call_len or chunk, max_calls=max_calls * per_run)
        runs = []
        for k in range(0, len(calls), per_run):
            part = calls[k:k + per_run]
            buf = np.zeros(chunk * ch, np.float32)
            for j, (x, _, _) in enumerate(part):
                buf[j * len(x):(j + 1) * len(x)] = x
            # out_len as sauGenerator_run gives it: the whole buffer while more is to come, else the frames made
            runs.append((buf, part[-1][1], chunk if part[-1][1] else (len(part) - 1) * (call_len or chunk) + part[-1][2]))
        want.append(runs)
    b = sa.Batch(prgs, rate)
    try:
        if call_len:
            b.set_call_len(call_len)
        outs = [[] for _ in prgs]
        for k in range(max(len(w) for w in want)):
            pcm, more, lens = b.run_f32(chunk, stereo)
            assert pcm.dtype == np.float32
            for s, w in enumerate(want):
                if k < len(w):  # (a stream that has ended is not looked at again)
                    x, m, n = w[k]
                    assert (more[s], lens[s]) == (m, n), (what, "stream", s, "run", k, (more[s], lens[s]), (m, n))
                    same_bits(pcm[s], x, (what, "stream", s, "run", k))
                    outs[s].append(pcm[s, :n * ch].copy())
    finally:
        b.close()
    return [np.concatenate(o) for o in outs]


def check_against_int16(sa, prg, rate, stereo, chunk, x, what, call_len=0):
    """quantise(the float samples) == the int16 run of a fresh batch (the header: "the int16 sample of sauAmd_Batch_run is this
    one clamped and rounded")"""
    b = sa.Batch([prg], rate)
    if call_len:
        b.set_call_len(call_len)
    pcm = b.render(stereo=stereo, chunk=chunk)[0]
    b.close()
    q = quantise(x)
    assert len(q) == len(pcm), (what, len(q), len(pcm))
    d = np.flatnonzero(q != pcm)
    assert len(d) == 0, f"{what}: {len(d)} samples differ, first at {d[0]}: float {x[d[0]]!r} int16 {pcm[d[0]]}"


# ---- a. the corpus ---------------------------------------------------------------------------------------------------------

def _corpus_keys():
    import json
    from conftest import GOLDEN
    return sorted(json.load(open(os.path.join(GOLDEN, "index.json")))["corpus"])


CORPUS_BATCHES = [_corpus_keys()[i:i + 32] for i in range(0, len(_corpus_keys()), 32)]


@pytest.mark.parametrize("stereo", [True, False])
@pytest.mark.parametrize("part", range(len(CORPUS_BATCHES)))
def test_corpus(sa, oracle, index, part, stereo):
    """every corpus script, stereo at the corpus rate and mono at 8000 Hz, in batches of up to 32 streams: the first twelve
    calls of 11289 frames, or to the stream's end"""
    prgs = [load_program(sa, k) for k in CORPUS_BATCHES[part]]
    rate = index["corpus_rate"] if stereo else 8000
    check_batch(sa, oracle, prgs, rate, stereo, to.CORPUS_CALL, ("corpus", part), max_calls=to.CORPUS_CALLS)


# ---- b. random graphs, d. float against int16 ------------------------------------------------------------------------------

@pytest.mark.parametrize("part", range(4))
def test_random_operator_graphs(sa, oracle, part):
    """test_gpu_units.py's 64 random programs, each in its own mono or stereo, in runs of 4000 frames and cut into its own
    runs; sixteen programs to a batch where the format and run length are shared"""
    made = [to.random_graph(seed) for seed in range(16 * part, 16 * part + 16)]
    for stereo in (False, True):
        prgs = [p for p, st, _ in made if st == stereo]
        outs = check_batch(sa, oracle, prgs, RATE, stereo, 4000, ("random", part, stereo))
        for k, (p, x) in enumerate(zip(prgs, outs)):
            check_against_int16(sa, p, RATE, stereo, 4000, x, ("random", part, stereo, k))
    for k, (p, stereo, chunk) in enumerate(made):
        check_batch(sa, oracle, [p], RATE, stereo, chunk, ("random", 16 * part + k, chunk))


@pytest.mark.parametrize("part", range(4))
def test_random_graphs_with_later_events(sa, oracle, part):
    made = [to.later_event_graph(seed) for seed in range(12 * part, 12 * part + 12)]
    for stereo in (False, True):
        prgs = [p for p, st, _ in made if st == stereo]
        outs = check_batch(sa, oracle, prgs, RATE, stereo, to.WHOLE, ("later events", part, stereo))
        for k, (p, x) in enumerate(zip(prgs, outs)):
            check_against_int16(sa, p, RATE, stereo, to.WHOLE, x, ("later events", part, stereo, k))
    for k, (p, stereo, chunk) in enumerate(made):
        check_batch(sa, oracle, [p], RATE, stereo, chunk, ("later events", 12 * part + k, chunk))


@pytest.mark.parametrize("seed", tu.EXTREME_SEEDS)
def test_extreme_parameters(sa, oracle, seed):
    """test_gpu_units.py::test_extreme_parameters' programs at their own rate and call size (calls below 300 frames: one run
    of 1500 calls on the lattice of set_call_len), mono and stereo: sums far beyond +-1, infinities and NaN among them"""
    prg, rate, call = tu.extreme_program(seed)
    for stereo in (False, True):
        if call < 300:
            x = check_batch(sa, oracle, [prg], rate, stereo, call * 1500, ("extreme", seed, stereo), call_len=call)[0]
            check_against_int16(sa, prg, rate, stereo, call * 1500, x, ("extreme", seed, stereo), call_len=call)
        else:
            x = check_batch(sa, oracle, [prg], rate, stereo, call, ("extreme", seed, stereo))[0]
            check_against_int16(sa, prg, rate, stereo, call, x, ("extreme", seed, stereo))


# ---- c. the other builds ---------------------------------------------------------------------------------------------------

def _env_id(env):
    return ",".join(f"{k}={v}" for k, v in env.items()) or "default"


# (that test's own list of environments)
OTHER_BUILDS = list(tu.test_random_graphs_in_other_kernel_configurations.pytestmark[0].args[1])
assert len(OTHER_BUILDS) >= 18 and all(isinstance(e, dict) for e in OTHER_BUILDS)


@pytest.mark.parametrize("env", OTHER_BUILDS, ids=_env_id)
def test_random_graphs_in_other_kernel_configurations(sa, oracle, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for seed in range(100, 108):
        prg, stereo, chunk = to.later_event_graph(seed)
        check_batch(sa, oracle, [prg], RATE, stereo, chunk, (env, seed))


LM_CHUNK = 70001
LM_NEEDS = {"r": {"SAU_AMD_NO_SEQ": "1"}, "amod ramps": {"SAU_AMD_NO_SEQ": "1"}, "amp op ramps": {"SAU_AMD_NO_SEQ": "1"},
            "big pm ramps": {"SAU_AMD_NO_SEQ": "1"}, "amod ramps cub": {"SAU_AMD_NO_SEQ": "1"},
            "zero steps": {"SAU_AMD_NO_REPAIR": "1"}}
# what test_gpu_lanemajor_ops.py's tests say of the report's lines: every closed-form segment in the form asked for, some, or none
LM_INNER = {"events": "some"}
LM_INNER.update({name: "none" for name in tl._banks() if name.startswith("not inner: ")})


@pytest.mark.parametrize("name", sorted(tl._banks()))
def test_lane_major_and_row_major_forms(sa, oracle, capfd, monkeypatch, name):
    """tests/test_gpu_lanemajor_ops.py's programs (k_fast_group_lm.h is a second hand-written copy of the group evaluation), the
    banks that must not take the inner launch among them, under the switches of its tests: the first run of 70001 stereo frames
    in the lane-major and in the row-major form, and the report's line says which one ran"""
    monkeypatch.setenv("SAU_AMD_POISON", "1")
    monkeypatch.setenv("SAU_AMD_INNER_REPORT", "1")
    for k, v in LM_NEEDS.get(name, {}).items():
        monkeypatch.setenv(k, v)
    voices, ups = tl._banks()[name]()
    prg = vb.build_program(voices, updates=ups)
    for form in ("lane-major", "row-major"):
        if form == "row-major":
            monkeypatch.setenv("SAU_AMD_NO_LANEMAJOR", "1")
        capfd.readouterr()
        # (the events' bursts, whose segments go without the inner launch, begin in the second run)
        check_batch(sa, oracle, [prg], RATE, True, LM_CHUNK, (name, form), max_calls=3 if name == "events" else 1)
        err = capfd.readouterr().err
        lines = tl.INNER.findall(err)
        inner = LM_INNER.get(name, "all")
        if inner == "all":
            assert set(lines) == {form}, (name, form, "the inner launch ran as", lines)
        elif inner == "some":
            assert set(lines) == {form, "none"}, (name, form, "the inner launch ran as", lines)
        else:
            assert lines and set(lines) == {"none"}, (name, form, lines)


@pytest.mark.parametrize("env", tg.CLOSED_FORM, ids=_env_id)
def test_guard_programs_across_the_closed_form_builds(sa, oracle, monkeypatch, env):
    """tests/test_gpu_range_guards.py's programs (PM across 2^20 cycles, increments across 2^50 and 2^51, W and R feedback across
    their switches) at every closed-form build"""
    for k, v in env.items():
        monkeypatch.setenv("SAU_AMD_" + k, str(v))
    for name, voices in tg.guard_programs().items():
        check_batch(sa, oracle, [vb.build_program(voices)], RATE, name in ("pm", "fb"), tg.CHUNK, (name, env))


def test_a_bank_of_closed_form_and_look_back_voices(sa, oracle):
    """tests/test_gpu_duo.py's bank: closed-form and look-back waves in one launch"""
    check_batch(sa, oracle, [td._bank_of_both_kinds()], RATE, False, 88200, "duo bank")


@pytest.mark.parametrize("stereo", [False, True])
def test_feedback_chains_and_look_back(sa, oracle, stereo):
    """config 5's feedback voices (chain_kernel) and config 3's with FM (running sums, one pass with look-back): the first 11025 frames"""
    for name, prg in (("config5", vb.build_program(vb.config5_voices(256, 1))), ("config3_fm", vb.config3_fm(128, 1))):
        check_batch(sa, oracle, [prg], RATE, stereo, 11025, name, max_calls=1)


@pytest.mark.parametrize("stereo", [False, True])
def test_many_voice_mixer(sa, oracle, stereo):
    """mix_kernel_f32 over a full tile of 256 voices and a remainder of 44 (test_gpu_f32.py's bank)"""
    check_batch(sa, oracle, [tf._bank300(tf.BANK_AMP)], RATE, stereo, tf.BANK_FRAMES, "bank300", max_calls=1)


@pytest.mark.parametrize("stereo", [False, True])
def test_few_voice_streams(sa, oracle, stereo):
    """mix_few_kernel_f32 (test_gpu_f32.py's eight streams of two voices)"""
    check_batch(sa, oracle, tf._small_scripts(), RATE, stereo, 6000, "small scripts")


# ---- e. the edges ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(to.EDGES))
def test_edge_programs(sa, oracle, name):
    """subnormal sums (a flushing instruction would give zeros), sums beyond +-1 up to 3e38, infinities of both signs by their bits,
    NaN by the rule above; tests/test_oracle_f32.py asserts on the oracle that the programs reach these"""
    prg = to.edge_program(*to.EDGES[name])
    for stereo in (True, False):
        check_batch(sa, oracle, [prg], RATE, stereo, 4096, (name, stereo))


@pytest.mark.parametrize("stereo", [True, False])
def test_meters_on_a_row_of_infinities_and_nan(sa, oracle, stereo):
    """the device row of the (1e30, 1e30) program through the two meters: the levels record counts the oracle's non-finite samples,
    the loudness record is the restatement's (tests/loudness_model.py) fed the oracle's samples"""
    import loudness_model as lm
    from test_gpu_loudness import check_hops, check_record
    ch = 2 if stereo else 1
    prg = to.edge_program(*to.EDGES["infinite"])
    want, more, frames = oracle.oracle_calls_f32(prg.ptr, RATE, stereo, chunk=4096)[0]
    assert (more, frames) == (False, 2205)
    want = want[:frames * ch]
    b = sa.Batch([prg], RATE)
    try:
        pcm, more, lens = b.run_f32(4096, stereo)
        assert (more, lens) == ([False], [frames])
        same_bits(pcm[0, :frames * ch], want, "row")
        b.sync()
        ptr, pitch = b.device_pcm_f32(0), b.device_pcm_pitch()
        ld, hops = b.measure_loudness_rows(ptr, pitch, 1, frames, ch, RATE)
        lv = b.measure_rows(ptr, pitch, 1, True, frames, ch)[0]
    finally:
        b.close()
    bad = ~np.isfinite(want)
    assert bad.sum() > 1000
    assert int(lv.frames) == frames
    for c in range(ch):
        assert int(lv.nonfinite[c]) == int(bad[c::ch].sum()), (c, lv, int(bad[c::ch].sum()))
    m = lm.Meter(sa.loudness_filter(RATE), sa.truepeak_taps(), RATE // 10, ch)
    m.run(want)
    check_hops(hops[0], m, "row")
    check_record(sa, ld[0], m, "row")


# ---- f. float WAV ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("channels", [1, 2])
def test_float_wav_data(sa, oracle, tmp_path, channels):
    """the data bytes of a WAVE_FORMAT_IEEE_FLOAT file are the float oracle's samples on the writer's call lattice"""
    prg = load_program(sa, "examples__tests__panning")
    want = oracle.oracle_render_f32(prg.ptr, RATE, channels == 2, chunk=256 * RATE // 1000)
    path = str(tmp_path / "f32.wav")
    assert sa.render_file(prg, RATE, path, sa.api.SNDFILE_WAV_F32, channels) == len(want) // channels
    raw = open(path, "rb").read()
    cid, size = struct.unpack_from("<4sI", raw, 50)
    assert (cid, size) == (b"data", len(want) * 4) and len(raw) == 58 + size
    same_bits(np.frombuffer(raw, "<f4", offset=58), want, "samples")
