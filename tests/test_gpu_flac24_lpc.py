"""The LPC mode of the 24-bit FLAC encoder on the device (include/saugns_amd.h, section "FLAC", paragraph "LPC at 24 bits":
sauAmd_Batch_create_flac_lpc24, sauAmd_render_file_flac_lpc24, sauAmd_render_file_flac_loudness_lpc24; kernels:
saugns_amd/csrc/k_flac.h -- flac_analyze_kernel<FlacS32, true> and flac_write_kernel<FlacS32, true>).

The bytes are a function of the fed floats, the gains and (B, channels, M) only, so what the device delivers is compared BYTE
FOR BYTE with the library's host restatement (sauAmd_flac_quantize, then sauAmd_flac_encode_block_lpc24 block by block) and with
the numpy model (tests/flac24_lpc_model.py), whose independent decoder reads the device's streams back to the quantised floats;
a sequence cut into feeds of any lengths is compared with itself in one piece. Step 5b's shared function is run as compiled
for gfx950 (tests/hooks_flac24_lpc) over the host test's vectors."""
import hashlib
import os
import subprocess
import sys
import traceback

import numpy as np
import pytest

import flac24_lpc_model as mdl
import test_flac24_lpc_host as host
from conftest import load_program
from test_gpu_flac24 import info_of, stage

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALE = 8388607.0


def as_f32(s):
    """int samples (|s| <= 8388607) -> the floats whose pcm24 values they are: the division's rounding error times 8388607 is
    below half a step"""
    x = (np.asarray(s, np.float64) / SCALE).astype(np.float32)
    assert (mdl.quantize(x) == np.asarray(s)).all()
    return x


def block_f32(kind, B, ch, seed):
    """one block of float material: "pm"; "ar<p>" (mono: that process; stereo: it and the process of order 9 - p); "guard" (B = 256
    stereo: flac24_lpc_model.guard_stream); or one of flac24_model's crafted kinds -- the rails and one_loud among them"""
    if kind == "pm":
        return mdl.pm_f32(2 * B, ch, seed=1 + seed)[B * ch:]
    if kind == "guard":
        assert (B, ch) == (256, 2)
        return as_f32(mdl.guard_stream())
    if kind.startswith("ar"):
        p = int(kind[2:])
        return as_f32(mdl.rows(mdl.ar(p, B, p + seed)) if ch == 1 else mdl.rows(mdl.ar(p, B, p + seed), mdl.ar(9 - p, B, 40 + p + seed)))
    return mdl.crafted_f32(kind, B, ch, seed=seed, B=B)


def row_f32(kinds, B, ch, tail, seed):
    """whole blocks of the kinds named and `tail` frames of the PM voice, with floats out of range and a NaN sown into the tail"""
    parts = [block_f32(k, B, ch, seed + i) for i, k in enumerate(kinds)]
    if tail:
        t = mdl.pm_f32(tail, ch, seed=3).copy()
        t[0], t[-1] = np.nan, 1.5
        parts.append(t)
    return np.concatenate(parts) if parts else np.zeros(0, np.float32)


def host_stream(sa, x, gain, ch, B, M):
    """the host restatement of a whole row -> (the bytes, the frames' sizes, the quantised samples)"""
    q = sa.flac_quantize(x, gain, 24)
    out, sizes = [], []
    for k in range((len(q) // ch + B - 1) // B):
        f = sa.flac_encode_block_lpc24(q[k * B * ch:(k + 1) * B * ch], ch, B, k, M)
        assert f, ("the host refuses block", k)
        out.append(f)
        sizes.append(len(f))
    return b"".join(out), sizes, q


def check_row(sa, data, x, gain, ch, B, M, info, what, stat=None):
    """device == host == model, the decoder returns the quantised floats, no frame is longer than with M = 0 -> the kinds"""
    want, sizes, q = host_stream(sa, x, gain, ch, B, M)
    assert len(data) == len(want), (what, len(data), len(want))
    if data != want:
        at = next(i for i in range(len(want)) if data[i] != want[i])
        raise AssertionError((what, "first difference at byte", at, "of", len(want), data[at:at + 8].hex(), want[at:at + 8].hex()))
    assert (q == mdl.quantize(x, gain)).all(), what
    model = b"".join(mdl.encode_block(q[k * B * ch:(k + 1) * B * ch], ch, B, k, M, stat=stat) for k in range(len(sizes)))
    assert data == model, (what, "the model")
    got, s2, kinds = mdl.decode_frames(data, ch, B)
    assert s2 == sizes and (got.astype(np.int64) == q).all(), what
    assert info == info_of(len(x) // ch, sizes), (what, info, info_of(len(x) // ch, sizes))
    plain = host_stream(sa, x, gain, ch, B, 0)[1]
    assert len(plain) == len(sizes) and all(a <= b for a, b in zip(sizes, plain)), (what, sizes, plain)
    assert all(o <= M for o in mdl.lpc_orders_seen(kinds)), (what, kinds)
    return kinds


def encode_twice(torch, b, rows, gains, ch, B, M, extra):
    """one encoder, the rows in one feed with finish, twice behind a reset -> (the rows' bytes, their records)"""
    frames = [len(x) // ch for x in rows]
    keep, out = [], []
    e = b.create_flac_lpc24(len(rows), ch, B, M)
    for _ in range(2):
        ptr, pitch = stage(torch, keep, rows, extra=extra)
        e.feed_f32(ptr, pitch, frames, gains, finish=True)
        need, info_q = e.unread()
        data, info = e.read(reset=True)
        assert need == [len(d) for d in data] and info_q == info
        out.append(data)
    e.close()
    assert out[0] == out[1], ("called twice", B, ch, M)
    return out[0], info


GAINS = [1.0, 0.5, 1.0, -0.83]


# ---- 1. every order at B = 256, the other block sizes, the guard stream -----------------------------------------------------

def bytes_main(torch, sa, b):
    seen = {}
    configs = []
    for M in range(1, 9):
        for ch in (1, 2):
            kinds = ["ar%d" % p for p in range(1, 9)] if M == 8 else ["ar%d" % M, "pm", "ar%d" % min(M + 1, 8)]
            second = (["guard"] if ch == 2 and M == 8 else []) + ["rails", "one_loud", "pm", "anti_rails"]
            configs.append((256, ch, M, kinds, second))
    configs += [(512, 2, 8, ["ar5", "pm", "ar2"], ["one_loud", "pm", "rails"]), (1024, 2, 5, ["ar5", "pm", "ar8"], ["rails", "pm", "one_loud"]),
                (2048, 2, 3, ["ar3", "pm", "ar1"], ["pm", "one_loud", "rails"]), (4096, 2, 8, ["ar8", "pm", "ar4"], ["one_loud", "pm", "rails"]),
                (4096, 1, 8, ["pm", "ar6", "noise"], ["ar3", "pm", "quiet_sine"])]
    for case, (B, ch, M, first, second) in enumerate(configs):
        x = [row_f32(first, B, ch, 37, case), np.zeros(0, np.float32), row_f32(second, B, ch, 5, case + 50), row_f32(["pm"], B, ch, B - 1, case)]
        data, info = encode_twice(torch, b, x, GAINS, ch, B, M, 4 * (1 + case % 3))
        assert data[1] == b"" and info[1] == info_of(0, [])
        for r in (0, 2, 3):
            stat = {}
            kinds = check_row(sa, data[r], x[r], GAINS[r], ch, B, M, info[r], ("B", B, "ch", ch, "M", M, "row", r), stat)
            seen.setdefault((B, ch, M), set()).update(mdl.lpc_orders_seen(kinds))
            if r == 2 and "guard" in second:  # step 5b took the side channel's order 8 out of the first block, and nothing else
                assert (25, 8) in stat["guarded"] and all(g == (25, 8) for g in stat["guarded"]), stat
                print("the guard stream: guarded", stat["guarded"], "kinds", kinds[0])
    for key in sorted(seen):
        print("LPC orders chosen on the device at B, channels, M = %s: %s" % (key, sorted(seen[key])))
    assert seen[(256, 1, 8)] == set(range(1, 9)) and seen[(256, 2, 8)] == set(range(1, 9)), seen
    for M in range(1, 8):
        for ch in (1, 2):
            assert M in seen[(256, ch, M)], (M, ch, seen[(256, ch, M)])
    assert all(seen[k] for k in seen), seen
    print("cases:", len(configs))


# ---- 2. feeds ---------------------------------------------------------------------------------------------------------------

def cuts_main(torch, sa, b):
    for B, ch, M in ((256, 2, 8), (1024, 1, 6)):
        lengths = [5 * B + 37, 0, 4 * B, 3 * B + 1]
        gains = [0.9, 1.0, -0.25, 1.0]
        x = [row_f32((["pm", "ar7", "rails", "ar3", "one_loud", "pm"] * 2)[r:r + n // B], B, ch, n % B, 10 + r) for r, n in enumerate(lengths)]
        assert [len(r) // ch for r in x] == lengths
        pieces = [1, 255, 257, B + 1, 6 * B]
        e = b.create_flac_lpc24(4, ch, B, M)
        keep, got, cur = [], [b""] * 4, [0] * 4
        for i, n in enumerate(pieces):
            last = i == len(pieces) - 1
            fr = [0 if (i + r) % 5 == 4 and not last else min(n, lengths[r] - cur[r]) for r in range(4)]
            ptr, pitch = stage(torch, keep, [x[r][cur[r] * ch:(cur[r] + fr[r]) * ch] for r in range(4)])
            e.feed_f32(ptr, pitch, fr, gains, finish=last)
            for r in range(4):
                cur[r] += fr[r]
            if i % 2 == 1 or last:  # reads in between: what is complete so far, nothing twice
                data, info = e.read()
                for r in range(4):
                    got[r] += data[r]
                    assert info[r]["frames"] == cur[r] and info[r]["bytes"] == len(got[r])
        assert cur == lengths
        _, info = e.read()
        seen = set()
        for r in (0, 2, 3):
            seen |= mdl.lpc_orders_seen(check_row(sa, got[r], x[r], gains[r], ch, B, M, info[r], ("cuts", B, ch, r)))
        assert seen, (B, ch)
        for _ in range(2):  # in one piece, twice behind a reset: the same bytes
            e.read(reset=True)
            ptr, pitch = stage(torch, keep, x)
            e.feed_f32(ptr, pitch, lengths, gains, finish=True)
            data, info2 = e.read()
            assert data == got and info2 == info, ("one piece", B, ch)
        e.close()


# ---- 3. MD5; order 0; what the other entry point still refuses ------------------------------------------------------------------

def md5_main(torch, sa, b):
    B, ch, M = 256, 2, 8
    x = [row_f32(["pm", "ar4", "pm"], B, ch, 100, 60), np.zeros(0, np.float32), row_f32(["ar8"], B, ch, 0, 61)]
    gains = [0.7, 1.0, -1.0]
    frames = [len(r) // ch for r in x]
    keep = []
    e = b.create_flac_lpc24(3, ch, B, M)
    ptr, pitch = stage(torch, keep, x)
    e.feed_f32(ptr, pitch, frames, gains, finish=True)
    plain, _ = e.read(reset=True)
    e.set_md5(True)
    e.feed_f32(ptr, pitch, [B + 1, 0, 7], gains)
    ptr2, pitch2 = stage(torch, keep, [x[0][(B + 1) * ch:], x[1], x[2][7 * ch:]])
    e.feed_f32(ptr2, pitch2, [frames[0] - B - 1, 0, frames[2] - 7], gains, finish=True)
    data, info = e.read()
    digests = e.md5()
    e.close()
    assert data == plain  # MD5 changes no byte
    for r in range(3):
        q = sa.flac_quantize(x[r], gains[r], 24)
        raw = b"".join(int(v).to_bytes(3, "little", signed=True) for v in q)
        assert digests[r] == hashlib.md5(raw).digest(), r
        assert digests[r] == sa.flac_md5(q, 24)


def order0_main(torch, sa, b):
    for B, ch in ((256, 2), (4096, 1)):
        x = [row_f32(["pm", "rails", "ar5"], B, ch, 37, 70), row_f32(["one_loud"], B, ch, 1, 71)]
        frames = [len(r) // ch for r in x]
        keep, out = [], []
        for make in (lambda: b.create_flac_lpc24(2, ch, B, 0), lambda: b.create_flac_f32(2, ch, B, bits=24)):
            e = make()
            ptr, pitch = stage(torch, keep, x)
            e.feed_f32(ptr, pitch, frames, [0.5, 1.0], finish=True)
            out.append(e.read())
            e.close()
        assert out[0] == out[1], ("order 0", B, ch)
        for r in range(2):
            want = b"".join(sa.flac_encode_block_s32(sa.flac_quantize(x[r], [0.5, 1.0][r], 24)[k * B * ch:(k + 1) * B * ch], ch, B, k, bits=24)
                            for k in range((frames[r] + B - 1) // B))
            assert out[0][0][r] == want, ("order 0 against the host", B, ch, r)

    def refused(fn, *args, **kw):
        try:
            fn(*args, **kw)
        except RuntimeError as err:
            assert "bad argument" in str(err), (args, err)
        else:
            raise AssertionError(("not refused", args, kw))

    for M in (1, 8):  # the entry point that takes `bits` keeps refusing, on this backend too
        refused(b.create_flac_f32, 2, 2, 256, bits=24, max_lpc_order=M)
    for args in ((0, 1, 256, 8), (65536, 1, 256, 8), (1, 0, 256, 8), (1, 3, 256, 8), (1, 1, 255, 8), (1, 1, 256, 9)):
        refused(b.create_flac_lpc24, *args)
    e = b.create_flac_lpc24(1, 1, 256, 8)  # an encoder of one kind: fed floats
    keep = []
    q = np.zeros(64, np.int16)
    t = torch.from_numpy(q).to("cuda")
    keep.append(t)
    refused(e.feed, t.data_ptr(), 128, [8])
    e.close()


SECTIONS = [("bytes", bytes_main), ("cuts", cuts_main), ("md5", md5_main), ("order0", order0_main)]


def torch_main():
    """(in a process of its own, torch imported first: tests/test_gpu_flac24.py's fixture) every section on one batch's device; a
    section that fails ends the process -- nothing more is started on the device behind a failure"""
    import torch
    import saugns_amd as sa
    from saugns_amd import voicebank as vb
    b = sa.Batch([vb.build_program([vb.Op("sin", freq=200.0, time_ms=10)])], 44100)  # (never run: its device is all that is used)
    for name, fn in SECTIONS:
        try:
            fn(torch, sa, b)
        except Exception:
            print("flac24 lpc %s FAILED\n%s" % (name, traceback.format_exc()))
            break
        print("flac24 lpc %s ok" % name)
    b.close()


TORCH = r"""
import sys
import torch  # (before the library: tests/test_gpu_flac24.py)
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_flac24_lpc
test_gpu_flac24_lpc.torch_main()
"""


@pytest.fixture(scope="module")
def torch_run():
    run = subprocess.run([sys.executable, "-c", TORCH, ROOT], capture_output=True, text=True, timeout=600)
    print(run.stdout[-6000:])
    return run


def _section(run, name):
    assert "flac24 lpc %s ok" % name in run.stdout, (run.returncode, run.stdout[-4000:], run.stderr[-4000:])


def test_device_bytes_equal_the_hosts_and_the_models(torch_run):
    """4 rows per feed -- 3 or 8 blocks + 37 frames, none, 4 or 5 blocks + 5, one block + B - 1 --, gains 1, 0.5, 1, -0.83, POISON
    between the rows. B = 256 with every max_lpc_order 1 .. 8, mono and stereo: all-pole processes whose best predictor has a
    known order (all eight at M = 8: every order is chosen), the PM voice, the rails, one loud partition, L = -R at the rails,
    and in the stereo M = 8 case the stream on which step 5b takes the side channel's order 8. One stereo case each at B = 512,
    1024 and 2048, and B = 4096 stereo and mono with M = 8, the LDS maximum. The bytes equal the host restatement's and the
    model's, the model's decoder returns sauAmd_flac_quantize of the floats with the row's gain, no frame is longer than with
    M = 0, and two identical feeds give identical bytes."""
    _section(torch_run, "bytes")


def test_cuts(torch_run):
    """four rows of unequal length, one empty, distinct gains, cut into feeds of 1, 255, 257 and B + 1 frames and the rest, some
    rows given nothing in some feeds, with reads in between: the same bytes as in one piece, twice behind a reset, and as the host's
    and the model's; B = 256 stereo with M = 8 and B = 1024 mono with M = 6."""
    _section(torch_run, "cuts")


def test_md5_of_the_unencoded_samples(torch_run):
    """MD5 on, two feeds: the digests are hashlib's of the quantised samples as 3-byte little-endian integers, and no byte of
    the frames changes"""
    _section(torch_run, "md5")


def test_order_0_is_the_float_fed_encoder_and_the_old_entry_point_refuses(torch_run):
    """sauAmd_Batch_create_flac_lpc24(.., 0) and sauAmd_Batch_create_flac_f32(.., 24, 0) give equal bytes and records;
    sauAmd_Batch_create_flac_f32 refuses (24, M > 0) as before; bad arguments; an int16 feed"""
    _section(torch_run, "order0")
    assert torch_run.returncode == 0, (torch_run.stdout[-2000:], torch_run.stderr[-4000:])


# ---- 4. step 5b as compiled for gfx950 ---------------------------------------------------------------------------------------------

@pytest.mark.timeout(120)
def test_the_device_guard_equals_the_hosts_and_the_models():
    """one launch: the pole vectors and test_flac_lpc_steps_host's, at bps 24 and 25, lane 0 of a wave each, q and shift in LDS"""
    L = host.guard_hooks_lib()
    items, want, n_pole = host.guard_items()
    got = host.run_guard(L.sauAmd_kat_flac_lpc_guard_device, items)
    assert got == host.run_guard(L.sauAmd_kat_flac_lpc_guard_host, items)
    assert got == want and got[:n_pole] != [it[0] for it in items[:n_pole]]


# ---- 5. the file writers ------------------------------------------------------------------------------------------------------

RATE = 8000
FILE_KEY = "devtests__voice-reuse"
WAV_F32, WAV_F32_HEADER = 3, 58


def frame_sizes(data):
    return mdl.decode_frames(data[42:], mdl.parse_header(data)["channels"], mdl.parse_header(data)["max_block"])[1]


@pytest.mark.parametrize("channels", [1, 2])
def test_render_file_flac_lpc24_holds_the_quantised_floats_and_is_never_longer(sa, tmp_path, channels):
    prg = load_program(sa, FILE_KEY)
    wav, flac, flac0, flacm = (str(tmp_path / n) for n in ("x.wav", "x.flac", "x0.flac", "xm.flac"))
    n = sa.render_file(prg, RATE, wav, WAV_F32, channels)
    x = np.frombuffer(open(wav, "rb").read(), "<f4", offset=WAV_F32_HEADER)
    frames, info = sa.render_file_flac_lpc24(prg, RATE, flac, channels, 1024, max_lpc_order=8, gain=0.5)
    frames0, info0 = sa.render_file_flac_f32(prg, RATE, flac0, channels, 1024, bits=24, gain=0.5)
    data, data0 = open(flac, "rb").read(), open(flac0, "rb").read()
    assert frames == frames0 == n == info.frames and len(x) == n * channels
    h, got, kinds = mdl.decode_file(data)  # (STREAMINFO is held against the frames there)
    assert (h["srate"], h["channels"], h["max_block"], h["bps"], h["frames"]) == (RATE, channels, 1024, 24, n)
    want = sa.flac_quantize(x, 0.5, 24)
    assert (got == want).all()
    assert data[:42] == sa.flac_header(RATE, channels, 1024, info, bits=24)
    s8, s0 = frame_sizes(data), frame_sizes(data0)
    assert len(s8) == len(s0) == info.blocks == info0.blocks and all(a <= b for a, b in zip(s8, s0)) and len(data) < len(data0)
    assert mdl.lpc_orders_seen(kinds)
    # M = 0 through the new writer is the sibling's file
    sa.render_file_flac_lpc24(prg, RATE, flacm, channels, 1024, max_lpc_order=0, gain=0.5)
    assert open(flacm, "rb").read() == data0
    # the file MD5 switch: the digest of the samples in the header, every other byte the same
    was = sa.set_flac_file_md5(True)
    try:
        sa.render_file_flac_lpc24(prg, RATE, flacm, channels, 1024, max_lpc_order=8, gain=0.5)
    finally:
        sa.set_flac_file_md5(was)
    md = open(flacm, "rb").read()
    digest = hashlib.md5(b"".join(int(v).to_bytes(3, "little", signed=True) for v in want)).digest()
    assert md[26:42] == digest and md[:26] == data[:26] and md[42:] == data[42:]
    mdl.decode_file(md, md5=digest)
    print("FLAC 24 bits M = 8 / M = 0 / WAV_F32: %d / %d / %d" % (len(data), len(data0), os.path.getsize(wav)))


@pytest.mark.parametrize("limited", [False, True])
def test_render_file_flac_loudness_lpc24_is_its_siblings_samples_in_fewer_bytes(sa, tmp_path, limited):
    prg = load_program(sa, FILE_KEY)
    channels = 2
    wav, flac, flac0, flacm = (str(tmp_path / n) for n in ("x.wav", "x.flac", "x0.flac", "xm.flac"))
    _, ld0, _ = sa.render_file_loudness(prg, RATE, wav, WAV_F32, channels, -23.0, 1.0)
    target, ceiling = ld0.integrated + 9.0, float(max(ld0.true_peak))
    a = sa.render_file_flac_loudness_lpc24(prg, RATE, flac, channels, 1024, max_lpc_order=8, target_lufs=target, max_true_peak=ceiling,
                                           limited=limited)
    z = sa.render_file_flac_loudness(prg, RATE, flac0, channels, 1024, bits=24, target_lufs=target, max_true_peak=ceiling, limited=limited)
    assert a[0] == z[0] and bytes(a[1]) == bytes(z[1]) and np.float32(a[2]).view(np.uint32) == np.float32(z[2]).view(np.uint32)
    if limited:
        assert bytes(a[3]) == bytes(z[3]) and a[3].limited > 0
    data, data0 = open(flac, "rb").read(), open(flac0, "rb").read()
    h, got, kinds = mdl.decode_file(data)
    h0, got0, _ = mdl.decode_file(data0)
    assert h["frames"] == h0["frames"] == a[0] and (got == got0).all() and np.abs(got).max() > 100000
    s8, s0 = frame_sizes(data), frame_sizes(data0)
    assert len(s8) == len(s0) and all(x <= y for x, y in zip(s8, s0)) and len(data) < len(data0)
    assert mdl.lpc_orders_seen(kinds)
    sa.render_file_flac_loudness_lpc24(prg, RATE, flacm, channels, 1024, max_lpc_order=0, target_lufs=target, max_true_peak=ceiling,
                                       limited=limited)
    assert open(flacm, "rb").read() == data0


def test_the_writers_refuse_before_there_is_a_file(sa, tmp_path):
    prg = load_program(sa, FILE_KEY)
    path = str(tmp_path / "x.flac")
    for kw in (dict(max_lpc_order=9), dict(block_frames=100), dict(channels=3), dict(gain=float("nan"))):
        a = dict(channels=1, block_frames=256, max_lpc_order=8, gain=1.0)
        a.update(kw)
        with pytest.raises(RuntimeError, match="bad argument"):
            sa.render_file_flac_lpc24(prg, RATE, path, **a)
        assert not os.path.exists(path)
    for kw in (dict(max_lpc_order=9), dict(block_frames=100), dict(max_true_peak=0.0)):
        a = dict(channels=1, block_frames=256, max_lpc_order=8, target_lufs=-20.0, max_true_peak=0.9)
        a.update(kw)
        for limited in (False, True):
            with pytest.raises(RuntimeError, match="bad argument"):
                sa.render_file_flac_loudness_lpc24(prg, RATE, path, limited=limited, **a)
            assert not os.path.exists(path)
    for M in (1, 8):  # the writers that take `bits` keep refusing
        with pytest.raises(RuntimeError, match="bad argument"):
            sa.render_file_flac_f32(prg, RATE, path, 1, 256, bits=24, max_lpc_order=M)
        assert not os.path.exists(path)
