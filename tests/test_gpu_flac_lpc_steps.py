"""The LPC mode's steps 3 to 5 on the device (include/saugns_amd.h, section "FLAC", "The LPC mode"), and the product kernels
(saugns_amd/csrc/k_flac.h) at every block size and order and on blocks in which those steps find nothing.

Two halves that together hold the product. The probe (tests/hooks/kat_kernels.hip: kat_flac_lpc_orders_kernel) runs the shared
function flac_lpc_orders (sau_flac.h) as hipcc compiles it for gfx950 with the product's flags, on LDS arrays laid out like the
kernel's, over the vectors of tests/test_flac_lpc_steps_host.py, and compares g, the mask, q, shift and the work array a[] BIT
FOR BIT with tests/flac_lpc_model.py: a[] is where a fused multiply-add would show, which the bytes do not see. The stream
sections take flac_analyze_kernel<true> and flac_write_kernel<true> -- which hand that function exact integers -- through
B = 512, 1024 and 2048, every max_lpc_order at B = 256, every chosen order, a mask with a hole, the m == 0 path and
R[0] == 0, byte for byte against the model; the product kernel's own copy of the function is held through q, shift and the
bytes only. The materials and what the model says they reach are in tests/test_flac_lpc_steps_host.py."""
import os
import subprocess
import sys
import traceback

import pytest

import flac_lpc_model as mdl
import test_flac_lpc_steps_host as steps
from test_gpu_flac_lpc import check_row, material, stage
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the probe -----------------------------------------------------------------------------------------------------------------

@pytest.mark.timeout(120)
def test_the_device_probe_equals_the_model(hooks):
    """one launch: 1470 autocorrelations, lane 0 of a wave each"""
    vecs = steps.vectors()
    steps.check_probe(steps.run_probe(hooks.sauAmd_kat_flac_lpc_orders_device, vecs), vecs, steps.model_results(), "device")


# ---- 1. every block size and order ------------------------------------------------------------------------------------------

def encode_twice(torch, b, rows, ch, B, M, extra):
    """one encoder, the rows in one feed with finish, twice behind a reset -> (the rows' bytes, their records)"""
    frames = [len(x) // ch for x in rows]
    keep, out = [], []
    e = b.create_flac(len(rows), ch, B, max_lpc_order=M)
    for _ in range(2):
        ptr, pitch = stage(torch, keep, rows, ch, extra=extra)
        e.feed(ptr, pitch, frames, finish=True)
        need, info_q = e.unread()
        data, info = e.read(reset=True)
        assert need == [len(d) for d in data] and info_q == info
        out.append(data)
    e.close()
    assert out[0] == out[1], ("called twice", B, ch, M)
    return out[0], info


def orders_main(torch, sa, b):
    seen = {}
    for case, (B, ch, M, rows) in enumerate(steps.stream_cases()):
        data, info = encode_twice(torch, b, [x for _, x in rows], ch, B, M, 8 * (1 + case % 3))
        for r, (name, x) in enumerate(rows):
            kd = check_row(data[r], x, ch, B, M, info[r], ("B", B, "ch", ch, "M", M, name))
            got = {int(k.split("/")[0][3:]) for f in kd for k in f if k.startswith("lpc")}
            assert all(o <= M for o in got), (B, ch, M, name, got)
            seen.setdefault(B, set()).update(got)
    for B in sorted(seen):
        print("LPC orders chosen on the device at B = %d: %s" % (B, sorted(seen[B])))
    assert sorted(seen) == list(mdl.BLOCKS)
    assert seen[256] == set(range(1, 9)), seen[256]
    for B in mdl.BLOCKS[1:]:
        assert min(seen[B]) <= 3 and max(seen[B]) >= 5, (B, seen[B])


# ---- 2. degenerate blocks ---------------------------------------------------------------------------------------------------

def degenerate_main(torch, sa, b):
    M = 8
    for case, (B, ch, rows) in enumerate(steps.degenerate_cases()):
        data, info = encode_twice(torch, b, [x for _, x in rows], ch, B, M, 8 * (1 + case % 3))
        for r, (name, x) in enumerate(rows):
            kd = check_row(data[r], x, ch, B, M, info[r], ("degenerate", B, ch, name))
            for k, f in enumerate(kd):  # no LPC subframe where the model has none
                _, (_, an) = mdl.encode_block(x[k * B * ch:(k + 1) * B * ch], ch, B, k, M, with_choice=True)
                assert [a["type"] == "lpc" for a in an] == [s.startswith("lpc") for s in f], (B, ch, name, k, f)
            if name == "impulse" or name.startswith("edge"):
                assert not any(s.startswith("lpc") for f in kd for s in f), (B, ch, name, kd)
            if name == "impulse,ar8":
                assert not any(s.startswith("lpc") for s in kd[0]) and any(s.startswith("lpc8") for s in kd[1]), (B, ch, kd)
        print("degenerate", B, ch, [n for n, _ in rows])


# ---- 3. order 0 at the sizes no encoder has had ---------------------------------------------------------------------------

def order0_main(torch, sa, b):
    import flac_model
    case = 0
    for B in (512, 2048):
        for ch in (1, 2):
            frames = 2 * B + 37
            kinds = [mdl.KINDS[(3 * case + r + 1) % len(mdl.KINDS)] for r in range(3)]
            x = [material(k, frames, ch, case + r) for r, k in enumerate(kinds)]
            keep, out = [], []
            for make in (b.create_flac_lpc, b.create_flac):
                e = make(3, ch, B)
                ptr, pitch = stage(torch, keep, x, ch)
                e.feed(ptr, pitch, [frames] * 3, finish=True)
                out.append(e.read())
                e.close()
            assert out[0] == out[1], ("order 0", B, ch)
            for r in range(3):
                want, sizes = flac_model.encode_stream(x[r], ch, B)
                assert out[0][0][r] == want, ("order 0 against the model", B, ch, kinds[r])
                assert out[0][1][r] == flac_model.info(frames, sizes), (B, ch, kinds[r])
            case += 1


# ---- 4. feeds ---------------------------------------------------------------------------------------------------------------------

def feeds_main(torch, sa, b):
    B, ch, M, rows = steps.feed_case()
    x = [r for _, r in rows]
    lengths = [len(r) // ch for r in x]
    pieces = [1, B - 1, B + 1, 2 * B, 6 * B]
    e = b.create_flac(4, ch, B, max_lpc_order=M)
    keep, got, cur = [], [b""] * 4, [0] * 4
    for i, n in enumerate(pieces):
        last = i == len(pieces) - 1
        fr = [0 if (i + r) % 5 == 4 and not last else min(n, lengths[r] - cur[r]) for r in range(4)]
        ptr, pitch = stage(torch, keep, [x[r][cur[r] * ch:(cur[r] + fr[r]) * ch] for r in range(4)], ch)
        e.feed(ptr, pitch, fr, finish=last)
        for r in range(4):
            cur[r] += fr[r]
        data, info = e.read()  # reads in between: what is complete so far, nothing twice
        for r in range(4):
            got[r] += data[r]
            assert info[r]["frames"] == cur[r] and info[r]["bytes"] == len(got[r])
    assert cur == lengths
    _, info = e.read()
    e.read(reset=True)
    ptr, pitch = stage(torch, keep, x, ch)
    e.feed(ptr, pitch, lengths, finish=True)
    data, info2 = e.read()
    assert data == got and info2 == info, ("one piece", B, ch)
    e.close()
    seen = set()
    for r, (name, _) in enumerate(rows):
        kd = check_row(got[r], x[r], ch, B, M, info[r], ("feeds", B, ch, name))
        seen.update(k.split("/")[0] for f in kd for k in f)
    print("feeds", B, ch, sorted(seen))
    assert {"lpc5", "lpc2"} <= seen, seen


SECTIONS = [("orders", orders_main), ("degenerate", degenerate_main), ("order0", order0_main), ("feeds", feeds_main)]


def torch_main():
    """(in a process of its own, torch imported first: tests/test_gpu_flac_lpc.py's fixture) every section on one batch's device;
    a section that fails ends the process -- nothing more is started on the device behind a failure"""
    import torch
    import saugns_amd as sa
    from saugns_amd import voicebank as vb
    b = sa.Batch([vb.build_program([vb.Op("sin", freq=200.0, time_ms=10)])], 44100)  # (never run: its device is all that is used)
    for name, fn in SECTIONS:
        try:
            fn(torch, sa, b)
        except Exception:
            print("flac lpc steps %s FAILED\n%s" % (name, traceback.format_exc()))
            break
        print("flac lpc steps %s ok" % name)
    b.close()


TORCH = r"""
import sys
import torch  # (before the library: tests/test_gpu_flac_lpc.py)
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_flac_lpc_steps
test_gpu_flac_lpc_steps.torch_main()
"""


@pytest.fixture(scope="module")
def torch_run():
    run = subprocess.run([sys.executable, "-c", TORCH, ROOT], capture_output=True, text=True, timeout=600)
    print(run.stdout[-6000:])
    return run


def _section(run, name):
    assert "flac lpc steps %s ok" % name in run.stdout, (run.returncode, run.stdout[-4000:], run.stderr[-4000:])


def test_every_block_size_and_order(torch_run):
    """B = 256 with max_lpc_order 1 .. 8, mono and stereo by turns; B = 512, 1024, 2048 and 4096 mono and stereo with M = 8 and one
    of 3, 5, 6, 7; three rows of 2 B + 37 frames each -- all-pole processes whose best predictor has a known order, pm, the
    extremes -- in one feed with finish: the model's bytes, the input back from the model's decoder, the model's records, the
    same bytes from a second identical feed; every order 1 .. 8 is chosen at B = 256, an order <= 3 and one >= 5 at every other
    size (a lane's run is B / 64 frames: at 256 the warm-up cuts i0 > M and i0 > m fall differently for every M and m)."""
    _section(torch_run, "orders")


def test_blocks_without_a_candidate_order(torch_run):
    """B = 256, 1024 and 4096, M = 8, mono and stereo: an impulse (R[1 ..] = 0: no candidate, the kernel's m == 0 path), two samples
    two frames apart (order 1 skipped under a candidate order 2: a hole in the mask), a first sample the window takes to 0 (R[0] == 0
    in a block that is not constant) or to -1 (the arithmetic shift of a negative product; R[0] = 1), and an impulse block followed
    by one that chooses order 8 (what the block without a candidate leaves behind): bytes, decoder and records as above, and LPC
    subframes exactly where the model has them."""
    _section(torch_run, "degenerate")


def test_order_0_at_512_and_2048(torch_run):
    """the block sizes no encoder had been given: sauAmd_Batch_create_flac and sauAmd_Batch_create_flac_lpc(.., 0) give equal bytes
    and records, flac_model's"""
    _section(torch_run, "order0")


def test_feeds_in_pieces_at_512(torch_run):
    """B = 512 stereo, max_lpc_order 5: four rows (an order-5 process, an empty row, the pair, an order-2 process) in feeds of 1,
    B - 1, B + 1, 2 B frames and the rest with reads in between, then in one piece: the same bytes, the model's"""
    _section(torch_run, "feeds")
    assert torch_run.returncode == 0, (torch_run.stdout[-2000:], torch_run.stderr[-4000:])
