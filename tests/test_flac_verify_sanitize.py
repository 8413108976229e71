"""The FLAC decoder's arithmetic (saugns_amd/csrc/sau_flac_dec.h) under AddressSanitizer and UndefinedBehaviorSanitizer, as a
stand-alone program of host code only (tests/flac_verify_fuzz/main.cpp): every single-bit flip and every prefix of one frame per
subframe type and width, seeded mutations, and a few thousand seeded random byte strings, each in a heap buffer of exactly its
length. The kernel runs the same source, so this is where its reader is shown to stay inside the frame. The program is built and
run once; nothing is loaded into Python under a sanitizer."""
import os
import shutil
import struct
import subprocess
import sys

import flac_verify_cases as fc
from test_flac_verify_host import _one_of_each_type

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "flac_verify_fuzz", "main.cpp")


def _compiler():
    for cxx in (os.environ.get("CXX"), "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    raise AssertionError("no C++ compiler for the sanitizer program")


def run_fuzz(sa, tmp_path):
    """build the program, write the frames, run it once: exit status 0 (tests/test_gpu_flac_verify.py runs it too, ahead of the
    first corrupt frame it hands to the kernel)"""
    exe = str(tmp_path / "flac_verify_fuzz")
    subprocess.check_call([_compiler(), "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-Wall", SRC, "-o", exe])
    records = []
    for (bits, t), c in sorted(_one_of_each_type(sa).items()):  # B = 256, whole blocks: flips and every prefix
        records.append((c, 1))
    for c in fc.valid_cases(sa):  # short blocks of every mode, and the longest whole B = 4096 frame of each width
        if c["kind"] in ("noise", "burst", "extremes") and c["n"] in (1, 5, 255) and c["B"] == 256:
            records.append((c, 1))
    for bits in (16, 24):
        records.append((max((c for c in fc.valid_cases(sa) if c["B"] == 4096 and c["bits"] == bits), key=lambda c: len(c["frame"])), 0))
    path = str(tmp_path / "frames.bin")
    with open(path, "wb") as f:
        for c, flips in records:
            f.write(struct.pack("<6I", c["channels"], c["B"], c["bits"], c["number"], flips, len(c["frame"])) + c["frame"])
        for name, fr, ch, B, bits, number, x in fc.handmade_valid():
            f.write(struct.pack("<6I", ch, B, bits, number, 1 if B == 256 else 0, len(fr)) + fr)
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    sys.stdout.write(r.stdout.decode(errors="replace")[-4000:])
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-4000:]
    assert r.stdout.decode().startswith("ok: ")


def test_decoder_under_sanitizers(sa, tmp_path):
    run_fuzz(sa, tmp_path)
