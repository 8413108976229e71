"""ctypes binding of libsaugns_amd.so -- the same calls a C host would make.

``Generator`` mirrors the reference interface for this path
(``sau_create_Generator`` / ``sauGenerator_run`` / ``sau_destroy_Generator``,
sau/generator.h:17-26): same names, argument meaning and error behaviour
(``None``/``RuntimeError`` where the C function returns NULL).  ``Batch`` is
the multi-program extension.  Nothing here computes audio: without the HIP
library and a GPU, creation fails loudly.
"""
import ctypes as C
import os
import weakref

import numpy as np

from . import build as _build

_lib = None


class SauLine(C.Structure):
    _fields_ = [("v0", C.c_float), ("vt", C.c_float), ("pos", C.c_uint32),
                ("end", C.c_uint32), ("time_ms", C.c_uint32), ("type", C.c_uint8),
                ("flags", C.c_uint8)]


class SauTime(C.Structure):
    _fields_ = [("v_ms", C.c_uint32), ("flags", C.c_uint8)]


class SauRasOpt(C.Structure):
    _fields_ = [("word", C.c_uint32), ("alpha", C.c_uint32)]


class SauMode(C.Union):
    _fields_ = [("main", C.c_uint8), ("ras", SauRasOpt)]


class SauOpData(C.Structure):
    _fields_ = [("id", C.c_uint32), ("params", C.c_uint32), ("time", SauTime),
                ("pan", C.POINTER(SauLine)), ("amp", C.POINTER(SauLine)),
                ("amp2", C.POINTER(SauLine)), ("freq", C.POINTER(SauLine)),
                ("freq2", C.POINTER(SauLine)), ("pm_a", C.POINTER(SauLine)),
                ("phase", C.c_uint32), ("seed", C.c_uint32), ("use_type", C.c_uint8),
                ("type", C.c_uint8), ("mode", SauMode),
                ("camods", C.c_void_p), ("amods", C.c_void_p), ("ramods", C.c_void_p),
                ("fmods", C.c_void_p), ("rfmods", C.c_void_p), ("pmods", C.c_void_p),
                ("apmods", C.c_void_p), ("fpmods", C.c_void_p)]


class SauEvent(C.Structure):
    _fields_ = [("wait_ms", C.c_uint32), ("vo_id", C.c_uint16),
                ("carr_op_id", C.c_uint32), ("op_count", C.c_uint32),
                ("op_data_count", C.c_uint32), ("op_list", C.c_void_p),
                ("op_data", C.POINTER(SauOpData))]


class SauProgram(C.Structure):
    _fields_ = [("events", C.POINTER(SauEvent)), ("ev_count", C.c_size_t),
                ("mode", C.c_uint16), ("vo_count", C.c_uint16), ("op_count", C.c_uint32),
                ("op_nest_depth", C.c_uint8), ("duration_ms", C.c_uint32),
                ("ampmult", C.c_float), ("name", C.c_char_p), ("mp", C.c_void_p),
                ("parse", C.c_void_p)]


assert C.sizeof(SauLine) == 24 and C.sizeof(SauOpData) == 152
assert C.sizeof(SauEvent) == 40 and C.sizeof(SauProgram) == 64

# enum values of include/sau_abi.h
LINES = "cos lin sah exp log xpe lge sqe cub smo ncl nhl uwh".split()
WAVES = "sin tri srs sqr ean cat eto par mto saw hsi spa".split()
NOISES = "wh gw bw tw re vi bv".split()
LP_STATE, LP_STATE_RATIO, LP_GOAL, LP_GOAL_RATIO, LP_TYPE, LP_TIME, LP_TIME_IF_NEW = \
    1, 2, 4, 8, 16, 32, 64
POPT_AMP, POPT_NOISE, POPT_WAVE, POPT_RASEG = 0, 1, 2, 3
POP_CARR, POP_CAMOD, POP_AMOD, POP_RAMOD, POP_FMOD, POP_RFMOD, POP_PMOD, POP_APMOD, \
    POP_FPMOD = range(9)
TIMEP_SET, TIMEP_DEFAULT, TIMEP_IMPLICIT = 1, 2, 4
PMODE_AMP_DIV_VOICES = 1


class LineDesc(C.Structure):
    _fields_ = [("present", C.c_uint8), ("has_goal", C.c_uint8), ("ratio", C.c_uint8), ("shape", C.c_uint8),
                ("v0", C.c_float), ("goal", C.c_float)]


class OpDesc(C.Structure):
    """sauAmdOpDesc (include/saugns_amd.h): one operator of a voice bank for sauAmd_build_bank."""
    _fields_ = [("parent", C.c_uint32), ("use", C.c_uint32), ("type", C.c_uint32), ("mode", C.c_uint32),
                ("time_ms", C.c_uint32), ("start_ms", C.c_uint32), ("phase", C.c_uint32), ("seed", C.c_uint32),
                ("pan", LineDesc), ("amp", LineDesc), ("amp2", LineDesc), ("freq", LineDesc),
                ("freq2", LineDesc), ("pm_a", LineDesc)]


class Levels(C.Structure):
    """sauAmdLevels (include/saugns_amd.h): what the level meter reports of one stream or row. [0] is L or mono, [1] R."""
    _fields_ = [("frames", C.c_uint64), ("peak", C.c_float * 2), ("sum_sq", C.c_double * 2), ("over", C.c_uint64 * 2),
                ("full_scale", C.c_uint64 * 2), ("nonfinite", C.c_uint64 * 2)]

    def as_dict(self):
        return {"frames": int(self.frames), "peak": list(self.peak), "sum_sq": list(self.sum_sq), "over": list(self.over),
                "full_scale": list(self.full_scale), "nonfinite": list(self.nonfinite)}

    def __repr__(self):
        return "Levels(%r)" % (self.as_dict(),)


assert C.sizeof(Levels) == 80


class Loudness(C.Structure):
    """sauAmdLoudness (include/saugns_amd.h): BS.1770 loudness and true peak of one stream or row. [0] is L or mono, [1] R."""
    _fields_ = [("frames", C.c_uint64), ("blocks", C.c_uint64), ("gated_blocks", C.c_uint64), ("integrated", C.c_double),
                ("momentary_max", C.c_double), ("true_peak", C.c_float * 2)]

    def as_dict(self):
        return {"frames": int(self.frames), "blocks": int(self.blocks), "gated_blocks": int(self.gated_blocks),
                "integrated": float(self.integrated), "momentary_max": float(self.momentary_max),
                "true_peak": list(self.true_peak)}

    def __repr__(self):
        return "Loudness(%r)" % (self.as_dict(),)


assert C.sizeof(Loudness) == 48


class LimiterStats(C.Structure):
    """sauAmdLimiterStats (include/saugns_amd.h): what the limiter did to one stream or row."""
    _fields_ = [("frames", C.c_uint64), ("limited", C.c_uint64), ("min_gain", C.c_double)]

    def as_dict(self):
        return {"frames": int(self.frames), "limited": int(self.limited), "min_gain": float(self.min_gain)}

    def __repr__(self):
        return "LimiterStats(%r)" % (self.as_dict(),)


assert C.sizeof(LimiterStats) == 24


class FlacInfo(C.Structure):
    """sauAmdFlacInfo: what an encoder's stream has made since the last reset"""
    _fields_ = [("frames", C.c_uint64), ("blocks", C.c_uint64), ("bytes", C.c_uint64), ("min_frame_bytes", C.c_uint32),
                ("max_frame_bytes", C.c_uint32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}

    def __repr__(self):
        return "FlacInfo(%r)" % (self.as_dict(),)


assert C.sizeof(FlacInfo) == 32


class FlacVerify(C.Structure):
    """sauAmdFlacVerify: what a verifying encoder has checked of a stream since the last reset"""
    _fields_ = [("blocks", C.c_uint64), ("bad_blocks", C.c_uint64), ("first_bad_block", C.c_uint64), ("first_status", C.c_uint32),
                ("pad_", C.c_uint32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "pad_"}

    def __repr__(self):
        return "FlacVerify(%r)" % (self.as_dict(),)


assert C.sizeof(FlacVerify) == 32


class Dither(C.Structure):
    """sauAmdDither (include/saugns_amd.h, section "Dither and noise shaping"): a quantiser's spec -- the dither's seed,
    ``dither`` 0 (none) or 1 (TPDF), and ``taps`` error-feedback coefficients, coef[0] on the most recent error."""
    _fields_ = [("seed", C.c_uint64), ("dither", C.c_uint32), ("taps", C.c_uint32), ("coef", C.c_double * 9)]

    def __init__(self, seed=0, dither=0, coef=()):
        super().__init__()
        self.seed, self.dither, self.taps = int(seed) & (2**64 - 1), int(dither), len(coef)
        for j, v in enumerate(list(coef)[:9]):
            self.coef[j] = float(v)

    def as_dict(self):
        return {"seed": int(self.seed), "dither": int(self.dither), "taps": int(self.taps),
                "coef": [float(v) for v in self.coef[:min(int(self.taps), 9)]]}

    def __repr__(self):
        return "Dither(%r)" % (self.as_dict(),)


assert C.sizeof(Dither) == 88


class DitherStats(C.Structure):
    """sauAmdDitherStats: the frames a quantiser's row was fed and, per channel, the samples its clamp changed"""
    _fields_ = [("frames", C.c_uint64), ("clipped", C.c_uint64 * 2)]

    def as_dict(self):
        return {"frames": int(self.frames), "clipped": [int(self.clipped[0]), int(self.clipped[1])]}

    def __repr__(self):
        return "DitherStats(%r)" % (self.as_dict(),)


assert C.sizeof(DitherStats) == 24
DITHER_FLAT, DITHER_HP1, DITHER_E3, DITHER_E5, DITHER_F9 = range(5)


def _declare(L):
    """The C ABI of include/saugns_amd.h on a loaded library."""
    L.sau_create_Generator.restype = C.c_void_p
    L.sau_create_Generator.argtypes = [C.c_void_p, C.c_uint32]
    L.sau_destroy_Generator.argtypes = [C.c_void_p]
    L.sauGenerator_run.restype = C.c_bool
    L.sauGenerator_run.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_bool,
                                   C.POINTER(C.c_size_t)]
    L.sauAmd_create_Batch.restype = C.c_void_p
    L.sauAmd_create_Batch.argtypes = [C.POINTER(C.c_void_p), C.c_size_t, C.c_uint32]
    if hasattr(L, "sauAmd_create_Batch_on"):  # (SAU_AMD_LIB may name an older build)
        L.sauAmd_create_Batch_on.restype = C.c_void_p
        L.sauAmd_create_Batch_on.argtypes = [C.c_int, C.POINTER(C.c_void_p), C.c_size_t, C.c_uint32]
    L.sauAmd_destroy_Batch.argtypes = [C.c_void_p]
    L.sauAmd_render_file.restype = C.c_bool
    L.sauAmd_render_file.argtypes = [C.c_void_p, C.c_uint32, C.c_char_p, C.c_int, C.c_int,
                                     C.POINTER(C.c_uint64)]
    L.sauAmd_Batch_run.restype = C.c_bool
    L.sauAmd_Batch_run.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_size_t, C.c_bool,
                                   C.POINTER(C.c_bool), C.POINTER(C.c_size_t)]
    L.sauAmd_Batch_set_call_len.argtypes = [C.c_void_p, C.c_size_t]
    L.sauAmd_Batch_device_pcm.restype = C.c_void_p
    L.sauAmd_Batch_device_pcm.argtypes = [C.c_void_p, C.c_size_t]
    L.sauAmd_Batch_sync.restype = C.c_bool
    L.sauAmd_Batch_sync.argtypes = [C.c_void_p]
    L.sauAmd_Batch_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                      C.POINTER(C.c_uint64), C.c_int]
    L.sauAmd_Batch_timing_ex.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.c_int]
    L.sauAmd_Batch_set_timing.argtypes = [C.c_void_p, C.c_int]
    if hasattr(L, "sauAmd_Batch_order_after"):  # (SAU_AMD_LIB may name an older build: A/B timing against earlier rounds)
        L.sauAmd_Batch_order_after.restype = C.c_bool
        L.sauAmd_Batch_order_after.argtypes = [C.c_void_p, C.c_void_p]
    L.sauAmd_Batch_stream.restype = C.c_void_p
    L.sauAmd_Batch_stream.argtypes = [C.c_void_p]
    if hasattr(L, "sauAmd_Batch_run_f32"):  # float32 sample output (SAU_AMD_LIB may name an older build)
        L.sauAmd_Batch_run_f32.restype = C.c_bool
        L.sauAmd_Batch_run_f32.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_size_t, C.c_bool,
                                           C.POINTER(C.c_bool), C.POINTER(C.c_size_t)]
    if hasattr(L, "sauAmd_Batch_device_pcm_f32"):
        L.sauAmd_Batch_device_pcm_f32.restype = C.c_void_p
        L.sauAmd_Batch_device_pcm_f32.argtypes = [C.c_void_p, C.c_size_t]
    if hasattr(L, "sauAmd_Batch_device_pcm_pitch"):
        L.sauAmd_Batch_device_pcm_pitch.restype = C.c_size_t
        L.sauAmd_Batch_device_pcm_pitch.argtypes = [C.c_void_p]
    if hasattr(L, "sauAmd_Batch_set_metering"):  # level metering (SAU_AMD_LIB may name an older build)
        L.sauAmd_Batch_set_metering.restype = C.c_bool
        L.sauAmd_Batch_set_metering.argtypes = [C.c_void_p, C.c_int]
        L.sauAmd_Batch_levels.restype = C.c_bool
        L.sauAmd_Batch_levels.argtypes = [C.c_void_p, C.POINTER(Levels), C.c_int]
        L.sauAmd_Batch_measure_rows.restype = C.c_bool
        L.sauAmd_Batch_measure_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_size_t, C.c_int,
                                                C.POINTER(Levels)]
        L.sauAmd_render_file_normalized.restype = C.c_bool
        L.sauAmd_render_file_normalized.argtypes = [C.c_void_p, C.c_uint32, C.c_char_p, C.c_int, C.c_int, C.c_float,
                                                    C.POINTER(C.c_uint64), C.POINTER(Levels)]
    if hasattr(L, "sauAmd_Batch_run_decimated_f32"):  # oversampled rendering (SAU_AMD_LIB may name an older build)
        L.sauAmd_Batch_run_decimated_f32.restype = C.c_bool
        L.sauAmd_Batch_run_decimated_f32.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.c_size_t, C.c_bool,
                                                     C.POINTER(C.c_bool), C.POINTER(C.c_size_t)]
        L.sauAmd_Batch_device_decimated_f32.restype = C.c_void_p
        L.sauAmd_Batch_device_decimated_f32.argtypes = [C.c_void_p, C.c_size_t]
        L.sauAmd_Batch_device_decimated_pitch.restype = C.c_size_t
        L.sauAmd_Batch_device_decimated_pitch.argtypes = [C.c_void_p]
        L.sauAmd_decimator_taps.restype = C.c_size_t
        L.sauAmd_decimator_taps.argtypes = [C.c_int, C.POINTER(C.c_double), C.c_size_t]
        L.sauAmd_decimator_latency.restype = C.c_size_t
        L.sauAmd_decimator_latency.argtypes = [C.c_int]
        L.sauAmd_render_file_oversampled.restype = C.c_bool
        L.sauAmd_render_file_oversampled.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_char_p, C.c_int, C.c_int,
                                                     C.POINTER(C.c_uint64)]
    if hasattr(L, "sauAmd_Batch_set_loudness"):  # loudness and true peak (SAU_AMD_LIB may name an older build)
        L.sauAmd_loudness_filter.restype = C.c_bool
        L.sauAmd_loudness_filter.argtypes = [C.c_uint32, C.POINTER(C.c_double)]
        L.sauAmd_truepeak_taps.restype = C.c_size_t
        L.sauAmd_truepeak_taps.argtypes = [C.POINTER(C.c_double), C.c_size_t]
        L.sauAmd_loudness_gate.restype = C.c_bool
        L.sauAmd_loudness_gate.argtypes = [C.POINTER(C.c_double), C.c_size_t, C.c_uint32, C.c_int, C.POINTER(Loudness)]
        L.sauAmd_Batch_set_loudness.restype = C.c_bool
        L.sauAmd_Batch_set_loudness.argtypes = [C.c_void_p, C.c_int]
        L.sauAmd_Batch_loudness.restype = C.c_bool
        L.sauAmd_Batch_loudness.argtypes = [C.c_void_p, C.POINTER(Loudness), C.c_int]
        L.sauAmd_Batch_loudness_hops.restype = C.c_size_t
        L.sauAmd_Batch_loudness_hops.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_double), C.c_size_t]
        L.sauAmd_Batch_measure_loudness_rows.restype = C.c_bool
        L.sauAmd_Batch_measure_loudness_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int,
                                                         C.c_uint32, C.POINTER(Loudness), C.POINTER(C.c_double), C.c_size_t]
        L.sauAmd_render_file_loudness.restype = C.c_bool
        L.sauAmd_render_file_loudness.argtypes = [C.c_void_p, C.c_uint32, C.c_char_p, C.c_int, C.c_int, C.c_double, C.c_float,
                                                  C.POINTER(C.c_uint64), C.POINTER(Loudness), C.POINTER(C.c_float)]
    if hasattr(L, "sauAmd_Batch_run_limited_f32"):  # the limiter (SAU_AMD_LIB may name an older build)
        L.sauAmd_limiter_window.restype = C.c_size_t
        L.sauAmd_limiter_window.argtypes = [C.c_uint32, C.POINTER(C.c_double), C.c_size_t]
        L.sauAmd_limiter_latency.restype = C.c_size_t
        L.sauAmd_limiter_latency.argtypes = [C.c_uint32]
        L.sauAmd_Batch_run_limited_f32.restype = C.c_bool
        L.sauAmd_Batch_run_limited_f32.argtypes = [C.c_void_p, C.c_float, C.c_float, C.POINTER(C.c_void_p), C.c_size_t, C.c_bool,
                                                   C.POINTER(C.c_bool), C.POINTER(C.c_size_t)]
        L.sauAmd_Batch_device_limited_f32.restype = C.c_void_p
        L.sauAmd_Batch_device_limited_f32.argtypes = [C.c_void_p, C.c_size_t]
        L.sauAmd_Batch_device_limited_pitch.restype = C.c_size_t
        L.sauAmd_Batch_device_limited_pitch.argtypes = [C.c_void_p]
        L.sauAmd_Batch_limiter_stats.restype = C.c_bool
        L.sauAmd_Batch_limiter_stats.argtypes = [C.c_void_p, C.POINTER(LimiterStats), C.c_int]
        L.sauAmd_Batch_limit_rows.restype = C.c_bool
        L.sauAmd_Batch_limit_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_uint32,
                                              C.c_float, C.c_float, C.c_void_p, C.c_size_t, C.POINTER(LimiterStats)]
        L.sauAmd_render_file_loudness_limited.restype = C.c_bool
        L.sauAmd_render_file_loudness_limited.argtypes = [C.c_void_p, C.c_uint32, C.c_char_p, C.c_int, C.c_int, C.c_double,
                                                          C.c_float, C.POINTER(C.c_uint64), C.POINTER(Loudness),
                                                          C.POINTER(C.c_float), C.POINTER(LimiterStats)]
    if hasattr(L, "sauAmd_Batch_create_spectrum"):  # the spectrum meter (SAU_AMD_LIB may name an older build)
        L.sauAmd_spectrum_window.restype = C.c_size_t
        L.sauAmd_spectrum_window.argtypes = [C.c_uint, C.POINTER(C.c_double), C.c_size_t]
        L.sauAmd_spectrum_twiddles.restype = C.c_size_t
        L.sauAmd_spectrum_twiddles.argtypes = [C.c_uint, C.POINTER(C.c_double), C.c_size_t]
        L.sauAmd_Batch_create_spectrum.restype = C.c_void_p
        L.sauAmd_Batch_create_spectrum.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_uint, C.c_uint32]
        L.sauAmd_Spectrum_destroy.argtypes = [C.c_void_p]
        L.sauAmd_Spectrum_feed.restype = C.c_bool
        L.sauAmd_Spectrum_feed.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)]
        L.sauAmd_Spectrum_read.restype = C.c_bool
        L.sauAmd_Spectrum_read.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.c_int]
        L.sauAmd_Batch_spectrum_rows.restype = C.c_bool
        L.sauAmd_Batch_spectrum_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_uint,
                                                 C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_float),
                                                 C.c_size_t]
        L.sauAmd_render_spectrum.restype = C.c_bool
        L.sauAmd_render_spectrum.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_uint, C.c_uint32, C.POINTER(C.c_double),
                                             C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    if hasattr(L, "sauAmd_Batch_create_flac"):  # the FLAC encoder (SAU_AMD_LIB may name an older build)
        L.sauAmd_flac_header.restype = C.c_size_t
        L.sauAmd_flac_header.argtypes = [C.c_uint32, C.c_int, C.c_uint32, C.POINTER(FlacInfo), C.c_void_p, C.c_size_t]
        L.sauAmd_flac_encode_block.restype = C.c_size_t
        L.sauAmd_flac_encode_block.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t]
        L.sauAmd_Batch_create_flac.restype = C.c_void_p
        L.sauAmd_Batch_create_flac.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_uint32]
        L.sauAmd_Flac_destroy.argtypes = [C.c_void_p]
        L.sauAmd_Flac_feed.restype = C.c_bool
        L.sauAmd_Flac_feed.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32), C.c_int]
        L.sauAmd_Flac_read.restype = C.c_bool
        L.sauAmd_Flac_read.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t),
                                       C.POINTER(FlacInfo), C.c_int]
        L.sauAmd_render_file_flac.restype = C.c_bool
        L.sauAmd_render_file_flac.argtypes = [C.c_void_p, C.c_uint32, C.c_char_p, C.c_int, C.c_uint32, C.POINTER(C.c_uint64),
                                              C.POINTER(FlacInfo)]
    if hasattr(L, "sauAmd_Batch_create_quantizer"):  # dither and noise shaping (SAU_AMD_LIB may name an older build)
        L.sauAmd_dither_preset.restype = C.c_bool
        L.sauAmd_dither_preset.argtypes = [C.c_int, C.c_uint64, C.POINTER(Dither)]
        L.sauAmd_dither_quantize.restype = C.c_bool
        L.sauAmd_dither_quantize.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_float, C.POINTER(Dither), C.c_uint64, C.c_uint64,
                                             C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
        L.sauAmd_Batch_create_quantizer.restype = C.c_void_p
        L.sauAmd_Batch_create_quantizer.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.POINTER(Dither)]
        L.sauAmd_Quantizer_destroy.argtypes = [C.c_void_p]
        L.sauAmd_Quantizer_feed.restype = C.c_bool
        L.sauAmd_Quantizer_feed.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_float)]
        L.sauAmd_Quantizer_rows.restype = C.c_void_p
        L.sauAmd_Quantizer_rows.argtypes = [C.c_void_p]
        L.sauAmd_Quantizer_pitch.restype = C.c_size_t
        L.sauAmd_Quantizer_pitch.argtypes = [C.c_void_p]
        L.sauAmd_Quantizer_read.restype = C.c_bool
        L.sauAmd_Quantizer_read.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        L.sauAmd_Quantizer_stats.restype = C.c_bool
        L.sauAmd_Quantizer_stats.argtypes = [C.c_void_p, C.POINTER(DitherStats), C.c_int]
        L.sauAmd_render_file_dithered.restype = C.c_bool
        L.sauAmd_render_file_dithered.argtypes = [C.c_void_p, C.c_uint32, C.c_char_p, C.c_int, C.c_int, C.c_float, C.POINTER(Dither),
                                                  C.POINTER(C.c_uint64), C.POINTER(DitherStats)]
        L.sauAmd_render_file_flac_dithered.restype = C.c_bool
        L.sauAmd_render_file_flac_dithered.argtypes = [C.c_void_p, C.c_uint32, C.c_char_p, C.c_int, C.c_uint32, C.c_uint32, C.c_float,
                                                       C.POINTER(Dither), C.POINTER(C.c_uint64), C.POINTER(FlacInfo),
                                                       C.POINTER(DitherStats)]
        L.sauAmd_render_file_loudness_dithered.restype = C.c_bool
        L.sauAmd_render_file_loudness_dithered.argtypes = [C.c_void_p, C.c_uint32, C.c_char_p, C.c_int, C.c_int, C.c_double, C.c_float,
                                                           C.POINTER(Dither), C.POINTER(C.c_uint64), C.POINTER(Loudness),
                                                           C.POINTER(C.c_float), C.POINTER(DitherStats)]
    if hasattr(L, "sauAmd_Batch_create_flac_lpc"):  # the encoder's LPC mode (SAU_AMD_LIB may name an older build)
        L.sauAmd_flac_encode_block_lpc.restype = C.c_size_t
        L.sauAmd_flac_encode_block_lpc.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                                   C.c_size_t]
        L.sauAmd_Batch_create_flac_lpc.restype = C.c_void_p
        L.sauAmd_Batch_create_flac_lpc.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.c_uint32]
        L.sauAmd_render_file_flac_lpc.restype = C.c_bool
        L.sauAmd_render_file_flac_lpc.argtypes = [C.c_void_p, C.c_uint32, C.c_char_p, C.c_int, C.c_uint32, C.c_uint32,
                                                  C.POINTER(C.c_uint64), C.POINTER(FlacInfo)]
    if hasattr(L, "sauAmd_Flac_set_md5"):  # the encoder's MD5 (SAU_AMD_LIB may name an older build)
        L.sauAmd_Flac_set_md5.restype = C.c_bool
        L.sauAmd_Flac_set_md5.argtypes = [C.c_void_p, C.c_int]
        L.sauAmd_Flac_md5.restype = C.c_bool
        L.sauAmd_Flac_md5.argtypes = [C.c_void_p, C.c_void_p]
        L.sauAmd_flac_header_md5.restype = C.c_size_t
        L.sauAmd_flac_header_md5.argtypes = [C.c_uint32, C.c_int, C.c_uint32, C.c_int, C.POINTER(FlacInfo), C.c_void_p, C.c_void_p,
                                             C.c_size_t]
        L.sauAmd_flac_md5.restype = C.c_bool
        L.sauAmd_flac_md5.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        L.sauAmd_set_flac_file_md5.restype = C.c_int
        L.sauAmd_set_flac_file_md5.argtypes = [C.c_int]
    if hasattr(L, "sauAmd_flac_decode_block"):  # the decoder and the verify mode (SAU_AMD_LIB may name an older build)
        L.sauAmd_flac_decode_block.restype = C.c_size_t
        L.sauAmd_flac_decode_block.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.c_int, C.c_uint32, C.c_void_p, C.c_size_t,
                                               C.POINTER(C.c_uint32), C.POINTER(C.c_int)]
        L.sauAmd_Flac_set_verify.restype = C.c_bool
        L.sauAmd_Flac_set_verify.argtypes = [C.c_void_p, C.c_int]
        L.sauAmd_Flac_verify.restype = C.c_bool
        L.sauAmd_Flac_verify.argtypes = [C.c_void_p, C.POINTER(FlacVerify)]
        L.sauAmd_set_flac_file_verify.restype = C.c_int
        L.sauAmd_set_flac_file_verify.argtypes = [C.c_int]
    if hasattr(L, "sauAmd_Batch_create_flac_lpc24"):  # LPC at 24 bits (SAU_AMD_LIB may name an older build)
        L.sauAmd_flac_encode_block_lpc24.restype = C.c_size_t
        L.sauAmd_flac_encode_block_lpc24.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                                     C.c_size_t]
        L.sauAmd_Batch_create_flac_lpc24.restype = C.c_void_p
        L.sauAmd_Batch_create_flac_lpc24.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.c_uint32]
        L.sauAmd_render_file_flac_lpc24.restype = C.c_bool
        L.sauAmd_render_file_flac_lpc24.argtypes = [C.c_void_p, C.c_uint32, C.c_char_p, C.c_int, C.c_uint32, C.c_uint32, C.c_float,
                                                    C.POINTER(C.c_uint64), C.POINTER(FlacInfo)]
        L.sauAmd_render_file_flac_loudness_lpc24.restype = C.c_bool
        L.sauAmd_render_file_flac_loudness_lpc24.argtypes = [C.c_void_p, C.c_uint32, C.c_char_p, C.c_int, C.c_uint32, C.c_uint32,
                                                             C.c_double, C.c_float, C.c_int, C.POINTER(C.c_uint64), C.POINTER(Loudness),
                                                             C.POINTER(C.c_float), C.POINTER(LimiterStats), C.POINTER(FlacInfo)]
    if hasattr(L, "sauAmd_Batch_create_flac_f32"):  # 24 bits and float-fed encoders (SAU_AMD_LIB may name an older build)
        L.sauAmd_flac_header_bits.restype = C.c_size_t
        L.sauAmd_flac_header_bits.argtypes = [C.c_uint32, C.c_int, C.c_uint32, C.c_int, C.POINTER(FlacInfo), C.c_void_p, C.c_size_t]
        L.sauAmd_flac_encode_block_s32.restype = C.c_size_t
        L.sauAmd_flac_encode_block_s32.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32,
                                                   C.c_void_p, C.c_size_t]
        L.sauAmd_flac_quantize.restype = C.c_bool
        L.sauAmd_flac_quantize.argtypes = [C.c_void_p, C.c_size_t, C.c_float, C.c_int, C.c_void_p]
        L.sauAmd_Batch_create_flac_f32.restype = C.c_void_p
        L.sauAmd_Batch_create_flac_f32.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.c_int, C.c_uint32]
        L.sauAmd_Flac_feed_f32.restype = C.c_bool
        L.sauAmd_Flac_feed_f32.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.c_int]
        L.sauAmd_render_file_flac_f32.restype = C.c_bool
        L.sauAmd_render_file_flac_f32.argtypes = [C.c_void_p, C.c_uint32, C.c_char_p, C.c_int, C.c_uint32, C.c_int, C.c_uint32,
                                                  C.c_float, C.POINTER(C.c_uint64), C.POINTER(FlacInfo)]
        L.sauAmd_render_file_flac_loudness.restype = C.c_bool
        L.sauAmd_render_file_flac_loudness.argtypes = [C.c_void_p, C.c_uint32, C.c_char_p, C.c_int, C.c_uint32, C.c_int, C.c_uint32,
                                                       C.c_double, C.c_float, C.c_int, C.POINTER(C.c_uint64), C.POINTER(Loudness),
                                                       C.POINTER(C.c_float), C.POINTER(LimiterStats), C.POINTER(FlacInfo)]
    L.sauAmd_set_piluts.argtypes = [C.c_void_p]
    L.sauAmd_get_piluts.restype = C.POINTER(C.c_float)
    L.sauAmd_last_error.restype = C.c_char_p
    L.sauAmd_device_count.restype = C.c_int
    L.sauAmd_device_pci_bus_id.restype = C.c_bool
    L.sauAmd_device_pci_bus_id.argtypes = [C.c_int, C.c_char_p, C.c_size_t]
    L.sauAmd_program_serialize.restype = C.c_size_t
    L.sauAmd_program_serialize.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.sauAmd_program_load.restype = C.c_void_p
    L.sauAmd_program_load.argtypes = [C.c_void_p, C.c_size_t]
    L.sauAmd_program_free.argtypes = [C.c_void_p]
    L.sauAmd_build_bank.restype = C.c_void_p
    L.sauAmd_build_bank.argtypes = [C.c_void_p, C.c_size_t, C.c_float, C.c_uint32]
    L.sauAmd_free_bank.argtypes = [C.c_void_p]
    return L


def lib():
    """Load (building if stale) libsaugns_amd.so and declare its C ABI."""
    global _lib
    if _lib is not None:
        return _lib
    # SAU_AMD_LIB: load another build of the same library (A/B timing of kernel variants)
    path = os.environ.get("SAU_AMD_LIB") or _build.build()
    _lib = _declare(C.CDLL(path))
    if _tables is not None:
        _lib.sauAmd_set_piluts(_tables.ctypes.data)
    return _lib


_hooks = None
_tables = None


def use_hooks(path):
    """tests/ only: load the test-hook library (tests/hooks/libsaugns_amd_hooks.so: the product's object files + the entry
    points that run the host control plane over an injected backend, + the known-answer probes). The product library has
    none of those; objects made with ``backend=...`` live in, and are driven through, the hook library."""
    global _hooks
    if _hooks is None:
        L = _declare(C.CDLL(path))
        L.sauAmd_create_Generator_with_backend.restype = C.c_void_p
        L.sauAmd_create_Generator_with_backend.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
        L.sauAmd_create_Batch_with_backend.restype = C.c_void_p
        L.sauAmd_create_Batch_with_backend.argtypes = [C.POINTER(C.c_void_p), C.c_size_t, C.c_uint32, C.c_void_p]
        L.sauAmd_render_file_with_backend.restype = C.c_bool
        L.sauAmd_render_file_with_backend.argtypes = [C.c_void_p, C.c_uint32, C.c_char_p, C.c_int, C.c_int,
                                                      C.c_void_p, C.POINTER(C.c_uint64)]
        L.sauAmd_Generator_rewinds.restype = C.c_uint
        L.sauAmd_Generator_rewinds.argtypes = [C.c_void_p]
        if _tables is not None:
            L.sauAmd_set_piluts(_tables.ctypes.data)
        _hooks = L
    return _hooks


def hooks():
    if _hooks is None:
        raise RuntimeError("the test-hook library is not loaded (tests/conftest.py: use_hooks)")
    return _hooks


_last_used = None  # the library the most recent Generator / Batch call went to (the hook library for backend=... objects)


def last_error(L=None):
    return (L or _last_used or lib()).sauAmd_last_error().decode()


def _used(L):
    global _last_used
    _last_used = L
    return L


def device_pci_bus_id(device=0):
    """PCI address of HIP device `device` ("0000:c1:00.0"), or None without one."""
    buf = C.create_string_buffer(64)
    return buf.value.decode() if lib().sauAmd_device_pci_bus_id(int(device), buf, 64) else None


def set_piluts(tables):
    global _tables
    t = np.ascontiguousarray(tables, dtype=np.float32).copy()
    assert t.shape == (12, 2048)
    _tables = t
    lib().sauAmd_set_piluts(t.ctypes.data)
    if _hooks is not None:
        _hooks.sauAmd_set_piluts(t.ctypes.data)


SNDFILE_RAW, SNDFILE_AU, SNDFILE_WAV = 0, 1, 2
SNDFILE_WAV_F32 = 3  # WAVE_FORMAT_IEEE_FLOAT: the mixers' f32 samples, unclamped


def render_file(program, srate, path, fmt=SNDFILE_WAV, channels=1, backend=None):
    """sauAmd_render_file: render a whole program into a raw/AU/WAV (int16) or float32 WAV file -> frames written.
    ``backend`` (tests): a sauengine::Backend* to run the same output stage without a GPU."""
    n = C.c_uint64()
    if backend is None:
        ok = lib().sauAmd_render_file(program.ptr, srate, os.fsencode(path), fmt, channels, C.byref(n))
    else:
        ok = hooks().sauAmd_render_file_with_backend(program.ptr, srate, os.fsencode(path), fmt,
                                                     channels, backend, C.byref(n))
    if not ok:
        raise RuntimeError("sauAmd_render_file failed: " + last_error(None if backend is None else hooks()))
    return n.value


_file_hooks = None


def use_file_hooks(path):
    """tests/ only: load the library that runs the normalised file writer over an injected backend
    (tests/hooks_levels: the product's object files + sauAmd_render_file_normalized_with_backend)."""
    global _file_hooks
    if _file_hooks is None:
        L = _declare(C.CDLL(path))
        L.sauAmd_render_file_normalized_with_backend.restype = C.c_bool
        L.sauAmd_render_file_normalized_with_backend.argtypes = [C.c_void_p, C.c_uint32, C.c_char_p, C.c_int, C.c_int, C.c_float,
                                                                 C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(Levels)]
        _file_hooks = L
    return _file_hooks


def render_file_normalized(program, srate, path, fmt=SNDFILE_WAV, channels=1, target_peak=1.0, backend=None):
    """sauAmd_render_file_normalized: render a whole program into a file scaled to `target_peak` -> (frames written, Levels of
    the render before the gain). Two passes over the program: one that measures, one that writes x * gain (the int16 formats
    round once, after the gain). ``backend`` (tests): a sauengine::Backend* for the first pass, without a GPU."""
    n, lv = C.c_uint64(), Levels()
    if backend is None:
        L = _used(lib())
        ok = L.sauAmd_render_file_normalized(program.ptr, srate, os.fsencode(path), fmt, channels, target_peak,
                                             C.byref(n), C.byref(lv))
    else:
        if _file_hooks is None:
            raise RuntimeError("the file-hook library is not loaded (use_file_hooks)")
        L = _used(_file_hooks)
        ok = L.sauAmd_render_file_normalized_with_backend(program.ptr, srate, os.fsencode(path), fmt, channels, target_peak,
                                                          backend, C.byref(n), C.byref(lv))
    if not ok:
        raise RuntimeError("sauAmd_render_file_normalized failed: " + last_error(L))
    return n.value, lv


_oversample_hooks = None


def use_oversample_hooks(path):
    """tests/ only: load the library that runs the oversampled file writer over an injected backend
    (tests/hooks_oversample: the product's object files + sauAmd_render_file_oversampled_with_backend)."""
    global _oversample_hooks
    if _oversample_hooks is None:
        L = _declare(C.CDLL(path))
        L.sauAmd_render_file_oversampled_with_backend.restype = C.c_bool
        L.sauAmd_render_file_oversampled_with_backend.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_char_p, C.c_int, C.c_int,
                                                                  C.c_void_p, C.POINTER(C.c_uint64)]
        _oversample_hooks = L
    return _oversample_hooks


def render_file_oversampled(program, srate, factor, path, fmt=SNDFILE_WAV, channels=1, backend=None):
    """sauAmd_render_file_oversampled: render a whole program at ``srate * factor`` (factor 2, 4 or 8), decimate it on the
    device and write it at ``srate`` -> frames written: ceil(N / factor) for N high-rate frames, time-aligned with them.
    ``backend`` (tests): a sauengine::Backend* to run the writer over, without a GPU."""
    n = C.c_uint64()
    if backend is None:
        L = _used(lib())
        ok = L.sauAmd_render_file_oversampled(program.ptr, srate, factor, os.fsencode(path), fmt, channels, C.byref(n))
    else:
        if _oversample_hooks is None:
            raise RuntimeError("the oversample-hook library is not loaded (use_oversample_hooks)")
        L = _used(_oversample_hooks)
        ok = L.sauAmd_render_file_oversampled_with_backend(program.ptr, srate, factor, os.fsencode(path), fmt, channels,
                                                           backend, C.byref(n))
    if not ok:
        raise RuntimeError("sauAmd_render_file_oversampled failed: " + last_error(L))
    return n.value


def decimator_taps(factor):
    """sauAmd_decimator_taps: the decimating filter's L = 64 * factor + 1 taps as a float64 array (empty for a factor
    other than 2, 4, 8) -- the one definition the device, the file writer and the tests share."""
    L = lib()
    n = int(L.sauAmd_decimator_taps(int(factor), None, 0))
    out = np.zeros(n, np.float64)
    if n:
        L.sauAmd_decimator_taps(int(factor), out.ctypes.data_as(C.POINTER(C.c_double)), n)
    return out


def decimator_latency(factor):
    """sauAmd_decimator_latency: the filter's delay in output frames (32), 0 for a factor other than 2, 4, 8."""
    return int(lib().sauAmd_decimator_latency(int(factor)))


_loudness_hooks = None


def use_loudness_hooks(path):
    """tests/ only: load the library that runs the loudness-normalised file writer over an injected backend
    (tests/hooks_loudness: the product's object files + sauAmd_render_file_loudness_with_backend)."""
    global _loudness_hooks
    if _loudness_hooks is None:
        L = _declare(C.CDLL(path))
        L.sauAmd_render_file_loudness_with_backend.restype = C.c_bool
        L.sauAmd_render_file_loudness_with_backend.argtypes = [C.c_void_p, C.c_uint32, C.c_char_p, C.c_int, C.c_int, C.c_double,
                                                               C.c_float, C.c_void_p, C.POINTER(C.c_uint64),
                                                               C.POINTER(Loudness), C.POINTER(C.c_float)]
        _loudness_hooks = L
    return _loudness_hooks


def render_file_loudness(program, srate, path, fmt=SNDFILE_WAV, channels=1, target_lufs=-23.0, max_true_peak=1.0, backend=None):
    """sauAmd_render_file_loudness: render a whole program into a file at `target_lufs` integrated loudness (BS.1770) with its
    true peak held at or under `max_true_peak` -> (frames written, Loudness of the render before the gain, the gain). Two
    passes over the program: one that measures, one that writes x * gain. ``backend`` (tests): a sauengine::Backend* for the
    first pass, without a GPU."""
    n, ld, gain = C.c_uint64(), Loudness(), C.c_float()
    if backend is None:
        L = _used(lib())
        ok = L.sauAmd_render_file_loudness(program.ptr, srate, os.fsencode(path), fmt, channels, target_lufs, max_true_peak,
                                           C.byref(n), C.byref(ld), C.byref(gain))
    else:
        if _loudness_hooks is None:
            raise RuntimeError("the loudness-hook library is not loaded (use_loudness_hooks)")
        L = _used(_loudness_hooks)
        ok = L.sauAmd_render_file_loudness_with_backend(program.ptr, srate, os.fsencode(path), fmt, channels, target_lufs,
                                                        max_true_peak, backend, C.byref(n), C.byref(ld), C.byref(gain))
    if not ok:
        raise RuntimeError("sauAmd_render_file_loudness failed: " + last_error(L))
    return n.value, ld, gain.value


_limiter_hooks = None


def use_limiter_hooks(path):
    """tests/ only: load the library that runs the limited file writer over an injected backend
    (tests/hooks_limiter: the product's object files + sauAmd_render_file_loudness_limited_with_backend)."""
    global _limiter_hooks
    if _limiter_hooks is None:
        L = _declare(C.CDLL(path))
        L.sauAmd_render_file_loudness_limited_with_backend.restype = C.c_bool
        L.sauAmd_render_file_loudness_limited_with_backend.argtypes = [C.c_void_p, C.c_uint32, C.c_char_p, C.c_int, C.c_int,
                                                                       C.c_double, C.c_float, C.c_void_p, C.POINTER(C.c_uint64),
                                                                       C.POINTER(Loudness), C.POINTER(C.c_float),
                                                                       C.POINTER(LimiterStats)]
        _limiter_hooks = L
    return _limiter_hooks


def render_file_loudness_limited(program, srate, path, fmt=SNDFILE_WAV, channels=1, target_lufs=-23.0, max_true_peak=1.0,
                                 backend=None):
    """sauAmd_render_file_loudness_limited: render a whole program into a file at the gain that reaches `target_lufs`, with a
    look-ahead limiter holding every sample at or under `max_true_peak` -> (frames written, Loudness of the render before the
    gain, the gain, LimiterStats of the writing pass). ``backend`` (tests): a sauengine::Backend* for the first pass, without
    a GPU."""
    n, ld, gain, st = C.c_uint64(), Loudness(), C.c_float(), LimiterStats()
    if backend is None:
        L = _used(lib())
        ok = L.sauAmd_render_file_loudness_limited(program.ptr, srate, os.fsencode(path), fmt, channels, target_lufs,
                                                   max_true_peak, C.byref(n), C.byref(ld), C.byref(gain), C.byref(st))
    else:
        if _limiter_hooks is None:
            raise RuntimeError("the limiter-hook library is not loaded (use_limiter_hooks)")
        L = _used(_limiter_hooks)
        ok = L.sauAmd_render_file_loudness_limited_with_backend(program.ptr, srate, os.fsencode(path), fmt, channels, target_lufs,
                                                                max_true_peak, backend, C.byref(n), C.byref(ld), C.byref(gain),
                                                                C.byref(st))
    if not ok:
        raise RuntimeError("sauAmd_render_file_loudness_limited failed: " + last_error(L))
    return n.value, ld, gain.value, st


_spectrum_hooks = None


def use_spectrum_hooks(path):
    """tests/ only: load the library that runs sauAmd_render_spectrum over an injected backend and reaches the host's
    restatement of one segment and the spectrum meter's launch plan (tests/hooks_spectrum: the product's object files +
    sauAmd_render_spectrum_with_backend, sauAmd_spectrum_segment, sauAmd_spectrum_plan)."""
    global _spectrum_hooks
    if _spectrum_hooks is None:
        L = _declare(C.CDLL(path))
        L.sauAmd_render_spectrum_with_backend.restype = C.c_bool
        L.sauAmd_render_spectrum_with_backend.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_uint, C.c_uint32, C.c_void_p,
                                                          C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.sauAmd_spectrum_segment.restype = C.c_bool
        L.sauAmd_spectrum_segment.argtypes = [C.c_uint, C.c_void_p, C.c_size_t, C.POINTER(C.c_double)]
        L.sauAmd_spectrum_plan.restype = C.c_int
        L.sauAmd_spectrum_plan.argtypes = [C.c_uint, C.c_uint32, C.c_uint32, C.c_size_t, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32),
                                           C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        _spectrum_hooks = L
    return _spectrum_hooks


def spectrum_window(log2n):
    """sauAmd_spectrum_window: the periodic Hann window of N = 2^log2n float64 values (empty for log2n outside 8 .. 12) -- the
    one definition the device and the tests share."""
    L = lib()
    n = int(L.sauAmd_spectrum_window(int(log2n), None, 0))
    out = np.zeros(n, np.float64)
    if n:
        L.sauAmd_spectrum_window(int(log2n), out.ctypes.data_as(C.POINTER(C.c_double)), n)
    return out


def spectrum_twiddles(log2n):
    """sauAmd_spectrum_twiddles: the twiddles (cos, -sin)(2 pi k / N) as a float64 array [N/2, 2] (empty for log2n outside
    8 .. 12)."""
    L = lib()
    n = int(L.sauAmd_spectrum_twiddles(int(log2n), None, 0))
    out = np.zeros(n, np.float64)
    if n:
        L.sauAmd_spectrum_twiddles(int(log2n), out.ctypes.data_as(C.POINTER(C.c_double)), n)
    return out.reshape(-1, 2)


def render_spectrum(program, srate, factor=1, channels=1, log2n=11, hop=1024, backend=None):
    """sauAmd_render_spectrum: render a whole program (at srate * factor, decimated on the device, for factor 2, 4, 8) and sum
    the power spectra of its segments on the device, fetching no sample -> (float64 sums [channels, N/2+1], segments, frames
    measured). ``backend`` (tests): a sauengine::Backend* to run the same loop without a GPU."""
    log2n = int(log2n)
    bins = (1 << log2n) // 2 + 1 if 0 <= log2n < 31 else 1
    power = np.zeros((max(int(channels), 1), bins), np.float64)
    segs, n = C.c_uint64(), C.c_uint64()
    if backend is None:
        L = _used(lib())
        ok = L.sauAmd_render_spectrum(program.ptr, srate, factor, channels, log2n, hop, power.ctypes.data_as(C.POINTER(C.c_double)),
                                      C.byref(segs), C.byref(n))
    else:
        if _spectrum_hooks is None:
            raise RuntimeError("the spectrum-hook library is not loaded (use_spectrum_hooks)")
        L = _used(_spectrum_hooks)
        ok = L.sauAmd_render_spectrum_with_backend(program.ptr, srate, factor, channels, log2n, hop, backend,
                                                   power.ctypes.data_as(C.POINTER(C.c_double)), C.byref(segs), C.byref(n))
    if not ok:
        raise RuntimeError("sauAmd_render_spectrum failed: " + last_error(L))
    return power, segs.value, n.value


_flac_hooks = None


def use_flac_hooks(path):
    """tests/ only: load the library that runs sauAmd_render_file_flac over an injected backend and reaches the encoder's
    launch plan (tests/hooks_flac: the product's object files + sauAmd_render_file_flac_with_backend, sauAmd_flac_plan)."""
    global _flac_hooks
    if _flac_hooks is None:
        L = _declare(C.CDLL(path))
        L.sauAmd_render_file_flac_with_backend.restype = C.c_bool
        L.sauAmd_render_file_flac_with_backend.argtypes = [C.c_void_p, C.c_uint32, C.c_char_p, C.c_int, C.c_uint32, C.c_void_p,
                                                           C.POINTER(C.c_uint64), C.POINTER(FlacInfo)]
        L.sauAmd_flac_plan.restype = C.c_int
        L.sauAmd_flac_plan.argtypes = [C.c_uint32, C.c_uint32, C.c_size_t, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.c_int,
                                       C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        _flac_hooks = L
    return _flac_hooks


def flac_header(srate, channels, block_frames, info=None, bits=None, md5=None):
    """sauAmd_flac_header, or with ``bits`` (16 or 24) sauAmd_flac_header_bits: the 42 bytes ahead of the frames ("fLaC", the
    metadata block header, STREAMINFO) for a record (a FlacInfo, a dict of its fields, or None: an empty one); b"" for arguments
    that are refused. With ``md5`` (16 bytes) sauAmd_flac_header_md5: the same with the MD5 field filled in (bits None: 16)."""
    if isinstance(info, dict):
        info = FlacInfo(**info)
    out = (C.c_uint8 * 42)()
    ref = C.byref(info) if info is not None else None
    if md5 is not None:
        md5 = bytes(md5)
        if len(md5) != 16:
            raise ValueError("an MD5 digest is 16 bytes")
        n = lib().sauAmd_flac_header_md5(srate, channels, block_frames, 16 if bits is None else int(bits), ref, md5, out, 42)
    elif bits is None:
        n = lib().sauAmd_flac_header(srate, channels, block_frames, ref, out, 42)
    else:
        n = lib().sauAmd_flac_header_bits(srate, channels, block_frames, int(bits), ref, out, 42)
    return bytes(out) if n == 42 else b""


def flac_md5(samples, bits):
    """sauAmd_flac_md5: the MD5 of the interleaved samples as an encoder of ``bits`` (16 or 24) per sample with MD5 on makes it
    -> 16 bytes (None when the library refuses the bits or a sample that does not fit them)"""
    x = np.ascontiguousarray(samples, np.int32).reshape(-1)
    out = (C.c_uint8 * 16)()
    ok = lib().sauAmd_flac_md5(x.ctypes.data if x.size else None, x.size, int(bits), out)
    return bytes(out) if ok else None


def set_flac_file_md5(on):
    """sauAmd_set_flac_file_md5: the process-wide switch that makes the FLAC file writers fill STREAMINFO's MD5 field
    -> the previous value"""
    return int(lib().sauAmd_set_flac_file_md5(1 if on else 0))


def set_flac_file_verify(on):
    """sauAmd_set_flac_file_verify: the process-wide switch that makes the FLAC file writers decode every frame they made on the
    device and hold it against the samples (include/saugns_amd.h, FLAC, "Verify") -> the previous value"""
    return int(lib().sauAmd_set_flac_file_verify(1 if on else 0))


# sauAmd_flac_decode_block's statuses (SAU_AMD_FLAC_DEC_*)
FLAC_DEC_OK, FLAC_DEC_LENGTH, FLAC_DEC_SYNC, FLAC_DEC_HEADER, FLAC_DEC_NUMBER, FLAC_DEC_CRC8, FLAC_DEC_SUBFRAME, FLAC_DEC_RESIDUAL, \
    FLAC_DEC_PADDING, FLAC_DEC_CRC16, FLAC_DEC_RANGE, FLAC_DEC_MISMATCH = range(12)
FLAC_DEC_BAD_ARGUMENT = 255
FLAC_DEC_NAMES = ("OK", "LENGTH", "SYNC", "HEADER", "NUMBER", "CRC8", "SUBFRAME", "RESIDUAL", "PADDING", "CRC16", "RANGE", "MISMATCH")


def flac_decode_block(data, channels, block_frames, bits, frame_number, cap_frames=None):
    """sauAmd_flac_decode_block: the host's restatement of the decoder on the one frame that begins at ``data`` (bytes; the library
    is handed a buffer of exactly that length) -> (status, the frame's size in bytes, int32 samples [n, channels]); size 0 and no
    samples unless the status is FLAC_DEC_OK. ``cap_frames`` (tests): the room to state instead of block_frames'."""
    data = bytes(data)
    buf = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data if data else b"\0")
    B = int(block_frames) if int(block_frames) in (256, 512, 1024, 2048, 4096) else 4096
    cap = B if cap_frames is None else int(cap_frames)
    out = np.zeros((max(cap, 1), max(int(channels), 1)), np.int32)
    n, st = C.c_uint32(0), C.c_int(-1)
    size = lib().sauAmd_flac_decode_block(buf if data else None, len(data), int(channels), int(block_frames), int(bits), int(frame_number),
                                          out.ctypes.data if cap else None, cap, C.byref(n), C.byref(st))
    if st.value != FLAC_DEC_OK:
        assert size == 0 and n.value == 0, "a refused frame with a size or a length"
        return st.value, 0, None
    return st.value, int(size), out[:n.value].copy()


def flac_quantize(x, gain=1.0, bits=24):
    """sauAmd_flac_quantize: what a float-fed encoder of ``bits`` makes of the float32 samples x with ``gain`` -> int32 array
    (None when the library refuses the bits)"""
    x = np.ascontiguousarray(x, np.float32)
    out = np.zeros(x.shape, np.int32)
    ok = lib().sauAmd_flac_quantize(x.ctypes.data, x.size, float(gain), int(bits), out.ctypes.data)
    return out if ok else None


def flac_encode_block_s32(x, channels, block_frames, frame_number, bits=24, max_lpc_order=0):
    """sauAmd_flac_encode_block_s32: the host's restatement of one frame of ``bits`` per sample from interleaved int32 samples
    -> bytes (b"" when the arguments are refused)"""
    x = np.ascontiguousarray(x, np.int32)
    n = len(x) // max(int(channels), 1)
    L = lib()

    def call(out, cap):
        return L.sauAmd_flac_encode_block_s32(x.ctypes.data, n, channels, block_frames, frame_number, int(bits),
                                              _lpc_order(max_lpc_order), out, cap)
    size = call(None, 0)
    if not size:
        return b""
    out = (C.c_uint8 * size)()
    assert call(out, size) == size
    return bytes(out)


def flac_encode_block_lpc24(x, channels, block_frames, frame_number, max_lpc_order=0):
    """sauAmd_flac_encode_block_lpc24: the host's restatement of one 24-bit frame in the LPC mode ("LPC at 24 bits") from
    interleaved int32 samples -> bytes (b"" when the arguments are refused)"""
    x = np.ascontiguousarray(x, np.int32)
    n = len(x) // max(int(channels), 1)
    L = lib()

    def call(out, cap):
        return L.sauAmd_flac_encode_block_lpc24(x.ctypes.data, n, channels, block_frames, frame_number, _lpc_order(max_lpc_order), out, cap)
    size = call(None, 0)
    if not size:
        return b""
    out = (C.c_uint8 * size)()
    assert call(out, size) == size
    return bytes(out)


def _lpc_order(max_lpc_order):
    """0 .. 2^32 - 1 as the library takes it (it refuses what is above 8); anything else is refused here the same way"""
    m = int(max_lpc_order)
    return m if 0 <= m < 1 << 32 else 0xffffffff


def flac_encode_block(x, channels, block_frames, frame_number, max_lpc_order=0):
    """sauAmd_flac_encode_block, or with max_lpc_order != 0 sauAmd_flac_encode_block_lpc: the host's restatement of one frame,
    from interleaved int16 samples -> bytes (b"" when the arguments are refused)"""
    x = np.ascontiguousarray(x, np.int16)
    n = len(x) // max(int(channels), 1)
    L = lib()
    if max_lpc_order:
        def call(out, cap):
            return L.sauAmd_flac_encode_block_lpc(x.ctypes.data, n, channels, block_frames, frame_number, _lpc_order(max_lpc_order), out, cap)
    else:
        def call(out, cap):
            return L.sauAmd_flac_encode_block(x.ctypes.data, n, channels, block_frames, frame_number, out, cap)
    size = call(None, 0)
    if not size:
        return b""
    out = (C.c_uint8 * size)()
    assert call(out, size) == size
    return bytes(out)


def render_file_flac(program, srate, path, channels=1, block_frames=0, backend=None, max_lpc_order=0):
    """sauAmd_render_file_flac, or with max_lpc_order != 0 sauAmd_render_file_flac_lpc: render a whole program into a FLAC file,
    encoded on the device -> (frames, FlacInfo). ``backend`` (tests): a sauengine::Backend* to run the same writer without a
    GPU (without the LPC mode)."""
    n, info = C.c_uint64(), FlacInfo()
    if backend is None and max_lpc_order:
        L = _used(lib())
        ok = L.sauAmd_render_file_flac_lpc(program.ptr, srate, os.fsencode(path), channels, block_frames, _lpc_order(max_lpc_order),
                                           C.byref(n), C.byref(info))
    elif backend is None:
        L = _used(lib())
        ok = L.sauAmd_render_file_flac(program.ptr, srate, os.fsencode(path), channels, block_frames, C.byref(n), C.byref(info))
    elif max_lpc_order:
        raise ValueError("the FLAC-hook library runs the writer without the LPC mode")
    else:
        if _flac_hooks is None:
            raise RuntimeError("the FLAC-hook library is not loaded (use_flac_hooks)")
        L = _used(_flac_hooks)
        ok = L.sauAmd_render_file_flac_with_backend(program.ptr, srate, os.fsencode(path), channels, block_frames, backend,
                                                    C.byref(n), C.byref(info))
    if not ok:
        raise RuntimeError("sauAmd_render_file_flac failed: " + last_error(L))
    return n.value, info


def dither_preset(shape, seed=0):
    """sauAmd_dither_preset: the Dither spec of a preset (DITHER_FLAT, _HP1, _E3, _E5, _F9) with TPDF dither of ``seed``"""
    d = Dither()
    if not lib().sauAmd_dither_preset(int(shape), int(seed) & (2**64 - 1), C.byref(d)):
        raise ValueError("sauAmd_dither_preset refused shape %r" % (shape,))
    return d


def dither_quantize(x, channels, gain, spec, row=0, first_frame=0, history=None):
    """sauAmd_dither_quantize: the host's restatement of a quantiser, from the same source as the kernels. x: float32 samples,
    ``channels`` interleaved, the frames from ``first_frame`` on of the quantiser's row ``row``. ``history``: float64
    [channels, 9], the errors 1 .. 9 frames back (None: zeros) -> (int16 samples, the history behind them, [clipped per
    channel]). Raises ValueError on what the library refuses."""
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    frames = x.size // channels if channels in (1, 2) else 0
    h = np.zeros((max(int(channels), 1), 9), np.float64) if history is None else np.array(history, np.float64).reshape(channels, 9)
    out = np.zeros(x.size, np.int16)
    cl = (C.c_uint64 * 2)()
    if not lib().sauAmd_dither_quantize(x.ctypes.data, frames, int(channels), float(gain), C.byref(spec), int(row), int(first_frame),
                                        h.ctypes.data, out.ctypes.data, cl):
        raise ValueError("sauAmd_dither_quantize refused its arguments")
    return out, h, [int(cl[0]), int(cl[1])]


def render_file_dithered(program, srate, path, spec, fmt=SNDFILE_WAV, channels=1, gain=1.0):
    """sauAmd_render_file_dithered: render a whole program in float32 into a 16-bit RAW, AU or WAV file, scaled by ``gain`` and
    quantised on the device with the Dither ``spec`` -> (frames written, DitherStats as a dict)."""
    n, st = C.c_uint64(), DitherStats()
    L = _used(lib())
    if not L.sauAmd_render_file_dithered(program.ptr, srate, os.fsencode(path), fmt, channels, float(gain), C.byref(spec),
                                         C.byref(n), C.byref(st)):
        raise RuntimeError("sauAmd_render_file_dithered failed: " + last_error(L))
    return n.value, st.as_dict()


def render_file_flac_dithered(program, srate, path, spec, channels=1, block_frames=0, max_lpc_order=0, gain=1.0):
    """sauAmd_render_file_flac_dithered: the same samples into a 16-bit FLAC file, encoded on the device
    -> (frames, FlacInfo, DitherStats as a dict)."""
    n, info, st = C.c_uint64(), FlacInfo(), DitherStats()
    L = _used(lib())
    if not L.sauAmd_render_file_flac_dithered(program.ptr, srate, os.fsencode(path), channels, block_frames, _lpc_order(max_lpc_order),
                                              float(gain), C.byref(spec), C.byref(n), C.byref(info), C.byref(st)):
        raise RuntimeError("sauAmd_render_file_flac_dithered failed: " + last_error(L))
    return n.value, info, st.as_dict()


def render_file_loudness_dithered(program, srate, path, spec, fmt=SNDFILE_WAV, channels=1, target_lufs=-23.0, max_true_peak=1.0):
    """sauAmd_render_file_loudness_dithered: render_file_loudness's measuring pass and gain, then render_file_dithered's pass
    with that gain -> (frames written, Loudness of the render before the gain, the gain, DitherStats as a dict)."""
    n, ld, gain, st = C.c_uint64(), Loudness(), C.c_float(), DitherStats()
    L = _used(lib())
    if not L.sauAmd_render_file_loudness_dithered(program.ptr, srate, os.fsencode(path), fmt, channels, target_lufs, max_true_peak,
                                                  C.byref(spec), C.byref(n), C.byref(ld), C.byref(gain), C.byref(st)):
        raise RuntimeError("sauAmd_render_file_loudness_dithered failed: " + last_error(L))
    return n.value, ld, gain.value, st.as_dict()


_flac24_hooks = None


def use_flac24_hooks(path):
    """tests/ only: load the library that runs the float-fed FLAC writers over an injected backend and reaches the encoder's
    launch plan at a sample width (tests/hooks_flac24: the product's object files + the two _with_backend entry points and
    sauAmd_flac_plan_bits)."""
    global _flac24_hooks
    if _flac24_hooks is None:
        L = _declare(C.CDLL(path))
        L.sauAmd_render_file_flac_f32_with_backend.restype = C.c_bool
        L.sauAmd_render_file_flac_f32_with_backend.argtypes = [C.c_void_p, C.c_uint32, C.c_char_p, C.c_int, C.c_uint32, C.c_int,
                                                               C.c_uint32, C.c_float, C.c_void_p, C.POINTER(C.c_uint64),
                                                               C.POINTER(FlacInfo)]
        L.sauAmd_render_file_flac_loudness_with_backends.restype = C.c_bool
        L.sauAmd_render_file_flac_loudness_with_backends.argtypes = [C.c_void_p, C.c_uint32, C.c_char_p, C.c_int, C.c_uint32, C.c_int,
                                                                     C.c_uint32, C.c_double, C.c_float, C.c_int, C.c_void_p, C.c_void_p,
                                                                     C.POINTER(C.c_uint64)]
        L.sauAmd_flac_plan_bits.restype = C.c_int
        L.sauAmd_flac_plan_bits.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_size_t, C.POINTER(C.c_uint64),
                                            C.POINTER(C.c_uint32), C.c_int, C.POINTER(C.c_uint64)]
        _flac24_hooks = L
    return _flac24_hooks


def render_file_flac_f32(program, srate, path, channels=1, block_frames=0, bits=24, max_lpc_order=0, gain=1.0, backend=None):
    """sauAmd_render_file_flac_f32: render a whole program in float32 into a FLAC file of ``bits`` per sample, scaled by
    ``gain``, quantised and encoded on the device -> (frames, FlacInfo). ``backend`` (tests): a sauengine::Backend* to run the
    same writer without a GPU."""
    n, info = C.c_uint64(), FlacInfo()
    if backend is None:
        L = _used(lib())
        ok = L.sauAmd_render_file_flac_f32(program.ptr, srate, os.fsencode(path), channels, block_frames, int(bits),
                                           _lpc_order(max_lpc_order), gain, C.byref(n), C.byref(info))
    else:
        if _flac24_hooks is None:
            raise RuntimeError("the FLAC-24 hook library is not loaded (use_flac24_hooks)")
        L = _used(_flac24_hooks)
        ok = L.sauAmd_render_file_flac_f32_with_backend(program.ptr, srate, os.fsencode(path), channels, block_frames, int(bits),
                                                        _lpc_order(max_lpc_order), gain, backend, C.byref(n), C.byref(info))
    if not ok:
        raise RuntimeError("sauAmd_render_file_flac_f32 failed: " + last_error(L))
    return n.value, info


def render_file_flac_loudness(program, srate, path, channels=1, block_frames=0, bits=24, max_lpc_order=0, target_lufs=-23.0,
                              max_true_peak=1.0, limited=False, backends=None):
    """sauAmd_render_file_flac_loudness: the loudness-normalised writer (``limited``: the limited one) with FLAC output of
    ``bits`` per sample -> (frames, Loudness, gain, LimiterStats or None, FlacInfo). ``backends`` (tests): two
    sauengine::Backend*, one per pass, to run the same writer without a GPU."""
    n, ld, gain, st, info = C.c_uint64(), Loudness(), C.c_float(), LimiterStats(), FlacInfo()
    if backends is None:
        L = _used(lib())
        ok = L.sauAmd_render_file_flac_loudness(program.ptr, srate, os.fsencode(path), channels, block_frames, int(bits),
                                                _lpc_order(max_lpc_order), target_lufs, max_true_peak, 1 if limited else 0,
                                                C.byref(n), C.byref(ld), C.byref(gain), C.byref(st), C.byref(info))
    else:
        if _flac24_hooks is None:
            raise RuntimeError("the FLAC-24 hook library is not loaded (use_flac24_hooks)")
        L = _used(_flac24_hooks)
        ok = L.sauAmd_render_file_flac_loudness_with_backends(program.ptr, srate, os.fsencode(path), channels, block_frames,
                                                              int(bits), _lpc_order(max_lpc_order), target_lufs, max_true_peak,
                                                              1 if limited else 0, backends[0], backends[1], C.byref(n))
    if not ok:
        raise RuntimeError("sauAmd_render_file_flac_loudness failed: " + last_error(L))
    return n.value, ld, gain.value, (st if limited else None), info


def render_file_flac_lpc24(program, srate, path, channels=1, block_frames=0, max_lpc_order=0, gain=1.0):
    """sauAmd_render_file_flac_lpc24: render_file_flac_f32 at 24 bits with the encoder of "LPC at 24 bits" -> (frames, FlacInfo)"""
    n, info = C.c_uint64(), FlacInfo()
    L = _used(lib())
    if not L.sauAmd_render_file_flac_lpc24(program.ptr, srate, os.fsencode(path), channels, block_frames, _lpc_order(max_lpc_order),
                                           gain, C.byref(n), C.byref(info)):
        raise RuntimeError("sauAmd_render_file_flac_lpc24 failed: " + last_error(L))
    return n.value, info


def render_file_flac_loudness_lpc24(program, srate, path, channels=1, block_frames=0, max_lpc_order=0, target_lufs=-23.0,
                                    max_true_peak=1.0, limited=False):
    """sauAmd_render_file_flac_loudness_lpc24: render_file_flac_loudness at 24 bits with the encoder of "LPC at 24 bits"
    -> (frames, Loudness, gain, LimiterStats or None, FlacInfo)"""
    n, ld, gain, st, info = C.c_uint64(), Loudness(), C.c_float(), LimiterStats(), FlacInfo()
    L = _used(lib())
    if not L.sauAmd_render_file_flac_loudness_lpc24(program.ptr, srate, os.fsencode(path), channels, block_frames,
                                                    _lpc_order(max_lpc_order), target_lufs, max_true_peak, 1 if limited else 0,
                                                    C.byref(n), C.byref(ld), C.byref(gain), C.byref(st), C.byref(info)):
        raise RuntimeError("sauAmd_render_file_flac_loudness_lpc24 failed: " + last_error(L))
    return n.value, ld, gain.value, (st if limited else None), info


def limiter_window(srate):
    """sauAmd_limiter_window: the limiter's smoothing window h, 2 A + 1 float64 values, for a rate (empty for rate 0) -- the
    one definition the device, the writer and the tests share."""
    L = lib()
    n = int(L.sauAmd_limiter_window(int(srate), None, 0))
    out = np.zeros(n, np.float64)
    if n:
        L.sauAmd_limiter_window(int(srate), out.ctypes.data_as(C.POINTER(C.c_double)), n)
    return out


def limiter_latency(srate):
    """sauAmd_limiter_latency: the limiter's delay D = 2 A + 16 in frames for a rate (0 for rate 0)."""
    return int(lib().sauAmd_limiter_latency(int(srate)))


def loudness_filter(srate):
    """sauAmd_loudness_filter: the K-weighting coefficients b0 b1 b2 a1 a2, b0' b1' b2' a1' a2' for a rate as a float64 array
    of ten -- the one definition the device, the writer and the tests share; None below 2560 Hz."""
    out = np.zeros(10, np.float64)
    ok = lib().sauAmd_loudness_filter(int(srate), out.ctypes.data_as(C.POINTER(C.c_double)))
    return out if ok else None


def truepeak_taps():
    """sauAmd_truepeak_taps: the 4x true-peak interpolator's 129 taps g (not normalised) as a float64 array."""
    L = lib()
    n = int(L.sauAmd_truepeak_taps(None, 0))
    out = np.zeros(n, np.float64)
    L.sauAmd_truepeak_taps(out.ctypes.data_as(C.POINTER(C.c_double)), n)
    return out


def loudness_gate(hops, hop_frames, channels):
    """sauAmd_loudness_gate: BS.1770 gating of complete hop energies [n][2] (float64) -> Loudness (frames = n * hop_frames)."""
    h = np.ascontiguousarray(hops, dtype=np.float64).reshape(-1, 2)
    out = Loudness()
    if not _used(lib()).sauAmd_loudness_gate(h.ctypes.data_as(C.POINTER(C.c_double)), len(h), int(hop_frames), int(channels),
                                             C.byref(out)):
        raise RuntimeError("sauAmd_loudness_gate failed: " + last_error(lib()))
    return out


def get_piluts():
    p = lib().sauAmd_get_piluts()
    return np.ctypeslib.as_array(p, shape=(12 * 2048,)).reshape(12, 2048).copy()


class Program:
    """A ``sauProgram`` in host memory: from an image, or borrowed from a parser."""

    def __init__(self, ptr, owner=None, free=None):
        self.ptr = ptr
        self._owner = owner
        self._free = free

    @classmethod
    def from_image(cls, blob):
        buf = bytes(blob)
        p = lib().sauAmd_program_load(buf, len(buf))
        if not p:
            raise ValueError("not a valid SAUPIMG1 program image")
        return cls(p, free=lib().sauAmd_program_free)

    @classmethod
    def borrow(cls, ptr, owner=None):
        return cls(ptr, owner=owner)

    def image(self):
        n = lib().sauAmd_program_serialize(self.ptr, None, 0)
        buf = C.create_string_buffer(n)
        lib().sauAmd_program_serialize(self.ptr, buf, n)
        return buf.raw

    @property
    def struct(self):
        return SauProgram.from_address(self.ptr)

    def __del__(self):
        if getattr(self, "_free", None) and self.ptr:
            self._free(self.ptr)
            self.ptr = None


class Generator:
    """sau_create_Generator / sauGenerator_run / sau_destroy_Generator."""

    def __init__(self, program, srate, backend=None):
        self._prg = program  # borrowed by the C side: keep alive
        self._L = _used(lib() if backend is None else hooks())
        if backend is None:
            self._g = self._L.sau_create_Generator(program.ptr, srate)
        else:  # tests: an injected backend (owned by the generator from here on), in the hook library
            self._g = self._L.sauAmd_create_Generator_with_backend(program.ptr, srate, backend)
        if not self._g:
            raise RuntimeError("sau_create_Generator returned NULL: " + last_error(self._L))

    def run(self, buf, buf_len, stereo=False):
        """-> (more, out_len); buf is an int16 numpy array of buf_len*(1|2)."""
        n = C.c_size_t()
        more = _used(self._L).sauGenerator_run(self._g, buf.ctypes.data, buf_len, stereo, C.byref(n))
        return bool(more), n.value

    def render(self, stereo=False, chunk=11289, max_frames=0):
        ch = 2 if stereo else 1
        buf = np.zeros(chunk * ch, np.int16)
        out, total = [], 0
        while True:
            more, n = self.run(buf, chunk, stereo)
            out.append(buf[: n * ch].copy())
            total += n
            if not more or (max_frames and total >= max_frames):
                break
        pcm = np.concatenate(out) if out else np.zeros(0, np.int16)
        return pcm[: max_frames * ch] if max_frames else pcm

    def rewinds(self):
        """tests: how often a call of another size / channel layout took the read-ahead back (hook library only)"""
        return int(self._L.sauAmd_Generator_rewinds(self._g))

    def close(self):
        if getattr(self, "_g", None):
            self._L.sau_destroy_Generator(self._g)
            self._g = None

    def __del__(self):
        self.close()


class Batch:
    """Many programs rendered in lock step (sauAmd_*Batch*)."""

    def __init__(self, programs, srate, backend=None, device=None):
        """device: the HIP device of this process to render on (sauAmd_create_Batch_on); None: SAU_AMD_DEVICE's, else device 0"""
        self._prgs = list(programs)
        self.n = len(self._prgs)
        arr = (C.c_void_p * self.n)(*[p.ptr for p in self._prgs])
        self._L = _used(lib() if backend is None else hooks())
        if backend is None and device is not None:
            self._b = self._L.sauAmd_create_Batch_on(int(device), arr, self.n, srate)
        elif backend is None:
            self._b = self._L.sauAmd_create_Batch(arr, self.n, srate)
        else:  # tests only: host control plane on an injected executor, in the hook library
            self._b = self._L.sauAmd_create_Batch_with_backend(arr, self.n, srate, backend)
        if not self._b:
            raise RuntimeError("sauAmd_create_Batch returned NULL: " + last_error(self._L))

    def run(self, buf_len, stereo=False, fetch=True):
        """-> (pcm [n, buf_len*ch] or None, more[n], out_len[n])"""
        ch = 2 if stereo else 1
        more = (C.c_bool * self.n)()
        lens = (C.c_size_t * self.n)()
        if fetch:
            pcm = np.zeros((self.n, buf_len * ch), np.int16)
            ptrs = (C.c_void_p * self.n)(*[pcm[i].ctypes.data for i in range(self.n)])
        else:
            pcm, ptrs = None, None
        ok = _used(self._L).sauAmd_Batch_run(self._b, ptrs, buf_len, stereo, more, lens)
        if not ok:
            raise RuntimeError("sauAmd_Batch_run failed: " + last_error(self._L))
        return pcm, [bool(m) for m in more], [int(x) for x in lens]

    def run_f32(self, buf_len, stereo=False, fetch=True):
        """sauAmd_Batch_run_f32: the same run with the mixers' float32 samples, neither clamped nor rounded
        -> (float32 pcm [n, buf_len*ch] or None, more[n], out_len[n]). May alternate with run() on one batch."""
        ch = 2 if stereo else 1
        more = (C.c_bool * self.n)()
        lens = (C.c_size_t * self.n)()
        if fetch:
            pcm = np.zeros((self.n, buf_len * ch), np.float32)
            ptrs = (C.c_void_p * self.n)(*[pcm[i].ctypes.data for i in range(self.n)])
        else:
            pcm, ptrs = None, None
        ok = _used(self._L).sauAmd_Batch_run_f32(self._b, ptrs, buf_len, stereo, more, lens)
        if not ok:
            raise RuntimeError("sauAmd_Batch_run_f32 failed: " + last_error(self._L))
        return pcm, [bool(m) for m in more], [int(x) for x in lens]

    def run_decimated(self, factor, buf_len, stereo=False, fetch=True):
        """sauAmd_Batch_run_decimated_f32: a float run of buf_len * factor frames (the batch was created at the output rate
        times `factor`), decimated on the device to buf_len frames per stream
        -> (float32 [n, buf_len*ch] or None, more[n], out_len[n]); out_len = ceil(the float run's / factor). Every row holds
        buf_len valid frames, a stream's filter tail included; the rows stay on the device (device_decimated_f32)."""
        ch = 2 if stereo else 1
        more = (C.c_bool * self.n)()
        lens = (C.c_size_t * self.n)()
        if fetch:
            pcm = np.zeros((self.n, buf_len * ch), np.float32)
            ptrs = (C.c_void_p * self.n)(*[pcm[i].ctypes.data for i in range(self.n)])
        else:
            pcm, ptrs = None, None
        ok = _used(self._L).sauAmd_Batch_run_decimated_f32(self._b, int(factor), ptrs, buf_len, stereo, more, lens)
        if not ok:
            raise RuntimeError("sauAmd_Batch_run_decimated_f32 failed: " + last_error(self._L))
        return pcm, [bool(m) for m in more], [int(x) for x in lens]

    def device_decimated_f32(self, stream):
        """Device address of the stream's decimated float32 row of the last decimated run; None before one."""
        return self._L.sauAmd_Batch_device_decimated_f32(self._b, stream)

    def device_decimated_pitch(self):
        """Bytes between the decimated rows of consecutive streams (a multiple of 256)."""
        return int(self._L.sauAmd_Batch_device_decimated_pitch(self._b))

    def render(self, stereo=False, chunk=11289, max_frames=0):
        """Render every stream to its end -> list of int16 arrays."""
        ch = 2 if stereo else 1
        outs = [[] for _ in range(self.n)]
        alive = [True] * self.n
        total = 0
        while any(alive):
            pcm, more, lens = self.run(chunk, stereo)
            for i in range(self.n):
                if alive[i]:
                    outs[i].append(pcm[i, : lens[i] * ch].copy())
                    alive[i] = more[i]
            total += chunk
            if max_frames and total >= max_frames:
                break
        res = [np.concatenate(o) if o else np.zeros(0, np.int16) for o in outs]
        return [r[: max_frames * ch] for r in res] if max_frames else res

    def set_call_len(self, frames):
        """The sauGenerator_run call size whose block lattice the batch reproduces (0: every run
        is one call)."""
        self._L.sauAmd_Batch_set_call_len(self._b, frames)

    def order_after(self, before):
        """This batch's next run renders on the device only when everything issued for `before` has finished
        (sauAmd_Batch_order_after): scripts one after the other with two generators alive."""
        if not self._L.sauAmd_Batch_order_after(self._b, before._b):
            raise RuntimeError(last_error(self._L))

    def sync(self):
        if not self._L.sauAmd_Batch_sync(self._b):
            raise RuntimeError(last_error(self._L))

    def timing(self, reset=False):
        r, m, n = C.c_double(), C.c_double(), C.c_uint64()
        self._L.sauAmd_Batch_timing(self._b, C.byref(r), C.byref(m), C.byref(n), int(reset))
        return r.value, m.value, n.value

    def set_timing(self, level):
        self._L.sauAmd_Batch_set_timing(self._b, int(level))

    def timing_ex(self, reset=False):
        """-> dict of accumulated kernel times (ms) and the number of segments."""
        out = (C.c_double * 4)()
        n = C.c_uint64()
        self._L.sauAmd_Batch_timing_ex(self._b, out, C.byref(n), int(reset))
        return {"fast_ms": out[0], "block_ms": out[1], "mix_ms": out[2], "aux_ms": out[3],
                "segments": n.value}

    def set_metering(self, on):
        """sauAmd_Batch_set_metering: from the next run on, every run ends with the device measuring each stream's frames of
        that run into the stream's Levels record (off by default; off costs nothing)."""
        if not _used(self._L).sauAmd_Batch_set_metering(self._b, 1 if on else 0):
            raise RuntimeError("sauAmd_Batch_set_metering failed: " + last_error(self._L))

    def levels(self, reset=False):
        """sauAmd_Batch_levels: wait for the batch's stream -> the streams' accumulated records, a list of Levels."""
        out = (Levels * self.n)()
        if not _used(self._L).sauAmd_Batch_levels(self._b, out, 1 if reset else 0):
            raise RuntimeError("sauAmd_Batch_levels failed: " + last_error(self._L))
        return list(out)

    def measure_rows(self, ptr, pitch, n_rows, f32, frames, channels):
        """sauAmd_Batch_measure_rows: measure n_rows rows of device memory at `ptr`, `pitch` bytes apart, of `frames` frames of
        `channels` float32 (f32) or int16 samples -> a list of Levels. ptr and pitch must be multiples of 16."""
        out = (Levels * max(int(n_rows), 1))()
        if not _used(self._L).sauAmd_Batch_measure_rows(self._b, ptr, pitch, n_rows, 1 if f32 else 0, frames, channels, out):
            raise RuntimeError("sauAmd_Batch_measure_rows failed: " + last_error(self._L))
        return list(out)[:int(n_rows)]

    def set_loudness(self, on):
        """sauAmd_Batch_set_loudness: from the next run on, every float32 run ends with the device taking each stream's frames
        of that run into the stream's loudness record; int16 and decimated runs are refused while on (off by default)."""
        if not _used(self._L).sauAmd_Batch_set_loudness(self._b, 1 if on else 0):
            raise RuntimeError("sauAmd_Batch_set_loudness failed: " + last_error(self._L))

    def loudness(self, reset=False):
        """sauAmd_Batch_loudness: wait for the batch's stream -> the streams' records, a list of Loudness."""
        out = (Loudness * self.n)()
        if not _used(self._L).sauAmd_Batch_loudness(self._b, out, 1 if reset else 0):
            raise RuntimeError("sauAmd_Batch_loudness failed: " + last_error(self._L))
        return list(out)

    def loudness_hops(self, stream):
        """sauAmd_Batch_loudness_hops: the stream's complete 100 ms hop energies, float64 [hops, 2]."""
        L = _used(self._L)
        n = int(L.sauAmd_Batch_loudness_hops(self._b, stream, None, 0))
        out = np.zeros((n, 2), np.float64)
        if n and int(L.sauAmd_Batch_loudness_hops(self._b, stream, out.ctypes.data_as(C.POINTER(C.c_double)), n)) != n:
            raise RuntimeError("sauAmd_Batch_loudness_hops failed: " + last_error(self._L))
        return out

    def measure_loudness_rows(self, ptr, pitch, n_rows, frames, channels, srate):
        """sauAmd_Batch_measure_loudness_rows: measure n_rows float32 rows of device memory at `ptr`, `pitch` bytes apart, of
        `frames` frames of `channels` samples at the rate `srate`, from zero state -> (a list of Loudness, the rows' complete
        hop energies as float64 [n_rows, hops, 2]). ptr and pitch must be multiples of 16."""
        n_rows, frames, srate = int(n_rows), int(frames), int(srate)
        nh = frames // (srate // 10) if srate >= 10 else 0
        out = (Loudness * max(n_rows, 1))()
        hops = np.zeros((n_rows, nh, 2), np.float64)
        if not _used(self._L).sauAmd_Batch_measure_loudness_rows(self._b, ptr, pitch, n_rows, frames, channels, srate, out,
                                                                 hops.ctypes.data_as(C.POINTER(C.c_double)), hops.size):
            raise RuntimeError("sauAmd_Batch_measure_loudness_rows failed: " + last_error(self._L))
        return list(out)[:n_rows], hops

    def run_limited(self, pre_gain, ceiling, buf_len, stereo=False, fetch=True):
        """sauAmd_Batch_run_limited_f32: a float run of buf_len frames, limited on the device
        -> (float32 [n, buf_len*ch] or None, more[n], out_len[n]) with more and out_len the float run's. Every row holds buf_len
        valid frames of the sequence delayed by limiter_latency(rate); the rows stay on the device (device_limited_f32)."""
        ch = 2 if stereo else 1
        more = (C.c_bool * self.n)()
        lens = (C.c_size_t * self.n)()
        if fetch:
            pcm = np.zeros((self.n, buf_len * ch), np.float32)
            ptrs = (C.c_void_p * self.n)(*[pcm[i].ctypes.data for i in range(self.n)])
        else:
            pcm, ptrs = None, None
        ok = _used(self._L).sauAmd_Batch_run_limited_f32(self._b, pre_gain, ceiling, ptrs, buf_len, stereo, more, lens)
        if not ok:
            raise RuntimeError("sauAmd_Batch_run_limited_f32 failed: " + last_error(self._L))
        return pcm, [bool(m) for m in more], [int(x) for x in lens]

    def device_limited_f32(self, stream):
        """Device address of the stream's limited float32 row of the last limited run; None before one."""
        return self._L.sauAmd_Batch_device_limited_f32(self._b, stream)

    def device_limited_pitch(self):
        """Bytes between the limited rows of consecutive streams (a multiple of 256)."""
        return int(self._L.sauAmd_Batch_device_limited_pitch(self._b))

    def limiter_stats(self, reset=False):
        """sauAmd_Batch_limiter_stats: wait for the batch's stream -> the streams' records, a list of LimiterStats."""
        out = (LimiterStats * self.n)()
        if not _used(self._L).sauAmd_Batch_limiter_stats(self._b, out, 1 if reset else 0):
            raise RuntimeError("sauAmd_Batch_limiter_stats failed: " + last_error(self._L))
        return list(out)

    def limit_rows(self, ptr, pitch, n_rows, frames, channels, srate, pre_gain, ceiling, out_ptr, out_pitch):
        """sauAmd_Batch_limit_rows: the limiter from zero history on n_rows float32 rows of device memory at `ptr`, `pitch`
        bytes apart, into the float32 rows at `out_ptr`, `out_pitch` bytes apart, time-aligned -> a list of LimiterStats."""
        n_rows = int(n_rows)
        out = (LimiterStats * max(n_rows, 1))()
        if not _used(self._L).sauAmd_Batch_limit_rows(self._b, ptr, pitch, n_rows, int(frames), channels, int(srate), pre_gain,
                                                      ceiling, out_ptr, out_pitch, out):
            raise RuntimeError("sauAmd_Batch_limit_rows failed: " + last_error(self._L))
        return list(out)[:n_rows]

    def create_spectrum(self, n_rows, channels, log2n, hop):
        """sauAmd_Batch_create_spectrum: a Spectrum of n_rows records on the batch's device and stream. Close it before the
        batch."""
        return Spectrum(self, n_rows, channels, log2n, hop)

    def spectrum_rows(self, ptr, pitch, n_rows, frames, channels, log2n, hop, spectrogram=False, spectrogram_cap=None):
        """sauAmd_Batch_spectrum_rows: the summed power spectra of n_rows float32 rows of device memory at `ptr`, `pitch` bytes
        apart, of `frames` frames of `channels` samples, from empty records -> (float64 sums [n_rows, channels, N/2+1], the
        segments per row as a list[, the spectrogram, float32 [n_rows, channels, S, N/2+1]]). ``spectrogram_cap`` (tests): the
        capacity to state instead of the array's."""
        n_rows, frames, log2n = int(n_rows), int(frames), int(log2n)
        ok_l = 8 <= log2n <= 12
        N = 1 << log2n if ok_l else 2
        bins = N // 2 + 1
        S = 0 if (frames < N or not hop or not ok_l) else (frames - N) // int(hop) + 1
        ch = max(int(channels), 1)
        power = np.zeros((max(n_rows, 1), ch, bins), np.float64)
        segs = (C.c_uint64 * max(n_rows, 1))()
        gram = np.zeros((max(n_rows, 1), ch, S, bins), np.float32) if spectrogram else None
        cap = (gram.size if gram is not None else 0) if spectrogram_cap is None else int(spectrogram_cap)
        if not _used(self._L).sauAmd_Batch_spectrum_rows(self._b, ptr, pitch, n_rows, frames, channels, log2n, hop,
                                                        power.ctypes.data_as(C.POINTER(C.c_double)), segs,
                                                        gram.ctypes.data_as(C.POINTER(C.c_float)) if gram is not None else None, cap):
            raise RuntimeError("sauAmd_Batch_spectrum_rows failed: " + last_error(self._L))
        out = (power[:n_rows], [int(x) for x in segs][:n_rows])
        return out + (gram[:n_rows],) if spectrogram else out

    def create_flac(self, n_rows, channels, block_frames=0, max_lpc_order=0):
        """sauAmd_Batch_create_flac, or with max_lpc_order != 0 sauAmd_Batch_create_flac_lpc: a Flac encoder of n_rows streams on
        the batch's device and stream. Close it before the batch."""
        return Flac(self, n_rows, channels, block_frames, max_lpc_order)

    def create_flac_f32(self, n_rows, channels, block_frames=0, bits=24, max_lpc_order=0):
        """sauAmd_Batch_create_flac_f32: a float-fed Flac encoder of ``bits`` (16 or 24) per sample; ``feed_f32`` takes float
        rows and per-row gains. Close it before the batch."""
        return Flac(self, n_rows, channels, block_frames, max_lpc_order, bits=bits)

    def create_flac_lpc24(self, n_rows, channels, block_frames=0, max_lpc_order=0):
        """sauAmd_Batch_create_flac_lpc24: a float-fed Flac encoder of 24 bits per sample in the LPC mode ("LPC at 24 bits");
        fed, read and closed like create_flac_f32's. Close it before the batch."""
        return Flac(self, n_rows, channels, block_frames, max_lpc_order, bits=24, lpc24=True)

    def create_flac_lpc(self, n_rows, channels, block_frames=0, max_lpc_order=0):
        """(tests) sauAmd_Batch_create_flac_lpc whatever max_lpc_order is -- create_flac reaches it only with an order above 0 --:
        with 0 the encoder create_flac makes, by the other entry point"""
        return Flac(self, n_rows, channels, block_frames, max_lpc_order, lpc_entry=True)

    def create_quantizer(self, n_rows, channels, spec):
        """sauAmd_Batch_create_quantizer: a Quantizer of n_rows streams with the Dither ``spec`` on the batch's device and
        stream. Close it before the batch."""
        return Quantizer(self, n_rows, channels, spec)

    def device_pcm(self, stream):
        """Device address of the stream's int16 row of the last run; None after a float32 run."""
        return self._L.sauAmd_Batch_device_pcm(self._b, stream)

    def device_pcm_f32(self, stream):
        """Device address of the stream's float32 row of the last run; None after an int16 run."""
        return self._L.sauAmd_Batch_device_pcm_f32(self._b, stream)

    def device_pcm_pitch(self):
        """Bytes between the rows of consecutive streams, in the last run's format."""
        return int(self._L.sauAmd_Batch_device_pcm_pitch(self._b))

    def device_tensor(self, frames, stereo=False):
        """The last run's PCM rows as a torch tensor [n, frames, ch] on the batch's device -- int16 after run(), float32 after
        run_f32() -- that ALIASES the device rows: no copy. Call sync() first (the run is asynchronous). The tensor is valid
        until the batch's next run or close(); `frames` and `stereo` are those of the last run (or fewer frames).
        A process has room for one HIP runtime, and torch's wheels bring their own: import torch before the first saugns_amd
        call (as bench.py does), so that the library binds to the runtime torch has loaded."""
        import torch  # (only here: the binding itself does not need torch)
        if not torch.cuda.is_available():
            raise RuntimeError("torch sees no GPU in this process: import torch before the first saugns_amd call "
                               "(torch loads a HIP runtime of its own, and the one loaded first has the device)")
        f32 = self.device_pcm_f32(0)
        ptr = f32 or self.device_pcm(0)
        if not ptr:
            raise RuntimeError("no device PCM: nothing has run yet, or the backend keeps none")
        size = 4 if f32 else 2
        ch = 2 if stereo else 1
        pitch = self.device_pcm_pitch()
        if frames * ch * size > pitch:
            raise ValueError("frames beyond the rows of the last run")

        class _Rows:  # the rows as one strided array, the way any CUDA-array consumer reads it
            __cuda_array_interface__ = {"shape": (self.n, int(frames), ch), "typestr": "<f4" if f32 else "<i2",
                                        "data": (int(ptr), False), "strides": (pitch, ch * size, size), "version": 3}

        return torch.as_tensor(_Rows(), device="cuda")

    def close(self):
        if getattr(self, "_b", None):
            for ref in getattr(self, "_meters", []):  # (a spectrum meter or an encoder goes before its batch)
                m = ref()
                if m is not None:
                    m.close()
            self._L.sauAmd_destroy_Batch(self._b)
            self._b = None

    def __del__(self):
        self.close()


class Spectrum:
    """sauAmdSpectrum: Welch power spectra of float32 rows, summed on the device in f64 (include/saugns_amd.h, section
    "Spectrum"). A meter that is fed rows: ``feed`` takes row r's next frames[r] frames from device memory, on the batch's stream;
    ``read`` waits and returns the sums and the segment counts. Close it before its batch."""

    def __init__(self, batch, n_rows, channels, log2n, hop):
        self._L = batch._L
        self.n_rows, self.channels, self.log2n, self.hop = int(n_rows), int(channels), int(log2n), int(hop)
        self._s = _used(self._L).sauAmd_Batch_create_spectrum(batch._b, self.n_rows, self.channels, self.log2n, self.hop)
        if not self._s:
            raise RuntimeError("sauAmd_Batch_create_spectrum returned NULL: " + last_error(self._L))
        self._batch = batch  # (the batch outlives the meter: its close() closes this one first)
        batch._meters = getattr(batch, "_meters", []) + [weakref.ref(self)]
        self.bins = (1 << self.log2n) // 2 + 1

    def feed(self, ptr, pitch, frames):
        """sauAmd_Spectrum_feed: row r's next frames[r] frames from the device rows at `ptr`, `pitch` bytes apart."""
        fr = (C.c_uint32 * self.n_rows)(*[int(f) for f in frames])
        if not _used(self._L).sauAmd_Spectrum_feed(self._s, ptr, pitch, fr):
            raise RuntimeError("sauAmd_Spectrum_feed failed: " + last_error(self._L))

    def read(self, reset=False):
        """sauAmd_Spectrum_read -> (float64 sums [n_rows, channels, N/2+1], the segments per row as a list)"""
        power = np.zeros((self.n_rows, self.channels, self.bins), np.float64)
        segs = (C.c_uint64 * self.n_rows)()
        if not _used(self._L).sauAmd_Spectrum_read(self._s, power.ctypes.data_as(C.POINTER(C.c_double)), segs, 1 if reset else 0):
            raise RuntimeError("sauAmd_Spectrum_read failed: " + last_error(self._L))
        return power, [int(x) for x in segs]

    def close(self):
        if getattr(self, "_s", None):
            self._L.sauAmd_Spectrum_destroy(self._s)
            self._s = None
            self._batch = None

    def __del__(self):
        self.close()


class Flac:
    """sauAmdFlac: a lossless FLAC encoder of int16 rows on the device (include/saugns_amd.h, section "FLAC"). ``feed`` takes
    row r's next frames[r] frames from device memory, on the batch's stream; ``read`` waits and returns the rows' encoded bytes.
    Close it before its batch."""

    def __init__(self, batch, n_rows, channels, block_frames=0, max_lpc_order=0, lpc_entry=False, bits=None, lpc24=False):
        self._L = batch._L
        self.n_rows, self.channels, self.block_frames = int(n_rows), int(channels), int(block_frames)
        self.max_lpc_order = _lpc_order(max_lpc_order)
        self.bits = None if bits is None else int(bits)  # (None: fed int16 rows; 16 or 24: fed float rows)
        entry = "sauAmd_Batch_create_flac_lpc" if self.max_lpc_order or lpc_entry else "sauAmd_Batch_create_flac"
        if lpc24:  # (bits is 24)
            entry = "sauAmd_Batch_create_flac_lpc24"
            self._e = _used(self._L).sauAmd_Batch_create_flac_lpc24(batch._b, self.n_rows, self.channels, self.block_frames,
                                                                    self.max_lpc_order)
        elif self.bits is not None:
            entry = "sauAmd_Batch_create_flac_f32"
            self._e = _used(self._L).sauAmd_Batch_create_flac_f32(batch._b, self.n_rows, self.channels, self.block_frames,
                                                                  self.bits, self.max_lpc_order)
        elif self.max_lpc_order or lpc_entry:  # (lpc_entry, tests: the _lpc entry point with order 0 too)
            self._e = _used(self._L).sauAmd_Batch_create_flac_lpc(batch._b, self.n_rows, self.channels, self.block_frames,
                                                                  self.max_lpc_order)
        else:
            self._e = _used(self._L).sauAmd_Batch_create_flac(batch._b, self.n_rows, self.channels, self.block_frames)
        if not self._e:
            raise RuntimeError(entry + " returned NULL: " + last_error(self._L))
        self._batch = batch  # (the batch outlives the encoder: its close() closes this one first)
        batch._meters = getattr(batch, "_meters", []) + [weakref.ref(self)]

    def feed(self, ptr, pitch, frames, finish=False):
        """sauAmd_Flac_feed: row r's next frames[r] frames from the device rows at `ptr`, `pitch` bytes apart."""
        fr = (C.c_uint32 * self.n_rows)(*[int(f) for f in frames])
        if not _used(self._L).sauAmd_Flac_feed(self._e, ptr, pitch, fr, 1 if finish else 0):
            raise RuntimeError("sauAmd_Flac_feed failed: " + last_error(self._L))

    def feed_f32(self, ptr, pitch, frames, gains=None, finish=False):
        """sauAmd_Flac_feed_f32: row r's next frames[r] float frames from the device rows at `ptr`, `pitch` bytes apart, times
        gains[r] (None: 1.0)."""
        fr = (C.c_uint32 * self.n_rows)(*[int(f) for f in frames])
        g = None if gains is None else (C.c_float * self.n_rows)(*[float(v) for v in gains])
        if not _used(self._L).sauAmd_Flac_feed_f32(self._e, ptr, pitch, fr, g, 1 if finish else 0):
            raise RuntimeError("sauAmd_Flac_feed_f32 failed: " + last_error(self._L))

    def set_md5(self, on=True):
        """sauAmd_Flac_set_md5: keep the MD5 of every row's unencoded samples; only while every stream stands at its start"""
        if not _used(self._L).sauAmd_Flac_set_md5(self._e, 1 if on else 0):
            raise RuntimeError("sauAmd_Flac_set_md5 failed: " + last_error(self._L))

    def set_verify(self, on=True):
        """sauAmd_Flac_set_verify: decode every frame behind the kernel that wrote it and hold it against the samples; only while
        every stream stands at its start"""
        if not _used(self._L).sauAmd_Flac_set_verify(self._e, 1 if on else 0):
            raise RuntimeError("sauAmd_Flac_set_verify failed: " + last_error(self._L))

    def verify(self):
        """sauAmd_Flac_verify -> the rows' records as dicts (blocks, bad_blocks, first_bad_block, first_status); with verify on"""
        out = (FlacVerify * self.n_rows)()
        if not _used(self._L).sauAmd_Flac_verify(self._e, out):
            raise RuntimeError("sauAmd_Flac_verify failed: " + last_error(self._L))
        return [v.as_dict() for v in out]

    def md5(self):
        """sauAmd_Flac_md5 -> the rows' digests as a list of 16-byte objects; behind a finish, with MD5 on"""
        out = np.full(16 * self.n_rows + 8, 0xa5, np.uint8)
        if not _used(self._L).sauAmd_Flac_md5(self._e, out.ctypes.data):
            assert (out == 0xa5).all(), "a refused md5() has written"
            raise RuntimeError("sauAmd_Flac_md5 failed: " + last_error(self._L))
        assert (out[16 * self.n_rows:] == 0xa5).all(), "a store behind the digests"
        return [bytes(out[16 * r:16 * r + 16]) for r in range(self.n_rows)]

    def unread(self):
        """sauAmd_Flac_read without buffers -> (the unread bytes per row as a list, the rows' FlacInfo as dicts)"""
        n = (C.c_size_t * self.n_rows)()
        info = (FlacInfo * self.n_rows)()
        if not _used(self._L).sauAmd_Flac_read(self._e, None, None, n, info, 0):
            raise RuntimeError("sauAmd_Flac_read failed: " + last_error(self._L))
        return [int(v) for v in n], [i.as_dict() for i in info]

    def read(self, reset=False, caps=None):
        """sauAmd_Flac_read -> (the rows' unread bytes as a list of bytes objects, the rows' FlacInfo as dicts); the bytes
        are consumed. ``caps`` (tests): the capacities to state instead of what the rows need."""
        need, _ = self.unread()
        bufs = [np.full(max(c, 1) + 8, 0xa5, np.uint8) for c in (need if caps is None else caps)]
        ptrs = (C.c_void_p * self.n_rows)(*[b.ctypes.data for b in bufs])
        cap = (C.c_size_t * self.n_rows)(*(need if caps is None else caps))
        n = (C.c_size_t * self.n_rows)()
        info = (FlacInfo * self.n_rows)()
        if not _used(self._L).sauAmd_Flac_read(self._e, ptrs, cap, n, info, 1 if reset else 0):
            assert all((b == 0xa5).all() for b in bufs), "a refused read has written"
            raise RuntimeError("sauAmd_Flac_read failed: " + last_error(self._L))
        for b, v in zip(bufs, n):
            assert (b[int(v):] == 0xa5).all(), "a store behind the row's bytes"
        return [bytes(b[:int(v)]) for b, v in zip(bufs, n)], [i.as_dict() for i in info]

    def close(self):
        if getattr(self, "_e", None):
            self._L.sauAmd_Flac_destroy(self._e)
            self._e = None
            self._batch = None

    def __del__(self):
        self.close()


class Quantizer:
    """sauAmdQuantizer: the 16-bit quantiser stage with TPDF dither and error-feedback noise shaping (include/saugns_amd.h,
    section "Dither and noise shaping"). ``feed`` takes row r's next frames[r] float frames from device memory, on the batch's
    stream, and leaves int16 rows of the stage's own on the device (``rows``, ``pitch``); ``read`` waits and returns the last
    feed's samples. Close it before its batch."""

    def __init__(self, batch, n_rows, channels, spec):
        self._L = batch._L
        self.n_rows, self.channels = int(n_rows), int(channels)
        self._last = [0] * self.n_rows
        self._q = _used(self._L).sauAmd_Batch_create_quantizer(batch._b, self.n_rows, self.channels, C.byref(spec))
        if not self._q:
            raise RuntimeError("sauAmd_Batch_create_quantizer returned NULL: " + last_error(self._L))
        self._batch = batch  # (the batch outlives the quantiser: its close() closes this one first)
        batch._meters = getattr(batch, "_meters", []) + [weakref.ref(self)]

    def feed(self, ptr, pitch, frames, gains=None):
        """sauAmd_Quantizer_feed: row r's next frames[r] float frames from the device rows at `ptr`, `pitch` bytes apart, times
        gains[r] (None: 1.0)."""
        fr = (C.c_uint32 * self.n_rows)(*[int(f) for f in frames])
        g = None if gains is None else (C.c_float * self.n_rows)(*[float(v) for v in gains])
        if not _used(self._L).sauAmd_Quantizer_feed(self._q, ptr, pitch, fr, g):
            raise RuntimeError("sauAmd_Quantizer_feed failed: " + last_error(self._L))
        self._last = [int(f) for f in frames]

    def rows(self):
        """sauAmd_Quantizer_rows: the device address of the output rows (None before the first feed with frames)"""
        return self._L.sauAmd_Quantizer_rows(self._q)

    def pitch(self):
        """sauAmd_Quantizer_pitch: the bytes between the output rows"""
        return int(self._L.sauAmd_Quantizer_pitch(self._q))

    def read(self):
        """sauAmd_Quantizer_read -> the last feed's samples per row, a list of int16 arrays [frames[r] * channels]"""
        bufs = [np.full(n * self.channels + 8, 0x5a5a, np.int16) for n in self._last]
        ptrs = (C.c_void_p * self.n_rows)(*[b.ctypes.data for b in bufs])
        if not _used(self._L).sauAmd_Quantizer_read(self._q, ptrs):
            raise RuntimeError("sauAmd_Quantizer_read failed: " + last_error(self._L))
        for b, n in zip(bufs, self._last):
            assert (b[n * self.channels:] == 0x5a5a).all(), "a store behind the row's frames"
        return [b[:n * self.channels].copy() for b, n in zip(bufs, self._last)]

    def stats(self, reset=False):
        """sauAmd_Quantizer_stats -> the rows' DitherStats as dicts; ``reset`` restarts every stream at frame 0"""
        st = (DitherStats * self.n_rows)()
        if not _used(self._L).sauAmd_Quantizer_stats(self._q, st, 1 if reset else 0):
            raise RuntimeError("sauAmd_Quantizer_stats failed: " + last_error(self._L))
        return [s.as_dict() for s in st]

    def close(self):
        if getattr(self, "_q", None):
            self._L.sauAmd_Quantizer_destroy(self._q)
            self._q = None
            self._batch = None

    def __del__(self):
        self.close()
