"""saugns_amd -- MI355X-native backend for the saugns audio generator hot path.

The product is ``libsaugns_amd.so`` (HIP kernels + C++ host control plane behind
the reference's C API); this package builds it in-tree and binds it with ctypes.
"""
from .api import (Batch, Flac, FlacInfo, Generator, Levels, LimiterStats, Loudness, Program, Spectrum, SNDFILE_AU, SNDFILE_RAW, SNDFILE_WAV,  # noqa: F401
                  decimator_latency, decimator_taps, get_piluts, last_error, lib, limiter_latency, limiter_window,
                  loudness_filter, loudness_gate, render_file, render_file_flac, flac_encode_block, flac_header, flac_encode_block_s32, flac_quantize,
                  flac_md5, set_flac_file_md5, FlacVerify, flac_decode_block, set_flac_file_verify,
                  FLAC_DEC_OK, FLAC_DEC_LENGTH, FLAC_DEC_SYNC, FLAC_DEC_HEADER, FLAC_DEC_NUMBER, FLAC_DEC_CRC8, FLAC_DEC_SUBFRAME, FLAC_DEC_RESIDUAL,
                  FLAC_DEC_PADDING, FLAC_DEC_CRC16, FLAC_DEC_RANGE, FLAC_DEC_MISMATCH, FLAC_DEC_BAD_ARGUMENT, FLAC_DEC_NAMES,
                  render_file_flac_f32, render_file_flac_loudness, flac_encode_block_lpc24, render_file_flac_lpc24, render_file_flac_loudness_lpc24, render_file_loudness, render_file_loudness_limited,
                  render_file_normalized, render_file_oversampled, render_spectrum, set_piluts, spectrum_twiddles, spectrum_window,
                  truepeak_taps,
                  Dither, DitherStats, Quantizer, DITHER_FLAT, DITHER_HP1, DITHER_E3, DITHER_E5, DITHER_F9, dither_preset, dither_quantize,
                  render_file_dithered, render_file_flac_dithered, render_file_loudness_dithered)
from .build import build  # noqa: F401
