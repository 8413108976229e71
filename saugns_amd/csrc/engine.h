/* engine.h -- host control plane of the MI355X generator backend.
 *
 * Mirrors the control flow of sau/generator.c (event timeline, voice
 * durations, end-of-signal detection: generator.c:172-195,348-377,833-973)
 * on the host, flattens every voice's operator graph into a plan
 * (plan.cpp), and drives a Backend that owns the operator state and does the
 * per-sample work.  The product backend is the HIP one (hip_backend.hip);
 * the interface exists so that the host logic can be exercised without a GPU
 * by tests/ (which inject their own sequential executor) -- the library
 * itself never falls back to a CPU path.
 */
#ifndef SAU_ENGINE_H
#define SAU_ENGINE_H

#include "../../include/sau_abi.h"
#include "sau_dev_types.h"
#include "sau_flac.h"
#include "sau_dither.h"
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string>
#include <unordered_map>
#include <vector>

namespace sauengine {

using namespace saudev;

/* What a run stores per sample: the reference's int16 (clamped to +-1, rounded to 15 bits: pcm16 in sau_dev_math.h), or the
 * mixer's f32 sum as it stands (include/saugns_amd.h: sauAmd_Batch_run_f32). The format belongs to the run, not to the engine. */
enum SampleFormat : uint8_t { SF_S16 = 0, SF_F32 = 1 };

/* What a level meter reports of one stream or row (include/saugns_amd.h: sauAmdLevels, the same 80 bytes). */
struct Levels {
	uint64_t frames;
	float peak[2];
	double sum_sq[2];
	uint64_t over[2], full_scale[2], nonfinite[2];
};
static_assert(sizeof(Levels) == 80, "sauAmdLevels");

/* What the loudness meter reports of one stream or row (include/saugns_amd.h: sauAmdLoudness, the same 48 bytes). */
struct Loudness {
	uint64_t frames, blocks, gated_blocks;
	double integrated, momentary_max;
	float true_peak[2];
};
static_assert(sizeof(Loudness) == 48, "sauAmdLoudness");
/* Loudness on the host (tables.cpp; include/saugns_amd.h states the arithmetic). loudness_filter: the ten K-weighting
 * coefficients for a rate (false below LOUD_MIN_RATE); loudness_chunk_map: the state's 4x4 map M over `chunk` frames of zero
 * input, row-major; loudness_step: one frame of the recurrence on st[4] -> y; truepeak_taps: as decimator_taps, 129 taps g;
 * loudness_gate: BS.1770 gating of complete hops [n][2] into out (frames = n_hops * hop_frames, true_peak 0);
 * truepeak_tail: the positions that lag behind a row's last frame -- hist holds the row's last TP_HIST + 1 = 32 frames
 * (cleaned, interleaved) and is followed by 31 zero frames -- folded into peak_bits[channels]. */
constexpr uint32_t LOUD_MIN_RATE = 2560;
constexpr size_t TP_TAPS = 129, TP_LEAD = 32;
bool loudness_filter(uint32_t srate, double out[10]);
void loudness_chunk_map(const double f[10], uint32_t chunk, double m[16]);
double loudness_step(double st[4], const double f[10], double x);
size_t truepeak_taps(double *out, size_t cap);
bool loudness_gate(const double *hops, size_t n_hops, uint32_t hop_frames, int channels, Loudness *out);
void truepeak_tail(const float *hist, int channels, const double *taps, uint32_t *peak_bits);

/* The decimator's filter (tables.cpp; include/saugns_amd.h: sauAmd_decimator_taps). Factors 2, 4 and 8; half-length
 * DECIM_HALF output frames, which is also the filter's latency; L = 2 * DECIM_HALF * factor + 1 taps in f64.
 * decimator_taps returns L and writes the taps when cap >= L (nothing otherwise); both return 0 for another factor. */
constexpr size_t DECIM_HALF = 32;
size_t decimator_taps(int factor, double *out, size_t cap);
size_t decimator_latency(int factor);

/* The limiter on the host (tables.cpp; include/saugns_amd.h, section "Limiter"). limiter_lookahead: A = min(max(srate / 200,
 * 16), 1024) frames (0 for srate == 0); limiter_latency: D = 2 A + 16 (0 likewise); limiter_window: 2 A + 1, and the smoothing
 * window h in out[] when cap suffices (nothing otherwise), shaped like decimator_taps. LimiterStats is sauAmdLimiterStats. */
constexpr uint32_t LIM_A_MIN = 16, LIM_A_MAX = 1024;
struct LimiterStats {
	uint64_t frames, limited;
	double min_gain;
};
static_assert(sizeof(LimiterStats) == 24, "sauAmdLimiterStats");
size_t limiter_lookahead(uint32_t srate);
size_t limiter_latency(uint32_t srate);
size_t limiter_window(uint32_t srate, double *out, size_t cap);
/* pre_gain and ceiling: finite and > 0 (a NaN fails every comparison) */
inline bool limiter_param_ok(float v) { return v > 0.f && v <= 3.402823466e+38f; }

/* The spectrum meter on the host (tables.cpp; include/saugns_amd.h, section "Spectrum"). N = 2^log2n, log2n in SPEC_L_MIN ..
 * SPEC_L_MAX; N / 8 <= hop <= N; segments are summed in groups of SPEC_GROUP. spectrum_window: N, and the periodic Hann window
 * in out[] when cap suffices (nothing otherwise); spectrum_twiddles: N doubles, the N / 2 pairs (cos, -sin); both 0 for another
 * log2n. spectrum_segment: one segment of one channel, x[j * stride] for j = 0 .. N-1, through re[N] and im[N] into p[N/2 + 1]. */
constexpr uint32_t SPEC_L_MIN = 8, SPEC_L_MAX = 12, SPEC_GROUP = 16;
size_t spectrum_window(unsigned log2n, double *out, size_t cap);
size_t spectrum_twiddles(unsigned log2n, double *out, size_t cap);
bool spectrum_segment(unsigned log2n, const double *w, const double *tw, const float *x, size_t stride, double *re, double *im,
		double *p);
inline bool spectrum_params_ok(int channels, unsigned log2n, uint32_t hop) {
	return (channels == 1 || channels == 2) && log2n >= SPEC_L_MIN && log2n <= SPEC_L_MAX && hop >= (1u << log2n) / 8 && hop <= (1u << log2n);
}
/* S(P): the complete segments of P frames */
inline uint64_t spectrum_segments(uint64_t frames, uint32_t N, uint32_t hop) { return frames < N ? 0 : (frames - N) / hop + 1; }

/* A spectrum meter of a backend (Backend::create_spectrum): records that are fed rows. Destroyed before its backend. */
class SpectrumMeter {
public:
	virtual ~SpectrumMeter() {}
	virtual size_t n_rows() const = 0;
	virtual uint32_t channels() const = 0;
	virtual uint32_t log2n() const = 0;
	/* row r's next frames[r] frames, from rows + pitch_bytes * r: device work on the backend's stream */
	virtual bool feed(const void *rows, size_t pitch_bytes, const uint32_t *frames, std::string &err) = 0;
	/* wait for the stream; power_out[n_rows][channels][N/2 + 1] the sums (the group at hand added in the copy), segments_out[n_rows];
	 * `reset`: empty records behind the read */
	virtual bool read(double *power_out, uint64_t *segments_out, bool reset, std::string &err) = 0;
};

/* The FLAC encoder on the host (tables.cpp; include/saugns_amd.h, section "FLAC"; the arithmetic is sau_flac.h's, which the
 * kernels use too). FlacInfo is sauAmdFlacInfo. flac_header: 42, and "fLaC", the metadata block header and STREAMINFO in out[]
 * when cap suffices; 0 on a bad argument. flac_encode_block: one frame of n interleaved frames as the device makes it -> its
 * size, written when cap suffices; 0 on a bad argument. */
struct FlacInfo {
	uint64_t frames, blocks, bytes;
	uint32_t min_frame_bytes, max_frame_bytes;
};
static_assert(sizeof(FlacInfo) == 32, "FlacInfo is sauAmdFlacInfo");
size_t flac_header(uint32_t srate, int channels, uint32_t block_frames, const FlacInfo *info, uint8_t *out, size_t cap);
size_t flac_encode_block(const int16_t *x, uint32_t n, int channels, uint32_t block_frames, uint32_t frame_number, uint8_t *out, size_t cap);
/* ... with the LPC mode's max_lpc_order (0 .. 8; 0: flac_encode_block) */
size_t flac_encode_block_lpc(const int16_t *x, uint32_t n, int channels, uint32_t block_frames, uint32_t frame_number, uint32_t max_lpc_order,
		uint8_t *out, size_t cap);
/* 24 bits and float-fed encoders (the header's "24 bits"). flac_header_bits: flac_header with STREAMINFO's bits per sample, 16 or
 * 24. flac_encode_block_s32: one frame of int32 samples -- bits 16: every sample fits int16, the bytes of flac_encode_block_lpc;
 * bits 24: every sample in -2^23 .. 2^23 - 1 and max_lpc_order 0 -- else 0. flac_quantize: what flac_quant_kernel makes,
 * pcm16(x * gain) or pcm24(x * gain); false for other bits. */
size_t flac_header_bits(uint32_t srate, int channels, uint32_t block_frames, int bits, const FlacInfo *info, uint8_t *out, size_t cap);
size_t flac_encode_block_s32(const int32_t *x, uint32_t n, int channels, uint32_t block_frames, uint32_t frame_number, int bits,
		uint32_t max_lpc_order, uint8_t *out, size_t cap);
bool flac_quantize(const float *x, size_t n, float gain, int bits, int32_t *out);
/* LPC at 24 bits (the header's paragraph of that name): one frame of int32 samples in -2^23 .. 2^23 - 1 with the LPC mode's
 * max_lpc_order (0 .. 8; 0: flac_encode_block_s32's bytes at 24 bits) -- else 0. */
size_t flac_encode_block_lpc24(const int32_t *x, uint32_t n, int channels, uint32_t block_frames, uint32_t frame_number, uint32_t max_lpc_order,
		uint8_t *out, size_t cap);
/* MD5 (the header's "MD5"; the arithmetic is sau_md5.h's). flac_header_md5: flac_header_bits with STREAMINFO's MD5 field, bytes
 * 26 .. 41, taken from md5 (NULL: zeros). flac_md5: the digest of n interleaved samples of `bits` (16 or 24) per sample as the
 * device makes it; false for other bits, a sample that does not fit them or a NULL pointer with n > 0. */
size_t flac_header_md5(uint32_t srate, int channels, uint32_t block_frames, int bits, const FlacInfo *info, const uint8_t md5[16],
		uint8_t *out, size_t cap);
bool flac_md5(const int32_t *x, size_t n, int bits, uint8_t out[16]);
/* The decoder (the header's "Verify"; the arithmetic is sau_flac_dec.h's, which flac_decode_kernel uses too): the one frame that
 * begins at data, of the encoders' own making -> its size with *status_out == FLAC_DEC_OK, *n_out its frames and
 * out[n * channels] its samples; otherwise 0 with the status (sauflac::FlacDecStatus; FLAC_DEC_BAD_ARGUMENT for a bad argument
 * or cap_frames < n). data[len] and beyond are never read. */
size_t flac_decode_block(const uint8_t *data, size_t len, int channels, uint32_t block_frames, int bits, uint32_t frame_number, int32_t *out,
		size_t cap_frames, uint32_t *n_out, int *status_out);
/* What a verifying encoder keeps per row (FlacEncoder::verify): sauAmdFlacVerify. */
struct FlacVerify {
	uint64_t blocks, bad_blocks, first_bad_block;
	uint32_t first_status, pad_;
};
static_assert(sizeof(FlacVerify) == 32, "FlacVerify is sauAmdFlacVerify");
inline bool flac_params_ok(int channels, uint32_t block_frames) {
	return (channels == 1 || channels == 2) && sauflac::flac_block_frames(block_frames) != 0;
}

/* A FLAC encoder of a backend (Backend::create_flac): streams that are fed int16 rows. Destroyed before its backend. */
class FlacEncoder {
public:
	virtual ~FlacEncoder() {}
	virtual size_t n_rows() const = 0;
	virtual uint32_t channels() const = 0;
	virtual uint32_t block_frames() const = 0;
	/* row r's next frames[r] frames, from rows + pitch_bytes * r: device work on the backend's stream; `finish` closes the rows */
	virtual bool feed(const void *rows, size_t pitch_bytes, const uint32_t *frames, bool finish, std::string &err) = 0;
	/* a float-fed encoder (Backend::create_flac_f32): row r's next frames[r] float frames times gains[r] (NULL: 1.0f), quantised
	 * into rows of the encoder's own and fed from there. An encoder is of one kind: the other kind's feed is a bad argument. */
	virtual bool feed_f32(const void *rows, size_t pitch_bytes, const uint32_t *frames, const float *gains, bool finish, std::string &err) {
		(void)rows; (void)pitch_bytes; (void)frames; (void)gains; (void)finish; err = "bad argument: this encoder is fed int16 rows"; return false;
	}
	virtual uint32_t bits() const { return 16; }
	/* wait for the stream; bytes_out[n_rows] the unread bytes; bufs (may be NULL): they are copied there and consumed, every
	 * caps[r] has to suffice; info_out (may be NULL) [n_rows]; `reset`: new streams behind the read */
	virtual bool read(uint8_t *const *bufs, const size_t *caps, size_t *bytes_out, FlacInfo *info_out, bool reset, std::string &err) = 0;
	/* the MD5 of the unencoded samples (the header's "MD5"), off until asked for. set_md5: only while every stream stands at its
	 * start -- nothing fed since creation or since the last read with reset --, else a bad argument; the setting outlives resets.
	 * md5: waits for the stream; out[n_rows][16] the digests when MD5 is on and a finish has closed the rows, else false with a
	 * bad argument and nothing written. */
	virtual bool set_md5(bool on, std::string &err) { (void)on; err = "bad argument: this backend's FLAC encoder has no MD5"; return false; }
	virtual bool md5(uint8_t *out, std::string &err) { (void)out; err = "bad argument: this backend's FLAC encoder has no MD5"; return false; }
	/* the verify mode (the header's "Verify"), off until asked for. set_verify: set_md5's rules. verify: waits for the stream;
	 * out[n_rows] the rows' records since the last reset; false with a bad argument when verify is off. */
	virtual bool set_verify(bool on, std::string &err) { (void)on; err = "bad argument: this backend's FLAC encoder has no verify mode"; return false; }
	virtual bool verify(FlacVerify *out, std::string &err) { (void)out; err = "bad argument: this backend's FLAC encoder has no verify mode"; return false; }
};

/* The 16-bit quantiser on the host (tables.cpp; include/saugns_amd.h, section "Dither and noise shaping"; the arithmetic is
 * sau_dither.h's, which the kernels use too). DitherStats is sauAmdDitherStats. dither_quantize: row `row`'s frames
 * [first_frame, first_frame + frames) as a quantiser makes them; history (may be NULL: zeros) [channels][9] in and out, left
 * alone by a spec without taps; clipped (may be NULL) [2] is set to this call's counts. False on a bad spec, channels other
 * than 1 or 2, a gain that is not finite or a NULL pointer with frames > 0. */
struct DitherStats {
	uint64_t frames;
	uint64_t clipped[2];
};
static_assert(sizeof(DitherStats) == 24, "DitherStats is sauAmdDitherStats");
bool dither_quantize(const float *x, size_t frames, int channels, float gain, const saudither::DitherSpec *spec, uint64_t row,
		uint64_t first_frame, double *history, int16_t *out, uint64_t *clipped);

/* A quantiser of a backend (Backend::create_quantizer): streams that are fed float rows and leave int16 rows of the stage's
 * own on the device. Destroyed before its backend. */
class Quantizer {
public:
	virtual ~Quantizer() {}
	virtual size_t n_rows() const = 0;
	virtual uint32_t channels() const = 0;
	/* row r's next frames[r] float frames times gains[r] (NULL: 1.0f), from rows + pitch_bytes * r: device work on the backend's
	 * stream, into the first frames[r] frames of the stage's row r */
	virtual bool feed(const void *rows, size_t pitch_bytes, const uint32_t *frames, const float *gains, std::string &err) = 0;
	/* the output rows: device address (16-byte aligned, one allocation) and pitch in bytes (a multiple of 256), valid until the
	 * next feed; NULL and 0 before the first feed with frames */
	virtual const int16_t *rows() const = 0;
	virtual size_t pitch() const = 0;
	/* wait for the stream, then the last feed's frames per row to bufs[r] (may be NULL where the row had none) */
	virtual bool read(int16_t *const *bufs, std::string &err) = 0;
	/* queue the copy of the first `bytes` bytes of row 0 out, like Backend::fetch_pcm_async (`slot`, wait_fetch): the file writers */
	virtual bool fetch_async(void *dst, size_t bytes, int slot, std::string &err) = 0;
	/* wait for the stream; out (may be NULL) [n_rows]; `reset`: every stream starts again at frame 0 with zero history */
	virtual bool stats(DitherStats *out, bool reset, std::string &err) = 0;
};

/* Everything the backend needs to render one segment (no events inside). */
struct SegmentDesc {
	uint32_t len;             /* frames */
	uint32_t pcm_offset;      /* frame offset into each stream's PCM row */
	bool stereo;
	bool swap_bytes;          /* store PCM big-endian (AU files, player/sndfile.c:160-168) */
	SampleFormat format = SF_S16; /* of the run the segment belongs to (Backend::set_format has announced it) */
	/* active voices of all streams, ascending (stream, voice id) */
	const VoiceDesc *voices;
	uint32_t n_voices;
	/* per stream: range of `voices`, amp_scale, frames to write (last_len) */
	struct Stream {
		uint32_t first_voice, n_voices;
		float amp_scale;
		uint32_t write_len;
	};
	const Stream *streams;
	uint32_t n_streams;
	uint32_t n_slots;         /* max over active plans of main + frequency slots */
	uint32_t n_main;          /* max main-pool slots (slot_index() base) */
	uint32_t n_fast;          /* max block buffers the time-parallel path needs (fast_slot_compact) */
	uint32_t n_fast_full;     /* the same with frequency blocks, over voices that may need them */
	bool may_scan;            /* some voice may have ramped or modulated frequencies (running-sum phases) */
	uint32_t sum_levels = 2; /* running sums nested that deep may occur (host estimate; the device checks) */
	uint32_t max_ops;         /* max operators in any active voice */
	uint32_t max_steps;       /* longest active plan */
	uint32_t n_pan_rows;
	uint64_t wave_mask;       /* wave ids in use (bit per id) */
	bool maybe_block;         /* some voice may need the block loop (sweeps, FM, ...) */
	bool serial;              /* some voice may run a per-sample feedback recurrence (self-modulation) */
	bool maybe_cub = false;   /* some voice has an R operator with `cub` segments and the loop tails are on (the builds with that code are launched) */
	uint32_t n_chain_rows = 0;/* row pairs the voices' chain_base/n_chain span */
	uint32_t n_inc_rows = 0;  /* row pairs the voices' inc_base/n_inc span (voices that may have running-sum phases) */
	uint32_t n_look_rows = 0; /* rows the voices' look_base/n_look span (those of them without feedback chains) */
	uint32_t n_may_scan = 0;  /* voices that may have running-sum phases this segment (the device decides: analyze_kernel) */
	uint32_t n_chain_slots = 0; /* lanes of the chain kernels' waves the voices' chain_slot/n_chain span (>= n_chain_rows) */
	bool chain_rows_padded = false; /* some of the n_chain_slots lanes belong to no voice (kinds of R feedback chains begin waves of their own) */
	/* every active voice's steps are W oscillators with one amplitude value each: no amplitude modulators, no sweep ever given to
	 * an operator, nothing layered, no R, N or A operator, no line step, no operator that runs out inside the segment.
	 * Conservative (false wherever the host cannot be sure): the lane-major inner launch's wave-only instantiation */
	bool wave_only = false;
};

/* Bytes a backend has for the rows of a segment's feedback chains (8 B per chain and frame; the engine cuts segments with
 * feedback voices accordingly, never below CHAIN_SEG frames). free_bytes: what was free on the backend's device when the
 * process first opened it (0: not told -- the sequential executor of the tests); alloc_failures: allocations of rows that
 * failed on this backend. SAU_AMD_CHAIN_ROWS_MB sets the budget; without it: 24 GiB (288 GB of HBM hold BASELINE config 5's
 * 4096 chains x 441000 frames, 14.4 GB, as one segment -- one fill and one drain of the pass / chain pipeline),
 * or an eighth of free_bytes where that is less; every failed allocation halves it (the backend renders the segment that did
 * not fit in the block loop). Per backend since round 6 (Backend::chain_rows_budget): the hint used to be the first device's
 * of the process and the failures every engine's -- one full GPU of eight cut every other GPU's segments short (ADVICE r04,
 * VERDICT r05). (inline: the test executor's library has the interface without engine.cpp) */
inline size_t chain_rows_budget(size_t free_b, unsigned fails) {
	static const long long env_mb = [] {
		const char *v = getenv("SAU_AMD_CHAIN_ROWS_MB");
		return v ? atoll(v) : -1ll;
	}();
	const unsigned sh = fails > 40 ? 40 : fails; /* (after a few failures: segments with feedback voices are CHAIN_SEG frames) */
	if (env_mb >= 0) return ((size_t)env_mb << 20) >> sh;
	const size_t dflt = (size_t)24 << 30; /* of an MI355X's 288 GB */
	if (!free_b) return dflt >> sh;
	return (free_b / 8 < dflt ? free_b / 8 : dflt) >> sh;
}

struct BackendConfig {
	uint32_t srate;
	uint32_t op_count;        /* all streams */
	uint32_t voice_count;     /* all streams */
	uint32_t n_streams;
	uint32_t max_frames;      /* PCM row capacity, frames */
	const float *piluts;      /* 12 x 2048 */
	const WaveConst *wconst;  /* 12 */
};


class Backend {
public:
	virtual ~Backend() {}
	virtual bool init(const BackendConfig &cfg, std::string &err) = 0;
	/* grow PCM / voice matrices when a caller passes a longer buffer */
	virtual bool reserve_frames(uint32_t max_frames, bool stereo, std::string &err) = 0;
	/* plans changed: full step array + op id lists; fast_ids holds 2 * n_steps entries:
	 * the numbering without frequency blocks, then the one with them */
	virtual bool upload_plans(const Step *steps, const FastIds *fast_ids, size_t n_steps,
			const uint32_t *op_ids, size_t n_ids, std::string &err) = 0;
	/* apply operator updates in order; ops are distinct within one call */
	virtual bool apply_updates(const OpUpdate *recs, size_t n, std::string &err) = 0;
	/* zero the frames [first_frame, first_frame + n_frames) of the PCM rows of streams [first_stream, first_stream + n_streams):
	 * what a run's mixers do not write (generator.c:911-914 clears the whole buffer ahead of every call; here only the frames
	 * behind a stream's last voice and the segments nothing sounds in are cleared, ordered with the rendering like any device work) */
	virtual bool zero_pcm(uint32_t first_stream, uint32_t n_streams, uint32_t first_frame, uint32_t n_frames, bool stereo,
			std::string &err) = 0;
	/* tests (SAU_AMD_POISON): a run of `frames` frames is about to start -- fill the streams' whole PCM rows with a pattern
	 * no mixer writes (0x5a5a), so that a frame that is neither mixed nor cleared by zero_pcm shows in the PCM instead of the
	 * previous run's, usually correct, data. Called after any reserve_frames and before the run's first segment. */
	virtual bool poison_run(uint32_t frames, bool stereo, std::string &err) { (void)frames; (void)stereo; (void)err; return true; }
	virtual bool render(const SegmentDesc &seg, std::string &err) = 0;
	/* copy stream `s` PCM [0, frames) to host memory (blocks until done) */
	virtual bool fetch_pcm(uint32_t stream, int16_t *dst, uint32_t frames,
			bool stereo, std::string &err) = 0;
	/* device address of stream s PCM row, or NULL (test backends) */
	virtual const int16_t *device_pcm(uint32_t stream) = 0;
	virtual bool sync(std::string &err) = 0;
	/* Output stage: queue a copy of stream s PCM [0, frames) into host memory from
	 * alloc_host(); `slot` (0..3) names the copy for wait_fetch(). Later device
	 * work is ordered behind the copy. Defaults suit CPU test backends. */
	virtual bool fetch_pcm_async(uint32_t stream, int16_t *dst, uint32_t frames, bool stereo,
			int slot, std::string &err) { (void)slot; return fetch_pcm(stream, dst, frames, stereo, err); }
	virtual bool wait_fetch(int slot, std::string &err) { (void)slot; (void)err; return true; }
	virtual void *alloc_host(size_t bytes) { return malloc(bytes); }
	virtual void free_host(void *p) { free(p); }
	/* Operator state kept / brought back (Engine::snapshot / restore: the drop-in generator's read-ahead rewinds when
	 * its host changes the size or the channel layout of its calls). `slot` (0..3) names the copy; both are ordered
	 * with the rendering like any other device work. */
	virtual bool save_state(int slot, std::string &err) { (void)slot; err = "this backend keeps no state snapshots"; return false; }
	virtual bool load_state(int slot, std::string &err) { (void)slot; err = "this backend keeps no state snapshots"; return false; }
	/* bytes this backend has for the feedback chains' rows of one segment (engine.h: chain_rows_budget; the engine cuts segments
	 * with such voices accordingly) */
	virtual size_t chain_rows_budget() { return sauengine::chain_rows_budget(0, 0); }
	/* Float32 sample output. A run of another format than the last one is announced here, ahead of everything else of the
	 * run (reserve_frames, poison_run, zero_pcm, render and the fetches then go by it); a backend without float output
	 * refuses -- these defaults -- and the engine then renders nothing and stands where it stood. */
	virtual bool set_format(SampleFormat fmt, std::string &err) {
		if (fmt == SF_S16) return true;
		err = "this backend has no float32 sample output";
		return false;
	}
	/* fetch_pcm / fetch_pcm_async after a float run */
	virtual bool fetch_pcm_f32(uint32_t stream, float *dst, uint32_t frames, bool stereo, std::string &err) {
		(void)stream; (void)dst; (void)frames; (void)stereo; err = "this backend has no float32 sample output"; return false;
	}
	virtual bool fetch_pcm_f32_async(uint32_t stream, float *dst, uint32_t frames, bool stereo, int slot, std::string &err) {
		(void)stream; (void)dst; (void)frames; (void)stereo; (void)slot; err = "this backend has no float32 sample output"; return false;
	}
	/* device address of stream s float row when the last run was a float run, else NULL (device_pcm: NULL after a float run) */
	virtual const float *device_pcm_f32(uint32_t stream) { (void)stream; return nullptr; }
	/* bytes between the rows of consecutive streams in the last run's format (0: no device PCM) */
	virtual size_t device_pcm_pitch() { return 0; }
	/* Level metering (include/saugns_amd.h: sauAmdLevels), where the samples are. A backend without it refuses -- these
	 * defaults, as with float output -- and nothing changes. begin_metering: make the streams' records (zeroed) if they are
	 * not there yet. */
	virtual bool begin_metering(std::string &err) { err = "this backend has no level metering"; return false; }
	/* measure frames [0, frames[s]) of every stream's row of the run just rendered (its format, its channels) and add the
	 * result to the stream's record: device work on the backend's stream, behind the run's mixers and ahead of any fetch */
	virtual bool measure_streams(const uint32_t *frames, bool stereo, SampleFormat format, std::string &err) {
		(void)frames; (void)stereo; (void)format; err = "this backend has no level metering"; return false;
	}
	/* wait for the stream and copy the records out; `reset`: clear them */
	virtual bool read_levels(Levels *out, bool reset, std::string &err) {
		(void)out; (void)reset; err = "this backend has no level metering"; return false;
	}
	/* the same measurement of rows the caller holds on the backend's device (synchronous; the streams' records are untouched) */
	virtual bool measure_rows(const void *rows, size_t pitch_bytes, size_t n_rows, SampleFormat format, size_t frames,
			bool stereo, Levels *out, std::string &err) {
		(void)rows; (void)pitch_bytes; (void)n_rows; (void)format; (void)frames; (void)stereo; (void)out;
		err = "this backend has no level metering"; return false;
	}
	/* The normalised file writer's second pass: frames [0, frames) of stream s's float row of the run just rendered, times
	 * `gain`, into a device buffer of the backend's own -- as int16 (pcm16 of the product; `swap_bytes`: big-endian) or as
	 * float32 -- and fetch_requant_async queues the copy of that buffer out, like fetch_pcm_async (`slot`, wait_fetch). */
	virtual bool requantize(uint32_t stream, uint32_t frames, bool stereo, float gain, SampleFormat out, bool swap_bytes, std::string &err) {
		(void)stream; (void)frames; (void)stereo; (void)gain; (void)out; (void)swap_bytes; err = "this backend has no level metering"; return false;
	}
	virtual bool fetch_requant_async(void *dst, size_t bytes, int slot, std::string &err) {
		(void)dst; (void)bytes; (void)slot; err = "this backend has no level metering"; return false;
	}
	/* Decimation of float runs rendered at `factor` times the wanted rate (include/saugns_amd.h: sauAmd_Batch_run_decimated_f32),
	 * where the samples are. A backend without it refuses -- these defaults -- and nothing changes. begin_decimation: a
	 * sequence of decimated runs with this factor and channel layout starts: every stream's history is zero. */
	virtual bool begin_decimation(int factor, bool stereo, std::string &err) {
		(void)factor; (void)stereo; err = "this backend has no decimator"; return false;
	}
	/* buf_len output frames of every stream from the float run just rendered (buf_len * factor frames, of which the first
	 * frames_hi[s] are stream s's; the rest, whatever the rows hold there, count as +0) and the stream's history, into device
	 * rows of the backend's own -- float32, or int16 (pcm16 of the sum; `swap_bytes`: big-endian) -- and the history moves on:
	 * device work on the backend's stream, behind the run's mixers. frames_hi all 0: the rows are not read. */
	virtual bool decimate(const uint32_t *frames_hi, uint32_t buf_len, int factor, bool stereo, SampleFormat out_fmt, bool swap_bytes,
			std::string &err) {
		(void)frames_hi; (void)buf_len; (void)factor; (void)stereo; (void)out_fmt; (void)swap_bytes;
		err = "this backend has no decimator"; return false;
	}
	/* queue the copy of the first `bytes` bytes of stream s's decimated row out, like fetch_pcm_async (`slot`, wait_fetch);
	 * into memory that is not from alloc_host() the copy has finished on return */
	virtual bool fetch_decimated_async(uint32_t stream, void *dst, size_t bytes, int slot, std::string &err) {
		(void)stream; (void)dst; (void)bytes; (void)slot; err = "this backend has no decimator"; return false;
	}
	/* device address of stream s's decimated float row of the last decimated run (NULL: none, or int16 rows), and the bytes
	 * between the rows of consecutive streams (a multiple of 256; 0: none) */
	virtual const float *device_decimated_f32(uint32_t stream) { (void)stream; return nullptr; }
	virtual size_t device_decimated_pitch() { return 0; }
	/* BS.1770 loudness and true peak of float runs (include/saugns_amd.h: sauAmdLoudness), where the samples are. A backend
	 * without it refuses -- these defaults -- and nothing changes. begin_loudness: make the streams' records (empty) for the
	 * backend's rate if they are not there yet. */
	virtual bool begin_loudness(std::string &err) { err = "this backend has no loudness metering"; return false; }
	/* measure frames [0, frames[s]) of every stream's float row of the run just rendered and take them into the stream's
	 * record -- hop energies, filter state, true peak, history, frame count: device work on the backend's stream, behind the
	 * run's mixers and ahead of any fetch */
	virtual bool measure_loudness(const uint32_t *frames, bool stereo, std::string &err) {
		(void)frames; (void)stereo; err = "this backend has no loudness metering"; return false;
	}
	/* wait for the stream, fetch hops, peaks and histories, gate, cover the true-peak tail in the copy; `reset`: empty records */
	virtual bool read_loudness(Loudness *out, bool reset, std::string &err) {
		(void)out; (void)reset; err = "this backend has no loudness metering"; return false;
	}
	/* *n_hops = the stream's complete hops; their energies [h][2] into out when cap (in hops) suffices */
	virtual bool read_loudness_hops(uint32_t stream, double *out, size_t cap, size_t *n_hops, std::string &err) {
		(void)stream; (void)out; (void)cap; (void)n_hops; err = "this backend has no loudness metering"; return false;
	}
	/* the same measurement, from zero state, of float rows the caller holds on the backend's device (synchronous; the streams'
	 * records are untouched). hops_out, when given and hops_cap (in doubles) suffices: [n_rows][frames / hop][2] */
	virtual bool measure_loudness_rows(const void *rows, size_t pitch_bytes, size_t n_rows, size_t frames, bool stereo, uint32_t srate,
			Loudness *out, double *hops_out, size_t hops_cap, std::string &err) {
		(void)rows; (void)pitch_bytes; (void)n_rows; (void)frames; (void)stereo; (void)srate; (void)out; (void)hops_out; (void)hops_cap;
		err = "this backend has no loudness metering"; return false;
	}
	/* The look-ahead true-peak limiter on float runs (include/saugns_amd.h, section "Limiter"), where the samples are. A backend
	 * without it refuses -- these defaults -- and nothing changes. begin_limiting: a sequence of limited runs with this channel
	 * layout starts at the backend's rate: every stream's history is zero. The statistics are not touched. */
	virtual bool begin_limiting(bool stereo, std::string &err) { (void)stereo; err = "this backend has no limiter"; return false; }
	/* buf_len output frames of every stream -- the sequence delayed by D -- from the float run just rendered (buf_len frames, of
	 * which the first frames[s] are stream s's; the rest, whatever the rows hold there, count as +0) and the stream's history,
	 * into device rows of the backend's own -- float32, or int16 (pcm16 of y; `swap_bytes`: big-endian) -- the history moves on
	 * and the streams' statistics take the run in: device work on the backend's stream, behind the run's mixers. frames all 0:
	 * the rows are not read. */
	virtual bool limit(const uint32_t *frames, uint32_t buf_len, float pre_gain, float ceiling, bool stereo, SampleFormat out_fmt,
			bool swap_bytes, std::string &err) {
		(void)frames; (void)buf_len; (void)pre_gain; (void)ceiling; (void)stereo; (void)out_fmt; (void)swap_bytes;
		err = "this backend has no limiter"; return false;
	}
	/* queue the copy of the first `bytes` bytes of stream s's limited row out, like fetch_decimated_async */
	virtual bool fetch_limited_async(uint32_t stream, void *dst, size_t bytes, int slot, std::string &err) {
		(void)stream; (void)dst; (void)bytes; (void)slot; err = "this backend has no limiter"; return false;
	}
	/* device address of stream s's limited float row of the last limited run (NULL: none, or int16 rows), and the bytes between
	 * the rows of consecutive streams (a multiple of 256; 0: none) */
	virtual const float *device_limited_f32(uint32_t stream) { (void)stream; return nullptr; }
	virtual size_t device_limited_pitch() { return 0; }
	/* wait for the stream and fetch the streams' statistics; `reset`: empty records behind the read */
	virtual bool read_limiter_stats(LimiterStats *out, bool reset, std::string &err) {
		(void)out; (void)reset; err = "this backend has no limiter"; return false;
	}
	/* the limiter from zero history on float rows the caller holds on the backend's device, time-aligned (the delay dropped)
	 * into float rows of the caller's; synchronous, the streams' histories and statistics untouched */
	virtual bool limit_rows(const void *rows, size_t pitch_bytes, size_t n_rows, size_t frames, bool stereo, uint32_t srate,
			float pre_gain, float ceiling, void *out_rows, size_t out_pitch_bytes, LimiterStats *stats_out, std::string &err) {
		(void)rows; (void)pitch_bytes; (void)n_rows; (void)frames; (void)stereo; (void)srate; (void)pre_gain; (void)ceiling;
		(void)out_rows; (void)out_pitch_bytes; (void)stats_out;
		err = "this backend has no limiter"; return false;
	}
	/* Welch power spectra of float rows (include/saugns_amd.h, section "Spectrum"), where the samples are. A backend without
	 * them refuses -- these defaults -- and nothing changes. create_spectrum: a meter of n_rows empty records on the backend's
	 * device and stream (the caller owns it and destroys it before the backend); the arguments have been looked at. */
	virtual SpectrumMeter *create_spectrum(size_t n_rows, uint32_t channels, unsigned log2n, uint32_t hop, std::string &err) {
		(void)n_rows; (void)channels; (void)log2n; (void)hop; err = "this backend has no spectrum meter"; return nullptr;
	}
	/* A FLAC encoder of n_rows streams on the backend's stream (include/saugns_amd.h, section "FLAC"), where the samples are. A
	 * backend without one refuses -- this default -- and nothing changes. */
	virtual FlacEncoder *create_flac(size_t n_rows, uint32_t channels, uint32_t block_frames, std::string &err) {
		(void)n_rows; (void)channels; (void)block_frames; err = "this backend has no FLAC encoder"; return nullptr;
	}
	/* ... with the LPC mode's max_lpc_order (0 .. 8). 0 is create_flac; this default refuses every other value: a backend whose
	 * FLAC encoder predates the LPC mode keeps working as it is. */
	virtual FlacEncoder *create_flac_lpc(size_t n_rows, uint32_t channels, uint32_t block_frames, uint32_t max_lpc_order, std::string &err) {
		if (!max_lpc_order) return create_flac(n_rows, channels, block_frames, err);
		err = "this backend's FLAC encoder has no LPC mode"; return nullptr;
	}
	/* A float-fed encoder of 16 or 24 bits per sample (FlacEncoder::feed_f32); 24 with max_lpc_order 0 only. */
	virtual FlacEncoder *create_flac_f32(size_t n_rows, uint32_t channels, uint32_t block_frames, int bits, uint32_t max_lpc_order, std::string &err) {
		(void)n_rows; (void)channels; (void)block_frames; (void)bits; (void)max_lpc_order;
		err = "this backend has no float-fed FLAC encoder"; return nullptr;
	}
	/* A float-fed encoder of 24 bits per sample with the LPC mode's max_lpc_order (0 .. 8; the header's "LPC at 24 bits"). 0 is
	 * create_flac_f32 at 24 bits; this default refuses every other value, as create_flac_lpc's does. */
	virtual FlacEncoder *create_flac_lpc24(size_t n_rows, uint32_t channels, uint32_t block_frames, uint32_t max_lpc_order, std::string &err) {
		if (!max_lpc_order) return create_flac_f32(n_rows, channels, block_frames, 24, 0, err);
		err = "this backend's FLAC encoder has no LPC mode at 24 bits"; return nullptr;
	}
	/* A quantiser of n_rows streams on the backend's stream (include/saugns_amd.h, section "Dither and noise shaping"); the
	 * arguments have been looked at. A backend without one refuses -- this default -- and nothing changes. */
	virtual Quantizer *create_quantizer(size_t n_rows, uint32_t channels, const saudither::DitherSpec &spec, std::string &err) {
		(void)n_rows; (void)channels; (void)spec; err = "this backend has no quantiser"; return nullptr;
	}
	/* the same from empty records on rows of `frames` frames each, synchronous; spectrogram_out (may be NULL): every segment's
	 * (float)p[k], [n_rows][channels][S][N/2 + 1], refused when spectrogram_cap (in floats) does not suffice */
	virtual bool spectrum_rows(const void *rows, size_t pitch_bytes, size_t n_rows, size_t frames, uint32_t channels, unsigned log2n,
			uint32_t hop, double *power_out, uint64_t *segments_out, float *spectrogram_out, size_t spectrogram_cap, std::string &err) {
		(void)rows; (void)pitch_bytes; (void)n_rows; (void)frames; (void)channels; (void)log2n; (void)hop; (void)power_out;
		(void)segments_out; (void)spectrogram_out; (void)spectrogram_cap;
		err = "this backend has no spectrum meter"; return false;
	}
};

/* ---- plan compiler (plan.cpp) -------------------------------------------- */

struct OpMirror { /* host-side knowledge about one operator */
	bool inited = false;
	uint8_t type = 0;
	uint32_t time = 0;
	bool time_inf = false;
	uint8_t line_set = 0;             /* bit per L_*: line ever given */
	LineState pan;                    /* mirrored exactly (never ratio-scaled) */
	const sauProgramIDArr *mods[SAU_POP_NAMED] = {}; /* by use type; [0] unused */
	uint8_t wave = 0;
	bool ras_cub_seen = false;        /* an R operator that was ever given `cub` segments (conservative: SegmentDesc.maybe_cub) */
	uint32_t ras_kind = 0;            /* an R operator's line shape | function << 8 | flags << 16 as last given (the order feedback chains are dealt to waves in) */
	bool goal_seen = false;           /* some event gave one of its lines a sweep */
	bool freq_goal_seen = false;      /* ... one of its frequency lines */
	bool freq_ratio_seen = false;     /* some event gave one of its frequency lines a ratio (state or goal) */
	OpMirror() { pan = LineState{0, 0, 0, 0, 0, 0}; }
};

struct VoicePlan {
	std::vector<Step> steps;       /* (empty in a voice that uses its shape's: Engine::shapes_) */
	uint32_t n_steps = 0;          /* length of the step list the voice runs */
	std::vector<uint32_t> op_ids;  /* voice-local index -> stream-local op id */
	uint32_t carr_local = 0;
	uint32_t n_slots = 0;          /* memory slots: main pool + frequency pool */
	uint32_t n_main = 0;           /* main-pool slots (ids below FSLOT_BASE) */
	uint32_t n_fast = 0;           /* buffers live at once in the time-parallel path */
	std::vector<FastIds> fast_ids; /* per step: block buffers renumbered by liveness */
	uint32_t n_fast_full = 0;      /* ... counting frequency blocks too (ramps, FM) */
	std::vector<FastIds> fast_ids_full;
	uint64_t wave_mask = 0;
	bool has_camods = false;
	bool no_fast = false;          /* an operator is evaluated twice per block */
	bool wide = false;             /* step pairs with 16-bit buffer ids (sau_dev_types.h: wide plans); no_fast too */
	bool static_block = false;     /* graph has FM / feedback / R / filtered noise: block loop */
	bool selfmod = false;          /* a self-modulation amount has modulators of its own */
	bool ras_cub = false;          /* an R operator that was ever given `cub` segments */
	/* every step evaluates a W oscillator that takes its amplitude from its own line and was never given a sweep, replaces its
	 * output (nothing layered) and reads no amplitude, self-modulation or frequency-scaled PM block, or is that operator's
	 * unforced frequency line (one value on the closed-form path: FM forces it and is a static_block). A function of
	 * what the plan cache's key holds (plan.cpp: voice_plan_shape): types, list uses and counts, the sticky sweep marks */
	bool wave_only = false;
	uint32_t n_chain = 0;          /* oscillator steps that may run a feedback recurrence (step_may_chain) */
	uint32_t n_osc = 0;            /* W and R oscillator steps (their phase increments may be saved between passes) */
};

/* Flatten the graph under `carrier` into steps. Returns false (with err) when
 * the graph exceeds what a workgroup can hold. */
bool compile_voice_plan(const std::vector<OpMirror> &ops, uint32_t carrier,
		VoicePlan &out, std::string &err);
/* the graph's shape as a token stream + its operators in plan order (plan.cpp); false: not cacheable */
bool voice_plan_shape(const std::vector<OpMirror> &ops, uint32_t carrier, std::vector<uint32_t> &tokens,
		std::vector<uint32_t> &op_ids, std::vector<uint32_t> &stamp, uint32_t mark, uint64_t &wave_mask);

/* ---- engine ---------------------------------------------------------------- */

/* Segments with feedback voices are at most this long: the recurrences' inputs and outputs pass
 * through per-chain rows in HBM, sized for one segment. */
constexpr uint32_t CHAIN_SEG = 131072;
/* Environment switches. Product settings are read as they are (INTEGRATION.md has the table: SAU_AMD_DEVICE,
 * SAU_AMD_READAHEAD*, SAU_AMD_LOOP_TAILS, SAU_AMD_CHAIN_ROWS_MB, SAU_AMD_POOL_MB, SAU_AMD_PINNED_POOL_MB, SAU_AMD_DEBUG*);
 * every other SAU_AMD_* name is a tuning or test aid and is looked at only when SAU_AMD_TUNE is set -- a stray variable
 * in a host's environment cannot change how, or on which kernels, a render runs. */
const char *tune_env(const char *name);
uint32_t chain_seg_frames(size_t n_chains, size_t budget_bytes);

class Engine {
public:
	/* programs are borrowed and must outlive the engine (generator.c:191) */
	static Engine *create(const sauProgram *const *prgs, size_t n_prgs,
			uint32_t srate, Backend *backend /* owned */, std::string &err);
	~Engine();

	/* Advance every stream by buf_len frames. host_bufs[s] may be NULL (PCM
	 * stays on the device). more[s]/out_len[s] as sauGenerator_run. */
	bool run(int16_t *const *host_bufs, size_t buf_len, bool stereo,
			bool *more, size_t *out_len, std::string &err) {
		return run((void *const *)host_bufs, SF_S16, buf_len, stereo, more, out_len, err);
	}
	/* The same run with float32 samples (SampleFormat). int16 and float runs may alternate; each continues where the last one
	 * stopped. False, with nothing rendered and no position moved, on a backend without float output. */
	bool run_f32(float *const *host_bufs, size_t buf_len, bool stereo,
			bool *more, size_t *out_len, std::string &err) {
		return run((void *const *)host_bufs, SF_F32, buf_len, stereo, more, out_len, err);
	}
	bool run(void *const *host_bufs, SampleFormat format, size_t buf_len, bool stereo,
			bool *more, size_t *out_len, std::string &err);
	/* Announce the next run's format to the backend now (run() does it itself; the file writer asks before it opens a file). */
	bool set_format(SampleFormat format, std::string &err) {
		if (format != format_ && !backend_->set_format(format, err)) return false;
		format_ = format;
		return true;
	}

	/* A float run of buf_len * factor frames, decimated on the device to buf_len frames per stream (include/saugns_amd.h:
	 * sauAmd_Batch_run_decimated_f32; the engine was created at the output rate times `factor`). The decimated rows stay on
	 * the device (Backend::device_decimated_f32, fetch_decimated_async) -- float32, or with out_fmt SF_S16 the kernels' own
	 * pcm16, byte-swapped on request (the file writer) -- and host_bufs[s], when given, gets stream s's buf_len frames.
	 * more[s] is the float run's; out_len[s] = ceil(the float run's / factor). The history belongs to a sequence of decimated
	 * runs with one (factor, stereo): any other run in between, or another pair, starts it from zero. False with "bad
	 * argument" on another factor or buf_len * factor beyond 32 bits, and with the backend's text on one without a decimator
	 * or float output; nothing is rendered then and the batch stands where it stood. Once every stream has ended nothing is
	 * rendered; the rows then hold the filter's tail. */
	bool run_decimated(void *const *host_bufs, SampleFormat out_fmt, bool swap_bytes, int factor, size_t buf_len, bool stereo,
			bool *more, size_t *out_len, std::string &err);
	/* start such a sequence now (run_decimated does it itself; the file writer asks before it opens a file) */
	bool begin_decimated(int factor, bool stereo, std::string &err);

	/* A float run of buf_len frames, limited on the device (include/saugns_amd.h: sauAmd_Batch_run_limited_f32). The limited
	 * rows stay on the device (Backend::device_limited_f32, fetch_limited_async) -- float32, or with out_fmt SF_S16 the kernels'
	 * own pcm16, byte-swapped on request (the file writer) -- and host_bufs[s], when given, gets stream s's buf_len frames: the
	 * sequence delayed by limiter_latency(rate). more[s] and out_len[s] are the float run's. The history belongs to a sequence
	 * of limited runs with one (pre_gain, ceiling, stereo): any other run in between, or another triple, starts it from zero.
	 * False with "bad argument" on parameters that are not finite and positive or while loudness metering is on, and with the
	 * backend's text on one without a limiter or float output; nothing is rendered then and the batch stands where it stood.
	 * Once every stream has ended nothing is rendered; the rows then hold the tail. */
	bool run_limited(void *const *host_bufs, SampleFormat out_fmt, bool swap_bytes, float pre_gain, float ceiling, size_t buf_len,
			bool stereo, bool *more, size_t *out_len, std::string &err);
	/* start such a sequence now (run_limited does it itself; the file writer asks before it opens a file) */
	bool begin_limited(float pre_gain, float ceiling, bool stereo, std::string &err);
	/* the streams' statistics, out[n_streams()]; empty ones (0, 0, 1.0) while no limited sequence has ever begun */
	bool limiter_stats(LimiterStats *out, bool reset, std::string &err);

	/* Level metering (include/saugns_amd.h: sauAmd_Batch_set_metering). On: every run ends with the backend measuring each
	 * stream's frames [0, out_len) of that run, in the run's format, into the stream's record. Off (the default): run() makes
	 * no call for it. False, with the switch where it was, on a backend without metering. */
	bool set_metering(bool on, std::string &err) {
		if (on && !metering_ && !backend_->begin_metering(err)) return false;
		if (on) metered_ = true;
		metering_ = on;
		return true;
	}
	bool metering() const { return metering_; }
	/* the streams' records, out[n_streams()]; all zero while metering has never been on */
	bool levels(Levels *out, bool reset, std::string &err);

	/* Loudness metering (include/saugns_amd.h: sauAmd_Batch_set_loudness). On: every float run ends with the backend taking
	 * each stream's frames [0, out_len) into the stream's loudness record, and int16 and decimated runs are refused. Off (the
	 * default): run() makes no call for it. False, with the switch where it was, on a backend without it or a rate below
	 * LOUD_MIN_RATE. The records belong to one channel layout: a float run of the other one while on is refused until a reset. */
	bool set_loudness(bool on, std::string &err) {
		if (on && srate_ < LOUD_MIN_RATE) { err = "bad argument: loudness metering needs a rate of 2560 Hz or more"; return false; }
		if (on && !loud_begun_ && !backend_->begin_loudness(err)) return false;
		if (on) loud_begun_ = true;
		loudness_ = on;
		return true;
	}
	/* the streams' records, out[n_streams()]; empty ones while loudness has never been on */
	bool loudness(Loudness *out, bool reset, std::string &err);
	bool loudness_hops(size_t stream, double *out, size_t cap, size_t *n_hops, std::string &err);

	/* Size the device buffers for runs of up to `frames` frames now (run() grows them on demand, which waits for the
	 * stream: a host that knows its longest run says so once). */
	bool reserve(size_t frames, bool stereo, std::string &err);

	/* The size of the sauGenerator_run calls whose block lattice the engine reproduces (see
	 * Lattice in sau_dev_math.h): the reference starts a new <= 1024-frame block at every call
	 * (generator.c:854-878). 0 (default): every run() is one such call; otherwise a run() covers
	 * calls of that many frames each (read-ahead, file output). */
	void set_call_len(size_t frames) { call_len_ = frames > UINT32_MAX ? UINT32_MAX : (uint32_t)frames; }

	/* PCM is produced byte-swapped from the next run on (AU output) */
	void set_pcm_byteswap(bool on) { pcm_swap_ = on; }
	size_t n_streams() const { return streams_.size(); }
	Backend *backend() { return backend_; }

	/* The engine as it stands -- event positions, voice durations, operator mirrors, the call lattice's phase, and (by the
	 * backend, under `slot`) every operator's record -- so that restore() can take a render back to this frame: sauGenerator_run
	 * takes `buf_len` and `stereo` per call (sau/generator.c:905-913), and frames rendered ahead for calls of one kind are
	 * not what the reference gives a host that then asks for another. Plans are not kept: they are a function of the
	 * operator mirrors and are compiled again after a restore. */
	struct Snapshot {
		struct StreamState {
			size_t event = 0; uint32_t event_pos = 0, voice = 0; uint64_t since_event = 0;
			struct Vo { uint32_t duration, carr_op; bool init; };
			std::vector<Vo> voices;
			std::vector<OpMirror> ops;
		};
		std::vector<StreamState> streams;
		uint64_t frames_done = 0;
		uint32_t call_len = 0, lat_call = 0, call_phase = 0;
		bool out_dirty = false, valid = false;
	};
	bool snapshot(Snapshot &s, int slot, std::string &err);
	bool restore(const Snapshot &s, int slot, std::string &err);
	uint64_t frames_done() const { return frames_done_; }

private:
	struct EventNode { uint32_t wait; const sauProgramEvent *pe; };
	struct VoiceHost {
		uint32_t duration = 0;
		bool init = false;
		uint32_t carr_op = 0;
		VoicePlan plan;
		bool plan_valid = false;
		int32_t shape = -1;  /* its entry of shapes_ (voices of one shape share one step list on the device), or -1 */
	};
	/* compiled plans by graph shape (voice_plan_shape) */
	struct Shape { std::vector<uint32_t> tokens; VoicePlan plan; uint32_t plan_ofs = 0; uint64_t placed = 0; };
	std::vector<Shape> shapes_;
	std::unordered_multimap<uint64_t, uint32_t> shape_by_hash_;
	std::vector<uint32_t> shape_tokens_, shape_ids_, shape_stamp_;
	uint32_t shape_mark_ = 0;
	uint64_t rebuilds_ = 0;
	bool plan_cache_ = true, plan_check_ = false;
	bool loop_tails_ = true;
	bool poison_ = false; /* SAU_AMD_POISON (tests): Backend::poison_run ahead of every run */
	struct Stream {
		const sauProgram *prg = nullptr;
		std::vector<EventNode> events;
		size_t event = 0;
		uint32_t event_pos = 0;
		std::vector<VoiceHost> voices;
		uint32_t voice = 0;
		float amp_scale = 0.f;
		uint32_t op_base = 0;   /* offset into the global op array */
		uint32_t vo_base = 0;
		std::vector<OpMirror> ops;
		/* per-call output length accounting (generator.c:938-949) */
		size_t call_gen = 0, part_start = 0, part_gen = 0;
		uint64_t since_event = 0; /* frames since this program's latest event */
	};

	Engine() {}
	bool handle_event(Stream &st, const EventNode &e, std::vector<OpUpdate> &batch,
			std::vector<uint8_t> &touched, std::string &err);
	bool flush_updates(std::vector<OpUpdate> &batch, std::vector<uint8_t> &touched,
			std::string &err);
	bool rebuild_plans(std::string &err);
	uint32_t estimate_sum_levels(const Stream &st, uint32_t op, uint32_t parent_dep, bool parent_varies,
			uint32_t &need, uint32_t nest) const;
	bool render_segment(uint32_t len, uint32_t offset, bool stereo, std::string &err);

	Backend *backend_ = nullptr;
	uint32_t srate_ = 0;
	std::vector<Stream> streams_;
	uint32_t total_ops_ = 0, total_voices_ = 0;
	uint32_t reserved_frames_ = 0;
	bool reserved_stereo_ = false;
	bool pcm_swap_ = false;
	SampleFormat format_ = SF_S16;   /* of the run being rendered */
	bool metering_ = false;          /* set_metering() */
	bool metered_ = false;           /* ... has ever been on: the backend has records */
	std::vector<uint32_t> meter_frames_; /* per stream: out_len of the run at hand */
	bool loudness_ = false;          /* set_loudness() */
	bool loud_begun_ = false;        /* ... has ever been on: the backend has records */
	int loud_channels_ = 0;          /* the channel layout the records belong to (0: none yet, or reset) */
	int decim_factor_ = 0;           /* run_decimated(): the sequence at hand (0: none -- any other run ends it) */
	bool decim_stereo_ = false;
	bool in_decimated_ = false;      /* run() is run_decimated()'s own */
	bool all_ended_ = false;         /* the last run left no stream with anything to render */
	std::vector<uint32_t> decim_frames_; /* per stream: the float run's out_len */
	bool lim_seq_ = false;           /* run_limited(): a sequence is at hand (any other run ends it) */
	bool lim_begun_ = false;         /* ... one has ever begun: the backend has statistics */
	float lim_gain_ = 0.f, lim_ceiling_ = 0.f;
	bool lim_stereo_ = false;
	bool in_limited_ = false;        /* run() is run_limited()'s own */
	bool plans_dirty_ = true;
	/* concatenated plans as uploaded; per (stream,voice) offsets */
	std::vector<Step> all_steps_;
	std::vector<FastIds> all_fast_ids_, all_fast_ids_full_;
	std::vector<uint32_t> all_op_ids_;
	struct PlanRef { uint32_t plan_ofs, plan_len, ops_ofs, nops; };
	std::vector<PlanRef> plan_refs_; /* indexed by global voice index */
	uint64_t frames_done_ = 0;
	uint32_t call_len_ = 0;          /* set_call_len() */
	uint32_t lat_call_ = 0;          /* call size of the lattice in force */
	uint32_t call_phase_ = 0;        /* frames into the reference's current call at the start of run() */
	uint32_t seg_call_pos_ = 0;      /* ... at the start of the segment being rendered */
};

/* tables.cpp */
const float *builtin_piluts();            /* 12 x 2048, built on first use */
const WaveConst *wave_consts();           /* 12 */
void override_piluts(const float *tables);/* replace (e.g. host's own tables) */

} /* namespace sauengine */
#endif
