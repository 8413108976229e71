/* saugns_amd.h -- C ABI of the MI355X generator backend (libsaugns_amd.so).
 *
 * Part 1 is the drop-in boundary: exactly the symbols sau/generator.o exports
 * in the reference, with the same argument meaning and
 * error behaviour.  Linking this library ahead of -lsau makes the unchanged
 * reference host (parser, player) render on the GPU; see INTEGRATION.md.
 *
 * Part 2 are extensions around the same hot path: many programs rendered in
 * lock step (BASELINE config 4), device-resident PCM, wave-table injection,
 * and a pointer-free program image so that programs can be stored and
 * rebuilt without the reference parser.
 *
 * Plain pointers and sizes only; no C++ or torch types cross this boundary.
 */
#ifndef SAUGNS_AMD_H
#define SAUGNS_AMD_H

#include "sau_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SAU_AMD_API __attribute__((visibility("default")))

/* ---- Part 1: drop-in boundary ------------------------------------------- */

typedef struct sauGenerator sauGenerator;

/* replaces sau/generator.h:20-21 (generator.c:200-217).
 * NULL on failure (no usable GPU, out of memory, graph too large). */
SAU_AMD_API sauGenerator *sau_create_Generator(const sauProgram *prg, uint32_t srate);

/* replaces sau/generator.h:22 (generator.c:222-228). NULL-safe. */
SAU_AMD_API void sau_destroy_Generator(sauGenerator *o);

/* replaces sau/generator.h:24-26 (generator.c:905-973): fill buf with
 * buf_len frames (interleaved L,R when stereo, else (L+R)/2); returns false
 * once the signal has ended, with *out_len = frames generated this call. */
SAU_AMD_API bool sauGenerator_run(sauGenerator *o, int16_t *buf, size_t buf_len,
		bool stereo, size_t *out_len);

/* replaces the definition in sau/generator/noise.h:18-21, which the
 * reference's parser.o and help.o import. */
SAU_AMD_API extern const char *const sauNoise_names[SAU_NOISE_NAMED + 1];

/* ---- Part 2: extensions --------------------------------------------------- */

typedef struct sauAmdBatch sauAmdBatch;

/* n independent programs rendered together; stream i renders prgs[i].
 * Programs are borrowed and must outlive the batch. NULL on failure. */
SAU_AMD_API sauAmdBatch *sauAmd_create_Batch(const sauProgram *const *prgs, size_t n,
		uint32_t srate);
/* The same on HIP device `device` (0 <= device < sauAmd_device_count()) whatever SAU_AMD_DEVICE says: a host that shards
 * independent renders over the GPUs of a node from one process (contiguous blocks of renders per GPU, no exchange
 * step) creates one batch per device and runs them side by side -- every batch has its own stream, buffers, pools and budget
 * for the feedback chains' rows. NULL on failure (sauAmd_last_error), also for a device that does not exist. */
SAU_AMD_API sauAmdBatch *sauAmd_create_Batch_on(int device, const sauProgram *const *prgs, size_t n,
		uint32_t srate);
SAU_AMD_API void sauAmd_destroy_Batch(sauAmdBatch *b);

/* Advance every stream by buf_len frames. bufs may be NULL, or hold one host
 * pointer per stream (entries may be NULL): PCM is copied there; otherwise it
 * stays on the device. more[i]/out_len[i] (either may be NULL) as
 * sauGenerator_run for stream i. Returns false on a backend error. */
SAU_AMD_API bool sauAmd_Batch_run(sauAmdBatch *b, int16_t *const *bufs, size_t buf_len,
		bool stereo, bool *more, size_t *out_len);

/* The reference restarts its <= 1024-frame rendering blocks at every sauGenerator_run call
 * (generator.c:854-878), and the positions of held lines move block by block (sau/line.c:385-398),
 * so a render depends -- in rare event sequences -- on the caller's buffer size. By default each
 * sauAmd_Batch_run call stands for one such call. frames > 0: a run covers consecutive calls of
 * that many frames each (rendering far ahead of a host that asks for 11289 frames at a time). */
SAU_AMD_API void sauAmd_Batch_set_call_len(sauAmdBatch *b, size_t frames);

/* Device address of stream i's PCM row of the last run (hipMalloc memory); NULL when that run was a float32 run. */
SAU_AMD_API const int16_t *sauAmd_Batch_device_pcm(sauAmdBatch *b, size_t stream);

/* Float32 sample output. sauAmd_Batch_run_f32 is sauAmd_Batch_run, sample for sample in time (buf_len, the block lattice and
 * sauAmd_Batch_set_call_len mean what they mean there), with the mixer's f32 accumulator stored as it stands: the reference's
 * ordered voice sum (generator.c:749-788), L, R interleaved when stereo, else (L + R) * 0.5f -- not clamped to +-1, not
 * rounded to 15 bits, a NaN left a NaN; frames of [0, out_len) in which nothing sounds are +0.0f. The int16 sample of
 * sauAmd_Batch_run is this one clamped and rounded. The format belongs to the call: run and run_f32 calls may alternate on
 * one batch in any order, each continues where the last one stopped. False (sauAmd_last_error) on a backend without float
 * output: nothing is rendered then and the batch stands where it stood. */
SAU_AMD_API bool sauAmd_Batch_run_f32(sauAmdBatch *b, float *const *bufs, size_t buf_len,
		bool stereo, bool *more, size_t *out_len);
/* Device address of stream i's float32 row of the last run; NULL when that run was an int16 run. */
SAU_AMD_API const float *sauAmd_Batch_device_pcm_f32(sauAmdBatch *b, size_t stream);
/* Bytes between the rows of consecutive streams in the last run's format: all streams' rows are one strided array
 * (0 on a backend that keeps no device PCM). Rows may move when a run is longer than any before it or changes the format. */
SAU_AMD_API size_t sauAmd_Batch_device_pcm_pitch(sauAmdBatch *b);

/* Wait for all queued device work of the batch. */
SAU_AMD_API bool sauAmd_Batch_sync(sauAmdBatch *b);

/* Accumulated HIP-event timings of the render / mix kernels since the last
 * call with reset != 0 (any pointer may be NULL). Enables timing on first use. */
SAU_AMD_API void sauAmd_Batch_timing(sauAmdBatch *b, double *render_ms, double *mix_ms,
		uint64_t *render_launches, int reset);

/* Per-kernel split of the same timings: out4[0] time-parallel kernel
 * (fast_kernel), [1] block-loop kernel (render_kernel), [2] mixer, [3] analyze
 * + finalize, all in ms; *segments = number of rendered segments. */
SAU_AMD_API void sauAmd_Batch_timing_ex(sauAmdBatch *b, double *out4, uint64_t *segments,
		int reset);

/* HIP-event timing: 0 off, 1 only the dominant (time-parallel) kernel,
 * 2 every kernel. The query functions above switch level 2 on when still off. */
SAU_AMD_API void sauAmd_Batch_set_timing(sauAmdBatch *b, int level);

/* The stream the batch launches its kernels on, as a hipStream_t. */
SAU_AMD_API void *sauAmd_Batch_stream(sauAmdBatch *b);

/* Order b's next run behind what has been issued for `before` so far: the rendering kernels of b's next
 * sauAmd_Batch_run start on the device only when everything queued for `before` has finished (b's bookkeeping --
 * operator updates, plan uploads, the per-voice analysis -- may run earlier: it touches nothing of `before`'s).
 * A host that renders one script after another with two generators alive (saugns.c:583-621 per script) issues
 * script k + 1 while script k's last kernels drain: the host work of a run's start (events at t = 0, plans: 1.2 ms
 * for BASELINE config 5's 4096 voices) overlaps the device's tail, and the two scripts' kernels never compete for
 * the device -- two runs simply issued side by side did, at three times the time per script. Both on the same
 * device. false (sauAmd_last_error) on a HIP error. */
SAU_AMD_API bool sauAmd_Batch_order_after(sauAmdBatch *b, sauAmdBatch *before);

/* Use these twelve 2048-entry tables (wave-id order) instead of the built-in
 * ones for generators created afterwards. */
SAU_AMD_API void sauAmd_set_piluts(const float *tables);
/* The tables a new generator would use. */
SAU_AMD_API const float *sauAmd_get_piluts(void);

/* Text of the last error on this thread ("" if none). */
SAU_AMD_API const char *sauAmd_last_error(void);

/* Number of visible HIP devices; <= 0 when none or HIP is unusable. */
SAU_AMD_API int sauAmd_device_count(void);
/* PCI address ("0000:c1:00.0") of HIP device `device` into buf (len >= 16); false when there is no such device. One
 * process per GPU (SAU_AMD_DEVICE selects it): a multi-rank job can show that its ranks sit on distinct boards. */
SAU_AMD_API bool sauAmd_device_pci_bus_id(int device, char *buf, size_t len);

/* Program image: every struct of a sauProgram in one relocatable block.
 * serialize returns the size needed; nothing is written if cap is smaller. */
SAU_AMD_API size_t sauAmd_program_serialize(const sauProgram *prg, void *buf, size_t cap);
/* Rebuild a sauProgram from an image (one allocation; free with _free). */
SAU_AMD_API sauProgram *sauAmd_program_load(const void *image, size_t len);
SAU_AMD_API void sauAmd_program_free(sauProgram *prg);

/* Voice banks without the parser (for a 1024-voice bank sau_build_Program,
 * sau/parser.c:2092, takes longer than the whole render here). Operators are given as a flat array: carriers
 * (use == SAU_POP_N_carr, one voice each, in time order) and modulators naming their parent's index and how it
 * uses them. The result is laid out as the parser lays out the equivalent script -- one event per voice,
 * operator data in post-order, ids in pre-order, line and time flags of freshly created operators -- and is
 * accepted by sau_create_Generator / sauAmd_create_Batch like any other program. */
typedef struct sauAmdLineDesc {
	uint8_t present;   /* 0: the parameter is not given (the generator's default applies) */
	uint8_t has_goal;  /* a sweep to `goal` over the operator's time */
	uint8_t ratio;     /* frequency lines: value is a ratio of the parent's frequency */
	uint8_t shape;     /* SAU_LINE_N_* */
	float v0, goal;
} sauAmdLineDesc;
typedef struct sauAmdOpDesc {
	uint32_t parent;   /* index of the operator this one modulates (ignored for carriers) */
	uint32_t use;      /* SAU_POP_N_* */
	uint32_t type;     /* SAU_POPT_N_* */
	uint32_t mode;     /* W: wave id; N: noise id; R: line | function flags << 8 | function << 16 */
	uint32_t time_ms;  /* 0: implicit (lasts as long as its parent), lines then take default_mod_ms */
	uint32_t start_ms; /* carriers: when the voice begins */
	uint32_t phase;    /* cycle fraction, 2^32 = one turn */
	uint32_t seed;
	sauAmdLineDesc pan, amp, amp2, freq, freq2, pm_a;
} sauAmdOpDesc;
/* NULL on a malformed description: parent out of range, cycles, voices out of time order, an operator type,
 * wave / noise id, R line or function or a ramp shape outside its enum, a carrier with time_ms == 0 (a voice's
 * length is its carrier's), nesting deeper than 255, a duration beyond 32 bits of milliseconds. */
SAU_AMD_API sauProgram *sauAmd_build_bank(const sauAmdOpDesc *ops, size_t n_ops, float ampmult,
		uint32_t default_mod_ms);
SAU_AMD_API void sauAmd_free_bank(sauProgram *prg);

/* Output stage (replaces the reference's player/sndfile.c:125-210 writer fed
 * from Player_run's chunk loop, saugns.c:589-618): render prg to a sound file.
 * format as SGS_SNDFILE_* (player/sndfile.h:21-26); channels 1 or 2. The file
 * is byte-identical to what the reference writer produces from the same PCM.
 * *frames_out (may be NULL) = frames written. False on failure. */
/* SAU_AMD_SNDFILE_WAV_F32 (an extension: the reference writes int16 only): the float32 samples of sauAmd_Batch_run_f32 as
 * WAVE_FORMAT_IEEE_FLOAT -- `fmt ` chunk of 18 bytes (tag 3, 32 bits, cbSize 0), `fact` chunk with the frame count, `data`. */
enum { SAU_AMD_SNDFILE_RAW = 0, SAU_AMD_SNDFILE_AU = 1, SAU_AMD_SNDFILE_WAV = 2, SAU_AMD_SNDFILE_WAV_F32 = 3 };
SAU_AMD_API bool sauAmd_render_file(const sauProgram *prg, uint32_t srate, const char *path,
		int format, int channels, uint64_t *frames_out);

/* ---- Level metering ---------------------------------------------------------
 * Is this render clipping, and by how much should it be scaled? -- answered where the samples are, without fetching them.
 * One record per stream (or row). What a sample x is: a float row's sample as it stands; an int16 row's sample s measured
 * in integers (max |s|, the sum of s * s in 64 bits) and converted once on the host: peak = (float)max|s| / 32767.0f,
 * sum_sq = (double)sum / (32767.0 * 32767.0), full_scale counts |s| >= 32767, over counts s == -32768, nonfinite is 0 -- a
 * single int16 measurement is exact. Float rows: x * x is formed in f64 (exact) and summed in f64; full_scale counts what an
 * int16 run of the same frames would put on the rail (the kernels' own rounding, a NaN included: it becomes -32767).
 * The sums are reproducible: no atomics, a fixed share of the row per workgroup and a fixed order of every addition, so
 * the same rows give the same bits on any MI355X partition. */
typedef struct sauAmdLevels {
	uint64_t frames;        /* frames measured */
	float    peak[2];       /* max |x| over finite samples; [0] L or mono, [1] R (0 on mono) */
	double   sum_sq[2];     /* sum of x*x over finite samples, in f64 */
	uint64_t over[2];       /* samples the int16 clamp alters: |x| > 1, or not finite */
	uint64_t full_scale[2]; /* samples whose pcm16() is +-32767 */
	uint64_t nonfinite[2];  /* NaN or +-inf (left out of peak and sum_sq) */
} sauAmdLevels;
#ifdef __cplusplus
static_assert(sizeof(sauAmdLevels) == 80, "sauAmdLevels is 80 bytes");
#else
_Static_assert(sizeof(sauAmdLevels) == 80, "sauAmdLevels is 80 bytes");
#endif

/* Metering is off by default, and while it is off a run does nothing for it. On: every sauAmd_Batch_run / _run_f32 ends with
 * the device measuring stream i over the frames [0, out_len[i]) of that run -- in the run's format, on the batch's stream,
 * before any copy to the host; frames behind a stream's end are not measured and a stream that has ended adds nothing -- and
 * adding the result to stream i's record on the device. int16 and float runs may alternate. False (sauAmd_last_error), with
 * nothing changed, on a backend without metering; switching it off always succeeds and keeps the records. */
SAU_AMD_API bool sauAmd_Batch_set_metering(sauAmdBatch *b, int on);
/* Wait for the batch's stream and copy the records out, one per stream; reset != 0 clears them afterwards. All zero while
 * metering has never been on. */
SAU_AMD_API bool sauAmd_Batch_levels(sauAmdBatch *b, sauAmdLevels *out /* [streams] */, int reset);
/* The same measurement of n_rows rows the caller holds on the batch's device (say, the rows of sauAmd_Batch_device_pcm_f32
 * after the caller's own processing): row r begins pitch_bytes * r bytes behind `rows` and holds `frames` frames of
 * `channels` (1, or 2 interleaved) samples, float32 when f32 != 0, else int16 in host byte order. `rows` and pitch_bytes must
 * be multiples of 16 and channels 1 or 2 -- anything else is refused as a bad argument, as are rows that are not wholly inside
 * one allocation of that device. Synchronous: what the caller has queued for the rows on other streams must have finished;
 * the call returns with out[0 .. n_rows) written. The batch's own records are untouched. frames == 0 gives zeroed records. */
SAU_AMD_API bool sauAmd_Batch_measure_rows(sauAmdBatch *b, const void *rows, size_t pitch_bytes, size_t n_rows,
		int f32, size_t frames, int channels, sauAmdLevels *out /* [n_rows] */);
/* sauAmd_render_file to a target peak: the file holds x * gain, gain = target_peak / max(peak[0], peak[1]) (one f32 division;
 * 1 for a silent program), and the int16 formats round once, after the gain: pcm16(x * gain). The render is made TWICE: a
 * script's length is unbounded, so the whole render cannot be kept in device memory until its peak is known, and renders are
 * deterministic -- the first pass renders float runs with metering on and fetches nothing, the second renders the same runs
 * again and writes them scaled. format and channels as for sauAmd_render_file (SAU_AMD_SNDFILE_WAV_F32 writes x * gain as
 * floats); target_peak must be finite and > 0. *levels_out (may be NULL) = the first pass's record, before the gain. False
 * (sauAmd_last_error), before any file is created, on a bad argument or a backend without metering. */
SAU_AMD_API bool sauAmd_render_file_normalized(const sauProgram *prg, uint32_t srate, const char *path, int format,
		int channels, float target_peak, uint64_t *frames_out, sauAmdLevels *levels_out);

/* ---- Oversampled rendering ---------------------------------------------------
 * The reference's oscillators are not band-limited: PM chains, `sqr`/`saw` tables, FM and noise put energy above the
 * Nyquist frequency, and a render folds it back into the audible band. The cure is to render at `factor` times the wanted
 * rate and low-pass down to it -- here on the device, on the float rows of sauAmd_Batch_run_f32, without fetching them.
 *
 * The filter, for factor K in {2, 4, 8}: half-length H = 32 output frames, L = 2 * H * K + 1 taps (129, 257, 513), centre
 * C = H * K; g[n] = sinc((n - C) / K) * I0(beta * sqrt(1 - ((n - C) / C)^2)) / I0(beta) for n = 0 .. C, beta = 10.06,
 * sinc(t) = sin(pi t) / (pi t), I0 by its power series; g[L - 1 - n] = g[n] mirrored; h = g / sum(g). In f64, on the host.
 * Passband to 0.45 of the output rate within 2e-4 dB, -6.02 dB at half of it, stopband from 0.55 of it below -98 dB.
 *
 * The arithmetic is reproducible bit for bit. With x[i] the float sample of high-rate frame i of a stream and channel,
 * counted from the start of the decimated sequence, +0.0f for i < 0 and for every frame at or behind the stream's end:
 *   acc = +0.0 (f64); for j = 0 .. L-1 ascending: acc = acc + h[j] * (double)x[m * K - j]; y[m] = (float)acc
 * -- one accumulator per output sample, a multiply and then an add, no sum split or reordered. The filter is causal: the
 * output lags the input by exactly H output frames. */

/* sauAmd_decimator_taps: L, and the L taps h in out[] when cap >= L (nothing is written when cap < L; out may then be
 * NULL); 0 for a factor other than 2, 4, 8. sauAmd_decimator_latency: H = 32 output frames; 0 for such a factor. */
SAU_AMD_API size_t sauAmd_decimator_taps(int factor, double *out, size_t cap);
SAU_AMD_API size_t sauAmd_decimator_latency(int factor);
/* A float run of buf_len * factor frames, decimated on the device to buf_len frames per stream. The batch was created at
 * srate_out * factor: a run advances every stream by buf_len * factor frames of the batch's rate, and
 * sauAmd_Batch_set_call_len stays in those high-rate frames. more[i] is the float run's; out_len[i] =
 * ceil(out_len_hi[i] / factor) of the float run's out_len_hi. Every stream's decimated row -- and bufs[i] when given (bufs
 * may be NULL) -- holds buf_len valid frames, the input zero-extended behind the stream's end: a stream's tail therefore
 * appears in later runs, and a run after every stream has ended renders nothing and still delivers buf_len frames of it.
 * The history belongs to a sequence of decimated runs with the same (factor, stereo): a decimated run that follows a
 * sauAmd_Batch_run, a sauAmd_Batch_run_f32, or a decimated run with another (factor, stereo) starts from zero history.
 * False (sauAmd_last_error) with "bad argument" on a factor other than 2, 4, 8 or buf_len * factor beyond 32 bits, and on a
 * backend without a decimator or float output; nothing is rendered then and the batch stands where it stood. A batch that
 * never makes a decimated run does nothing for it. */
SAU_AMD_API bool sauAmd_Batch_run_decimated_f32(sauAmdBatch *b, int factor, float *const *bufs, size_t buf_len,
		bool stereo, bool *more, size_t *out_len);
/* Device address of stream i's decimated float row of the last decimated run (NULL before one), and the bytes between the
 * rows of consecutive streams. The rows are 16-byte aligned and the pitch is a multiple of 256, so
 * sauAmd_Batch_measure_rows measures them as they are. Valid until the batch's next decimated run (call sauAmd_Batch_sync
 * first: the run is asynchronous). */
SAU_AMD_API const float *sauAmd_Batch_device_decimated_f32(sauAmdBatch *b, size_t stream);
SAU_AMD_API size_t sauAmd_Batch_device_decimated_pitch(sauAmdBatch *b);
/* sauAmd_render_file, rendered at srate * factor and decimated on the device: the high-rate signal is exactly what
 * sauAmd_render_file(prg, srate * factor, ..) writes (the same call lattice), the filter's delay of H frames is dropped and
 * its tail kept, so the file holds exactly ceil(N / factor) frames for N high-rate frames, time-aligned with them, and its
 * header carries srate. format and channels as for sauAmd_render_file; the int16 formats are pcm16 of the f64 sum rounded
 * to float, formed (and for AU byte-swapped) on the device. False (sauAmd_last_error), before any file is created, on a
 * bad argument -- another factor, srate * factor beyond 32 bits -- or a backend without float output or a decimator. */
SAU_AMD_API bool sauAmd_render_file_oversampled(const sauProgram *prg, uint32_t srate, int factor, const char *path,
		int format, int channels, uint64_t *frames_out);

#ifdef __cplusplus
}
#endif
#endif /* SAUGNS_AMD_H */
