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
 * sauAmd_Batch_run is this one clamped and rounded. The claim is tested against the oracle's float output (ora_run_f32), bit for
 * bit, a NaN for a NaN (tests/test_gpu_f32_oracle.py). The format belongs to the call: run and run_f32 calls may alternate on
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

/* The stream the batch launches its kernels on, as a hipStream_t, with everything issued for the batch so far ordered on it.
 * A run's last kernel -- the mixer that writes the PCM rows -- may run on a second stream of the batch's (beside the next
 * run's set-up); this call, like sauAmd_Batch_device_pcm, _device_pcm_f32 and _device_pcm_pitch, joins it onto the stream it
 * returns. So a caller that reads a run's rows on the device (bufs == NULL) with work of its own on this stream calls
 * sauAmd_Batch_stream -- or one of those three -- AFTER that run, every run: the handle and the row pointers stay the same
 * from run to run, the ordering is what the call makes. Work enqueued on a handle obtained before the run, with no such
 * call and no sauAmd_Batch_sync in between, is not ordered behind that run's mixer. */
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

/* ---- Loudness and true peak ---------------------------------------------------
 * sauAmdLevels answers "is it clipping"; a delivery target is programme loudness (ITU-R BS.1770-4 / EBU R 128, in LUFS) under a
 * true-peak ceiling (dBTP: the peaks between the samples included). Both are measured where the samples are, on the float rows
 * of sauAmd_Batch_run_f32; the gating runs on the host over 16 bytes per 100 ms.
 *
 * The arithmetic is a fixed order of IEEE operations (the build is -ffp-contract=off: a product is rounded, then the sum): the
 * same rows in the same sequence of run lengths give the same bits on any MI355X partition -- no atomics, no sum whose order
 * depends on scheduling. A sample x is the float sample as a double; a NaN or +-inf counts as +0.0 throughout
 * (sauAmdLevels.nonfinite counts those).
 *
 * K-weighting, for the rate fs, in f64 on the host (the bilinear-transform forms that give BS.1770's table at 48 kHz):
 *   stage 1, high shelf: f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196;
 *     K = tan(pi f0 / fs), Vh = 10^(G / 20), Vb = Vh^0.4996667741545416, a0 = 1 + K / Q + K K;
 *     b = [(Vh + Vb K / Q + K K) / a0, 2 (K K - Vh) / a0, (Vh - Vb K / Q + K K) / a0], a1 = 2 (K K - 1) / a0, a2 = (1 - K / Q + K K) / a0
 *   stage 2, high-pass: f0 = 38.13547087602444, Q = 0.5003270373238773, K and a0 as above;
 *     b' = [1, -2, 1], a1' = 2 (K K - 1) / a0, a2' = (1 - K / Q + K K) / a0
 * One frame updates the state (s1, s2, t1, t2), transposed direct form II, every product rounded and then every sum:
 *   u = b0 x + s1;    s1 = (b1 x - a1 u) + s2;     s2 = b2 x - a2 u
 *   y = b0' u + t1;   t1 = (b1' u - a1' y) + t2;   t2 = b2' u - a2' y
 * Chunks make the recurrence parallel. A chunk is 256 frames -- a constant, never a function of the device: chunk c of a run
 * is the stream's frames [256 c, 256 c + 256) of that run, cut at the stream's frame count for the run. M is the 4x4 map of
 * the state over 256 frames of zero input (column k: the frame update run 256 times from the k-th unit state), z_c the state
 * after chunk c evaluated from zero state, S_0 the state the stream's previous metered run left (zero at the start and after
 * a reset). Behind a FULL chunk c
 *   S_{c+1}[r] = ((((0.0 + M[r][0] S_c[0]) + M[r][1] S_c[1]) + M[r][2] S_c[2]) + M[r][3] S_c[3]) + z_c[r]
 * and chunk c is then evaluated frame by frame from S_c; the state after the run's last chunk, full or partial, evaluated that
 * way is what the stream carries on. A stream with no frames in a run changes nothing.
 * Hop energies. hop = fs / 10 frames (integer division; fs >= 2560, so a chunk never touches more than two hops). A stream
 * counts its metered frames from 0, and the frame at position p belongs to hop p / hop. Evaluating chunk c gives one sum per
 * hop it touches: acc = +0.0, then for its frames of that hop ascending acc = acc + y y. E[h][ch], the running f64 sum of
 * hop h (+0.0 before anything is added), takes those sums in ascending chunk order, within a chunk the earlier hop first.
 * True peak. 4x interpolation with the decimator's formula for K = 4, half-length H = 16 input frames, beta = 5.0: g[n],
 * n = 0 .. 128, is that section's Kaiser-windowed sinc, NOT normalised (passband to 0.45 of the rate within 0.02 dB, stopband
 * from 0.55 of it below -53 dB). For a stream's frame m and phase p = 1, 2, 3:
 *   acc = +0.0; for q = 0 .. 31 ascending: acc = acc + g[4 q + p] x[m - q]; w = (float)acc
 * with x = +0.0 before the stream's first metered frame (31 frames are carried from run to run). true_peak[ch] is the largest
 * of |x[m]| as a float and every finite |w|, compared as bit patterns. The positions that lag behind a stream's last frame
 * -- m = N .. N + 30 with zeros for x[N ..] -- are covered when the record is read: on the host, into the copy that is
 * returned; the device state is untouched and later runs continue exactly.
 * Gating, in f64 on the host over the complete hops. Block j covers hops j .. j + 3:
 *   z_j = 0.0, then for ch ascending z_j = z_j + (((E[j][ch] + E[j+1][ch]) + E[j+2][ch]) + E[j+3][ch]) / (4.0 hop)
 * (every channel has weight 1: BS.1770 for mono and for L/R); l_j = -0.691 + 10 log10(z_j), or -inf for 0; momentary_max =
 * max l_j; the absolute gate keeps blocks with l_j > -70, the relative gate those of them with l_j > (-0.691 + 10 log10(mean
 * z of the absolute-gated blocks)) - 10; integrated = -0.691 + 10 log10(mean z of the blocks passing both). A mean is the
 * sum in ascending j divided by the count. With no block, or none passing, the result is -HUGE_VAL.
 *
 * Limits: float runs only (decimated rows are not metered yet -- fetch the hops of a float run at the low rate instead);
 * fs >= 2560; one channel layout per record; no loudness range or short-term measure yet (sauAmd_Batch_loudness_hops gives a
 * caller what those need). */
typedef struct sauAmdLoudness {
	uint64_t frames;        /* frames measured */
	uint64_t blocks;        /* 400 ms blocks: complete hops - 3, or 0 */
	uint64_t gated_blocks;  /* those passing both gates */
	double   integrated;    /* LUFS; -HUGE_VAL when no block passes */
	double   momentary_max; /* LUFS; -HUGE_VAL without a block */
	float    true_peak[2];  /* [0] L or mono, [1] R (0 on mono) */
} sauAmdLoudness;
#ifdef __cplusplus
static_assert(sizeof(sauAmdLoudness) == 48, "sauAmdLoudness is 48 bytes");
#else
_Static_assert(sizeof(sauAmdLoudness) == 48, "sauAmdLoudness is 48 bytes");
#endif

/* The ten coefficients b0 b1 b2 a1 a2, b0' b1' b2' a1' a2' for a rate; false (nothing written) below 2560 Hz. */
SAU_AMD_API bool sauAmd_loudness_filter(uint32_t srate, double out[10]);
/* 129, and the taps g in out[] when cap >= 129 (nothing is written when cap < 129; out may then be NULL). */
SAU_AMD_API size_t sauAmd_truepeak_taps(double *out, size_t cap);
/* The gating above over n_hops complete hops, hops[h][2] ([h][1] is not read for channels == 1), of hop_frames frames each:
 * blocks, gated_blocks, integrated and momentary_max; frames = n_hops * hop_frames and true_peak = 0. Public so that a caller
 * can gate windows of its own. False on channels other than 1 or 2, hop_frames == 0 or a NULL pointer. */
SAU_AMD_API bool sauAmd_loudness_gate(const double *hops /* [n_hops][2] */, size_t n_hops, uint32_t hop_frames, int channels,
		sauAmdLoudness *out);
/* Loudness metering is off by default, and while it is off a run does nothing for it. On: every sauAmd_Batch_run_f32 ends with
 * the device measuring stream i over the frames [0, out_len[i]) of that run -- on the batch's stream, before any copy to the
 * host -- into stream i's record on the device: hop energies (16 bytes per 100 ms, growing with the stream), filter state,
 * true peak, the 31-frame history, the frame count. Independent of sauAmd_Batch_set_metering; both may be on. While on,
 * sauAmd_Batch_run, sauAmd_Batch_run_decimated_f32, sauAmd_Batch_run_limited_f32 and a float run of the other channel layout than the record's are refused
 * as a bad argument: nothing is rendered and the batch stands where it stood. False (sauAmd_last_error), with nothing
 * changed, on a backend without it or a batch rate below 2560 Hz; switching it off always succeeds and keeps the records. */
SAU_AMD_API bool sauAmd_Batch_set_loudness(sauAmdBatch *b, int on);
/* Wait for the batch's stream, fetch hops, peaks and histories, gate, and cover the true-peak tail in the copy: one record per
 * stream. reset != 0 then clears hops, filter state, history, peaks and frame count. Empty records (-HUGE_VAL, zeros) while
 * loudness metering has never been on. */
SAU_AMD_API bool sauAmd_Batch_loudness(sauAmdBatch *b, sauAmdLoudness *out /* [streams] */, int reset);
/* The number of complete hops of a stream, and their energies out[h][2] when cap (in hops) suffices (nothing is written when
 * it does not; out may then be NULL). Waits for the batch's stream. */
SAU_AMD_API size_t sauAmd_Batch_loudness_hops(sauAmdBatch *b, size_t stream, double *out, size_t cap);
/* The same measurement, from zero state, of n_rows float32 rows the caller holds on the batch's device, at the rate srate
 * (>= 2560): the argument rules are sauAmd_Batch_measure_rows' (and frames must fit 32 bits). Synchronous; the batch's own
 * records are untouched. hops_out (may be NULL): the rows' frames / (srate / 10) complete hops each, [n_rows][hops][2], when
 * hops_cap (in doubles) suffices. frames == 0 gives empty records. */
SAU_AMD_API bool sauAmd_Batch_measure_loudness_rows(sauAmdBatch *b, const void *rows, size_t pitch_bytes, size_t n_rows,
		size_t frames, int channels, uint32_t srate, sauAmdLoudness *out /* [n_rows] */, double *hops_out, size_t hops_cap);
/* sauAmd_render_file to a target loudness under a true-peak ceiling. Rendered twice, as sauAmd_render_file_normalized is and on
 * the same call lattice: pass 1 makes float runs with loudness metering on and fetches nothing;
 *   gain = (float)pow(10.0, (target_lufs - integrated) / 20.0);
 *   if max(true_peak) * gain > max_true_peak (f32): gain = max_true_peak / max(true_peak), one f32 division;
 * gain = 1 when integrated is -HUGE_VAL; pass 2 writes x * gain through the same requantiser (the int16 formats round once,
 * after the gain). *loud_out (may be NULL) = pass 1's record, before the gain; *gain_out (may be NULL) = the gain. False
 * (sauAmd_last_error), before any file is created, on a bad argument -- a target that is not finite, max_true_peak not finite
 * or <= 0, srate < 2560 -- or a backend without float output or loudness metering. */
SAU_AMD_API bool sauAmd_render_file_loudness(const sauProgram *prg, uint32_t srate, const char *path, int format, int channels,
		double target_lufs, float max_true_peak, uint64_t *frames_out, sauAmdLoudness *loud_out, float *gain_out);

/* ---- Limiter -------------------------------------------------------------------
 * sauAmd_render_file_loudness lowers the gain of the whole file where true_peak * gain would pass the ceiling, so one loud
 * transient leaves a file several dB under the loudness asked for. A look-ahead true-peak limiter closes that gap: it lowers
 * the gain around the peaks only. It runs where the samples are, on the float rows of sauAmd_Batch_run_f32.
 *
 * The limiter is feed-forward and non-recursive: its output is a function of the input sequence only, never of how the
 * sequence is cut into runs, of tiles, or of the partition of the device. The arithmetic is a fixed order of IEEE operations
 * (the build is -ffp-contract=off), reproducible bit for bit.
 *
 * Constants, for the rate fs: look-ahead A = min(max(fs / 200, 16), 1024) frames (integer division: 5 ms, clamped); delay
 * D = 2 A + 16 frames; g[0 .. 128] the taps of sauAmd_truepeak_taps. Parameters: pre_gain g0 and ceiling c, floats, finite
 * and > 0. x[i][ch] is the stream's float sample of frame i, counted from the start of the limited sequence; a NaN or +-inf
 * counts as +0.0f; x is +0.0f for i < 0 and for every frame at or behind the stream's end.
 *  1. Interpolated points, the loudness section's: for p = 1, 2, 3: acc = +0.0; for q = 0 .. 31 ascending:
 *     acc = acc + g[4 q + p] * (double)x[m - q][ch]; w[m][p][ch] = (float)acc -- the point at time m - 16 + p / 4.
 *  2. Envelope, the channels linked: e[i] = the largest, compared as bit patterns, over ch and p, of |x[i][ch]|, every finite
 *     |w[i + 15][p][ch]| and every finite |w[i + 16][p][ch]|: the sample and the three points on either side of it.
 *  3. Required gain, f64: E = (double)e[i] * (double)g0 (exact); r[i] = 1.0 when E <= (double)c, else (double)c / E;
 *     s[i] = 1.0 - r[i].
 *  4. Hold: d[k] = max(s[k - A .. k + A]) -- exact, so any order of evaluation gives the same value.
 *  5. Smoothing window, f64 on the host: u[j] = 1.0 + cos(pi * (j - A) / (A + 1)) for j = 0 .. 2A, S the sum of u in
 *     ascending j, h[j] = u[j] / S (sauAmd_limiter_window).
 *  6. Gain: acc = +0.0; for j = 0 .. 2A ascending: acc = acc + h[j] * d[i - A + j]; G[i] = min(1.0 - acc, r[i]). Where
 *     nothing within +-2A frames needs reduction every d is +0.0 and G[i] is exactly 1.0.
 *  7. Output: y[i][ch] = (float)(((double)x[i][ch] * (double)g0) * G[i]); the int16 formats take pcm16(y), the kernels' own
 *     rounding, byte-swapped on the device for AU.
 * Two consequences. |y[i][ch]| <= c as floats, exactly: G <= r, both products round monotonically, and c (1 + 2^-52) rounds
 * to the float c. Where G[i] == 1.0, y is (float)((double)x * (double)g0): with g0 == 1 the untouched passages pass through
 * bit for bit.
 * The true peak of y -- the peaks between its samples -- is NOT bounded exactly: a gain that varies in time moves them.
 * Measured with the loudness section's interpolator on this arithmetic (noise, a faded quarter-rate sine at 45 degrees, a
 * 50 Hz sine and a 20x burst, each mono and stereo at 3200, 8000 and 44100 Hz, at 5 to 12 dB of reduction) the true peak of y passed c
 * by at most +0.0121 dB at 3200 Hz (noise, A = 16), +0.0007 dB at 8000 Hz and less than 0.00001 dB at 44100 Hz; a caller
 * that needs the ceiling held between the samples at a low rate leaves that margin under it.
 * Limiting lowers the integrated loudness slightly below the target of sauAmd_render_file_loudness_limited; no third pass
 * corrects it.
 * Limits: float runs only; decimated rows are not limited; limited rows are not loudness-metered; the release is the
 * symmetric window's, no longer. */
typedef struct sauAmdLimiterStats {
	uint64_t frames;    /* delivered output frames */
	uint64_t limited;   /* those of them with G < 1.0 */
	double   min_gain;  /* the smallest G delivered; 1.0 before any */
} sauAmdLimiterStats;
#ifdef __cplusplus
static_assert(sizeof(sauAmdLimiterStats) == 24, "sauAmdLimiterStats is 24 bytes");
#else
_Static_assert(sizeof(sauAmdLimiterStats) == 24, "sauAmdLimiterStats is 24 bytes");
#endif

/* sauAmd_limiter_window: 2 A + 1, and the window h in out[] when cap >= 2 A + 1 (nothing is written when cap is less; out may
 * then be NULL). sauAmd_limiter_latency: D. Both 0 for srate == 0. */
SAU_AMD_API size_t sauAmd_limiter_window(uint32_t srate, double *out, size_t cap);
SAU_AMD_API size_t sauAmd_limiter_latency(uint32_t srate);
/* A float run of buf_len frames, then the limiter on the batch's stream. Every stream's limited row -- and bufs[i] when given
 * (bufs may be NULL) -- holds buf_len valid frames: the sequence delayed by D, so that position P + n of the sequence holds
 * y[P + n - D] (y[i] = +0.0f for i < 0). The input is zero-extended behind the stream's end: a stream's tail therefore appears
 * in later runs, and a run after every stream has ended renders nothing and still delivers. more[i] and out_len[i] are the
 * float run's. The history belongs to a sequence of limited runs with the same (pre_gain, ceiling, stereo): a limited run
 * that follows any other kind of run, or one with another of the three, starts from zero history. Level metering, when on,
 * measures the float run as it does for a decimated run. False (sauAmd_last_error) with "bad argument" on parameters that are
 * not finite and positive, while loudness metering is on (see sauAmd_Batch_set_loudness), and on a backend without a limiter
 * or float output; nothing is rendered then and the batch stands where it stood. A batch that never makes a limited run
 * allocates and does nothing for it. */
SAU_AMD_API bool sauAmd_Batch_run_limited_f32(sauAmdBatch *b, float pre_gain, float ceiling, float *const *bufs, size_t buf_len,
		bool stereo, bool *more, size_t *out_len);
/* Device address of stream i's limited float row of the last limited run (NULL before one), and the bytes between the rows of
 * consecutive streams. The rows are 16-byte aligned and the pitch is a multiple of 256. Valid until the batch's next limited
 * run (call sauAmd_Batch_sync first: the run is asynchronous). */
SAU_AMD_API const float *sauAmd_Batch_device_limited_f32(sauAmdBatch *b, size_t stream);
SAU_AMD_API size_t sauAmd_Batch_device_limited_pitch(sauAmdBatch *b);
/* Wait for the batch's stream and fetch one record per stream: every frame the batch's limited runs have delivered since the
 * last reset, the D frames ahead of a sequence's first sample and the tail included. The records run on through the batch's
 * sequences; reset != 0 then clears them. Empty records (0, 0, 1.0) before any limited run. */
SAU_AMD_API bool sauAmd_Batch_limiter_stats(sauAmdBatch *b, sauAmdLimiterStats *out /* [streams] */, int reset);
/* The limiter from zero history on n_rows float32 rows the caller holds on the batch's device, at the rate srate (> 0):
 * out_rows[r] receives `frames` float frames, time-aligned -- out[i] = y[i], the delay dropped -- and stats_out[r] (may be
 * NULL) the row's record over those frames. The argument rules are sauAmd_Batch_measure_loudness_rows', for rows and for
 * out_rows alike (any rate above 0); output rows that overlap the input rows are refused. Synchronous; the batch's own
 * histories and records are untouched. frames == 0 gives empty records. */
SAU_AMD_API bool sauAmd_Batch_limit_rows(sauAmdBatch *b, const void *rows, size_t pitch_bytes, size_t n_rows, size_t frames,
		int channels, uint32_t srate, float pre_gain, float ceiling, void *out_rows, size_t out_pitch_bytes,
		sauAmdLimiterStats *stats_out /* [n_rows] */);
/* sauAmd_render_file_loudness with the limiter in place of the lowered gain. Pass 1 is the same; then
 *   gain = (float)pow(10.0, (target_lufs - integrated) / 20.0), never reduced for the ceiling (1 when integrated is -HUGE_VAL);
 * pass 2 makes the same runs on the same call lattice, each through the limiter with pre_gain = gain and ceiling =
 * max_true_peak into rows of the file's format; the first D frames are dropped and one last run of D frames behind the
 * program's end is made, so the file holds exactly the frames sauAmd_render_file writes. No sample of it exceeds
 * max_true_peak; its true peak may, by the gap stated above. Limiting lowers the integrated loudness slightly below the
 * target, and no third pass corrects it. *stats_out (may be NULL) is pass 2's record: it counts the D frames ahead of the
 * file's first and the rest of the last run behind its last too. The argument refusals are sauAmd_render_file_loudness',
 * before any file is created; so is that of a backend without float output, loudness metering or a limiter. */
SAU_AMD_API bool sauAmd_render_file_loudness_limited(const sauProgram *prg, uint32_t srate, const char *path, int format,
		int channels, double target_lufs, float max_true_peak, uint64_t *frames_out, sauAmdLoudness *loud_out, float *gain_out,
		sauAmdLimiterStats *stats_out);

/* ---- Spectrum -------------------------------------------------------------------
 * The oscillators are not band-limited (see "Oversampled rendering"): what did a factor buy, and does a script need one at
 * all? That takes a spectrum, and fetching every float sample for a host FFT is what the meters above exist to avoid. This is
 * a Welch / STFT power spectrum of float32 rows in f64, on the device. Unlike loudness and the limiter it is not tied to a
 * kind of run: it is a meter that is FED rows -- float rows, decimated rows, limited rows, a caller's own device rows alike.
 *
 * The arithmetic is a fixed order of IEEE operations (the build is -ffp-contract=off: every product is rounded, then the sum
 * or difference), reproducible bit for bit: no atomics, no sum whose order depends on scheduling, and the result is a function
 * of the fed sequence only, never of how it was cut into feeds or of the partition of the device.
 *
 * Parameters: log2n = L in 8 .. 12, N = 2^L; hop, an integer with N / 8 <= hop <= N; channels 1, or 2 interleaved.
 * Tables, in f64 on the host (sauAmd_spectrum_window, sauAmd_spectrum_twiddles; the device uses them as returned there):
 *   w[j] = 0.5 - 0.5 * cos(2.0 * pi * j / N), j = 0 .. N-1 (the periodic Hann window);
 *   T[k] = (c_k, d_k) = (cos(2.0 * pi * k / N), -sin(2.0 * pi * k / N)), k = 0 .. N/2 - 1.
 * A sample is the row's float converted to double; a NaN or +-inf counts as +0.0f.
 * Segments. A row counts its frames from 0. Segment s covers the frames [s hop, s hop + N) and exists once s hop + N <= P, P
 * the number of frames so far: S(P) = 0 for P < N, else (P - N) / hop + 1. Frames behind the last complete segment are
 * pending: they are not measured, and nothing is zero-extended.
 * One segment and channel, an in-place radix-2 decimation in time:
 *   for j = 0 .. N-1: re[rev_L(j)] = w[j] * (double)x[j]; im[rev_L(j)] = 0.0   (rev_L: the L-bit reversal)
 *   for stage t = 1 .. L, with m = 2^t, h = m / 2, st = N / m: for every k0 that is a multiple of m and j = 0 .. h-1, with
 *   a = k0 + j, b = a + h, (c, d) = T[j st]:
 *     tr = c * re[b] - d * im[b];  ti = c * im[b] + d * re[b];  ur = re[a];  ui = im[a];
 *     re[a] = ur + tr;  im[a] = ui + ti;  re[b] = ur - tr;  im[b] = ui - ti;
 *   p_s[k] = re[k] * re[k] + im[k] * im[k] for k = 0 .. N/2: two rounded products and one sum.
 * The butterflies of a stage are independent, so any distribution over lanes, and any fusion of consecutive stages in
 * registers that performs exactly these operations, gives these bits.
 * Averaging, in an order that does not depend on the device. Group g holds the segments [16 g, 16 g + 16):
 *   acc_g[k] = +0.0, then acc_g[k] = acc_g[k] + p_s[k] for the group's segments in ascending s;
 *   total[k] = +0.0, then total[k] = total[k] + acc_g[k] for every COMPLETE group in ascending g.
 * What is reported is the sum, not the mean, with S: the caller divides. When a record is read, the group at hand, if it
 * holds at least one segment, is added into the copy that is returned: total[k] + acc[k]; the device state is untouched and
 * later feeds continue exactly (the rule of the true-peak tail).
 * Limits: a feed whose groups' sums would take more than 1 GiB of scratch (rows * channels * groups * (N/2 + 1) * 8 bytes) is
 * refused as a bad argument; feed it in pieces -- the result is the same. At most 65535 rows per meter. */
typedef struct sauAmdSpectrum sauAmdSpectrum;

/* sauAmd_spectrum_window: N, and the window w in out[] when cap >= N (nothing is written when cap < N; out may then be NULL).
 * sauAmd_spectrum_twiddles: N, and the N doubles c_0 d_0 c_1 d_1 .. under the same rules. Both 0 for L outside 8 .. 12. */
SAU_AMD_API size_t sauAmd_spectrum_window(unsigned log2n, double *out, size_t cap);
SAU_AMD_API size_t sauAmd_spectrum_twiddles(unsigned log2n, double *out, size_t cap);
/* A meter of n_rows empty records on the batch's device and stream, independent of the batch's own runs and of every other
 * switch. NULL (sauAmd_last_error) on a bad argument -- L outside 8 .. 12, hop outside [N / 8, N], channels other than 1 or 2,
 * n_rows == 0 -- or on a backend without it. It must be destroyed before the batch. sauAmd_Spectrum_destroy(NULL) is allowed. */
SAU_AMD_API sauAmdSpectrum *sauAmd_Batch_create_spectrum(sauAmdBatch *b, size_t n_rows, int channels, unsigned log2n, uint32_t hop);
SAU_AMD_API void sauAmd_Spectrum_destroy(sauAmdSpectrum *s);
/* Row r's next frames[r] frames, read from rows + pitch_bytes * r; 0 changes nothing for that row. Queued on the batch's
 * stream: it may directly follow the run that produced the rows (sauAmd_Batch_device_pcm_f32, _device_decimated_f32,
 * _device_limited_f32), and the rows may be reused once the batch's stream has passed it. The argument rules are
 * sauAmd_Batch_measure_rows': `rows` and pitch_bytes multiples of 16, the rows -- as long as the longest frames[r] -- wholly
 * inside one allocation of that device. False with "bad argument" and nothing changed otherwise. */
SAU_AMD_API bool sauAmd_Spectrum_feed(sauAmdSpectrum *s, const void *rows, size_t pitch_bytes, const uint32_t *frames /* [n_rows] */);
/* Wait for the batch's stream and copy out the sums, the group at hand included, and S per row. reset != 0 then clears
 * position, pending frames and sums. */
SAU_AMD_API bool sauAmd_Spectrum_read(sauAmdSpectrum *s, double *power_out /* [n_rows][channels][N/2+1] */,
		uint64_t *segments_out /* [n_rows] */, int reset);
/* The same from empty records on n_rows rows of `frames` frames each, synchronous; the argument rules are
 * sauAmd_Batch_measure_loudness_rows'. spectrogram_out may be NULL; otherwise it receives every segment's (float)p_s[k] as
 * [n_rows][channels][S][N/2+1], and a spectrogram_cap (in floats) below that count is refused as a bad argument before
 * anything runs. frames == 0, or S == 0, gives zero sums. */
SAU_AMD_API bool sauAmd_Batch_spectrum_rows(sauAmdBatch *b, const void *rows, size_t pitch_bytes, size_t n_rows, size_t frames,
		int channels, unsigned log2n, uint32_t hop, double *power_out /* [n_rows][channels][N/2+1] */,
		uint64_t *segments_out /* [n_rows] */, float *spectrogram_out, size_t spectrogram_cap);
/* Render prg and measure it, fetching no sample. factor 1: the measured sequence is exactly the floats that
 * sauAmd_render_file(.., SAU_AMD_SNDFILE_WAV_F32, ..) writes (the same call lattice); factor 2, 4 or 8: exactly those that
 * sauAmd_render_file_oversampled writes (the filter's delay dropped, its tail kept). *frames_out (may be NULL) = the frames
 * measured. False (sauAmd_last_error) with "bad argument", before anything renders, on another factor, a bad L, hop or
 * channels, a NULL pointer or srate * factor beyond 32 bits; also on a backend without a spectrum meter, without float output,
 * or without a decimator where one is needed. */
SAU_AMD_API bool sauAmd_render_spectrum(const sauProgram *prg, uint32_t srate, int factor, int channels, unsigned log2n,
		uint32_t hop, double *power_out /* [channels][N/2+1] */, uint64_t *segments_out, uint64_t *frames_out);

/* ---- FLAC -----------------------------------------------------------------------
 * The meters above spare a fetch; when the audio itself is wanted, every sample still crosses to the host as PCM. This is a
 * lossless FLAC encoder for int16 rows where they are, on the batch's device. Like the spectrum meter it is FED rows: the rows
 * of an int16 run (sauAmd_Batch_device_pcm), or a caller's own. What comes back is a sequence of FLAC frames per row; with the
 * 42 bytes of sauAmd_flac_header ahead of them they are a FLAC file. The bytes are a function of the fed sequence only -- every
 * choice below is integer arithmetic with stated ties -- never of how the sequence was cut into feeds, of the partition of the
 * device or of scheduling. sauAmd_flac_encode_block restates one frame on the host, from the same source as the kernels.
 *
 * Parameters: channels 1, or 2 interleaved; 16 bits per sample; block_frames B one of 256, 512, 1024, 2048, 4096 (0 means
 * 4096). Row r's block k covers its frames [k B, k B + B) and becomes FLAC frame number k; frames behind the last complete block
 * are pending until a later feed completes the block or a finish makes them one last short block. At most 65535 rows per
 * encoder and 2^31 - 1 blocks per row.
 * Limits: MD5 only on request ("MD5" below), a decoder for these streams only ("Verify" below), no seek table, no comments, no wasted-bits detection, no escape
 * partitions, no dither of its own (a quantiser's rows can be fed: "Dither and noise shaping" below); LPC only on request (max_lpc_order, "The LPC mode" below), of order <= 8 with 12-bit coefficients, one
 * precision and one window. At 24 bits the LPC mode has entry points of its own, whose names end in _lpc24 ("LPC at 24 bits"
 * below); the entry points that take `bits` -- sauAmd_flac_encode_block_s32, sauAmd_Batch_create_flac_f32,
 * sauAmd_render_file_flac_f32, sauAmd_render_file_flac_loudness -- refuse max_lpc_order > 0 with bits == 24 as a bad argument,
 * as they always have. 24-bit output comes from float rows only ("24 bits" below). The
 * peak-normalised and oversampled writers have no FLAC variant; the fed encoders take any int16 or float device rows, decimated
 * ones included.
 *
 * All fields are big-endian and packed MSB first.
 * The header (42 bytes): "fLaC"; one metadata block header, 80 00 00 22 (last = 1, type 0, length 34); STREAMINFO:
 *   min blocksize 16 bits = B; max blocksize 16 = B; min framesize 24 and max framesize 24 from the record (0 before any
 *   frame); sample rate 20; channels - 1 in 3; bits per sample - 1 in 5 = 15; total samples 36 = the record's frames; MD5 128
 *   bits of zeros ("not computed"), or the digest ("MD5" below).
 * A frame's header:
 *   FF F8 (the sync code, reserved 0, fixed block size);
 *   4 bits block size code: 8 + log2(B / 256) for a block of B frames; 0111 for any other length n (also for n <= 256), and
 *     n - 1 then follows as 16 bits at the header's end;
 *   4 bits sample rate code 0000 (from STREAMINFO);
 *   4 bits channel assignment: 0000 mono; 0001 L, R; 1000 left, side; 1001 side, right; 1010 mid, side;
 *   3 bits sample size 100 (16 bits); one bit 0;
 *   the block's number within its row in the extended UTF-8 coding: below 0x80 one byte, the number itself; below 0x800 two
 *     bytes, lead 110xxxxx; below 0x10000 three, 1110xxxx; below 0x200000 four, 11110xxx; below 0x4000000 five, 111110xx; below
 *     2^31 six, 1111110x; continuation bytes 10xxxxxx, six bits each, the most significant first;
 *   the 16 bits of n - 1 when the code is 0111;
 *   CRC-8 of every header byte before it: polynomial 0x07, initial value 0, MSB first ("123456789" gives 0xF4).
 * A frame's body: the channels' subframes one after another, bit-contiguous; zero bits up to a byte boundary; CRC-16 of the
 * whole frame from the sync code on: polynomial 0x8005, initial value 0, MSB first, not reflected, high byte first
 * ("123456789" gives 0xFEE8).
 * A subframe: one 0 bit, 6 bits of type, one 0 bit (no wasted bits). bps is 16, or 17 for a side channel; samples are two's
 * complement in bps bits.
 *   000000 CONSTANT: one sample.  000001 VERBATIM: the n samples.  001ooo FIXED of order o = 0 .. 4: o warm-up samples, then
 *   the residual: 2 bits 00, 4 bits partition order p, and for each of the 2^p partitions a 4-bit Rice parameter k <= 14
 *   (never the escape 1111) and the partition's residuals. Partition 0 holds (n >> p) - o residuals, the others n >> p.
 *   A residual r: u = 2 r for r >= 0, else -2 r - 1; u >> k zero bits, a one bit, the low k bits of u.
 *   Residuals (integers that fit 32 bits): order 0: s_i; 1: s_i - s_{i-1}; 2: s_i - 2 s_{i-1} + s_{i-2};
 *   3: s_i - 3 s_{i-1} + 3 s_{i-2} - s_{i-3}; 4: s_i - 4 s_{i-1} + 6 s_{i-2} - 4 s_{i-3} + s_{i-4}.
 * Stereo: mid = (L + R) >> 1 (an arithmetic shift), side = L - R.
 * Choices, all in integers, ties to the first named. For a channel candidate of a block of n frames:
 *   1. all n samples equal: CONSTANT, 8 + bps bits.
 *   2. the order: 0 for n <= 4; otherwise the o in 0 .. 4 with the least sum of |r_i| of order o over i = 4 .. n-1 (in 64
 *      bits), the lowest o on ties.
 *   3. the partitions, with P = 4 for n == B and P = 0 otherwise: for p in 0 .. P and each partition, the cost of k is the sum
 *      of u >> k over its residuals + (1 + k) * their count; the k in 0 .. 14 with the least cost, the lowest on ties. The cost
 *      of p is the sum over its partitions of (4 + that least cost); the p with the least cost, the lowest on ties.
 *   4. FIXED costs 8 + bps * o + 6 + cost(p) bits, VERBATIM 8 + bps * n.
 *   5. VERBATIM when its cost is <= FIXED's, otherwise FIXED.
 * Mono encodes its one channel. Stereo evaluates L (16 bits), R (16), M (16), S (17), takes the least of L+R, L+S, S+R, M+S,
 * in that order on ties, and emits the two channels in the order named.
 * Consequences: a frame is at most 15 + channels * (1 + 2 n) bytes (13 header bytes, every channel verbatim, the CRC-16). A
 * sample's code places at most 15 non-zero bits; the unary zeros are what a cleared buffer holds.
 *
 * The LPC mode. A further parameter max_lpc_order M in 0 .. 8 (the entry points whose names end in _lpc); M = 0 is everything
 * above and nothing else. With M > 0 a channel candidate is also tried with a linear predictor when the block is a whole one
 * (n == B), the candidate is not constant and R[0] of step 2 is not 0; a short last block is encoded as with M = 0. The bytes stay
 * a function of the fed sequence and (B, channels, M) only: whatever is summed over the block is summed in integers, which is
 * exact and so free of any order, and the floating-point steps 4 and 5 are a short serial sequence of IEEE 754 binary64
 * operations in the order written, every product rounded before the sum it enters (no fused multiply-add). The coefficient
 * precision is 12 bits. >> is an arithmetic shift throughout. With Lg = log2 B:
 *   1. the window, W[j] = (B B - (2 j + 1 - B)^2) >> (2 Lg - 12) for j = 0 .. B-1 (a Welch window, 0 .. 4095), and the windowed
 *      samples ws[j] = (s[j] W[j]) >> 3, |ws| < 2^25.
 *   2. the autocorrelation R[l] = the sum over j = l .. n-1 of ws[j] ws[j - l], l = 0 .. M, in 64-bit integers (a product is
 *      below 2^50, a sum below 2^62).
 *   3. g is the least shift >= 0 with R[0] >> g < 2^53, and r[l] = (double)(R[l] >> g): |R[l]| <= R[0], so every conversion is
 *      exact.
 *   4. Levinson-Durbin: a[0 .. M-1] = 0, err = r[0]; for i = 0 .. M-1:
 *        acc = r[i + 1]; for j = 0 .. i-1 ascending: acc = acc + a[j] * r[i - j];
 *        k = -acc / err; a[i] = k;
 *        for j = 0 .. i/2 - 1 (i/2 rounded down): t = a[j]; u = a[i - 1 - j]; a[j] = t + k * u; a[i - 1 - j] = u + k * t;
 *        if i is odd: t = a[i/2]; a[i/2] = t + k * t;
 *        err = err * (1.0 - k * k);
 *        if !(err > 0.0) or err is not finite: stop -- neither order i + 1 nor a higher one is a candidate;
 *        otherwise order m = i + 1 has the coefficients c[j] = -a[j], j = 0 .. m-1: the prediction of s_i is the sum of
 *        c[j] s_{i-1-j}.
 *   5. the quantisation of order m: cmax = the largest |c[j]|; the order is no candidate when cmax is 0, subnormal or not
 *      finite. e is the integer with 2^(e-1) <= cmax < 2^e, read from cmax's exponent field (the field - 1022);
 *      shift = 11 - e; a shift above 15 becomes 15; with a shift below 0 the order is no candidate. E = 0.0, then for j
 *      ascending: E = E + c[j] * 2^shift (the scaling is exact); q[j] = floor(E + 0.5) clamped to -2048 .. 2047;
 *      E = E - (double)q[j].
 *   6. the residual of order m, r_i = s_i - ((the sum over j = 0 .. m-1 of q[j] s_{i-1-j}) >> shift) for i >= m. The sum is at
 *      most 8 * 2048 * 65535 < 2^30 in size and |r_i| < 2^31: everything fits 32 bits (17 + 12 + 3 = 32 is also what lets a
 *      decoder use 32-bit accumulators).
 *   7. the order: for each candidate order m, A_m = the sum of |r_i| over i = M .. n-1 (from M on whatever m is, in 64 bits) and
 *      est(m) = the least over k = 0 .. 14 of ((1 + k) (n - M) + ((2 A_m) >> k)), plus m (bps + 12). The m with the least est,
 *      the lowest on ties. No candidate order: no LPC for this channel candidate.
 *   8. the partitions: rule 3 above with o = m (P = 4; partition 0 holds (n >> p) - m residuals; the same costs and ties,
 *      k <= 14, never the escape).
 *   9. LPC costs 8 + bps * m + 4 + 5 + 12 * m + 6 + cost(p) bits, and rule 5 becomes: VERBATIM when its cost is <= both
 *      others'; otherwise FIXED when its cost is <= LPC's; otherwise LPC. The stereo rule is unchanged.
 *  10. the subframe (RFC 9639): one 0 bit, the type 1ooooo with ooooo = m - 1, one 0 bit; the m warm-up samples of bps bits;
 *      4 bits 1011 (the precision - 1); 5 bits shift, two's complement (never negative); the coefficients q[0] .. q[m-1] in
 *      that order -- q[0] belongs to the most recent sample --, 12 bits each, two's complement; then the residual exactly as
 *      in FIXED: 00, the partition order, the parameters, the codes.
 * A candidate's LPC subframe is taken only where it is cheaper, so no frame is longer than with M = 0; the frame bound holds
 * (VERBATIM still caps every channel), and so does "a sample's code places at most 15 non-zero bits". The streams stay inside
 * FLAC's streamable subset (order <= 12 at up to 48 kHz, Rice parameter <= 14).
 *
 * 24 bits. A float-fed encoder (sauAmd_Batch_create_flac_f32, sauAmd_Flac_feed_f32) quantises float rows on the device and
 * encodes the result; `bits` is 16 or 24. The quantiser: y = x * gain[row], one f32 multiply; a NaN becomes -1; y is clamped to
 * [-1, 1]; bits 16: the int16 the runs themselves store (the nearest integer to y * 32767 in f32, ties to even); bits 24: the
 * nearest integer to (double)y * 8388607.0, ties to even -- the product is exact in f64, so there is one rounding --, in
 * -8388607 .. 8388607. sauAmd_flac_quantize restates it on the host. With bits == 16 there is no new format: the stream is
 * exactly what the int16 encoder makes of those samples, max_lpc_order 0 .. 8 allowed. With bits == 24 everything of the 16-bit
 * text holds with these differences:
 *   STREAMINFO: bits per sample - 1 = 23. Frame header: sample size code 110.
 *   bps is 24, or 25 for a side channel. Samples are any value in -2^23 .. 2^23 - 1 (the quantiser makes only +-8388607).
 *   A FIXED residual is at most 16 * 2^24 = 2^28 in size and fits 32 bits; its u is below 2^30.
 *   The residual: 2 bits 01 (coding method 1), 4 bits partition order, and 5-bit Rice parameters k in 0 .. 30, never the escape
 *   11111.
 *   Rule 3: candidates k = 0 .. 30, the lowest on ties; a partition costs 5 + its least cost.
 *   Rule 4: FIXED costs 8 + bps * o + 6 + cost(p), VERBATIM 8 + bps * n, with those bps.
 *   Unchanged: P = 4 for whole blocks, the order rule (sums of |r| over i >= 4, in 64 bits), the stereo rule and every tie.
 *   A frame is at most 15 + channels * (1 + 3 n) bytes. A code's non-zero part is at most 31 bits: the stop bit and k low bits.
 *   No LPC through these entry points (Limits); "LPC at 24 bits" below has it.
 * sauAmd_flac_encode_block_s32 restates one such frame on the host. The bytes are a function of the fed floats, the gains and
 * (B, channels, bits, M) only, never of how the sequence was cut into feeds.
 *
 * LPC at 24 bits. The entry points whose names end in _lpc24 -- sauAmd_flac_encode_block_lpc24, sauAmd_Batch_create_flac_lpc24,
 * sauAmd_render_file_flac_lpc24, sauAmd_render_file_flac_loudness_lpc24 -- make 24-bit streams with max_lpc_order M in 0 .. 8;
 * M = 0 is "24 bits" above and nothing else, byte for byte and launch for launch. Everything in "The LPC mode", steps 1 to 10,
 * holds with bps 24, or 25 for a side channel, and with the 24-bit residual coding: method 01, 5-bit Rice parameters
 * k = 0 .. 30, a partition costing 5 plus its least cost. Whole blocks only, as at 16 bits. The differences:
 *   Step 1: ws[j] = (s[j] W[j]) >> 11, the product in 64-bit integers. |s| <= 2^24 and W <= 4095, so |ws| < 2^25 as at 16
 *     bits, and step 2's bounds (a product below 2^50, a sum below 2^62) stay as written.
 *   Step 5b (new), after the quantisation of order m: S = the sum of |q[j]| over j < m. The order is no candidate for this
 *     channel candidate when (S << (bps - 1)) >> shift >= 2^30, computed in 64-bit integers. This is the only place where the
 *     candidate orders depend on bps. It makes step 6 safe on every input: a prediction is at most that quantity + 1 in size,
 *     so |r_i| < 2^30 + 2^24 + 1 < 2^31 -- a residual fits int32, as RFC 9639 requires, and its u fits uint32. It fires at a
 *     sum of |c[j]| of about 64 for a side channel and 128 otherwise, far above what ordinary material gives.
 *   Step 6: the sum of q[j] s_{i-1-j} is in 64-bit integers (below 2^39 in size), >> shift is arithmetic on that, and the
 *     residual is then narrowed to 32 bits.
 *   Step 7: est's k runs over 0 .. 30; the order term is m (bps + 12) with these bps.
 *   Steps 8 to 10: rule 3 as in "24 bits" (k = 0 .. 30, 5 bits a parameter); the cost formula of step 9 is unchanged; the
 *     subframe is step 10's with its residual section in method 01: 01, the partition order, 5-bit parameters, the codes.
 * An LPC residual's u may take all 32 bits ("u is below 2^30" is said of FIXED only). A code's non-zero part is still at most
 * 31 bits, the stop bit and k <= 30 low bits, and the frame bound 15 + channels * (1 + 3 n) holds: LPC is taken only where it
 * is cheaper, so no frame is longer than with M = 0. The 16-bit rules have no step 5b and no other change.
 *
 * MD5. STREAMINFO's MD5 field is zeros unless it is asked for: sauAmd_Flac_set_md5 on a fed encoder, sauAmd_set_flac_file_md5
 * for the file writers. Off, every byte and every launch is what it is without this paragraph. On, the encoder keeps the MD5
 * (RFC 1321) of each row's unencoded samples (RFC 9639 section 8.2) on the device, where the samples are: the samples that the
 * analysis sees -- behind a float-fed encoder's quantiser, behind a dither quantiser upstream --, in stream order, channels
 * interleaved L, R whatever assignment the frames chose, each sample as a signed little-endian integer of 2 bytes (16 bits) or 3
 * bytes (24 bits). An empty stream has the digest of the empty message, d41d8cd98f00b204e9800998ecf8427e. It is 32-bit integer
 * arithmetic throughout: the digest is a function of the samples only, never of how the sequence was cut into feeds. A whole
 * block is a multiple of 64 bytes, so the running state of four words per row is all that is carried between feeds; a finish
 * hashes the short block, if there is one, and the padding, and leaves the 16 bytes, which sauAmd_Flac_md5 fetches.
 * sauAmd_flac_md5 restates it on the host, and sauAmd_flac_header_md5 writes the header with the field filled in.
 *
 * Verify. The library can read back what it writes: a strict decoder of exactly the frames stated above, and nothing else --
 * no variable block size, no other LPC precision or order, no escape partitions, no wasted bits, no third channel, no scan for a
 * sync code. sauAmd_flac_decode_block decodes one frame on the host; the same source decodes on the device. A frame is checked
 * in stream order and the first failure gives the status (SAU_AMD_FLAC_DEC_*):
 *   LENGTH    the data ends inside the frame (only the frame bound's bytes are ever looked at);
 *   SYNC      not FF F8;
 *   HEADER    a block size code that is neither 0111 nor B's, a sample rate code other than 0000, a channel assignment other
 *             than 0, 1, 8, 9, 10 or one that does not go with `channels`, a sample size code other than that of `bits`, the
 *             reserved bit, a code 0111 whose n is not below B;
 *   NUMBER    a frame number that is malformed, not in its shortest form, or not the expected one;
 *   CRC8      the header's CRC-8;
 *   SUBFRAME  a subframe's padding bit, a type other than CONSTANT, VERBATIM, FIXED 0 .. 4 (no order above n) or LPC 1 .. 8
 *             (only where n == B), the wasted-bits flag, an LPC precision field other than 1011 or a negative shift;
 *   RESIDUAL  a coding method other than the width's own, a partition order above 4 or above 0 in a short block, a Rice
 *             parameter above 14 (16 bits) or 30 (24 bits), the escape among them, a code whose u passes 32 bits;
 *   PADDING   a non-zero bit ahead of the byte boundary;
 *   CRC16     the frame's CRC-16;
 *   RANGE     a restored L or R beyond `bits`;
 *   MISMATCH  (verify only) the frame decoded, but not to the block's samples, length or size.
 * The inverses: r = (u >> 1) for an even u, -((u + 1) >> 1) for an odd one; a FIXED sample is its residual plus the
 * prediction the residual formula subtracts; an LPC sample is r_i + ((the sum of q[j] s_{i-1-j}) >> shift), the sum in 32 bits
 * at 16 bits per sample and in 64 at 24; left/side: R = L - S; side/right: L = S + R; mid/side: m = (M << 1) | (S & 1),
 * L = (m + S) >> 1, R = (m - S) >> 1.
 * The verify mode is off unless asked for: sauAmd_Flac_set_verify on a fed encoder, sauAmd_set_flac_file_verify for the file
 * writers. Off, every byte and every launch is what it is without this paragraph. On, every feed decodes each frame it made
 * where the encoder left it, on the device, behind the kernel that wrote it and ahead of the one that moves the pending
 * frames, and compares the result with the samples the analysis saw -- the fed rows and the pending frames; no PCM is fetched.
 * The expected frame number and length come from the feed's plan, not from what the analysis left. Per row the encoder keeps
 * the blocks checked, the bad ones, and the lowest bad block with its status (integer atomics: no order enters), which
 * sauAmd_Flac_verify fetches; a read with reset clears them, the setting stays. The encoded bytes are the same on or off.
 *
 * The worst case of a feed is that bound summed over the blocks it completes. Unread output lives on the device: a feed whose
 * worst case would bring the unread total above 1 GiB is refused; read first. (Until a read has fetched the frames' sizes, a
 * feed counts in that total with its worst case.) */
typedef struct sauAmdFlac sauAmdFlac;
typedef struct sauAmdFlacInfo {
	uint64_t frames;              /* sample frames encoded */
	uint64_t blocks;              /* FLAC frames made */
	uint64_t bytes;               /* their bytes */
	uint32_t min_frame_bytes, max_frame_bytes;   /* 0, 0 before the first */
} sauAmdFlacInfo;
#ifdef __cplusplus
static_assert(sizeof(sauAmdFlacInfo) == 32, "sauAmdFlacInfo is 32 bytes");
#else
_Static_assert(sizeof(sauAmdFlacInfo) == 32, "sauAmdFlacInfo is 32 bytes");
#endif

/* 42, and "fLaC", the metadata block header and STREAMINFO in out[] when cap >= 42 (nothing is written when cap < 42; out may
 * then be NULL). info may be NULL: an empty record. 0 for srate == 0 or > 655350, channels other than 1 or 2, a block_frames
 * that is not allowed. */
SAU_AMD_API size_t sauAmd_flac_header(uint32_t srate, int channels, uint32_t block_frames, const sauAmdFlacInfo *info, uint8_t *out, size_t cap);
/* The host restatement: one FLAC frame of n (1 .. block_frames) interleaved frames x, numbered frame_number (< 2^31), as the
 * device makes it. Returns its size; nothing is written when cap is less (out may then be NULL); 0 on a bad argument. */
SAU_AMD_API size_t sauAmd_flac_encode_block(const int16_t *x, uint32_t n, int channels, uint32_t block_frames, uint32_t frame_number,
		uint8_t *out, size_t cap);
/* ... with the LPC mode's max_lpc_order (0 .. 8; above 8 is a bad argument: 0). With 0 it is sauAmd_flac_encode_block. */
SAU_AMD_API size_t sauAmd_flac_encode_block_lpc(const int16_t *x, uint32_t n, int channels, uint32_t block_frames, uint32_t frame_number,
		uint32_t max_lpc_order, uint8_t *out, size_t cap);
/* An encoder of n_rows empty streams on the batch's device and stream, independent of the batch's own runs. NULL
 * (sauAmd_last_error) on a bad argument -- channels, block_frames, n_rows == 0 or above 65535 -- or on a backend without it. It
 * must be destroyed before the batch. sauAmd_Flac_destroy(NULL) is allowed. */
SAU_AMD_API sauAmdFlac *sauAmd_Batch_create_flac(sauAmdBatch *b, size_t n_rows, int channels, uint32_t block_frames);
/* ... whose streams are encoded in the LPC mode with max_lpc_order (0 .. 8; above 8 is a bad argument: NULL). With 0 it is
 * sauAmd_Batch_create_flac. */
SAU_AMD_API sauAmdFlac *sauAmd_Batch_create_flac_lpc(sauAmdBatch *b, size_t n_rows, int channels, uint32_t block_frames, uint32_t max_lpc_order);
SAU_AMD_API void sauAmd_Flac_destroy(sauAmdFlac *e);
/* Row r's next frames[r] frames, int16 in host order, `channels` interleaved, read from rows + pitch_bytes * r; 0 changes
 * nothing for that row. Queued on the batch's stream: it may directly follow the run that produced the rows
 * (sauAmd_Batch_device_pcm), and the rows may be reused once the batch's stream has passed it. The argument rules are
 * sauAmd_Spectrum_feed's. Every block the feed completes is encoded; the frames behind are pending on the device. finish != 0
 * encodes each row's pending frames, if there are any, as one last short block and closes the rows: a later feed is refused
 * until a read with reset != 0. False with "bad argument" and nothing changed otherwise -- also for a feed of more than 2^24
 * blocks (feed it in pieces: the bytes are the same) and for one that the 1 GiB rule above refuses. */
SAU_AMD_API bool sauAmd_Flac_feed(sauAmdFlac *e, const void *rows, size_t pitch_bytes, const uint32_t *frames /* [n_rows] */, int finish);
/* Wait for the batch's stream. bytes_out[r] = the encoded bytes of row r not yet read. With bufs != NULL every caps[r] must
 * suffice (bufs[r] may be NULL where row r has nothing unread): then the bytes are copied to bufs[r] and consumed; otherwise
 * false with "bad argument", and nothing is consumed or written. info_out (may be NULL) counts everything since the last
 * reset. reset != 0 then starts new streams at frame number 0: records, pending frames and whatever is still unread go. */
SAU_AMD_API bool sauAmd_Flac_read(sauAmdFlac *e, uint8_t *const *bufs, const size_t *caps, size_t *bytes_out /* [n_rows] */,
		sauAmdFlacInfo *info_out /* [n_rows], may be NULL */, int reset);
/* Render prg into a FLAC file: the same int16 runs on the same call lattice as sauAmd_render_file(.., SAU_AMD_SNDFILE_RAW, ..),
 * each run's device row fed where that writer fetches it, the last feed a finish; the encoded bytes go through the two
 * page-locked slots to the file while the next run renders, and the 42 header bytes are rewritten at the end with the final
 * record. Decoding the file gives exactly the samples sauAmd_render_file writes. *frames_out and *info_out may be NULL. False
 * (sauAmd_last_error) with "bad argument" on a NULL pointer, srate == 0 or > 655350, channels other than 1 or 2 or a
 * block_frames that is not allowed, and on a backend without an encoder -- all before any file is created. */
SAU_AMD_API bool sauAmd_render_file_flac(const sauProgram *prg, uint32_t srate, const char *path, int channels, uint32_t block_frames,
		uint64_t *frames_out, sauAmdFlacInfo *info_out);
/* ... in the LPC mode with max_lpc_order (0 .. 8; above 8 is a bad argument, refused before any file is created). With 0 it is
 * sauAmd_render_file_flac. The file decodes to the same samples and is never longer. */
SAU_AMD_API bool sauAmd_render_file_flac_lpc(const sauProgram *prg, uint32_t srate, const char *path, int channels, uint32_t block_frames,
		uint32_t max_lpc_order, uint64_t *frames_out, sauAmdFlacInfo *info_out);

/* ---- 24 bits and float-fed encoders ("24 bits" above) ---- */
/* sauAmd_flac_header with STREAMINFO's bits per sample: `bits` 16 (sauAmd_flac_header's bytes) or 24; anything else: 0. */
SAU_AMD_API size_t sauAmd_flac_header_bits(uint32_t srate, int channels, uint32_t block_frames, int bits, const sauAmdFlacInfo *info,
		uint8_t *out, size_t cap);
/* The host restatement for int32 samples. bits == 16: every sample must fit int16, and the bytes are
 * sauAmd_flac_encode_block_lpc's. bits == 24: every sample must lie in -2^23 .. 2^23 - 1, and this entry point refuses
 * max_lpc_order > 0 (sauAmd_flac_encode_block_lpc24 takes it). Otherwise, and for other bits, 0. */
SAU_AMD_API size_t sauAmd_flac_encode_block_s32(const int32_t *x, uint32_t n, int channels, uint32_t block_frames, uint32_t frame_number,
		int bits, uint32_t max_lpc_order, uint8_t *out, size_t cap);
/* The quantiser on the host: out[i] = what a float-fed encoder of `bits` makes of x[i] with `gain`. False for bits other than 16
 * or 24, or a NULL pointer with n > 0. */
SAU_AMD_API bool sauAmd_flac_quantize(const float *x, size_t n, float gain, int bits, int32_t *out);
/* MD5 (the text's "MD5"). sauAmd_Flac_set_md5: on != 0 turns an encoder's MD5 on, 0 off; allowed only while every stream stands
 * at its start -- nothing fed since creation or since the last read with reset --, otherwise false with "bad argument" and
 * nothing changed. The setting outlives resets, which put the running states back to MD5's initial value. sauAmd_Flac_md5: waits
 * for the batch's stream; out[n_rows][16] the rows' digests when MD5 is on and a finish has closed the rows (before a read with
 * reset), otherwise false with "bad argument" and nothing written. */
SAU_AMD_API bool sauAmd_Flac_set_md5(sauAmdFlac *e, int on);
SAU_AMD_API bool sauAmd_Flac_md5(sauAmdFlac *e, uint8_t *out /* [n_rows][16] */);
/* sauAmd_flac_header_bits's bytes with bytes 26 .. 41, the MD5 field, replaced by md5[16] (NULL: zeros). */
SAU_AMD_API size_t sauAmd_flac_header_md5(uint32_t srate, int channels, uint32_t block_frames, int bits, const sauAmdFlacInfo *info,
		const uint8_t md5[16], uint8_t *out, size_t cap);
/* The host restatement: the digest of n_samples interleaved samples of `bits` per sample. False for bits other than 16 or 24, a
 * sample that does not fit `bits`, or a NULL pointer (x with n_samples > 0, or out). */
SAU_AMD_API bool sauAmd_flac_md5(const int32_t *x, size_t n_samples, int bits, uint8_t out[16]);
/* The FLAC file writers' process-wide default (atomic; initially 0): returns the previous value. Every sauAmd_render_file_flac*
 * writer reads it once at entry. On, the writer turns its encoder's MD5 on, fetches the digest behind the last read and writes
 * it into the header it rewrites at the end; every other byte of the file is the same. A backend whose encoder has no MD5 then
 * gives "bad argument" before any file is created. Off, a writer does what it does without this switch. */
SAU_AMD_API int sauAmd_set_flac_file_md5(int on);
/* The decoder and the verify mode (the text's "Verify"). */
enum {
	SAU_AMD_FLAC_DEC_OK = 0, SAU_AMD_FLAC_DEC_LENGTH = 1, SAU_AMD_FLAC_DEC_SYNC = 2, SAU_AMD_FLAC_DEC_HEADER = 3,
	SAU_AMD_FLAC_DEC_NUMBER = 4, SAU_AMD_FLAC_DEC_CRC8 = 5, SAU_AMD_FLAC_DEC_SUBFRAME = 6, SAU_AMD_FLAC_DEC_RESIDUAL = 7,
	SAU_AMD_FLAC_DEC_PADDING = 8, SAU_AMD_FLAC_DEC_CRC16 = 9, SAU_AMD_FLAC_DEC_RANGE = 10, SAU_AMD_FLAC_DEC_MISMATCH = 11,
	SAU_AMD_FLAC_DEC_BAD_ARGUMENT = 255
};
/* The host restatement of the decoder: the one frame that begins at data, a frame of `channels`, block_frames and `bits` as the
 * encoders above make it, numbered frame_number. Returns the frame's size in bytes with *status_out == SAU_AMD_FLAC_DEC_OK,
 * *n_out its frames and out[n * channels] its samples, interleaved. Otherwise 0 with the status, *n_out == 0 and nothing
 * promised about out; a bad argument -- channels, block_frames, bits, a frame_number of 2^31 or more, a NULL pointer -- or
 * cap_frames < n gives 0 with SAU_AMD_FLAC_DEC_BAD_ARGUMENT. data[len] and beyond are never read. */
SAU_AMD_API size_t sauAmd_flac_decode_block(const uint8_t *data, size_t len, int channels, uint32_t block_frames, int bits,
		uint32_t frame_number, int32_t *out /* [cap_frames * channels], interleaved */, size_t cap_frames, uint32_t *n_out, int *status_out);
typedef struct sauAmdFlacVerify {
	uint64_t blocks;              /* frames decoded since the last reset */
	uint64_t bad_blocks;
	uint64_t first_bad_block;     /* valid when bad_blocks > 0 */
	uint32_t first_status, pad_;  /* SAU_AMD_FLAC_DEC_*; 0 when bad_blocks == 0 */
} sauAmdFlacVerify;
#ifdef __cplusplus
static_assert(sizeof(sauAmdFlacVerify) == 32, "sauAmdFlacVerify is 32 bytes");
#else
_Static_assert(sizeof(sauAmdFlacVerify) == 32, "sauAmdFlacVerify is 32 bytes");
#endif
/* sauAmd_Flac_set_verify: sauAmd_Flac_set_md5's rules -- only while every stream stands at its start, otherwise false with
 * "bad argument" and nothing changed; the setting outlives resets, which clear the records. sauAmd_Flac_verify: waits for the
 * batch's stream; out[n_rows] the rows' records; false with "bad argument" when verify is off. */
SAU_AMD_API bool sauAmd_Flac_set_verify(sauAmdFlac *e, int on);
SAU_AMD_API bool sauAmd_Flac_verify(sauAmdFlac *e, sauAmdFlacVerify *out /* [n_rows] */);
/* The FLAC file writers' process-wide default (atomic; initially 0): returns the previous value. Every sauAmd_render_file_flac*
 * writer reads it once at entry. On, the writer turns its encoder's verify on and fetches the record behind the last read; with
 * bad_blocks > 0 it returns false and sauAmd_last_error names the block and the status, the file closed as written, for
 * inspection. Every byte of the file is the same on or off. A backend whose encoder has no verify mode then gives "bad
 * argument" before any file is created. */
SAU_AMD_API int sauAmd_set_flac_file_verify(int on);
/* A float-fed encoder: sauAmd_Batch_create_flac_lpc's rules, and bits 16 or 24; this entry point refuses 24 with
 * max_lpc_order > 0 as a bad argument (sauAmd_Batch_create_flac_lpc24 takes it). */
SAU_AMD_API sauAmdFlac *sauAmd_Batch_create_flac_f32(sauAmdBatch *b, size_t n_rows, int channels, uint32_t block_frames, int bits,
		uint32_t max_lpc_order);
/* sauAmd_Flac_feed for a float-fed encoder: row r's next frames[r] float frames times gains[r] (gains NULL: 1.0f everywhere; a
 * gain that is not finite is a bad argument). rows and pitch_bytes must be multiples of 4 (not 16: a feed may begin anywhere in
 * a float row); otherwise the argument rules are sauAmd_Spectrum_feed's. The floats are quantised into rows of the encoder's own,
 * so the fed rows may be reused once the batch's stream has passed the feed. An encoder is of one kind: sauAmd_Flac_feed on a
 * float-fed encoder, and this on an int16-fed one, is a bad argument that changes nothing. sauAmd_Flac_read and
 * sauAmd_Flac_destroy serve both kinds. */
SAU_AMD_API bool sauAmd_Flac_feed_f32(sauAmdFlac *e, const void *rows, size_t pitch_bytes, const uint32_t *frames /* [n_rows] */,
		const float *gains /* [n_rows]; NULL: 1.0f */, int finish);
/* Render prg into a FLAC file of `bits` per sample from float runs: sauAmd_render_file_normalized's second pass with a
 * sauAmd_Flac_feed_f32 of the run's device row (gain `gain`) where that writer requantises and fetches; the file I/O is
 * sauAmd_render_file_flac's. The file decodes to the quantiser's values of x * gain for the floats x that
 * sauAmd_render_file(.., SAU_AMD_SNDFILE_WAV_F32, ..) writes. False with "bad argument" on what sauAmd_render_file_flac_lpc
 * refuses, bits other than 16 or 24, 24 with max_lpc_order > 0 (this writer refuses it; sauAmd_render_file_flac_lpc24 takes it), a
 * gain that is not finite, and on a backend without the encoder or float output -- all before any file is created. */
SAU_AMD_API bool sauAmd_render_file_flac_f32(const sauProgram *prg, uint32_t srate, const char *path, int channels, uint32_t block_frames,
		int bits, uint32_t max_lpc_order, float gain, uint64_t *frames_out, sauAmdFlacInfo *info_out);
/* The loudness-normalised writers with FLAC output. Pass 1 is sauAmd_render_file_loudness's. limited == 0: the gain follows that
 * writer's rule and pass 2 is sauAmd_render_file_flac_f32's with it. limited != 0: the gain follows
 * sauAmd_render_file_loudness_limited's rule, and pass 2 is that writer's with float limited rows fed with gain 1 -- the first D
 * frames skipped, the D-frame tail run fed too. Either way the file holds the samples the WAV_F32 variant of that writer holds,
 * quantised, and exactly as many frames. Refusals: those writers', and sauAmd_render_file_flac_f32's, all before any file is
 * created. The out pointers may be NULL; stats_out is written only when limited. */
SAU_AMD_API bool sauAmd_render_file_flac_loudness(const sauProgram *prg, uint32_t srate, const char *path, int channels,
		uint32_t block_frames, int bits, uint32_t max_lpc_order, double target_lufs, float max_true_peak, int limited,
		uint64_t *frames_out, sauAmdLoudness *loud_out, float *gain_out, sauAmdLimiterStats *stats_out, sauAmdFlacInfo *info_out);

/* ---- LPC at 24 bits (the paragraph of that name above) ---- */
/* The host restatement for int32 samples in -2^23 .. 2^23 - 1 with max_lpc_order 0 .. 8: sauAmd_flac_encode_block_s32's rules
 * for its other arguments, and with max_lpc_order 0 its bytes at bits == 24. 0 on a bad argument. */
SAU_AMD_API size_t sauAmd_flac_encode_block_lpc24(const int32_t *x, uint32_t n, int channels, uint32_t block_frames, uint32_t frame_number,
		uint32_t max_lpc_order, uint8_t *out, size_t cap);
/* A float-fed encoder of 24 bits per sample in the LPC mode with max_lpc_order (0 .. 8; above 8 is a bad argument: NULL). It is
 * fed with sauAmd_Flac_feed_f32, read with sauAmd_Flac_read, and sauAmd_Flac_set_md5, sauAmd_Flac_md5 and sauAmd_Flac_destroy
 * serve it too. With 0 it is sauAmd_Batch_create_flac_f32(.., 24, 0): the same bytes from the same launches. */
SAU_AMD_API sauAmdFlac *sauAmd_Batch_create_flac_lpc24(sauAmdBatch *b, size_t n_rows, int channels, uint32_t block_frames, uint32_t max_lpc_order);
/* sauAmd_render_file_flac_f32 at 24 bits with that encoder: the same refusals (max_lpc_order above 8 among them), all before any
 * file is created; sauAmd_set_flac_file_md5 applies. The file decodes to the same samples as with max_lpc_order 0, has as many
 * frames and none of them is longer. */
SAU_AMD_API bool sauAmd_render_file_flac_lpc24(const sauProgram *prg, uint32_t srate, const char *path, int channels, uint32_t block_frames,
		uint32_t max_lpc_order, float gain, uint64_t *frames_out, sauAmdFlacInfo *info_out);
/* sauAmd_render_file_flac_loudness at 24 bits with that encoder, both its variants: that writer's argument list without `bits`. */
SAU_AMD_API bool sauAmd_render_file_flac_loudness_lpc24(const sauProgram *prg, uint32_t srate, const char *path, int channels,
		uint32_t block_frames, uint32_t max_lpc_order, double target_lufs, float max_true_peak, int limited,
		uint64_t *frames_out, sauAmdLoudness *loud_out, float *gain_out, sauAmdLimiterStats *stats_out, sauAmdFlacInfo *info_out);

/* ---- Dither and noise shaping ------------------------------------------------------
 * A quantiser stage for 16-bit output: float device rows in, int16 device rows of its own out, with TPDF dither and
 * error-feedback noise shaping, reproducible bit for bit. Every other writer rounds pcm16(x * gain) bare: a tone below half an
 * LSB becomes zeros and a fade becomes harmonic distortion. With TPDF dither the error is noise that does not depend on the
 * signal, and a shaper moves that noise to where the ear is least sensitive.
 *
 * The spec: `dither` 0 (none) or 1 (TPDF); `taps` T = 0 .. 9 error-feedback coefficients coef[0 .. T), coef[0] on the most
 * recent error; `seed` of the dither. Valid when dither <= 1, taps <= 9, every used coefficient is finite and the sum of
 * |coef[j]| over the used taps is at most 64; anything else is a bad argument everywhere. The noise transfer function is
 * 1 - sum(coef[j] z^-(j+1)).
 *
 * The dither of row r, channel c (0 or 1), frame i -- counted from the stream's start in 64 bits, never per feed -- with all
 * integer arithmetic modulo 2^64:
 *     seed_r = seed + 0xD1B54A32D192ED03 r
 *     z = seed_r + 0x9E3779B97F4A7C15 (2 i + c + 1)
 *     z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  z = z ^ (z >> 31)
 *     d = (float)((int32)(z >> 40) - (int32)((z >> 16) & 0xFFFFFF)) * 2^-24
 * (splitmix64's output at a counter): exact, triangular on (-1, 1) LSB and a function of position only, so no result depends on
 * how a sequence is cut into feeds. Without dither d = 0.
 *
 * One sample: y = x * gain in one f32 multiply, a NaN becomes -1, y is clamped to [-1, 1], s = (double)y * 32767.0 (exact).
 * With e[j] the error j + 1 frames earlier on that channel of that row, zeros at the stream's start:
 *     t = +0.0;  for j = T-1 down to 1: t = t + coef[j] * e[j]
 *     w = T ? (s - t) - coef[0] * e[0] : s
 *     q = rint(w + (double)d)       (ties to even)
 *     e_new = q - w
 * in f64, every product rounded before the sum it enters. The error comes from the unclamped q, so |e| < 1.5 and |w - s| < 96;
 * the stored sample is q clamped to -32767 .. 32767, and a clamp that changes q is counted per channel. With dither 0 and
 * taps 0 the stored sample is exactly pcm16(y) = sauAmd_flac_quantize(x, gain, 16): such a quantiser reproduces the existing
 * writers' int16s.
 *
 * Dither and shaped noise are added after the gain, so a signal at full scale clips: at constant full scale with F9 (seed 7,
 * row 0) the quantiser clamps 902 of 2000 samples. The stats say how often it happened; the caller leaves headroom (the shaped sets'
 * noise reaches a few tens of LSB).
 *
 * Presets (dither 1): FLAT no taps; HP1 {1.0}; E3 {1.623, -0.982, 0.109}; E5 {2.033, -2.165, 1.959, -1.590, 0.6149};
 * F9 {2.412, -3.370, 3.937, -4.174, 3.353, -2.205, 1.281, -0.569, 0.0847}. E3, E5 and F9 are the published psychoacoustic sets
 * (PAPERS.md), designed for 44.1 kHz and accepted at any rate. E5's noise gain is 0.148 at DC and 9.36 at Nyquist.
 *
 * Out of scope: 24-bit dither, dither in the int16 runs of sauAmd_Batch_run, rate-specific shapers, a limited dithered writer. */
typedef struct sauAmdDither {
	uint64_t seed;
	uint32_t dither;   /* 0 none, 1 TPDF */
	uint32_t taps;     /* T, 0 .. 9 */
	double coef[9];
} sauAmdDither;
typedef struct sauAmdDitherStats {
	uint64_t frames;       /* fed since the last reset */
	uint64_t clipped[2];   /* per channel: samples the clamp to -32767 .. 32767 changed */
} sauAmdDitherStats;
enum { SAU_AMD_DITHER_FLAT = 0, SAU_AMD_DITHER_HP1 = 1, SAU_AMD_DITHER_E3 = 2, SAU_AMD_DITHER_E5 = 3, SAU_AMD_DITHER_F9 = 4 };
typedef struct sauAmdQuantizer sauAmdQuantizer;
/* *out = the preset `shape` with TPDF dither of `seed` (unused coefficients zero). False for any other shape or out == NULL. */
SAU_AMD_API bool sauAmd_dither_preset(int shape, uint64_t seed, sauAmdDither *out);
/* The host restatement, from the same source as the kernels: out = what a quantiser makes of frames [first_frame,
 * first_frame + frames) of its row `row`, `channels` interleaved. history: [channels][9] in and out, the errors 1 .. 9 frames
 * back (NULL: zeros, and nothing is handed back); a spec without taps leaves it alone. clipped (may be NULL) gets this call's
 * counts. False on an invalid spec, channels other than 1 or 2, a gain that is not finite, or a NULL x or out with frames > 0. */
SAU_AMD_API bool sauAmd_dither_quantize(const float *x, size_t frames, int channels, float gain, const sauAmdDither *spec, uint64_t row,
		uint64_t first_frame, double *history, int16_t *out, uint64_t clipped[2]);
/* A quantiser of n_rows streams (1 .. 65535) of 1 or 2 channels on the batch's device and stream, independent of the batch's
 * own runs. NULL (sauAmd_last_error) on a bad argument or on a backend without it. It must be destroyed before the batch.
 * sauAmd_Quantizer_destroy(NULL) is allowed. */
SAU_AMD_API sauAmdQuantizer *sauAmd_Batch_create_quantizer(sauAmdBatch *b, size_t n_rows, int channels, const sauAmdDither *spec);
SAU_AMD_API void sauAmd_Quantizer_destroy(sauAmdQuantizer *q);
/* Row r's next frames[r] float frames times gains[r] (NULL: 1.0f everywhere), read from rows + pitch_bytes * r, become the
 * first frames[r] frames of the quantiser's own row r. The argument rules are sauAmd_Flac_feed_f32's: rows and pitch_bytes
 * multiples of 4, the rows inside one allocation of the device, and a gain that is not finite is a bad argument that changes
 * nothing. Queued on the batch's stream: it may directly follow the run that produced the rows. A feed waits for nothing on
 * the host, except that one whose longest row is longer than that of every feed before it replaces the output rows with
 * larger ones, which waits for the device once (as a float-fed encoder's rows do). */
SAU_AMD_API bool sauAmd_Quantizer_feed(sauAmdQuantizer *q, const void *rows, size_t pitch_bytes, const uint32_t *frames /* [n_rows] */,
		const float *gains /* [n_rows]; NULL: 1.0f */);
/* The output rows: device address and pitch in bytes (NULL and 0 before the first feed with frames). The rows are 16-byte
 * aligned and in one allocation, the pitch is a multiple of 256, and they are valid until the next feed: they can go straight
 * into sauAmd_Flac_feed (int16-fed, every LPC order) or sauAmd_Batch_measure_rows on the same batch. */
SAU_AMD_API const int16_t *sauAmd_Quantizer_rows(sauAmdQuantizer *q);
SAU_AMD_API size_t sauAmd_Quantizer_pitch(sauAmdQuantizer *q);
/* Wait for the batch's stream, then copy the last feed's frames of row r to bufs[r] (may be NULL where that feed gave row r
 * no frames). */
SAU_AMD_API bool sauAmd_Quantizer_read(sauAmdQuantizer *q, int16_t *const *bufs /* [n_rows] */);
/* Wait for the batch's stream and report per row (out may be NULL). reset != 0 then restarts every stream at frame 0 with
 * zero history and zero counts. */
SAU_AMD_API bool sauAmd_Quantizer_stats(sauAmdQuantizer *q, sauAmdDitherStats *out /* [n_rows] */, int reset);
/* Render prg into a 16-bit file through a quantiser: sauAmd_render_file_normalized's second pass with a sauAmd_Quantizer_feed
 * of the run's device row (gain `gain`, row 0, the frames counted through the whole file) where that writer requantises; the
 * int16s go through the two page-locked slots to the file. format is RAW, AU (the same values big-endian) or WAV;
 * SAU_AMD_SNDFILE_WAV_F32 is a bad argument. Headers and frame counts are sauAmd_render_file's, and the samples are
 * sauAmd_dither_quantize's of the floats sauAmd_render_file(.., SAU_AMD_SNDFILE_WAV_F32, ..) writes. The out pointers may be
 * NULL. False with "bad argument" on a NULL pointer, channels other than 1 or 2, such a format, an invalid spec or a gain that
 * is not finite, and on a backend without the quantiser or float output -- all before any file is created. */
SAU_AMD_API bool sauAmd_render_file_dithered(const sauProgram *prg, uint32_t srate, const char *path, int format, int channels,
		float gain, const sauAmdDither *spec, uint64_t *frames_out, sauAmdDitherStats *stats_out);
/* ... into a 16-bit FLAC file: the float runs go through the quantiser into an int16-fed encoder of one stream
 * (sauAmd_Batch_create_flac_lpc's parameters); the file I/O is sauAmd_render_file_flac's. The file decodes to the samples
 * sauAmd_render_file_dithered writes. Refusals: that writer's and sauAmd_render_file_flac_lpc's, all before any file is created. */
SAU_AMD_API bool sauAmd_render_file_flac_dithered(const sauProgram *prg, uint32_t srate, const char *path, int channels,
		uint32_t block_frames, uint32_t max_lpc_order, float gain, const sauAmdDither *spec, uint64_t *frames_out,
		sauAmdFlacInfo *info_out, sauAmdDitherStats *stats_out);
/* The loudness-normalised writer through a quantiser: pass 1 and the gain rule are sauAmd_render_file_loudness's, pass 2 is
 * sauAmd_render_file_dithered's with that gain. Refusals: those two writers', all before any file is created. */
SAU_AMD_API bool sauAmd_render_file_loudness_dithered(const sauProgram *prg, uint32_t srate, const char *path, int format, int channels,
		double target_lufs, float max_true_peak, const sauAmdDither *spec, uint64_t *frames_out, sauAmdLoudness *loud_out,
		float *gain_out, sauAmdDitherStats *stats_out);

#ifdef __cplusplus
}
#endif
#endif /* SAUGNS_AMD_H */
