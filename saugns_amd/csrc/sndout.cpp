/* sndout.cpp -- output stage: render a program straight into a sound file.
 *
 * Row f-2 of SURVEY.md section 8: the reference writes finished PCM with
 * player/sndfile.c (AU header 63-72 + size update 74-80, WAV header 82-99 +
 * size update 101-109, in-place byte swap for AU 160-168, fwrite 179-187) from
 * Player_run's synchronous chunk loop (saugns.c:589-618). Here the generator
 * produces the file's byte order on the device, and finished chunks travel to
 * page-locked memory and to the file while the next chunk renders.
 * Files are byte-identical to the reference writer's for the same PCM,
 * including its AU quirk of storing the frame count in the size field.
 * SAU_AMD_SNDFILE_WAV_F32 has no counterpart there: the mixers' float32 samples
 * (Engine::run_f32) as a WAVE_FORMAT_IEEE_FLOAT file, through the same stage.
 */
#include "../../include/saugns_amd.h"
#include "engine.h"
#include "hip_backend.h"
#include "capi_internal.h"
#include <float.h>
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <atomic>
#include <exception>
#include <string>

using sauengine::Backend;
using sauengine::Engine;

namespace {

void put_le16(FILE *f, uint16_t v) { putc(v & 0xff, f); putc((v >> 8) & 0xff, f); }
void put_le32(FILE *f, uint32_t v) { put_le16(f, (uint16_t)(v & 0xffff)); put_le16(f, (uint16_t)(v >> 16)); }
void put_be32(FILE *f, uint32_t v) {
	putc((v >> 24) & 0xff, f); putc((v >> 16) & 0xff, f); putc((v >> 8) & 0xff, f); putc(v & 0xff, f);
}

struct SndOut {
	FILE *f = nullptr;
	int format = SAU_AMD_SNDFILE_RAW;
	uint16_t channels = 1;
	uint64_t frames = 0;

	bool open(const char *path, int fmt, uint16_t ch, uint32_t srate) {
		f = fopen(path, "wb");
		if (!f) return false;
		format = fmt; channels = ch; frames = 0;
		if (fmt == SAU_AMD_SNDFILE_AU) { /* player/sndfile.c:63-72 */
			fputs(".snd", f);
			put_be32(f, 28);
			put_be32(f, 0xffffffffu); /* size: unspecified until closed */
			put_be32(f, 3);           /* 16-bit linear PCM */
			put_be32(f, srate);
			put_be32(f, ch);
			put_be32(f, 0);
		} else if (fmt == SAU_AMD_SNDFILE_WAV) { /* player/sndfile.c:82-99 */
			fputs("RIFF", f);
			put_le32(f, 36);
			fputs("WAVE", f);
			fputs("fmt ", f);
			put_le32(f, 16);
			put_le16(f, 1);
			put_le16(f, ch);
			put_le32(f, srate);
			put_le32(f, (uint32_t)ch * srate * 2);
			put_le16(f, (uint16_t)(ch * 2));
			put_le16(f, 16);
			fputs("data", f);
			put_le32(f, 0);
		} else if (fmt == SAU_AMD_SNDFILE_WAV_F32) {
			/* a non-PCM format: the `fmt ` chunk carries cbSize, and a `fact` chunk the frame count */
			fputs("RIFF", f);
			put_le32(f, 50);
			fputs("WAVE", f);
			fputs("fmt ", f);
			put_le32(f, 18);
			put_le16(f, 3); /* WAVE_FORMAT_IEEE_FLOAT */
			put_le16(f, ch);
			put_le32(f, srate);
			put_le32(f, (uint32_t)ch * srate * 4);
			put_le16(f, (uint16_t)(ch * 4));
			put_le16(f, 32);
			put_le16(f, 0); /* cbSize */
			fputs("fact", f);
			put_le32(f, 4);
			put_le32(f, 0);
			fputs("data", f);
			put_le32(f, 0);
		}
		return true;
	}
	size_t sample_bytes() const { return format == SAU_AMD_SNDFILE_WAV_F32 ? 4 : 2; }
	bool write(const void *buf, size_t n_frames) {
		size_t w = fwrite(buf, (size_t)channels * sample_bytes(), n_frames, f);
		frames += w;
		return w == n_frames;
	}
	int close() {
		if (!f) return 0;
		if (format == SAU_AMD_SNDFILE_AU) { /* player/sndfile.c:74-80 */
			if (frames < UINT32_MAX) { fseek(f, 8, SEEK_SET); put_be32(f, (uint32_t)frames); }
		} else if (format == SAU_AMD_SNDFILE_WAV) { /* player/sndfile.c:101-109 */
			uint32_t bytes = (uint32_t)(channels * frames * 2);
			fseek(f, 4, SEEK_SET);
			put_le32(f, 36 + bytes);
			fseek(f, 32, SEEK_CUR);
			put_le32(f, bytes);
		} else if (format == SAU_AMD_SNDFILE_WAV_F32) {
			uint32_t bytes = (uint32_t)(channels * frames * 4);
			fseek(f, 4, SEEK_SET);
			put_le32(f, 50 + bytes);
			fseek(f, 46, SEEK_SET);
			put_le32(f, (uint32_t)frames);
			fseek(f, 54, SEEK_SET);
			put_le32(f, bytes);
		}
		int err = ferror(f);
		fclose(f);
		f = nullptr;
		return err;
	}
};

thread_local std::string g_file_error;

bool render_file_over(const sauProgram *prg, uint32_t srate, const char *path, int format,
		int channels, Backend *backend /* owned */, uint64_t *frames_out, std::string &err) {
	if (!prg || !path || (channels != 1 && channels != 2) || format < 0 || format > SAU_AMD_SNDFILE_WAV_F32) {
		err = "bad argument";
		delete backend;
		return false;
	}
	Engine *engine = Engine::create(&prg, 1, srate, backend, err);
	if (!engine) return false;
	const bool stereo = channels == 2;
	const bool f32 = format == SAU_AMD_SNDFILE_WAV_F32;
	engine->set_pcm_byteswap(format == SAU_AMD_SNDFILE_AU);
	/* (a backend without float output says so before there is a file) */
	if (f32 && !engine->set_format(sauengine::SF_F32, err)) { delete engine; return false; }
	/* Player_run asks the generator for 256 ms at a time (saugns.c:471,526: ch_len); the
	 * reference's block lattice restarts at each of those calls, so a device run covers whole ones */
	size_t call = (size_t)((uint64_t)256 * srate / 1000);
	if (call == 0) call = 1;
	engine->set_call_len(call);
	const size_t chunk = call >= 176400 ? call : 176400 / call * call; /* frames per device run */
	const size_t bytes = chunk * (size_t)channels * (f32 ? sizeof(float) : sizeof(int16_t));
	void *host[2] = {backend->alloc_host(bytes), backend->alloc_host(bytes)};
	SndOut out;
	bool ok = host[0] && host[1];
	if (!ok) err = "out of page-locked memory";
	if (ok && !out.open(path, format, (uint16_t)channels, srate)) {
		err = std::string("couldn't open \"") + path + "\" for writing";
		ok = false;
	}
	size_t pending[2] = {0, 0};
	int slot = 0;
	bool more = ok;
	while (ok && more) {
		size_t len = 0;
		/* PCM stays on the device; the copy below queues behind the mixer */
		ok = f32 ? engine->run_f32(nullptr, chunk, stereo, &more, &len, err) : engine->run(nullptr, chunk, stereo, &more, &len, err);
		if (!ok) break;
		if (len) {
			ok = f32 ? backend->fetch_pcm_f32_async(0, (float *)host[slot], (uint32_t)len, stereo, slot, err)
			         : backend->fetch_pcm_async(0, (int16_t *)host[slot], (uint32_t)len, stereo, slot, err);
			pending[slot] = len;
		}
		/* while this chunk renders and copies, the previous one goes to the file */
		const int other = slot ^ 1;
		if (ok && pending[other]) {
			ok = backend->wait_fetch(other, err);
			if (ok && !out.write(host[other], pending[other])) { err = "write failed"; ok = false; }
			pending[other] = 0;
		}
		slot = other;
	}
	for (int s = 0; ok && s < 2; ++s) { /* oldest first: `slot` is the older of the two */
		const int k = slot ^ s;
		if (pending[k]) {
			ok = backend->wait_fetch(k, err);
			if (ok && !out.write(host[k], pending[k])) { err = "write failed"; ok = false; }
			pending[k] = 0;
		}
	}
	(void)backend->sync(err);
	if (out.f && out.close() != 0 && ok) { err = "write failed"; ok = false; }
	if (frames_out) *frames_out = out.frames;
	backend->free_host(host[0]);
	backend->free_host(host[1]);
	delete engine; /* owns the backend */
	return ok;
}

/* Player_run's call size and the frames per device run that sauAmd_render_file uses (above): both passes of the normalised
 * writer render on the same lattice, so they -- and sauAmd_render_file -- compute the same samples */
void file_lattice(uint32_t srate, size_t &call, size_t &chunk) {
	call = (size_t)((uint64_t)256 * srate / 1000);
	if (call == 0) call = 1;
	chunk = call >= 176400 ? call : 176400 / call * call;
}

/* Pass 1 of the normalised writer: the whole program in float runs with metering on, nothing fetched -> its record.
 * Every refusal of a backend without float output or metering happens here, before there is a file. */
bool measure_program(const sauProgram *prg, uint32_t srate, bool stereo, Backend *backend /* owned */, sauengine::Levels &lv,
		std::string &err) {
	Engine *engine = Engine::create(&prg, 1, srate, backend, err);
	if (!engine) return false;
	size_t call, chunk;
	file_lattice(srate, call, chunk);
	engine->set_call_len(call);
	bool ok = engine->set_format(sauengine::SF_F32, err) && engine->set_metering(true, err);
	bool more = ok;
	while (ok && more) {
		size_t len = 0;
		ok = engine->run_f32(nullptr, chunk, stereo, &more, &len, err);
	}
	ok = ok && engine->levels(&lv, false, err);
	delete engine; /* owns the backend */
	return ok;
}

/* Pass 1 of the loudness-normalised writer: the same runs with loudness metering on, nothing fetched -> the program's record.
 * Every refusal of a backend without float output or loudness metering happens here, before there is a file. */
bool measure_program_loudness(const sauProgram *prg, uint32_t srate, bool stereo, Backend *backend /* owned */, sauengine::Loudness &ld,
		std::string &err) {
	Engine *engine = Engine::create(&prg, 1, srate, backend, err);
	if (!engine) return false;
	size_t call, chunk;
	file_lattice(srate, call, chunk);
	engine->set_call_len(call);
	bool ok = engine->set_format(sauengine::SF_F32, err) && engine->set_loudness(true, err);
	bool more = ok;
	while (ok && more) {
		size_t len = 0;
		ok = engine->run_f32(nullptr, chunk, stereo, &more, &len, err);
	}
	ok = ok && engine->loudness(&ld, false, err);
	delete engine; /* owns the backend */
	return ok;
}

/* Pass 2: the same runs on a fresh engine, each through requant_kernel into a device buffer of its own and from there
 * through the two page-locked slots to the file, as render_file_over's chunks go. */
bool write_scaled(const sauProgram *prg, uint32_t srate, const char *path, int format, int channels, float gain,
		Backend *backend /* owned */, uint64_t *frames_out, std::string &err) {
	Engine *engine = Engine::create(&prg, 1, srate, backend, err);
	if (!engine) return false;
	const bool stereo = channels == 2;
	const bool f32 = format == SAU_AMD_SNDFILE_WAV_F32;
	const sauengine::SampleFormat out_fmt = f32 ? sauengine::SF_F32 : sauengine::SF_S16;
	size_t call, chunk;
	file_lattice(srate, call, chunk);
	engine->set_call_len(call);
	if (!engine->set_format(sauengine::SF_F32, err)) { delete engine; return false; }
	const size_t frame_bytes = (size_t)channels * (f32 ? sizeof(float) : sizeof(int16_t));
	void *host[2] = {backend->alloc_host(chunk * frame_bytes), backend->alloc_host(chunk * frame_bytes)};
	SndOut out;
	bool ok = host[0] && host[1];
	if (!ok) err = "out of page-locked memory";
	if (ok && !out.open(path, format, (uint16_t)channels, srate)) {
		err = std::string("couldn't open \"") + path + "\" for writing";
		ok = false;
	}
	size_t pending[2] = {0, 0};
	int slot = 0;
	bool more = ok;
	while (ok && more) {
		size_t len = 0;
		ok = engine->run_f32(nullptr, chunk, stereo, &more, &len, err);
		if (!ok) break;
		if (len) {
			/* (the rounding happens here, once, after the gain; AU files get their byte order here too) */
			ok = backend->requantize(0, (uint32_t)len, stereo, gain, out_fmt, format == SAU_AMD_SNDFILE_AU, err) &&
			     backend->fetch_requant_async(host[slot], len * frame_bytes, slot, err);
			pending[slot] = len;
		}
		const int other = slot ^ 1;
		if (ok && pending[other]) {
			ok = backend->wait_fetch(other, err);
			if (ok && !out.write(host[other], pending[other])) { err = "write failed"; ok = false; }
			pending[other] = 0;
		}
		slot = other;
	}
	for (int s = 0; ok && s < 2; ++s) { /* oldest first */
		const int k = slot ^ s;
		if (pending[k]) {
			ok = backend->wait_fetch(k, err);
			if (ok && !out.write(host[k], pending[k])) { err = "write failed"; ok = false; }
			pending[k] = 0;
		}
	}
	{ std::string e2; (void)backend->sync(e2); }
	if (out.f && out.close() != 0 && ok) { err = "write failed"; ok = false; }
	if (frames_out) *frames_out = out.frames;
	backend->free_host(host[0]);
	backend->free_host(host[1]);
	delete engine;
	return ok;
}

/* The oversampled writer: float runs at srate * factor on render_file_over's lattice for that rate, each decimated on the
 * device (Engine::run_decimated) into rows of the file's format, and those through the two page-locked slots to the file, as
 * write_scaled's chunks go. The filter delays by H = decimator_latency output frames: with y the decimated runs end to end
 * and N the high-rate frames rendered, the file is y[H .. H + ceil(N / factor)) -- time-aligned with the input -- and one
 * last decimated run of H frames behind the program's end delivers what of it the runs so far have not. */
bool write_oversampled(const sauProgram *prg, uint32_t srate, int factor, const char *path, int format, int channels,
		Backend *backend /* owned */, uint64_t *frames_out, std::string &err) {
	const uint32_t srate_hi = srate * (uint32_t)factor;
	Engine *engine = Engine::create(&prg, 1, srate_hi, backend, err);
	if (!engine) return false;
	const bool stereo = channels == 2;
	const bool f32 = format == SAU_AMD_SNDFILE_WAV_F32;
	const sauengine::SampleFormat out_fmt = f32 ? sauengine::SF_F32 : sauengine::SF_S16;
	const bool swap = format == SAU_AMD_SNDFILE_AU;
	const size_t H = sauengine::decimator_latency(factor);
	size_t call, chunk;
	file_lattice(srate_hi, call, chunk); /* a device run is chunk * factor high-rate frames: whole calls, and `chunk` output frames */
	engine->set_call_len(call);
	/* a backend without float output or without a decimator says so here, before there is a file */
	if (!engine->set_format(sauengine::SF_F32, err) || !engine->begin_decimated(factor, stereo, err)) { delete engine; return false; }
	const size_t frame_bytes = (size_t)channels * (f32 ? sizeof(float) : sizeof(int16_t));
	const size_t slot_frames = chunk > H ? chunk : H;
	void *host[2] = {backend->alloc_host(slot_frames * frame_bytes), backend->alloc_host(slot_frames * frame_bytes)};
	SndOut out;
	bool ok = host[0] && host[1];
	if (!ok) err = "out of page-locked memory";
	if (ok && !out.open(path, format, (uint16_t)channels, srate)) {
		err = std::string("couldn't open \"") + path + "\" for writing";
		ok = false;
	}
	size_t pending[2] = {0, 0}, first[2] = {0, 0}; /* frames of the slot to write, and where they begin in it */
	int slot = 0;
	bool more = ok, tail = false;
	uint64_t y_pos = 0, wanted = 0; /* decimated frames made so far; ceil(N / factor) of the N high-rate frames rendered so far */
	while (ok && !tail) {
		tail = !more; /* behind the program's end: the one run for the filter's tail */
		const size_t n = tail ? H : chunk;
		size_t len = 0;
		ok = engine->run_decimated(nullptr, out_fmt, swap, factor, n, stereo, &more, &len, err);
		if (!ok) break;
		wanted += len; /* (every run but the program's last is whole: the ceilings add up to the ceiling of the sum) */
		/* the file is y[H, H + wanted): while the program runs that covers every frame of a run but the first H */
		const uint64_t lo = y_pos > H ? y_pos : H, end = y_pos + n, hi = H + wanted < end ? H + wanted : end;
		if (hi > lo) {
			ok = backend->fetch_decimated_async(0, host[slot], (size_t)(hi - y_pos) * frame_bytes, slot, err);
			first[slot] = (size_t)(lo - y_pos);
			pending[slot] = (size_t)(hi - lo);
		}
		y_pos = end;
		const int other = slot ^ 1;
		if (ok && pending[other]) {
			ok = backend->wait_fetch(other, err);
			if (ok && !out.write((const char *)host[other] + first[other] * frame_bytes, pending[other])) { err = "write failed"; ok = false; }
			pending[other] = 0;
		}
		slot = other;
	}
	for (int s = 0; ok && s < 2; ++s) { /* oldest first */
		const int k = slot ^ s;
		if (pending[k]) {
			ok = backend->wait_fetch(k, err);
			if (ok && !out.write((const char *)host[k] + first[k] * frame_bytes, pending[k])) { err = "write failed"; ok = false; }
			pending[k] = 0;
		}
	}
	{ std::string e2; (void)backend->sync(e2); }
	if (out.f && out.close() != 0 && ok) { err = "write failed"; ok = false; }
	if (frames_out) *frames_out = out.frames;
	backend->free_host(host[0]);
	backend->free_host(host[1]);
	delete engine;
	return ok;
}

/* The limited writer: float runs on render_file_over's lattice, each through the limiter (Engine::run_limited) into rows of
 * the file's format, and those through the two page-locked slots to the file, as write_oversampled's go. The limiter delays by
 * D = limiter_latency frames: with y the limited runs end to end and N the frames rendered, the file is y[D .. D + N) --
 * time-aligned with the input -- and one last run of D frames behind the program's end delivers what of it the runs so far
 * have not. */
bool write_limited(const sauProgram *prg, uint32_t srate, const char *path, int format, int channels, float pre_gain, float ceiling,
		Backend *backend /* owned */, uint64_t *frames_out, sauengine::LimiterStats *stats_out, std::string &err) {
	Engine *engine = Engine::create(&prg, 1, srate, backend, err);
	if (!engine) return false;
	const bool stereo = channels == 2;
	const bool f32 = format == SAU_AMD_SNDFILE_WAV_F32;
	const sauengine::SampleFormat out_fmt = f32 ? sauengine::SF_F32 : sauengine::SF_S16;
	const bool swap = format == SAU_AMD_SNDFILE_AU;
	const size_t D = sauengine::limiter_latency(srate);
	size_t call, chunk;
	file_lattice(srate, call, chunk);
	engine->set_call_len(call);
	/* a backend without float output or without a limiter says so here, before there is a file */
	if (!engine->set_format(sauengine::SF_F32, err) || !engine->begin_limited(pre_gain, ceiling, stereo, err)) { delete engine; return false; }
	const size_t frame_bytes = (size_t)channels * (f32 ? sizeof(float) : sizeof(int16_t));
	const size_t slot_frames = chunk > D ? chunk : D;
	void *host[2] = {backend->alloc_host(slot_frames * frame_bytes), backend->alloc_host(slot_frames * frame_bytes)};
	SndOut out;
	bool ok = host[0] && host[1];
	if (!ok) err = "out of page-locked memory";
	if (ok && !out.open(path, format, (uint16_t)channels, srate)) {
		err = std::string("couldn't open \"") + path + "\" for writing";
		ok = false;
	}
	size_t pending[2] = {0, 0}, first[2] = {0, 0}; /* frames of the slot to write, and where they begin in it */
	int slot = 0;
	bool more = ok, tail = false;
	uint64_t y_pos = 0, wanted = 0; /* limited frames made so far; the N frames rendered so far */
	while (ok && !tail) {
		tail = !more; /* behind the program's end: the one run for the limiter's tail */
		const size_t n = tail ? D : chunk;
		size_t len = 0;
		ok = engine->run_limited(nullptr, out_fmt, swap, pre_gain, ceiling, n, stereo, &more, &len, err);
		if (!ok) break;
		wanted += len;
		/* the file is y[D, D + wanted): while the program runs that covers every frame of a run but the first D */
		const uint64_t lo = y_pos > D ? y_pos : D, end = y_pos + n, hi = D + wanted < end ? D + wanted : end;
		if (hi > lo) {
			ok = backend->fetch_limited_async(0, host[slot], (size_t)(hi - y_pos) * frame_bytes, slot, err);
			first[slot] = (size_t)(lo - y_pos);
			pending[slot] = (size_t)(hi - lo);
		}
		y_pos = end;
		const int other = slot ^ 1;
		if (ok && pending[other]) {
			ok = backend->wait_fetch(other, err);
			if (ok && !out.write((const char *)host[other] + first[other] * frame_bytes, pending[other])) { err = "write failed"; ok = false; }
			pending[other] = 0;
		}
		slot = other;
	}
	for (int s = 0; ok && s < 2; ++s) { /* oldest first */
		const int k = slot ^ s;
		if (pending[k]) {
			ok = backend->wait_fetch(k, err);
			if (ok && !out.write((const char *)host[k] + first[k] * frame_bytes, pending[k])) { err = "write failed"; ok = false; }
			pending[k] = 0;
		}
	}
	if (ok && stats_out) ok = engine->limiter_stats(stats_out, false, err);
	{ std::string e2; (void)backend->sync(e2); }
	if (out.f && out.close() != 0 && ok) { err = "write failed"; ok = false; }
	if (frames_out) *frames_out = out.frames;
	backend->free_host(host[0]);
	backend->free_host(host[1]);
	delete engine;
	return ok;
}

/* sauAmd_render_spectrum's render: the runs of render_file_over (factor 1: measure_program's loop) or of write_oversampled,
 * with a feed of the run's device row where those fetch it -- the spectrum meter of one record takes exactly the floats the
 * float32 file would hold, and no sample leaves the device. The meter goes before the engine, which owns the backend. */
bool measure_spectrum(const sauProgram *prg, uint32_t srate, int factor, int channels, unsigned log2n, uint32_t hop,
		Backend *backend /* owned */, double *power_out, uint64_t *segments_out, uint64_t *frames_out, std::string &err) {
	const uint32_t rate = srate * (uint32_t)factor;
	Engine *engine = Engine::create(&prg, 1, rate, backend, err);
	if (!engine) return false;
	const bool stereo = channels == 2;
	size_t call, chunk;
	file_lattice(rate, call, chunk);
	engine->set_call_len(call);
	/* a backend without a spectrum meter, float output or a decimator says so here, before anything renders */
	sauengine::SpectrumMeter *meter = backend->create_spectrum(1, (uint32_t)channels, log2n, hop, err);
	bool ok = meter && engine->set_format(sauengine::SF_F32, err) && (factor == 1 || engine->begin_decimated(factor, stereo, err));
	uint64_t fed = 0;
	if (ok && factor == 1) {
		bool more = true;
		while (ok && more) {
			size_t len = 0;
			ok = engine->run_f32(nullptr, chunk, stereo, &more, &len, err);
			if (ok && len) {
				const uint32_t n = (uint32_t)len;
				const float *row = backend->device_pcm_f32(0);
				if (!row) { err = "the backend keeps no float rows on the device"; ok = false; }
				else ok = meter->feed(row, backend->device_pcm_pitch(), &n, err);
				fed += len;
			}
		}
	} else if (ok) {
		const size_t H = sauengine::decimator_latency(factor);
		bool more = true, tail = false;
		uint64_t y_pos = 0, wanted = 0; /* as write_oversampled counts them: what is measured is y[H, H + wanted) */
		while (ok && !tail) {
			tail = !more;
			const size_t n = tail ? H : chunk;
			size_t len = 0;
			ok = engine->run_decimated(nullptr, sauengine::SF_F32, false, factor, n, stereo, &more, &len, err);
			if (!ok) break;
			wanted += len;
			const uint64_t lo = y_pos > H ? y_pos : H, end = y_pos + n, hi = H + wanted < end ? H + wanted : end;
			if (hi > lo) {
				const uint32_t cnt = (uint32_t)(hi - lo);
				const float *row = backend->device_decimated_f32(0);
				if (!row) { err = "the backend keeps no decimated rows on the device"; ok = false; }
				else ok = meter->feed(row + (size_t)(lo - y_pos) * (size_t)channels, backend->device_decimated_pitch(), &cnt, err);
				fed += cnt;
			}
			y_pos = end;
		}
	}
	ok = ok && meter->read(power_out, segments_out, false, err);
	if (ok && frames_out) *frames_out = fed;
	delete meter;
	delete engine; /* owns the backend */
	return ok;
}

/* The FLAC file writers' process-wide MD5 switch (include/saugns_amd.h, FLAC, "MD5"): every writer below reads it once, where it
 * begins. On: the writer turns its encoder's MD5 on -- a backend whose encoder has none refuses there, before there is a file
 * --, fetches the digest behind the last read and puts it into the header it rewrites at the end. Off: nothing differs. */
static std::atomic<int> g_flac_file_md5{0};
static bool flac_file_md5() { return g_flac_file_md5.load(std::memory_order_relaxed) != 0; }
/* ... and their verify switch ("Verify"), its exact twin: on, the writer turns its encoder's verify mode on and fetches the
 * record behind the last read; a bad block makes the writer fail once the file is complete and closed. */
static std::atomic<int> g_flac_file_verify{0};
static bool flac_file_verify() { return g_flac_file_verify.load(std::memory_order_relaxed) != 0; }
/* false: the record could not be fetched (err); bad: what to say of the first bad block, empty when there is none */
static bool flac_file_verified(sauengine::FlacEncoder *enc, std::string &bad, std::string &err) {
	static const char *const names[] = {"OK", "LENGTH", "SYNC", "HEADER", "NUMBER", "CRC8", "SUBFRAME", "RESIDUAL", "PADDING", "CRC16", "RANGE", "MISMATCH"};
	sauengine::FlacVerify v{0, 0, 0, 0, 0};
	if (!enc->verify(&v, err)) return false;
	if (v.bad_blocks)
		bad = "FLAC verify failed: " + std::to_string(v.bad_blocks) + " of " + std::to_string(v.blocks) + " blocks bad, the first block " +
			std::to_string(v.first_bad_block) + " with status " + std::to_string(v.first_status) + " (" + (v.first_status < 12 ? names[v.first_status] : "?") + ")";
	return true;
}

/* The FLAC writer: render_file_over's int16 runs (no byte swap) on the same lattice, each run's device row fed to an encoder
 * of one stream where that writer fetches it, the last feed a finish. A read brings the run's frames into a page-locked slot;
 * the slot before it goes to the file once the next run has been queued, so the file is written while the device renders.
 * The encoder goes before the engine, which owns the backend. */
bool write_flac(const sauProgram *prg, uint32_t srate, const char *path, int channels, uint32_t block_frames, uint32_t max_lpc_order,
		Backend *backend /* owned */, uint64_t *frames_out, sauengine::FlacInfo *info_out, std::string &err) {
	Engine *engine = Engine::create(&prg, 1, srate, backend, err);
	if (!engine) return false;
	const bool stereo = channels == 2;
	const uint32_t B = sauflac::flac_block_frames(block_frames);
	size_t call, chunk;
	file_lattice(srate, call, chunk);
	engine->set_call_len(call);
	/* a backend without an encoder says so here, before there is a file */
	sauengine::FlacEncoder *enc = backend->create_flac_lpc(1, (uint32_t)channels, B, max_lpc_order, err);
	if (!enc) { delete engine; return false; }
	const bool md5 = flac_file_md5(), verify = flac_file_verify();
	std::string bad; /* (verify: the first bad block, if there is one) */
	if ((md5 && !enc->set_md5(true, err)) || (verify && !enc->set_verify(true, err))) { delete enc; delete engine; return false; }
	/* what a run can come to: the blocks it completes, with what was pending, and a last short one, each at its bound */
	const size_t slot_bytes = (chunk / B + 2) * (size_t)sauflac::flac_frame_bound(B, (uint32_t)channels, 16);
	uint8_t *host[2] = {(uint8_t *)backend->alloc_host(slot_bytes), (uint8_t *)backend->alloc_host(slot_bytes)};
	FILE *f = nullptr;
	bool ok = host[0] && host[1];
	if (!ok) err = "out of page-locked memory";
	uint8_t head[42], digest[16];
	sauengine::FlacInfo info{0, 0, 0, 0, 0};
	if (ok) {
		f = fopen(path, "wb");
		if (!f) { err = std::string("couldn't open \"") + path + "\" for writing"; ok = false; }
		else if (sauengine::flac_header(srate, channels, B, &info, head, sizeof head) != 42 || fwrite(head, 1, 42, f) != 42) { err = "write failed"; ok = false; }
	}
	size_t pending[2] = {0, 0};
	int slot = 0;
	bool more = ok;
	while (ok && more) {
		size_t len = 0;
		ok = engine->run(nullptr, chunk, stereo, &more, &len, err);
		if (!ok) break;
		const uint32_t n = (uint32_t)len;
		const int16_t *row = backend->device_pcm(0);
		if (!row) { err = "the backend keeps no int16 rows on the device"; ok = false; break; }
		ok = enc->feed(row, backend->device_pcm_pitch(), &n, !more, err);
		/* while this run renders and is encoded, the one before goes to the file */
		const int other = slot ^ 1;
		if (ok && pending[other]) {
			if (fwrite(host[other], 1, pending[other], f) != pending[other]) { err = "write failed"; ok = false; }
			pending[other] = 0;
		}
		if (ok) {
			uint8_t *const bufs[1] = {host[slot]};
			size_t got = 0;
			ok = enc->read(bufs, &slot_bytes, &got, &info, false, err);
			pending[slot] = got;
		}
		slot = other;
	}
	for (int s = 0; ok && s < 2; ++s) { /* oldest first: `slot` is the older of the two */
		const int k = slot ^ s;
		if (pending[k] && fwrite(host[k], 1, pending[k], f) != pending[k]) { err = "write failed"; ok = false; }
		pending[k] = 0;
	}
	if (ok && md5) ok = enc->md5(digest, err); /* (the last feed was the finish, and nothing has reset the stream) */
	if (ok && verify) ok = flac_file_verified(enc, bad, err);
	delete enc;
	{ std::string e2; (void)backend->sync(e2); }
	if (f) {
		if (ok && (sauengine::flac_header_md5(srate, channels, B, 16, &info, md5 ? digest : nullptr, head, sizeof head) != 42 || fseek(f, 0, SEEK_SET) != 0 ||
		           fwrite(head, 1, 42, f) != 42)) { err = "write failed"; ok = false; }
		const int ferr = ferror(f);
		if ((fclose(f) != 0 || ferr) && ok) { err = "write failed"; ok = false; }
	}
	if (ok && !bad.empty()) { err = bad; ok = false; } /* (the file is complete and closed as written, for inspection) */
	if (frames_out) *frames_out = info.frames;
	if (ok && info_out) *info_out = info;
	backend->free_host(host[0]);
	backend->free_host(host[1]);
	delete engine; /* owns the backend */
	return ok;
}

/* The scaled FLAC writer: write_scaled's float runs on the file lattice, each run's device row fed with `gain` to a float-fed
 * encoder of one stream (`bits` per sample) where that writer requantises and fetches; the file I/O is write_flac's. A backend
 * without float output or without the encoder says so before there is a file. */
bool write_flac_scaled(const sauProgram *prg, uint32_t srate, const char *path, int channels, uint32_t block_frames, int bits,
		uint32_t max_lpc_order, float gain, Backend *backend /* owned */, uint64_t *frames_out, sauengine::FlacInfo *info_out, std::string &err,
		bool lpc24 = false /* the encoder of "LPC at 24 bits" (bits is 24) */) {
	Engine *engine = Engine::create(&prg, 1, srate, backend, err);
	if (!engine) return false;
	const bool stereo = channels == 2;
	const uint32_t B = sauflac::flac_block_frames(block_frames);
	size_t call, chunk;
	file_lattice(srate, call, chunk);
	engine->set_call_len(call);
	if (!engine->set_format(sauengine::SF_F32, err)) { delete engine; return false; }
	sauengine::FlacEncoder *enc = lpc24 ? backend->create_flac_lpc24(1, (uint32_t)channels, B, max_lpc_order, err) :
			backend->create_flac_f32(1, (uint32_t)channels, B, bits, max_lpc_order, err);
	if (!enc) { delete engine; return false; }
	const bool md5 = flac_file_md5(), verify = flac_file_verify();
	std::string bad; /* (verify: the first bad block, if there is one) */
	if ((md5 && !enc->set_md5(true, err)) || (verify && !enc->set_verify(true, err))) { delete enc; delete engine; return false; }
	const size_t slot_bytes = (chunk / B + 2) * (size_t)sauflac::flac_frame_bound(B, (uint32_t)channels, (unsigned)bits);
	uint8_t *host[2] = {(uint8_t *)backend->alloc_host(slot_bytes), (uint8_t *)backend->alloc_host(slot_bytes)};
	FILE *f = nullptr;
	bool ok = host[0] && host[1];
	if (!ok) err = "out of page-locked memory";
	uint8_t head[42], digest[16];
	sauengine::FlacInfo info{0, 0, 0, 0, 0};
	if (ok) {
		f = fopen(path, "wb");
		if (!f) { err = std::string("couldn't open \"") + path + "\" for writing"; ok = false; }
		else if (sauengine::flac_header_bits(srate, channels, B, bits, &info, head, sizeof head) != 42 || fwrite(head, 1, 42, f) != 42) { err = "write failed"; ok = false; }
	}
	size_t pending[2] = {0, 0};
	int slot = 0;
	bool more = ok;
	while (ok && more) {
		size_t len = 0;
		ok = engine->run_f32(nullptr, chunk, stereo, &more, &len, err);
		if (!ok) break;
		const uint32_t n = (uint32_t)len;
		const float *row = backend->device_pcm_f32(0);
		if (!row) { err = "the backend keeps no float rows on the device"; ok = false; break; }
		/* (the rounding happens in the feed, once, after the gain) */
		ok = enc->feed_f32(row, backend->device_pcm_pitch(), &n, &gain, !more, err);
		/* while this run renders and is encoded, the one before goes to the file */
		const int other = slot ^ 1;
		if (ok && pending[other]) {
			if (fwrite(host[other], 1, pending[other], f) != pending[other]) { err = "write failed"; ok = false; }
			pending[other] = 0;
		}
		if (ok) {
			uint8_t *const bufs[1] = {host[slot]};
			size_t got = 0;
			ok = enc->read(bufs, &slot_bytes, &got, &info, false, err);
			pending[slot] = got;
		}
		slot = other;
	}
	for (int s = 0; ok && s < 2; ++s) { /* oldest first: `slot` is the older of the two */
		const int k = slot ^ s;
		if (pending[k] && fwrite(host[k], 1, pending[k], f) != pending[k]) { err = "write failed"; ok = false; }
		pending[k] = 0;
	}
	if (ok && md5) ok = enc->md5(digest, err); /* (the last feed was the finish, and nothing has reset the stream) */
	if (ok && verify) ok = flac_file_verified(enc, bad, err);
	delete enc;
	{ std::string e2; (void)backend->sync(e2); }
	if (f) {
		if (ok && (sauengine::flac_header_md5(srate, channels, B, bits, &info, md5 ? digest : nullptr, head, sizeof head) != 42 || fseek(f, 0, SEEK_SET) != 0 ||
		           fwrite(head, 1, 42, f) != 42)) { err = "write failed"; ok = false; }
		const int ferr = ferror(f);
		if ((fclose(f) != 0 || ferr) && ok) { err = "write failed"; ok = false; }
	}
	if (ok && !bad.empty()) { err = bad; ok = false; } /* (the file is complete and closed as written, for inspection) */
	if (frames_out) *frames_out = info.frames;
	if (ok && info_out) *info_out = info;
	backend->free_host(host[0]);
	backend->free_host(host[1]);
	delete engine; /* owns the backend */
	return ok;
}

/* The limited FLAC writer: write_limited's loop with float limited rows, each run's part of y[D, D + N) fed with gain 1 to a
 * float-fed encoder from where it lies in the device row (D frames in for the first run: the feed needs float alignment only),
 * the D-frame tail run fed too and as the finish; the file I/O is write_flac's. */
bool write_flac_limited(const sauProgram *prg, uint32_t srate, const char *path, int channels, uint32_t block_frames, int bits,
		uint32_t max_lpc_order, float pre_gain, float ceiling, Backend *backend /* owned */, uint64_t *frames_out,
		sauengine::LimiterStats *stats_out, sauengine::FlacInfo *info_out, std::string &err, bool lpc24 = false /* as write_flac_scaled's */) {
	Engine *engine = Engine::create(&prg, 1, srate, backend, err);
	if (!engine) return false;
	const bool stereo = channels == 2;
	const uint32_t B = sauflac::flac_block_frames(block_frames);
	const size_t D = sauengine::limiter_latency(srate);
	size_t call, chunk;
	file_lattice(srate, call, chunk);
	engine->set_call_len(call);
	/* a backend without float output, without a limiter or without the encoder says so here, before there is a file */
	if (!engine->set_format(sauengine::SF_F32, err) || !engine->begin_limited(pre_gain, ceiling, stereo, err)) { delete engine; return false; }
	sauengine::FlacEncoder *enc = lpc24 ? backend->create_flac_lpc24(1, (uint32_t)channels, B, max_lpc_order, err) :
			backend->create_flac_f32(1, (uint32_t)channels, B, bits, max_lpc_order, err);
	if (!enc) { delete engine; return false; }
	const bool md5 = flac_file_md5(), verify = flac_file_verify();
	std::string bad; /* (verify: the first bad block, if there is one) */
	if ((md5 && !enc->set_md5(true, err)) || (verify && !enc->set_verify(true, err))) { delete enc; delete engine; return false; }
	const size_t slot_frames = chunk > D ? chunk : D;
	const size_t slot_bytes = (slot_frames / B + 2) * (size_t)sauflac::flac_frame_bound(B, (uint32_t)channels, (unsigned)bits);
	uint8_t *host[2] = {(uint8_t *)backend->alloc_host(slot_bytes), (uint8_t *)backend->alloc_host(slot_bytes)};
	FILE *f = nullptr;
	bool ok = host[0] && host[1];
	if (!ok) err = "out of page-locked memory";
	uint8_t head[42], digest[16];
	sauengine::FlacInfo info{0, 0, 0, 0, 0};
	if (ok) {
		f = fopen(path, "wb");
		if (!f) { err = std::string("couldn't open \"") + path + "\" for writing"; ok = false; }
		else if (sauengine::flac_header_bits(srate, channels, B, bits, &info, head, sizeof head) != 42 || fwrite(head, 1, 42, f) != 42) { err = "write failed"; ok = false; }
	}
	size_t pending[2] = {0, 0};
	int slot = 0;
	bool more = ok, tail = false;
	uint64_t y_pos = 0, wanted = 0; /* limited frames made so far; the N frames rendered so far */
	while (ok && !tail) {
		tail = !more; /* behind the program's end: the one run for the limiter's tail, and the encoder's finish */
		const size_t n = tail ? D : chunk;
		size_t len = 0;
		ok = engine->run_limited(nullptr, sauengine::SF_F32, false, pre_gain, ceiling, n, stereo, &more, &len, err);
		if (!ok) break;
		wanted += len;
		/* the file is y[D, D + wanted): while the program runs that covers every frame of a run but the first D */
		const uint64_t lo = y_pos > D ? y_pos : D, end = y_pos + n, hi = D + wanted < end ? D + wanted : end;
		const uint32_t cnt = hi > lo ? (uint32_t)(hi - lo) : 0;
		if (cnt || tail) {
			const float *row = backend->device_limited_f32(0);
			if (!row) { err = "the backend keeps no limited rows on the device"; ok = false; break; }
			ok = enc->feed_f32(row + (cnt ? (size_t)(lo - y_pos) * (size_t)channels : 0), backend->device_limited_pitch(), &cnt, nullptr, tail, err);
		}
		y_pos = end;
		const int other = slot ^ 1;
		if (ok && pending[other]) {
			if (fwrite(host[other], 1, pending[other], f) != pending[other]) { err = "write failed"; ok = false; }
			pending[other] = 0;
		}
		if (ok) {
			uint8_t *const bufs[1] = {host[slot]};
			size_t got = 0;
			ok = enc->read(bufs, &slot_bytes, &got, &info, false, err);
			pending[slot] = got;
		}
		slot = other;
	}
	for (int s = 0; ok && s < 2; ++s) { /* oldest first */
		const int k = slot ^ s;
		if (pending[k] && fwrite(host[k], 1, pending[k], f) != pending[k]) { err = "write failed"; ok = false; }
		pending[k] = 0;
	}
	if (ok && stats_out) ok = engine->limiter_stats(stats_out, false, err);
	if (ok && md5) ok = enc->md5(digest, err); /* (the last feed was the finish, and nothing has reset the stream) */
	if (ok && verify) ok = flac_file_verified(enc, bad, err);
	delete enc;
	{ std::string e2; (void)backend->sync(e2); }
	if (f) {
		if (ok && (sauengine::flac_header_md5(srate, channels, B, bits, &info, md5 ? digest : nullptr, head, sizeof head) != 42 || fseek(f, 0, SEEK_SET) != 0 ||
		           fwrite(head, 1, 42, f) != 42)) { err = "write failed"; ok = false; }
		const int ferr = ferror(f);
		if ((fclose(f) != 0 || ferr) && ok) { err = "write failed"; ok = false; }
	}
	if (ok && !bad.empty()) { err = bad; ok = false; } /* (the file is complete and closed as written, for inspection) */
	if (frames_out) *frames_out = info.frames;
	if (ok && info_out) *info_out = info;
	backend->free_host(host[0]);
	backend->free_host(host[1]);
	delete engine; /* owns the backend */
	return ok;
}

/* The dithered writer: write_scaled's pass with a quantiser of one stream in place of requant_kernel -- each float run's
 * device row fed with `gain`, the stage's int16 row fetched through the two page-locked slots. The quantiser's rows are in
 * host order: an AU file's samples are swapped in the slot, behind the fetch. A backend without float output or without the
 * quantiser says so before there is a file. The quantiser goes before the engine, which owns the backend. */
bool write_dithered(const sauProgram *prg, uint32_t srate, const char *path, int format, int channels, float gain,
		const saudither::DitherSpec &spec, Backend *backend /* owned */, uint64_t *frames_out, sauengine::DitherStats *stats_out, std::string &err) {
	Engine *engine = Engine::create(&prg, 1, srate, backend, err);
	if (!engine) return false;
	const bool stereo = channels == 2;
	size_t call, chunk;
	file_lattice(srate, call, chunk);
	engine->set_call_len(call);
	if (!engine->set_format(sauengine::SF_F32, err)) { delete engine; return false; }
	sauengine::Quantizer *q = backend->create_quantizer(1, (uint32_t)channels, spec, err);
	if (!q) { delete engine; return false; }
	const size_t frame_bytes = (size_t)channels * sizeof(int16_t);
	void *host[2] = {backend->alloc_host(chunk * frame_bytes), backend->alloc_host(chunk * frame_bytes)};
	SndOut out;
	bool ok = host[0] && host[1];
	if (!ok) err = "out of page-locked memory";
	if (ok && !out.open(path, format, (uint16_t)channels, srate)) {
		err = std::string("couldn't open \"") + path + "\" for writing";
		ok = false;
	}
	const bool swap = format == SAU_AMD_SNDFILE_AU;
	auto flush = [&](int k, size_t len) -> bool {
		if (!backend->wait_fetch(k, err)) return false;
		if (swap) {
			int16_t *s = (int16_t *)host[k];
			for (size_t i = 0; i < len * (size_t)channels; ++i) s[i] = saudev::pcm_swap(s[i]);
		}
		if (!out.write(host[k], len)) { err = "write failed"; return false; }
		return true;
	};
	size_t pending[2] = {0, 0};
	int slot = 0;
	bool more = ok;
	while (ok && more) {
		size_t len = 0;
		ok = engine->run_f32(nullptr, chunk, stereo, &more, &len, err);
		if (!ok) break;
		if (len) {
			const uint32_t n = (uint32_t)len;
			const float *row = backend->device_pcm_f32(0);
			if (!row) { err = "the backend keeps no float rows on the device"; ok = false; break; }
			/* (the rounding happens here, once, after the gain) */
			ok = q->feed(row, backend->device_pcm_pitch(), &n, &gain, err) && q->fetch_async(host[slot], len * frame_bytes, slot, err);
			pending[slot] = len;
		}
		const int other = slot ^ 1;
		if (ok && pending[other]) {
			ok = flush(other, pending[other]);
			pending[other] = 0;
		}
		slot = other;
	}
	for (int s = 0; ok && s < 2; ++s) { /* oldest first */
		const int k = slot ^ s;
		if (pending[k]) {
			ok = flush(k, pending[k]);
			pending[k] = 0;
		}
	}
	sauengine::DitherStats st{0, {0, 0}};
	if (ok) ok = q->stats(&st, false, err);
	delete q;
	{ std::string e2; (void)backend->sync(e2); }
	if (out.f && out.close() != 0 && ok) { err = "write failed"; ok = false; }
	if (frames_out) *frames_out = out.frames;
	if (ok && stats_out) *stats_out = st;
	backend->free_host(host[0]);
	backend->free_host(host[1]);
	delete engine; /* owns the backend */
	return ok;
}

/* The dithered FLAC writer: write_flac_scaled's float runs, each through a quantiser of one stream whose int16 row is fed to
 * an int16-fed encoder where that writer feeds the floats; the file I/O is write_flac's. */
bool write_flac_dithered(const sauProgram *prg, uint32_t srate, const char *path, int channels, uint32_t block_frames,
		uint32_t max_lpc_order, float gain, const saudither::DitherSpec &spec, Backend *backend /* owned */, uint64_t *frames_out,
		sauengine::FlacInfo *info_out, sauengine::DitherStats *stats_out, std::string &err) {
	Engine *engine = Engine::create(&prg, 1, srate, backend, err);
	if (!engine) return false;
	const bool stereo = channels == 2;
	const uint32_t B = sauflac::flac_block_frames(block_frames);
	size_t call, chunk;
	file_lattice(srate, call, chunk);
	engine->set_call_len(call);
	if (!engine->set_format(sauengine::SF_F32, err)) { delete engine; return false; }
	sauengine::Quantizer *q = backend->create_quantizer(1, (uint32_t)channels, spec, err);
	if (!q) { delete engine; return false; }
	sauengine::FlacEncoder *enc = backend->create_flac_lpc(1, (uint32_t)channels, B, max_lpc_order, err);
	if (!enc) { delete q; delete engine; return false; }
	const bool md5 = flac_file_md5(), verify = flac_file_verify();
	std::string bad; /* (verify: the first bad block, if there is one) */
	if ((md5 && !enc->set_md5(true, err)) || (verify && !enc->set_verify(true, err))) { delete enc; delete q; delete engine; return false; }
	const size_t slot_bytes = (chunk / B + 2) * (size_t)sauflac::flac_frame_bound(B, (uint32_t)channels, 16);
	uint8_t *host[2] = {(uint8_t *)backend->alloc_host(slot_bytes), (uint8_t *)backend->alloc_host(slot_bytes)};
	FILE *f = nullptr;
	bool ok = host[0] && host[1];
	if (!ok) err = "out of page-locked memory";
	uint8_t head[42], digest[16];
	sauengine::FlacInfo info{0, 0, 0, 0, 0};
	if (ok) {
		f = fopen(path, "wb");
		if (!f) { err = std::string("couldn't open \"") + path + "\" for writing"; ok = false; }
		else if (sauengine::flac_header(srate, channels, B, &info, head, sizeof head) != 42 || fwrite(head, 1, 42, f) != 42) { err = "write failed"; ok = false; }
	}
	size_t pending[2] = {0, 0};
	int slot = 0;
	bool more = ok;
	while (ok && more) {
		size_t len = 0;
		ok = engine->run_f32(nullptr, chunk, stereo, &more, &len, err);
		if (!ok) break;
		const uint32_t n = (uint32_t)len;
		const float *row = backend->device_pcm_f32(0);
		if (!row) { err = "the backend keeps no float rows on the device"; ok = false; break; }
		ok = q->feed(row, backend->device_pcm_pitch(), &n, &gain, err);
		if (ok) { /* (a feed without frames -- the finish behind the last run -- names rows but reads none) */
			static const int16_t none[8] __attribute__((aligned(16))) = {0};
			ok = n ? enc->feed(q->rows(), q->pitch(), &n, !more, err) : enc->feed(none, 16, &n, !more, err);
		}
		/* while this run renders and is encoded, the one before goes to the file */
		const int other = slot ^ 1;
		if (ok && pending[other]) {
			if (fwrite(host[other], 1, pending[other], f) != pending[other]) { err = "write failed"; ok = false; }
			pending[other] = 0;
		}
		if (ok) {
			uint8_t *const bufs[1] = {host[slot]};
			size_t got = 0;
			ok = enc->read(bufs, &slot_bytes, &got, &info, false, err);
			pending[slot] = got;
		}
		slot = other;
	}
	for (int s = 0; ok && s < 2; ++s) { /* oldest first: `slot` is the older of the two */
		const int k = slot ^ s;
		if (pending[k] && fwrite(host[k], 1, pending[k], f) != pending[k]) { err = "write failed"; ok = false; }
		pending[k] = 0;
	}
	sauengine::DitherStats st{0, {0, 0}};
	if (ok) ok = q->stats(&st, false, err);
	if (ok && md5) ok = enc->md5(digest, err); /* (the last feed was the finish, and nothing has reset the stream) */
	if (ok && verify) ok = flac_file_verified(enc, bad, err);
	delete enc;
	delete q;
	{ std::string e2; (void)backend->sync(e2); }
	if (f) {
		if (ok && (sauengine::flac_header_md5(srate, channels, B, 16, &info, md5 ? digest : nullptr, head, sizeof head) != 42 || fseek(f, 0, SEEK_SET) != 0 ||
		           fwrite(head, 1, 42, f) != 42)) { err = "write failed"; ok = false; }
		const int ferr = ferror(f);
		if ((fclose(f) != 0 || ferr) && ok) { err = "write failed"; ok = false; }
	}
	if (ok && !bad.empty()) { err = bad; ok = false; } /* (the file is complete and closed as written, for inspection) */
	if (frames_out) *frames_out = info.frames;
	if (ok && info_out) *info_out = info;
	if (ok && stats_out) *stats_out = st;
	backend->free_host(host[0]);
	backend->free_host(host[1]);
	delete engine; /* owns the backend */
	return ok;
}

/* what the dithered writers refuse of a spec and a gain */
bool dither_args_ok(const sauAmdDither *spec, float gain) {
	return spec && saudither::dither_spec_ok(*(const saudither::DitherSpec *)spec) && gain >= -FLT_MAX && gain <= FLT_MAX;
}

/* what every FLAC writer of float runs refuses of its encoder's parameters */
bool flac_f32_params_ok(int channels, uint32_t block_frames, int bits, uint32_t max_lpc_order) {
	return sauengine::flac_params_ok(channels, block_frames) && sauflac::flac_bits_ok(bits) && max_lpc_order <= sauflac::FLAC_LPC_MAX &&
	       !(bits == 24 && max_lpc_order);
}

} /* namespace */

extern "C" int sauAmd_set_flac_file_md5(int on) { return g_flac_file_md5.exchange(on ? 1 : 0, std::memory_order_relaxed); }
extern "C" int sauAmd_set_flac_file_verify(int on) { return g_flac_file_verify.exchange(on ? 1 : 0, std::memory_order_relaxed); }

/* render_file_flac_f32's body, and with lpc24 render_file_flac_lpc24's: 24 bits, any order up to 8 */
static bool flac_f32_file(const sauProgram *prg, uint32_t srate, const char *path, int channels, uint32_t block_frames,
		int bits, uint32_t max_lpc_order, float gain, bool lpc24, const std::function<Backend *(std::string &)> &make_backend,
		uint64_t *frames_out, sauAmdFlacInfo *info_out, std::string &err) {
	if (frames_out) *frames_out = 0;
	if (!prg || !path || !srate || srate > 655350u || !flac_f32_params_ok(channels, block_frames, bits, lpc24 ? 0 : max_lpc_order) ||
	    max_lpc_order > sauflac::FLAC_LPC_MAX || !(gain >= -FLT_MAX && gain <= FLT_MAX)) { /* (a NaN fails both comparisons) */
		err = "bad argument";
		return false;
	}
	Backend *backend = make_backend(err);
	if (!backend) return false;
	return write_flac_scaled(prg, srate, path, channels, block_frames, bits, max_lpc_order, gain, backend, frames_out,
			(sauengine::FlacInfo *)info_out, err, lpc24);
}

bool sauamd_internal::render_file_flac_f32(const sauProgram *prg, uint32_t srate, const char *path, int channels, uint32_t block_frames,
		int bits, uint32_t max_lpc_order, float gain, const std::function<Backend *(std::string &)> &make_backend, uint64_t *frames_out,
		sauAmdFlacInfo *info_out, std::string &err) {
	return flac_f32_file(prg, srate, path, channels, block_frames, bits, max_lpc_order, gain, false, make_backend, frames_out, info_out, err);
}

bool sauamd_internal::render_file_flac_lpc24(const sauProgram *prg, uint32_t srate, const char *path, int channels, uint32_t block_frames,
		uint32_t max_lpc_order, float gain, const std::function<Backend *(std::string &)> &make_backend, uint64_t *frames_out,
		sauAmdFlacInfo *info_out, std::string &err) {
	return flac_f32_file(prg, srate, path, channels, block_frames, 24, max_lpc_order, gain, true, make_backend, frames_out, info_out, err);
}

extern "C" bool sauAmd_render_file_flac_lpc24(const sauProgram *prg, uint32_t srate, const char *path, int channels, uint32_t block_frames,
		uint32_t max_lpc_order, float gain, uint64_t *frames_out, sauAmdFlacInfo *info_out) {
	std::string err;
	bool ok = false;
	try {
		ok = sauamd_internal::render_file_flac_lpc24(prg, srate, path, channels, block_frames, max_lpc_order, gain,
				[](std::string &e) -> Backend * { return sauhip::create_hip_backend(e); }, frames_out, info_out, err);
	} catch (const std::exception &ex) { /* (nothing C++ crosses the C ABI) */
		err = std::string("internal error: ") + ex.what();
	}
	if (!ok) sauamd_internal::set_last_error("output", err);
	return ok;
}

extern "C" bool sauAmd_render_file_flac_f32(const sauProgram *prg, uint32_t srate, const char *path, int channels, uint32_t block_frames,
		int bits, uint32_t max_lpc_order, float gain, uint64_t *frames_out, sauAmdFlacInfo *info_out) {
	std::string err;
	bool ok = false;
	try {
		ok = sauamd_internal::render_file_flac_f32(prg, srate, path, channels, block_frames, bits, max_lpc_order, gain,
				[](std::string &e) -> Backend * { return sauhip::create_hip_backend(e); }, frames_out, info_out, err);
	} catch (const std::exception &ex) { /* (nothing C++ crosses the C ABI) */
		err = std::string("internal error: ") + ex.what();
	}
	if (!ok) sauamd_internal::set_last_error("output", err);
	return ok;
}

/* render_file_flac_loudness's body, and with lpc24 render_file_flac_loudness_lpc24's */
static bool flac_loudness_file(const sauProgram *prg, uint32_t srate, const char *path, int channels, uint32_t block_frames,
		int bits, uint32_t max_lpc_order, double target_lufs, float max_true_peak, bool limited, bool lpc24,
		const std::function<Backend *(std::string &)> &make_backend, uint64_t *frames_out, sauAmdLoudness *loud_out, float *gain_out,
		sauAmdLimiterStats *stats_out, sauAmdFlacInfo *info_out, std::string &err) {
	if (frames_out) *frames_out = 0;
	if (!prg || !path || srate > 655350u || !flac_f32_params_ok(channels, block_frames, bits, lpc24 ? 0 : max_lpc_order) ||
	    max_lpc_order > sauflac::FLAC_LPC_MAX || !(target_lufs >= -DBL_MAX && target_lufs <= DBL_MAX) || !(max_true_peak > 0.f) || !(max_true_peak <= FLT_MAX) ||
	    srate < sauengine::LOUD_MIN_RATE) { /* (a NaN fails every comparison) */
		err = "bad argument";
		return false;
	}
	Backend *first = make_backend(err);
	if (!first) return false;
	sauengine::Loudness ld;
	if (!measure_program_loudness(prg, srate, channels == 2, first, ld, err)) return false;
	if (loud_out) memcpy(loud_out, &ld, sizeof ld);
	float gain = 1.0f;
	if (!limited) { /* render_file_loudness's rule */
		const float tp = ld.true_peak[0] > ld.true_peak[1] ? ld.true_peak[0] : ld.true_peak[1];
		if (ld.integrated > -HUGE_VAL) {
			gain = (float)pow(10.0, (target_lufs - ld.integrated) / 20.0);
			if (tp * gain > max_true_peak) gain = max_true_peak / tp; /* the ceiling binds: one f32 division */
		}
		if (gain_out) *gain_out = gain;
		if (!(gain >= -FLT_MAX && gain <= FLT_MAX)) { err = "bad argument: the gain to the target loudness is not finite"; return false; }
		Backend *second = make_backend(err);
		if (!second) return false;
		return write_flac_scaled(prg, srate, path, channels, block_frames, bits, max_lpc_order, gain, second, frames_out,
				(sauengine::FlacInfo *)info_out, err, lpc24);
	}
	/* render_file_loudness_limited's rule: never lowered for the ceiling, the limiter holds that */
	if (ld.integrated > -HUGE_VAL) gain = (float)pow(10.0, (target_lufs - ld.integrated) / 20.0);
	if (gain_out) *gain_out = gain;
	if (!(gain > 0.f) || !(gain <= FLT_MAX)) { err = "bad argument: the gain to the target loudness is not a finite positive float"; return false; }
	Backend *second = make_backend(err);
	if (!second) return false;
	sauengine::LimiterStats st{0, 0, 1.0};
	const bool ok = write_flac_limited(prg, srate, path, channels, block_frames, bits, max_lpc_order, gain, max_true_peak, second, frames_out,
			&st, (sauengine::FlacInfo *)info_out, err, lpc24);
	if (ok && stats_out) memcpy(stats_out, &st, sizeof st);
	return ok;
}

bool sauamd_internal::render_file_flac_loudness(const sauProgram *prg, uint32_t srate, const char *path, int channels, uint32_t block_frames,
		int bits, uint32_t max_lpc_order, double target_lufs, float max_true_peak, bool limited,
		const std::function<Backend *(std::string &)> &make_backend, uint64_t *frames_out, sauAmdLoudness *loud_out, float *gain_out,
		sauAmdLimiterStats *stats_out, sauAmdFlacInfo *info_out, std::string &err) {
	return flac_loudness_file(prg, srate, path, channels, block_frames, bits, max_lpc_order, target_lufs, max_true_peak, limited, false,
			make_backend, frames_out, loud_out, gain_out, stats_out, info_out, err);
}

bool sauamd_internal::render_file_flac_loudness_lpc24(const sauProgram *prg, uint32_t srate, const char *path, int channels,
		uint32_t block_frames, uint32_t max_lpc_order, double target_lufs, float max_true_peak, bool limited,
		const std::function<Backend *(std::string &)> &make_backend, uint64_t *frames_out, sauAmdLoudness *loud_out, float *gain_out,
		sauAmdLimiterStats *stats_out, sauAmdFlacInfo *info_out, std::string &err) {
	return flac_loudness_file(prg, srate, path, channels, block_frames, 24, max_lpc_order, target_lufs, max_true_peak, limited, true,
			make_backend, frames_out, loud_out, gain_out, stats_out, info_out, err);
}

extern "C" bool sauAmd_render_file_flac_loudness_lpc24(const sauProgram *prg, uint32_t srate, const char *path, int channels,
		uint32_t block_frames, uint32_t max_lpc_order, double target_lufs, float max_true_peak, int limited,
		uint64_t *frames_out, sauAmdLoudness *loud_out, float *gain_out, sauAmdLimiterStats *stats_out, sauAmdFlacInfo *info_out) {
	std::string err;
	bool ok = false;
	try {
		ok = sauamd_internal::render_file_flac_loudness_lpc24(prg, srate, path, channels, block_frames, max_lpc_order, target_lufs,
				max_true_peak, limited != 0, [](std::string &e) -> Backend * { return sauhip::create_hip_backend(e); }, frames_out,
				loud_out, gain_out, stats_out, info_out, err);
	} catch (const std::exception &ex) { /* (nothing C++ crosses the C ABI) */
		err = std::string("internal error: ") + ex.what();
	}
	if (!ok) sauamd_internal::set_last_error("output", err);
	return ok;
}

extern "C" bool sauAmd_render_file_flac_loudness(const sauProgram *prg, uint32_t srate, const char *path, int channels,
		uint32_t block_frames, int bits, uint32_t max_lpc_order, double target_lufs, float max_true_peak, int limited,
		uint64_t *frames_out, sauAmdLoudness *loud_out, float *gain_out, sauAmdLimiterStats *stats_out, sauAmdFlacInfo *info_out) {
	std::string err;
	bool ok = false;
	try {
		ok = sauamd_internal::render_file_flac_loudness(prg, srate, path, channels, block_frames, bits, max_lpc_order, target_lufs,
				max_true_peak, limited != 0, [](std::string &e) -> Backend * { return sauhip::create_hip_backend(e); }, frames_out,
				loud_out, gain_out, stats_out, info_out, err);
	} catch (const std::exception &ex) { /* (nothing C++ crosses the C ABI) */
		err = std::string("internal error: ") + ex.what();
	}
	if (!ok) sauamd_internal::set_last_error("output", err);
	return ok;
}

bool sauamd_internal::render_file_normalized(const sauProgram *prg, uint32_t srate, const char *path, int format, int channels,
		float target_peak, const std::function<Backend *(std::string &)> &make_backend, uint64_t *frames_out,
		sauAmdLevels *levels_out, std::string &err) {
	if (frames_out) *frames_out = 0;
	if (!prg || !path || (channels != 1 && channels != 2) || format < 0 || format > SAU_AMD_SNDFILE_WAV_F32 ||
	    !(target_peak > 0.f) || !(target_peak <= FLT_MAX)) { /* (a NaN fails both comparisons) */
		err = "bad argument";
		return false;
	}
	Backend *first = make_backend(err);
	if (!first) return false;
	sauengine::Levels lv;
	if (!measure_program(prg, srate, channels == 2, first, lv, err)) return false;
	if (levels_out) memcpy(levels_out, &lv, sizeof lv);
	const float peak = lv.peak[0] > lv.peak[1] ? lv.peak[0] : lv.peak[1];
	const float gain = peak == 0.f ? 1.0f : target_peak / peak;
	Backend *second = make_backend(err);
	if (!second) return false;
	return write_scaled(prg, srate, path, format, channels, gain, second, frames_out, err);
}

extern "C" bool sauAmd_render_file_normalized(const sauProgram *prg, uint32_t srate, const char *path, int format,
		int channels, float target_peak, uint64_t *frames_out, sauAmdLevels *levels_out) {
	std::string err;
	bool ok = false;
	try {
		ok = sauamd_internal::render_file_normalized(prg, srate, path, format, channels, target_peak,
				[](std::string &e) -> Backend * { return sauhip::create_hip_backend(e); }, frames_out, levels_out, err);
	} catch (const std::exception &ex) { /* (nothing C++ crosses the C ABI) */
		err = std::string("internal error: ") + ex.what();
	}
	if (!ok) sauamd_internal::set_last_error("output", err);
	return ok;
}

bool sauamd_internal::render_file_loudness(const sauProgram *prg, uint32_t srate, const char *path, int format, int channels,
		double target_lufs, float max_true_peak, const std::function<Backend *(std::string &)> &make_backend, uint64_t *frames_out,
		sauAmdLoudness *loud_out, float *gain_out, std::string &err) {
	if (frames_out) *frames_out = 0;
	if (!prg || !path || (channels != 1 && channels != 2) || format < 0 || format > SAU_AMD_SNDFILE_WAV_F32 ||
	    !(target_lufs >= -DBL_MAX && target_lufs <= DBL_MAX) || !(max_true_peak > 0.f) || !(max_true_peak <= FLT_MAX) ||
	    srate < sauengine::LOUD_MIN_RATE) { /* (a NaN fails every comparison) */
		err = "bad argument";
		return false;
	}
	Backend *first = make_backend(err);
	if (!first) return false;
	sauengine::Loudness ld;
	if (!measure_program_loudness(prg, srate, channels == 2, first, ld, err)) return false;
	if (loud_out) memcpy(loud_out, &ld, sizeof ld);
	const float tp = ld.true_peak[0] > ld.true_peak[1] ? ld.true_peak[0] : ld.true_peak[1];
	float gain = 1.0f;
	if (ld.integrated > -HUGE_VAL) {
		gain = (float)pow(10.0, (target_lufs - ld.integrated) / 20.0);
		if (tp * gain > max_true_peak) gain = max_true_peak / tp; /* the ceiling binds: one f32 division */
	}
	if (gain_out) *gain_out = gain;
	Backend *second = make_backend(err);
	if (!second) return false;
	return write_scaled(prg, srate, path, format, channels, gain, second, frames_out, err);
}

extern "C" bool sauAmd_render_file_loudness(const sauProgram *prg, uint32_t srate, const char *path, int format, int channels,
		double target_lufs, float max_true_peak, uint64_t *frames_out, sauAmdLoudness *loud_out, float *gain_out) {
	std::string err;
	bool ok = false;
	try {
		ok = sauamd_internal::render_file_loudness(prg, srate, path, format, channels, target_lufs, max_true_peak,
				[](std::string &e) -> Backend * { return sauhip::create_hip_backend(e); }, frames_out, loud_out, gain_out, err);
	} catch (const std::exception &ex) { /* (nothing C++ crosses the C ABI) */
		err = std::string("internal error: ") + ex.what();
	}
	if (!ok) sauamd_internal::set_last_error("output", err);
	return ok;
}

/* ---- the dithered writers (include/saugns_amd.h, section "Dither and noise shaping"): every argument is looked at before a
 * backend is made, and every refusal comes before any file is created ---- */
extern "C" bool sauAmd_render_file_dithered(const sauProgram *prg, uint32_t srate, const char *path, int format, int channels,
		float gain, const sauAmdDither *spec, uint64_t *frames_out, sauAmdDitherStats *stats_out) {
	std::string err;
	bool ok = false;
	if (frames_out) *frames_out = 0;
	try {
		if (!prg || !path || (channels != 1 && channels != 2) || format < 0 || format > SAU_AMD_SNDFILE_WAV || !dither_args_ok(spec, gain))
			err = "bad argument";
		else if (Backend *backend = sauhip::create_hip_backend(err))
			ok = write_dithered(prg, srate, path, format, channels, gain, *(const saudither::DitherSpec *)spec, backend, frames_out,
					(sauengine::DitherStats *)stats_out, err);
	} catch (const std::exception &ex) { /* (nothing C++ crosses the C ABI) */
		err = std::string("internal error: ") + ex.what();
	}
	if (!ok) sauamd_internal::set_last_error("output", err);
	return ok;
}

extern "C" bool sauAmd_render_file_flac_dithered(const sauProgram *prg, uint32_t srate, const char *path, int channels,
		uint32_t block_frames, uint32_t max_lpc_order, float gain, const sauAmdDither *spec, uint64_t *frames_out,
		sauAmdFlacInfo *info_out, sauAmdDitherStats *stats_out) {
	std::string err;
	bool ok = false;
	if (frames_out) *frames_out = 0;
	try {
		if (!prg || !path || !srate || srate > 655350u || !sauengine::flac_params_ok(channels, block_frames) ||
		    max_lpc_order > sauflac::FLAC_LPC_MAX || !dither_args_ok(spec, gain))
			err = "bad argument";
		else if (Backend *backend = sauhip::create_hip_backend(err))
			ok = write_flac_dithered(prg, srate, path, channels, block_frames, max_lpc_order, gain, *(const saudither::DitherSpec *)spec,
					backend, frames_out, (sauengine::FlacInfo *)info_out, (sauengine::DitherStats *)stats_out, err);
	} catch (const std::exception &ex) { /* (nothing C++ crosses the C ABI) */
		err = std::string("internal error: ") + ex.what();
	}
	if (!ok) sauamd_internal::set_last_error("output", err);
	return ok;
}

extern "C" bool sauAmd_render_file_loudness_dithered(const sauProgram *prg, uint32_t srate, const char *path, int format, int channels,
		double target_lufs, float max_true_peak, const sauAmdDither *spec, uint64_t *frames_out, sauAmdLoudness *loud_out,
		float *gain_out, sauAmdDitherStats *stats_out) {
	std::string err;
	bool ok = false;
	if (frames_out) *frames_out = 0;
	try {
		if (!prg || !path || (channels != 1 && channels != 2) || format < 0 || format > SAU_AMD_SNDFILE_WAV || !dither_args_ok(spec, 1.0f) ||
		    !(target_lufs >= -DBL_MAX && target_lufs <= DBL_MAX) || !(max_true_peak > 0.f) || !(max_true_peak <= FLT_MAX) ||
		    srate < sauengine::LOUD_MIN_RATE) /* (a NaN fails every comparison) */
			err = "bad argument";
		else if (Backend *first = sauhip::create_hip_backend(err)) {
			sauengine::Loudness ld;
			if (measure_program_loudness(prg, srate, channels == 2, first, ld, err)) {
				if (loud_out) memcpy(loud_out, &ld, sizeof ld);
				/* render_file_loudness's rule */
				const float tp = ld.true_peak[0] > ld.true_peak[1] ? ld.true_peak[0] : ld.true_peak[1];
				float gain = 1.0f;
				if (ld.integrated > -HUGE_VAL) {
					gain = (float)pow(10.0, (target_lufs - ld.integrated) / 20.0);
					if (tp * gain > max_true_peak) gain = max_true_peak / tp; /* the ceiling binds: one f32 division */
				}
				if (gain_out) *gain_out = gain;
				if (!(gain >= -FLT_MAX && gain <= FLT_MAX)) err = "bad argument: the gain to the target loudness is not finite";
				else if (Backend *second = sauhip::create_hip_backend(err))
					ok = write_dithered(prg, srate, path, format, channels, gain, *(const saudither::DitherSpec *)spec, second, frames_out,
							(sauengine::DitherStats *)stats_out, err);
			}
		}
	} catch (const std::exception &ex) { /* (nothing C++ crosses the C ABI) */
		err = std::string("internal error: ") + ex.what();
	}
	if (!ok) sauamd_internal::set_last_error("output", err);
	return ok;
}

bool sauamd_internal::render_file_loudness_limited(const sauProgram *prg, uint32_t srate, const char *path, int format, int channels,
		double target_lufs, float max_true_peak, const std::function<Backend *(std::string &)> &make_backend, uint64_t *frames_out,
		sauAmdLoudness *loud_out, float *gain_out, sauAmdLimiterStats *stats_out, std::string &err) {
	if (frames_out) *frames_out = 0;
	if (!prg || !path || (channels != 1 && channels != 2) || format < 0 || format > SAU_AMD_SNDFILE_WAV_F32 ||
	    !(target_lufs >= -DBL_MAX && target_lufs <= DBL_MAX) || !(max_true_peak > 0.f) || !(max_true_peak <= FLT_MAX) ||
	    srate < sauengine::LOUD_MIN_RATE) { /* (a NaN fails every comparison) */
		err = "bad argument";
		return false;
	}
	Backend *first = make_backend(err);
	if (!first) return false;
	sauengine::Loudness ld;
	if (!measure_program_loudness(prg, srate, channels == 2, first, ld, err)) return false;
	if (loud_out) memcpy(loud_out, &ld, sizeof ld);
	float gain = 1.0f; /* never lowered for the ceiling: the limiter holds that */
	if (ld.integrated > -HUGE_VAL) gain = (float)pow(10.0, (target_lufs - ld.integrated) / 20.0);
	if (gain_out) *gain_out = gain;
	if (!(gain > 0.f) || !(gain <= FLT_MAX)) { err = "bad argument: the gain to the target loudness is not a finite positive float"; return false; }
	Backend *second = make_backend(err);
	if (!second) return false;
	sauengine::LimiterStats st{0, 0, 1.0};
	const bool ok = write_limited(prg, srate, path, format, channels, gain, max_true_peak, second, frames_out, &st, err);
	if (ok && stats_out) memcpy(stats_out, &st, sizeof st);
	return ok;
}

extern "C" bool sauAmd_render_file_loudness_limited(const sauProgram *prg, uint32_t srate, const char *path, int format, int channels,
		double target_lufs, float max_true_peak, uint64_t *frames_out, sauAmdLoudness *loud_out, float *gain_out,
		sauAmdLimiterStats *stats_out) {
	std::string err;
	bool ok = false;
	try {
		ok = sauamd_internal::render_file_loudness_limited(prg, srate, path, format, channels, target_lufs, max_true_peak,
				[](std::string &e) -> Backend * { return sauhip::create_hip_backend(e); }, frames_out, loud_out, gain_out, stats_out, err);
	} catch (const std::exception &ex) { /* (nothing C++ crosses the C ABI) */
		err = std::string("internal error: ") + ex.what();
	}
	if (!ok) sauamd_internal::set_last_error("output", err);
	return ok;
}

bool sauamd_internal::render_file_oversampled(const sauProgram *prg, uint32_t srate, int factor, const char *path, int format,
		int channels, const std::function<Backend *(std::string &)> &make_backend, uint64_t *frames_out, std::string &err) {
	if (frames_out) *frames_out = 0;
	if (!prg || !path || (channels != 1 && channels != 2) || format < 0 || format > SAU_AMD_SNDFILE_WAV_F32 ||
	    !sauengine::decimator_latency(factor) || !srate || srate > UINT32_MAX / (uint32_t)factor) {
		err = "bad argument";
		return false;
	}
	Backend *backend = make_backend(err);
	if (!backend) return false;
	return write_oversampled(prg, srate, factor, path, format, channels, backend, frames_out, err);
}

extern "C" bool sauAmd_render_file_oversampled(const sauProgram *prg, uint32_t srate, int factor, const char *path, int format,
		int channels, uint64_t *frames_out) {
	std::string err;
	bool ok = false;
	try {
		ok = sauamd_internal::render_file_oversampled(prg, srate, factor, path, format, channels,
				[](std::string &e) -> Backend * { return sauhip::create_hip_backend(e); }, frames_out, err);
	} catch (const std::exception &ex) { /* (nothing C++ crosses the C ABI) */
		err = std::string("internal error: ") + ex.what();
	}
	if (!ok) sauamd_internal::set_last_error("output", err);
	return ok;
}

extern "C" bool sauAmd_render_file(const sauProgram *prg, uint32_t srate, const char *path,
		int format, int channels, uint64_t *frames_out) {
	std::string err;
	sauhip::HipBackend *hip = sauhip::create_hip_backend(err);
	bool ok = hip && render_file_over(prg, srate, path, format, channels, hip, frames_out, err);
	if (!ok) {
		g_file_error = err;
		fprintf(stderr, "error [output]: %s\n", err.c_str());
	}
	return ok;
}

/* (tests/hooks: the same output stage over a caller-supplied backend -- CPU tests of headers, chunking, byte order) */
bool sauamd_internal::render_file(const sauProgram *prg, uint32_t srate, const char *path, int format, int channels,
		Backend *injected, uint64_t *frames_out, std::string &err) {
	return injected && render_file_over(prg, srate, path, format, channels, injected, frames_out, err);
}

bool sauamd_internal::render_spectrum(const sauProgram *prg, uint32_t srate, int factor, int channels, unsigned log2n, uint32_t hop,
		const std::function<Backend *(std::string &)> &make_backend, double *power_out, uint64_t *segments_out, uint64_t *frames_out,
		std::string &err) {
	if (frames_out) *frames_out = 0;
	if (!prg || !power_out || !segments_out || !sauengine::spectrum_params_ok(channels, log2n, hop) || !srate ||
	    (factor != 1 && !sauengine::decimator_latency(factor)) || srate > UINT32_MAX / (uint32_t)factor) {
		err = "bad argument";
		return false;
	}
	Backend *backend = make_backend(err);
	if (!backend) return false;
	return measure_spectrum(prg, srate, factor, channels, log2n, hop, backend, power_out, segments_out, frames_out, err);
}

extern "C" bool sauAmd_render_spectrum(const sauProgram *prg, uint32_t srate, int factor, int channels, unsigned log2n, uint32_t hop,
		double *power_out, uint64_t *segments_out, uint64_t *frames_out) {
	std::string err;
	bool ok = false;
	try {
		ok = sauamd_internal::render_spectrum(prg, srate, factor, channels, log2n, hop,
				[](std::string &e) -> Backend * { return sauhip::create_hip_backend(e); }, power_out, segments_out, frames_out, err);
	} catch (const std::exception &ex) { /* (nothing C++ crosses the C ABI) */
		err = std::string("internal error: ") + ex.what();
	}
	if (!ok) sauamd_internal::set_last_error("output", err);
	return ok;
}

bool sauamd_internal::render_file_flac(const sauProgram *prg, uint32_t srate, const char *path, int channels, uint32_t block_frames,
		const std::function<Backend *(std::string &)> &make_backend, uint64_t *frames_out, sauAmdFlacInfo *info_out, std::string &err) {
	return render_file_flac_lpc(prg, srate, path, channels, block_frames, 0, make_backend, frames_out, info_out, err);
}

bool sauamd_internal::render_file_flac_lpc(const sauProgram *prg, uint32_t srate, const char *path, int channels, uint32_t block_frames,
		uint32_t max_lpc_order, const std::function<Backend *(std::string &)> &make_backend, uint64_t *frames_out, sauAmdFlacInfo *info_out,
		std::string &err) {
	if (frames_out) *frames_out = 0;
	if (!prg || !path || !srate || srate > 655350u || !sauengine::flac_params_ok(channels, block_frames) || max_lpc_order > sauflac::FLAC_LPC_MAX) {
		err = "bad argument";
		return false;
	}
	Backend *backend = make_backend(err);
	if (!backend) return false;
	return write_flac(prg, srate, path, channels, block_frames, max_lpc_order, backend, frames_out, (sauengine::FlacInfo *)info_out, err);
}

extern "C" bool sauAmd_render_file_flac(const sauProgram *prg, uint32_t srate, const char *path, int channels, uint32_t block_frames,
		uint64_t *frames_out, sauAmdFlacInfo *info_out) {
	std::string err;
	bool ok = false;
	try {
		ok = sauamd_internal::render_file_flac(prg, srate, path, channels, block_frames,
				[](std::string &e) -> Backend * { return sauhip::create_hip_backend(e); }, frames_out, info_out, err);
	} catch (const std::exception &ex) { /* (nothing C++ crosses the C ABI) */
		err = std::string("internal error: ") + ex.what();
	}
	if (!ok) sauamd_internal::set_last_error("output", err);
	return ok;
}

extern "C" bool sauAmd_render_file_flac_lpc(const sauProgram *prg, uint32_t srate, const char *path, int channels, uint32_t block_frames,
		uint32_t max_lpc_order, uint64_t *frames_out, sauAmdFlacInfo *info_out) {
	std::string err;
	bool ok = false;
	try {
		ok = sauamd_internal::render_file_flac_lpc(prg, srate, path, channels, block_frames, max_lpc_order,
				[](std::string &e) -> Backend * { return sauhip::create_hip_backend(e); }, frames_out, info_out, err);
	} catch (const std::exception &ex) { /* (nothing C++ crosses the C ABI) */
		err = std::string("internal error: ") + ex.what();
	}
	if (!ok) sauamd_internal::set_last_error("output", err);
	return ok;
}
