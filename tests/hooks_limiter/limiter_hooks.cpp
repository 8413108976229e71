/* limiter_hooks.cpp -- TEST INFRASTRUCTURE: sauAmd_render_file_loudness_limited (saugns_amd/csrc/sndout.cpp) over a
 * caller-supplied sauengine::Backend, for tests/test_limiter_host.py: the writer's refusals -- a backend without float output,
 * loudness metering or a limiter, a bad target or ceiling, a rate below 2560 Hz -- happen before a file exists, and that is
 * checked without a GPU. The backend serves the first pass (the engine made over it owns it); there is no second one to hand
 * out, and no test here gets that far. */
#include "../../saugns_amd/csrc/capi_internal.h"

#define HOOK extern "C" __attribute__((visibility("default")))

HOOK bool sauAmd_render_file_loudness_limited_with_backend(const sauProgram *prg, uint32_t srate, const char *path, int format,
		int channels, double target_lufs, float max_true_peak, void *backend, uint64_t *frames_out, sauAmdLoudness *loud_out,
		float *gain_out, sauAmdLimiterStats *stats_out) {
	std::string err;
	sauengine::Backend *be = (sauengine::Backend *)backend;
	const bool ok = sauamd_internal::render_file_loudness_limited(prg, srate, path, format, channels, target_lufs, max_true_peak,
			[&be](std::string &e) -> sauengine::Backend * {
				sauengine::Backend *b = be;
				be = nullptr;
				if (!b) e = "the test hook has one backend only";
				return b;
			}, frames_out, loud_out, gain_out, stats_out, err);
	delete be; /* (a refusal ahead of the first pass: nothing has taken the backend over) */
	if (!ok) sauamd_internal::set_last_error("output", err);
	return ok;
}
