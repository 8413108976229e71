/* oversample_hooks.cpp -- TEST INFRASTRUCTURE: sauAmd_render_file_oversampled (saugns_amd/csrc/sndout.cpp) over a
 * caller-supplied sauengine::Backend, for tests/test_decimate_host.py: the writer's refusals -- a backend without float output
 * or a decimator, a bad factor, format or channel count -- happen before a file exists, and that is checked without a GPU.
 * The engine made over the backend owns it; a refusal ahead of that leaves it to this hook. */
#include "../../saugns_amd/csrc/capi_internal.h"

#define HOOK extern "C" __attribute__((visibility("default")))

HOOK bool sauAmd_render_file_oversampled_with_backend(const sauProgram *prg, uint32_t srate, int factor, const char *path,
		int format, int channels, void *backend, uint64_t *frames_out) {
	std::string err;
	sauengine::Backend *be = (sauengine::Backend *)backend;
	const bool ok = sauamd_internal::render_file_oversampled(prg, srate, factor, path, format, channels,
			[&be](std::string &e) -> sauengine::Backend * {
				sauengine::Backend *b = be;
				be = nullptr;
				if (!b) e = "the test hook has one backend only";
				return b;
			}, frames_out, err);
	delete be; /* (a refusal ahead of the render: nothing has taken the backend over) */
	if (!ok) sauamd_internal::set_last_error("output", err);
	return ok;
}
