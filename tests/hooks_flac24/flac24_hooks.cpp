/* flac24_hooks.cpp -- TEST INFRASTRUCTURE for tests/test_flac24_host.py, without a GPU:
 *   sauAmd_render_file_flac_f32_with_backend        sauAmd_render_file_flac_f32 (saugns_amd/csrc/sndout.cpp) over a caller-supplied
 *       sauengine::Backend: its refusals -- a bad argument, a backend without float output or the encoder -- happen before any
 *       file is created.
 *   sauAmd_render_file_flac_loudness_with_backends  sauAmd_render_file_flac_loudness over two caller-supplied backends, one
 *       per pass, likewise.
 *   sauAmd_flac_plan_bits                           what launch_plan.h plans for a feed at a sample width. */
#include "../../saugns_amd/csrc/capi_internal.h"
#include "../../saugns_amd/csrc/sau_dev_ops.h"
#include "../../saugns_amd/csrc/launch_plan.h"
#include <vector>

#define HOOK extern "C" __attribute__((visibility("default")))

HOOK bool sauAmd_render_file_flac_f32_with_backend(const sauProgram *prg, uint32_t srate, const char *path, int channels,
		uint32_t block_frames, int bits, uint32_t max_lpc_order, float gain, void *backend, uint64_t *frames_out, sauAmdFlacInfo *info_out) {
	std::string err;
	sauengine::Backend *be = (sauengine::Backend *)backend;
	const bool ok = sauamd_internal::render_file_flac_f32(prg, srate, path, channels, block_frames, bits, max_lpc_order, gain,
			[&be](std::string &e) -> sauengine::Backend * {
				sauengine::Backend *b = be;
				be = nullptr;
				if (!b) e = "the test hook has one backend only";
				return b;
			}, frames_out, info_out, err);
	delete be; /* (a refusal ahead of the render: nothing has taken the backend over) */
	if (!ok) sauamd_internal::set_last_error("output", err);
	return ok;
}

HOOK bool sauAmd_render_file_flac_loudness_with_backends(const sauProgram *prg, uint32_t srate, const char *path, int channels,
		uint32_t block_frames, int bits, uint32_t max_lpc_order, double target_lufs, float max_true_peak, int limited, void *first,
		void *second, uint64_t *frames_out) {
	std::string err;
	sauengine::Backend *be[2] = {(sauengine::Backend *)first, (sauengine::Backend *)second};
	int next = 0;
	const bool ok = sauamd_internal::render_file_flac_loudness(prg, srate, path, channels, block_frames, bits, max_lpc_order, target_lufs,
			max_true_peak, limited != 0,
			[&be, &next](std::string &e) -> sauengine::Backend * {
				sauengine::Backend *b = next < 2 ? be[next] : nullptr;
				if (next < 2) be[next++] = nullptr;
				if (!b) e = "the test hook has two backends only";
				return b;
			}, frames_out, nullptr, nullptr, nullptr, nullptr, err);
	delete be[0]; /* (a refusal ahead of a pass: nothing has taken that pass' backend over) */
	delete be[1];
	if (!ok) sauamd_internal::set_last_error("output", err);
	return ok;
}

/* a feed of n_rows rows standing at pos[r] and taking frames[r] at `bits` per sample: plan_out[8] = {B, jobs, analyze_threads,
 * analyze_lds, write_lds, pend_pitch, worst, out_bytes} -> 1, 0 when the plan is not ok (nothing written then) */
HOOK int sauAmd_flac_plan_bits(uint32_t block_frames, uint32_t channels, uint32_t bits, size_t n_rows, const uint64_t *pos,
		const uint32_t *frames, int finish, uint64_t *plan_out) {
	using namespace sauplan;
	const uint32_t B = sauflac::flac_block_frames(block_frames);
	if (!B || (channels != 1 && channels != 2)) return 0;
	std::vector<FlacRow> d(n_rows);
	for (size_t r = 0; r < n_rows; ++r) d[r] = plan_flac_row(pos[r], frames[r], B, finish != 0);
	const FlacPlan p = plan_flac(block_frames, channels, n_rows, d.data(), bits);
	if (!p.ok) return 0;
	const uint64_t v[8] = {p.B, p.jobs, p.analyze_threads, p.analyze_lds, p.write_lds, p.pend_pitch, p.worst, p.out_bytes};
	for (int i = 0; i < 8; ++i) plan_out[i] = v[i];
	return 1;
}
