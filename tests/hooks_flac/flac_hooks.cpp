/* flac_hooks.cpp -- TEST INFRASTRUCTURE for tests/test_flac_host.py, without a GPU:
 *   sauAmd_render_file_flac_with_backend  sauAmd_render_file_flac (saugns_amd/csrc/sndout.cpp) over a caller-supplied
 *       sauengine::Backend: its refusals -- a bad argument, a backend without an encoder -- happen before any file is created.
 *   sauAmd_flac_plan                      what launch_plan.h plans for a feed: plan_flac_row per row, plan_flac for all. */
#include "../../saugns_amd/csrc/capi_internal.h"
#include "../../saugns_amd/csrc/sau_dev_ops.h"
#include "../../saugns_amd/csrc/launch_plan.h"
#include <vector>

#define HOOK extern "C" __attribute__((visibility("default")))

HOOK bool sauAmd_render_file_flac_with_backend(const sauProgram *prg, uint32_t srate, const char *path, int channels, uint32_t block_frames,
		void *backend, uint64_t *frames_out, sauAmdFlacInfo *info_out) {
	std::string err;
	sauengine::Backend *be = (sauengine::Backend *)backend;
	const bool ok = sauamd_internal::render_file_flac(prg, srate, path, channels, block_frames,
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

/* a feed of n_rows rows standing at pos[r] and taking frames[r]: rows_out[r][8] = {block0, n_blocks, last_n, pend, pend_next,
 * job0, out_off, the row's worst case}; plan_out[8] = {B, jobs, analyze_threads, analyze_lds, write_lds, pend_pitch, worst,
 * out_bytes} -> 1, 0 when the plan is not ok (nothing written to plan_out then) */
HOOK int sauAmd_flac_plan(uint32_t block_frames, uint32_t channels, size_t n_rows, const uint64_t *pos, const uint32_t *frames, int finish,
		uint64_t *rows_out, uint64_t *plan_out) {
	using namespace sauplan;
	const uint32_t B = sauflac::flac_block_frames(block_frames);
	if (!B || (channels != 1 && channels != 2)) return 0;
	std::vector<FlacRow> d(n_rows);
	for (size_t r = 0; r < n_rows; ++r) d[r] = plan_flac_row(pos[r], frames[r], B, finish != 0);
	const FlacPlan p = plan_flac(block_frames, channels, n_rows, d.data());
	for (size_t r = 0; r < n_rows; ++r) {
		const uint64_t v[8] = {d[r].block0, d[r].n_blocks, d[r].last_n, d[r].pend, d[r].pend_next, d[r].job0, d[r].out_off,
		                       flac_row_worst(d[r], B, channels)};
		for (int i = 0; i < 8; ++i) rows_out[r * 8 + i] = v[i];
	}
	if (!p.ok) return 0;
	const uint64_t v[8] = {p.B, p.jobs, p.analyze_threads, p.analyze_lds, p.write_lds, p.pend_pitch, p.worst, p.out_bytes};
	for (int i = 0; i < 8; ++i) plan_out[i] = v[i];
	return 1;
}
