/* spectrum_hooks.cpp -- TEST INFRASTRUCTURE for tests/test_spectrum_host.py, without a GPU:
 *   sauAmd_render_spectrum_with_backend  sauAmd_render_spectrum (saugns_amd/csrc/sndout.cpp) over a caller-supplied
 *       sauengine::Backend: its refusals -- a bad argument, a backend without a spectrum meter -- happen before anything renders.
 *   sauAmd_spectrum_segment              tables.cpp's restatement of one segment of one channel, with the library's own tables.
 *   sauAmd_spectrum_plan                 what launch_plan.h plans for a feed: plan_spectrum_row per row, plan_spectrum for all. */
#include "../../saugns_amd/csrc/capi_internal.h"
#include "../../saugns_amd/csrc/sau_dev_ops.h"
#include "../../saugns_amd/csrc/launch_plan.h"
#include <vector>

#define HOOK extern "C" __attribute__((visibility("default")))

HOOK bool sauAmd_render_spectrum_with_backend(const sauProgram *prg, uint32_t srate, int factor, int channels, unsigned log2n,
		uint32_t hop, void *backend, double *power_out, uint64_t *segments_out, uint64_t *frames_out) {
	std::string err;
	sauengine::Backend *be = (sauengine::Backend *)backend;
	const bool ok = sauamd_internal::render_spectrum(prg, srate, factor, channels, log2n, hop,
			[&be](std::string &e) -> sauengine::Backend * {
				sauengine::Backend *b = be;
				be = nullptr;
				if (!b) e = "the test hook has one backend only";
				return b;
			}, power_out, segments_out, frames_out, err);
	delete be; /* (a refusal ahead of the render: nothing has taken the backend over) */
	if (!ok) sauamd_internal::set_last_error("output", err);
	return ok;
}

/* x[j * stride], j = 0 .. N-1 -> p[N/2 + 1]; false for log2n outside 8 .. 12 */
HOOK bool sauAmd_spectrum_segment(unsigned log2n, const float *x, size_t stride, double *p) {
	const size_t N = sauengine::spectrum_window(log2n, nullptr, 0);
	if (!N) return false;
	std::vector<double> w(N), tw(N), re(N), im(N);
	sauengine::spectrum_window(log2n, w.data(), N);
	sauengine::spectrum_twiddles(log2n, tw.data(), N);
	return sauengine::spectrum_segment(log2n, w.data(), tw.data(), x, stride, re.data(), im.data(), p);
}

/* a feed of n_rows rows standing at pos[r] and taking frames[r]: rows_out[r][8] = {seg0, n_seg, pend, pend_next, acc_cnt,
 * n_groups, n_complete, 0}; plan_out[8] = {N, bins, max_groups, lds_bytes, pend_pitch, sum_pitch, scratch, rows}
 * -> 1, 0 when the plan is not ok (nothing written to plan_out then) */
HOOK int sauAmd_spectrum_plan(unsigned log2n, uint32_t hop, uint32_t channels, size_t n_rows, const uint64_t *pos, const uint32_t *frames,
		uint64_t *rows_out, uint64_t *plan_out) {
	using namespace sauplan;
	if (!sauengine::spectrum_params_ok((int)channels, log2n, hop)) return 0;
	std::vector<SpecRow> d(n_rows);
	for (size_t r = 0; r < n_rows; ++r) {
		d[r] = plan_spectrum_row(pos[r], frames[r], 1u << log2n, hop);
		const uint64_t v[8] = {d[r].seg0, d[r].n_seg, d[r].pend, d[r].pend_next, d[r].acc_cnt, d[r].n_groups, d[r].n_complete, 0};
		for (int i = 0; i < 8; ++i) rows_out[r * 8 + i] = v[i];
	}
	const SpectrumPlan p = plan_spectrum(log2n, hop, channels, n_rows, d.data());
	if (!p.ok) return 0;
	const uint64_t v[8] = {p.N, p.bins, p.max_groups, p.lds_bytes, p.pend_pitch, p.sum_pitch, p.scratch, p.rows};
	for (int i = 0; i < 8; ++i) plan_out[i] = v[i];
	return 1;
}
