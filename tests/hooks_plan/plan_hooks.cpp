/* plan_hooks.cpp -- TEST INFRASTRUCTURE: what saugns_amd/csrc/launch_plan.h decides about the inner launch of a closed-form
 * segment (plan_closed_form: which form, FastPlan::inner_lds: its dynamic LDS), for tests/test_inner_plan.py. No GPU, no
 * pointers into the product: the segment comes as the scalars tests/hooks' sauAmd_launch_plan takes, in the same order. */
#include "../../saugns_amd/csrc/capi_internal.h"
#include "../../saugns_amd/csrc/sau_dev_ops.h"
#include "../../saugns_amd/csrc/launch_plan.h"
#include <stdlib.h>
#include <string.h>

#define HOOK extern "C" __attribute__((visibility("default")))

/* in = a segment's 24 scalars (tests/seqexec: seq_backend_last_segment), then lds per CU, CUs, row_stride, pcm_row, f32,
 * max_write, max_rows; the switches come from the environment as the backend reads them.
 * out = {use_fast, main_build, rows, wide_cf, n_fast, tables in LDS, inner, dyn_chunks, the inner launch's LDS bytes, the
 * 12-row wide build's with its block buffers in LDS, bytes of one wide table block, the device's LDS limit} -> 12, or -1 */
HOOK int sauAmd_inner_plan(const uint32_t *in, uint32_t n_in, uint32_t *out, uint32_t n_out) {
	using namespace sauplan;
	if (n_in < 31 || n_out < 12) return -1;
	const Tuning tun = tuning_from_env([](const char *name) -> const char * { return getenv(name); });
	sauengine::SegmentDesc seg;
	memset((void *)&seg, 0, sizeof seg);
	seg.n_main = in[0]; seg.n_fast = in[1]; seg.n_fast_full = in[2]; seg.may_scan = in[3]; seg.serial = in[4];
	seg.len = in[5]; seg.n_voices = in[6]; seg.n_streams = in[7]; seg.n_slots = in[8]; seg.sum_levels = in[9]; seg.max_ops = in[10];
	seg.max_steps = in[11]; seg.n_pan_rows = in[12]; seg.wave_mask = in[13]; seg.maybe_block = in[14]; seg.maybe_cub = in[15];
	seg.n_chain_rows = in[16]; seg.n_inc_rows = in[17]; seg.n_look_rows = in[18]; seg.n_may_scan = in[19]; seg.n_chain_slots = in[20];
	seg.chain_rows_padded = in[21]; seg.stereo = in[22]; seg.pcm_offset = in[23];
	const DeviceLimits dev = device_limits(in[24], in[25], tun);
	PlanInputs pi;
	pi.row_stride = in[26]; pi.pcm_row = in[27]; pi.f32 = in[28]; pi.max_write = in[29]; pi.max_rows = in[30];
	pi.chain_budget = sauengine::chain_rows_budget(0, 0);
	seg.format = pi.f32 ? sauengine::SF_F32 : sauengine::SF_S16;
	const FastPlan k = plan_fast(seg, tun, dev, pi);
	const uint32_t vals[12] = {k.use_fast, (uint32_t)k.main_build, k.rows, k.wide_cf, k.n_fast, k.tabs.n, (uint32_t)k.inner,
		k.tasks.dyn_chunks, (uint32_t)k.inner_lds(), (uint32_t)k.launch_lds(0, 12, true), (uint32_t)FAST_TAB_BYTES_WIDE,
		(uint32_t)dev.lds_limit};
	memcpy(out, vals, sizeof vals);
	return 12;
}
