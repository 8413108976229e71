/* inner_issue_hooks.cpp -- TEST INFRASTRUCTURE: which instantiation of the lane-major inner launch saugns_amd/csrc/launch_plan.h
 * gives a closed-form segment (plan_closed_form: FastPlan.inner_tab0, the one-table form), for tests/test_inner_tab0_plan.py.
 * No GPU, no pointers into the product: the segment comes as the scalars tests/hooks_plan's sauAmd_inner_plan takes, in the same
 * order. A library of its own beside tests/hooks_plan, which it leaves as it is. */
#include "../../saugns_amd/csrc/capi_internal.h"
#include "../../saugns_amd/csrc/sau_dev_ops.h"
#include "../../saugns_amd/csrc/launch_plan.h"
#include <stdlib.h>
#include <string.h>

#define HOOK extern "C" __attribute__((visibility("default")))

/* in = a segment's 24 scalars, then lds per CU, CUs, row_stride, pcm_row, f32, max_write, max_rows (tests/hooks_plan); the
 * switches come from the environment as the backend reads them.
 * out = {inner, tables in LDS, inner_tab0, n_fast, rows, inmix_flags} -> 6, or -1 */
HOOK int sauAmd_inner_tab0_plan(const uint32_t *in, uint32_t n_in, uint32_t *out, uint32_t n_out) {
	using namespace sauplan;
	if (n_in < 31 || n_out < 6) return -1;
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
	const uint32_t vals[6] = {(uint32_t)k.inner, k.tabs.n, k.inner_tab0 ? 1u : 0u, k.n_fast, k.rows, k.inmix_flags};
	memcpy(out, vals, sizeof vals);
	return 6;
}
