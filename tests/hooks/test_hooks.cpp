/* test_hooks.cpp -- TEST INFRASTRUCTURE: the entry points tests/ need beside the product's C ABI, in a library of their
 * own (tests/hooks/libsaugns_amd_hooks.so = the product's object files + this file + kat_kernels.hip). The product library
 * exports none of them (`nm -D saugns_amd/libsaugns_amd.so` is checked by tests/test_host.py).
 *   sauAmd_create_Generator_with_backend / sauAmd_create_Batch_with_backend / sauAmd_render_file_with_backend:
 *     the host control plane, the drop-in generator and the output stage over a caller-supplied sauengine::Backend
 *     (tests/seqexec: the sequential plan executor) -- host logic without a GPU
 *   sauAmd_Generator_rewinds: how often a changed call size / channel layout took a generator's read-ahead back
 *   sauAmd_launch_plan: what saugns_amd/csrc/launch_plan.h decides for a segment given as scalars (no GPU, no pointers)
 *   sauAmd_kat_line_device / _host, sauAmd_kat_div_device: the shared arithmetic as compiled for the device and the host
 *   sauAmd_kat_scan64_device: the kernels' 64-bit wave scan and sum (k_wave_scan.h) over caller-supplied values
 *   sauAmd_kat_round32_device: the 32-bit rounding forms of phases (sau_dev_math.h, k_common.h) on every bit pattern
 *   sauAmd_kat_flac_lpc_orders_host / _device: steps 3 to 5 of the FLAC encoder's LPC mode (sau_flac.h: flac_lpc_orders) on
 *     caller-supplied autocorrelations, with the recursion's work array a[] as bit patterns */
#include "../../saugns_amd/csrc/capi_internal.h"
#include "../../saugns_amd/csrc/sau_dev_ops.h"
#include "../../saugns_amd/csrc/launch_plan.h"
#include "../../saugns_amd/csrc/sau_flac.h"
#include <stdio.h>
#include <string.h>

#define HOOK extern "C" __attribute__((visibility("default")))

#ifndef SAU_HOOKS_NO_HIP
bool kat_div(float a, int variant, unsigned long long *mismatches, uint32_t *first_bad);
bool kat_line(const saudev::LineState &st, uint32_t len, const float *mul, float *out, saudev::LineState *st_out);
bool kat_scan64(const unsigned long long *in, unsigned long long *scan, unsigned long long *sum, uint32_t n_waves);
bool kat_rint64(int scattered, unsigned long long *mismatches, uint32_t *first_bad);
bool kat_round32(int fn, int scattered, unsigned long long *counts, uint32_t *first_bad);
bool kat_flac_lpc_orders(const int64_t *R, const uint32_t *M, uint32_t n, uint32_t *g, uint32_t *mask, int16_t *q, uint8_t *shift,
		uint64_t *a_bits);
#endif

/* Steps 3 to 5 of the LPC mode for n autocorrelations R[v][0 .. 8] with their own largest order M[v] in 1 .. 8, strung together as
 * the analysis does (k_flac.h: flac_analyze_lpc; tables.cpp: flac_encode_block): g, the conversions (double)(R[l] >> g),
 * flac_lpc_orders. -> g[v], mask[v], q[v][(m - 1) * 8 + j] and shift[v][m - 1] where flac_lpc_orders wrote them, and a[0 .. M-1]
 * as it stands behind the call, as bit patterns. What the function does not write keeps what the caller put there. 0 for a bad
 * argument (the _device twin: or a device error). */
HOOK int sauAmd_kat_flac_lpc_orders_host(const int64_t *R /* [n][9] */, const uint32_t *M, uint32_t n, uint32_t *g, uint32_t *mask,
		int16_t *q /* [n][64] */, uint8_t *shift /* [n][8] */, uint64_t *a_bits /* [n][8] */) {
	using namespace sauflac;
	if (!R || !M || !g || !mask || !q || !shift || !a_bits) return 0;
	for (uint32_t v = 0; v < n; ++v)
		if (M[v] < 1 || M[v] > FLAC_LPC_MAX) return 0;
	for (uint32_t v = 0; v < n; ++v) {
		const int64_t *Rv = R + (size_t)v * (FLAC_LPC_MAX + 1);
		double r[FLAC_LPC_MAX + 1], a[FLAC_LPC_MAX];
		g[v] = flac_lpc_f64_shift(Rv[0]);
		for (unsigned l = 0; l <= FLAC_LPC_MAX; ++l) r[l] = (double)(Rv[l] >> g[v]);
		mask[v] = flac_lpc_orders(r, M[v], a, q + (size_t)v * FLAC_LPC_MAX * FLAC_LPC_MAX, shift + (size_t)v * FLAC_LPC_MAX);
		for (unsigned j = 0; j < M[v]; ++j) a_bits[(size_t)v * FLAC_LPC_MAX + j] = flac_f64_bits(a[j]);
	}
	return 1;
}
#ifndef SAU_HOOKS_NO_HIP
HOOK int sauAmd_kat_flac_lpc_orders_device(const int64_t *R, const uint32_t *M, uint32_t n, uint32_t *g, uint32_t *mask, int16_t *q,
		uint8_t *shift, uint64_t *a_bits) {
	if (!R || !M || !g || !mask || !q || !shift || !a_bits) return 0;
	for (uint32_t v = 0; v < n; ++v)
		if (M[v] < 1 || M[v] > sauflac::FLAC_LPC_MAX) return 0;
	return n == 0 || kat_flac_lpc_orders(R, M, n, g, mask, q, shift, a_bits) ? 1 : 0;
}
#endif

HOOK sauGenerator *sauAmd_create_Generator_with_backend(const sauProgram *prg, uint32_t srate, void *backend) {
	return sauamd_internal::make_generator(prg, srate, (sauengine::Backend *)backend);
}
HOOK sauAmdBatch *sauAmd_create_Batch_with_backend(const sauProgram *const *prgs, size_t n, uint32_t srate, void *backend) {
	if (!backend) return nullptr;
	return sauamd_internal::make_batch_over(prgs, n, srate, (sauengine::Backend *)backend);
}
HOOK bool sauAmd_render_file_with_backend(const sauProgram *prg, uint32_t srate, const char *path, int format, int channels,
		void *backend, uint64_t *frames_out) {
	std::string err;
	const bool ok = sauamd_internal::render_file(prg, srate, path, format, channels, (sauengine::Backend *)backend, frames_out, err);
	if (!ok) fprintf(stderr, "error [output]: %s\n", err.c_str());
	return ok;
}
HOOK unsigned sauAmd_Generator_rewinds(const sauGenerator *g) { return sauamd_internal::generator_rewinds(g); }

/* The HIP backend's launch planner on its own. The switches come from the environment as the backend reads them (plain
 * getenv here: no SAU_AMD_TUNE needed). -> values written to `out`, or -1.
 *   what 0: in = a segment's 24 scalars in the order of tests/seqexec's seq_backend_last_segment, then lds per CU, CUs,
 *           row_stride, pcm_row, f32, max_write, max_rows; out = the plans' scalars (tests/test_launch_plan.py names them)
 *   what 1: in = {len}; out = {chunks, short last chunk, cb[0..chunks]} (chain_chunk_bounds)
 *   what 2: in = {d, q...}; out = {q / d by the kernels' udiv_magic with the host's divisor words...} */
HOOK int sauAmd_launch_plan(int what, const uint32_t *in, uint32_t n_in, uint32_t *out, uint32_t n_out) {
	using namespace sauplan;
	const Tuning tun = tuning_from_env([](const char *name) -> const char * { return getenv(name); });
	if (what == 1 && n_in >= 1 && n_out >= 36) {
		const ChainChunks k = chain_chunk_bounds(in[0], tun);
		out[0] = k.n; out[1] = k.short_last;
		for (uint32_t c = 0; c <= k.n; ++c) out[2 + c] = k.cb[c];
		return (int)(3 + k.n);
	}
	if (what == 2 && n_in >= 1 && n_out + 1 >= n_in) {
		const MagicDiv d = magic_div(in[0]);
		for (uint32_t i = 1; i < n_in; ++i) out[i - 1] = magic_quotient(in[i], d);
		return (int)(n_in - 1);
	}
	if (what != 0 || n_in < 31 || n_out < 52) return -1;
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
	const BlockLoopPlan b = plan_block_loop(seg, tun, dev);
	const FastPlan k = plan_fast(seg, tun, dev, pi);
	/* the most LDS any launch of the plan asks for */
	size_t lds = 0;
	auto ask = [&](bool on, size_t bytes) { if (on && bytes > lds) lds = bytes; };
	if (k.use_fast) {
		ask(k.main_build != 2, k.launch_lds(k.main_build, k.rows, k.wide_cf));
		ask(k.main_build == 2, k.launch_lds(0, k.rows_cf, k.wide_cf, true));
		ask(k.main_build == 2, k.launch_lds(2, k.rows, k.wide_look));
		ask(k.main_build == 2, k.launch_lds(1, k.rows_multi > 4 ? 4 : k.rows_multi, false));
		ask(k.lean_on, k.launch_lds(3, k.rows_lean, false));
		ask(k.cub_ok, k.launch_lds(k.main_build == 2 ? 2 : 0, FAST_CUB_ROWS, false));
		ask(true, k.launch_lds(0, k.rows_repair, k.wide_cf, k.main_build == 2));
	}
	const uint32_t vals[52] = {b.ok, b.W, b.T, b.V, b.HB, (uint32_t)b.lds, b.tabs.n, b.ok ? b.grid(seg, k.use_fast) : 0u,
		k.use_fast, (uint32_t)k.main_build, k.rows, k.rows_multi, k.rows_cf, k.rows_lean, k.lean_on, k.tabs.n, k.wide_cf, k.wide_look,
		k.cub_ok, k.look_split, k.scan, k.look, k.look_wpv, k.look_inside, k.look_words_real, k.chains, k.chunks.n, k.chunks.short_last,
		k.duo, k.tailmix, k.queues, k.inmix, (uint32_t)k.inner, k.tasks.dyn_chunks, k.tasks.dyn_static, k.tasks.dyn_small, k.div.m, k.div.s,
		k.grid, k.grid_cf, k.grid_look, k.pass_grid, (uint32_t)lds, (uint32_t)dev.lds_limit,
		(uint32_t)plan_mixer(seg, tun, pi, (pi.pcm_row * (pi.f32 ? 4 : 2)), k.inmix, 0), k.tasks_cf.dyn_chunks, k.tasks_cf.dyn_static,
		k.groups, task_groups(seg, tun), tun.dyn_min_tasks, k.n_want, dev.fk_grid};
	memcpy(out, vals, sizeof vals);
	return 52;
}

/* state = {v0, vt, pos, end, type, flags} as 6 dwords, updated in place */
HOOK int sauAmd_kat_line_host(uint32_t *state, uint32_t len, const float *mul, float *out) {
	saudev::LineState st;
	memcpy(&st, state, sizeof st);
	saudev::LineBlock lb = saudev::line_begin(st, len, mul != nullptr, mul ? mul[0] : 0.f, saudev::lattice_none(), 0);
	for (uint32_t j = 0; j < len; ++j) out[j] = saudev::line_value(lb, j, mul ? mul[j] : 1.f);
	memcpy(state, &st, sizeof st);
	return 1;
}
#ifndef SAU_HOOKS_NO_HIP
HOOK int sauAmd_kat_line_device(uint32_t *state, uint32_t len, const float *mul, float *out) {
	saudev::LineState st, st2;
	memcpy(&st, state, sizeof st);
	if (!kat_line(st, len, mul, out, &st2)) return 0;
	memcpy(state, &st2, sizeof st2);
	return 1;
}
/* for wave id w: how many divisors make div_diff_scale differ from IEEE division (and the first such bit pattern);
 * variant 1 is the uncorrected product a * rcp(b), which the probe must catch; variant 2 is div_f32_normal (the unmodulated
 * rows' division). -1 on a device error. */
HOOK long long sauAmd_kat_div_device(uint32_t wave, int variant, uint32_t *first_bad) {
	unsigned long long m = 0;
	uint32_t fb = 0xffffffffu;
	if (wave >= 12 || !kat_div(sauengine::wave_consts()[wave].diff_scale, variant, &m, &fb)) return -1;
	if (first_bad) *first_bad = fb;
	return (long long)m;
}
/* in[64 * n_waves] -> scan[64 * n_waves] (inclusive per wave), sum[n_waves]; 0 on a device error */
/* rint64() and franssgauss32()'s conversions over every 32-bit pattern (kat_kernels.hip): mismatches, or -1 */
HOOK long long sauAmd_kat_rint64_device(int scattered, uint32_t *first_bad) {
	unsigned long long m = 0;
	uint32_t fb = 0;
	if (!kat_rint64(scattered, &m, &fb)) return -1;
	if (first_bad) *first_bad = fb;
	return (long long)m;
}
/* the 32-bit rounding forms (kat_kernels.hip: kat_round32_kernel, `fn` 0..5) over every 32-bit pattern: counts[3] = mismatches where
 * the form must hold, in the positive and in the negative control range; 0 on a device error */
HOOK int sauAmd_kat_round32_device(int fn, int scattered, unsigned long long *counts, uint32_t *first_bad) {
	if (fn < 0 || fn > 5) return 0;
	return kat_round32(fn, scattered, counts, first_bad) ? 1 : 0;
}
HOOK int sauAmd_kat_scan64_device(const unsigned long long *in, unsigned long long *scan, unsigned long long *sum, uint32_t n_waves) {
	return kat_scan64(in, scan, sum, n_waves) ? 1 : 0;
}
#endif
