/* wonly_hooks.cpp -- TEST INFRASTRUCTURE for tests/test_inner_wonly_plan.py: the host's "every active voice is wave oscillators
 * with constant amplitude" (SegmentDesc.wave_only, engine.cpp) against the decoded steps and the operators' own state, the
 * planner's choice of the wave-only instantiation of the lane-major inner launch (launch_plan.h: FastPlan.inner_wonly), and the
 * plan cache's key (plan.cpp: voice_plan_shape) beside the flag. No GPU.
 * The backend is tests/seqexec's sequential executor, taken in as it is (this file includes its source: the class lives in an
 * anonymous namespace), with render() looking at the segment first. A library of its own; only tests/ load it. */
#include "../seqexec/seq_backend.cpp"
#include "../../saugns_amd/csrc/capi_internal.h"
#include "../../saugns_amd/csrc/launch_plan.h"
#include <stdlib.h>

#define HOOK extern "C" __attribute__((visibility("default")))

namespace {

/* {segments, segments the host flagged, flagged segments whose steps have the shape, segments whose steps have the shape,
 *  the last segment's flag, the last segment's shape} */
static uint32_t g_wonly[6];

struct WonlyBackend : public SeqBackend {
	explicit WonlyBackend(uint32_t b) : SeqBackend(b) {}
	/* What the wave-only instantiation holds (k_fast_group_lm.h), read from the voice's steps and from the operators as the
	 * executor has them at the segment's start: every step a W oscillator's with its amplitude one value (no amplitude block,
	 * no ramp in progress), nothing layered, no frequency-scaled PM, no frequency or self-modulation block, and no operator that
	 * runs out of time inside the segment (its step then becomes a line of zeros: k_decode.h). */
	bool voice_has_shape(const VoiceDesc &vd) const {
		if (vd.flags & (VD_WIDE | VD_NO_FAST)) return false;
		for (uint32_t si = 0; si < vd.plan_len; ++si) {
			const Step &st = steps[vd.plan_ofs + si];
			const DevOp &op = ops[op_ids[vd.ops_ofs + st.op]];
			/* (a frequency line that is not forced into its block -- no FM -- and holds one value: no step of the
			 * closed-form path) */
			if (st.kind == ST_LINE && st.which == L_FREQ && !(st.flags & SF_FORCE) && !(op.line[L_FREQ].flags & LP_GOAL)) continue;
			if (st.kind != ST_OSC) return false;
			if (st.flags & (SF_LAYER | SF_WAVE_ENV)) return false;
			if (st.amp != NO_SLOT || st.fpm != NO_SLOT || st.sm != NO_SLOT) return false;
			if (st.freq != NO_SLOT && st.freq < FSLOT_BASE) return false; /* (a frequency read from a block that is no frequency slot) */
			/* (self-modulation: a pm_a line that holds or ramps to an amount, or a step that evaluates one) */
			if ((st.flags & SF_SM_INLINE) || op.line[L_PMA].v0 != 0.f || (op.line[L_PMA].flags & LP_GOAL)) return false;
			if (op.line[L_FREQ].flags & LP_GOAL) return false;
			if (op.type != OT_WAVE) return false;
			if (op.line[L_AMP].flags & LP_GOAL) return false;
			if (!(op.flags & OPF_TIME_INF) && op.time < vd.run_len) return false;
		}
		return true;
	}
	bool render(const SegmentDesc &seg, std::string &err) override {
		bool shape = true;
		for (uint32_t v = 0; v < seg.n_voices; ++v) shape = shape && voice_has_shape(seg.voices[v]);
		++g_wonly[0];
		if (seg.wave_only) ++g_wonly[1];
		if (seg.wave_only && shape) ++g_wonly[2];
		if (shape) ++g_wonly[3];
		g_wonly[4] = seg.wave_only ? 1u : 0u; g_wonly[5] = shape ? 1u : 0u;
		return SeqBackend::render(seg, err);
	}
};

} /* namespace */

HOOK void *wonly_backend_create(uint32_t block_len) { return new WonlyBackend(block_len ? block_len : 1024); }
HOOK void wonly_backend_counts(uint32_t *out6, int reset) {
	for (int i = 0; i < 6; ++i) out6[i] = g_wonly[i];
	if (reset) memset(g_wonly, 0, sizeof g_wonly);
}

/* in = a segment's 24 scalars, then lds per CU, CUs, row_stride, pcm_row, f32, max_write, max_rows (tests/hooks_plan), then
 * SegmentDesc.wave_only; the switches come from the environment as the backend reads them.
 * out = {inner, inner_wonly, inner_tab0, inmix_flags, tables in LDS} -> 5, or -1 */
HOOK int sauAmd_inner_wonly_plan(const uint32_t *in, uint32_t n_in, uint32_t *out, uint32_t n_out) {
	using namespace sauplan;
	if (n_in < 32 || n_out < 5) return -1;
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
	seg.wave_only = in[31] != 0;
	const FastPlan k = plan_fast(seg, tun, dev, pi);
	const uint32_t vals[5] = {(uint32_t)k.inner, k.inner_wonly ? 1u : 0u, k.inner_tab0 ? 1u : 0u, k.inmix_flags, k.tabs.n};
	memcpy(out, vals, sizeof vals);
	return 5;
}

/* A voice made by hand -- a W carrier over one modulator -- as the plan cache sees it (plan.cpp): `what` chooses the modulator.
 * 0: a W phase modulator; 1: the same, once given a sweep (OpMirror.goal_seen); 2: an N phase modulator; 3: an R phase modulator;
 * 4: an A phase modulator; 5: the W operator as amplitude modulator; 6: as frequency-scaled phase modulator; 7: two W phase
 * modulators (the second is layered); 8: as 0 with the CARRIER once given a sweep.
 * out = {the key's hash (FNV-1a over the shape's tokens), VoicePlan.wave_only of a fresh compile, tokens} -> 3, or -1 */
HOOK int sauAmd_wonly_key_probe(uint32_t what, unsigned long long *out) {
	using namespace sauengine;
	std::vector<OpMirror> ops(3);
	for (OpMirror &m : ops) { m.inited = true; m.type = SAU_POPT_N_wave; m.time_inf = true; m.line_set = (1u << L_AMP) | (1u << L_FREQ); }
	ops[0].time_inf = false; ops[0].time = 44100;
	struct { uint32_t count; uint32_t ids[2]; } one = {1, {1, 0}}, two = {2, {1, 2}};
	const sauProgramIDArr *l1 = (const sauProgramIDArr *)&one, *l2 = (const sauProgramIDArr *)&two;
	int use = SAU_POP_N_pmod;
	switch (what) {
	case 0: break;
	case 1: ops[1].goal_seen = true; break;
	case 2: ops[1].type = SAU_POPT_N_noise; break;
	case 3: ops[1].type = SAU_POPT_N_raseg; break;
	case 4: ops[1].type = SAU_POPT_N_amp; break;
	case 5: use = SAU_POP_N_amod; break;
	case 6: use = SAU_POP_N_fpmod; break;
	case 7: l1 = l2; break;
	case 8: ops[0].goal_seen = true; break;
	default: return -1;
	}
	ops[0].mods[use] = l1;
	std::vector<uint32_t> tokens, ids, stamp;
	uint64_t wmask = 0;
	if (!voice_plan_shape(ops, 0, tokens, ids, stamp, 1, wmask)) return -1;
	unsigned long long h = 1469598103934665603ull;
	for (uint32_t t : tokens) { h ^= t; h *= 1099511628211ull; }
	VoicePlan plan;
	std::string err;
	if (!compile_voice_plan(ops, 0, plan, err)) return -1;
	out[0] = h; out[1] = plan.wave_only ? 1u : 0u; out[2] = tokens.size();
	return 3;
}
