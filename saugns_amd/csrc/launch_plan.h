/* launch_plan.h -- what the HIP backend launches for a segment, decided on the host.
 *
 * Plain C++: no HIP, no device, no allocation. Everything here is arithmetic on a SegmentDesc, the tuning switches and four
 * device limits -- rows per pass and LDS budgets, which build of the time-parallel kernels a segment takes, wide or narrow
 * tables, split / duo / inner launches, in-launch mixing, chain chunk boundaries, task sizes, every grid. hip_backend.hip
 * asks for a plan per segment and carries it out (buffers, parameter blocks, launches, events); tests/test_launch_plan.py
 * asks for the same plans without a GPU (tests/hooks/test_hooks.cpp: sauAmd_launch_plan).
 *
 * The measurement comments are the project's memory of why a rule is what it is: they stay with their rule.
 */
#ifndef SAU_LAUNCH_PLAN_H
#define SAU_LAUNCH_PLAN_H

#include "engine.h"
#include "mix_overlap.h"
#include "sau_dev_math.h"
#include <string.h>

namespace sauplan {

using namespace saudev;
using sauengine::SegmentDesc;

/* ---- constants both sides see (the kernel parts of hip_backend.hip take them from here; where a value follows a
 * device-only type, a static_assert there ties the two together) ---- */
#ifndef FK_GRID
#define FK_GRID 256 /* workgroups of a time-parallel launch at most: one per CU (LDS allows no more at T = 4) */
#endif
/* a wave table in the time-parallel kernels' LDS, narrow and wide form (k_fast_types.h: FkTab) */
constexpr uint32_t FAST_TAB_BYTES = (uint32_t)(WAVE_LEN * (sizeof(HerpC23) + sizeof(HerpC01))), FAST_TAB_BYTES_WIDE = 65536u;
constexpr uint32_t FAST_MAX_SCAN = 8;   /* oscillators with running-sum phases per multi-pass voice */
constexpr uint32_t LOOK_LDS_BYTES = FAST_MAX_SCAN * 2 * 64 * sizeof(unsigned long long); /* the look-back rings of a workgroup */
constexpr uint32_t FAST_MAX_LEVELS = 3; /* running sums that depend on running sums: at most that many sum passes
                                         * (FastParams.sum_levels of them are launched for a segment) */
constexpr uint32_t FAST_CUB_ROWS = 4;   /* rows per pass of the builds with the loop tails of `cub` R segments */
/* Decoded steps are kept once per pass that runs them ([list][voice][step]): a pass walks its own list and never
 * loads a step only to find that another pass needs it (the per-step cost of the interpreter is most of a pass). */
constexpr uint32_t FAST_LISTS = 5; /* 0: only / final pass, 1..3: sum passes, 4: chain-input pass */
constexpr uint32_t INMIX_NSMALL = 8; /* short chunks at the end of the closed-form launch's queues: one per XCD (k_fast_types.h: INMIX_NCH1) */
#ifndef SAU_CHAIN_BATCH_FRAMES
#define SAU_CHAIN_BATCH_FRAMES 32
#endif
/* chain_kernel (k_chain.h): frames per lane and batch: what a batch costs beside the recurrence itself (its LDS reads and writes, the bound check
 * of the short rounding form, the barrier) is spread over that many sample steps -- 16: 117 ns per step, 32: see DESIGN.md 4.3 */
constexpr uint32_t CHAIN_BATCH = SAU_CHAIN_BATCH_FRAMES;
constexpr uint32_t CHAIN_IO_WORDS = CHAIN_BATCH * 64; /* one array of one batch */
constexpr uint32_t CHAIN_TAB_BYTES = 65536, CHAIN_TAB_C01 = 32768; /* a wave table in chain_kernel's LDS: [c3, c2] x 2048, then [c1, c0] x 2048 as f64 */
constexpr size_t CHAIN_IO_BYTES = (size_t)(2 * 2 + 2) * CHAIN_IO_WORDS * 4; /* in[2][2] + out[2] */
constexpr size_t MISC_BYTES = 1488;      /* sizeof(Misc), the block loop's per-team record (k_common.h) */
/* a wave table as the block loop stages it: the Hermite coefficients as they are in HBM */
constexpr size_t BLOCK_TAB_BYTES = (size_t)WAVE_LEN * (sizeof(HerpC23) + sizeof(HerpC01));

/* ---- the tuning switches (SAU_AMD_*, looked at only under SAU_AMD_TUNE: engine.h) ---- */
struct Tuning {
	/* block loop */
	int geo = 1;                 /* SAU_AMD_GEOMETRY: "4x4" (1, default: 4 waves x 4 samples per lane) or "8x2" (0) */
	/* voices per segment from which feedback voices get sixteen one-wave teams per workgroup
	 * (0: never; 1: always, also without feedback -- tests) */
	uint32_t multi_min = 256;    /* SAU_AMD_MULTI_MIN */
	uint32_t multi_teams = 16;   /* SAU_AMD_MULTI_TEAMS: 8 or 16 single-wave teams per workgroup */
	/* device limits as set by hand */
	uint32_t fk_grid = 0;        /* SAU_AMD_FK_GRID: 1..FK_GRID (0: what the device has) */
	bool lds_limit_set = false;  /* SAU_AMD_LDS_LIMIT */
	size_t lds_limit = 0;
	/* time-parallel path */
	bool fast = true;            /* SAU_AMD_NO_FAST */
	bool seq = true;             /* SAU_AMD_NO_SEQ: running-sum phases in the time-parallel kernel */
	bool two_pass = true;        /* SAU_AMD_NO_TWO_PASS: ... in two passes where possible */
	bool lookback = true;        /* SAU_AMD_NO_LOOKBACK: single-pass running sums */
	bool inc_rows = true;        /* SAU_AMD_NO_INC_ROWS */
	uint32_t fast_rows = 8;      /* SAU_AMD_FAST_ROWS: 8 (default), 6, 5, 4 or 2 */
	uint32_t look_rows = 8;      /* rows per pass of the single-pass build (SAU_AMD_LOOK_ROWS; 0: no such build, the full one takes every voice) */
	uint32_t look_min_voices = 1;/* SAU_AMD_LOOK_MIN_VOICES: segments with fewer voices keep the several-pass form */
	bool look_no_lds = false, look_withhold = false, look_spread = false; /* SAU_AMD_LOOK_NO_LDS / _WITHHOLD / _SPREAD (FastParams.look_wpv_flags) */
	bool wide_tabs = true;       /* SAU_AMD_NO_WIDE_TABS: closed-form launches with f64 [c1, c0] table entries in LDS */
	bool wide_look = true;       /* SAU_AMD_NO_WIDE_LOOK: ... and the look-back launch */
	uint32_t more_rows = 12;     /* SAU_AMD_MORE_ROWS: 0, 10 or 12 */
	bool repair = true;          /* SAU_AMD_NO_REPAIR */
	bool analyze_lds = true;     /* SAU_AMD_ANALYZE_NO_LDS: analyze_kernel on the records in HBM */
	/* feedback chains */
	bool chain = true;           /* SAU_AMD_NO_CHAIN: feedback recurrences with lanes = voices */
	bool chain_inline = true;    /* SAU_AMD_NO_CHAIN_INLINE: chains fed from their own lines: chain_kernel's feeder waves evaluate them */
	bool chain_early = true;     /* SAU_AMD_NO_EARLY_CHAINS */
	uint32_t chain_chunks = 0;   /* SAU_AMD_CHAIN_CHUNKS: a fixed number of chunks per segment, 1..32 (1: no pipeline; 0: by frames) */
	uint32_t chain_chunk_frames = 16384; /* SAU_AMD_CHAIN_CHUNK_FRAMES, at least 4096 */
	bool short_last_chunk = true;/* SAU_AMD_NO_SHORT_LAST_CHUNK */
	bool chain_alone = false;    /* SAU_AMD_CHAIN_ALONE (hip_backend.hip: chain_alone_lds) */
	bool lean = true;            /* SAU_AMD_NO_LEAN: chains' passes in a build without the several-pass sums */
	uint32_t lean_rows = 6;      /* SAU_AMD_LEAN_ROWS: rows per pass of fast_kernel<T, 3> at most (6, 5 or 4) */
	/* closed-form launches: tasks, queues, mixing */
	bool dyn = true;             /* SAU_AMD_NO_DYN: closed-form launches deal tasks out through a counter */
	uint32_t dyn_groups = 12;    /* row groups per task of a closed-form launch, at least (SAU_AMD_DYN_GROUPS) */
	/* ... and steps x row groups per task, at least (SAU_AMD_DYN_FLOOR), and the tasks per wave from which the queues deal them out
	 * (fewer: a fixed share per wave; SAU_AMD_DYN_MIN_TASKS). Round 6: 48 -> 24 and 4 -> 2, which takes BASELINE config 2 (256 voices of
	 * one step: 20 tasks a voice were 1.25 a wave, so every wave got a sixteenth of a voice, fixed) to the queues: its launch 0.192 ->
	 * 0.163-0.166 ms, the step 0.287 -> 0.259 (floors 4-12 the same, 16: 0.272; profiles/r06_ab.txt [17]) */
	uint32_t dyn_floor = 24;
	uint32_t dyn_min_tasks = 2;
	bool xcd_queues = true;      /* a closed-form launch's tasks come from one queue per XCD, chunk-major (SAU_AMD_NO_XCD_QUEUES: the one counter, voice-major) */
	bool inmix = true;           /* a many-voice stream's closed-form launch mixes its own rows (SAU_AMD_NO_INMIX: the mixer alone) */
	uint32_t inmix_min_voices = 64; /* ... from that many voices on (SAU_AMD_INMIX_MIN_VOICES) */
	uint32_t inmix_min_steps = 2;/* ... of two steps or more (SAU_AMD_INMIX_MIN_STEPS): behind one-step voices (config 2) the launch's mixing
	                              * costs it more than the mixer saves -- step 0.269-0.272 ms with it, 0.258-0.261 without */
	bool inmix_taper = false;    /* SAU_AMD_INMIX_TAPER: the queues' last eight chunks are short ones, so that less is left to mix_kernel. Measured
	                              * slower on config 3 (2.04 -> 2.08 ms per step, the launch 1.91 -> 1.94: profiles/r06_ab.txt): off */
	uint32_t inmix_at = 13;      /* which of a chunk's tasks mix the chunk before: from this many sixteenths into it (SAU_AMD_INMIX_AT) */
	uint32_t inmix_at_lm = 15;   /* ... in the lane-major inner launch with its round-10 forms (FK_LM_SHORT_TASKS): a task mixes a tile of the chunk
	                              * before only if it finds that chunk whole, and at 13 the shorter tasks looked too early (the step 1.1 % slower
	                              * for a launch 7 % shorter). From ONE scan of config 3, ms per step at 9 ... 15: 1.778, 1.778, 1.791, 1.779,
	                              * 1.782, 1.761, 1.741 -- the end of the range; the forms before are slower at 15 than at 13
	                              * (profiles/r10_inner_issue_ab.json). SAU_AMD_INMIX_AT sets both */
	bool inmix_dry = false;      /* SAU_AMD_INMIX_DRY: timing aid (FastParams.inmix_flags bit 4) */
	bool inner = true;           /* the 12-row wide closed-form build as two launches, edges and inner groups (SAU_AMD_NO_INNER: one) */
	bool lanemajor = true;       /* ... its groups between in the lane-major form (SAU_AMD_NO_LANEMAJOR: row-major) */
	bool inner_wonly = true;     /* ... in the wave-only instantiation where the segment says every voice is wave oscillators with constant
	                              * amplitude (SegmentDesc.wave_only; SAU_AMD_NO_INNER_WONLY: the general instantiation, for A/B and tests) */
	bool inner_wonly_force = false; /* SAU_AMD_INNER_WONLY_FORCE (tests): ... whatever the segment says -- the kernel's own guard then sends
	                              * every voice that is not of that shape to the block loop */
	bool duo = true;             /* closed-form and look-back voices of a segment in one launch where there are plenty of both (SAU_AMD_NO_DUO: two launches) */
	uint32_t duo_lw = 0, duo_prio = 0; /* SAU_AMD_DUO_LW (4 bits), SAU_AMD_DUO_PRIO (1: none, 2: 1, 3: 2 (default), 4: 3): FastParams.look_wpv_flags */
	bool tailmix = false;        /* SAU_AMD_TAILMIX: the look-back launch mixes few-voice streams itself. Exact (357 GPU tests with it on), and
	                              * measured slower: BASELINE config 4 4.19 -> 4.26 ms per step -- the launch is issue-bound and pays 0.32 ms for
	                              * the six flops, the clamp and the conversion per frame (and 42 spilled registers), the mixer gives back 0.25
	                              * (profiles/r06_ab.txt). Off; kept for the record */
	/* mixers */
	bool mix_few = true;         /* SAU_AMD_NO_MIX_FEW */
	bool early_mix = true;       /* SAU_AMD_NO_EARLY_MIX: segments with chains in chunks: the mixer follows the final passes chunk by chunk */
	bool mix64 = true;           /* behind a launch that has mixed most tiles itself: the mixer in blocks of 64 frames (SAU_AMD_NO_MIX64: 256) */
	bool poison = false;         /* SAU_AMD_POISON: voice and pan rows filled with 0x3ea5a5a5 ahead of every segment (tests) */
	/* a segment's final mixer on a stream of its own, beside the next segment's set-up launches (mix_overlap.h) */
	bool mix_overlap = true;     /* SAU_AMD_NO_MIX_OVERLAP: the mixer on the main stream, behind the segment's kernels */
	bool mix_overlap_shared = false; /* SAU_AMD_MIX_OVERLAP_SHARED: never a second block of voice and pan rows */
	/* SAU_AMD_MIX_OVERLAP_MB: the second block is asked for only while a segment's voice and pan rows are no more than this. 4 GiB:
	 * BASELINE config 3's rows are 1.81 GB (1024 voices x 441000 frames x 4 bytes; 2.26 GB as the pool rounds them), admitted with
	 * as much again to spare, and under 1.5 % of the device's 288 GB */
	uint32_t mix_overlap_mb = 4096;
	bool mix_overlap_fail = false; /* SAU_AMD_MIX_OVERLAP_FAIL (tests): the second block's allocation fails, by not being asked for */
};

/* The switches as the environment has them, with their clamps. `env`: sauengine::tune_env (a name -> its value or NULL). */
inline Tuning tuning_from_env(const char *(*env)(const char *)) {
	Tuning t;
	auto off = [&](const char *name) { return env(name) == nullptr; }; /* a SAU_AMD_NO_* switch: true while it is not set */
	auto num = [&](const char *name, uint32_t &v) { if (const char *s = env(name)) v = (uint32_t)atoi(s); };
	auto at_least_1 = [&](const char *name, uint32_t &v) { if (const char *s = env(name)) { const int n = atoi(s); v = n >= 1 ? (uint32_t)n : 1u; } };
	const char *wt = env("SAU_AMD_GEOMETRY");
	t.geo = (wt && !strcmp(wt, "8x2")) ? 0 : 1;
	if (const char *mm = env("SAU_AMD_MULTI_MIN")) t.multi_min = (uint32_t)atol(mm);
	if (const char *mt = env("SAU_AMD_MULTI_TEAMS")) t.multi_teams = atoi(mt) == 8 ? 8u : 16u;
	if (const char *fg = env("SAU_AMD_FK_GRID")) { const int n = atoi(fg); if (n >= 1 && n <= (int)FK_GRID) t.fk_grid = (uint32_t)n; }
	if (const char *ll = env("SAU_AMD_LDS_LIMIT")) { t.lds_limit_set = true; t.lds_limit = (size_t)atol(ll); }
	t.fast = off("SAU_AMD_NO_FAST");
	t.seq = off("SAU_AMD_NO_SEQ");
	t.two_pass = off("SAU_AMD_NO_TWO_PASS");
	t.lookback = off("SAU_AMD_NO_LOOKBACK");
	t.inc_rows = off("SAU_AMD_NO_INC_ROWS");
	if (const char *fr = env("SAU_AMD_FAST_ROWS")) {
		const int r = atoi(fr);
		t.fast_rows = r >= 8 ? 8 : r >= 6 ? 6 : r >= 5 ? 5 : r >= 4 ? 4 : 2;
	}
	num("SAU_AMD_LOOK_ROWS", t.look_rows);
	num("SAU_AMD_LOOK_MIN_VOICES", t.look_min_voices);
	t.look_no_lds = !off("SAU_AMD_LOOK_NO_LDS");
	t.look_withhold = !off("SAU_AMD_LOOK_WITHHOLD");
	t.look_spread = !off("SAU_AMD_LOOK_SPREAD");
	t.wide_tabs = off("SAU_AMD_NO_WIDE_TABS");
	t.wide_look = off("SAU_AMD_NO_WIDE_LOOK");
	num("SAU_AMD_MORE_ROWS", t.more_rows);
	t.repair = off("SAU_AMD_NO_REPAIR");
	t.analyze_lds = off("SAU_AMD_ANALYZE_NO_LDS");
	t.chain = off("SAU_AMD_NO_CHAIN");
	t.chain_inline = off("SAU_AMD_NO_CHAIN_INLINE");
	t.chain_early = off("SAU_AMD_NO_EARLY_CHAINS");
	if (const char *cc = env("SAU_AMD_CHAIN_CHUNKS")) { /* pipeline depth of a segment with chains (1: off; default: by frames) */
		const int n = atoi(cc);
		t.chain_chunks = n >= 32 ? 32 : n >= 1 ? (uint32_t)n : 1;
	}
	if (const char *cf = env("SAU_AMD_CHAIN_CHUNK_FRAMES")) { const int n = atoi(cf); if (n >= 4096) t.chain_chunk_frames = (uint32_t)n; }
	t.short_last_chunk = off("SAU_AMD_NO_SHORT_LAST_CHUNK");
	if (const char *ca = env("SAU_AMD_CHAIN_ALONE")) t.chain_alone = atoi(ca) != 0;
	t.lean = off("SAU_AMD_NO_LEAN");
	num("SAU_AMD_LEAN_ROWS", t.lean_rows);
	t.dyn = off("SAU_AMD_NO_DYN");
	at_least_1("SAU_AMD_DYN_GROUPS", t.dyn_groups);
	at_least_1("SAU_AMD_DYN_FLOOR", t.dyn_floor);
	at_least_1("SAU_AMD_DYN_MIN_TASKS", t.dyn_min_tasks);
	t.xcd_queues = off("SAU_AMD_NO_XCD_QUEUES");
	t.inmix = off("SAU_AMD_NO_INMIX");
	num("SAU_AMD_INMIX_MIN_VOICES", t.inmix_min_voices);
	num("SAU_AMD_INMIX_MIN_STEPS", t.inmix_min_steps);
	t.inmix_taper = !off("SAU_AMD_INMIX_TAPER");
	if (const char *ia = env("SAU_AMD_INMIX_AT")) t.inmix_at = t.inmix_at_lm = (uint32_t)atoi(ia) & 15u;
	t.inmix_dry = !off("SAU_AMD_INMIX_DRY");
	t.inner = off("SAU_AMD_NO_INNER");
	t.lanemajor = off("SAU_AMD_NO_LANEMAJOR");
	t.inner_wonly = off("SAU_AMD_NO_INNER_WONLY");
	t.inner_wonly_force = !off("SAU_AMD_INNER_WONLY_FORCE");
	t.duo = off("SAU_AMD_NO_DUO");
	if (const char *lw = env("SAU_AMD_DUO_LW")) t.duo_lw = (uint32_t)atoi(lw) & 15u;
	if (const char *pr = env("SAU_AMD_DUO_PRIO")) t.duo_prio = (uint32_t)atoi(pr) & 7u;
	t.tailmix = !off("SAU_AMD_TAILMIX");
	t.mix_few = off("SAU_AMD_NO_MIX_FEW");
	t.early_mix = off("SAU_AMD_NO_EARLY_MIX");
	t.mix64 = off("SAU_AMD_NO_MIX64");
	t.poison = !off("SAU_AMD_POISON");
	t.mix_overlap = off("SAU_AMD_NO_MIX_OVERLAP");
	t.mix_overlap_shared = !off("SAU_AMD_MIX_OVERLAP_SHARED");
	if (const char *mb = env("SAU_AMD_MIX_OVERLAP_MB")) { const long n = atol(mb); t.mix_overlap_mb = n < 0 ? 0u : n > 0x7fffffffl ? 0x7fffffffu : (uint32_t)n; }
	t.mix_overlap_fail = !off("SAU_AMD_MIX_OVERLAP_FAIL");
	return t;
}

/* ---- what the rules need to know of the device ---- */
struct DeviceLimits {
	size_t lds_limit = 160 * 1024; /* bytes of LDS a workgroup may ask for */
	uint32_t fk_grid = FK_GRID;    /* workgroups of a time-parallel launch at most */
	uint32_t cus = 256;
	bool eight_xcds = true;        /* the device is a whole MI355X */
};
/* From a device's LDS per CU and its CU count. The time-parallel kernels' grids are one 1024-thread workgroup per CU at most:
 * waves that wait for other workgroups' sums (spread look-back launches) need the whole grid resident, so the grid follows the
 * CUs this device really has (a partitioned or CU-masked device has fewer than 256). The per-XCD task queues and the launch's
 * own mixing take chunk k mod 8 for XCD k mod 8 and hand rows from wave to wave through ONE XCD's L2 (k_fast_types.h): only on
 * a device that is the whole MI355X -- 256 CUs = 8 XCDs x 32. A partition (CPX: 32 CUs, one XCD) or a masked device keeps the
 * single counter and mix_kernel */
inline DeviceLimits device_limits(size_t lds_per_cu, uint32_t cus, const Tuning &t) {
	DeviceLimits d;
	d.cus = cus;
	d.eight_xcds = cus == 256;
	d.fk_grid = t.fk_grid ? t.fk_grid : cus < FK_GRID ? cus : FK_GRID;
	d.lds_limit = t.lds_limit_set ? t.lds_limit : lds_per_cu > 160 * 1024 ? (size_t)160 * 1024 : lds_per_cu;
	return d;
}

/* what else of the backend the rules read */
struct PlanInputs {
	uint32_t row_stride = 0;   /* floats per voice row */
	size_t pcm_row = 0;        /* samples per stream's PCM row */
	size_t chain_budget = 0;   /* Backend::chain_rows_budget() */
	bool f32 = false;          /* a float32 run */
	uint32_t max_write = 0;    /* the longest write_len of the segment's streams */
	uint32_t max_rows = 0;     /* the most voices any of them has */
};

/* ---- helpers ---- */
/* which wave tables a launch stages in LDS: the first `max_tabs` of those the segment uses */
struct TableMap {
	uint32_t n = 0;
	int8_t tab_of_wave[12];  /* LDS table index per wave id, or -1 */
	uint8_t wave_of_tab[12];
};
inline TableMap map_tables(uint64_t wave_mask, size_t max_tabs) {
	TableMap m;
	memset(m.wave_of_tab, 0, sizeof m.wave_of_tab);
	for (int wv = 0; wv < 12; ++wv) {
		m.tab_of_wave[wv] = -1;
		if (((wave_mask >> wv) & 1) && m.n < max_tabs) {
			m.tab_of_wave[wv] = (int8_t)m.n;
			m.wave_of_tab[m.n] = (uint8_t)wv;
			++m.n;
		}
	}
	return m;
}
inline size_t tabs_that_fit(size_t limit, size_t fixed, size_t tab_bytes) { return fixed > limit ? 0 : (limit - fixed) / tab_bytes; }
inline uint32_t n_waves_used(uint64_t wave_mask) { return (uint32_t)__builtin_popcountll(wave_mask & 0xffffffffull); }

/* a wave's block buffers in a time-parallel launch: `n_bufs` rows-of-64 x `rows` floats, and a word per step */
inline size_t buf_area(uint32_t n_bufs, uint32_t rows, uint32_t fmax_steps) {
	return (size_t)n_bufs * 64 * rows * sizeof(float) + (size_t)fmax_steps * sizeof(unsigned long long);
}
/* THE fit test of a time-parallel launch: its tables, sixteen waves' buffers, what else the build keeps in LDS (the look-back
 * rings), and 1 KiB for the rest */
inline bool fits_lds(const DeviceLimits &d, size_t n_tabs, size_t tab_bytes, size_t area, size_t extra = 0) {
	return n_tabs * tab_bytes + 16 * area + extra + 1024 <= d.lds_limit;
}
inline uint32_t row_groups(uint32_t len, uint32_t rows) { return (len + (60 * rows) - 1) / (60 * rows); }
/* THE grid of a time-parallel launch: sixteen waves per workgroup, `max_grid` workgroups at most, one at least */
inline uint32_t wave_grid(unsigned long long waves, uint32_t max_grid) {
	const unsigned long long g = (waves + 15) / 16;
	return g > max_grid ? max_grid : g < 1 ? 1u : (uint32_t)g;
}
/* ... with as many waves per voice as it has row groups (up to 64) when voices are few */
inline uint32_t group_grid(uint32_t n_voices, uint32_t groups, uint32_t max_grid) {
	return wave_grid((unsigned long long)n_voices * (groups < 64 ? groups : 64), max_grid);
}
/* 8, 6, 5, 4 or 2 rows per pass */
inline uint32_t fewer_rows(uint32_t t) { return t > 6 ? 6u : t > 5 ? 5u : t > 4 ? 4u : 2u; }
inline uint32_t rows_at_most(uint32_t r) { return r >= 8 ? 8u : r >= 6 ? 6u : r >= 5 ? 5u : r >= 4 ? 4u : 2u; }

/* ---- the block loop ---- */
struct BlockLoopPlan {
	bool ok = true;          /* false: the voice does not fit a workgroup's LDS */
	uint32_t W = 4, T = 4, V = 1;
	bool HB = false;         /* block buffers in HBM (render_kernel<1, 1, 1, true>) */
	size_t team_bytes = 0, lds = 0;
	TableMap tabs;
	/* persistent over the device-built work list. When the host knows of nothing that needs it (no sweeps, FM, feedback or
	 * expiring operators), a token grid still serves the rare dphase == 0 bail-out. */
	uint32_t grid(const SegmentDesc &seg, bool use_fast) const {
		const bool all = seg.maybe_block || !use_fast;
		if (V > 1) {
			const uint32_t full = (seg.n_voices + V - 1) / V;
			return all ? (full < 512 ? full : 512) : 2;
		}
		return all ? (seg.n_voices < 1024 ? seg.n_voices : 1024) : 16;
	}
};
/* Block-loop geometry. Few voices: W waves share one voice (4x4 or 8x2 frames per lane). Many voices: sixteen single-wave
 * teams per workgroup, each with its own voice, so that every CU has 16 voices in flight. */
inline BlockLoopPlan plan_block_loop(const SegmentDesc &seg, const Tuning &tun, const DeviceLimits &dev) {
	BlockLoopPlan p;
	p.W = tun.geo ? 4 : 8; p.T = tun.geo ? 4 : 2;
	auto team_size = [&](uint32_t w, uint32_t t) {
		size_t b = p.HB ? MISC_BYTES + 64 /* (buffers, operator records and steps in HBM) */
			: (size_t)w * 64 * t * sizeof(float) * seg.n_slots + (size_t)seg.max_ops * sizeof(DevOp) +
			MISC_BYTES + (size_t)seg.max_steps * sizeof(Step) + 64;
		return (b + 15) & ~(size_t)15;
	};
	if (tun.multi_min && seg.n_voices >= tun.multi_min && (seg.serial || tun.multi_min == 1)) {
		const size_t need_tab = seg.wave_mask ? BLOCK_TAB_BYTES : 0;
		/* longer blocks amortise the per-step bookkeeping: 255 samples per block measured
		 * 14 % faster than 127 on BASELINE config 5 */
		const uint32_t mt = tun.multi_teams; /* single-wave teams per workgroup: 8 (512 threads: 256 VGPRs each, no scratch) or 16 */
		for (uint32_t t : {4u, 3u, 2u, 1u})
			if (mt * team_size(1, t) + need_tab <= dev.lds_limit) { p.W = 1; p.T = t; p.V = mt; break; }
	}
	/* a voice with very many block buffers: one wave, one frame per lane (256 B per buffer) */
	if (p.V == 1 && team_size(p.W, p.T) > dev.lds_limit) { p.W = 1; p.T = 1; }
	/* more of them than LDS holds (wide plans: graphs nested hundreds of levels deep): the buffers go to HBM */
	if (p.V == 1 && p.W == 1 && team_size(1, 1) > dev.lds_limit) p.HB = true;
	/* LDS budget: slots + operator cache + misc per team, rest for tables */
	p.team_bytes = team_size(p.W, p.T);
	const size_t fixed = p.team_bytes * p.V;
	if (fixed > dev.lds_limit) { p.ok = false; return p; }
	/* keep two workgroups per CU when possible: cap at half the LDS */
	size_t budget = dev.lds_limit / 2 > fixed ? dev.lds_limit / 2 - fixed : 0;
	if (p.V > 1) budget = dev.lds_limit - fixed;
	if (budget < BLOCK_TAB_BYTES && dev.lds_limit - fixed >= BLOCK_TAB_BYTES) budget = BLOCK_TAB_BYTES;
	p.tabs = map_tables(seg.wave_mask, budget / BLOCK_TAB_BYTES);
	p.lds = p.tabs.n * BLOCK_TAB_BYTES + fixed;
	return p;
}

/* ---- feedback chains in chunks ---- */
/* Chunks of about chain_chunk_frames frames (what the first chunk's inputs and the last chunk's final pass take is not
 * overlapped with the chains), 32 at most. Boundaries: multiples of the chain kernel's batch. What follows the last chunk's
 * chains is not overlapped with anything -- its final pass, finalize_kernel, its share of the mixer (which follows the other
 * chunks since round 5) -- so the last chunk is a short one (4096 frames: 0.4 ms of chains, 0.15 ms of final pass behind them
 * instead of 0.5-0.7) */
struct ChainChunks {
	uint32_t n = 1;        /* chunks (more than one: the chains run on a stream of their own) */
	uint32_t cb[34];       /* chunk c is frames [cb[c], cb[c + 1]) */
	bool short_last = false;
};
inline ChainChunks chain_chunk_bounds(uint32_t len, const Tuning &tun) {
	ChainChunks k;
	uint32_t n = tun.chain_chunks ? tun.chain_chunks : (len + tun.chain_chunk_frames - 1) / tun.chain_chunk_frames;
	if (n > 32) n = 32;
	while (n > 1 && len / n < 4096) --n;
	if (n < 1) n = 1;
	k.short_last = !tun.chain_chunks && tun.short_last_chunk && n >= 4 && n < 32 && len > 8 * 4096u;
	const uint32_t tail = k.short_last ? 4096u : 0u;
	const uint32_t body = tail ? (len - tail) & ~255u : len;
	const uint32_t clen0 = ((body + n - 1) / n + 255) & ~255u;
	for (uint32_t c = 0; c <= n; ++c) k.cb[c] = (unsigned long long)c * clen0 < body ? c * clen0 : body;
	if (tail) { ++n; k.cb[n] = len; }
	/* (with the rounded-up chunk length the last body chunks can come out empty -- len 81930 in 20
	 * chunks: cb[19] == cb[20] -- and each would still cost a chain launch, two pass launches and two events) */
	uint32_t m = 0;
	for (uint32_t c = 0; c < n; ++c)
		if (k.cb[c + 1] > k.cb[c]) { k.cb[m] = k.cb[c]; ++m; k.cb[m] = k.cb[c + 1]; }
	if (m) n = m;
	k.n = n;
	return k;
}

/* ---- closed-form tasks ---- */
struct Tasks { uint32_t dyn_chunks = 0, dyn_static = 0, dyn_small = 0; };
/* row groups per task: dyn_groups, or what makes steps x groups reach dyn_floor */
inline uint32_t task_groups(const SegmentDesc &seg, const Tuning &tun) {
	const uint32_t S = seg.max_steps ? seg.max_steps : 1;
	uint32_t G = tun.dyn_groups;
	if (G * S < tun.dyn_floor) G = (tun.dyn_floor + S - 1) / S;
	return G;
}
/* Tasks of a closed-form launch: G row groups each. The counter takes about one add per 12 ns chip-wide (r03: config 3 with
 * tasks of 3 or 4 groups x 4 steps, one add per 8 ns, ran 1.3-1.6x slower), and a task of G groups x S steps keeps a wave for
 * about G x S x 2.2 us, so G x S >= 48 leaves a factor of two; and dealing tasks out only pays when there are several per
 * wave -- a short segment's few tasks go out in fixed strides, one contiguous run of groups per wave (1024 one-operator
 * voices x 44100 frames: 0.15 ms in strides, 0.31 ms through the counter). */
inline Tasks plan_tasks(const SegmentDesc &seg, const Tuning &tun, uint32_t n_groups, uint32_t grid) {
	Tasks q;
	const uint32_t waves = grid * 16;
	const uint32_t G = task_groups(seg, tun);
	const uint32_t k_dyn = (n_groups + G - 1) / G;
	if (tun.dyn && (unsigned long long)seg.n_voices * k_dyn >= (unsigned long long)tun.dyn_min_tasks * waves) {
		q.dyn_chunks = k_dyn ? k_dyn : 1;
		q.dyn_static = 0;
	} else {
		uint32_t k = waves / seg.n_voices;
		if (k > n_groups) k = n_groups;
		q.dyn_chunks = k ? k : 1;
		q.dyn_static = 1;
	}
	return q;
}
/* fixed strides: what `grid` workgroups' waves make per voice, one task per row group at most */
inline Tasks static_tasks(const SegmentDesc &seg, uint32_t n_groups, uint32_t grid) {
	Tasks q;
	uint32_t k = grid * 16 / seg.n_voices;
	if (k > n_groups) k = n_groups;
	q.dyn_chunks = k ? k : 1; q.dyn_static = 1;
	return q;
}
/* d as a divisor for the kernels' udiv_magic (k_fast_voice.h): s = ceil(log2 d), m = floor(2^(32 + s) / d) + 1 - 2^32 */
struct MagicDiv { uint32_t m = 0, s = 0; };
inline MagicDiv magic_div(uint32_t d) {
	MagicDiv q;
	while ((1ull << q.s) < d) ++q.s;
	q.m = (uint32_t)(((1ull << (32 + q.s)) / d) + 1ull - (1ull << 32));
	return q;
}
/* (the host's copy of udiv_magic: tests) */
inline uint32_t magic_quotient(uint32_t q, MagicDiv d) {
	if (d.s == 0) return q;
	const uint32_t t = (uint32_t)(((unsigned long long)q * d.m) >> 32);
	return (t + ((q - t) >> 1)) >> (d.s - 1);
}

/* ---- the time-parallel path ---- */
/* The forms of the lane-major inner launch's wave oscillator (k_fast_voice.h has what each is): defaults here, because the
 * plan depends on them -- with (a) and (c) the launch's tasks are shorter and mix later into a chunk (Tuning.inmix_at_lm). */
#ifndef FK_LM_ONE_PHASE_SET
#define FK_LM_ONE_PHASE_SET 1
#endif
#ifndef FK_LM_TAB0
#define FK_LM_TAB0 0
#endif
#ifndef FK_LM_AHEAD
#define FK_LM_AHEAD 1
#endif
constexpr bool FK_LM_SHORT_TASKS = FK_LM_ONE_PHASE_SET && FK_LM_AHEAD;
/* Round 11, the wave-only instantiation of that launch (k_fast_voice.h: fast_kernel's WONLY; FastPlan.inner_wonly) and the two
 * forms inside it, each behind a macro of its own for A/B (python saugns_amd/build.py --variant NAME DEFS...):
 * FK_LM_WONLY          the instantiation exists and the host picks it (0: every lane-major launch takes the general one)
 * FK_LM_WONLY_ADD3     a PM operator's phases in one three-operand add a sample, base + k inc + offset, the multiples of the
 *                      increment on the scalar side (0: acc += inc, then ph += offset)
 * FK_LM_WONLY_INPLACE  (off: measured, within noise) amplitude and combine written straight to the block's registers or to the row
 *                      store (0: through r[] -- in the small kernel the compiler drops that copy itself: the same counts) */
#ifndef FK_LM_WONLY
#define FK_LM_WONLY 1
#endif
#ifndef FK_LM_WONLY_ADD3
#define FK_LM_WONLY_ADD3 1
#endif
#ifndef FK_LM_WONLY_INPLACE
#define FK_LM_WONLY_INPLACE 0
#endif
enum Inner : uint32_t { INNER_NONE = 0, INNER_ROW_MAJOR = 1, INNER_LANE_MAJOR = 2 };
enum Mixer : uint32_t { MIX_NONE = 0, MIX_FEW_F32, MIX_F32, MIX_FEW, MIX_64, MIX_256 };

struct FastPlan {
	/* rows per pass and what sits in LDS */
	bool use_fast = false;
	bool seq_ok = false;       /* block buffers with frequency blocks: some voice may need the sequential scan */
	bool look_split = false;   /* the single-pass (look-back) build takes the running-sum voices it serves */
	/* build 0: closed-form phases only; 1: every kind of running-sum voice; 2: single-pass voices and closed-form ones */
	int main_build = 0;
	uint32_t fmax_steps = 0, n_fast = 0, n_fast_cf = 0;
	uint32_t rows = 2;         /* rows per pass of the main build */
	uint32_t rows_multi = 2;   /* ... of the full build */
	uint32_t rows_cf = 2;      /* ... of a split segment's closed-form launch */
	uint32_t rows_lean = 4;    /* ... of the build for voices with chains and nothing to scan */
	bool lean_on = false;
	TableMap tabs;
	uint32_t n_want = 0;       /* tables the segment uses */
	bool wide_cf = false;      /* the closed-form launch (and repair_kernel) take wide table blocks */
	bool wide_look = false;    /* ... and so does the look-back launch */
	bool cub_ok = false;
	uint32_t sum_levels = 2;
	/* running sums */
	uint32_t scan_groups = 0;
	bool scan = false;         /* the several-pass form's sums are wanted */
	bool look = false;         /* the look-back launch runs */
	size_t look_words = 0;
	bool look_words_real = false; /* this segment's look-back words in HBM are usable (not the token block) */
	uint32_t look_wpv = 1;     /* the single-pass launch: waves per voice, and whether every voice sits */
	bool look_inside = true;   /* inside one workgroup (LDS rings, no waits across workgroups) */
	uint32_t look_wpv_flags = 0;
	bool inc_rows = false;     /* saved phase increments between the sum pass and the final pass */
	uint32_t inc_stride = 0;
	/* feedback chains */
	bool chains = false;
	uint32_t chain_stride = 0, chain_grid = 0;
	TableMap ctabs;
	ChainChunks chunks;
	uint32_t pass_grid = 0;    /* the time-parallel passes leave the chains' CUs alone while both run */
	bool early_mix = false;
	/* launches */
	bool split_cf = false, duo = false, tailmix = false;
	bool queues = false;       /* the closed-form launch's tasks come from the XCDs' queues */
	bool inmix = false;        /* ... and it mixes its own rows */
	uint32_t inmix_flags = 0;
	MagicDiv div;
	Inner inner = INNER_NONE;
	bool inner_tab0 = false;   /* the lane-major inner launch stages ONE table: the instantiation that reads it at LDS address 0 */
	bool inner_wonly = false;  /* ... every voice is wave oscillators with constant amplitude: the instantiation that holds nothing else */
	Tasks tasks, tasks_cf, tasks_cub;
	uint32_t groups = 0, groups_cf = 0;
	uint32_t grid = 1, grid_cf = 1, grid_look = 1, grid_edge = 1, grid_cub = 1, grid_repair = 1;
	uint32_t rows_repair = 2;

	/* If allocating the chain rows fails, the segment's feedback voices take the block loop, and the lean build goes with them. */
	void drop_chains() { chains = false; lean_on = false; }
	/* LDS bytes of a launch of `build` at `rows` rows per pass (cf: over the closed-form voices' buffers only) */
	size_t launch_lds(int build, uint32_t r, bool wide, bool cf = false) const {
		return tabs.n * (size_t)(wide ? FAST_TAB_BYTES_WIDE : FAST_TAB_BYTES) + 16 * buf_area(cf ? n_fast_cf : n_fast, r, fmax_steps) +
			(build == 2 ? LOOK_LDS_BYTES : 0);
	}
	/* LDS bytes of the inner launch. Row-major: the 12-row wide build's. Lane-major: the table blocks and nothing else -- its block
	 * buffer is registers (k_fast_group_lm.h), and fast_kernel's task loop and mixing tail keep nothing in LDS */
	size_t inner_lds() const {
		return inner == INNER_LANE_MAJOR ? tabs.n * (size_t)FAST_TAB_BYTES_WIDE : launch_lds(0, rows, true);
	}
};

/* Rows per wave and pass: as many as LDS holds beside one wave table (more rows amortise the per-step work: 8 rows measured
 * 8 % faster than 4, 4 rows 28 % faster than 2) -- and which tables. */
inline void plan_rows(FastPlan &p, const SegmentDesc &seg, const Tuning &tun, const DeviceLimits &dev) {
	p.fmax_steps = seg.max_steps < 64 ? seg.max_steps : 64;
	uint32_t FT = tun.fast_rows;
	/* The build with all the running-sum code needs more registers: 8 rows per pass would spill. Where the
	 * single-pass (look-back) build serves, it takes those voices and the closed-form ones at the full rows
	 * per pass, and the full build's launches only see what is left (voices with feedback chains, voices
	 * one wave walks in order). */
	p.look_split = tun.seq && seg.may_scan && tun.two_pass && tun.lookback && tun.look_rows != 0 && seg.n_voices >= tun.look_min_voices;
	if (tun.seq && seg.may_scan && FT > 4 && !p.look_split) FT = 4;
	if (p.look_split && FT > tun.look_rows) FT = rows_at_most(tun.look_rows);
	/* block buffers: without frequency blocks, or with them when some voice may need
	 * the sequential scan (ramped or modulated frequencies) */
	p.seq_ok = tun.seq && seg.may_scan;
	p.n_fast = p.seq_ok && seg.n_fast_full > seg.n_fast ? seg.n_fast_full : seg.n_fast;
	p.n_fast_cf = seg.n_fast;
	p.n_want = n_waves_used(seg.wave_mask);
	auto area_of = [&](uint32_t t) { return buf_area(p.n_fast, t, p.fmax_steps); };
	const size_t look_lds = p.look_split ? LOOK_LDS_BYTES : 0;
	while (FT > 2 && !fits_lds(dev, seg.wave_mask ? 1 : 0, FAST_TAB_BYTES, area_of(FT), look_lds)) FT = fewer_rows(FT);
	{ /* every wave table the segment uses in LDS is worth more than rows per pass (an oscillator whose table
	   * is left out reads it from L2 per sample): fewer rows where that makes them all fit */
		uint32_t t = FT;
		while (t > 4 && !fits_lds(dev, p.n_want, FAST_TAB_BYTES, area_of(t), look_lds)) t = fewer_rows(t); /* (but not below 4 rows: that costs more) */
		if (fits_lds(dev, p.n_want, FAST_TAB_BYTES, area_of(t), look_lds)) FT = t;
	}
	p.use_fast = tun.fast && fits_lds(dev, 0, 0, area_of(FT), look_lds);
	p.rows = FT;
	p.rows_multi = FT > 4 && p.seq_ok ? 4 : FT; /* rows per pass of the full build */
	p.tabs = map_tables(seg.wave_mask, p.use_fast ? tabs_that_fit(dev.lds_limit, 16 * area_of(FT) + look_lds + 1024, FAST_TAB_BYTES) : 0);
	const uint32_t ft = p.tabs.n;
	const bool all_wide_ok = tun.wide_tabs && tun.more_rows && ft > 0 && ft == p.n_want && seg.max_steps >= 2;
	/* Closed-form segments whose tables all sit in LDS in the wide form: more rows per pass where LDS holds them (round 4:
	 * a group's rows are contiguous in time since then, which took the 8-row build from 128 to 114 VGPRs) */
	if (p.use_fast && !p.seq_ok && all_wide_ok && FT == 8)
		for (uint32_t t : {12u, 10u}) /* (14 and 16 rows: hipcc's "requires even aligned vector registers" error on their spills) */
			if (t <= tun.more_rows && fits_lds(dev, ft, FAST_TAB_BYTES_WIDE, area_of(t))) { p.rows = p.rows_multi = t; break; }
	/* the closed-form voices of a segment that may also have look-back voices: a launch of their own (FastParams.vlists) */
	p.split_cf = p.use_fast && p.seq_ok && p.look_split;
	auto area_cf = [&](uint32_t t) { return buf_area(p.n_fast_cf, t, p.fmax_steps); };
	p.rows_cf = 2;
	if (p.split_cf) {
		for (uint32_t t : {8u, 6u, 5u, 4u})
			if (t <= tun.fast_rows && fits_lds(dev, ft, FAST_TAB_BYTES, area_cf(t))) { p.rows_cf = t; break; }
		/* (10 or 12 rows exist in the wide-table form only: where that fits -- the same test as wide_fits below) */
		if (p.rows_cf == 8 && all_wide_ok)
			for (uint32_t t : {12u, 10u})
				if (t <= tun.more_rows && fits_lds(dev, ft, FAST_TAB_BYTES_WIDE, area_cf(t))) { p.rows_cf = t; break; }
	}
	p.cub_ok = p.use_fast && seg.maybe_cub && fits_lds(dev, ft, FAST_TAB_BYTES, area_cf(FAST_CUB_ROWS)) &&
		(!p.look_split || fits_lds(dev, ft, FAST_TAB_BYTES, area_of(FAST_CUB_ROWS), LOOK_LDS_BYTES));
	/* the build for voices with chains and nothing to scan: as many rows per pass as fit beside the tables */
	p.rows_lean = 4;
	for (uint32_t t : {6u, 5u}) /* (decode_kernel lays the slots out for exactly the rows the build has: 4, 5 or 6) */
		if (t <= tun.fast_rows && t <= tun.lean_rows && fits_lds(dev, ft, FAST_TAB_BYTES, area_of(t))) { p.rows_lean = t; break; }
	p.main_build = !p.seq_ok ? 0 : p.look_split ? 2 : 1;
	/* the closed-form build with wide table blocks in LDS (k_fast_types.h: FkTab), at 6, 8, 10 and 12 rows per pass: taken when
	 * every table the segment wants is in LDS and still fits in that form at the launch's rows */
	auto wide_fits = [&](uint32_t rows, size_t area) {
		/* (voices of one step -- flat banks, BASELINE config 2 -- have no modulation to evaluate: fewer VALU
		 * instructions per sample to begin with, and the wider gather costs them 3-4 %) */
		return tun.wide_tabs && (rows == 8 || rows == 6 || rows == 10 || rows == 12) && ft > 0 && ft == p.n_want && seg.max_steps >= 2 &&
			fits_lds(dev, ft, FAST_TAB_BYTES_WIDE, area);
	};
	/* (which form the closed-form launch of this segment takes -- repair_kernel runs in the same layout) */
	p.wide_cf = p.main_build == 2 ? wide_fits(p.rows_cf, area_cf(p.rows_cf)) : p.main_build == 0 && wide_fits(p.rows, area_of(p.rows));
	/* (wide table blocks for the look-back voices too, where they fit beside the buffers at 8 rows: the carrier-FM bank) */
	p.wide_look = tun.wide_tabs && tun.wide_look && p.rows == 8 && ft > 0 && ft == p.n_want &&
		fits_lds(dev, ft, FAST_TAB_BYTES_WIDE, area_of(p.rows), LOOK_LDS_BYTES);
	p.sum_levels = seg.sum_levels >= FAST_MAX_LEVELS ? FAST_MAX_LEVELS : 2u;
}

/* The running sums: the several-pass form's scan words, the single-pass build's look-back words and waves per voice, the saved
 * phase increments. */
inline void plan_sums(FastPlan &p, const SegmentDesc &seg, const Tuning &tun, const DeviceLimits &dev) {
	if (p.seq_ok && tun.two_pass) {
		/* row groups per voice at most: rows hold at least 32 new frames (H <= 32) */
		p.scan_groups = seg.len / (32 * p.rows_multi) + 2;
		/* (the several-pass form's sums: with look-back only voices that have, or may get, feedback chains take it) */
		p.scan = !p.look_split || seg.n_chain_rows;
		p.look = p.look_split && seg.n_look_rows;
	}
	if (p.look) {
		/* Waves per voice of the single-pass build's launch (as many as the voice has row groups, up to 64,
		 * when voices are few). Voices whose waves sit in one workgroup (1, 2, 4, 8 or 16 of them) look back
		 * through rings in LDS and need no words in HBM; only a launch that spreads voices over
		 * neighbouring workgroups does. Those words (8 B x 2 x row groups per running-sum oscillator) are
		 * capped at 1 GiB: beyond that the launch keeps every voice inside a workgroup instead. */
		const uint32_t groups = row_groups(seg.len, p.rows);
		unsigned long long wpv = ((unsigned long long)dev.fk_grid * 16) / seg.n_voices;
		if (wpv > 64) wpv = 64;
		if (wpv > groups) wpv = groups;
		if (wpv < 1) wpv = 1;
		auto is_inside = [&](unsigned long long w) { return w <= 16 && (16 % w) == 0 && !tun.look_no_lds; };
		p.look_words = (size_t)seg.n_look_rows * 2 * p.scan_groups;
		/* the words exist whenever they fit 1 GiB: the kernel then picks the waves per voice from the number of
		 * look-back voices analyze_kernel finds (the host only knows how many there may be) */
		p.look_words_real = p.look_words * sizeof(unsigned long long) <= ((size_t)1 << 30);
		if (!p.look_words_real && !is_inside(wpv) && !tun.look_no_lds)
			wpv = wpv > 16 ? 16 : wpv > 8 ? 8 : wpv > 4 ? 4 : 2;
		p.look_wpv = (uint32_t)wpv;
		p.look_inside = !p.look_words_real && is_inside(wpv);
	}
	/* saved phase increments of running-sum oscillators (sum pass -> final pass), one segment long */
	/* (only voices that take several passes use them -- with look-back those with feedback chains -- and a
	 * bank of thousands of those would ask for gigabytes: beyond 1 GiB the final pass recomputes instead) */
	p.inc_stride = (seg.len + 63) & ~63u;
	p.inc_rows = tun.inc_rows && p.use_fast && p.scan && seg.n_inc_rows && seg.len <= sauengine::CHAIN_SEG &&
		(size_t)seg.n_inc_rows * 2 * p.inc_stride * sizeof(uint32_t) <= ((size_t)1 << 30);
}

/* Feedback chains: a pair of rows per chain in HBM, one segment long (the engine keeps segments with such voices within
 * CHAIN_SEG frames); without them those voices take the block loop. `grid`: the main launches'. */
inline void plan_chains(FastPlan &p, const SegmentDesc &seg, const Tuning &tun, const DeviceLimits &dev, const PlanInputs &in) {
	p.chains = tun.chain && p.use_fast && p.scan && seg.serial && seg.n_chain_rows &&
		seg.len <= sauengine::chain_seg_frames(seg.n_chain_rows, in.chain_budget);
	p.chain_stride = (seg.len + 63) & ~63u;
	p.ctabs = map_tables(seg.wave_mask, tabs_that_fit(dev.lds_limit, CHAIN_IO_BYTES + 1024, CHAIN_TAB_BYTES));
	p.lean_on = p.chains && tun.lean &&
		fits_lds(dev, p.tabs.n, FAST_TAB_BYTES, buf_area(p.n_fast, p.rows_lean, p.fmax_steps)); /* (a tight LDS budget: the full build's rows) */
	p.chain_grid = (seg.n_chain_slots + 63) / 64;
	if (p.chains) p.chunks = chain_chunk_bounds(seg.len, tun);
	p.pass_grid = p.chunks.n > 1 && p.grid + p.chain_grid > dev.fk_grid ? (dev.fk_grid > p.chain_grid + 32 ? dev.fk_grid - p.chain_grid : 32) : p.grid;
	/* the mixer follows the final passes chunk by chunk (k_finish.h: premix_kernel): after the pass over the
	 * row groups that end in chunk c, every frame below the chunk's end less one group's span is written
	 * (a group has at most 64 x 6 frames in the builds that run here) */
	/* (not where a launch BEHIND the chunks still writes voice rows: the closed-form build with the loop tails of
	 * `cub` R segments -- found by round 5's drop-in sweep, 2 programs of 3000; rows that repair_kernel
	 * touches afterwards make the last launch mix everything again: fast_voice notes it in work_count[1]) */
	p.early_mix = tun.early_mix && in.max_write && !p.cub_ok && !(tun.mix_few && in.max_rows <= 8 && seg.n_streams >= 8);
}

/* A split segment (main build 2): the closed-form launch and the look-back launch, or both in one (duo_kernel). */
inline void plan_split(FastPlan &p, const SegmentDesc &seg, const Tuning &tun, const DeviceLimits &dev, const PlanInputs &in) {
	const uint32_t ft = p.tabs.n;
	/* many streams of a few voices (a batch of small scripts): where a stream's last row is a look-back voice's and the
	 * others are closed-form voices', the look-back launch mixes the stream as it stores that row (k_fast_types.h:
	 * FastParams.tail_ok) and mix_few_kernel has nothing left to do (SAU_AMD_TAILMIX; off by default: see Tuning.tailmix) */
	p.tailmix = p.look && p.rows == 8 && tun.tailmix && !in.f32 && in.max_write && !p.cub_ok && seg.len < (1u << 30) &&
		tun.mix_few && in.max_rows <= 8 && seg.n_streams >= 8 && (seg.pcm_offset & 3u) == 0 && (in.pcm_row & 3u) == 0;
	p.groups_cf = row_groups(seg.len, p.rows_cf);
	p.grid_cf = group_grid(seg.n_voices, p.groups_cf, dev.fk_grid);
	/* Both kinds of voice in ONE launch (duo_kernel, k_fast_voice.h; round 6) where both launches would run 8 rows per pass
	 * on narrow tables and the look-back voices' words in HBM exist (a voice then takes as many waves as there are). How
	 * many voices are of which kind only analyze_kernel knows: the kernel splits its waves by the lists' lengths */
	/* (wide_look: the look-back launch would take wide tables: better apart) */
	p.duo = tun.duo && p.look && p.look_words_real && p.rows == 8 && p.rows_cf == 8 && !p.cub_ok && !p.tailmix &&
		!p.wide_look && !p.wide_cf && fits_lds(dev, ft, FAST_TAB_BYTES, buf_area(p.n_fast, p.rows, p.fmax_steps), LOOK_LDS_BYTES);
	p.tasks_cf = plan_tasks(seg, tun, p.groups_cf, p.duo ? (dev.fk_grid + 1) / 2 : p.grid_cf); /* (duo: half a workgroup's waves take closed-form tasks) */
	p.look_wpv_flags = (tun.look_no_lds ? 1u : 0u) | (tun.look_withhold ? 2u : 0u) | (tun.look_spread ? 4u : 0u);
	if (p.duo) p.look_wpv_flags |= (tun.duo_lw << 8) | (tun.duo_prio << 12);
	p.grid_look = wave_grid((unsigned long long)seg.n_voices * (p.look_words_real ? (p.groups < 64 ? p.groups : 64) : p.look_wpv), dev.fk_grid);
}

/* A closed-form segment (nothing to scan): tasks of about eight row groups dealt out by a counter, the XCDs' queues, the
 * launch's own mixing, the inner two-launch form. */
inline void plan_closed_form(FastPlan &p, const SegmentDesc &seg, const Tuning &tun, const DeviceLimits &dev, const PlanInputs &in) {
	if (p.main_build == 0) p.tasks = plan_tasks(seg, tun, p.groups, p.grid);
	/* tasks dealt out by the counter: one queue per XCD, chunk-major (k_fast_types.h) -- 1.80 -> 1.76 ms per config-3
	 * launch against the one counter in voice order */
	p.queues = tun.xcd_queues && dev.eight_xcds && p.main_build == 0 && !p.tasks.dyn_static && p.tasks.dyn_chunks >= 16 && !p.cub_ok;
	if (p.queues) {
		p.inmix_flags = 64u; /* (analyze_kernel has cleared the queues) */
		/* ... whose last eight chunks are short ones (k_fast_types.h: INMIX_NCH1): a quarter of a task's row groups, where the
		 * segment has at least four regular chunks per XCD besides */
		if (tun.inmix_taper) {
			const uint32_t G = task_groups(seg, tun);
			const uint32_t small = G / 4 ? G / 4 : 1;
			if (p.groups >= 32 * G + INMIX_NSMALL * small) {
				p.tasks.dyn_small = small;
				p.tasks.dyn_chunks = (p.groups - INMIX_NSMALL * small + G - 1) / G + INMIX_NSMALL;
			}
		}
		p.div = magic_div(seg.n_voices); /* the voice count as a divisor (k_fast_voice.h: udiv_magic) */
		/* ... and a bank of voices mixed into one stream: the launch mixes its own rows, chunk by chunk behind the rendering;
		 * premix_kernel has the last word. Config 3: 2.056 -> 1.995 ms per step (the launch 1.74 -> 1.87 ms, the mixer
		 * 0.26 -> 0.07 ms) */
		/* (not on a float run: the launch's tiles store int16 -- the 12-row build has no register to spare for another
		 * store form -- so mix_kernel_f32 writes every frame, as under SAU_AMD_NO_INMIX) */
		p.inmix = tun.inmix && !in.f32 && seg.n_streams == 1 && in.max_write && seg.n_voices >= tun.inmix_min_voices &&
			seg.max_steps >= tun.inmix_min_steps && in.row_stride < (1u << 24);
		if (p.inmix)
			p.inmix_flags = 64u | 32u | (seg.stereo ? 1u : 0u) | (seg.swap_bytes ? 2u : 0u) | (tun.inmix_dry ? 4u : 0u) | ((tun.inmix_at & 15u) << 8);
	}
	/* BASELINE config 3's build in two launches (k_fast_voice.h: INNER): every voice's first and last row group by the plain
	 * build, a wave per group; then the groups between by the build that holds only the form without in-segment masks */
	/* (the groups in the lane-major form, k_fast_group_lm.h; SAU_AMD_NO_LANEMAJOR: the row-major one) */
	/* (... which keeps the block buffer in registers: only where the launch's voices share exactly ONE buffer. 12 rows of buffers
	 * fit beside a 64 KiB table only at one buffer on a 160 KiB LDS, so the rule costs no segment the form; it is what the
	 * kernel relies on, said here and not left to the sizes) */
	if (tun.inner && p.main_build == 0 && p.wide_cf && p.rows == 12 && p.tasks.dyn_chunks >= 3)
		p.inner = tun.lanemajor && p.n_fast == 1 ? INNER_LANE_MAJOR : INNER_ROW_MAJOR;
	/* (round 10) ... and a lane-major launch of one table has that table at LDS address 0: the kernel whose table address is the
	 * index alone (k_fast_voice.h: fk_entry's TAB0). Two tables or more: the form that adds the table's base. */
	p.inner_tab0 = p.inner == INNER_LANE_MAJOR && p.tabs.n == 1;
	/* (round 11) ... and one whose voices are all wave oscillators with constant amplitude, by the engine's conservative word
	 * (SegmentDesc.wave_only), takes the instantiation that holds only that (k_fast_voice.h: fast_kernel's WONLY). A voice of
	 * another shape in such a launch would still be rendered right -- the kernel sends it to the block loop -- but slowly:
	 * tests/test_inner_wonly_plan.py holds the flag against the decoded steps. */
	p.inner_wonly = FK_LM_WONLY && p.inner == INNER_LANE_MAJOR && ((tun.inner_wonly && seg.wave_only) || tun.inner_wonly_force);
	if (FK_LM_SHORT_TASKS && p.inmix && p.inner == INNER_LANE_MAJOR) p.inmix_flags = (p.inmix_flags & ~(15u << 8)) | ((tun.inmix_at_lm & 15u) << 8);
	p.grid_edge = wave_grid(2ull * seg.n_voices, dev.fk_grid); /* (two tasks a voice: its first group, its last) */
}

/* Everything the time-parallel path of a segment launches. */
inline FastPlan plan_fast(const SegmentDesc &seg, const Tuning &tun, const DeviceLimits &dev, const PlanInputs &in) {
	FastPlan p;
	plan_rows(p, seg, tun, dev);
	plan_sums(p, seg, tun, dev);
	/* as many waves per voice as it has row groups (up to 64) when voices are few, one CU-filling grid at most */
	p.groups = row_groups(seg.len, p.rows);
	p.grid = group_grid(seg.n_voices, p.groups, dev.fk_grid);
	plan_chains(p, seg, tun, dev, in);
	if (p.use_fast && p.main_build == 2) plan_split(p, seg, tun, dev, in);
	if (p.use_fast && !p.scan) plan_closed_form(p, seg, tun, dev, in);
	/* closed-form voices with the loop tails of `cub` R segments (FastInfo.cub): FAST_CUB_ROWS rows per pass, fixed strides
	 * over the same voices as the closed-form launch */
	const uint32_t g4 = row_groups(seg.len, FAST_CUB_ROWS);
	p.grid_cub = group_grid(seg.n_voices, g4, dev.fk_grid);
	p.tasks_cub = static_tasks(seg, g4, p.grid_cub);
	/* row groups noted for a second evaluation */
	/* (only closed-form voices note any: with split launches they run at rows_cf rows per pass, in the closed-form launch's layout) */
	p.rows_repair = p.main_build == 2 ? p.rows_cf : p.rows;
	p.grid_repair = wave_grid(seg.n_voices, 64);
	return p;
}

/* The mixer behind the segment's kernels. `early_blocks`: 256-frame blocks that launches between the chain chunks have mixed. */
inline Mixer plan_mixer(const SegmentDesc &seg, const Tuning &tun, const PlanInputs &in, size_t pcm_pitch, bool inmix_live,
		uint32_t early_blocks) {
	if (!in.max_write) return MIX_NONE;
	const bool few = tun.mix_few && in.max_rows <= 8 && seg.n_streams >= 8;
	/* mix_few_kernel_f32's 16-byte stores, derived for 4-byte samples: a thread's four frames begin at byte
	 * pcm_pitch * stream + (pcm_offset + i0) * 4 * channels of a 256-byte-aligned block, i0 a multiple of 4 -- aligned
	 * when the pitch is a multiple of 16 bytes and pcm_offset a multiple of 4 (mono), of 2 (stereo: a frame is 8 bytes).
	 * (Its 16-byte row loads are at i0 of the voice rows, whatever pcm_offset is.) */
	const bool few_f32_aligned = (pcm_pitch & 15u) == 0 && (seg.pcm_offset & (seg.stereo ? 1u : 3u)) == 0;
	if (in.f32) return few && few_f32_aligned ? MIX_FEW_F32 : MIX_F32; /* (no launch has mixed anything on a float run) */
	/* many streams of a few voices each: four frames per thread, no tile staging (k_finish.h) */
	if (few && (seg.pcm_offset & 3u) == 0 && (in.pcm_row & 3u) == 0) return MIX_FEW;
	if (inmix_live && !early_blocks && tun.mix64) return MIX_64;
	return MIX_256;
}

/* Where that mixer runs (mix_overlap.h). On the side stream only for the kind of segment measured to gain by it: one whose
 * closed-form launch mixes tiles into the PCM itself (BASELINE config 3's kind). There the join sits in front of that launch, so
 * the mixer runs beside the set-up launches and nothing else. A segment without such a launch has no PCM writer ahead of its own
 * mixer, and the last segment's mixer would run on beside its rendering launches: measured slower in every such workload --
 * BASELINE config 2 1.67e9 -> 0.80e9 frames/s, the carrier-FM bank 1.41e8 -> 1.26e8, config 5 (the mixer beside the next step's
 * chain kernels) 9.8e6 -> 9.4e6, config 4 and the drop-in rate -1 to -2 % (profiles/r09_mix_overlap_ab.json) -- so those keep the
 * serial order. With the launch split into edge and inner groups the two sets get rows of their own while they are small
 * enough and the device gives them (the edge launch then runs beside the mixer too); otherwise they share one block.
 * `rows_bytes`: the segment's voice and pan rows; `second_refused`: the second block's allocation has failed on this backend
 * (shared rows for good). */
inline MixOverlap plan_mix_overlap(const Tuning &tun, const PlanInputs &in, const FastPlan &fk, size_t rows_bytes, bool second_refused) {
	if (!tun.mix_overlap || !in.max_write) return MIXO_OFF; /* (no frame to write: plan_mixer launches nothing) */
	if (!fk.use_fast || fk.scan || !fk.queues || !fk.inmix) return MIXO_OFF;
	if (fk.inner == INNER_NONE || tun.mix_overlap_shared || second_refused || rows_bytes > ((size_t)tun.mix_overlap_mb << 20)) return MIXO_SHARED;
	return MIXO_ALTERNATE;
}

/* ---- level metering (k_levels.h) ----
 * A workgroup of levels_kernel owns LEVELS_WG_SAMPLES consecutive samples of one row -- samples, not frames: the two channels
 * of a stereo row interleave, and an even block start keeps every block's channel parity the same. The number is a constant,
 * never a function of the device: which samples meet in which partial sum, and in which order, is part of the result's bits,
 * and the same rows must give the same bits on any partition of an MI355X. One sweep is the 256 lanes' one 16-byte load each:
 * LEVELS_SWEEP_F32 float or LEVELS_SWEEP_S16 int16 samples; a block is 16 (8) sweeps, four of them in flight per lane.
 * 16384 samples: a 10 s stereo float render of 64 streams is 3456 workgroups of 64 KiB each, thirteen per CU -- enough to hide
 * the tail, and 54 partial records per row for the one thread that folds them. */
constexpr uint32_t LEVELS_THREADS = 256;
constexpr uint32_t LEVELS_SWEEP_F32 = LEVELS_THREADS * 4, LEVELS_SWEEP_S16 = LEVELS_THREADS * 8;
constexpr uint32_t LEVELS_WG_SAMPLES = 16384;
static_assert(LEVELS_WG_SAMPLES % LEVELS_SWEEP_S16 == 0 && LEVELS_WG_SAMPLES % LEVELS_SWEEP_F32 == 0, "a block is whole sweeps (and begins on an even sample, on 16 bytes)");
constexpr uint32_t LEVELS_MAX_ROWS = 65535; /* grid.y */
struct LevelsPlan {
	bool ok = false;      /* false: more rows or blocks than a grid has */
	uint32_t blocks = 0;  /* grid.x of levels_kernel: blocks of the longest row (0: nothing to measure, no launch) */
	uint32_t rows = 0;    /* grid.y */
	uint32_t finish_grid = 0; /* levels_finish_kernel: 64 rows per workgroup */
	size_t parts = 0;     /* partial records: rows * blocks */
};
inline LevelsPlan plan_levels(uint64_t max_frames, uint32_t channels, size_t n_rows) {
	LevelsPlan p;
	const uint64_t samples = max_frames * channels;
	const uint64_t blocks = (samples + LEVELS_WG_SAMPLES - 1) / LEVELS_WG_SAMPLES;
	if (n_rows > LEVELS_MAX_ROWS || blocks > 0x7fffffffull || max_frames > (~(uint64_t)0 >> 2)) return p;
	p.ok = true;
	p.blocks = (uint32_t)blocks;
	p.rows = (uint32_t)n_rows;
	p.finish_grid = (uint32_t)((n_rows + 63) / 64);
	p.parts = (size_t)n_rows * (size_t)blocks;
	return p;
}

/* ---- the decimator (k_decimate.h) ----
 * A workgroup of decimate_kernel -- one wave -- owns DECIM_TILE consecutive output frames of one stream, both channels of a
 * stereo row: lane l computes the DECIM_PER_LANE frames l, l + 64, ... of the tile, each channel of each in an f64 chain of
 * its own (four chains on a mono row, eight on a stereo one). The tile is a constant, as LEVELS_WG_SAMPLES is and never a
 * function of the device; unlike there no sum is shared between lanes, so it decides speed only, not bits. The tile's input
 * span in LDS is (DECIM_TILE + 2 * DECIM_HALF) * K frames: 320 * K * channels floats, 20 KiB at K = 8 stereo.
 * 256 frames: a 10 s render at 44.1 kHz is 1723 workgroups per stream, seven one-wave workgroups per CU. */
constexpr uint32_t DECIM_THREADS = 64, DECIM_PER_LANE = 4;
constexpr uint32_t DECIM_TILE = 256;
static_assert(DECIM_TILE == DECIM_THREADS * DECIM_PER_LANE, "a lane's frames are DECIM_THREADS apart");
constexpr uint32_t DECIM_HALF = (uint32_t)sauengine::DECIM_HALF; /* H: the filter's half-length, and its latency, in output frames */
constexpr uint32_t DECIM_SPAN_Q = DECIM_TILE + 2 * DECIM_HALF; /* input frames of one phase in a tile's span */
constexpr uint32_t DECIM_CARRY_THREADS = 256; /* decimate_carry_kernel: one workgroup per stream, four floats per thread */
constexpr uint32_t DECIM_MAX_STREAMS = 65535; /* grid.y */
struct DecimPlan {
	bool ok = false;       /* false: a factor that is not 2, 4 or 8, channels not 1 or 2, more streams or tiles than a grid has */
	uint32_t tiles = 0;    /* grid.x of decimate_kernel (0: no output frame, no launch) */
	uint32_t streams = 0;  /* grid.y, and decimate_carry_kernel's grid.x */
	uint32_t taps = 0;     /* L = 2 * H * K + 1 */
	uint32_t hist_floats = 0; /* a stream's history: (L - 1) * channels */
	uint32_t lds_bytes = 0;   /* the span of one tile */
	size_t out_pitch = 0;  /* bytes between the output rows: buf_len * channels samples, rounded up to 256 */
};
inline DecimPlan plan_decimate(uint64_t buf_len, int factor, uint32_t channels, size_t n_streams, size_t sample_bytes) {
	DecimPlan p;
	if ((factor != 2 && factor != 4 && factor != 8) || (channels != 1 && channels != 2) || n_streams > DECIM_MAX_STREAMS) return p;
	const uint64_t tiles = (buf_len + DECIM_TILE - 1) / DECIM_TILE;
	if (tiles > 0x7fffffffull || buf_len * (uint64_t)factor > 0xffffffffull) return p;
	p.ok = true;
	p.tiles = (uint32_t)tiles;
	p.streams = (uint32_t)n_streams;
	p.taps = 2 * DECIM_HALF * (uint32_t)factor + 1;
	p.hist_floats = (p.taps - 1) * channels;
	p.lds_bytes = DECIM_SPAN_Q * (uint32_t)factor * channels * (uint32_t)sizeof(float);
	p.out_pitch = ((size_t)buf_len * channels * sample_bytes + 255) & ~(size_t)255;
	return p;
}
static_assert(2 * DECIM_HALF * 8 * 2 <= DECIM_CARRY_THREADS * 4, "decimate_carry_kernel: a stream's longest history, four floats per thread");

/* ---- loudness and true peak (k_loudness.h) ----
 * The K-weighting recurrence is made parallel over chunks of LOUD_CHUNK frames: a lane of loud_chunk_kernel owns one chunk of
 * one (stream, channel). The chunk is part of the result's bits (include/saugns_amd.h: which frames meet in which partial
 * sum, and where the state is propagated by the 4x4 map instead of frame by frame), so it is a constant and never a function
 * of the device. A workgroup -- one wave -- owns LOUD_WG_CHUNKS consecutive chunks of one stream and stages them through LDS
 * LOUD_SUB frames of every chunk at a time: 8 KiB (mono) or 16 KiB (stereo) per step, rows padded by one access width.
 * The true-peak kernel is laid out like decimate_kernel: a one-wave workgroup owns TP_TILE consecutive frames of one stream,
 * lane l the TP_PER_LANE frames l, l + 64, ...; its span in LDS is the tile and TP_LEAD frames ahead of it (TP_HIST = 31 of
 * them are read: the 4x interpolator's 32 taps per phase; 32 are staged and carried so that every 16-byte vector is aligned).
 * Unlike the chunk, the tile decides speed only: a maximum over bit patterns has no order. */
constexpr uint32_t LOUD_CHUNK = 256;
constexpr uint32_t LOUD_THREADS = 64, LOUD_WG_CHUNKS = LOUD_THREADS, LOUD_SUB = 32;
static_assert(LOUD_CHUNK % LOUD_SUB == 0 && LOUD_SUB % 4 == 0, "a chunk is whole sub-tiles of whole 16-byte vectors");
constexpr uint32_t LOUD_MIN_RATE = sauengine::LOUD_MIN_RATE;  /* 2560: hop = rate / 10 >= LOUD_CHUNK: a chunk never touches more than two hops */
constexpr uint32_t TP_FACTOR = 4, TP_HALF = 16, TP_TAPS = 2 * TP_HALF * TP_FACTOR + 1; /* 129 taps g[], 32 per phase */
constexpr uint32_t TP_HIST = 2 * TP_HALF - 1, TP_LEAD = 2 * TP_HALF;
static_assert(TP_TAPS == sauengine::TP_TAPS && TP_LEAD == sauengine::TP_LEAD, "engine.h: the host's copies");
constexpr uint32_t TP_THREADS = 64, TP_PER_LANE = 4, TP_TILE = TP_THREADS * TP_PER_LANE;
constexpr uint32_t LOUD_MAX_ROWS = 65535; /* grid.y */
struct LoudPlan {
	bool ok = false;          /* false: channels not 1 or 2, a rate below LOUD_MIN_RATE, more rows or frames than a grid has */
	uint32_t hop = 0;         /* frames of a 100 ms hop: rate / 10 */
	uint32_t chunks = 0;      /* chunks of the longest row (0: nothing to measure, no launch) */
	uint32_t chunk_grid = 0;  /* grid.x of loud_chunk_kernel: LOUD_WG_CHUNKS chunks per workgroup */
	uint32_t tiles = 0;       /* grid.x of truepeak_kernel */
	uint32_t rows = 0;        /* grid.y of both, and the lanes of the scan and finish kernels */
	uint32_t lane_grid = 0;   /* loud_scan_kernel (a lane per row and channel) and loud_finish_kernel: 64 lanes per workgroup */
	uint32_t lds_bytes = 0;   /* of loud_chunk_kernel */
};
inline LoudPlan plan_loudness(uint64_t max_frames, uint32_t channels, size_t n_rows, uint32_t srate) {
	LoudPlan p;
	if ((channels != 1 && channels != 2) || srate < LOUD_MIN_RATE || n_rows > LOUD_MAX_ROWS || max_frames > 0xffffffffull) return p;
	p.ok = true;
	p.hop = srate / 10;
	p.chunks = (uint32_t)((max_frames + LOUD_CHUNK - 1) / LOUD_CHUNK);
	p.chunk_grid = (p.chunks + LOUD_WG_CHUNKS - 1) / LOUD_WG_CHUNKS;
	p.tiles = (uint32_t)((max_frames + TP_TILE - 1) / TP_TILE);
	p.rows = (uint32_t)n_rows;
	p.lane_grid = (uint32_t)((n_rows * 2 + 63) / 64);
	p.lds_bytes = LOUD_WG_CHUNKS * (LOUD_SUB * channels + channels) * (uint32_t)sizeof(float);
	return p;
}

/* ---- the limiter (k_limiter.h) ----
 * Two passes over a run of one stream, both in tiles that decide speed only: the limiter's output is a function of the input
 * sequence alone (include/saugns_amd.h, section "Limiter"), every value of it has one accumulator of its own, and a maximum
 * has no order. With A the look-ahead in frames and n output frames, position u of a stream's scratch, u = 0 .. n + 4A - 1,
 * belongs to the sequence's frame k = first + u - 4A - 16, where `first` is the frame of output 0 plus D = 2A + 16:
 * lim_env_kernel gives s[k] and r[k] there, and output frame o reads s over u = o .. o + 4A and r at u = o + 2A.
 * lim_env_kernel: a workgroup of LIM_THREADS owns LIM_ENV_TILE positions; its span in LDS is the tile and TP_LEAD frames
 * around it, channels apart. lim_gain_kernel: a workgroup owns LIM_TILE output frames, LIM_PER_LANE f64 chains per lane;
 * its s span is LIM_TILE + 4A doubles -- 36 KiB at A = LIM_A_MAX, inside the static 64 KiB -- in which the sliding maximum
 * is formed in place. LIM_HIST = 4A + 32 frames of every stream are carried from run to run. */
constexpr uint32_t LIM_A_MIN = sauengine::LIM_A_MIN, LIM_A_MAX = sauengine::LIM_A_MAX;
constexpr uint32_t LIM_THREADS = 256, LIM_PER_LANE = 2, LIM_TILE = LIM_THREADS * LIM_PER_LANE;
constexpr uint32_t LIM_ENV_TILE = LIM_THREADS;
constexpr uint32_t LIM_SPAN_MAX = LIM_TILE + 4 * LIM_A_MAX; /* doubles of lim_gain_kernel's LDS */
constexpr uint32_t LIM_SPAN_PER_THREAD = (LIM_SPAN_MAX + LIM_THREADS - 1) / LIM_THREADS;
static_assert(LIM_SPAN_MAX * sizeof(double) <= 65536, "lim_gain_kernel's span is static LDS");
constexpr uint32_t LIM_MAX_STREAMS = 65535; /* grid.y */
struct LimitPlan {
	bool ok = false;        /* false: rate 0, channels not 1 or 2, more streams or frames than a grid has */
	uint32_t A = 0, D = 0;  /* look-ahead and delay in frames */
	uint32_t taps = 0;      /* 2A + 1: the smoothing window, and the hold */
	uint32_t hist_frames = 0; /* 4A + 32: a stream's history */
	uint32_t env_n = 0;     /* positions of a stream's scratch: frames + 4A (0: no output frame, no launch) */
	uint32_t env_tiles = 0; /* grid.x of lim_env_kernel */
	uint32_t tiles = 0;     /* grid.x of lim_gain_kernel, and the stride of its partial records */
	uint32_t streams = 0;   /* grid.y of both */
	uint32_t span = 0;      /* doubles of a gain tile's s span: LIM_TILE + 4A */
	size_t scratch_pitch = 0; /* doubles between the streams' rows of s and of r: env_n rounded up to 32 */
	size_t out_pitch = 0;   /* bytes between the output rows: frames * channels samples, rounded up to 256 */
};
inline LimitPlan plan_limit(uint64_t frames, uint32_t srate, uint32_t channels, size_t n_streams, size_t sample_bytes) {
	LimitPlan p;
	if (!srate || (channels != 1 && channels != 2) || n_streams > LIM_MAX_STREAMS || frames > 0xffffffffull - 4 * LIM_A_MAX) return p;
	p.ok = true;
	p.A = srate / 200 < LIM_A_MIN ? LIM_A_MIN : srate / 200 > LIM_A_MAX ? LIM_A_MAX : srate / 200; /* (engine.h: limiter_lookahead) */
	p.D = 2 * p.A + 16;
	p.taps = 2 * p.A + 1;
	p.hist_frames = 4 * p.A + 32;
	p.streams = (uint32_t)n_streams;
	p.span = LIM_TILE + 4 * p.A;
	if (frames) {
		p.env_n = (uint32_t)frames + 4 * p.A;
		p.env_tiles = (p.env_n + LIM_ENV_TILE - 1) / LIM_ENV_TILE;
		p.tiles = (uint32_t)((frames + LIM_TILE - 1) / LIM_TILE);
	}
	p.scratch_pitch = ((size_t)p.env_n + 31) & ~(size_t)31;
	p.out_pitch = ((size_t)frames * channels * sample_bytes + 255) & ~(size_t)255;
	return p;
}

/* ---- the spectrum meter (k_spectrum.h) ----
 * A feed of one row: the row stood at `pos` frames and takes `frames` more. With S(P) = 0 for P < N, else (P - N) / hop + 1,
 * the feed completes the segments [S(pos), S(pos + frames)); segment s covers the frames [s hop, s hop + N), of which those
 * below pos are the row's pending frames -- the pos - S(pos) hop (< N) frames from S(pos) hop on -- and the rest lie in the fed
 * row. Group g holds the segments [16 g, 16 g + 16): the feed touches the groups g0 = S(pos) / 16 .. (S(pos + frames) - 1) / 16,
 * one workgroup of spec_segment_kernel per (group, row, channel); the first continues the carried accumulator when S(pos) is no
 * multiple of 16, and spec_finish_kernel adds the groups that are complete behind the feed into the total in ascending g and
 * keeps the last one as the carried accumulator when it is not. All of it is a function of (pos, frames, N, hop): the sums
 * never depend on how a sequence was cut into feeds, on the grid or on the device. */
constexpr uint32_t SPEC_THREADS = 256, SPEC_GROUP = sauengine::SPEC_GROUP;
constexpr uint32_t SPEC_MAX_ROWS = 65535;            /* grid.y */
constexpr uint64_t SPEC_MAX_SCRATCH = 1ull << 27;    /* doubles of one feed's group sums (1 GiB): a longer feed is made in pieces */
struct SpecRow { /* (what the kernels read of a row's feed: uploaded as it stands) */
	uint64_t seg0;        /* S(pos): the first segment this feed completes */
	uint32_t n_seg;       /* how many it completes */
	uint32_t pend;        /* pending frames ahead of the feed: pos - seg0 * hop */
	uint32_t pend_next;   /* ... and behind it */
	uint32_t acc_cnt;     /* segments in the carried accumulator: seg0 % 16 */
	uint32_t n_groups;    /* groups this feed touches (0: no segment) */
	uint32_t n_complete;  /* the first so many of them are complete behind the feed */
};
static_assert(sizeof(SpecRow) == 32, "SpecRow is uploaded as it stands");
inline SpecRow plan_spectrum_row(uint64_t pos, uint32_t frames, uint32_t N, uint32_t hop) {
	SpecRow r;
	const uint64_t s0 = sauengine::spectrum_segments(pos, N, hop), s1 = sauengine::spectrum_segments(pos + frames, N, hop);
	r.seg0 = s0;
	r.n_seg = (uint32_t)(s1 - s0);
	r.pend = (uint32_t)(pos - s0 * hop);
	r.pend_next = (uint32_t)(pos + frames - s1 * hop);
	r.acc_cnt = (uint32_t)(s0 % SPEC_GROUP);
	r.n_groups = s1 > s0 ? (uint32_t)((s1 - 1) / SPEC_GROUP - s0 / SPEC_GROUP + 1) : 0;
	r.n_complete = s1 > s0 ? (uint32_t)(s1 / SPEC_GROUP - s0 / SPEC_GROUP) : 0;
	return r;
}
struct SpectrumPlan {
	bool ok = false;          /* false: log2n, hop or channels out of range, no row or more than a grid has, a feed too long */
	uint32_t N = 0, bins = 0; /* 2^log2n; N / 2 + 1 */
	uint32_t rows = 0, channels = 0;
	uint32_t max_groups = 0;  /* grid.x of spec_segment_kernel, and the groups' stride in the scratch (0: no launch) */
	size_t lds_bytes = 0;     /* spec_segment_kernel's dynamic LDS: re and im, 16 N bytes */
	size_t pend_pitch = 0;    /* floats between the rows' pending frames: N * channels */
	size_t sum_pitch = 0;     /* doubles between the rows' sums: bins * channels */
	size_t scratch = 0;       /* doubles of the groups' sums: rows * channels * max_groups * bins */
};
/* rows: the feed's records (NULL: none, the meter's own sizes only) */
inline SpectrumPlan plan_spectrum(unsigned log2n, uint32_t hop, uint32_t channels, size_t n_rows, const SpecRow *rows) {
	SpectrumPlan p;
	if (!sauengine::spectrum_params_ok((int)channels, log2n, hop) || !n_rows || n_rows > SPEC_MAX_ROWS) return p;
	p.N = 1u << log2n; p.bins = p.N / 2 + 1;
	p.rows = (uint32_t)n_rows; p.channels = channels;
	for (size_t r = 0; rows && r < n_rows; ++r)
		if (rows[r].n_groups > p.max_groups) p.max_groups = rows[r].n_groups;
	p.lds_bytes = (size_t)p.N * 2 * sizeof(double);
	p.pend_pitch = (size_t)p.N * channels;
	p.sum_pitch = (size_t)p.bins * channels;
	const uint64_t sc = (uint64_t)n_rows * channels * p.max_groups * p.bins;
	if (sc > SPEC_MAX_SCRATCH) return p;
	p.scratch = (size_t)sc;
	p.ok = true;
	return p;
}

/* ---- the FLAC encoder (k_flac.h) ----
 * A feed of one row: the row stood at `pos` frames and takes `frames` more. Block k covers the frames [k B, k B + B); the feed
 * completes the blocks [pos / B, (pos + frames) / B), and with `finish` the frames behind the last complete block, if there
 * are any, as one more short block. Of what a block covers, the frames below pos are the row's pending frames -- the pos mod B
 * frames from (pos / B) B on -- and the rest lie in the fed row. The feed's blocks of all rows are numbered through as jobs, row
 * after row: one workgroup of flac_analyze_kernel and of flac_write_kernel per job (they find their row by bisection of job0),
 * one of flac_scan_kernel per row. A row's frames of one feed lie back to back from out_off on in the feed's output, which has
 * room for every block at its bound: flac_frame_bound. All of it is a function of (pos, frames, B, finish): the bytes never
 * depend on how a sequence was cut into feeds, on the grid or on the device. */
constexpr uint32_t FLAC_THREADS = 256;               /* flac_write_kernel, flac_scan_kernel, flac_carry_kernel */
constexpr uint64_t FLAC_MAX_JOBS = 1ull << 24;       /* blocks of one feed: a longer feed is made in pieces */
struct FlacRow { /* (what the kernels read of a row's feed: uploaded as it stands) */
	uint64_t block0;      /* pos / B: the first block this feed completes */
	uint32_t n_blocks;    /* how many it completes */
	uint32_t last_n;      /* frames of the last of them: B, or fewer for the short block of a finish */
	uint32_t pend;        /* pending frames ahead of the feed: pos - block0 * B */
	uint32_t pend_next;   /* ... and behind it (0 behind a finish) */
	uint32_t job0;        /* the blocks of the rows before this one (plan_flac) */
	uint32_t out_off;     /* where the row's frames begin in the feed's output (plan_flac); a multiple of 16 */
};
static_assert(sizeof(FlacRow) == 32, "FlacRow is uploaded as it stands");
inline FlacRow plan_flac_row(uint64_t pos, uint32_t frames, uint32_t B, bool finish) {
	FlacRow r;
	const uint64_t end = pos + frames, b0 = pos / B, full = end / B;
	const uint32_t rem = (uint32_t)(end - full * B);
	const bool tail = finish && rem;
	r.block0 = b0;
	r.n_blocks = (uint32_t)(full - b0) + (tail ? 1 : 0);
	r.last_n = tail ? rem : B;
	r.pend = (uint32_t)(pos - b0 * B);
	r.pend_next = finish ? 0 : rem;
	r.job0 = 0; r.out_off = 0;
	return r;
}
/* the worst case of a row's feed (include/saugns_amd.h, FLAC: the bound of every block it completes, summed) */
inline uint64_t flac_row_worst(const FlacRow &r, uint32_t B, uint32_t channels, unsigned bits = 16) {
	if (!r.n_blocks) return 0;
	return (uint64_t)(r.n_blocks - 1) * sauflac::flac_frame_bound(B, channels, bits) + sauflac::flac_frame_bound(r.last_n, channels, bits);
}
/* flac_analyze_kernel's static LDS beside the staged block (k_flac.h): the finest partitions' sums [4][16 * nk] of 8 bytes, the
 * nodes' costs and parameters [4][32], the four candidates' records, and in the LPC build FlacLpcLds -- counted for every
 * encoder, whatever its order. With the staged block it has to fit the 64 KiB of a workgroup: 52096 bytes at 24 bits, B = 4096,
 * stereo. */
constexpr size_t FLAC_LPC_LDS = 4 * ((sauflac::FLAC_LPC_MAX + 1) * 8 + sauflac::FLAC_LPC_MAX * 8 + sauflac::FLAC_LPC_MAX * sauflac::FLAC_LPC_MAX * 2 +
		sauflac::FLAC_LPC_MAX + 4);
constexpr size_t FLAC_LDS_MAX = 65536;
constexpr size_t flac_analyze_static_lds(unsigned bits) {
	return 4 * sauflac::FLAC_FINE * sauflac::flac_nk(bits) * 8 + 4 * 32 * 8 + 4 * 32 + 4 * sizeof(sauflac::FlacSub) + FLAC_LPC_LDS;
}
struct FlacPlan {
	bool ok = false;           /* false: B or channels not allowed, no row or more than 65535, a block number beyond 2^31 - 1, a feed
	                            * with more than FLAC_MAX_JOBS blocks or a worst case above FLAC_MAX_UNREAD */
	uint32_t B = 0, rows = 0, channels = 0;
	uint32_t jobs = 0;         /* grid.x of flac_analyze_kernel and flac_write_kernel (0: no launch) */
	uint32_t analyze_threads = 0; /* one wave per candidate channel: 64 mono; 256 stereo (L, R, M, S) */
	size_t analyze_lds = 0;    /* the block's frames as words, one more per 32 (k_flac.h: flac_ix); at 24 bits a word per sample */
	size_t write_lds = 0;      /* ... and the frame under construction: its bound, in words, and two more */
	size_t pend_pitch = 0;     /* samples (int16; int32 at 24 bits) between the rows' pending frames: B * channels */
	uint64_t worst = 0;        /* the feed's worst case: what the 1 GiB rule counts */
	size_t out_bytes = 0;      /* the feed's output: every row's worst case, each rounded up to 16 */
};
/* rows: the feed's records (NULL: none, the encoder's own sizes only); job0 and out_off are filled in. bits: 16, or 24 for the
 * wide kernels -- a word per sample in LDS, three bytes per sample in a frame's bound. */
inline FlacPlan plan_flac(uint32_t block_frames, uint32_t channels, size_t n_rows, FlacRow *rows, unsigned bits = 16) {
	FlacPlan p;
	const uint32_t B = sauflac::flac_block_frames(block_frames);
	if (!B || (channels != 1 && channels != 2) || !n_rows || n_rows > sauflac::FLAC_MAX_ROWS || !sauflac::flac_bits_ok((int)bits)) return p;
	p.B = B; p.rows = (uint32_t)n_rows; p.channels = channels;
	p.analyze_threads = channels == 2 ? 256 : 64;
	p.analyze_lds = (size_t)(B + B / 32) * sizeof(uint32_t) * (bits == 24 ? channels : 1);
	p.write_lds = p.analyze_lds + ((size_t)sauflac::flac_frame_bound(B, channels, bits) / 4 + 2) * sizeof(uint32_t);
	if (p.analyze_lds + flac_analyze_static_lds(bits) > FLAC_LDS_MAX) return p; /* (never, for the sizes allowed) */
	p.pend_pitch = (size_t)B * channels;
	uint64_t jobs = 0, out = 0;
	for (size_t r = 0; rows && r < n_rows; ++r) {
		if (rows[r].block0 + rows[r].n_blocks > sauflac::FLAC_MAX_BLOCKS) return p;
		if (jobs > FLAC_MAX_JOBS || out > sauflac::FLAC_MAX_UNREAD) return p;
		rows[r].job0 = (uint32_t)jobs;
		rows[r].out_off = (uint32_t)out;
		jobs += rows[r].n_blocks;
		const uint64_t w = flac_row_worst(rows[r], B, channels, bits);
		p.worst += w;
		out += (w + 15) & ~15ull;
	}
	if (jobs > FLAC_MAX_JOBS || p.worst > sauflac::FLAC_MAX_UNREAD) return p;
	p.jobs = (uint32_t)jobs;
	p.out_bytes = (size_t)out;
	p.ok = true;
	return p;
}

/* flac_decode_kernel's dynamic LDS (k_flac_dec.h; grid (jobs) x FLAC_THREADS, the jobs of the feed's plan): a word per sample of
 * the block, then the frame's bytes at their bound, rounded up to a word -- 57364 bytes at 24 bits, B = 4096, stereo. Beside it
 * the kernel has FLAC_DECODE_STATIC_LDS bytes at most of its own. 0: sizes that are not allowed. */
constexpr size_t FLAC_DECODE_STATIC_LDS = 256;
inline size_t plan_flac_decode_lds(uint32_t block_frames, uint32_t channels, unsigned bits) {
	const uint32_t B = sauflac::flac_block_frames(block_frames);
	if (!B || (channels != 1 && channels != 2) || !sauflac::flac_bits_ok((int)bits)) return 0;
	const size_t lds = (size_t)B * channels * sizeof(int32_t) + (((size_t)sauflac::flac_frame_bound(B, channels, bits) + 3) & ~(size_t)3);
	return lds + FLAC_DECODE_STATIC_LDS <= FLAC_LDS_MAX ? lds : 0;
}

/* ---- the quantiser (k_dither.h; include/saugns_amd.h, section "Dither and noise shaping") ----
 * Without taps a sample depends on its position only: dither_flat_kernel has flac_quant_kernel's geometry, four samples per
 * thread. With taps a chain -- one channel of one row -- is a recurrence that cannot be cut in time: dither_shape_kernel gives a
 * wave 64 chains, one per lane (64 mono rows or 32 stereo rows), and walks them through tiles of 64 frames staged in LDS
 * frame-major: s as f64, the dither as f32 and in its place the sample on the way back, 12 bytes per sample. A frame's 64
 * chains lie 64 + channels entries apart: the walking side (lanes a chain apart) reads consecutive entries, and the transposing
 * side (lanes a frame apart) no longer meets it 64 ways on one bank. That is by the address arithmetic only -- in stereo the
 * f64 stores may still meet two ways --, and no counter run has looked at it yet. */
constexpr uint32_t DITHER_TILE = 64;   /* frames of a tile */
constexpr uint32_t DITHER_CHAINS = 64; /* chains of a wave */
/* what a feed tells the kernels of a row (uploaded as it stands) */
struct DitherRow {
	uint64_t first;    /* the stream's frames before this feed */
	uint64_t seed_r;   /* sau_dither.h: dither_row_seed */
	uint32_t frames;   /* of this feed */
	float gain;
};
static_assert(sizeof(DitherRow) == 24, "DitherRow is uploaded as it stands");
struct DitherPlan {
	bool ok = false;          /* false: taps above 9, channels not 1 or 2, no row or more than 65535 */
	bool shaped = false;      /* dither_shape_kernel; else dither_flat_kernel */
	uint32_t rows = 0, channels = 0;
	uint32_t flat_grid_x = 0; /* dither_flat_kernel: grid (this, rows) x 256; 0: no launch */
	uint32_t shape_waves = 0; /* dither_shape_kernel: grid (this) x 64; 0: no launch */
	uint32_t rows_per_wave = 0;
	uint32_t tiles = 0;       /* of the feed's longest row */
	uint32_t lds_stride = 0;  /* entries between a tile's frames */
	size_t shape_lds = 0;     /* bytes of the tile and the wave's row records */
	size_t out_pitch = 0;     /* bytes between the output rows: a multiple of 256 (0 for a feed without frames) */
};
inline DitherPlan plan_dither(uint32_t taps, uint32_t channels, size_t n_rows, uint32_t longest) {
	DitherPlan p;
	if (taps > saudither::DITHER_TAPS_MAX || (channels != 1 && channels != 2) || !n_rows || n_rows > saudither::DITHER_MAX_ROWS) return p;
	p.shaped = taps != 0;
	p.rows = (uint32_t)n_rows; p.channels = channels;
	p.rows_per_wave = DITHER_CHAINS / channels;
	p.lds_stride = DITHER_CHAINS + channels;
	p.shape_lds = (size_t)DITHER_TILE * (DITHER_CHAINS + 2) * 12 + DITHER_CHAINS * sizeof(DitherRow);
	p.tiles = (uint32_t)(((uint64_t)longest + DITHER_TILE - 1) / DITHER_TILE);
	p.out_pitch = ((size_t)longest * channels * sizeof(int16_t) + 255) & ~(size_t)255;
	if (longest) {
		if (p.shaped) p.shape_waves = (uint32_t)((n_rows + p.rows_per_wave - 1) / p.rows_per_wave);
		/* thread 0 of a row takes the samples ahead of the first 16-byte boundary, every other thread four */
		else p.flat_grid_x = (uint32_t)(((uint64_t)longest * channels / 4 + 2 + 255) / 256);
	}
	p.ok = true;
	return p;
}

} /* namespace sauplan */
#endif
