/* overlap_ops.h -- TEST INFRASTRUCTURE: a sequence of backend operations played on the final mixer's ordering tracker
 * (saugns_amd/csrc/mix_overlap.h) and on plan_mix_overlap (launch_plan.h), in the order HipBackendImpl calls them at, with
 * everything either stream would do written to a log. tests/test_mix_overlap_host.py draws the sequences and replays the log in
 * a model of two in-order streams; overlap_hooks.cpp (a library for that test) and overlap_driver.cpp (a program of its own,
 * built with sanitizers) both run this one interpreter.
 *
 * An operation is six int64: {code, a, b, c, d, e}
 *   OP_SEGMENT  a: bit 0 the segment has a final mixer launch, bit 1 its closed-form launch mixes tiles into the PCM itself,
 *               bit 2 the rows are poisoned first, bit 3 that launch is split into edge and inner groups, bit 4 another launch of
 *               it writes PCM (a look-back launch's tails, the early mixers), bit 5 the timing pool drains inside the mixer's
 *               launch -- a join after the mixer's ticket is known and before its events are recorded; b: MiB of its rows
 *   OP_ENTRY    a: which entry point (fetch, sync, order_after, save_state, load_state, a format change, ...): a join
 *   OP_REFUSE   the next allocation of the second block of rows fails
 *   OP_SWITCHES a: SAU_AMD_NO_MIX_OVERLAP, b: SAU_AMD_MIX_OVERLAP_SHARED, c: SAU_AMD_MIX_OVERLAP_MB
 * A log entry is three int64: {kind, x, y}
 *   LOG_WAIT     the main stream waits for ticket x; y: where (W_*)
 *   LOG_RECORDS  the main stream writes records of set x
 *   LOG_ROWS     ... writes rows of block x
 *   LOG_PCM      ... reads or writes PCM
 *   LOG_ALL      ... an entry point that may touch anything (y: which)
 *   LOG_MIXER    mixer x goes onto the side stream, over set y & 1 and block y >> 1
 *   LOG_SEGMENT  a segment begins: mode x, set y */
#ifndef SAU_AMD_OVERLAP_OPS_H
#define SAU_AMD_OVERLAP_OPS_H
#include "../../saugns_amd/csrc/launch_plan.h"
#include <vector>

namespace overlap_ops {

enum : int64_t { OP_SEGMENT = 0, OP_ENTRY = 1, OP_REFUSE = 2, OP_SWITCHES = 3 };
enum : int64_t { LOG_WAIT = 1, LOG_RECORDS, LOG_ROWS, LOG_PCM, LOG_ALL, LOG_MIXER, LOG_SEGMENT };
enum : int64_t { W_RECORDS = 1, W_POISON, W_ROWS, W_PCM, W_MIXER_MAIN, W_ENTRY };

struct Player {
	sauplan::MixOverlapTracker tr;
	sauplan::Tuning tun;
	bool refuse_next = false, refused = false, second_there = false, bad = false;
	std::vector<int64_t> log;

	void put(int64_t k, int64_t x, int64_t y) { log.push_back(k); log.push_back(x); log.push_back(y); }
	void wait(uint64_t t, int64_t where) { if (t) put(LOG_WAIT, (int64_t)t, where); }

	void segment(int64_t flags, int64_t rows_mb) {
		using namespace sauplan;
		const bool has_mixer = flags & 1, inmix = flags & 2, poison = flags & 4, inner = flags & 8, pcm_inside = inmix || (flags & 16);
		PlanInputs in;
		in.max_write = has_mixer ? 1000u : 0u;
		FastPlan fk;
		fk.use_fast = true; fk.queues = inmix; fk.inmix = inmix; fk.inner = inner ? INNER_LANE_MAJOR : INNER_NONE;
		const uint32_t set = tr.begin_segment();
		MixOverlap mode = plan_mix_overlap(tun, in, fk, (size_t)rows_mb << 20, refused);
		if (mode == MIXO_ALTERNATE && set == 1 && !second_there) { /* the second block, on the first segment that would use it */
			if (refuse_next || tun.mix_overlap_fail) { refuse_next = false; refused = true; mode = MIXO_SHARED; }
			else second_there = true;
		}
		const uint32_t block = MixOverlapTracker::block_of(mode, set);
		put(LOG_SEGMENT, mode, set);
		wait(tr.before_records(set), W_RECORDS);
		put(LOG_RECORDS, set, 0); /* the stream records' upload */
		if (poison) { wait(tr.before_rows(block), W_POISON); put(LOG_ROWS, block, 0); }
		put(LOG_RECORDS, set, 0); /* analyze, decode, premix */
		wait(tr.before_rows(block), W_ROWS);
		put(LOG_ROWS, block, 0); /* the edge launch, or whichever launch writes rows first */
		if (pcm_inside) { wait(tr.before_pcm(), W_PCM); put(LOG_PCM, 0, 0); }
		put(LOG_ROWS, block, 0); /* the launches after it, the block loop */
		put(LOG_RECORDS, set, 0); /* finalize */
		if (!has_mixer) return;
		if (mode == MIXO_OFF) { wait(tr.before_pcm(), W_MIXER_MAIN); put(LOG_PCM, 0, 0); }
		else { /* (as launch_mixer goes: the ticket's number, the launch and its events, and only then the tracker's word of it) */
			const uint64_t t = tr.next_ticket();
			if (flags & 32) entry(8);
			if (tr.mixer_launched(set, block) != t) bad = true;
			put(LOG_MIXER, (int64_t)t, (int64_t)(set | block << 1));
		}
	}
	void entry(int64_t which) { wait(tr.join(), W_ENTRY); put(LOG_ALL, 0, which); }

	/* false: an operation it does not know */
	bool play(const int64_t *ops, size_t n) {
		for (size_t i = 0; i < n; ++i) {
			const int64_t *o = ops + 6 * i;
			switch (o[0]) {
			case OP_SEGMENT: segment(o[1], o[2]); break;
			case OP_ENTRY: entry(o[1]); break;
			case OP_REFUSE: refuse_next = true; break;
			case OP_SWITCHES:
				tun.mix_overlap = !o[1]; tun.mix_overlap_shared = o[2] != 0;
				tun.mix_overlap_mb = (uint32_t)(o[3] < 0 ? 0 : o[3]);
				break;
			default: return false;
			}
		}
		return !bad;
	}
};

} /* namespace overlap_ops */
#endif
