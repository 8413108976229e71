/* mix_overlap.h -- (plain C++, no HIP) the ordering rules of a segment's final mixer on a stream of its own.
 *
 * A segment's last mixer launch reads the segment's records and rows and writes PCM; nothing the next segment's set-up
 * launches (analyze, decode, premix, the edge groups) do depends on it. So the backend runs it on a side stream beside
 * them (hip_backend.hip: launch_mixer), and this tracker says where the main stream has to wait for it.
 *
 * A mixer is a ticket, 1, 2, 3 ... in launch order. The side stream is in order, so mixer k + 1 never overtakes mixer k
 * (on PCM or anything else), and a wait for ticket t is a wait for every ticket up to t: one watermark, `joined`, is all
 * the tracker keeps about what the main stream has waited for. The backend asks at named points and gets "wait for
 * ticket t now" or 0, nothing. What a pending mixer k holds:
 *   records  the small records of set s(k) -- stream and row records, the guard words, the control words of the launch's
 *            own mixing, the tail words: before the main stream writes any record of set s, it waits for the last mixer
 *            that read set s (two segments old and long done, normally)
 *   rows     the voice and pan rows of block b(k) -- block 0, or (alternate rows) block s: before the first launch that
 *            writes rows of a block, the main stream waits for the last mixer that read that block
 *   PCM      before the first launch (or copy, or memset) on the main stream that reads or writes PCM: the last mixer
 * and join() is all three for everything: what every entry point of the backend does first unless it is on the
 * allow-list there.
 *
 * Tested on the CPU over drawn sequences against a model of two in-order streams (tests/test_mix_overlap_host.py). */
#ifndef SAU_AMD_MIX_OVERLAP_H
#define SAU_AMD_MIX_OVERLAP_H
#include <stdint.h>

namespace sauplan {

enum MixOverlap : uint32_t {
	MIXO_OFF = 0,   /* the mixer on the main stream, behind the segment's kernels */
	MIXO_SHARED,    /* on the side stream; the two sets share one block of rows */
	MIXO_ALTERNATE  /* on the side stream; each set has rows of its own */
};

/* at most two mixers are ever unjoined (one per set: a set's segment begins with a wait for the set's last mixer, and the
 * watermark takes every older ticket with it), so a ring of four events serves the tickets: when ticket t + 4 is recorded,
 * ticket t has long been waited for -- and a wait holds the event's state as of the moment it was enqueued */
constexpr uint32_t MIXO_RING = 4;

struct MixOverlapTracker {
	uint64_t next = 0;               /* the last ticket handed out */
	uint64_t joined = 0;             /* the main stream has waited for (or is otherwise behind) every ticket up to this one */
	uint64_t set_reader[2] = {0, 0}; /* the last mixer that read the records of set s */
	uint64_t rows_reader[2] = {0, 0};/* the last mixer that read the rows of block b */
	uint64_t segments = 0;           /* segments begun: segment n uses set n mod 2 */

	/* the set of the segment that begins now */
	uint32_t begin_segment() { return (uint32_t)(segments++ & 1u); }
	/* the block of rows a segment of this mode on this set uses */
	static uint32_t block_of(MixOverlap mode, uint32_t set) { return mode == MIXO_ALTERNATE ? (set & 1u) : 0u; }

	/* each: the ticket the main stream must wait for before it goes on, or 0 */
	uint64_t before_records(uint32_t set) { return need(set_reader[set & 1u]); }
	uint64_t before_rows(uint32_t block) { return need(rows_reader[block & 1u]); }
	uint64_t before_pcm() { return need(next); }
	uint64_t join() { return need(next); }
	/* The ticket the next mixer will have. The backend records that mixer's events under it and tells the tracker of the mixer
	 * only when its done event is recorded: a join in between (a timing pool that drains, say) cannot take the ticket for
	 * waited-for, and whatever fails on the way leaves no ticket without an event. */
	uint64_t next_ticket() const { return next + 1; }
	/* a mixer of set `set` over block `block` is on the side stream, its done event recorded behind it: its ticket */
	uint64_t mixer_launched(uint32_t set, uint32_t block) {
		++next;
		set_reader[set & 1u] = next;
		rows_reader[block & 1u] = next;
		return next;
	}
	bool pending() const { return next > joined; }
	static uint32_t slot(uint64_t ticket) { return (uint32_t)(ticket % MIXO_RING); }

private:
	uint64_t need(uint64_t t) {
		if (t <= joined) return 0;
		joined = t;
		return t;
	}
};

} /* namespace sauplan */
#endif
