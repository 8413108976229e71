/* overlap_hooks.cpp -- TEST INFRASTRUCTURE for tests/test_mix_overlap_host.py, without a GPU:
 *   sauAmd_overlap_play   a sequence of operations on the final mixer's ordering tracker and plan_mix_overlap (overlap_ops.h)
 *   sauAmd_overlap_plan   plan_mix_overlap alone, with the switches as the environment has them */
#include "overlap_ops.h"
#include <stdlib.h>

#define HOOK extern "C" __attribute__((visibility("default")))

/* ops[6 * n_ops] -> log_out[3 * entries]; returns the entries (more than log_cap / 3: nothing was written), -1: a bad operation */
HOOK long long sauAmd_overlap_play(const int64_t *ops, size_t n_ops, int64_t *log_out, size_t log_cap) {
	overlap_ops::Player p;
	if (!p.play(ops, n_ops)) return -1;
	if (p.log.size() <= log_cap) memcpy(log_out, p.log.data(), p.log.size() * sizeof(int64_t));
	return (long long)(p.log.size() / 3);
}

/* (as sauengine::tune_env reads them: this library has none of the product's objects) */
static const char *tune(const char *name) { return getenv("SAU_AMD_TUNE") ? getenv(name) : nullptr; }

/* inmix: the segment's closed-form launch mixes tiles itself; inner: it is split into edge and inner groups */
HOOK int sauAmd_overlap_plan(uint32_t max_write, uint64_t rows_bytes, int second_refused, int inmix, int inner) {
	const sauplan::Tuning tun = sauplan::tuning_from_env(tune);
	sauplan::PlanInputs in;
	in.max_write = max_write;
	sauplan::FastPlan fk;
	fk.use_fast = true; fk.queues = inmix != 0; fk.inmix = inmix != 0; fk.inner = inner ? sauplan::INNER_LANE_MAJOR : sauplan::INNER_NONE;
	return (int)sauplan::plan_mix_overlap(tun, in, fk, (size_t)rows_bytes, second_refused != 0);
}
