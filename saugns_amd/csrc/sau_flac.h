/* sau_flac.h -- the FLAC encoder's arithmetic (include/saugns_amd.h, section "FLAC"), shared by the host restatement
 * (tables.cpp: flac_encode_block) and the kernels (k_flac.h) the way sau_dev_math.h is: candidate samples, residuals, the
 * zigzag, the cost of a Rice partition, the choice of order, of partitions and of the channel assignment, the frame header and
 * the two CRCs, and the LPC mode's window, Levinson-Durbin recursion, quantisation and choice. Everything summed over a block
 * is integer arithmetic, and the LPC mode's few f64 steps are serial with a stated order, so host and device agree by
 * construction; what differs between them is only who walks the samples. */
#ifndef SAU_FLAC_H
#define SAU_FLAC_H
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SAU_FLAC_HD __host__ __device__ inline
#else
#define SAU_FLAC_HD static inline
#endif

namespace sauflac {

constexpr uint32_t FLAC_MAX_ROWS = 65535;
constexpr uint64_t FLAC_MAX_BLOCKS = 0x7fffffffull;  /* per row: the frame number's six bytes hold 31 bits */
constexpr uint64_t FLAC_MAX_UNREAD = 1ull << 30;     /* bytes of unread output on the device */
constexpr unsigned FLAC_K_MAX = 14, FLAC_NK = 15;    /* 16 bits: Rice parameters 0 .. 14; 15 is the escape, never used */
constexpr unsigned FLAC_FINE = 16, FLAC_NODES = 31;  /* finest partitions of a whole block; (p, partition) pairs for p = 0 .. 4 */
/* The two sample widths (include/saugns_amd.h, FLAC, "24 bits"). 16: int16 samples, the side channel takes 17 bits, u is below
 * 2^21, the Rice parameters are 0 .. 14 in four bits each (method 00). 24: int32 samples in -2^23 .. 2^23 - 1, the side channel
 * takes 25 bits; a FIXED residual is at most 16 * 2^24 in size, so the residual functions below serve both; u is below 2^30, the
 * parameters are 0 .. 30 in five bits (method 01), and everything summed over a lane's run, not only over a block, needs 64
 * bits. In the LPC mode ("LPC at 24 bits") the window product and the coefficient sum are 64-bit, and a residual is below 2^31
 * in size -- flac_lpc_guard sees to that --, so its u takes all 32 bits: nothing behind an LPC residual may rely on 2^30. */
constexpr int32_t FLAC_S24_MIN = -8388608, FLAC_S24_MAX = 8388607;
SAU_FLAC_HD bool flac_bits_ok(int bits) { return bits == 16 || bits == 24; }
SAU_FLAC_HD constexpr unsigned flac_k_width(unsigned bits) { return bits == 24 ? 5 : 4; } /* bits of a partition's parameter */
SAU_FLAC_HD constexpr unsigned flac_nk(unsigned bits) { return (1u << flac_k_width(bits)) - 1; } /* parameters tried: FLAC_NK or 31 */
enum : uint8_t { FLAC_CONSTANT = 0, FLAC_VERBATIM = 1, FLAC_FIXED = 2, FLAC_LPC = 3 };
constexpr unsigned FLAC_LPC_MAX = 8, FLAC_LPC_PREC = 12; /* max_lpc_order's largest value; bits of a quantised coefficient */
enum : uint8_t { FLAC_CAND_L = 0, FLAC_CAND_R = 1, FLAC_CAND_M = 2, FLAC_CAND_S = 3 };

/* 0 stands for 4096; 0 when the size is not allowed */
SAU_FLAC_HD uint32_t flac_block_frames(uint32_t b) {
	if (b == 0) return 4096;
	return (b == 256 || b == 512 || b == 1024 || b == 2048 || b == 4096) ? b : 0;
}
/* the most bytes a frame of n frames takes at `bits` per sample: 13 header bytes, every channel verbatim, the CRC-16 */
SAU_FLAC_HD uint32_t flac_frame_bound(uint32_t n, uint32_t channels, unsigned bits) { return 15 + channels * (1 + bits / 8 * n); }

/* What a block's choices come to for one channel: kind, order, partition order and the partitions' Rice parameters. */
struct FlacSub {
	uint8_t cand;     /* FLAC_CAND_* */
	uint8_t type;     /* FLAC_CONSTANT, _VERBATIM, _FIXED, _LPC */
	uint8_t order;    /* FIXED: 0 .. 4; LPC: 1 .. 8 */
	uint8_t p;        /* FIXED, LPC: partition order, 0 .. 4 */
	uint8_t k[FLAC_FINE]; /* FIXED, LPC: partition j's parameter, j < 2^p */
	uint32_t bits;    /* the whole subframe */
	int16_t q[FLAC_LPC_MAX]; /* LPC: the quantised coefficients, q[0] the most recent sample's; zeros otherwise */
	uint8_t shift;    /* LPC: 0 .. 15 */
	uint8_t pad_[3];
};
static_assert(sizeof(FlacSub) == 44, "FlacSub is read by the kernels as it stands");
struct FlacFrameDesc {
	uint32_t n;       /* frames in the block */
	uint32_t bytes;   /* of the whole frame, CRC-16 included */
	uint32_t off;     /* where it begins in its row's part of the feed's output (flac_scan_kernel) */
	uint8_t assign;   /* the channel assignment's four bits */
	uint8_t n_sub;
	uint8_t pad_[2];
	FlacSub sub[2];
};
static_assert(sizeof(FlacFrameDesc) == 104, "FlacFrameDesc is read by the kernels as it stands");

/* a candidate channel's sample from the frame's two */
SAU_FLAC_HD int32_t flac_cand(int32_t l, int32_t r, unsigned cand) {
	switch (cand) {
	case FLAC_CAND_L: return l;
	case FLAC_CAND_R: return r;
	case FLAC_CAND_M: return (l + r) >> 1; /* (arithmetic) */
	default: return l - r;
	}
}
/* a 16-bit frame as one word: the left (or only) sample in the low half, the right one in the high half */
SAU_FLAC_HD uint32_t flac_pack(int16_t l, int16_t r) { return (uint32_t)(uint16_t)l | ((uint32_t)(uint16_t)r << 16); }
SAU_FLAC_HD int32_t flac_cand(uint32_t w, unsigned cand) { return flac_cand((int16_t)(uint16_t)(w & 0xffffu), (int16_t)(uint16_t)(w >> 16), cand); }
SAU_FLAC_HD unsigned flac_cand_bps(unsigned cand, unsigned bits) { return cand == FLAC_CAND_S ? bits + 1 : bits; }

/* the residuals of all five orders from s_i .. s_{i-4} */
SAU_FLAC_HD void flac_residuals(int32_t s0, int32_t s1, int32_t s2, int32_t s3, int32_t s4, int32_t r[5]) {
	r[0] = s0;
	r[1] = s0 - s1;
	r[2] = s0 - 2 * s1 + s2;
	r[3] = s0 - 3 * s1 + 3 * s2 - s3;
	r[4] = s0 - 4 * s1 + 6 * s2 - 4 * s3 + s4;
}
SAU_FLAC_HD int32_t flac_residual(unsigned o, int32_t s0, int32_t s1, int32_t s2, int32_t s3, int32_t s4) {
	switch (o) {
	case 0: return s0;
	case 1: return s0 - s1;
	case 2: return s0 - 2 * s1 + s2;
	case 3: return s0 - 3 * s1 + 3 * s2 - s3;
	default: return s0 - 4 * s1 + 6 * s2 - 4 * s3 + s4;
	}
}
SAU_FLAC_HD uint32_t flac_zigzag(int32_t r) { return r >= 0 ? 2u * (uint32_t)r : 2u * (uint32_t)(-(r + 1)) + 1u; }
SAU_FLAC_HD uint32_t flac_abs(int32_t r) { return r >= 0 ? (uint32_t)r : (uint32_t)(-(r + 1)) + 1u; }

/* the order with the least sum of |r_i| over i = 4 .. n-1, the lowest on ties; 0 for n <= 4 */
SAU_FLAC_HD unsigned flac_pick_order(uint32_t n, const uint64_t abs_sum[5]) {
	if (n <= 4) return 0;
	unsigned best = 0;
	uint64_t least = abs_sum[0];
	for (unsigned o = 1; o < 5; ++o)
		if (abs_sum[o] < least) { least = abs_sum[o]; best = o; }
	return best;
}

/* node (p, part) of a block of n frames whose finest sums are fine[f * nk + k] = the sum of u >> k over fine partition f
 * (f < 2^fine_log2; fine_log2 = 4 for a whole block, 0 otherwise; nk = flac_nk(bits)): the least cost over k, the lowest k on ties */
SAU_FLAC_HD uint64_t flac_node_cost(const uint64_t *fine, unsigned nk, unsigned fine_log2, unsigned p, unsigned part, uint32_t n, unsigned o,
		unsigned *k_out) {
	const unsigned span = 1u << (fine_log2 - p), first = part * span;
	const uint64_t count = (n >> p) - (part == 0 ? o : 0);
	uint64_t best = ~0ull;
	unsigned bk = 0;
	for (unsigned k = 0; k < nk; ++k) {
		uint64_t s = 0;
		for (unsigned f = 0; f < span; ++f) s += fine[(first + f) * nk + k];
		const uint64_t cost = s + (1 + k) * count;
		if (cost < best) { best = cost; bk = k; }
	}
	*k_out = bk;
	return best;
}
SAU_FLAC_HD unsigned flac_node_index(unsigned p, unsigned part) { return (1u << p) - 1 + part; }

/* From the nodes' costs and parameters (those of p = 0 .. fine_log2) to the channel's record: the partition order with the
 * least cost (the lowest on ties), FIXED against VERBATIM (VERBATIM on ties). all_equal: CONSTANT whatever the rest. `bits`
 * gives the sample's size and the four or five bits of a partition's parameter. */
SAU_FLAC_HD void flac_finish_sub(FlacSub *s, unsigned cand, uint32_t n, bool all_equal, unsigned o, unsigned fine_log2,
		const uint64_t *node_cost, const uint8_t *node_k, unsigned bits) {
	const unsigned bps = flac_cand_bps(cand, bits);
	s->cand = (uint8_t)cand; s->order = 0; s->p = 0;
	for (unsigned j = 0; j < FLAC_FINE; ++j) s->k[j] = 0;
	for (unsigned j = 0; j < FLAC_LPC_MAX; ++j) s->q[j] = 0;
	s->shift = 0; s->pad_[0] = s->pad_[1] = s->pad_[2] = 0;
	if (all_equal) { s->type = FLAC_CONSTANT; s->bits = 8 + bps; return; }
	uint64_t best = ~0ull;
	unsigned bp = 0;
	for (unsigned p = 0; p <= fine_log2; ++p) {
		uint64_t c = 0;
		for (unsigned j = 0; j < (1u << p); ++j) c += flac_k_width(bits) + node_cost[flac_node_index(p, j)];
		if (c < best) { best = c; bp = p; }
	}
	const uint64_t fixed =8 + (uint64_t)bps * o + 6 + best, verbatim = 8 + (uint64_t)bps * n;
	if (verbatim <= fixed) { s->type = FLAC_VERBATIM; s->bits = (uint32_t)verbatim; return; }
	s->type = FLAC_FIXED; s->order = (uint8_t)o; s->p = (uint8_t)bp; s->bits = (uint32_t)fixed;
	for (unsigned j = 0; j < (1u << bp); ++j) s->k[j] = node_k[flac_node_index(bp, j)];
}

/* ---- the LPC mode (include/saugns_amd.h, FLAC, "The LPC mode": the steps' numbers are those of that text) ----
 * Sums over a block are integers, so whoever adds them in whatever order gets the same; the floating-point steps are a short
 * serial sequence of IEEE f64 operations in a stated order (the build is -ffp-contract=off), done by one lane or one thread. */
/* step 1: the window's value at j, 0 .. 4095, and a windowed sample (|s| < 2^17: the product fits 32 bits; at 24 bits |s| <= 2^24,
 * the product is 64-bit and the shift 11, so |ws| < 2^25 at both widths) */
SAU_FLAC_HD int32_t flac_lpc_window(uint32_t j, uint32_t B, unsigned log2B) {
	const int32_t d = (int32_t)(2 * j + 1) - (int32_t)B;
	return (int32_t)((B * B - (uint32_t)(d * d)) >> (2 * log2B - 12));
}
SAU_FLAC_HD int32_t flac_lpc_windowed(int32_t s, int32_t w) { return (s * w) >> 3; }
SAU_FLAC_HD int32_t flac_lpc_windowed(int32_t s, int32_t w, unsigned bits) {
	return bits == 24 ? (int32_t)(((int64_t)s * w) >> 11) : flac_lpc_windowed(s, w);
}
/* step 3: the least shift that brings R[0] below 2^53 */
SAU_FLAC_HD unsigned flac_lpc_f64_shift(int64_t r0) {
	unsigned g = 0;
	while ((r0 >> g) >= (1ll << 53)) ++g;
	return g;
}
SAU_FLAC_HD uint64_t flac_f64_bits(double x) { uint64_t b; __builtin_memcpy(&b, &x, 8); return b; }
SAU_FLAC_HD double flac_f64_of_bits(uint64_t b) { double x; __builtin_memcpy(&x, &b, 8); return x; }
/* steps 4 and 5: from r[0 .. M] the quantised coefficients of every candidate order m: q[(m - 1) * 8 + j], shift[m - 1]; bit
 * m - 1 of the result is set where order m is a candidate. a[M] is work space (the kernels hand in LDS: every array here is
 * indexed at run time). */
SAU_FLAC_HD uint32_t flac_lpc_orders(const double *r, unsigned M, double *a, int16_t *q, uint8_t *shift) {
	uint32_t mask = 0;
	for (unsigned j = 0; j < M; ++j) a[j] = 0.0;
	double err = r[0];
	for (unsigned i = 0; i < M; ++i) {
		double acc = r[i + 1];
		for (unsigned j = 0; j < i; ++j) acc = acc + a[j] * r[i - j];
		const double k = -acc / err;
		a[i] = k;
		for (unsigned j = 0; j < i / 2; ++j) {
			const double t = a[j], u = a[i - 1 - j];
			a[j] = t + k * u;
			a[i - 1 - j] = u + k * t;
		}
		if (i & 1u) { const double t = a[i / 2]; a[i / 2] = t + k * t; }
		err = err * (1.0 - k * k);
		if (!(err > 0.0) || ((flac_f64_bits(err) >> 52) & 0x7ffu) == 0x7ffu) break;
		const unsigned m = i + 1;
		double cmax = 0.0;
		for (unsigned j = 0; j < m; ++j) {
			const double x = flac_f64_of_bits(flac_f64_bits(a[j]) & 0x7fffffffffffffffull);
			if (x > cmax) cmax = x;
		}
		const unsigned field = (unsigned)(flac_f64_bits(cmax) >> 52) & 0x7ffu;
		if (field == 0 || field == 0x7ffu) continue; /* 0 or subnormal; not finite */
		int sh = (int)FLAC_LPC_PREC - 1 - ((int)field - 1022);
		if (sh > 15) sh = 15;
		if (sh < 0) continue;
		const double scale = flac_f64_of_bits((uint64_t)(1023 + sh) << 52);
		double E = 0.0;
		for (unsigned j = 0; j < m; ++j) {
			E = E + (-a[j]) * scale;
			const double v = __builtin_floor(E + 0.5);
			const int32_t qi = v < -2048.0 ? -2048 : v > 2047.0 ? 2047 : (int32_t)v;
			q[i * FLAC_LPC_MAX + j] = (int16_t)qi;
			E = E - (double)qi;
		}
		shift[i] = (uint8_t)sh;
		mask |= 1u << i;
	}
	return mask;
}
/* step 5b ("LPC at 24 bits"): the mask without the orders whose prediction could pass 2^30 in size -- S = the sum of |q[j]|,
 * j < m; order m goes when (S << (bps - 1)) >> shift >= 2^30 (S < 2^15 and bps <= 25: below 2^40). Integers only, so host
 * and device agree; the 16-bit rules have no such step and never come here. */
SAU_FLAC_HD uint32_t flac_lpc_guard(uint32_t mask, const int16_t *q /* [(m - 1) * 8 + j] */, const uint8_t *shift /* [m - 1] */, unsigned bps) {
	for (unsigned m = 1; m <= FLAC_LPC_MAX; ++m)
		if (mask & (1u << (m - 1))) {
			uint64_t S = 0;
			for (unsigned j = 0; j < m; ++j) {
				const int32_t v = q[(m - 1) * FLAC_LPC_MAX + j];
				S += (uint64_t)(v < 0 ? -v : v);
			}
			if (((S << (bps - 1)) >> shift[m - 1]) >= (1ull << 30)) mask &= ~(1u << (m - 1));
		}
	return mask;
}
/* step 6 from the sum of q[j] * s_{i-1-j}: in 32 bits at 16 bits per sample; at 24 the sum is 64-bit (below 2^39 in size) and
 * the residual, below 2^31 in size behind flac_lpc_guard, is narrowed */
SAU_FLAC_HD int32_t flac_lpc_residual(int32_t s0, int32_t sum, unsigned shift) { return s0 - (sum >> shift); }
SAU_FLAC_HD int32_t flac_lpc_residual(int32_t s0, int64_t sum, unsigned shift) { return (int32_t)((int64_t)s0 - (sum >> shift)); }
/* step 7: what order m is estimated to cost, from A_m; nk = flac_nk(bits), the parameters tried. The kernels name nk at compile
 * time (the 16-bit build's loop is then the one it always had); the host hands it in. */
template <unsigned NK>
SAU_FLAC_HD uint64_t flac_lpc_est_nk(uint64_t abs_sum, uint32_t n, unsigned M, unsigned m, unsigned bps) {
	uint64_t best = ~0ull;
	for (unsigned k = 0; k < NK; ++k) {
		const uint64_t c = (uint64_t)(1 + k) * (n - M) + ((2 * abs_sum) >> k);
		if (c < best) best = c;
	}
	return best + (uint64_t)m * (bps + FLAC_LPC_PREC);
}
SAU_FLAC_HD uint64_t flac_lpc_est(uint64_t abs_sum, uint32_t n, unsigned M, unsigned m, unsigned bps, unsigned nk) {
	return nk == flac_nk(24) ? flac_lpc_est_nk<flac_nk(24)>(abs_sum, n, M, m, bps) : flac_lpc_est_nk<FLAC_NK>(abs_sum, n, M, m, bps);
}
/* the candidate order with the least estimate, the lowest on ties; 0 when there is none */
SAU_FLAC_HD unsigned flac_lpc_pick_order(uint32_t mask, const uint64_t *abs_sum /* [m - 1] */, uint32_t n, unsigned M, unsigned bps, unsigned nk) {
	unsigned best = 0;
	uint64_t least = ~0ull;
	for (unsigned m = 1; m <= M; ++m)
		if (mask & (1u << (m - 1))) {
			const uint64_t e = flac_lpc_est(abs_sum[m - 1], n, M, m, bps, nk);
			if (e < least) { least = e; best = m; }
		}
	return best;
}
/* steps 8 and 9 on a record flac_finish_sub has left as VERBATIM or FIXED (the cheaper of the two, VERBATIM on ties): LPC of
 * order m takes its place where it costs less. node_cost, node_k: the nodes of the LPC residual's partitions (o = m). `bits`
 * gives the sample's size and the four or five bits of a partition's parameter, as in flac_finish_sub. */
SAU_FLAC_HD void flac_lpc_choose(FlacSub *s, uint32_t n, unsigned m, const int16_t *q, unsigned shift, unsigned fine_log2,
		const uint64_t *node_cost, const uint8_t *node_k, unsigned bits) {
	if (s->type == FLAC_CONSTANT) return;
	const unsigned bps = flac_cand_bps(s->cand, bits);
	uint64_t best = ~0ull;
	unsigned bp = 0;
	for (unsigned p = 0; p <= fine_log2; ++p) {
		uint64_t c = 0;
		for (unsigned j = 0; j < (1u << p); ++j) c += flac_k_width(bits) + node_cost[flac_node_index(p, j)];
		if (c < best) { best = c; bp = p; }
	}
	const uint64_t lpc = 8 + (uint64_t)bps * m + 4 + 5 + (uint64_t)FLAC_LPC_PREC * m + 6 + best;
	if (lpc >= s->bits) return;
	s->type = FLAC_LPC; s->order = (uint8_t)m; s->p = (uint8_t)bp; s->bits = (uint32_t)lpc; s->shift = (uint8_t)shift;
	for (unsigned j = 0; j < FLAC_FINE; ++j) s->k[j] = 0;
	for (unsigned j = 0; j < (1u << bp); ++j) s->k[j] = node_k[flac_node_index(bp, j)];
	for (unsigned j = 0; j < m; ++j) s->q[j] = q[j];
}

/* the bytes of a frame number in the extended UTF-8 coding, and of a frame header: sync and codes, the number, n - 1 where
 * the block is not a whole one, the CRC-8 */
SAU_FLAC_HD uint32_t flac_utf8_len(uint32_t v) {
	return v < 0x80u ? 1 : v < 0x800u ? 2 : v < 0x10000u ? 3 : v < 0x200000u ? 4 : v < 0x4000000u ? 5 : 6;
}
SAU_FLAC_HD uint32_t flac_header_len(uint32_t n, uint32_t block_frames, uint32_t number) {
	return 4 + flac_utf8_len(number) + (n != block_frames ? 2 : 0) + 1;
}
/* the frame's record from the candidates' (mono: cand[0] alone; stereo: L, R, M, S): the pair with the fewest bits among
 * L+R, L+S, S+R, M+S, the first on ties; then the frame's size */
SAU_FLAC_HD void flac_finish_frame(FlacFrameDesc *d, const FlacSub *cand, uint32_t channels, uint32_t n, uint32_t block_frames, uint32_t number) {
	d->n = n; d->off = 0; d->pad_[0] = d->pad_[1] = 0;
	if (channels == 1) {
		d->assign = 0; d->n_sub = 1; d->sub[0] = cand[0]; d->sub[1] = cand[0];
	} else {
		const uint64_t l = cand[FLAC_CAND_L].bits, r = cand[FLAC_CAND_R].bits, m = cand[FLAC_CAND_M].bits, s = cand[FLAC_CAND_S].bits;
		uint64_t least = l + r;
		unsigned first = FLAC_CAND_L, second = FLAC_CAND_R;
		d->assign = 1;
		if (l + s < least) { least = l + s; d->assign = 8; first = FLAC_CAND_L; second = FLAC_CAND_S; }
		if (s + r < least) { least = s + r; d->assign = 9; first = FLAC_CAND_S; second = FLAC_CAND_R; }
		if (m + s < least) { least = m + s; d->assign = 10; first = FLAC_CAND_M; second = FLAC_CAND_S; }
		d->n_sub = 2; d->sub[0] = cand[first]; d->sub[1] = cand[second];
	}
	uint64_t bits = 8ull * flac_header_len(n, block_frames, number);
	for (unsigned i = 0; i < d->n_sub; ++i) bits += d->sub[i].bits;
	d->bytes = (uint32_t)((bits + 7) / 8) + 2;
}

/* ---- CRCs: MSB first, initial value 0, not reflected ---- */
SAU_FLAC_HD uint32_t flac_crc8_update(uint32_t crc, uint32_t byte) {
	crc ^= byte & 0xffu;
	for (int i = 0; i < 8; ++i) crc = (crc & 0x80u) ? ((crc << 1) ^ 0x07u) & 0xffu : (crc << 1) & 0xffu;
	return crc;
}
SAU_FLAC_HD uint32_t flac_crc16_update(uint32_t crc, uint32_t byte) {
	crc ^= (byte & 0xffu) << 8;
	for (int i = 0; i < 8; ++i) crc = (crc & 0x8000u) ? ((crc << 1) ^ 0x8005u) & 0xffffu : (crc << 1) & 0xffffu;
	return crc;
}
/* a * b in GF(2)[x] modulo x^16 + x^15 + x^2 + 1 */
SAU_FLAC_HD uint32_t flac_gf16_mul(uint32_t a, uint32_t b) {
	uint32_t r = 0;
	for (int i = 15; i >= 0; --i) {
		r = (r & 0x8000u) ? ((r << 1) ^ 0x8005u) & 0xffffu : (r << 1) & 0xffffu;
		if ((b >> i) & 1u) r ^= a;
	}
	return r;
}
/* the CRC-16 of A followed by `bytes` zero bytes, from crc(A): crc * x^(8 bytes). With initial value 0 the CRC is linear, so
 * crc(A || B) = flac_crc16_advance(crc(A), |B|) ^ crc(B) */
SAU_FLAC_HD uint32_t flac_crc16_advance(uint32_t crc, uint32_t bytes) {
	uint32_t sq = 0x0100u; /* x^8 */
	for (; bytes; bytes >>= 1) {
		if (bytes & 1u) crc = flac_gf16_mul(crc, sq);
		sq = flac_gf16_mul(sq, sq);
	}
	return crc;
}

/* the frame header, CRC-8 included -> its length (at most 13). assign: the channel assignment's four bits; the sample-size
 * code of `bits` is 100 for 16, 110 for 24. */
SAU_FLAC_HD uint32_t flac_frame_header(uint32_t n, uint32_t block_frames, uint32_t assign, uint32_t number, unsigned bits, uint8_t *out /* [16] */) {
	uint32_t len = 0;
	out[len++] = 0xff; out[len++] = 0xf8;
	uint32_t code = 7;
	if (n == block_frames) { code = 8; for (uint32_t b = 256; b < block_frames; b <<= 1) ++code; }
	out[len++] = (uint8_t)(code << 4);
	out[len++] = (uint8_t)((assign << 4) | ((bits == 24 ? 6u : 4u) << 1));
	const uint32_t ul = flac_utf8_len(number);
	if (ul == 1) out[len++] = (uint8_t)number;
	else {
		out[len++] = (uint8_t)((0xff00u >> ul) | (number >> (6 * (ul - 1)))); /* ul ones, a zero, the top bits */
		for (uint32_t i = ul - 1; i-- > 0;) out[len++] = (uint8_t)(0x80u | ((number >> (6 * i)) & 0x3fu));
	}
	if (n != block_frames) { out[len++] = (uint8_t)((n - 1) >> 8); out[len++] = (uint8_t)(n - 1); }
	uint32_t crc = 0;
	for (uint32_t i = 0; i < len; ++i) crc = flac_crc8_update(crc, out[i]);
	out[len++] = (uint8_t)crc;
	return len;
}

} /* namespace sauflac */
#endif
