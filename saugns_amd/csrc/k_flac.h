/* k_flac.h -- the FLAC encoder of int16 or int32 rows: part of hip_backend.hip (inside namespace sauhip). The format and every
 * choice are stated in include/saugns_amd.h, section "FLAC"; the arithmetic is sau_flac.h's, which the host restatement
 * (tables.cpp: flac_encode_block) uses too, so the bytes are a function of the fed sequence only. The kernels that read
 * samples are templates over a width, FlacS16 or FlacS32 (below, with the list of what differs); what follows is the 16-bit
 * account.
 *   flac_analyze_kernel  grid (jobs) x 64 (mono) or 256 (stereo): a workgroup owns one block of one row (a job: launch_plan.h)
 *       and a wave one candidate channel -- L, R, M, S. The block's frames are staged in LDS as words (L | R << 16); the wave
 *       finds whether its channel is constant, the sums of |r| of the five orders, for the order chosen the sums of u >> k,
 *       k = 0 .. 14, per finest partition (B / 16 frames; the whole of a short block), merges them upward (one lane per (p,
 *       partition)) and chooses; thread 0 then chooses the channel assignment and leaves the frame's record: FlacFrameDesc.
 *   flac_scan_kernel     grid (rows) x 256: the exclusive sum of a row's frame sizes -> where every frame begins behind the
 *       row's offset in the feed's output; the row's bytes of this feed and its running record (bytes, least and largest frame).
 *   flac_write_kernel    grid (jobs) x 256: stages the frames again, builds the frame in LDS words that start out cleared -- the
 *       header by thread 0; a verbatim sample or a residual's code (at most 15 non-zero bits: the stop bit and the low k bits;
 *       the unary zeros are what the cleared words hold) by an integer OR into at most two words, at the bit position an
 *       exclusive sum of the code lengths over the block gives -- and then the CRC-16: every lane takes a run of bytes and
 *       advances its remainder over what follows (flac_crc16_advance: the CRC is linear), and the remainders are XORed. OR and
 *       XOR do not depend on their order, so the bytes are reproducible. The finished bytes go to the frame's place.
 *   flac_carry_kernel    grid (parts, rows): the row's pending frames become those behind the feed, from one buffer into the
 *       other (the encoder swaps them), as spec_carry_kernel does.
 *   flac_quant_kernel<OutT>  grid (runs of 1024 samples, rows) x 256: dst = pcm16(x * gain[row]) or pcm24(x * gain[row]) of a
 *       float-fed encoder's rows, into rows of the encoder's own, ahead of the other kernels. A source row need only be
 *       float-aligned: thread 0 takes the samples ahead of the row's first 16-byte boundary one by one, every other thread
 *       four from a 16-byte load, the row's end again one by one.
 * The LPC mode (the header's "The LPC mode" and "LPC at 24 bits", max_lpc_order > 0) is a second build of the first and the third
 * kernel at either width, flac_analyze_kernel<W, true> and flac_write_kernel<W, true>; the <.., false> builds hold none of its
 * code and are what an encoder of order 0 launches. In the analysis of a whole block the candidate's wave goes on behind the
 * FIXED choice (flac_analyze_lpc): the windowed autocorrelation in 64-bit integers, a lane a run of n / 64 frames, the shares
 * added by the xor-shuffle sum; the Levinson-Durbin recursion and the quantisation of every order in f64 on lane 0, serial, in
 * the header's order; the orders' coefficient tables stay in LDS (a run-time index into registers would be scratch); the sums
 * of |r| of all candidate orders in one walk of the lane's run; the chosen order's sums of u >> k per finest partition in 64
 * bits, merged and priced as the FIXED ones; then LPC takes the record where it is cheaper. The writer reads the coefficients
 * from the record in LDS.
 * No lane walks a whole block: a lane's run is n / 64 frames in the analysis, n / 256 in the writer.
 *
 * LDS. Frame i is kept at word i + (i >> 5): in the partition sums a lane walks a run of consecutive frames (one new word per
 * frame) and the runs lie B / 64 apart, which without the extra word per 32 would put all lanes on one bank at B = 4096. The
 * analysis takes 4.1 B bytes + 10 KiB (the LPC build's tables are 1.1 KiB of them); the writer 4.1 B + the frame's bound,
 * 33 KiB at B = 4096 stereo.
 *
 * What FlacS32 (24 bits, the header's "24 bits"; int32 samples) does differently:
 *   - L and R are staged as two arrays, each with the padding above, R behind L; M and S are formed where they are read;
 *   - every sum of a lane is 64-bit (an order-4 residual takes 29 bits, u 30), the registers still indexed at compile time;
 *   - the Rice parameters are 0 .. 30 with five bits each (method 01), s_fine is [4][16 * 31];
 *   - samples take 24 or 25 bits in the frame, whose header says so and whose bound is larger;
 *   - the analysis takes 8.25 B bytes (stereo) + 17 KiB: 51 KiB at B = 4096; the writer 8.25 B + the frame's bound: 57 KiB;
 *   - the LPC build's analysis adds FlacLpcLds, 1.1 KiB: 33792 + 17200 + 1104 = 52096 bytes at B = 4096 stereo, the most any
 *     kernel here takes and under the 64 KiB a workgroup may have (launch_plan.h: FLAC_ANALYZE_STATIC_LDS);
 *   - in the LPC mode the window product is 64-bit (>> 11), the coefficient sum is 64-bit (below 2^39), and lane 0 takes the
 *     orders that step 5b excludes out of the mask (flac_lpc_guard) before the barrier that publishes it; a residual then is
 *     below 2^31 in size and its u takes 32 bits, which the 64-bit sums, flac_put's 32-bit field and the writer's bit counts
 *     (a subframe is cheaper than its verbatim form, below 2^18 bits) all hold. */
#ifndef SAU_K_FLAC_H
#define SAU_K_FLAC_H

using namespace sauflac;

struct FlacStats { /* per row, since the last reset */
	unsigned long long bytes;
	uint32_t min_bytes, max_bytes; /* 0, 0 before the first frame */
};
static_assert(sizeof(FlacStats) == 16, "FlacStats is fetched as it stands");

struct FlacParams {
	const void *rows;         /* the fed rows (or a float-fed encoder's own), int16 or int32; not read where a row's feed has no frames */
	size_t row_pitch;         /* bytes between them */
	const FlacRow *desc;      /* [n_rows] (launch_plan.h) */
	const void *pend;         /* [n_rows][pend_pitch], interleaved like the row: the frames from block0 * B on */
	void *pend_next;          /* flac_carry_kernel's target */
	size_t pend_pitch;        /* samples */
	FlacFrameDesc *frames;    /* [jobs] */
	uint8_t *out;             /* the feed's output */
	uint32_t *row_bytes;      /* [n_rows]: what this feed made of each row */
	FlacStats *stats;         /* [n_rows] */
	uint32_t B, channels, n_rows, jobs;
	uint32_t max_lpc;         /* the LPC mode's largest order, 1 .. 8, for the <true> kernels; 0 for the <false> ones */
};

__device__ __forceinline__ unsigned flac_ix(const unsigned i) { return i + (i >> 5); }

/* the row a job belongs to: the last one whose job0 is not above it (rows without blocks share the next row's job0) */
__device__ __forceinline__ unsigned flac_find_row(const FlacRow *__restrict__ desc, const unsigned n_rows, const unsigned job) {
	unsigned lo = 0, hi = n_rows;
	while (hi - lo > 1) {
		const unsigned mid = (lo + hi) >> 1;
		if (desc[mid].job0 <= job) lo = mid; else hi = mid;
	}
	return lo;
}

/* candidate c's sample i of a block staged as packed words (0 below the block's start) */
__device__ __forceinline__ int32_t flac_at(const uint32_t *s_w, const unsigned c, const int i) { return i >= 0 ? flac_cand(s_w[flac_ix((unsigned)i)], c) : 0; }

/* The two widths: the sample's type and size, the Rice parameters tried (k < NK) and their bits in the frame, the residual
 * coding method's two bits, the type of a lane's sums over its run, and how a block lies in LDS:
 *   lds_words  the words of a staged block; lds_words(B, 1) is R0, where the second array begins if there is one;
 *   stage      block j of the row's feed, n frames, into s_w: a pending frame, or one of the fed row;
 *   at         candidate c's sample i (0 below the block's start). c is the same for a whole wave.
 *   at_in      the same for an i that is inside the block: no look at its sign. */
struct FlacS16 { /* a frame is one word, L | R << 16 */
	typedef int16_t sample_t;
	typedef uint32_t run_t; /* (a lane's share fits 32 bits: at most 64 values below 2^21) */
	typedef int32_t acc_t;  /* the LPC mode's sum of q[j] * s_{i-1-j}: below 2^30 */
	static constexpr unsigned BITS = 16, NK = flac_nk(16), K_BITS = flac_k_width(16), METHOD = 0;
	static __device__ __forceinline__ unsigned lds_words(const unsigned B, const unsigned channels) { return B + (B >> 5); }
	static __device__ __forceinline__ void stage(const FlacParams &P, const FlacRow &d, const unsigned row, const unsigned j, const unsigned n,
			uint32_t *s_w, const unsigned R0) {
		const char *xrow = (const char *)P.rows + P.row_pitch * row;
		const int16_t *pend = (const int16_t *)P.pend + P.pend_pitch * row;
		const unsigned long long first = (unsigned long long)j * P.B; /* counted from the row's frame block0 * B */
		for (unsigned i = threadIdx.x; i < n; i += blockDim.x) {
			const unsigned long long rel = first + i;
			uint32_t w;
			if (P.channels == 2) /* (rows and pitches are multiples of 16: a frame is an aligned word, L in its low half) */
				w = rel < d.pend ? ((const uint32_t *)pend)[rel] : ((const uint32_t *)xrow)[rel - d.pend];
			else
				w = flac_pack(rel < d.pend ? pend[rel] : ((const int16_t *)xrow)[rel - d.pend], 0);
			s_w[flac_ix(i)] = w;
		}
	}
	static __device__ __forceinline__ int32_t at(const uint32_t *s_w, const unsigned R0, const unsigned c, const int i) { return flac_at(s_w, c, i); }
	static __device__ __forceinline__ int32_t at_in(const uint32_t *s_w, const unsigned R0, const unsigned c, const unsigned i) { return flac_cand(s_w[flac_ix(i)], c); }
};
struct FlacS32 { /* L (or the one channel) at s_w, R at s_w + R0; mono has c == 0 only and no R array */
	typedef int32_t sample_t;
	typedef unsigned long long run_t; /* (64 values of up to 2^28, of u up to 2^30) */
	typedef int64_t acc_t;  /* the LPC mode's sum of q[j] * s_{i-1-j}: below 2^39 */
	static constexpr unsigned BITS = 24, NK = flac_nk(24), K_BITS = flac_k_width(24), METHOD = 1;
	static __device__ __forceinline__ unsigned lds_words(const unsigned B, const unsigned channels) { return (B + (B >> 5)) * channels; }
	static __device__ __forceinline__ void stage(const FlacParams &P, const FlacRow &d, const unsigned row, const unsigned j, const unsigned n,
			uint32_t *s_w, const unsigned R0) {
		const char *xrow = (const char *)P.rows + P.row_pitch * row;
		const int32_t *pend = (const int32_t *)P.pend + P.pend_pitch * row;
		const unsigned long long first = (unsigned long long)j * P.B;
		for (unsigned i = threadIdx.x; i < n; i += blockDim.x) {
			const unsigned long long rel = first + i;
			if (P.channels == 2) { /* (rows and pitches are multiples of 16: a frame is an aligned pair of words) */
				const int2 f = rel < d.pend ? ((const int2 *)pend)[rel] : ((const int2 *)xrow)[rel - d.pend];
				s_w[flac_ix(i)] = (uint32_t)f.x;
				s_w[R0 + flac_ix(i)] = (uint32_t)f.y;
			} else
				s_w[flac_ix(i)] = (uint32_t)(rel < d.pend ? pend[rel] : ((const int32_t *)xrow)[rel - d.pend]);
		}
	}
	static __device__ __forceinline__ int32_t at(const uint32_t *s_w, const unsigned R0, const unsigned c, const int i) {
		if (i < 0) return 0;
		const unsigned x = flac_ix((unsigned)i);
		if (c == FLAC_CAND_L) return (int32_t)s_w[x];
		if (c == FLAC_CAND_R) return (int32_t)s_w[R0 + x];
		return flac_cand((int32_t)s_w[x], (int32_t)s_w[R0 + x], c);
	}
	static __device__ __forceinline__ int32_t at_in(const uint32_t *s_w, const unsigned R0, const unsigned c, const unsigned i) {
		const unsigned x = flac_ix(i);
		if (c == FLAC_CAND_L) return (int32_t)s_w[x];
		if (c == FLAC_CAND_R) return (int32_t)s_w[R0 + x];
		return flac_cand((int32_t)s_w[x], (int32_t)s_w[R0 + x], c);
	}
};

__device__ __forceinline__ unsigned long long flac_wave_sum(unsigned long long v, const int steps) {
	for (int m = 1; m < (1 << steps); m <<= 1) v += __shfl_xor(v, m);
	return v;
}

/* the sum of q[j] * s_{i-1-j}, j < m (i >= m): the coefficients are read from LDS, where a run-time index costs nothing */
template <typename W>
__device__ __forceinline__ typename W::acc_t flac_lpc_sum(const uint32_t *s_w, const unsigned R0, const unsigned c, const int16_t *q, const unsigned m,
		const unsigned i) {
	typename W::acc_t sum = 0;
	for (unsigned j = 0; j < m; ++j) sum += (typename W::acc_t)q[j] * W::at_in(s_w, R0, c, i - 1 - j);
	return sum;
}

/* What the LPC mode adds to a wave's analysis of its candidate (whole blocks only; every wave of the workgroup comes here,
 * since there are barriers inside): the windowed autocorrelation from the staged words -- a lane a run of n / 64 consecutive
 * frames, the window's value computed where it is used, products and sums in 64-bit integers, the lanes' shares added by the
 * xor-shuffle sum --, steps 3 to 5 on lane 0 with the orders' coefficient tables left in LDS, the sums of |r| of all
 * candidate orders in one walk of the lane's run, the chosen order's sums of u >> k per finest partition (64 bits: an LPC
 * residual may take 32), the nodes' costs, and the choice against what flac_finish_sub has left in s_cand[c]. At 24 bits the
 * samples come through W::at (M and S are formed where they are read), the coefficient sums are 64-bit, and lane 0 applies
 * step 5b to the mask. */
struct FlacLpcLds {
	double r[4][FLAC_LPC_MAX + 1];
	double a[4][FLAC_LPC_MAX];
	int16_t q[4][FLAC_LPC_MAX * FLAC_LPC_MAX];
	uint8_t shift[4][FLAC_LPC_MAX];
	uint32_t mask[4];
};
static_assert(sizeof(FlacLpcLds) == FLAC_LPC_LDS, "launch_plan.h counts FlacLpcLds in the analysis' LDS");
template <typename W>
__device__ __forceinline__ void flac_analyze_lpc(const FlacParams &P, const uint32_t *s_w, const unsigned R0, FlacLpcLds &L,
		uint64_t (*s_fine)[FLAC_FINE * W::NK], uint64_t (*s_node_cost)[32], uint8_t (*s_node_k)[32], FlacSub *s_cand, const unsigned c,
		const unsigned lane, const bool equal) {
	typedef typename W::acc_t acc_t;
	const unsigned n = P.B, M = P.max_lpc, log2B = 31 - __clz((int)P.B), bps = flac_cand_bps(c, W::BITS);
	const unsigned run = n >> 6, i0 = lane * run;
	/* steps 1 and 2 */
	long long R[FLAC_LPC_MAX + 1];
#pragma unroll
	for (unsigned l = 0; l <= FLAC_LPC_MAX; ++l) R[l] = 0;
	if (!equal) {
		int32_t h[FLAC_LPC_MAX + 1]; /* h[l] = ws[i - l] */
#pragma unroll
		for (unsigned l = 1; l <= FLAC_LPC_MAX; ++l)
			h[l] = i0 + 1 >= l + 1 ? flac_lpc_windowed(W::at(s_w, R0, c, (int)(i0 - l)), flac_lpc_window(i0 - l, n, log2B), W::BITS) : 0;
		for (unsigned i = i0; i < i0 + run; ++i) {
			h[0] = flac_lpc_windowed(W::at(s_w, R0, c, (int)i), flac_lpc_window(i, n, log2B), W::BITS);
#pragma unroll
			for (unsigned l = 0; l <= FLAC_LPC_MAX; ++l) R[l] += (long long)h[0] * h[l]; /* (h[l] is 0 where i < l; orders above M are not read) */
#pragma unroll
			for (unsigned l = FLAC_LPC_MAX; l > 0; --l) h[l] = h[l - 1];
		}
	}
#pragma unroll
	for (unsigned l = 0; l <= FLAC_LPC_MAX; ++l) R[l] = (long long)flac_wave_sum((unsigned long long)R[l], 6);
	const bool on = !equal && R[0] != 0; /* (the same in every lane of the wave) */
	/* steps 3 to 5, one lane */
	if (lane == 0) {
		uint32_t mask = 0;
		if (on) {
			const unsigned g = flac_lpc_f64_shift(R[0]);
#pragma unroll
			for (unsigned l = 0; l <= FLAC_LPC_MAX; ++l) L.r[c][l] = (double)(R[l] >> g);
			mask = flac_lpc_orders(L.r[c], M, L.a[c], L.q[c], L.shift[c]);
			if (W::BITS == 24) mask = flac_lpc_guard(mask, L.q[c], L.shift[c], bps); /* step 5b */
		}
		L.mask[c] = mask;
	}
	__syncthreads();
	const uint32_t mask = on ? L.mask[c] : 0;
	/* step 7: A_m of every candidate order over i = M .. n-1 */
	unsigned long long A[FLAC_LPC_MAX];
#pragma unroll
	for (unsigned m = 1; m <= FLAC_LPC_MAX; ++m) A[m - 1] = 0;
	if (mask)
		for (unsigned i = i0 > M ? i0 : M; i < i0 + run; ++i) {
			const int32_t s0 = W::at(s_w, R0, c, (int)i);
			int32_t hs[FLAC_LPC_MAX];
#pragma unroll
			for (unsigned j = 0; j < FLAC_LPC_MAX; ++j) hs[j] = j < M ? W::at(s_w, R0, c, (int)(i - 1 - j)) : 0;
#pragma unroll
			for (unsigned m = 1; m <= FLAC_LPC_MAX; ++m)
				if (mask & (1u << (m - 1))) {
					acc_t sum = 0;
#pragma unroll
					for (unsigned j = 0; j < m; ++j) sum += (acc_t)L.q[c][(m - 1) * FLAC_LPC_MAX + j] * hs[j];
					A[m - 1] += flac_abs(flac_lpc_residual(s0, sum, L.shift[c][m - 1]));
				}
		}
#pragma unroll
	for (unsigned m = 1; m <= FLAC_LPC_MAX; ++m) A[m - 1] = flac_wave_sum(A[m - 1], 6);
	unsigned m = 0;
	{ /* (flac_lpc_pick_order with the sums in registers) */
		uint64_t least = ~0ull;
#pragma unroll
		for (unsigned t = 1; t <= FLAC_LPC_MAX; ++t)
			if (mask & (1u << (t - 1))) {
				const uint64_t e = flac_lpc_est_nk<W::NK>(A[t - 1], n, M, t, bps);
				if (e < least) { least = e; m = t; }
			}
	}
	/* step 8: the chosen order's sums of u >> k per finest partition */
	unsigned long long f64[W::NK];
#pragma unroll
	for (unsigned k = 0; k < W::NK; ++k) f64[k] = 0;
	/* (m == 0, no candidate order: q and shift are then order 1's places, which nobody may have written -- they are not used;
	 * the lanes still store their zero sums and reach the barriers with the other waves) */
	const int16_t *q = &L.q[c][(m ? m - 1 : 0) * FLAC_LPC_MAX];
	const unsigned shift = L.shift[c][m ? m - 1 : 0];
	if (m)
		for (unsigned i = i0 > m ? i0 : m; i < i0 + run; ++i) {
			const uint32_t u = flac_zigzag(flac_lpc_residual(W::at(s_w, R0, c, (int)i), flac_lpc_sum<W>(s_w, R0, c, q, m, i), shift));
#pragma unroll
			for (unsigned k = 0; k < W::NK; ++k) f64[k] += u >> k;
		}
#pragma unroll
	for (unsigned k = 0; k < W::NK; ++k) {
		const unsigned long long s = flac_wave_sum(f64[k], 2);
		if ((lane & 3) == 0) s_fine[c][(lane >> 2) * W::NK + k] = s;
	}
	__syncthreads();
	if (m && lane < FLAC_NODES) {
		const unsigned p = 31 - __clz((int)(lane + 1)), part = lane + 1 - (1u << p);
		unsigned k;
		s_node_cost[c][lane] = flac_node_cost(s_fine[c], W::NK, 4, p, part, n, m, &k);
		s_node_k[c][lane] = (uint8_t)k;
	}
	__syncthreads();
	if (m && lane == 0) flac_lpc_choose(&s_cand[c], n, m, q, shift, 4, s_node_cost[c], s_node_k[c], W::BITS);
}

template <typename W, bool LPC>
__global__ __launch_bounds__(256) void flac_analyze_kernel(const FlacParams P) {
	extern __shared__ uint32_t flac_lds[];
	__shared__ uint64_t s_fine[4][FLAC_FINE * W::NK];
	__shared__ uint64_t s_node_cost[4][32];
	__shared__ uint8_t s_node_k[4][32];
	__shared__ FlacSub s_cand[4];
	uint32_t *s_w = flac_lds;
	const unsigned R0 = W::lds_words(P.B, 1);
	const unsigned job = blockIdx.x, row = flac_find_row(P.desc, P.n_rows, job);
	const FlacRow d = P.desc[row];
	const unsigned j = job - d.job0;
	if (j >= d.n_blocks) return; /* (never: the jobs are the rows' blocks; uniform) */
	const unsigned n = j == d.n_blocks - 1 ? d.last_n : P.B;
	W::stage(P, d, row, j, n, s_w, R0);
	__syncthreads();
	const unsigned c = threadIdx.x >> 6, lane = threadIdx.x & 63; /* one wave per candidate */
	/* constant? and the five orders' sums of |r_i|, i = 4 .. n-1 */
	const int32_t s_first = W::at(s_w, R0, c, 0);
	bool eq = true;
	typename W::run_t a[5] = {0, 0, 0, 0, 0};
	for (unsigned i = lane; i < n; i += 64) {
		const int32_t s0 = W::at(s_w, R0, c, (int)i);
		eq = eq && s0 == s_first;
		if (i >= 4) {
			int32_t r[5];
			flac_residuals(s0, W::at(s_w, R0, c, (int)i - 1), W::at(s_w, R0, c, (int)i - 2), W::at(s_w, R0, c, (int)i - 3), W::at(s_w, R0, c, (int)i - 4), r);
#pragma unroll
			for (int o = 0; o < 5; ++o) a[o] += flac_abs(r[o]);
		}
	}
	const bool equal = __all(eq ? 1 : 0) != 0;
	uint64_t abs_sum[5];
#pragma unroll
	for (int o = 0; o < 5; ++o) abs_sum[o] = flac_wave_sum(a[o], 6);
	const unsigned o = flac_pick_order(n, abs_sum);
	/* the sums of u >> k per finest partition: a whole block has sixteen, four lanes each, a lane a run of consecutive frames */
	const unsigned fine_log2 = n == P.B ? 4 : 0;
	typename W::run_t f[W::NK];
#pragma unroll
	for (unsigned k = 0; k < W::NK; ++k) f[k] = 0;
	if (fine_log2) {
		const unsigned run = n >> 6, i0 = lane * run; /* (lane >> 2 is the partition) */
		int32_t s1 = W::at(s_w, R0, c, (int)i0 - 1), s2 = W::at(s_w, R0, c, (int)i0 - 2), s3 = W::at(s_w, R0, c, (int)i0 - 3), s4 = W::at(s_w, R0, c, (int)i0 - 4);
		for (unsigned i = i0; i < i0 + run; ++i) {
			const int32_t s0 = W::at(s_w, R0, c, (int)i);
			if (i >= o) {
				const uint32_t u = flac_zigzag(flac_residual(o, s0, s1, s2, s3, s4));
#pragma unroll
				for (unsigned k = 0; k < W::NK; ++k) f[k] += u >> k;
			}
			s4 = s3; s3 = s2; s2 = s1; s1 = s0;
		}
	} else {
		for (unsigned i = lane; i < n; i += 64)
			if (i >= o) {
				const uint32_t u = flac_zigzag(flac_residual(o, W::at(s_w, R0, c, (int)i), W::at(s_w, R0, c, (int)i - 1), W::at(s_w, R0, c, (int)i - 2),
						W::at(s_w, R0, c, (int)i - 3), W::at(s_w, R0, c, (int)i - 4)));
#pragma unroll
				for (unsigned k = 0; k < W::NK; ++k) f[k] += u >> k;
			}
	}
#pragma unroll
	for (unsigned k = 0; k < W::NK; ++k) {
		const unsigned long long s = flac_wave_sum(f[k], fine_log2 ? 2 : 6);
		if (fine_log2 ? (lane & 3) == 0 : lane == 0) s_fine[c][(fine_log2 ? lane >> 2 : 0) * W::NK + k] = s;
	}
	__syncthreads();
	/* one lane per (p, partition): the best k and its cost */
	if (lane < (fine_log2 ? FLAC_NODES : 1u)) {
		const unsigned p = 31 - __clz((int)(lane + 1)), part = lane + 1 - (1u << p);
		unsigned k;
		s_node_cost[c][lane] = flac_node_cost(s_fine[c], W::NK, fine_log2, p, part, n, o, &k);
		s_node_k[c][lane] = (uint8_t)k;
	}
	__syncthreads();
	if (lane == 0) flac_finish_sub(&s_cand[c], c, n, equal, o, fine_log2, s_node_cost[c], s_node_k[c], W::BITS);
	__syncthreads();
	if constexpr (LPC) if (n == P.B) { /* (the same for the whole workgroup) */
		__shared__ FlacLpcLds s_lpc;
		flac_analyze_lpc<W>(P, s_w, R0, s_lpc, s_fine, s_node_cost, s_node_k, s_cand, c, lane, equal);
		__syncthreads();
	}
	if (threadIdx.x == 0) flac_finish_frame(&P.frames[job], s_cand, P.channels, n, P.B, (uint32_t)(d.block0 + j));
}

/* the exclusive sum of v over the 256 threads; s_scan[4] holds the waves' totals behind it */
__device__ __forceinline__ uint32_t flac_block_excl(const uint32_t v, uint32_t *s_scan) {
	const uint32_t incl = wave_incl_scan_dpp(v);
	const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	__syncthreads(); /* (whoever still reads the totals of the call before) */
	if (lane == 63) s_scan[wave] = incl;
	__syncthreads();
	uint32_t base = 0;
	for (unsigned w = 0; w < wave; ++w) base += s_scan[w];
	return base + incl - v;
}

__global__ __launch_bounds__(FLAC_THREADS) void flac_scan_kernel(const FlacParams P) {
	__shared__ uint32_t s_scan[4], s_min, s_max;
	const unsigned row = blockIdx.x, tid = threadIdx.x;
	const FlacRow d = P.desc[row];
	if (tid == 0) { s_min = 0xffffffffu; s_max = 0; }
	uint32_t running = 0;
	for (unsigned t0 = 0; t0 < d.n_blocks; t0 += FLAC_THREADS) { /* (uniform) */
		const unsigned j = t0 + tid;
		const uint32_t len = j < d.n_blocks ? P.frames[d.job0 + j].bytes : 0;
		const uint32_t excl = flac_block_excl(len, s_scan);
		if (j < d.n_blocks) {
			P.frames[d.job0 + j].off = running + excl;
			atomicMin(&s_min, len);
			atomicMax(&s_max, len);
		}
		running += s_scan[0] + s_scan[1] + s_scan[2] + s_scan[3];
	}
	__syncthreads();
	if (tid == 0) {
		P.row_bytes[row] = running;
		if (d.n_blocks) {
			FlacStats st = P.stats[row];
			st.bytes += running;
			st.min_bytes = st.max_bytes ? (s_min < st.min_bytes ? s_min : st.min_bytes) : s_min;
			st.max_bytes = s_max > st.max_bytes ? s_max : st.max_bytes;
			P.stats[row] = st;
		}
	}
}

/* `bits` (1 .. 32) bits of v at bit `pos` of the frame, MSB first, into words that hold zeros there */
__device__ __forceinline__ void flac_put(uint32_t *s_f, const uint32_t n_words, const uint32_t pos, const uint32_t bits, const uint32_t v) {
	const uint32_t w = pos >> 5;
	const unsigned long long x = (unsigned long long)v << (64 - (pos & 31) - bits);
	const uint32_t hi = (uint32_t)(x >> 32), lo = (uint32_t)x;
	if (hi && w < n_words) atomicOr(&s_f[w], hi);
	if (lo && w + 1 < n_words) atomicOr(&s_f[w + 1], lo);
}
__device__ __forceinline__ uint32_t flac_byte(const uint32_t *s_f, const uint32_t b) { return (s_f[b >> 2] >> (24 - 8 * (b & 3))) & 0xffu; }

/* the residual of frame i (>= the order) of a FIXED subframe, or, in the <true> kernel, of an LPC one */
template <typename W, bool LPC>
__device__ __forceinline__ int32_t flac_sub_residual(const uint32_t *s_w, const unsigned R0, const FlacSub &s, const unsigned c, const unsigned o,
		const unsigned i) {
	if (LPC && s.type == FLAC_LPC) return flac_lpc_residual(W::at(s_w, R0, c, (int)i), flac_lpc_sum<W>(s_w, R0, c, s.q, o, i), s.shift);
	return flac_residual(o, W::at(s_w, R0, c, (int)i), W::at(s_w, R0, c, (int)i - 1), W::at(s_w, R0, c, (int)i - 2), W::at(s_w, R0, c, (int)i - 3),
			W::at(s_w, R0, c, (int)i - 4));
}

template <typename W, bool LPC>
__global__ __launch_bounds__(FLAC_THREADS) void flac_write_kernel(const FlacParams P) {
	extern __shared__ uint32_t flac_lds[];
	__shared__ uint32_t s_scan[4], s_crc;
	__shared__ FlacFrameDesc s_fd; /* (in LDS: its fields are picked by index) */
	__shared__ uint8_t s_head[16];
	const unsigned R0 = W::lds_words(P.B, 1);
	uint32_t *s_w = flac_lds, *s_f = flac_lds + W::lds_words(P.B, P.channels);
	const uint32_t n_words = flac_frame_bound(P.B, P.channels, W::BITS) / 4 + 2;
	const unsigned tid = threadIdx.x, job = blockIdx.x, row = flac_find_row(P.desc, P.n_rows, job);
	const FlacRow d = P.desc[row];
	const unsigned j = job - d.job0;
	if (j >= d.n_blocks) return; /* (never; uniform) */
	const unsigned n = j == d.n_blocks - 1 ? d.last_n : P.B;
	if (tid < sizeof(FlacFrameDesc) / 4) ((uint32_t *)&s_fd)[tid] = ((const uint32_t *)&P.frames[job])[tid];
	__syncthreads();
	const FlacFrameDesc &fd = s_fd;
	const uint32_t number = (uint32_t)(d.block0 + j);
	const uint32_t head = flac_header_len(n, P.B, number);
	if (fd.n != n || fd.bytes > flac_frame_bound(n, P.channels, W::BITS) || fd.bytes < head + 2 || fd.n_sub > 2) return; /* (never: the record is this block's; uniform) */
	W::stage(P, d, row, j, n, s_w, R0);
	for (unsigned i = tid; i < n_words; i += FLAC_THREADS) s_f[i] = 0;
	if (tid == 0) s_crc = 0;
	__syncthreads();
	if (tid == 0) {
		const uint32_t hl = flac_frame_header(n, P.B, fd.assign, number, W::BITS, s_head);
		for (uint32_t i = 0; i < hl; ++i) flac_put(s_f, n_words, 8 * i, 8, s_head[i]);
	}
	const unsigned log2B = 31 - __clz((int)P.B);
	uint32_t pos = 8 * head;
	for (unsigned si = 0; si < fd.n_sub; ++si) { /* (everything that branches here is the same for the whole workgroup) */
		const FlacSub &s = fd.sub[si];
		const unsigned c = s.cand, bps = flac_cand_bps(c, W::BITS);
		const uint32_t mask = bps == W::BITS + 1 ? (2u << W::BITS) - 1 : (1u << W::BITS) - 1;
		const bool lpc = LPC && s.type == FLAC_LPC;
		if (tid == 0) flac_put(s_f, n_words, pos, 8, s.type == FLAC_CONSTANT ? 0u : s.type == FLAC_VERBATIM ? 2u :
				lpc ? (uint32_t)(0x40u | ((s.order - 1u) << 1)) : (uint32_t)(0x10u | (s.order << 1)));
		if (s.type == FLAC_CONSTANT) {
			if (tid == 0) flac_put(s_f, n_words, pos + 8, bps, (uint32_t)W::at(s_w, R0, c, 0) & mask);
		} else if (s.type == FLAC_VERBATIM) {
			for (unsigned i = tid; i < n; i += FLAC_THREADS) flac_put(s_f, n_words, pos + 8 + bps * i, bps, (uint32_t)W::at(s_w, R0, c, (int)i) & mask);
		} else {
			const unsigned o = s.order, p = s.p;
			if (tid < o) flac_put(s_f, n_words, pos + 8 + bps * tid, bps, (uint32_t)W::at(s_w, R0, c, (int)tid) & mask);
			uint32_t at_res = pos + 8 + bps * o;
			if (lpc) { /* 1011, the shift, the coefficients */
				if (tid == 0) {
					flac_put(s_f, n_words, at_res, 9, ((FLAC_LPC_PREC - 1) << 5) | s.shift);
					for (unsigned j = 0; j < o; ++j) flac_put(s_f, n_words, at_res + 9 + FLAC_LPC_PREC * j, FLAC_LPC_PREC, (uint32_t)s.q[j] & 0xfffu);
				}
				at_res += 9 + FLAC_LPC_PREC * o;
			}
			if (tid == 0) flac_put(s_f, n_words, at_res, 6, (W::METHOD << 4) | p); /* 00 pppp or 01 pppp */
			/* a thread's run of consecutive frames; partition of frame i: i >> (log2 B - p) -- p > 0 only in a whole block */
			const unsigned run = (n + FLAC_THREADS - 1) / FLAC_THREADS, i0 = tid * run, i1 = i0 + run < n ? i0 + run : n;
			const unsigned psh = p ? log2B - p : 31, pmask = p ? (1u << psh) - 1 : 0xffffffffu;
			uint32_t len = 0; /* (32 bits: the subframe is cheaper than its verbatim form, below 2^18 bits) */
			for (unsigned i = i0 > o ? i0 : o; i < i1; ++i) {
				const unsigned k = s.k[i >> psh];
				const uint32_t u = flac_zigzag(flac_sub_residual<W, LPC>(s_w, R0, s, c, o, i));
				len += (u >> k) + 1 + k + ((i & pmask) == 0 || i == o ? W::K_BITS : 0);
			}
			uint32_t b = at_res + 6 + flac_block_excl(len, s_scan);
			for (unsigned i = i0 > o ? i0 : o; i < i1; ++i) {
				const unsigned k = s.k[i >> psh];
				const uint32_t u = flac_zigzag(flac_sub_residual<W, LPC>(s_w, R0, s, c, o, i));
				if ((i & pmask) == 0 || i == o) { flac_put(s_f, n_words, b, W::K_BITS, k); b += W::K_BITS; }
				b += u >> k;
				flac_put(s_f, n_words, b, k + 1, (1u << k) | (u & ((1u << k) - 1))); /* (at most 31 bits) */
				b += k + 1;
			}
		}
		pos += s.bits;
	}
	__syncthreads();
	const uint32_t body = fd.bytes - 2; /* (pos + 7) / 8 by the analysis' count */
	{ /* CRC-16: a run of bytes per thread, advanced over what follows it, all XORed */
		const uint32_t run = (body + FLAC_THREADS - 1) / FLAC_THREADS, b0 = tid * run, b1 = b0 + run < body ? b0 + run : body;
		uint32_t crc = 0;
		for (uint32_t b = b0; b < b1; ++b) crc = flac_crc16_update(crc, flac_byte(s_f, b));
		crc = b0 < body ? flac_crc16_advance(crc, body - b1) : 0;
		for (int m = 1; m < 64; m <<= 1) crc ^= __shfl_xor(crc, m);
		if ((tid & 63) == 0) atomicXor(&s_crc, crc);
	}
	__syncthreads();
	uint8_t *dst = P.out + d.out_off + fd.off;
	for (uint32_t b = tid; b < body; b += FLAC_THREADS) dst[b] = (uint8_t)flac_byte(s_f, b);
	if (tid == 0) { dst[body] = (uint8_t)(s_crc >> 8); dst[body + 1] = (uint8_t)s_crc; }
}

template <typename W>
__global__ __launch_bounds__(FLAC_THREADS) void flac_carry_kernel(const FlacParams P) {
	typedef typename W::sample_t T;
	const unsigned e = blockIdx.x * FLAC_THREADS + threadIdx.x, row = blockIdx.y, ch = P.channels;
	const FlacRow d = P.desc[row];
	if (e >= d.pend_next * ch) return;
	const T *xrow = (const T *)((const char *)P.rows + P.row_pitch * row);
	const T *pend = (const T *)P.pend + P.pend_pitch * row;
	const unsigned long long at = (unsigned long long)d.n_blocks * P.B * ch + e; /* counted from the row's frame block0 * B, in samples */
	((T *)P.pend_next)[P.pend_pitch * row + e] = at < (unsigned long long)d.pend * ch ? pend[at] : xrow[at - (unsigned long long)d.pend * ch];
}

/* ---- the float-fed encoders' quantiser ---- */
struct FlacQuantRow {
	unsigned long long n;     /* samples of the row's feed */
	float gain;
	uint32_t pad_;
};
static_assert(sizeof(FlacQuantRow) == 16, "FlacQuantRow is uploaded as it stands");
struct FlacQuantParams {
	const float *src;         /* the fed rows */
	size_t src_pitch;         /* bytes */
	void *dst;                /* the encoder's rows: 256-byte aligned */
	size_t dst_pitch;         /* bytes, a multiple of 256 */
	const FlacQuantRow *rows; /* [grid.y] */
};
template <typename OutT>
__global__ __launch_bounds__(256) void flac_quant_kernel(const FlacQuantParams P) {
	typedef float __attribute__((ext_vector_type(4))) f32x4;
	typedef uint32_t __attribute__((ext_vector_type(2))) u32x2;
	typedef int32_t __attribute__((ext_vector_type(4))) i32x4;
	const unsigned row = blockIdx.y;
	const FlacQuantRow d = P.rows[row];
	const float *src = (const float *)((const char *)P.src + P.src_pitch * row);
	OutT *dst = (OutT *)((char *)P.dst + P.dst_pitch * row);
	const unsigned head = (unsigned)((16u - (unsigned)((uintptr_t)src & 15u)) & 15u) >> 2; /* samples ahead of the first 16-byte boundary */
	const unsigned long long t = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
	const unsigned long long i0 = t ? head + (t - 1) * 4 : 0;
	const unsigned cnt = t ? 4 : head;
	if (i0 >= d.n) return;
	auto one = [&](float x) -> OutT {
		const float y = x * d.gain;
		if constexpr (std::is_same<OutT, int16_t>::value) return pcm16(y);
		else return pcm24(y);
	};
	if (cnt == 4 && i0 + 4 <= d.n) {
		const f32x4 q = __builtin_nontemporal_load((const f32x4 *)(src + i0));
		const OutT a = one(q.x), b = one(q.y), c = one(q.z), e = one(q.w);
		if (head) { dst[i0] = a; dst[i0 + 1] = b; dst[i0 + 2] = c; dst[i0 + 3] = e; }
		else if constexpr (std::is_same<OutT, int16_t>::value) {
			u32x2 w;
			w.x = (uint32_t)(uint16_t)a | ((uint32_t)(uint16_t)b << 16);
			w.y = (uint32_t)(uint16_t)c | ((uint32_t)(uint16_t)e << 16);
			*(u32x2 *)(dst + i0) = w;
		} else {
			i32x4 w; w.x = a; w.y = b; w.z = c; w.w = e;
			*(i32x4 *)(dst + i0) = w;
		}
		return;
	}
	const unsigned long long i1 = i0 + cnt < d.n ? i0 + cnt : d.n;
	for (unsigned long long i = i0; i < i1; ++i) dst[i] = one(src[i]);
}

#endif
