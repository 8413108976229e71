/* k_limiter.h -- the look-ahead true-peak limiter on float rows: part of hip_backend.hip (inside namespace sauhip).
 *   lim_env_kernel<CH>         grid (env tiles, streams) x LIM_THREADS. A workgroup owns LIM_ENV_TILE positions of one stream's
 *       scratch: it stages the frames around them, forms the 4x interpolated points w (truepeak_kernel's chains, each point
 *       once, shared through LDS by the two frames it lies beside), the linked envelope e, and writes the required gain r and
 *       s = 1 - r as f64.
 *   lim_gain_kernel<OutT, CH>  grid (tiles, streams) x LIM_THREADS. A workgroup owns LIM_TILE output frames: it stages s over
 *       the tile and 4A frames, forms the hold d -- the sliding maximum over 2A + 1 -- in place by doubling, runs the 2A + 1-tap
 *       f64 chain of the smoothing window per output frame, multiplies, stores, and leaves ONE record (the smallest gain, the
 *       number of frames with G < 1) per workgroup.
 *   lim_finish_kernel          one wave per stream: the workgroups' records into the stream's statistics.
 *   lim_carry_kernel           grid (parts, streams): the stream's history becomes the last LIM_HIST = 4A + 32 frames of (old
 *       history, this run's cleaned, zero-extended input), from one buffer into the other (the backend swaps them): no run
 *       length needs an in-place shift.
 *
 * The arithmetic (include/saugns_amd.h, section "Limiter") is a function of the input sequence only. Nothing
 * recursive is carried: a run recomputes w, e, r, s and d over the 4A + 31 frames of history it needs, so cutting the
 * sequence into runs, or a run into tiles, cannot change a bit. Every sum has one accumulator per output value, a product and
 * then a sum (the build is -ffp-contract=off), never split or folded over the window's symmetry; a maximum of non-negative
 * finite doubles is exact in any order, so the doubling is free to group it as it likes; the statistics are a minimum and an
 * integer count. No atomics.
 *
 * Positions. With base = (the sequence's frame of output 0) - 2A, relative to the run's first frame, scratch position u holds
 * s and r of frame base + u; output o reads s at u = o .. o + 4A, r and x at u = o + 2A. x comes from the history (frames
 * below 0), the row (below the stream's frame count of the run, cleaned) or is +0.
 *
 * LDS. lim_env_kernel: the span is staged with the channels apart, s_x[channel][frame], as truepeak_kernel has it: at a
 * wave-uniform tap consecutive lanes read consecutive dwords (ds_read_b32, thirty-two lanes on thirty-two banks); the staging
 * stores are ds_write_b32, at most 2-way; the taps are a const __restrict__ argument at wave-uniform indices: scalar loads.
 * The points w[m] a tile needs are LIM_ENV_TILE + 1: one more than its threads, so wave 0 makes a second trip for the last.
 * lim_gain_kernel: s is f64, s_s[position]: lane l reads ds_read_b64 at consecutive 8-byte addresses -- thirty-two lanes on
 * sixty-four banks of dwords, the bank of a ds_read_b64 being (a / 4) % 64 -- and writes ds_write_b64, sixteen contiguous
 * lanes on thirty-two banks: conflict-free both ways, in the doubling steps (offsets are whole doubles) and in the chain,
 * where the window's tap is wave-uniform and again a scalar load. The span is LIM_TILE + 4A doubles, 36 KiB at A = 1024:
 * static, and four workgroups to a CU at the largest look-ahead. d is not kept beside s: each doubling step reads its
 * LIM_SPAN_PER_THREAD values into registers, waits, and writes them back, so the span is the only large array. */
#ifndef SAU_K_LIMITER_H
#define SAU_K_LIMITER_H

struct LimStats { unsigned long long frames, limited; double min_gain; };
static_assert(sizeof(LimStats) == sizeof(sauengine::LimiterStats), "sauAmdLimiterStats");

struct LimParams {
	const float *rows;        /* the float rows; not read where frames[] is 0 */
	size_t row_pitch;         /* bytes between them */
	const uint32_t *frames;   /* [streams]: the frames of this run that are the stream's; behind them x is +0 */
	const float *hist;        /* [streams][hist_frames * CH], cleaned: the frames ahead of this run; NULL: all +0 */
	float *hist_next;         /* lim_carry_kernel's target */
	double *s, *r;            /* [streams][scratch_pitch] */
	size_t scratch_pitch;     /* doubles */
	void *out;                /* OutT[streams][..], out_pitch bytes apart */
	size_t out_pitch;
	double *part_min;         /* [streams][tiles] */
	uint32_t *part_cnt;       /* [streams][tiles] */
	LimStats *stats;          /* [streams] */
	long long base;           /* the run-relative frame of scratch position 0 */
	uint32_t n_out;           /* output frames */
	uint32_t env_n;           /* scratch positions: n_out + 4A */
	uint32_t A, hist_frames;
	uint32_t tiles;           /* lim_gain_kernel's grid.x */
	uint32_t n_streams;
	uint32_t run_frames;      /* lim_carry_kernel: the run's frames, zero-extended input included */
	uint32_t swap_bytes;      /* int16 rows: big-endian */
	float pre_gain, ceiling;
};

/* the cleaned sample of run-relative frame j: the history below 0, the row below the stream's n frames, +0 elsewhere */
template <int CH>
__device__ __forceinline__ float lim_x(const float *row, const float *hist, const long long hist_frames, const long long j, const int ch,
		const long long n) {
	if (j < 0) {
		const long long h = j + hist_frames;
		return hist && h >= 0 ? hist[h * CH + ch] : 0.f;
	}
	return j < n ? loud_clean(row[j * CH + ch]) : 0.f;
}

template <int CH>
__global__ __launch_bounds__(LIM_THREADS) void lim_env_kernel(const LimParams P, const double *__restrict__ taps) {
	constexpr int SPAN_FR = (int)(LIM_ENV_TILE + TP_LEAD); /* frames k0 - 16 .. k0 + TILE + 15 of the tile that begins at k0 */
	__shared__ float s_x[CH * SPAN_FR];          /* [channel][frame] */
	__shared__ uint32_t s_w[LIM_ENV_TILE + 1];   /* the largest finite |w[m][p][ch]| of m = k0 + 15 + i, as bits */
	const uint32_t stream = blockIdx.y, tid = threadIdx.x;
	const uint32_t u0 = blockIdx.x * LIM_ENV_TILE;
	const long long k0 = P.base + (long long)u0, n = P.frames[stream];
	const float *row = (const float *)((const char *)P.rows + P.row_pitch * stream);
	const float *hist = P.hist ? P.hist + (size_t)stream * P.hist_frames * CH : nullptr;
	for (int i = (int)tid; i < SPAN_FR * CH; i += (int)LIM_THREADS) {
		const int fr = i / CH, ch = i % CH;
		s_x[ch * SPAN_FR + fr] = lim_x<CH>(row, hist, P.hist_frames, k0 - (long long)TP_HALF + fr, ch, n);
	}
	__syncthreads();
	for (int i = (int)tid; i < (int)LIM_ENV_TILE + 1; i += (int)LIM_THREADS) {
		uint32_t best = 0u;
#pragma unroll
		for (int ch = 0; ch < CH; ++ch) {
			/* tap q of every phase meets frame m - q, m = k0 + 15 + i: span frame 31 + i - q */
			const float *at = s_x + ch * SPAN_FR + (int)TP_HIST + i;
			double a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll 4
			for (int q = 0; q < 2 * (int)TP_HALF; ++q) {
				const double g1 = taps[4 * q + 1], g2 = taps[4 * q + 2], g3 = taps[4 * q + 3];
				const double d = (double)at[-q];
				a1 = a1 + g1 * d;
				a2 = a2 + g2 * d;
				a3 = a3 + g3 * d;
			}
			const uint32_t w1 = __float_as_uint((float)a1) & 0x7fffffffu, w2 = __float_as_uint((float)a2) & 0x7fffffffu,
				w3 = __float_as_uint((float)a3) & 0x7fffffffu;
			best = w1 < 0x7f800000u && w1 > best ? w1 : best;
			best = w2 < 0x7f800000u && w2 > best ? w2 : best;
			best = w3 < 0x7f800000u && w3 > best ? w3 : best;
		}
		s_w[i] = best;
	}
	__syncthreads();
	const uint32_t u = u0 + tid;
	if (u >= P.env_n) return;
	/* frame k = k0 + tid: the sample (span frame 16 + tid) and the points of m = k + 15 and m = k + 16 */
	uint32_t e = s_w[tid] > s_w[tid + 1] ? s_w[tid] : s_w[tid + 1];
#pragma unroll
	for (int ch = 0; ch < CH; ++ch) {
		const uint32_t ax = __float_as_uint(s_x[ch * SPAN_FR + (int)TP_HALF + (int)tid]) & 0x7fffffffu; /* (cleaned: finite) */
		e = ax > e ? ax : e;
	}
	const double E = (double)__uint_as_float(e) * (double)P.pre_gain, c = (double)P.ceiling;
	const double r = E <= c ? 1.0 : c / E;
	const size_t at = (size_t)stream * P.scratch_pitch + u;
	P.r[at] = r;
	P.s[at] = 1.0 - r;
}

template <typename OutT, int CH>
__global__ __launch_bounds__(LIM_THREADS) void lim_gain_kernel(const LimParams P, const double *__restrict__ win) {
	__shared__ __attribute__((aligned(16))) double s_s[LIM_SPAN_MAX];
	__shared__ double s_min[LIM_THREADS / 64];
	__shared__ uint32_t s_cnt[LIM_THREADS / 64];
	const uint32_t stream = blockIdx.y, tid = threadIdx.x;
	const uint32_t o0 = blockIdx.x * LIM_TILE;
	const int A = (int)P.A, N = (int)LIM_TILE + 4 * A, W = 2 * A + 1;
	const double *sp = P.s + (size_t)stream * P.scratch_pitch + o0;
	for (int i = (int)tid; i < N; i += (int)LIM_THREADS) s_s[i] = o0 + (uint32_t)i < P.env_n ? sp[i] : 0.0;
	__syncthreads();
	/* s_s[i] = max(s_s[i], s_s[i + w]): a window of p frames becomes one of p + w; positions whose window would pass the span's
	 * end keep a partial maximum that nothing reads (output t reads i = t .. t + 2A, whose windows end at t + 4A < N) */
	auto widen = [&](const int w) {
		double t[LIM_SPAN_PER_THREAD];
#pragma unroll
		for (int k = 0; k < (int)LIM_SPAN_PER_THREAD; ++k) {
			const int i = (int)tid + k * (int)LIM_THREADS;
			t[k] = 0.0;
			if (i < N) {
				const double a = s_s[i];
				t[k] = a;
				if (i + w < N) { const double b = s_s[i + w]; t[k] = b > a ? b : a; }
			}
		}
		__syncthreads();
#pragma unroll
		for (int k = 0; k < (int)LIM_SPAN_PER_THREAD; ++k) {
			const int i = (int)tid + k * (int)LIM_THREADS;
			if (i < N) s_s[i] = t[k];
		}
		__syncthreads();
	};
	int p = 1;
	while (2 * p <= W) { widen(p); p *= 2; }
	widen(W - p); /* (W is odd and p a power of two, 2 at least: 1 <= W - p < p) */
	/* s_s[i] is now d[i + A] of the span: output t of the tile meets d[t - A + j] at s_s[t + j] */
	double acc[LIM_PER_LANE];
#pragma unroll
	for (int q = 0; q < (int)LIM_PER_LANE; ++q) acc[q] = 0.0;
	const double *mine = s_s + tid;
#pragma unroll 4
	for (int j = 0; j < W; ++j) {
		const double h = win[j];
#pragma unroll
		for (int q = 0; q < (int)LIM_PER_LANE; ++q) acc[q] = acc[q] + h * mine[q * (int)LIM_THREADS + j];
	}
	const long long n = P.frames[stream];
	const float *row = (const float *)((const char *)P.rows + P.row_pitch * stream);
	const float *hist = P.hist ? P.hist + (size_t)stream * P.hist_frames * CH : nullptr;
	OutT *out = (OutT *)((char *)P.out + P.out_pitch * stream);
	const double g0 = (double)P.pre_gain;
	double mn = 1.0;
	uint32_t cnt = 0;
#pragma unroll
	for (int q = 0; q < (int)LIM_PER_LANE; ++q) {
		const uint32_t o = o0 + (uint32_t)q * LIM_THREADS + tid;
		if (o >= P.n_out) continue;
		const double r = P.r[(size_t)stream * P.scratch_pitch + o + 2 * (uint32_t)A], sm = 1.0 - acc[q];
		const double G = sm < r ? sm : r;
		mn = G < mn ? G : mn;
		cnt += G < 1.0 ? 1u : 0u;
		const long long c = P.base + (long long)o + 2 * A;
		float y[CH];
#pragma unroll
		for (int ch = 0; ch < CH; ++ch) y[ch] = (float)(((double)lim_x<CH>(row, hist, P.hist_frames, c, ch, n) * g0) * G);
		if constexpr (std::is_same<OutT, float>::value) {
#pragma unroll
			for (int ch = 0; ch < CH; ++ch) out[(size_t)o * CH + ch] = y[ch];
		} else {
#pragma unroll
			for (int ch = 0; ch < CH; ++ch) { const int16_t s16 = pcm16(y[ch]); out[(size_t)o * CH + ch] = P.swap_bytes ? pcm_swap(s16) : s16; }
		}
	}
#pragma unroll
	for (int off = 32; off >= 1; off >>= 1) {
		const double om = __shfl_xor(mn, off);
		mn = om < mn ? om : mn;
		cnt += (uint32_t)__shfl_xor((int)cnt, off);
	}
	if ((tid & 63u) == 0) { s_min[tid >> 6] = mn; s_cnt[tid >> 6] = cnt; }
	__syncthreads();
	if (tid == 0) {
#pragma unroll
		for (int k = 1; k < (int)(LIM_THREADS / 64); ++k) { mn = s_min[k] < mn ? s_min[k] : mn; cnt += s_cnt[k]; }
		const size_t at = (size_t)stream * P.tiles + blockIdx.x;
		P.part_min[at] = mn;
		P.part_cnt[at] = cnt;
	}
}

/* One wave per stream: the tiles' records into the stream's statistics. A minimum and an integer count have no order, so the
 * lanes take the tiles 64 apart and the wave folds them by __shfl_xor. */
__global__ __launch_bounds__(64) void lim_finish_kernel(const LimParams P) {
	const uint32_t stream = blockIdx.x, lane = threadIdx.x;
	const double *pm = P.part_min + (size_t)stream * P.tiles;
	const uint32_t *pc = P.part_cnt + (size_t)stream * P.tiles;
	double mn = 1.0;
	unsigned long long cnt = 0;
	for (uint32_t t = lane; t < P.tiles; t += 64) {
		mn = pm[t] < mn ? pm[t] : mn;
		cnt += pc[t];
	}
#pragma unroll
	for (int off = 32; off >= 1; off >>= 1) {
		const double om = __shfl_xor(mn, off);
		mn = om < mn ? om : mn;
		cnt += (unsigned long long)__shfl_xor((long long)cnt, off);
	}
	if (lane != 0) return;
	LimStats st = P.stats[stream];
	st.min_gain = mn < st.min_gain ? mn : st.min_gain;
	st.limited += cnt;
	st.frames += P.n_out;
	P.stats[stream] = st;
}

/* The history moves on by the run's run_frames frames: with X = (old history, the stream's n frames cleaned, zeros up to
 * run_frames), the new history is X's last hist_frames frames -- read from one buffer, written to the other. */
__global__ __launch_bounds__(LIM_THREADS) void lim_carry_kernel(const LimParams P, const uint32_t ch) {
	const uint32_t stream = blockIdx.y, hf = P.hist_frames * ch;
	const uint32_t k = blockIdx.x * LIM_THREADS + threadIdx.x;
	if (k >= hf) return;
	const float *row = (const float *)((const char *)P.rows + P.row_pitch * stream);
	const unsigned long long e = (unsigned long long)P.run_frames * ch + k, nfl = (unsigned long long)P.frames[stream] * ch;
	float v = 0.f;
	if (e < hf) v = P.hist[(size_t)stream * hf + e];
	else if (e - hf < nfl) v = loud_clean(row[e - hf]);
	P.hist_next[(size_t)stream * hf + k] = v;
}

#endif
