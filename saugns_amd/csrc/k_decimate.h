/* k_decimate.h -- the decimating FIR of oversampled rendering: part of hip_backend.hip (inside namespace sauhip).
 *   decimate_kernel<K, OutT, CH>  grid (tiles, streams) x DECIM_THREADS (one wave). A workgroup owns DECIM_TILE consecutive
 *       output frames of one stream (launch_plan.h: plan_decimate -- a constant), stages the tile's input span
 *       (DECIM_TILE + 2H) * K frames of CH channels into LDS with 16-byte loads, phase by phase, and every lane then runs
 *       DECIM_PER_LANE * CH f64 chains over the L taps.
 *   decimate_carry_kernel         one workgroup per stream, after decimate_kernel on the same stream: the stream's history
 *       becomes the last L - 1 frames of (old history, this run's zero-extended input).
 *
 * The arithmetic (include/saugns_amd.h: sauAmd_Batch_run_decimated_f32) is reproducible bit for bit:
 *   acc = +0.0 (f64); for j = 0 .. L-1 ascending: acc = acc + h[j] * (double)x[m * K - j]; y[m] = (float)acc
 * -- one accumulator per output sample, a multiply and then an add (the build is -ffp-contract=off), no sum split, folded
 * over the filter's symmetry or shared between lanes. x[i] is +0.0f below the start of the sequence (the history is zeroed
 * there) and at or behind the stream's frame count of the run, whatever the row holds. Those zero terms are not skipped
 * here: acc can never be -0, so adding +-0 changes nothing either way.
 *
 * The span in LDS. Lane t of the tile reads x[(t0 + t) * K - j] at the wave-uniform tap j: as the samples lie, a stride of
 * K (mono) or 2K (stereo) floats across the wave, a K- or 2K-way bank conflict. So the span is staged by phase -- with
 * span frame s = q * K + p, s_x[p][q][c] -- and at tap j = L - 1 - (qo * K + p) lane t reads s_x[p][t + qo][..]: consecutive
 * lanes, consecutive addresses. Mono: ds_read_b32 at consecutive dwords, 32 lanes on 32 banks. Stereo: the two channels of
 * a frame side by side, one ds_read_b64 per frame, 32 lanes on 64 banks. Conflict-free both ways (MI355X: LDS banking is
 * per instruction, in groups of 32 lanes). The staging stores are scattered ds_write_b32 (at most 2-way: free) -- 20 vectors
 * a lane, beside 8 * L f64 operations.
 * The taps: `taps` is a kernel argument of its own, const and __restrict__, read at a wave-uniform index only: scalar
 * loads, no vector register or LDS traffic for them. */
#ifndef SAU_K_DECIMATE_H
#define SAU_K_DECIMATE_H

struct DecimParams {
	const float *rows;        /* the float run's rows (16-byte aligned); not read where frames[] is 0 */
	size_t row_pitch;         /* bytes between them, a multiple of 16 */
	const uint32_t *frames;   /* [streams]: the frames of this run that are the stream's; behind them x is +0 */
	float *hist;              /* [streams][(L - 1) * CH]: the L - 1 input frames ahead of this run */
	void *out;                /* OutT[streams][..], out_pitch bytes apart */
	size_t out_pitch;
	uint32_t buf_len;         /* output frames of this run */
	uint32_t swap_bytes;      /* int16 rows: big-endian */
};

template <int K, typename OutT, int CH>
__global__ __launch_bounds__(DECIM_THREADS) void decimate_kernel(const DecimParams P, const double *__restrict__ taps) {
	typedef float __attribute__((ext_vector_type(4))) f32x4;
	typedef float __attribute__((ext_vector_type(2))) f32x2;
	constexpr int L1 = 2 * (int)DECIM_HALF * K;  /* L - 1: the history, and the span's lead, in input frames */
	constexpr int Q = (int)DECIM_SPAN_Q;         /* frames of one phase */
	constexpr int SPAN = Q * K * CH;             /* floats */
	static_assert(SPAN % 4 == 0 && (L1 * CH) % 4 == 0 && ((int)DECIM_TILE * K * CH) % 4 == 0, "16-byte vectors never straddle the history's end");
	__shared__ __attribute__((aligned(16))) float s_x[SPAN];
	const uint32_t stream = blockIdx.y, lane = threadIdx.x;
	const float *row = (const float *)((const char *)P.rows + P.row_pitch * stream);
	const float *hist = P.hist + (size_t)stream * (L1 * CH);
	const long long nfl = (long long)P.frames[stream] * CH;                           /* the stream's floats of this run */
	const long long f0 = ((long long)blockIdx.x * DECIM_TILE * K - L1) * CH;          /* the span's first float, from the row's start */
	for (int v = (int)lane; v < SPAN / 4; v += (int)DECIM_THREADS) {
		const long long f = f0 + 4 * v;
		f32x4 x = {0.f, 0.f, 0.f, 0.f};
		if (f < 0) x = *(const f32x4 *)(hist + (f + L1 * CH));
		else if (f < nfl) { /* (a vector that begins inside the stream's frames ends inside the row: rows are whole vectors) */
			x = *(const f32x4 *)(row + f);
			if (f + 1 >= nfl) x.y = 0.f;
			if (f + 2 >= nfl) x.z = 0.f;
			if (f + 3 >= nfl) x.w = 0.f;
		}
		const float xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
		for (int k = 0; k < 4; ++k) {
			const int sp = 4 * v + k, s = sp / CH, c = sp % CH;
			s_x[((s % K) * Q + s / K) * CH + c] = xs[k];
		}
	}
	__syncthreads();
	double acc[DECIM_PER_LANE][CH];
#pragma unroll
	for (int r = 0; r < (int)DECIM_PER_LANE; ++r)
#pragma unroll
		for (int c = 0; c < CH; ++c) acc[r][c] = 0.0;
	const float *base = s_x + lane * CH;
	/* tap j meets span frame t * K + (L - 1 - j) = (t + qo) * K + p */
	auto tap = [&](const int j, const int p, const int qo) {
		const double h = taps[j];
#pragma unroll
		for (int r = 0; r < (int)DECIM_PER_LANE; ++r) {
			const float *at = base + (p * Q + qo + r * (int)DECIM_THREADS) * CH;
			if constexpr (CH == 2) {
				const f32x2 x = *(const f32x2 *)at;
				acc[r][0] = acc[r][0] + h * (double)x.x;
				acc[r][1] = acc[r][1] + h * (double)x.y;
			} else {
				acc[r][0] = acc[r][0] + h * (double)at[0];
			}
		}
	};
	tap(0, 0, 2 * (int)DECIM_HALF);
#pragma unroll 2
	for (int qo = 2 * (int)DECIM_HALF - 1; qo >= 0; --qo) {
#pragma unroll
		for (int p = K - 1; p >= 0; --p) tap(L1 - (qo * K + p), p, qo);
	}
	OutT *out = (OutT *)((char *)P.out + P.out_pitch * stream);
#pragma unroll
	for (int r = 0; r < (int)DECIM_PER_LANE; ++r) {
		const uint32_t m = blockIdx.x * DECIM_TILE + r * DECIM_THREADS + lane;
		if (m >= P.buf_len) continue;
		if constexpr (std::is_same<OutT, float>::value) {
			if constexpr (CH == 2) { f32x2 y; y.x = (float)acc[r][0]; y.y = (float)acc[r][1]; *(f32x2 *)(out + (size_t)m * 2) = y; }
			else out[m] = (float)acc[r][0];
		} else {
			int16_t q[CH];
#pragma unroll
			for (int c = 0; c < CH; ++c) { const int16_t s16 = pcm16((float)acc[r][c]); q[c] = P.swap_bytes ? pcm_swap(s16) : s16; }
			if constexpr (CH == 2) *(uint32_t *)(out + (size_t)m * 2) = (uint32_t)(uint16_t)q[0] | ((uint32_t)(uint16_t)q[1] << 16);
			else out[m] = q[0];
		}
	}
}

/* The history moves on by this run's n_hi input frames: with E = (old history, the run's input zero-extended), of
 * hist_floats + n_hi * ch floats, the new history is E's last hist_floats. A run shorter than the history shifts it, so every
 * thread reads its (at most four) floats, all wait, and then every thread writes: in place, one buffer. */
__global__ __launch_bounds__(DECIM_CARRY_THREADS) void decimate_carry_kernel(const DecimParams P, const uint32_t hist_floats,
		const uint32_t ch, const unsigned long long n_hi) {
	const uint32_t stream = blockIdx.x, tid = threadIdx.x;
	float *hist = P.hist + (size_t)stream * hist_floats;
	const float *row = (const float *)((const char *)P.rows + P.row_pitch * stream);
	const unsigned long long nfl = (unsigned long long)P.frames[stream] * ch, shift = n_hi * ch;
	float v[4];
#pragma unroll
	for (int r = 0; r < 4; ++r) {
		const uint32_t k = tid + (uint32_t)r * DECIM_CARRY_THREADS;
		v[r] = 0.f;
		if (k < hist_floats) {
			const unsigned long long e = shift + k;
			if (e < hist_floats) v[r] = hist[e];
			else if (e - hist_floats < nfl) v[r] = row[e - hist_floats];
		}
	}
	__syncthreads();
#pragma unroll
	for (int r = 0; r < 4; ++r) {
		const uint32_t k = tid + (uint32_t)r * DECIM_CARRY_THREADS;
		if (k < hist_floats) hist[k] = v[r];
	}
}

#endif
