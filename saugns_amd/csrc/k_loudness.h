/* k_loudness.h -- BS.1770 loudness and true peak of float rows: part of hip_backend.hip (inside namespace sauhip).
 *   loud_chunk_kernel<CH, 0>  grid (chunk groups, rows) x LOUD_THREADS (one wave). A lane owns one chunk of LOUD_CHUNK frames
 *       of one row, both channels of a stereo row, and runs the K-weighting recurrence over it from ZERO state -> z_c.
 *   loud_scan_kernel          one lane per (row, channel) goes over the row's chunks in order: S_c -> S_{c+1} = M S_c + z_c
 *       (M: the state's 4x4 map over a chunk of zero input), and leaves every S_c for the pass that follows.
 *   loud_chunk_kernel<CH, 1>  the same chunks again, each from its S_c: the sum of y * y per hop the chunk touches (two at
 *       most: a hop is at least a chunk long), and the last chunk's end state becomes the row's carried state.
 *   truepeak_kernel<CH>       grid (tiles, rows) x TP_THREADS (one wave), laid out like decimate_kernel: a lane owns TP_PER_LANE
 *       frames of the tile and runs three f64 chains per frame and channel -- the phases 1, 2, 3 of a 4x interpolator --
 *       over the tile's span in LDS; the maximum over bit patterns is folded over the wave into ONE record per workgroup.
 *   loud_finish_kernel        one lane per row: the chunks' partial sums into the row's hop energies in chunk order, the
 *       tiles' maxima into the row's peaks, and the row's frame count moves on.
 *   loud_carry_kernel         one workgroup per row: the true-peak history becomes the last TP_LEAD frames of (old history,
 *       this run's frames).
 * No atomics, and no floating-point sum whose order depends on scheduling: include/saugns_amd.h states every operation's
 * order, and the same rows in the same run lengths give the same bits on any partition of the device.
 * The build is -ffp-contract=off: a product is rounded before it is added.
 *
 * What a sample is: the row's float as a double; a NaN or +-inf counts as +0.0 (loud_clean, applied where a sample is staged).
 *
 * LDS, loud_chunk_kernel. A lane's frames lie LOUD_CHUNK * CH floats from its neighbour's: read from HBM as they lie that is
 * sixty-four cache lines per load. So the wave stages LOUD_SUB frames of each of its chunks at a time with 16-byte loads --
 * eight (mono) or sixteen (stereo) consecutive lanes on one chunk's 128 or 256 contiguous bytes -- into s_x[chunk][..] with
 * a row stride of LOUD_SUB * CH + CH floats: 33 (mono: lane l reads ds_read_b32 at 33 l + j, thirty-two lanes on thirty-two
 * banks) or 66 (stereo: one ds_read_b64 per frame at 66 l + 2 j, thirty-two lanes on sixty-four banks). Conflict-free both
 * ways (LDS banking is per instruction, in groups of 32 lanes); the staging stores are ds_write_b32, at most 2-way.
 * truepeak_kernel: the span is staged with the channels apart, s_x[channel][frame], and a lane works through one channel at a
 * time: consecutive lanes read consecutive dwords at a wave-uniform tap (ds_read_b32, thirty-two lanes on thirty-two banks);
 * the staging stores are ds_write_b32, at most 2-way. The taps are a const __restrict__ kernel argument read at wave-uniform
 * indices: scalar loads. */
#ifndef SAU_K_LOUDNESS_H
#define SAU_K_LOUDNESS_H

/* K-weighting: stage 1 (high shelf) b0 b1 b2 a1 a2, stage 2 (high-pass) c0 c1 c2 d1 d2 -- sauAmd_loudness_filter's ten */
struct LoudFilter { double b0, b1, b2, a1, a2, c0, c1, c2, d1, d2; };
struct LoudMap { double m[4][4]; };
struct LoudState { double s1, s2, t1, t2; };
static_assert(sizeof(LoudState) == 32, "four doubles per (row, channel, chunk)");

struct LoudParams {
	const float *rows;          /* 16-byte aligned */
	size_t row_pitch;           /* bytes between rows, a multiple of 16 */
	const uint32_t *frames;     /* [n_rows]: the frames of this measurement that are the row's */
	uint32_t channels, n_rows, hop;
	uint32_t chunk_cap, tile_cap; /* chunks and tiles of the longest row: the strides of the arrays below */
	LoudState *state;           /* [n_rows][2]: carried from the row's previous measurement */
	unsigned long long *pos;    /* [n_rows]: frames metered so far */
	LoudState *zstate, *sstate; /* [n_rows * 2][chunk_cap] */
	double *parts;              /* [n_rows * 2][chunk_cap][2]: the sums of the earlier and of the later hop of a chunk */
	double *E;                  /* [e_cap][n_rows][2]: hop energies */
	uint32_t e_cap;
	uint32_t *tp_parts;         /* [n_rows][tile_cap][2]: bits of a float */
	uint32_t *peak;             /* [n_rows][2] */
	float *hist;                /* [n_rows][TP_LEAD * 2]: the row's last TP_LEAD frames, cleaned, interleaved like the row */
};

__device__ __forceinline__ float loud_clean(const float x) {
	return (__float_as_uint(x) & 0x7fffffffu) < 0x7f800000u ? x : 0.f;
}
/* one frame (include/saugns_amd.h): every product rounded, then every sum, in this order */
__device__ __forceinline__ double loud_step(LoudState &S, const LoudFilter &F, const double x) {
	const double u = F.b0 * x + S.s1;
	S.s1 = (F.b1 * x - F.a1 * u) + S.s2;
	S.s2 = F.b2 * x - F.a2 * u;
	const double y = F.c0 * u + S.t1;
	S.t1 = (F.c1 * u - F.d1 * y) + S.t2;
	S.t2 = F.c2 * u - F.d2 * y;
	return y;
}

template <int CH, int PASS>
__global__ __launch_bounds__(LOUD_THREADS) void loud_chunk_kernel(const LoudParams P, const LoudFilter F) {
	typedef float __attribute__((ext_vector_type(4))) f32x4;
	typedef float __attribute__((ext_vector_type(2))) f32x2;
	constexpr int STRIDE = (int)LOUD_SUB * CH + CH; /* floats of one chunk's sub-tile in LDS, padded by one access width */
	constexpr int VPC = (int)LOUD_SUB * CH / 4;     /* 16-byte vectors of it */
	__shared__ __attribute__((aligned(16))) float s_x[LOUD_WG_CHUNKS * STRIDE];
	const uint32_t row = blockIdx.y, lane = threadIdx.x;
	const unsigned long long n = P.frames[row];
	const unsigned long long c0 = (unsigned long long)blockIdx.x * LOUD_WG_CHUNKS;
	if (c0 * LOUD_CHUNK >= n) return; /* (the whole workgroup lies behind the row's end) */
	const unsigned long long c = c0 + lane, first = c * LOUD_CHUNK;
	const int cnt = first >= n ? 0 : n - first < LOUD_CHUNK ? (int)(n - first) : (int)LOUD_CHUNK; /* this lane's frames */
	const float *rowp = (const float *)((const char *)P.rows + P.row_pitch * row);
	const unsigned long long nfl = n * CH; /* the row's floats */
	const size_t at = ((size_t)row * 2) * P.chunk_cap + (size_t)c; /* channel 0's; channel 1's is chunk_cap further on */
	LoudState S[CH];
	double acc[CH][2];
	int fb = (int)LOUD_CHUNK; /* frames [fb, cnt) of the chunk belong to the later hop */
#pragma unroll
	for (int ch = 0; ch < CH; ++ch) {
		S[ch].s1 = S[ch].s2 = S[ch].t1 = S[ch].t2 = 0.0;
		acc[ch][0] = acc[ch][1] = 0.0;
		if (PASS == 1 && cnt) S[ch] = P.sstate[at + (size_t)ch * P.chunk_cap];
	}
	if (PASS == 1) {
		const unsigned long long left = P.hop - (P.pos[row] + first) % P.hop; /* frames left in the hop the chunk begins in: >= 1 */
		fb = left < LOUD_CHUNK ? (int)left : (int)LOUD_CHUNK;
	}
	for (int t = 0; t < (int)(LOUD_CHUNK / LOUD_SUB); ++t) {
		for (int v = (int)lane; v < (int)LOUD_WG_CHUNKS * VPC; v += (int)LOUD_THREADS) {
			const int k = v / VPC, part = v % VPC;
			const unsigned long long f = ((c0 + k) * LOUD_CHUNK + (unsigned)t * LOUD_SUB) * CH + 4u * (unsigned)part;
			float xs[4] = {0.f, 0.f, 0.f, 0.f};
			if (f + 4 <= nfl) { const f32x4 x = *(const f32x4 *)(rowp + f); xs[0] = x.x; xs[1] = x.y; xs[2] = x.z; xs[3] = x.w; }
			else {
#pragma unroll
				for (int e = 0; e < 4; ++e) if (f + e < nfl) xs[e] = rowp[f + e];
			}
			float *dst = s_x + k * STRIDE + 4 * part;
#pragma unroll
			for (int e = 0; e < 4; ++e) dst[e] = loud_clean(xs[e]);
		}
		__syncthreads();
		const float *mine = s_x + lane * STRIDE;
		const int base = t * (int)LOUD_SUB;
		if (base < cnt) {
			const int m = cnt - base < (int)LOUD_SUB ? cnt - base : (int)LOUD_SUB;
			for (int j = 0; j < m; ++j) {
				float x[CH];
				if constexpr (CH == 2) { const f32x2 q = *(const f32x2 *)(mine + 2 * j); x[0] = q.x; x[1] = q.y; }
				else x[0] = mine[j];
#pragma unroll
				for (int ch = 0; ch < CH; ++ch) {
					const double y = loud_step(S[ch], F, (double)x[ch]);
					if (PASS == 1) {
						const double yy = y * y;
						if (base + j < fb) acc[ch][0] = acc[ch][0] + yy;
						else acc[ch][1] = acc[ch][1] + yy;
					}
				}
			}
		}
		__syncthreads();
	}
	if (!cnt) return;
#pragma unroll
	for (int ch = 0; ch < CH; ++ch) {
		const size_t i = at + (size_t)ch * P.chunk_cap;
		if (PASS == 0) P.zstate[i] = S[ch];
		else {
			P.parts[2 * i] = acc[ch][0];
			P.parts[2 * i + 1] = acc[ch][1];
			if (first + (unsigned)cnt == n) P.state[(size_t)row * 2 + ch] = S[ch]; /* the row's last chunk, full or partial */
		}
	}
}

/* S_{c+1}[r] = ((((0.0 + M[r][0] S_c[0]) + M[r][1] S_c[1]) + M[r][2] S_c[2]) + M[r][3] S_c[3]) + z_c[r] behind every FULL chunk;
 * the next chunk's z is loaded ahead of the sixteen products, which keep their order */
__global__ __launch_bounds__(64) void loud_scan_kernel(const LoudParams P, const LoudMap M) {
	const uint32_t i = blockIdx.x * 64 + threadIdx.x, row = i >> 1, ch = i & 1u;
	if (row >= P.n_rows || ch >= P.channels) return;
	const unsigned long long n = P.frames[row];
	const uint32_t nch = (uint32_t)((n + LOUD_CHUNK - 1) / LOUD_CHUNK);
	if (!nch) return;
	const LoudState *z = P.zstate + (size_t)i * P.chunk_cap;
	LoudState *s = P.sstate + (size_t)i * P.chunk_cap;
	LoudState S = P.state[i], zn = z[0];
	for (uint32_t c = 0;; ++c) {
		s[c] = S;
		if (c + 1 == nch) break;
		const LoudState zc = zn;
		zn = z[c + 1];
		const double v[4] = {S.s1, S.s2, S.t1, S.t2};
		double w[4];
#pragma unroll
		for (int r = 0; r < 4; ++r) w[r] = (((0.0 + M.m[r][0] * v[0]) + M.m[r][1] * v[1]) + M.m[r][2] * v[2]) + M.m[r][3] * v[3];
		S.s1 = w[0] + zc.s1; S.s2 = w[1] + zc.s2; S.t1 = w[2] + zc.t1; S.t2 = w[3] + zc.t2;
	}
}

template <int CH>
__global__ __launch_bounds__(TP_THREADS) void truepeak_kernel(const LoudParams P, const double *__restrict__ taps) {
	typedef float __attribute__((ext_vector_type(4))) f32x4;
	constexpr int SPAN_FR = (int)(TP_TILE + TP_LEAD); /* frames: the tile and TP_LEAD frames ahead of it */
	constexpr int SPAN = SPAN_FR * CH;
	static_assert(SPAN % 4 == 0 && ((int)TP_LEAD * CH) % 4 == 0 && ((int)TP_TILE * CH) % 4 == 0, "16-byte vectors never straddle the history's end");
	__shared__ __attribute__((aligned(16))) float s_x[SPAN]; /* [channel][frame]: the channels apart, so that a lane's frames are consecutive dwords */
	const uint32_t row = blockIdx.y, lane = threadIdx.x;
	const unsigned long long n = P.frames[row];
	const unsigned long long t0 = (unsigned long long)blockIdx.x * TP_TILE;
	if (t0 >= n) return; /* (behind the row's end: loud_finish_kernel does not read this tile's record) */
	const float *rowp = (const float *)((const char *)P.rows + P.row_pitch * row);
	const float *hist = P.hist + (size_t)row * (TP_LEAD * 2);
	const long long nfl = (long long)n * CH, f0 = ((long long)t0 - (long long)TP_LEAD) * CH;
	for (int v = (int)lane; v < SPAN / 4; v += (int)TP_THREADS) {
		const long long f = f0 + 4 * v;
		float xs[4] = {0.f, 0.f, 0.f, 0.f};
		if (f < 0) { const f32x4 x = *(const f32x4 *)(hist + (f + (long long)TP_LEAD * CH)); xs[0] = x.x; xs[1] = x.y; xs[2] = x.z; xs[3] = x.w; }
		else if (f + 4 <= nfl) { const f32x4 x = *(const f32x4 *)(rowp + f); xs[0] = x.x; xs[1] = x.y; xs[2] = x.z; xs[3] = x.w; }
		else {
#pragma unroll
			for (int e = 0; e < 4; ++e) if (f + e < nfl) xs[e] = rowp[f + e];
		}
#pragma unroll
		for (int e = 0; e < 4; ++e) {
			const int sp = 4 * v + e;
			s_x[(sp % CH) * SPAN_FR + sp / CH] = loud_clean(xs[e]);
		}
	}
	__syncthreads();
	uint32_t pk[2] = {0u, 0u};
	for (int ch = 0; ch < CH; ++ch) { /* one channel at a time: twelve f64 chains per lane */
		double acc[TP_PER_LANE][3];
#pragma unroll
		for (int r = 0; r < (int)TP_PER_LANE; ++r) acc[r][0] = acc[r][1] = acc[r][2] = 0.0;
		/* tap q of every phase meets frame m - q: span frame (m - t0) + TP_LEAD - q */
		const float *base = s_x + ch * SPAN_FR + lane + TP_LEAD;
#pragma unroll 2
		for (int q = 0; q < 2 * (int)TP_HALF; ++q) {
			const double g1 = taps[4 * q + 1], g2 = taps[4 * q + 2], g3 = taps[4 * q + 3];
#pragma unroll
			for (int r = 0; r < (int)TP_PER_LANE; ++r) {
				const double d = (double)base[r * (int)TP_THREADS - q];
				acc[r][0] = acc[r][0] + g1 * d;
				acc[r][1] = acc[r][1] + g2 * d;
				acc[r][2] = acc[r][2] + g3 * d;
			}
		}
		uint32_t best = 0u;
#pragma unroll
		for (int r = 0; r < (int)TP_PER_LANE; ++r) {
			if (t0 + (unsigned)r * TP_THREADS + lane >= n) continue;
			const uint32_t ax = __float_as_uint(base[r * (int)TP_THREADS]) & 0x7fffffffu; /* (cleaned: finite) */
			best = ax > best ? ax : best;
#pragma unroll
			for (int p = 0; p < 3; ++p) {
				const uint32_t aw = __float_as_uint((float)acc[r][p]) & 0x7fffffffu;
				best = aw < 0x7f800000u && aw > best ? aw : best;
			}
		}
#pragma unroll
		for (int off = 32; off >= 1; off >>= 1) {
			const uint32_t o = (uint32_t)__shfl_xor((int)best, off);
			best = o > best ? o : best;
		}
		pk[ch] = best;
	}
	if (lane == 0) {
		uint32_t *out = P.tp_parts + ((size_t)row * P.tile_cap + blockIdx.x) * 2;
		out[0] = pk[0]; out[1] = pk[1];
	}
}

/* One lane per row: a chunk's sums go into the hop the chunk begins in and, where it reaches the next one, into that -- in
 * chunk order, the earlier hop first; a hop's running sum stays in a register while consecutive chunks add to it. */
__global__ __launch_bounds__(64) void loud_finish_kernel(const LoudParams P) {
	const uint32_t row = blockIdx.x * 64 + threadIdx.x;
	if (row >= P.n_rows) return;
	const unsigned long long n = P.frames[row];
	if (!n) return; /* a row without frames changes nothing */
	const unsigned long long pos0 = P.pos[row];
	const uint32_t nch = (uint32_t)((n + LOUD_CHUNK - 1) / LOUD_CHUNK), nt = (uint32_t)((n + TP_TILE - 1) / TP_TILE);
	const size_t e_stride = (size_t)P.n_rows * 2;
	for (uint32_t ch = 0; ch < P.channels; ++ch) {
		const double *parts = P.parts + ((size_t)row * 2 + ch) * P.chunk_cap * 2;
		double *E = P.E + (size_t)(pos0 / P.hop) * e_stride + (size_t)row * 2 + ch;
		unsigned long long rem = P.hop - pos0 % P.hop; /* frames left in the hop at hand */
		double e = *E;
		for (uint32_t c = 0; c < nch; ++c) {
			const unsigned long long left = n - (unsigned long long)c * LOUD_CHUNK, cnt = left < LOUD_CHUNK ? left : LOUD_CHUNK;
			e = e + parts[2 * c];
			if (cnt >= rem) { /* the hop is complete (host: e_cap covers the hop that pos0 + n lies in) */
				*E = e;
				E += e_stride;
				e = *E;
				if (cnt > rem) e = e + parts[2 * c + 1];
				rem += P.hop;
			}
			rem -= cnt;
		}
		*E = e;
		uint32_t pk = P.peak[(size_t)row * 2 + ch];
		const uint32_t *tp = P.tp_parts + (size_t)row * P.tile_cap * 2 + ch;
		for (uint32_t t = 0; t < nt; ++t) pk = tp[2 * t] > pk ? tp[2 * t] : pk;
		P.peak[(size_t)row * 2 + ch] = pk;
	}
	P.pos[row] = pos0 + n;
}

/* The history moves on by the row's own n frames: with X = (old history, the row's n frames), the new history is X's last
 * TP_LEAD frames. A row shorter than the history shifts it, so every thread reads its float, all wait, then every thread
 * writes: in place. Behind truepeak_kernel on the one stream. */
__global__ __launch_bounds__(64) void loud_carry_kernel(const LoudParams P) {
	const uint32_t row = blockIdx.x, k = threadIdx.x, hf = TP_LEAD * P.channels;
	float *hist = P.hist + (size_t)row * (TP_LEAD * 2);
	const float *rowp = (const float *)((const char *)P.rows + P.row_pitch * row);
	const unsigned long long e = (unsigned long long)P.frames[row] * P.channels + k;
	float v = 0.f;
	if (k < hf) v = e < hf ? hist[e] : loud_clean(rowp[e - hf]);
	__syncthreads();
	if (k < hf) hist[k] = v;
}
static_assert(TP_LEAD * 2 <= 64, "loud_carry_kernel: a row's history, one float per thread");

#endif
