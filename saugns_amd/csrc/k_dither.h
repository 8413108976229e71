/* k_dither.h -- part of hip_backend.hip: the 16-bit quantiser stage (include/saugns_amd.h, section "Dither and noise shaping";
 * the arithmetic is sau_dither.h's, the geometry launch_plan.h's plan_dither).
 *
 *   dither_flat_kernel   grid (runs of 1024 samples, rows) x 256: a spec without taps, where a sample depends on its position
 *       only -- the TPDF quantiser, and pcm16(x * gain) for a spec with neither dither nor taps. flac_quant_kernel's geometry
 *       and head and tail handling: thread 0 of a row takes the samples ahead of the row's first 16-byte boundary one by one,
 *       every other thread four from a 16-byte load, the row's end again one by one. Each thread hashes its own positions. The
 *       clamped samples are counted in the lanes, summed over the wave, and added to the two chains' records by one atomic
 *       instruction per wave, and only by a wave that clamped something: integers, so the order cannot matter.
 *   dither_shape_kernel  grid (waves) x 64: a spec with taps. A chain is one channel of one row, a wave takes 64 of them, one
 *       per lane -- 64 mono rows, or 32 stereo rows whose chain is 2 * row + (sample & 1) -- and walks tiles of 64 frames. For
 *       a tile all lanes load the rows coalesced (lane = sample in the row), form s (f64) and the dither (f32) off the chain
 *       and put them in LDS frame-major; lane l then walks chain l through the tile with its nine errors in registers and
 *       leaves the samples where the dither was; they go out through coalesced stores. The next tile's loads are issued ahead
 *       of the walk. The build is one of nine taps: coefficients above `taps` are zeros (sau_dither.h: dither_step). History
 *       and counts are the chain's record, read at the start and written at the end; where a row stands comes from the host's
 *       row records. */
struct DitherParams {
	const float *src;           /* the fed rows */
	size_t src_pitch;           /* bytes */
	int16_t *dst;               /* the stage's rows: 256-byte aligned */
	size_t dst_pitch;           /* bytes, a multiple of 256 */
	const DitherRow *rows;      /* [n_rows] */
	saudither::DitherChain *chains; /* [n_rows * channels] */
	uint32_t n_rows, channels;
	uint32_t dither;            /* 0 none, 1 TPDF */
	uint32_t plain;             /* neither dither nor taps: pcm16 */
	double coef[saudither::DITHER_TAPS_MAX]; /* zeros above the spec's taps */
};

__global__ __launch_bounds__(256) void dither_flat_kernel(const DitherParams P) {
	typedef float __attribute__((ext_vector_type(4))) f32x4;
	typedef uint32_t __attribute__((ext_vector_type(2))) u32x2;
	using namespace saudither;
	const unsigned row = blockIdx.y, ch = P.channels;
	const DitherRow d = P.rows[row];
	const unsigned long long n = (unsigned long long)d.frames * ch;
	const float *src = (const float *)((const char *)P.src + P.src_pitch * row);
	int16_t *dst = (int16_t *)((char *)P.dst + P.dst_pitch * row);
	const unsigned head = (unsigned)((16u - (unsigned)((uintptr_t)src & 15u)) & 15u) >> 2; /* samples ahead of the first 16-byte boundary */
	const unsigned long long t = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
	const unsigned long long i0 = t ? head + (t - 1) * 4 : 0;
	const unsigned cnt = t ? 4 : head;
	unsigned clips = 0; /* channel 0's in the low half, channel 1's in the high */
	auto one = [&](float x, unsigned long long k) -> int16_t {
		if (P.plain) return pcm16(x * d.gain);
		const unsigned c = ch == 2 ? (unsigned)(k & 1) : 0;
		const unsigned long long frame = d.first + (ch == 2 ? k >> 1 : k);
		const double s = dither_lsb(dither_scale(x, d.gain));
		const float dd = P.dither ? dither_tpdf(d.seed_r, frame, c) : 0.f;
		bool cl;
		const int32_t q = dither_step(nullptr, 0, nullptr, s, dd, cl);
		clips += cl ? 1u << (16 * c) : 0u;
		return (int16_t)q;
	};
	if (i0 < n) {
		if (cnt == 4 && i0 + 4 <= n) {
			const f32x4 q = __builtin_nontemporal_load((const f32x4 *)(src + i0));
			const int16_t a = one(q.x, i0), b = one(q.y, i0 + 1), c = one(q.z, i0 + 2), e = one(q.w, i0 + 3);
			if (head) { dst[i0] = a; dst[i0 + 1] = b; dst[i0 + 2] = c; dst[i0 + 3] = e; }
			else {
				u32x2 w;
				w.x = (uint32_t)(uint16_t)a | ((uint32_t)(uint16_t)b << 16);
				w.y = (uint32_t)(uint16_t)c | ((uint32_t)(uint16_t)e << 16);
				*(u32x2 *)(dst + i0) = w;
			}
		} else {
			const unsigned long long i1 = i0 + cnt < n ? i0 + cnt : n;
			for (unsigned long long i = i0; i < i1; ++i) dst[i] = one(src[i], i);
		}
	}
	/* (every lane of the wave is here: a whole block lies in one row) */
	if (__ballot(clips != 0)) {
		for (int m = 32; m >= 1; m >>= 1) clips += (unsigned)__shfl_xor((int)clips, m, 64);
		const unsigned lane = threadIdx.x & 63u;
		const unsigned mine = lane < ch ? (clips >> (16 * lane)) & 0xffffu : 0u;
		if (mine) atomicAdd((unsigned long long *)&P.chains[(size_t)row * ch + lane].clipped, (unsigned long long)mine);
	}
}

__global__ __launch_bounds__(64) void dither_shape_kernel(const DitherParams P) {
	using namespace saudither;
	constexpr unsigned TILE = DITHER_TILE, NCH = DITHER_CHAINS;
	__shared__ double s_s[TILE * (NCH + 2)];
	__shared__ uint32_t s_d[TILE * (NCH + 2)]; /* the dither's bits on the way in, the sample on the way out */
	__shared__ DitherRow s_row[NCH];
	const unsigned l = threadIdx.x, ch = P.channels, sh = ch - 1; /* (ch is 1 or 2: x / ch is x >> sh, x % ch is x & sh) */
	const unsigned S = NCH + ch;
	const unsigned rows_per = NCH >> sh;
	const unsigned row0 = blockIdx.x * rows_per;
	const unsigned nr = P.n_rows - row0 < rows_per ? P.n_rows - row0 : rows_per;
	if (l < nr) s_row[l] = P.rows[row0 + l];
	else { DitherRow z; z.first = 0; z.seed_r = 0; z.frames = 0; z.gain = 0.f; s_row[l] = z; }
	__syncthreads();
	uint32_t longest = 0;
	for (unsigned r = 0; r < nr; ++r) longest = s_row[r].frames > longest ? s_row[r].frames : longest;
	/* lane l's chain: row l / ch of the wave's, channel l % ch */
	const unsigned kmax = nr * ch; /* the loads of a tile that have a row: where the rolled loops below stop in a wave of few rows */
	const bool mine = (l >> sh) < nr;
	const uint32_t my_n = s_row[l >> sh].frames;
	DitherChain *rec = P.chains + ((size_t)blockIdx.x * NCH + l);
	double e[DITHER_TAPS_MAX], coef[DITHER_TAPS_MAX];
#pragma unroll
	for (unsigned j = 0; j < DITHER_TAPS_MAX; ++j) { e[j] = mine ? rec->e[j] : 0.0; coef[j] = P.coef[j]; }
	unsigned long long clips = 0;

	/* load k of a tile takes lane l to row k / ch of the wave's and to sample m = (k % ch) * 64 + l of the row's tile: frame
	 * m / ch, channel m % ch */
	float xr[NCH];
	auto load_tile = [&](const unsigned tile) {
#pragma unroll
		for (unsigned k = 0; k < NCH; ++k) {
			const unsigned lr = k >> sh, m = (k & sh) * 64 + l;
			const unsigned long long at = (unsigned long long)tile * (TILE * ch) + m; /* sample of the row's feed */
			const float *src = (const float *)((const char *)P.src + P.src_pitch * (row0 + lr));
			xr[k] = at < (unsigned long long)s_row[lr].frames * ch ? src[at] : 0.f;
		}
	};
	const unsigned tiles = (unsigned)(((unsigned long long)longest + TILE - 1) / TILE); /* (in 64 bits, as plan_dither counts them) */
	if (tiles) load_tile(0);
	for (unsigned tile = 0; tile < tiles; ++tile) {
		const unsigned long long f0 = (unsigned long long)tile * TILE;
		/* the samples are in registers, which only a loop unrolled in full can index: it stays this small. The dither needs no
		 * sample -- a loop of its own, rolled, whose hashes do not crowd the registers. */
#pragma unroll
		for (unsigned k = 0; k < NCH; ++k) {
			const unsigned lr = k >> sh, m = (k & sh) * 64 + l, f = m >> sh, c = m & sh;
			if (f0 + f < s_row[lr].frames) s_s[f * S + lr * ch + c] = dither_lsb(dither_scale(xr[k], s_row[lr].gain));
		}
#pragma unroll 2
		for (unsigned k = 0; k < kmax; ++k) {
			const unsigned lr = k >> sh, m = (k & sh) * 64 + l, f = m >> sh, c = m & sh;
			if (f0 + f < s_row[lr].frames)
				s_d[f * S + lr * ch + c] = __float_as_uint(P.dither ? dither_tpdf(s_row[lr].seed_r, s_row[lr].first + f0 + f, c) : 0.f);
		}
		__syncthreads();
		if (tile + 1 < tiles) load_tile(tile + 1); /* in flight across the walk */
		const unsigned left = longest - (unsigned)f0 < TILE ? longest - (unsigned)f0 : TILE;
		const unsigned cnt = my_n > f0 ? (my_n - f0 < TILE ? (unsigned)(my_n - f0) : TILE) : 0;
		/* eight frames at a time: their reads are issued together and ahead of the samples' stores into the same array, which
		 * would otherwise order every read behind the store before it (frames past the chain's end are read and not used) */
		for (unsigned fb = 0; fb < left; fb += 8) {
			double sv[8];
			float dv[8];
			int32_t qv[8];
#pragma unroll
			for (unsigned j = 0; j < 8; ++j) { sv[j] = s_s[(fb + j) * S + l]; dv[j] = __uint_as_float(s_d[(fb + j) * S + l]); }
#pragma unroll
			for (unsigned j = 0; j < 8; ++j) {
				qv[j] = 0;
				if (fb + j < cnt) {
					bool cl;
					qv[j] = dither_step(coef, DITHER_TAPS_MAX, e, sv[j], dv[j], cl);
					clips += cl ? 1 : 0;
				}
			}
#pragma unroll
			for (unsigned j = 0; j < 8; ++j)
				if (fb + j < cnt) s_d[(fb + j) * S + l] = (uint32_t)qv[j];
		}
		__syncthreads();
#pragma unroll 4
		for (unsigned k = 0; k < kmax; ++k) {
			const unsigned lr = k >> sh, m = (k & sh) * 64 + l, f = m >> sh, c = m & sh;
			if (f0 + f < s_row[lr].frames) {
				int16_t *dst = (int16_t *)((char *)P.dst + P.dst_pitch * (row0 + lr));
				dst[(unsigned long long)tile * (TILE * ch) + m] = (int16_t)(int32_t)s_d[f * S + lr * ch + c];
			}
		}
		__syncthreads(); /* (the next tile's staging writes where these reads were) */
	}
	if (mine && my_n) {
#pragma unroll
		for (unsigned j = 0; j < DITHER_TAPS_MAX; ++j) rec->e[j] = e[j];
		rec->clipped += clips;
	}
}
