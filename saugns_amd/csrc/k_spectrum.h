/* k_spectrum.h -- Welch power spectra of float rows in f64: part of hip_backend.hip (inside namespace sauhip).
 *   spec_segment_kernel<L>  grid (groups, rows, channels) x SPEC_THREADS, 16 N bytes of dynamic LDS. A workgroup owns one group
 *       of up to sixteen segments of one row and channel and works through them in ascending order: window, N = 2^L point
 *       radix-2 FFT in place, |X[k]|^2 for k = 0 .. N / 2 added to the group's sum, which its lanes hold in registers (bin k with
 *       lane k % SPEC_THREADS). The group a feed continues starts from the carried accumulator, every other from +0.0. The sums
 *       go to the feed's scratch, one record per group; a segment's (float)p[k] to the spectrogram when one is asked for.
 *   spec_finish_kernel      grid (bin tiles, rows, channels): total[k] takes the groups that are complete behind the feed in
 *       ascending order; the last group, when it is not, becomes the carried accumulator.
 *   spec_carry_kernel       grid (parts, rows): the row's pending frames become those behind the feed -- taken from (old pending
 *       frames, the fed row, cleaned) -- from one buffer into the other (the meter swaps them): nothing is overwritten that is
 *       still to be read, and a row fed nothing is copied as it stands.
 *
 * The arithmetic (include/saugns_amd.h, section "Spectrum") is a function of the fed sequence only. The butterflies of a stage
 * are independent and each is computed once, by one lane, with exactly the stated operations -- every product rounded, then the
 * sum or difference (the build is -ffp-contract=off), the twiddles (1, -0) included: nothing is special-cased. Three consecutive
 * stages are fused in registers: a lane takes the eight values 2^T apart that stages T+1 .. T+3 combine among themselves, so a
 * transform of L stages is ceil(L / 3) passes over LDS (the last pass takes the one or two stages left). The sums have a fixed
 * order: segments ascending within a group, groups ascending into the total. No atomics.
 *
 * LDS. re and im are N doubles each, 64 KiB at L = 12; nothing else is staged (the first pass reads the samples from global
 * memory at bit-reversed indices, straight into registers: a segment is at most 32 KiB and lies in L2; window and twiddles
 * likewise). In the first pass a lane writes eight consecutive doubles and its neighbour the next eight; in the later passes
 * lanes read and write 2^T apart. Stored as they lie, the first pass's ds_write_b64 would put sixteen lanes on two bank pairs
 * and the second pass's ds_read_b64 thirty-two lanes on eight. So position p is kept at
 *   spec_sw(p) = p ^ ((p >> 3) & 7) ^ (((p >> 6) & 3) << 3)
 * (bits 3..5 folded onto bits 0..2, bits 6..7 onto bits 3..4: a permutation, and one within every aligned block of 256
 * positions). With it the sixteen lanes of a ds_write_b64 group fall on sixteen different doubles modulo 16 and the thirty-two
 * of a ds_read_b64 group on thirty-two different ones modulo 32 in every pass: pass 1 writes (lane q, element i) at low bits
 * (i ^ q[0:3], q[0:2] ^ q[3:5]); pass 2 (T = 3) lane (j, b) element i at (j ^ i, i[0:2] ^ b[0:2]); passes 3 and 4 lanes j at
 * (j[0:3] ^ j[3:6], j[3:5] ^ const). A lane reads and writes only its own eight positions in a pass, so one barrier between
 * passes suffices. */
#ifndef SAU_K_SPECTRUM_H
#define SAU_K_SPECTRUM_H

struct SpecParams {
	const float *rows;        /* the float rows; not read where a row's feed has no frames */
	size_t row_pitch;         /* bytes between them */
	const SpecRow *desc;      /* [rows] (launch_plan.h) */
	const float *pend;        /* [rows][pend_pitch], cleaned and interleaved like the row: the frames from seg0 * hop on */
	float *pend_next;         /* spec_carry_kernel's target */
	size_t pend_pitch;        /* floats */
	double *acc;              /* [rows][channels][bins]: the group at hand */
	double *total;            /* [rows][channels][bins]: the complete groups */
	double *part;             /* [rows][channels][max_groups][bins]: this feed's groups */
	float *sgram;             /* [rows][channels][sgram_segs][bins], or NULL; segment s of the row at index s (rows from empty records) */
	size_t sgram_segs;
	const double *win;        /* [N] */
	const double2 *tw;        /* [N / 2]: (cos, -sin) */
	uint32_t hop, channels, max_groups;
};

__device__ __forceinline__ unsigned spec_sw(const unsigned p) { return p ^ ((p >> 3) & 7u) ^ (((p >> 6) & 3u) << 3); }

/* the cleaned sample of frame `rel`, counted from the row's frame seg0 * hop: a pending frame, or one of the fed row */
__device__ __forceinline__ float spec_x(const float *row, const float *pend, const unsigned n_pend, const unsigned long long rel, const unsigned ch,
		const unsigned c) {
	if (rel < n_pend) return pend[rel * ch + c];
	return loud_clean(row[(rel - n_pend) * ch + c]);
}

/* stages T+1 .. T+R of an N = 2^L point transform on the 2^R values that lie 2^T apart from position base = (..) + jl, jl the
 * position's low T bits: for stage t = T + s the pairs are (i, i + 2^(s-1)) for i with that bit clear, and the twiddle is
 * T[j * N / 2^t] with j = a mod 2^(t-1) = jl + (i mod 2^(s-1)) * 2^T */
template <int L, int T, int R>
__device__ __forceinline__ void spec_stages(double (&xr)[1 << R], double (&xi)[1 << R], const double2 *__restrict__ tw, const unsigned jl) {
#pragma unroll
	for (int s = 1; s <= R; ++s) {
#pragma unroll
		for (int i = 0; i < (1 << R); ++i) {
			if (i & (1 << (s - 1))) continue;
			const int i2 = i + (1 << (s - 1));
			const unsigned j = jl + ((unsigned)(i & ((1 << (s - 1)) - 1)) << T);
			const double2 cd = tw[j << (L - T - s)];
			const double tr = cd.x * xr[i2] - cd.y * xi[i2], ti = cd.x * xi[i2] + cd.y * xr[i2];
			const double ur = xr[i], ui = xi[i];
			xr[i] = ur + tr; xi[i] = ui + ti; xr[i2] = ur - tr; xi[i2] = ui - ti;
		}
	}
}

/* one pass over LDS: N / 2^R lanes' worth of work, each on its own 2^R positions */
template <int L, int T, int R>
__device__ __forceinline__ void spec_pass(double *s_re, double *s_im, const double2 *__restrict__ tw, const unsigned tid) {
	constexpr unsigned N = 1u << L, E = 1u << R;
	for (unsigned u = tid; u < (N >> R); u += SPEC_THREADS) {
		const unsigned jl = u & ((1u << T) - 1), base = ((u >> T) << (T + R)) + jl;
		double xr[E], xi[E];
#pragma unroll
		for (unsigned i = 0; i < E; ++i) {
			const unsigned at = spec_sw(base + (i << T));
			xr[i] = s_re[at]; xi[i] = s_im[at];
		}
		spec_stages<L, T, R>(xr, xi, tw, jl);
#pragma unroll
		for (unsigned i = 0; i < E; ++i) {
			const unsigned at = spec_sw(base + (i << T));
			s_re[at] = xr[i]; s_im[at] = xi[i];
		}
	}
}

template <int L>
__global__ __launch_bounds__(SPEC_THREADS) void spec_segment_kernel(const SpecParams P) {
	constexpr unsigned N = 1u << L, BINS = N / 2 + 1, PER = (BINS + SPEC_THREADS - 1) / SPEC_THREADS;
	extern __shared__ double spec_lds[];
	double *s_re = spec_lds, *s_im = spec_lds + N;
	const unsigned tid = threadIdx.x, gi = blockIdx.x, row = blockIdx.y, c = blockIdx.z, ch = P.channels;
	const SpecRow d = P.desc[row];
	if (gi >= d.n_groups) return; /* (uniform: the whole workgroup leaves) */
	const unsigned long long g = d.seg0 / SPEC_GROUP + gi, seg_end = d.seg0 + d.n_seg;
	const unsigned long long s_lo = g * SPEC_GROUP > d.seg0 ? g * SPEC_GROUP : d.seg0;
	const unsigned long long s_hi = (g + 1) * SPEC_GROUP < seg_end ? (g + 1) * SPEC_GROUP : seg_end;
	const size_t rc = (size_t)row * ch + c;
	const float *xrow = (const float *)((const char *)P.rows + P.row_pitch * row);
	const float *pend = P.pend + P.pend_pitch * row;
	double a[PER];
#pragma unroll
	for (unsigned i = 0; i < PER; ++i) {
		const unsigned k = tid + i * SPEC_THREADS;
		a[i] = gi == 0 && d.acc_cnt && k < BINS ? P.acc[rc * BINS + k] : 0.0;
	}
	for (unsigned long long s = s_lo; s < s_hi; ++s) {
		const unsigned long long first = (s - d.seg0) * P.hop; /* the segment's first frame, counted from seg0 * hop */
		/* pass 1: stages 1 .. 3 on the bit-reversed loads; lane u makes positions 8 u .. 8 u + 7 */
		for (unsigned u = tid; u < N / 8; u += SPEC_THREADS) {
			double xr[8], xi[8];
#pragma unroll
			for (unsigned i = 0; i < 8; ++i) {
				const unsigned j = __brev(8 * u + i) >> (32 - L);
				xr[i] = P.win[j] * (double)spec_x(xrow, pend, d.pend, first + j, ch, c);
				xi[i] = 0.0;
			}
			spec_stages<L, 0, 3>(xr, xi, P.tw, 0);
#pragma unroll
			for (unsigned i = 0; i < 8; ++i) {
				const unsigned at = spec_sw(8 * u + i);
				s_re[at] = xr[i]; s_im[at] = xi[i];
			}
		}
		__syncthreads();
		spec_pass<L, 3, 3>(s_re, s_im, P.tw, tid);
		__syncthreads();
		spec_pass<L, 6, (L - 6 < 3 ? L - 6 : 3)>(s_re, s_im, P.tw, tid);
		__syncthreads();
		if constexpr (L > 9) {
			spec_pass<L, 9, L - 9>(s_re, s_im, P.tw, tid);
			__syncthreads();
		}
		float *sg = P.sgram ? P.sgram + (rc * P.sgram_segs + (size_t)s) * BINS : nullptr;
#pragma unroll
		for (unsigned i = 0; i < PER; ++i) {
			const unsigned k = tid + i * SPEC_THREADS;
			if (k < BINS) {
				const unsigned at = spec_sw(k);
				const double re = s_re[at], im = s_im[at];
				const double p = re * re + im * im;
				a[i] = a[i] + p;
				if (sg) sg[k] = (float)p;
			}
		}
		__syncthreads(); /* (the next segment's first pass overwrites what was just read) */
	}
	double *out = P.part + (rc * P.max_groups + gi) * BINS;
#pragma unroll
	for (unsigned i = 0; i < PER; ++i) {
		const unsigned k = tid + i * SPEC_THREADS;
		if (k < BINS) out[k] = a[i];
	}
}

__global__ __launch_bounds__(SPEC_THREADS) void spec_finish_kernel(const SpecParams P, const unsigned bins) {
	const unsigned k = blockIdx.x * SPEC_THREADS + threadIdx.x, row = blockIdx.y, c = blockIdx.z;
	const SpecRow d = P.desc[row];
	if (k >= bins || !d.n_groups) return;
	const size_t rc = (size_t)row * P.channels + c;
	const double *part = P.part + rc * P.max_groups * bins + k;
	if (d.n_complete) {
		double t = P.total[rc * bins + k];
		for (unsigned gi = 0; gi < d.n_complete; ++gi) t = t + part[(size_t)gi * bins];
		P.total[rc * bins + k] = t;
	}
	if (d.n_complete < d.n_groups) P.acc[rc * bins + k] = part[(size_t)(d.n_groups - 1) * bins];
}

__global__ __launch_bounds__(SPEC_THREADS) void spec_carry_kernel(const SpecParams P) {
	const unsigned e = blockIdx.x * SPEC_THREADS + threadIdx.x, row = blockIdx.y, ch = P.channels;
	const SpecRow d = P.desc[row];
	if (e >= d.pend_next * ch) return;
	const float *xrow = (const float *)((const char *)P.rows + P.row_pitch * row);
	const unsigned long long rel = (unsigned long long)d.n_seg * P.hop + e / ch; /* counted from seg0 * hop */
	P.pend_next[P.pend_pitch * row + e] = spec_x(xrow, P.pend + P.pend_pitch * row, d.pend, rel, ch, e % ch);
}

#endif
