/* k_levels.h -- level metering and the normalised writer's requantiser: part of hip_backend.hip (inside namespace sauhip).
 *   levels_kernel<SampleT>  grid (blocks, rows) x 256 threads. A workgroup owns LEVELS_WG_SAMPLES consecutive samples of one row
 *       (launch_plan.h: plan_levels -- a constant, not a function of the device), reads them once with 16-byte streaming loads,
 *       keeps per-lane accumulators per channel, folds them across the wave with __shfl_xor, across the four waves through
 *       LDS in wave order, and writes ONE partial record with ordinary stores.
 *   levels_finish_kernel    one thread per row folds the row's partials in ascending block order and adds the result to the
 *       row's running record (or starts it: foreign rows).
 *   requant_kernel<OutT>    pcm16(x * gain), or x * gain as a float, of one float row into a buffer of its own.
 * No atomics, and no floating-point sum whose order depends on scheduling: which samples a lane takes, the butterfly of the
 * wave, the order of the waves and of the blocks are all fixed by the indices, so the same rows give the same bits on any
 * partition of the device.
 *
 * What a sample counts as (include/saugns_amd.h: sauAmdLevels). Float rows: x as it stands; peak over |x| of the finite
 * samples, compared as bit patterns (a non-negative float orders like its bits, and no denormal mode comes into it);
 * x * x as (double)x * (double)x, exact, summed in f64; `over` |x| > 1 or not finite; `full` pcm16(x) == +-32767 (a NaN is
 * -32767 there: sau_dev_math.h); `nonf` NaN or +-inf. int16 rows: integers throughout -- max |s|, sum of s * s in 64 bits,
 * `full` |s| >= 32767, `over` s == -32768 -- and the host divides once. */
#ifndef SAU_K_LEVELS_H
#define SAU_K_LEVELS_H

/* one workgroup's (and, in levels_finish_kernel, one row's) measurement. sum: the bits of a double (float rows) or a uint64
 * (int16 rows); peak: the bits of a float, or max |s| */
struct LevelsPart {
	unsigned long long sum[2];
	uint32_t peak[2], over[2], full[2], nonf[2];
};
/* a row's running record: int16 and float runs may alternate on a batch, so both domains are kept and the host joins them */
struct LevelsAcc {
	unsigned long long frames;
	unsigned long long isum[2];
	double fsum[2];
	unsigned long long over[2], full[2], nonf[2];
	uint32_t ipeak[2];
	float fpeak[2];
};
static_assert(sizeof(LevelsPart) == 48 && sizeof(LevelsAcc) == 104, "records of k_levels.h");

struct LevelsParams {
	const void *rows;            /* 16-byte aligned */
	size_t pitch;                /* bytes between rows, a multiple of 16 */
	const uint32_t *row_frames;  /* frames of each row, or NULL: `frames` for all */
	unsigned long long frames;
	uint32_t channels, blocks;   /* parts[row * blocks + block] */
	LevelsPart *parts;
	LevelsAcc *acc;              /* levels_finish_kernel: [rows] */
	uint32_t n_rows, f32, accumulate;
};

template <typename SampleT> struct LevelsLane;
template <> struct LevelsLane<float> {
	typedef float __attribute__((ext_vector_type(4))) Vec;
	static constexpr uint32_t PER = 4;
	uint32_t pk[2] = {0, 0}, ov[2] = {0, 0}, fs[2] = {0, 0}, nf[2] = {0, 0};
	double sm[2] = {0.0, 0.0};
	__device__ __forceinline__ void take(const float x, const int c) {
		const uint32_t ab = __float_as_uint(x) & 0x7fffffffu;
		const bool fin = ab < 0x7f800000u;
		const double d = fin ? (double)x : 0.0;
		sm[c] += d * d; /* (a product of two 24-bit significands: exact) */
		pk[c] = fin && ab > pk[c] ? ab : pk[c];
		nf[c] += fin ? 0u : 1u;
		ov[c] += ab > 0x3f800000u ? 1u : 0u; /* |x| > 1, +-inf, NaN */
		const int q = pcm16(x);
		fs[c] += q == 32767 || q == -32767 ? 1u : 0u;
	}
	__device__ __forceinline__ void take(const Vec v) { take(v.x, 0); take(v.y, 1); take(v.z, 0); take(v.w, 1); }
	__device__ __forceinline__ unsigned long long sum_bits(int c) const { return (unsigned long long)__double_as_longlong(sm[c]); }
	static __device__ __forceinline__ unsigned long long add(unsigned long long a, unsigned long long b) {
		return (unsigned long long)__double_as_longlong(__longlong_as_double((long long)a) + __longlong_as_double((long long)b));
	}
};
template <> struct LevelsLane<int16_t> {
	typedef uint32_t __attribute__((ext_vector_type(4))) Vec;
	static constexpr uint32_t PER = 8;
	uint32_t pk[2] = {0, 0}, ov[2] = {0, 0}, fs[2] = {0, 0}, nf[2] = {0, 0};
	unsigned long long sm[2] = {0, 0};
	__device__ __forceinline__ void take(const int16_t s16, const int c) {
		const int s = s16;
		const uint32_t a = (uint32_t)(s < 0 ? -s : s);
		sm[c] += a * a; /* (at most 2^30) */
		pk[c] = a > pk[c] ? a : pk[c];
		fs[c] += a >= 32767u ? 1u : 0u;
		ov[c] += a == 32768u ? 1u : 0u;
	}
	__device__ __forceinline__ void take(const uint32_t w) { take((int16_t)(uint16_t)(w & 0xffffu), 0); take((int16_t)(uint16_t)(w >> 16), 1); }
	__device__ __forceinline__ void take(const Vec v) { take(v.x); take(v.y); take(v.z); take(v.w); }
	__device__ __forceinline__ unsigned long long sum_bits(int c) const { return sm[c]; }
	static __device__ __forceinline__ unsigned long long add(unsigned long long a, unsigned long long b) { return a + b; }
};

template <typename SampleT> __device__ __forceinline__ void levels_fold(LevelsPart &a, const LevelsPart &b) {
#pragma unroll
	for (int c = 0; c < 2; ++c) {
		a.sum[c] = LevelsLane<SampleT>::add(a.sum[c], b.sum[c]);
		a.peak[c] = b.peak[c] > a.peak[c] ? b.peak[c] : a.peak[c];
		a.over[c] += b.over[c]; a.full[c] += b.full[c]; a.nonf[c] += b.nonf[c];
	}
}
__device__ __forceinline__ unsigned long long levels_shfl64(unsigned long long v, int off) {
	const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, off), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), off);
	return ((unsigned long long)hi << 32) | lo;
}

template <typename SampleT>
__global__ __launch_bounds__(LEVELS_THREADS) void levels_kernel(const LevelsParams P) {
	typedef LevelsLane<SampleT> Lane;
	typedef typename Lane::Vec Vec;
	constexpr uint32_t PER = Lane::PER;
	__shared__ LevelsPart s_part[LEVELS_THREADS / 64];
	const uint32_t row = blockIdx.y, tid = threadIdx.x;
	const unsigned long long n = (P.row_frames ? (unsigned long long)P.row_frames[row] : P.frames) * P.channels;
	const unsigned long long lo = (unsigned long long)blockIdx.x * LEVELS_WG_SAMPLES;
	if (lo >= n) return; /* (behind the row's end: levels_finish_kernel does not read this block's record) */
	const uint32_t cnt = n - lo < LEVELS_WG_SAMPLES ? (uint32_t)(n - lo) : LEVELS_WG_SAMPLES;
	/* Channels by parity. In an interleaved stereo row sample j belongs to channel j & 1. `lo` is even (LEVELS_WG_SAMPLES is),
	 * a vector begins PER samples (4 or 8: even) further on, and rows start on 16 bytes -- so the elements of every vector
	 * alternate L, R from element 0, and the tail's sample lo + nv * PER + t has the parity of t. A mono row is measured the
	 * same way, as two interleaved halves, which are then joined: [1] into [0]. */
	const SampleT *base = (const SampleT *)((const char *)P.rows + P.pitch * row) + lo;
	const uint32_t nv = cnt / PER; /* whole 16-byte vectors */
	Lane acc;
	uint32_t v = tid;
	for (; v + 3 * LEVELS_THREADS < nv; v += 4 * LEVELS_THREADS) { /* four loads in flight per lane */
		const Vec a = __builtin_nontemporal_load((const Vec *)base + v);
		const Vec b = __builtin_nontemporal_load((const Vec *)base + v + LEVELS_THREADS);
		const Vec c = __builtin_nontemporal_load((const Vec *)base + v + 2 * LEVELS_THREADS);
		const Vec d = __builtin_nontemporal_load((const Vec *)base + v + 3 * LEVELS_THREADS);
		acc.take(a); acc.take(b); acc.take(c); acc.take(d);
	}
	for (; v < nv; v += LEVELS_THREADS) acc.take(__builtin_nontemporal_load((const Vec *)base + v));
	if (tid < cnt - nv * PER) acc.take(base[nv * PER + tid], (int)(tid & 1u)); /* the last < PER samples */
	LevelsPart p;
#pragma unroll
	for (int c = 0; c < 2; ++c) { p.sum[c] = acc.sum_bits(c); p.peak[c] = acc.pk[c]; p.over[c] = acc.ov[c]; p.full[c] = acc.fs[c]; p.nonf[c] = acc.nf[c]; }
	/* the wave: a butterfly, the same pairs in the same order whatever the data (every lane ends with the total) */
#pragma unroll
	for (int off = 32; off >= 1; off >>= 1) {
		LevelsPart o;
#pragma unroll
		for (int c = 0; c < 2; ++c) {
			o.sum[c] = levels_shfl64(p.sum[c], off);
			o.peak[c] = (uint32_t)__shfl_xor((int)p.peak[c], off); o.over[c] = (uint32_t)__shfl_xor((int)p.over[c], off);
			o.full[c] = (uint32_t)__shfl_xor((int)p.full[c], off); o.nonf[c] = (uint32_t)__shfl_xor((int)p.nonf[c], off);
		}
		levels_fold<SampleT>(p, o);
	}
	if ((tid & 63u) == 0) s_part[tid >> 6] = p;
	__syncthreads();
	if (tid != 0) return;
	for (uint32_t w = 1; w < LEVELS_THREADS / 64; ++w) levels_fold<SampleT>(p, s_part[w]); /* the waves, in order */
	if (P.channels == 1) { /* mono: the two halves are one channel */
		p.sum[0] = Lane::add(p.sum[0], p.sum[1]);
		p.peak[0] = p.peak[1] > p.peak[0] ? p.peak[1] : p.peak[0];
		p.over[0] += p.over[1]; p.full[0] += p.full[1]; p.nonf[0] += p.nonf[1];
		p.sum[1] = 0; p.peak[1] = 0; p.over[1] = 0; p.full[1] = 0; p.nonf[1] = 0; /* (the bits of +0.0 too) */
	}
	P.parts[(size_t)row * P.blocks + blockIdx.x] = p;
}

/* one thread per row: the row's partials in ascending block order, then into the row's record */
__global__ __launch_bounds__(64) void levels_finish_kernel(const LevelsParams P) {
	const uint32_t row = blockIdx.x * 64 + threadIdx.x;
	if (row >= P.n_rows) return;
	const unsigned long long frames = P.row_frames ? (unsigned long long)P.row_frames[row] : P.frames;
	const unsigned long long n = frames * P.channels;
	const unsigned long long nb = (n + LEVELS_WG_SAMPLES - 1) / LEVELS_WG_SAMPLES;
	LevelsAcc a;
	if (P.accumulate) a = P.acc[row];
	else {
		a.frames = 0;
		for (int c = 0; c < 2; ++c) { a.isum[c] = 0; a.fsum[c] = 0.0; a.over[c] = a.full[c] = a.nonf[c] = 0; a.ipeak[c] = 0; a.fpeak[c] = 0.f; }
	}
	if (nb) {
		/* (the counts of a row are summed in 64 bits: a block's fit 32, a row's need not) */
		const LevelsPart *parts = P.parts + (size_t)row * P.blocks;
		unsigned long long sum[2] = {parts[0].sum[0], parts[0].sum[1]}, over[2] = {parts[0].over[0], parts[0].over[1]},
			full[2] = {parts[0].full[0], parts[0].full[1]}, nonf[2] = {parts[0].nonf[0], parts[0].nonf[1]};
		uint32_t peak[2] = {parts[0].peak[0], parts[0].peak[1]};
		auto fold = [&](const LevelsPart &p) {
			for (int c = 0; c < 2; ++c) {
				sum[c] = P.f32 ? LevelsLane<float>::add(sum[c], p.sum[c]) : sum[c] + p.sum[c];
				peak[c] = p.peak[c] > peak[c] ? p.peak[c] : peak[c];
				over[c] += p.over[c]; full[c] += p.full[c]; nonf[c] += p.nonf[c];
			}
		};
		unsigned long long b = 1;
		for (; b + 3 < nb; b += 4) { /* four records' loads in flight ahead of the adds, which keep their order */
			const LevelsPart p0 = parts[b], p1 = parts[b + 1], p2 = parts[b + 2], p3 = parts[b + 3];
			fold(p0); fold(p1); fold(p2); fold(p3);
		}
		for (; b < nb; ++b) fold(parts[b]);
		a.frames += frames;
		for (int c = 0; c < 2; ++c) {
			if (P.f32) {
				a.fsum[c] += __longlong_as_double((long long)sum[c]);
				const float pf = __uint_as_float(peak[c]);
				a.fpeak[c] = __float_as_uint(pf) > __float_as_uint(a.fpeak[c]) ? pf : a.fpeak[c];
			} else {
				a.isum[c] += sum[c];
				a.ipeak[c] = peak[c] > a.ipeak[c] ? peak[c] : a.ipeak[c];
			}
			a.over[c] += over[c]; a.full[c] += full[c]; a.nonf[c] += nonf[c];
		}
	}
	P.acc[row] = a;
}

/* The normalised writer's second pass (sndout.cpp): dst[i] = pcm16(src[i] * gain), byte-swapped for AU files, or src[i] * gain
 * as a float. One f32 multiply; pcm16()'s clamp sits between it and the * 32767, so nothing can contract. Four samples per
 * thread: a 16-byte streaming load, one 8- or 16-byte store (src and dst start on 256 bytes), a scalar tail. */
struct RequantParams {
	const float *src;
	void *dst;
	unsigned long long n; /* samples */
	float gain;
	uint32_t swap_bytes;
};
template <typename OutT>
__global__ __launch_bounds__(256) void requant_kernel(const RequantParams P) {
	typedef float __attribute__((ext_vector_type(4))) f32x4;
	typedef uint32_t __attribute__((ext_vector_type(2))) u32x2;
	const unsigned long long i0 = ((unsigned long long)blockIdx.x * 256 + threadIdx.x) * 4;
	if (i0 >= P.n) return;
	OutT *dst = (OutT *)P.dst;
	auto one = [&](float x) -> OutT {
		const float y = x * P.gain;
		if constexpr (std::is_same<OutT, float>::value) return y;
		else { const int16_t q = pcm16(y); return P.swap_bytes ? pcm_swap(q) : q; }
	};
	if (i0 + 4 <= P.n) {
		const f32x4 q = __builtin_nontemporal_load((const f32x4 *)(P.src + i0));
		if constexpr (std::is_same<OutT, float>::value) {
			f32x4 y; y.x = one(q.x); y.y = one(q.y); y.z = one(q.z); y.w = one(q.w);
			*(f32x4 *)(dst + i0) = y;
		} else {
			u32x2 w;
			w.x = (uint32_t)(uint16_t)one(q.x) | ((uint32_t)(uint16_t)one(q.y) << 16);
			w.y = (uint32_t)(uint16_t)one(q.z) | ((uint32_t)(uint16_t)one(q.w) << 16);
			*(u32x2 *)(dst + i0) = w;
		}
		return;
	}
	for (unsigned long long i = i0; i < P.n; ++i) dst[i] = one(P.src[i]);
}

#endif
