/* kat_kernels.hip -- TEST INFRASTRUCTURE (tests/hooks/libsaugns_amd_hooks.so only): known-answer probes of the shared
 * arithmetic (saugns_amd/csrc/sau_dev_math.h, sau_flac.h) as hipcc compiles it for gfx950, with the product's flags. Until round 4
 * these kernels sat in the product library; VERDICT r04 item 9 moved them here. */
#include <hip/hip_runtime.h>
#include "../../saugns_amd/csrc/sau_dev_ops.h"
#include <stdint.h>
#include "../../saugns_amd/csrc/k_wave_scan.h"
#include "../../saugns_amd/csrc/sau_flac.h"

using namespace saudev;

/* the kernels' wave-level helpers and short rounding forms, as hip_backend.hip includes them (inside a namespace there) */
namespace katk {
#include "../../saugns_amd/csrc/k_common.h"
}

/* div_diff_scale(a, b) against IEEE a / b for every f32 b with 1 <= |b| <= 2^31 (a superset of the rounded integers the
 * differentiator divides by). Thread t takes the bit patterns t, t + stride, ... */
__global__ void kat_div_kernel(float a, int variant, unsigned long long *mismatches, uint32_t *first_bad) {
	const uint32_t lo = 0x3f800000u, hi = 0x4f000000u; /* 1.0f .. 2^31 */
	unsigned long long bad = 0;
	for (uint32_t bits = lo + blockIdx.x * blockDim.x + threadIdx.x; bits <= hi; bits += gridDim.x * blockDim.x) {
		for (int sgn = 0; sgn < 2; ++sgn) {
			const float b = bits_f(bits | (sgn ? 0x80000000u : 0u));
			const float want = __fdiv_rn(a, b);
			float got;
			if (variant == 0) {
				got = div_diff_scale(a, b);
			} else if (variant == 2) { /* the unmodulated rows' one division per group (k_fast_group.h) */
				got = div_f32_normal(a, b);
			} else { /* no correction: the probe must be able to see this fail */
				got = a * __builtin_amdgcn_rcpf(b);
			}
			if (f_bits(want) != f_bits(got)) { ++bad; atomicMin(first_bad, bits); }
		}
		if (bits > hi - gridDim.x * blockDim.x) break; /* no wrap past the last pattern */
	}
	if (bad) atomicAdd(mismatches, bad);
}

/* one block evaluates a line for `len` samples exactly as the kernels' ST_LINE step does */
__global__ void kat_line_kernel(LineState st, uint32_t len, const float *mul, float *out, LineState *st_out) {
	LineState ls = st;
	LineBlock lb = line_begin(ls, len, mul != nullptr, mul ? mul[0] : 0.f, lattice_none(), 0);
	for (uint32_t j = threadIdx.x; j < len; j += blockDim.x)
		out[j] = line_value(lb, j, mul ? mul[j] : 1.f);
	if (threadIdx.x == 0) *st_out = ls;
}

bool kat_div(float a, int variant, unsigned long long *mismatches, uint32_t *first_bad) {
	unsigned long long *d_m = nullptr;
	uint32_t *d_f = nullptr;
	bool ok = hipMalloc((void **)&d_m, sizeof *d_m) == hipSuccess && hipMalloc((void **)&d_f, sizeof *d_f) == hipSuccess;
	if (ok) {
		const uint32_t none = 0xffffffffu;
		ok = hipMemset(d_m, 0, sizeof *d_m) == hipSuccess &&
			hipMemcpy(d_f, &none, sizeof none, hipMemcpyHostToDevice) == hipSuccess;
	}
	if (ok) {
		hipLaunchKernelGGL(kat_div_kernel, dim3(4096), dim3(256), 0, 0, a, variant, d_m, d_f);
		ok = hipDeviceSynchronize() == hipSuccess &&
			hipMemcpy(mismatches, d_m, sizeof *d_m, hipMemcpyDeviceToHost) == hipSuccess &&
			hipMemcpy(first_bad, d_f, sizeof *d_f, hipMemcpyDeviceToHost) == hipSuccess;
	}
	if (d_m) (void)hipFree(d_m);
	if (d_f) (void)hipFree(d_f);
	return ok;
}

bool kat_line(const LineState &st, uint32_t len, const float *mul, float *out, LineState *st_out) {
	float *d_mul = nullptr, *d_out = nullptr;
	LineState *d_st = nullptr;
	bool ok = hipMalloc((void **)&d_out, (len + 1) * sizeof(float)) == hipSuccess &&
		hipMalloc((void **)&d_st, sizeof(LineState)) == hipSuccess;
	if (ok && mul) {
		ok = hipMalloc((void **)&d_mul, (len + 1) * sizeof(float)) == hipSuccess &&
			hipMemcpy(d_mul, mul, len * sizeof(float), hipMemcpyHostToDevice) == hipSuccess;
	}
	if (ok) {
		hipLaunchKernelGGL(kat_line_kernel, dim3(1), dim3(256), 0, 0, st, len, d_mul, d_out, d_st);
		ok = hipDeviceSynchronize() == hipSuccess &&
			hipMemcpy(out, d_out, len * sizeof(float), hipMemcpyDeviceToHost) == hipSuccess &&
			hipMemcpy(st_out, d_st, sizeof(LineState), hipMemcpyDeviceToHost) == hipSuccess;
	}
	if (d_mul) (void)hipFree(d_mul);
	if (d_out) (void)hipFree(d_out);
	if (d_st) (void)hipFree(d_st);
	return ok;
}

/* the 64-bit wave scan and sum (k_wave_scan.h): one wave per 64 values */
__global__ void kat_scan64_kernel(const unsigned long long *in, unsigned long long *scan, unsigned long long *sum) {
	const uint32_t i = blockIdx.x * 64 + threadIdx.x;
	scan[i] = wave_incl_scan64_dpp(in[i]);
	const unsigned long long t = wave_sum64_dpp(in[i]);
	if (threadIdx.x == 0) sum[blockIdx.x] = t;
}
bool kat_scan64(const unsigned long long *in, unsigned long long *scan, unsigned long long *sum, uint32_t n_waves) {
	unsigned long long *d_in = nullptr, *d_scan = nullptr, *d_sum = nullptr;
	const size_t nb = (size_t)n_waves * 64 * sizeof(unsigned long long);
	bool ok = hipMalloc((void **)&d_in, nb) == hipSuccess && hipMalloc((void **)&d_scan, nb) == hipSuccess &&
		hipMalloc((void **)&d_sum, n_waves * sizeof(unsigned long long)) == hipSuccess &&
		hipMemcpy(d_in, in, nb, hipMemcpyHostToDevice) == hipSuccess;
	if (ok) {
		hipLaunchKernelGGL(kat_scan64_kernel, dim3(n_waves), dim3(64), 0, 0, d_in, d_scan, d_sum);
		ok = hipDeviceSynchronize() == hipSuccess && hipMemcpy(scan, d_scan, nb, hipMemcpyDeviceToHost) == hipSuccess &&
			hipMemcpy(sum, d_sum, n_waves * sizeof(unsigned long long), hipMemcpyDeviceToHost) == hipSuccess;
	}
	if (d_in) (void)hipFree(d_in);
	if (d_scan) (void)hipFree(d_scan);
	if (d_sum) (void)hipFree(d_sum);
	return ok;
}

/* rint64() (sau_dev_math.h: llrintf with the host's out-of-range answer) for EVERY f32 bit pattern against an independent
 * formulation -- the value rounded in f64 and taken apart by hand -- in two lane orders: consecutive patterns (a wave's lanes
 * alike in magnitude: the wave-uniform short form below 2^31, or the long form) and scattered ones (both forms' lanes in one
 * wave). franssgauss32()'s scaled conversions against the reference's double form, for every 32-bit integer, ride along. */
__device__ __forceinline__ long long kat_rint64_ref(float x) {
	if (!(fabsf(x) < 0x1p63f)) return (long long)0x8000000000000000ull; /* (NaN too) */
	const double d = rint((double)x); /* round-half-even, exact: an f32 has 24 significant bits */
	const double a = fabs(d);
	const double hi = floor(a * 0x1p-32);
	const unsigned long long mag = ((unsigned long long)(uint32_t)hi << 32) | (unsigned long long)(uint32_t)(a - hi * 0x1p32);
	return d < 0 ? (long long)(0ull - mag) : (long long)mag;
}
__global__ void kat_rint64_kernel(int scattered, unsigned long long *mismatches, uint32_t *first_bad) {
	unsigned long long bad = 0;
	const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x, n = gridDim.x * blockDim.x; /* n divides 2^32 */
	for (uint32_t k = 0; k < (uint32_t)(0x100000000ull / n); ++k) {
		uint32_t bits = k * n + tid;
		if (scattered) bits *= 0x9e3779b1u; /* (odd: a permutation of the patterns; neighbouring lanes far apart) */
		const float x = bits_f(bits);
		if (rint64(x) != kat_rint64_ref(x)) { ++bad; atomicMin(first_bad, bits); }
		const int32_t s0 = (int32_t)bits;
		if (f_bits((float)s0 * 0x1p-32f) != f_bits((float)((double)s0 * 0x1p-32))) { ++bad; atomicMin(first_bad, bits); }
	}
	if (bad) atomicAdd(mismatches, bad);
}
bool kat_rint64(int scattered, unsigned long long *mismatches, uint32_t *first_bad) {
	unsigned long long *d_m = nullptr;
	uint32_t *d_f = nullptr;
	bool ok = hipMalloc((void **)&d_m, sizeof *d_m) == hipSuccess && hipMalloc((void **)&d_f, sizeof *d_f) == hipSuccess;
	if (ok) {
		const uint32_t none = 0xffffffffu;
		ok = hipMemset(d_m, 0, sizeof *d_m) == hipSuccess && hipMemcpy(d_f, &none, sizeof none, hipMemcpyHostToDevice) == hipSuccess;
	}
	if (ok) {
		hipLaunchKernelGGL(kat_rint64_kernel, dim3(4096), dim3(256), 0, 0, scattered, d_m, d_f);
		ok = hipDeviceSynchronize() == hipSuccess &&
			hipMemcpy(mismatches, d_m, sizeof *d_m, hipMemcpyDeviceToHost) == hipSuccess &&
			hipMemcpy(first_bad, d_f, sizeof *d_f, hipMemcpyDeviceToHost) == hipSuccess;
	}
	if (d_m) (void)hipFree(d_m);
	if (d_f) (void)hipFree(d_f);
	return ok;
}

/* The 32-bit rounding forms of phase offsets, increments and cycle counts (sau_dev_math.h, k_common.h) for EVERY f32 bit
 * pattern against independent formulations in f64 (kat_rint64_ref for llrintf; cvttss2si and the reference build's floorf
 * below), in kat_rint64_kernel's two lane orders: the wave-wide guards in front of the short forms see waves of alike and
 * of mixed magnitudes. `fn`:
 *   0 rint32w(x)            == low word of llrintf(x), every x (NaN, infinities and |x| >= 2^63 give 0 on the host)
 *   1 rint32w_p31(p)        == low word of llrintf(p * 0x1p31f), the product rounded in f32 as the host rounds it
 *   2 rint32w_p31_small(p)  == the same for |p| < 2^20; counted apart: [2^20, 2^21) and (-2^21, -2^20], where it is wrong
 *   3 rint32w_small(x)      == low word of llrintf(x) for |x| < 2^50; counted apart: [2^51, 2^52), where it is wrong
 *   4 f2i_x86(x)            == cvttss2si: truncation, 0x80000000 out of range and for NaN
 *   5 floor_i32_ref(x)      == cvttss2si, then one off where that lies above x, in 32-bit arithmetic (below -2^31: INT32_MAX)
 * n[0]: mismatches where the form must hold, n[1] / n[2]: mismatches in the positive / negative control range. */
__device__ __forceinline__ int32_t kat_cvtt_ref(float x) {
	const double d = (double)x;
	if (!(d >= -0x1p31 && d < 0x1p31)) return (int32_t)0x80000000u; /* (NaN too) */
	return (int32_t)trunc(d);
}
__device__ __forceinline__ int32_t kat_floor_ref(float x) {
	const double d = (double)x;
	if (d < -0x1p31) return INT32_MAX; /* truncation gave 0x80000000 = -2^31, above x: minus one wraps */
	if (!(d < 0x1p31)) return (int32_t)0x80000000u; /* (NaN too) */
	return (int32_t)floor(d);
}
__global__ void kat_round32_kernel(int fn, int scattered, unsigned long long *n, uint32_t *first_bad) {
	unsigned long long bad = 0, ctrl_pos = 0, ctrl_neg = 0;
	const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x, nt = gridDim.x * blockDim.x; /* nt divides 2^32 */
	for (uint32_t k = 0; k < (uint32_t)(0x100000000ull / nt); ++k) {
		uint32_t bits = k * nt + tid;
		if (scattered) bits *= 0x9e3779b1u;
		const float x = bits_f(bits);
		const float ax = fabsf(x);
		uint32_t got, want;
		bool in = true;
		int ctrl = 0; /* +1 / -1: x lies in the positive / negative control range */
		switch (fn) {
		case 0: got = rint32w(x); want = (uint32_t)kat_rint64_ref(x); break;
		case 1: got = rint32w_p31(x); want = (uint32_t)kat_rint64_ref(x * 0x1p31f); break;
		case 2:
			got = katk::rint32w_p31_small(x); want = (uint32_t)kat_rint64_ref(x * 0x1p31f);
			in = ax < 0x1p20f;
			ctrl = (ax >= 0x1p20f && ax < 0x1p21f) ? (x > 0 ? 1 : -1) : 0;
			break;
		case 3:
			got = katk::rint32w_small(x); want = (uint32_t)kat_rint64_ref(x);
			in = ax < 0x1p50f;
			ctrl = (x >= 0x1p51f && x < 0x1p52f) ? 1 : 0;
			break;
		case 4: got = (uint32_t)f2i_x86(x); want = (uint32_t)kat_cvtt_ref(x); break;
		default: got = (uint32_t)floor_i32_ref(x); want = (uint32_t)kat_floor_ref(x); break;
		}
		if (got != want) {
			if (in) { ++bad; atomicMin(first_bad, bits); }
			else if (ctrl > 0) ++ctrl_pos;
			else if (ctrl < 0) ++ctrl_neg;
		}
	}
	if (bad) atomicAdd(&n[0], bad);
	if (ctrl_pos) atomicAdd(&n[1], ctrl_pos);
	if (ctrl_neg) atomicAdd(&n[2], ctrl_neg);
}
bool kat_round32(int fn, int scattered, unsigned long long *counts, uint32_t *first_bad) {
	unsigned long long *d_n = nullptr;
	uint32_t *d_f = nullptr;
	bool ok = hipMalloc((void **)&d_n, 3 * sizeof *d_n) == hipSuccess && hipMalloc((void **)&d_f, sizeof *d_f) == hipSuccess;
	if (ok) {
		const uint32_t none = 0xffffffffu;
		ok = hipMemset(d_n, 0, 3 * sizeof *d_n) == hipSuccess && hipMemcpy(d_f, &none, sizeof none, hipMemcpyHostToDevice) == hipSuccess;
	}
	if (ok) {
		hipLaunchKernelGGL(kat_round32_kernel, dim3(4096), dim3(256), 0, 0, fn, scattered, d_n, d_f);
		ok = hipDeviceSynchronize() == hipSuccess &&
			hipMemcpy(counts, d_n, 3 * sizeof *d_n, hipMemcpyDeviceToHost) == hipSuccess &&
			hipMemcpy(first_bad, d_f, sizeof *d_f, hipMemcpyDeviceToHost) == hipSuccess;
	}
	if (d_n) (void)hipFree(d_n);
	if (d_f) (void)hipFree(d_f);
	return ok;
}

/* Steps 3 to 5 of the FLAC encoder's LPC mode (sau_flac.h: flac_lpc_f64_shift, the conversions, flac_lpc_orders) as
 * flac_analyze_lpc (k_flac.h) strings them together: workgroups of 256, lane 0 of each of the four waves takes one
 * autocorrelation, and r, a, q and shift lie in LDS laid out like that kernel's FlacLpcLds, so that the function indexes LDS at
 * run time here as it does there. The wave then copies out what the function wrote -- q and shift of the orders in the mask,
 * a[0 .. M-1] as bit patterns -- with ordinary stores; everything else in the host's buffers keeps the host's pattern. */
struct KatLpcLds {
	double r[4][sauflac::FLAC_LPC_MAX + 1];
	double a[4][sauflac::FLAC_LPC_MAX];
	int16_t q[4][sauflac::FLAC_LPC_MAX * sauflac::FLAC_LPC_MAX];
	uint8_t shift[4][sauflac::FLAC_LPC_MAX];
	uint32_t mask[4];
};
__global__ __launch_bounds__(256) void kat_flac_lpc_orders_kernel(const long long *R, const uint32_t *M, uint32_t n, uint32_t *g_out,
		uint32_t *mask_out, int16_t *q_out, uint8_t *shift_out, unsigned long long *a_out) {
	using namespace sauflac;
	__shared__ KatLpcLds L;
	const unsigned c = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const uint32_t v = blockIdx.x * 4 + c;
	if (lane == 0 && v < n) {
		const long long *Rv = R + (size_t)v * (FLAC_LPC_MAX + 1);
		const unsigned g = flac_lpc_f64_shift(Rv[0]);
		for (unsigned l = 0; l <= FLAC_LPC_MAX; ++l) L.r[c][l] = (double)(Rv[l] >> g);
		L.mask[c] = flac_lpc_orders(L.r[c], M[v], L.a[c], L.q[c], L.shift[c]);
		g_out[v] = g;
	}
	__syncthreads();
	if (v < n) {
		const uint32_t mask = L.mask[c];
		const unsigned m1 = lane >> 3, j = lane & 7; /* q[(m - 1) * 8 + j] */
		if (((mask >> m1) & 1u) && j <= m1) q_out[(size_t)v * 64 + lane] = L.q[c][lane];
		if (lane < FLAC_LPC_MAX && ((mask >> lane) & 1u)) shift_out[(size_t)v * FLAC_LPC_MAX + lane] = L.shift[c][lane];
		if (lane < M[v]) a_out[(size_t)v * FLAC_LPC_MAX + lane] = flac_f64_bits(L.a[c][lane]);
		if (lane == 0) mask_out[v] = mask;
	}
}
/* (the host's buffers go to the device as they are and come back: what the kernel leaves alone keeps the caller's pattern) */
bool kat_flac_lpc_orders(const int64_t *R, const uint32_t *M, uint32_t n, uint32_t *g, uint32_t *mask, int16_t *q, uint8_t *shift,
		uint64_t *a_bits) {
	const size_t nb[7] = {(size_t)n * 9 * sizeof(int64_t), n * sizeof(uint32_t), n * sizeof(uint32_t), n * sizeof(uint32_t),
		(size_t)n * 64 * sizeof(int16_t), (size_t)n * 8, (size_t)n * 8 * sizeof(uint64_t)};
	const void *src[7] = {R, M, g, mask, q, shift, a_bits};
	void *dst[7] = {nullptr, nullptr, g, mask, q, shift, a_bits};
	void *d[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
	bool ok = true;
	for (int i = 0; i < 7 && ok; ++i)
		ok = hipMalloc(&d[i], nb[i]) == hipSuccess && hipMemcpy(d[i], src[i], nb[i], hipMemcpyHostToDevice) == hipSuccess;
	if (ok) {
		hipLaunchKernelGGL(kat_flac_lpc_orders_kernel, dim3((n + 3) / 4), dim3(256), 0, 0, (const long long *)d[0], (const uint32_t *)d[1], n,
			(uint32_t *)d[2], (uint32_t *)d[3], (int16_t *)d[4], (uint8_t *)d[5], (unsigned long long *)d[6]);
		ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess;
	}
	for (int i = 2; i < 7 && ok; ++i) ok = hipMemcpy(dst[i], d[i], nb[i], hipMemcpyDeviceToHost) == hipSuccess;
	for (int i = 0; i < 7; ++i)
		if (d[i]) (void)hipFree(d[i]);
	return ok;
}
