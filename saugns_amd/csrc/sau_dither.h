/* sau_dither.h -- the 16-bit quantiser's arithmetic (include/saugns_amd.h, section "Dither and noise shaping"), shared by the
 * host restatement (tables.cpp: dither_quantize) and the kernels (k_dither.h) the way sau_flac.h is: the spec and its rules,
 * the dither as a function of position, the scaling of one sample and one step of the error-feedback recurrence. The dither is
 * integer arithmetic up to one exact conversion, and the recurrence is f64 steps with a stated order (the build is
 * -ffp-contract=off), so host and device agree by construction; what differs between them is only who walks the samples. */
#ifndef SAU_DITHER_H
#define SAU_DITHER_H
#include <stdint.h>
#include <math.h>
#include "sau_dev_math.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SAU_DITHER_HD __host__ __device__ inline
#else
#define SAU_DITHER_HD static inline
#endif

namespace saudither {

constexpr unsigned DITHER_TAPS_MAX = 9;
constexpr uint32_t DITHER_MAX_ROWS = 65535;
constexpr double DITHER_COEF_SUM_MAX = 64.0; /* of |coef[j]| over the used taps: keeps |w - s| < 96 with |e| < 1.5 */
enum : int { DITHER_FLAT = 0, DITHER_HP1 = 1, DITHER_E3 = 2, DITHER_E5 = 3, DITHER_F9 = 4 };

/* sauAmdDither */
struct DitherSpec {
	uint64_t seed;
	uint32_t dither;   /* 0 none, 1 TPDF */
	uint32_t taps;     /* T, 0 .. 9 */
	double coef[DITHER_TAPS_MAX];
};
static_assert(sizeof(DitherSpec) == 88, "DitherSpec is sauAmdDither");

/* What a chain -- one channel of one row -- keeps between feeds: e[j] the error j + 1 frames back, and its clamped samples. */
struct DitherChain {
	double e[DITHER_TAPS_MAX];
	uint64_t clipped;
};
static_assert(sizeof(DitherChain) == 80, "DitherChain is read and written by the kernels as it stands");

SAU_DITHER_HD bool dither_spec_ok(const DitherSpec &s) {
	if (s.dither > 1 || s.taps > DITHER_TAPS_MAX) return false;
	double sum = 0.0;
	for (unsigned j = 0; j < s.taps; ++j) {
		const double a = fabs(s.coef[j]);
		if (!(a <= 1.7976931348623157e308)) return false; /* (a NaN fails the comparison) */
		sum += a;
	}
	return sum <= DITHER_COEF_SUM_MAX;
}
/* neither dither nor shaping: the stored sample is pcm16(x * gain), the existing writers' rounding */
SAU_DITHER_HD bool dither_spec_plain(const DitherSpec &s) { return !s.dither && !s.taps; }

/* the published error-feedback sets; false for any other shape (out is left alone) */
SAU_DITHER_HD bool dither_preset(int shape, uint64_t seed, DitherSpec &out) {
	const double hp1[1] = {1.0};
	const double e3[3] = {1.623, -0.982, 0.109};
	const double e5[5] = {2.033, -2.165, 1.959, -1.590, 0.6149};
	const double f9[9] = {2.412, -3.370, 3.937, -4.174, 3.353, -2.205, 1.281, -0.569, 0.0847};
	const double *c = nullptr;
	unsigned n = 0;
	switch (shape) {
	case DITHER_FLAT: break;
	case DITHER_HP1: c = hp1; n = 1; break;
	case DITHER_E3: c = e3; n = 3; break;
	case DITHER_E5: c = e5; n = 5; break;
	case DITHER_F9: c = f9; n = 9; break;
	default: return false;
	}
	out.seed = seed; out.dither = 1; out.taps = n;
	for (unsigned j = 0; j < DITHER_TAPS_MAX; ++j) out.coef[j] = j < n ? c[j] : 0.0;
	return true;
}

/* ---- the dither: splitmix64's output at a counter, a function of (seed, row, frame, channel) only ---- */
SAU_DITHER_HD uint64_t dither_row_seed(uint64_t seed, uint64_t row) { return seed + 0xD1B54A32D192ED03ull * row; }
SAU_DITHER_HD uint64_t dither_hash(uint64_t seed_r, uint64_t frame, unsigned ch) {
	uint64_t z = seed_r + 0x9E3779B97F4A7C15ull * (2 * frame + ch + 1);
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
	return z ^ (z >> 31);
}
/* two 24-bit fields' difference: triangular on (-1, 1) LSB, exact in f32 (|a - b| < 2^24, then a power of two) */
SAU_DITHER_HD float dither_tpdf(uint64_t seed_r, uint64_t frame, unsigned ch) {
	const uint64_t z = dither_hash(seed_r, frame, ch);
	const int32_t a = (int32_t)(z >> 40), b = (int32_t)((z >> 16) & 0xFFFFFFu);
	return (float)(a - b) * 5.9604644775390625e-08f;
}

/* ---- one sample ---- */
/* x * gain in one f32 multiply, pcm16's NaN rule and clamp */
SAU_DITHER_HD float dither_scale(float x, float gain) {
	float y = x * gain;
	if (y != y) y = -1.f;
	return saudev::clampf(y, -1.f, 1.f);
}
/* in LSB: exact (24 bits times 15) */
SAU_DITHER_HD double dither_lsb(float y) { return (double)y * 32767.0; }

/* One step of a chain. s: dither_lsb's; d: the position's dither (0 without); coef[0 .. T), T <= 9; e[0 .. 9) the chain's
 * errors, which move on by one when T > 0 (all nine: a build of nine taps whose upper coefficients are zeros keeps the same
 * state as one of T, and t + (+-0) leaves t, which starts at +0.0, as it is). Every product is rounded before the sum it
 * enters, the most recent error enters last: the dependent chain is multiply, subtract, add, round, subtract. -> the sample,
 * -32767 .. 32767; clipped: whether the clamp changed it. */
SAU_DITHER_HD int32_t dither_step(const double *coef, unsigned T, double *e, double s, float d, bool &clipped) {
	double w = s;
	if (T) {
		double t = 0.0;
		for (unsigned j = T - 1; j >= 1; --j) t = t + coef[j] * e[j];
		w = (s - t) - coef[0] * e[0];
	}
	const double q = rint(w + (double)d);
	if (T) {
		for (unsigned j = DITHER_TAPS_MAX - 1; j >= 1; --j) e[j] = e[j - 1];
		e[0] = q - w;
	}
	const double c = q < -32767.0 ? -32767.0 : (q > 32767.0 ? 32767.0 : q);
	clipped = c != q;
	return (int32_t)c;
}

} /* namespace saudither */
#endif /* SAU_DITHER_H */
