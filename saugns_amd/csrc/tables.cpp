/* tables.cpp -- the twelve pre-integrated wave tables ("PILUTs") and their
 * per-wave constants.
 *
 * Table *generation* is host-side, one-time work (sau/wave.c:77-221); only the
 * lookup is on the hot path.  Three sources, in order of preference:
 *   1. tables handed in through sauAmd_set_piluts() (tests use the compiled
 *      reference's own arrays, which differ from a strict-order build by 1 ulp
 *      in srs/ean/cat/mto because the reference compiles wave.c with
 *      -ffast-math),
 *   2. when this library is linked into the reference host: that host's own
 *      `sauWave_piluts` (looked up with dlsym, so the generator uses exactly
 *      the tables the rest of the program was built with),
 *   3. the strict-order builder below.
 */
#include "engine.h"
#include "sau_md5.h"
#include "sau_flac_dec.h"
#include <dlfcn.h>
#include <float.h>
#include <math.h>
#include <string.h>

namespace sauengine {

namespace {

enum { WLEN = 2048, WHALF = WLEN / 2, WQUART = WLEN / 4 };

float g_tables[SAU_WAVE_NAMED][WLEN];
bool g_ready = false;

/* sau/wave.h:33-69: {amp_scale, amp_dc, phase_adj} */
struct PiCoeff { float amp_scale, amp_dc; int32_t phase_adj; };
const PiCoeff g_pico[SAU_WAVE_NAMED] = {
	{1.27324153848f, 0.0f, INT32_MIN / 2},            /* sin */
	{1.00097751711f, 0.0f, 0},                        /* tri */
	{1.52547437578f, 0.0f, 0},                        /* srs */
	{2.00000000000f, 0.0f, INT32_MIN / 2},            /* sqr */
	{1.20275515347f, -0.24257955076f, 0},             /* ean */
	{1.37070880305f, -0.23725526633f, 0},             /* cat */
	{(float)(1.26113986272 * -1), 0.0f, -(INT32_MIN / 2)}, /* eto */
	{1.02639326795f, -0.33333333333f, 0},             /* par */
	{1.57268451738f, -0.23724704918f, 0},             /* mto */
	{(float)(1.00048851979 * -1), 0.0f, -(INT32_MIN / 2)}, /* saw */
	{1.40333871035f, -0.36334126990f, 0},             /* hsi */
	{1.07213756312f, 0.27322393756f, 0},              /* spa */
};
WaveConst g_wconst[SAU_WAVE_NAMED];
bool g_wconst_ready = false;

/* sau/wave.c:77-98 */
void integrate(float *dst, const float *src) {
	const float inv = 1.f / (WLEN * 0.125f);
	double mean = 0.f;
	for (int i = 0; i < WLEN; ++i) mean += src[i];
	mean /= WLEN;
	double run = 0.f;
	float lo = 0.f, hi = 0.f;
	for (int i = 0; i < WLEN; ++i) {
		run += src[i] - mean;
		float x = (float)(run * inv);
		if (x < lo) lo = x;
		if (x > hi) hi = x;
		dst[i] = x;
	}
	float gain = 1.f / ((hi - lo) * 0.5f);
	float shift = -(hi + lo) * 0.5f;
	for (int i = 0; i < WLEN; ++i) dst[i] = (dst[i] + shift) * gain;
}

/* sau/wave.c:105-214, only what the PILUT set needs */
void build() {
	static float sine[WLEN], tri[WLEN], tri_i[WLEN], ean[WLEN], par[WLEN];
	static float srs[WLEN], cat[WLEN], mto[WLEN], hsi[WLEN], spa[WLEN];
	const double pi = 3.14159265358979323846;
	for (int i = 0; i < WHALF; ++i) {
		const double x = i * (1.f / WHALF);
		const float sx = (float)sin(pi * x);
		sine[i] = sx; sine[i + WHALF] = -sx;
		const float rx = sqrtf(sx);
		srs[i] = rx;
		hsi[i] = sx * 2 - 1.f;
		mto[i] = rx * 2 - 1.f;
		const float px = (float)sin(pi * 0.5f * (1 + x));
		spa[i + WQUART] = px * 2 - 1.f;
		const double xr = (WHALF - i) * (1.f / WHALF);
		par[i + WQUART] = (float)((xr * xr) * 2.f - 1.f);
	}
	par[WHALF + WQUART] = -1.f;
	spa[WHALF + WQUART] = -1.f;
	for (int i = 0; i < WQUART; ++i) {
		const double x = i * (1.f / WQUART);
		const double xr = (WQUART - i) * (1.f / WQUART);
		tri_i[i] = (float)((x * x) - 1.f);
		tri_i[i + WQUART] = (float)(1.f - (xr * xr));
		tri[i] = (float)x;
		tri[i + WQUART] = (float)xr;
		par[i] = par[WHALF - i];
		par[i + WHALF + WQUART] = par[WHALF + WQUART - i];
		spa[i] = spa[WHALF - i];
		spa[i + WHALF + WQUART] = spa[WHALF + WQUART - i];
	}
	for (int i = WHALF; i < WLEN; ++i) {
		tri_i[i] = -tri_i[i - WHALF];
		tri[i] = -tri[i - WHALF];
		hsi[i] = -1.f;
		mto[i] = -1.f;
		srs[i] = -srs[i - WHALF];
	}
	const float ean_dc = (float)((1.14603185654 - 1.f) / 2.f);
	const float ean_gain = (float)(1.f / 1.07301592827);
	for (int i = 0; i < WLEN; ++i) {
		ean[i] = (sine[i] + par[i] - tri[i] + ean_dc) * ean_gain;
		cat[i] = sine[i] + mto[i] - srs[i];
	}
	/* sau/wave.c:49-62: which array differentiates into which wave */
	memcpy(g_tables[SAU_WAVE_N_sin], sine, sizeof sine);
	memcpy(g_tables[SAU_WAVE_N_tri], tri_i, sizeof tri_i);
	integrate(g_tables[SAU_WAVE_N_srs], srs);
	memcpy(g_tables[SAU_WAVE_N_sqr], tri, sizeof tri);
	integrate(g_tables[SAU_WAVE_N_ean], ean);
	integrate(g_tables[SAU_WAVE_N_cat], cat);
	memcpy(g_tables[SAU_WAVE_N_eto], ean, sizeof ean);
	integrate(g_tables[SAU_WAVE_N_par], par);
	integrate(g_tables[SAU_WAVE_N_mto], mto);
	memcpy(g_tables[SAU_WAVE_N_saw], par, sizeof par);
	integrate(g_tables[SAU_WAVE_N_hsi], hsi);
	integrate(g_tables[SAU_WAVE_N_spa], spa);
}

/* When the reference host is in the process image, adopt its tables. */
bool adopt_host_tables() {
	typedef void (*init_f)(void);
	init_f init = (init_f)dlsym(RTLD_DEFAULT, "sau_global_init_Wave");
	float *const *tabs = (float *const *)dlsym(RTLD_DEFAULT, "sauWave_piluts");
	if (!init || !tabs) return false;
	init();
	for (int w = 0; w < SAU_WAVE_NAMED; ++w) {
		if (!tabs[w]) return false;
		memcpy(g_tables[w], tabs[w], sizeof g_tables[w]);
	}
	return true;
}

} /* namespace */

const float *builtin_piluts() {
	if (!g_ready) {
		if (!adopt_host_tables()) build();
		g_ready = true;
	}
	return &g_tables[0][0];
}

void override_piluts(const float *tables) {
	memcpy(g_tables, tables, sizeof g_tables);
	g_ready = true;
}

const WaveConst *wave_consts() {
	if (!g_wconst_ready) {
		for (int w = 0; w < SAU_WAVE_NAMED; ++w) {
			/* sau/wave.h:144-149 */
			g_wconst[w].diff_scale = g_pico[w].amp_scale * 0.125f * (float)UINT32_MAX;
			g_wconst[w].diff_offset = g_pico[w].amp_dc;
			g_wconst[w].phase_adj = g_pico[w].phase_adj;
			g_wconst[w].pad = 0;
		}
		g_wconst_ready = true;
	}
	return g_wconst;
}

/* ---- the decimator's filter (engine.h: decimator_taps; the one definition every layer and the tests use) ----
 * A Kaiser-windowed sinc with its cutoff at the output rate's Nyquist frequency: for n = 0 .. C,
 *   g[n] = sinc((n - C) / K) * I0(beta * sqrt(1 - ((n - C) / C)^2)) / I0(beta),  sinc(t) = sin(pi t) / (pi t),  beta = 10.06,
 * the upper half mirrored from the lower (not computed again: the symmetry is exact), and h = g / S with S the sum of g in
 * ascending n. All in f64, on the host. */
namespace {

/* the modified Bessel function of order 0 by its power series, until a term no longer changes the sum */
double bessel_i0(double x) {
	const double q = x * x * 0.25;
	double sum = 1.0, term = 1.0;
	for (int k = 1; k < 1000; ++k) {
		term *= q / ((double)k * (double)k);
		const double next = sum + term;
		if (next == sum) break;
		sum = next;
	}
	return sum;
}

} /* namespace */

size_t decimator_latency(int factor) { return factor == 2 || factor == 4 || factor == 8 ? DECIM_HALF : 0; }

/* g[n], n = 0 .. 2C: the Kaiser-windowed sinc with K input frames per lobe, not normalised (g[C] = 1) */
static void kaiser_sinc(size_t K, size_t C, double beta, double *out) {
	const double pi = 3.14159265358979323846, i0b = bessel_i0(beta);
	const size_t L = 2 * C + 1;
	for (size_t n = 0; n <= C; ++n) {
		const double d = (double)n - (double)C; /* n - C */
		const double t = d / (double)K, r = d / (double)C;
		const double sinc = n == C ? 1.0 : sin(pi * t) / (pi * t);
		const double w = 1.0 - r * r;
		out[n] = sinc * bessel_i0(beta * sqrt(w > 0.0 ? w : 0.0)) / i0b;
	}
	for (size_t n = 0; n < C; ++n) out[L - 1 - n] = out[n];
}

size_t decimator_taps(int factor, double *out, size_t cap) {
	if (!decimator_latency(factor)) return 0;
	const size_t K = (size_t)factor, C = DECIM_HALF * K, L = 2 * C + 1;
	if (!out || cap < L) return L;
	kaiser_sinc(K, C, 10.06, out);
	double S = 0.0;
	for (size_t n = 0; n < L; ++n) S += out[n];
	for (size_t n = 0; n < L; ++n) out[n] /= S;
	return L;
}

/* ---- the limiter's constants and smoothing window (engine.h; include/saugns_amd.h, section "Limiter") ----
 * A raised cosine over 2 A + 1 frames that never reaches zero: u[j] = 1 + cos(pi (j - A) / (A + 1)), h = u / S with S the sum
 * of u in ascending j. The upper half is mirrored from the lower (the symmetry is exact). All in f64, on the host. */
size_t limiter_lookahead(uint32_t srate) {
	if (!srate) return 0;
	const uint32_t a = srate / 200;
	return a < LIM_A_MIN ? LIM_A_MIN : a > LIM_A_MAX ? LIM_A_MAX : a;
}

size_t limiter_latency(uint32_t srate) { return srate ? 2 * limiter_lookahead(srate) + 16 : 0; }

size_t limiter_window(uint32_t srate, double *out, size_t cap) {
	if (!srate) return 0;
	const size_t A = limiter_lookahead(srate), W = 2 * A + 1;
	if (!out || cap < W) return W;
	const double pi = 3.14159265358979323846;
	for (size_t j = 0; j <= A; ++j) out[j] = 1.0 + cos(pi * ((double)j - (double)A) / (double)(A + 1));
	for (size_t j = 0; j < A; ++j) out[W - 1 - j] = out[j];
	double S = 0.0;
	for (size_t j = 0; j < W; ++j) S += out[j];
	for (size_t j = 0; j < W; ++j) out[j] /= S;
	return W;
}

/* ---- the spectrum meter's tables and one segment on the host (engine.h; include/saugns_amd.h, section "Spectrum") ----
 * The periodic Hann window and the twiddles of N = 2^L, in f64: the device and the tests' restatement both take them from
 * here, so no comparison depends on two libm's agreeing. spectrum_segment restates one segment of one channel in plain loops,
 * every product rounded and then the sum or difference (the build is -ffp-contract=off): what spec_segment_kernel computes. */
size_t spectrum_window(unsigned log2n, double *out, size_t cap) {
	if (log2n < SPEC_L_MIN || log2n > SPEC_L_MAX) return 0;
	const size_t N = (size_t)1 << log2n;
	if (!out || cap < N) return N;
	const double pi = 3.14159265358979323846;
	for (size_t j = 0; j < N; ++j) out[j] = 0.5 - 0.5 * cos(2.0 * pi * (double)j / (double)N);
	return N;
}

size_t spectrum_twiddles(unsigned log2n, double *out, size_t cap) {
	if (log2n < SPEC_L_MIN || log2n > SPEC_L_MAX) return 0;
	const size_t N = (size_t)1 << log2n;
	if (!out || cap < N) return N;
	const double pi = 3.14159265358979323846;
	for (size_t k = 0; k < N / 2; ++k) {
		out[2 * k] = cos(2.0 * pi * (double)k / (double)N);
		out[2 * k + 1] = -sin(2.0 * pi * (double)k / (double)N);
	}
	return N;
}

bool spectrum_segment(unsigned log2n, const double *w, const double *tw, const float *x, size_t stride, double *re, double *im,
		double *p) {
	if (log2n < SPEC_L_MIN || log2n > SPEC_L_MAX || !w || !tw || !x || !re || !im || !p) return false;
	const size_t N = (size_t)1 << log2n;
	for (size_t j = 0; j < N; ++j) {
		size_t r = 0;
		for (unsigned b = 0; b < log2n; ++b) r |= ((j >> b) & 1) << (log2n - 1 - b);
		uint32_t bits;
		memcpy(&bits, &x[j * stride], sizeof bits);
		const float xf = (bits & 0x7fffffffu) < 0x7f800000u ? x[j * stride] : 0.f; /* (a NaN or +-inf counts as +0.0f) */
		re[r] = w[j] * (double)xf;
		im[r] = 0.0;
	}
	for (unsigned t = 1; t <= log2n; ++t) {
		const size_t m = (size_t)1 << t, h = m / 2, st = N / m;
		for (size_t k0 = 0; k0 < N; k0 += m)
			for (size_t j = 0; j < h; ++j) {
				const size_t a = k0 + j, b = a + h;
				const double c = tw[2 * j * st], d = tw[2 * j * st + 1];
				const double tr = c * re[b] - d * im[b], ti = c * im[b] + d * re[b];
				const double ur = re[a], ui = im[a];
				re[a] = ur + tr; im[a] = ui + ti; re[b] = ur - tr; im[b] = ui - ti;
			}
	}
	for (size_t k = 0; k <= N / 2; ++k) p[k] = re[k] * re[k] + im[k] * im[k];
	return true;
}

/* ---- loudness on the host (engine.h; include/saugns_amd.h states every formula and the order of every operation) ---- */

size_t truepeak_taps(double *out, size_t cap) {
	if (!out || cap < TP_TAPS) return TP_TAPS;
	kaiser_sinc(4, 64, 5.0, out); /* K = 4, H = 16 input frames: C = H * K */
	return TP_TAPS;
}

bool loudness_filter(uint32_t srate, double out[10]) {
	if (srate < LOUD_MIN_RATE || !out) return false;
	const double pi = 3.14159265358979323846, fs = (double)srate;
	{ /* stage 1: high shelf */
		const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
		const double K = tan(pi * f0 / fs), Vh = pow(10.0, G / 20.0), Vb = pow(Vh, 0.4996667741545416), a0 = 1.0 + K / Q + K * K;
		out[0] = (Vh + Vb * K / Q + K * K) / a0;
		out[1] = 2.0 * (K * K - Vh) / a0;
		out[2] = (Vh - Vb * K / Q + K * K) / a0;
		out[3] = 2.0 * (K * K - 1.0) / a0;
		out[4] = (1.0 - K / Q + K * K) / a0;
	}
	{ /* stage 2: high-pass */
		const double f0 = 38.13547087602444, Q = 0.5003270373238773;
		const double K = tan(pi * f0 / fs), a0 = 1.0 + K / Q + K * K;
		out[5] = 1.0; out[6] = -2.0; out[7] = 1.0;
		out[8] = 2.0 * (K * K - 1.0) / a0;
		out[9] = (1.0 - K / Q + K * K) / a0;
	}
	return true;
}

double loudness_step(double st[4], const double f[10], double x) {
	const double u = f[0] * x + st[0];
	st[0] = (f[1] * x - f[3] * u) + st[1];
	st[1] = f[2] * x - f[4] * u;
	const double y = f[5] * u + st[2];
	st[2] = (f[6] * u - f[8] * y) + st[3];
	st[3] = f[7] * u - f[9] * y;
	return y;
}

void loudness_chunk_map(const double f[10], uint32_t chunk, double m[16]) {
	for (int k = 0; k < 4; ++k) {
		double st[4] = {0.0, 0.0, 0.0, 0.0};
		st[k] = 1.0;
		for (uint32_t i = 0; i < chunk; ++i) (void)loudness_step(st, f, 0.0);
		for (int r = 0; r < 4; ++r) m[4 * r + k] = st[r];
	}
}

bool loudness_gate(const double *hops, size_t n_hops, uint32_t hop_frames, int channels, Loudness *out) {
	if (!out || (n_hops && !hops) || !hop_frames || (channels != 1 && channels != 2)) return false;
	const size_t n_blocks = n_hops >= 4 ? n_hops - 3 : 0;
	const double den = 4.0 * (double)hop_frames;
	auto z_of = [&](size_t j) {
		double z = 0.0;
		for (int ch = 0; ch < channels; ++ch) {
			const double *e = hops + 2 * j + ch;
			z = z + (((e[0] + e[2]) + e[4]) + e[6]) / den;
		}
		return z;
	};
	auto lufs = [](double z) { return z > 0.0 ? -0.691 + 10.0 * log10(z) : -HUGE_VAL; };
	double mmax = -HUGE_VAL, sum_abs = 0.0;
	size_t n_abs = 0;
	for (size_t j = 0; j < n_blocks; ++j) {
		const double z = z_of(j), l = lufs(z);
		if (l > mmax) mmax = l;
		if (l > -70.0) { sum_abs += z; ++n_abs; }
	}
	double integrated = -HUGE_VAL;
	size_t n_gated = 0;
	if (n_abs) {
		const double rel = lufs(sum_abs / (double)n_abs) - 10.0;
		double sum = 0.0;
		for (size_t j = 0; j < n_blocks; ++j) {
			const double z = z_of(j), l = lufs(z);
			if (l > -70.0 && l > rel) { sum += z; ++n_gated; }
		}
		if (n_gated) integrated = lufs(sum / (double)n_gated);
	}
	out->frames = (uint64_t)n_hops * hop_frames;
	out->blocks = n_blocks;
	out->gated_blocks = n_gated;
	out->integrated = integrated;
	out->momentary_max = mmax;
	out->true_peak[0] = out->true_peak[1] = 0.f;
	return true;
}

void truepeak_tail(const float *hist, int channels, const double *taps, uint32_t *peak_bits) {
	/* position N + t, t = 0 .. 30: x[N + t - q] is hist frame TP_LEAD + t - q for t - q < 0, else +0 */
	for (int ch = 0; ch < channels; ++ch)
		for (int t = 0; t < (int)TP_LEAD - 1; ++t)
			for (int p = 1; p < 4; ++p) {
				double acc = 0.0;
				for (int q = 0; q < 32; ++q) {
					const int i = (int)TP_LEAD + t - q;
					const double x = i < (int)TP_LEAD ? (double)hist[i * channels + ch] : 0.0;
					acc = acc + taps[4 * q + p] * x;
				}
				const float w = (float)acc;
				uint32_t b;
				memcpy(&b, &w, 4);
				b &= 0x7fffffffu;
				if (b < 0x7f800000u && b > peak_bits[ch]) peak_bits[ch] = b;
			}
}

/* ---- the FLAC encoder on the host (engine.h; include/saugns_amd.h, section "FLAC") ----
 * flac_encode_block restates in plain loops what flac_analyze_kernel and flac_write_kernel (k_flac.h) make of one block, with
 * the arithmetic of sau_flac.h that they use too; flac_header is the 42 bytes ahead of the frames. */
namespace {
struct FlacBits { /* MSB first into bytes that start out cleared */
	uint8_t *p;
	size_t pos = 0;
	void put(uint32_t v, unsigned bits) {
		for (unsigned i = bits; i-- > 0; ++pos)
			if ((v >> i) & 1u) p[pos >> 3] |= (uint8_t)(0x80u >> (pos & 7));
	}
	void zeros(size_t n) { pos += n; }
};
} /* namespace */

size_t flac_header(uint32_t srate, int channels, uint32_t block_frames, const FlacInfo *info, uint8_t *out, size_t cap) {
	using namespace sauflac;
	const uint32_t B = flac_block_frames(block_frames);
	if (!srate || srate > 655350u || (channels != 1 && channels != 2) || !B) return 0;
	if (!out || cap < 42) return 42;
	const uint64_t frames = info ? info->frames : 0;
	const uint32_t mn = info ? info->min_frame_bytes : 0, mx = info ? info->max_frame_bytes : 0;
	memset(out, 0, 42);
	memcpy(out, "fLaC", 4);
	out[4] = 0x80; out[5] = 0; out[6] = 0; out[7] = 34; /* last = 1, type 0, length 34 */
	FlacBits w{out + 8};
	w.put(B, 16); w.put(B, 16);
	w.put(mn & 0xffffffu, 24); w.put(mx & 0xffffffu, 24);
	w.put(srate, 20); w.put((uint32_t)channels - 1, 3); w.put(15, 5);
	w.put((uint32_t)((frames >> 32) & 0xfu), 4); w.put((uint32_t)frames, 32);
	/* (the MD5 stays zeros: not computed) */
	return 42;
}

/* One block of n frames of int32 samples, already checked: B a block size, n in 1 .. B, every sample within `bits`, M the LPC
 * mode's largest order. At 24 bits the LPC mode (the header's "LPC at 24 bits") runs only with lpc24, which
 * flac_encode_block_lpc24 alone sets; without it M is 0 there. */
static size_t flac_encode_block_any(const int32_t *x, uint32_t n, unsigned ch, uint32_t B, uint32_t frame_number, unsigned bits, unsigned M,
		uint8_t *out, size_t cap, bool lpc24 = false) {
	using namespace sauflac;
	const unsigned n_cand = ch == 2 ? 4 : 1, fine_log2 = n == B ? 4 : 0, F = 1u << fine_log2, nk = flac_nk(bits);
	auto at = [&](unsigned c, int64_t i) -> int32_t { return i < 0 ? 0 : ch == 2 ? flac_cand(x[2 * i], x[2 * i + 1], c) : x[i]; };
	auto resid = [&](unsigned c, unsigned o, uint32_t i) { return flac_residual(o, at(c, i), at(c, (int64_t)i - 1), at(c, (int64_t)i - 2), at(c, (int64_t)i - 3), at(c, (int64_t)i - 4)); };
	auto resid_lpc = [&](unsigned c, const int16_t *q, unsigned m, unsigned shift, uint32_t i) { /* (i >= m) */
		if (bits == 24) { /* (the sum is below 2^39 in size, the residual below 2^31 behind step 5b) */
			int64_t sum = 0;
			for (unsigned j = 0; j < m; ++j) sum += (int64_t)q[j] * at(c, (int64_t)i - 1 - j);
			return flac_lpc_residual(at(c, i), sum, shift);
		}
		int32_t sum = 0;
		for (unsigned j = 0; j < m; ++j) sum += (int32_t)q[j] * at(c, (int64_t)i - 1 - j);
		return flac_lpc_residual(at(c, i), sum, shift);
	};
	auto nodes = [&](const uint64_t *fine, unsigned fine_log2, unsigned o, uint64_t *node_cost, uint8_t *node_k) {
		for (unsigned p = 0; p <= fine_log2; ++p)
			for (unsigned j = 0; j < (1u << p); ++j) {
				unsigned k;
				node_cost[flac_node_index(p, j)] = flac_node_cost(fine, nk, fine_log2, p, j, n, o, &k);
				node_k[flac_node_index(p, j)] = (uint8_t)k;
			}
	};
	FlacSub cand[4];
	for (unsigned c = 0; c < n_cand; ++c) {
		bool equal = true;
		for (uint32_t i = 1; i < n; ++i) equal = equal && at(c, i) == at(c, 0);
		uint64_t abs_sum[5] = {0, 0, 0, 0, 0};
		for (uint32_t i = 4; i < n; ++i) {
			int32_t r[5];
			flac_residuals(at(c, i), at(c, i - 1), at(c, i - 2), at(c, i - 3), at(c, i - 4), r);
			for (int o = 0; o < 5; ++o) abs_sum[o] += flac_abs(r[o]);
		}
		const unsigned o = flac_pick_order(n, abs_sum);
		uint64_t fine[FLAC_FINE * flac_nk(24)]; /* [f * nk + k] */
		memset(fine, 0, sizeof fine);
		const uint32_t plen = n / F; /* (F == 1 unless n == B, a multiple of 16) */
		for (uint32_t i = o; i < n; ++i) {
			const uint32_t u = flac_zigzag(resid(c, o, i));
			for (unsigned k = 0; k < nk; ++k) fine[(i / plen) * nk + k] += u >> k;
		}
		uint64_t node_cost[FLAC_NODES];
		uint8_t node_k[FLAC_NODES];
		nodes(fine, fine_log2, o, node_cost, node_k);
		flac_finish_sub(&cand[c], c, n, equal, o, fine_log2, node_cost, node_k, bits);
		if (!M || n != B || equal || (bits == 24 && !lpc24)) continue;
		/* the LPC mode: the windowed autocorrelation in integers, the orders' coefficients, the order, its partitions */
		unsigned log2B = 0;
		while ((1u << log2B) < B) ++log2B;
		int64_t R[FLAC_LPC_MAX + 1];
		for (unsigned l = 0; l <= M; ++l) {
			R[l] = 0;
			for (uint32_t i = l; i < n; ++i)
				R[l] += (int64_t)flac_lpc_windowed(at(c, i), flac_lpc_window(i, B, log2B), bits) * flac_lpc_windowed(at(c, i - l), flac_lpc_window(i - l, B, log2B), bits);
		}
		if (R[0] == 0) continue;
		const unsigned g = flac_lpc_f64_shift(R[0]);
		double r[FLAC_LPC_MAX + 1], a[FLAC_LPC_MAX];
		for (unsigned l = 0; l <= M; ++l) r[l] = (double)(R[l] >> g);
		int16_t q[FLAC_LPC_MAX * FLAC_LPC_MAX];
		uint8_t shift[FLAC_LPC_MAX];
		uint32_t mask = flac_lpc_orders(r, M, a, q, shift);
		if (bits == 24) mask = flac_lpc_guard(mask, q, shift, flac_cand_bps(c, bits)); /* step 5b */
		uint64_t lpc_abs[FLAC_LPC_MAX];
		for (unsigned m = 1; m <= M; ++m) {
			lpc_abs[m - 1] = 0;
			if (mask & (1u << (m - 1)))
				for (uint32_t i = M; i < n; ++i) lpc_abs[m - 1] += flac_abs(resid_lpc(c, q + (m - 1) * FLAC_LPC_MAX, m, shift[m - 1], i));
		}
		const unsigned m = flac_lpc_pick_order(mask, lpc_abs, n, M, flac_cand_bps(c, bits), nk);
		if (!m) continue;
		memset(fine, 0, sizeof fine);
		for (uint32_t i = m; i < n; ++i) {
			const uint32_t u = flac_zigzag(resid_lpc(c, q + (m - 1) * FLAC_LPC_MAX, m, shift[m - 1], i));
			for (unsigned k = 0; k < nk; ++k) fine[(i / plen) * nk + k] += u >> k;
		}
		nodes(fine, fine_log2, m, node_cost, node_k);
		flac_lpc_choose(&cand[c], n, m, q + (m - 1) * FLAC_LPC_MAX, shift[m - 1], fine_log2, node_cost, node_k, bits);
	}
	FlacFrameDesc d;
	flac_finish_frame(&d, cand, ch, n, B, frame_number);
	if (!out || cap < d.bytes) return d.bytes;
	memset(out, 0, d.bytes);
	uint8_t hdr[16];
	const uint32_t hl = flac_frame_header(n, B, d.assign, frame_number, bits, hdr);
	memcpy(out, hdr, hl);
	FlacBits bw{out, (size_t)hl * 8};
	for (unsigned si = 0; si < d.n_sub; ++si) {
		const FlacSub &s = d.sub[si];
		const unsigned c = s.cand, bps = flac_cand_bps(c, bits);
		const uint32_t mask = (1u << bps) - 1;
		bw.put(s.type == FLAC_CONSTANT ? 0u : s.type == FLAC_VERBATIM ? 2u : s.type == FLAC_LPC ? (uint32_t)(0x40u | ((s.order - 1u) << 1)) :
				(uint32_t)(0x10u | (s.order << 1)), 8); /* 0 tttttt 0 */
		if (s.type == FLAC_CONSTANT) bw.put((uint32_t)at(c, 0) & mask, bps);
		else if (s.type == FLAC_VERBATIM) for (uint32_t i = 0; i < n; ++i) bw.put((uint32_t)at(c, i) & mask, bps);
		else {
			for (uint32_t i = 0; i < s.order; ++i) bw.put((uint32_t)at(c, i) & mask, bps);
			if (s.type == FLAC_LPC) {
				bw.put(FLAC_LPC_PREC - 1, 4);
				bw.put(s.shift, 5);
				for (uint32_t i = 0; i < s.order; ++i) bw.put((uint32_t)s.q[i] & 0xfffu, FLAC_LPC_PREC);
			}
			bw.put((bits == 24 ? 0x10u : 0u) | s.p, 6); /* 00 pppp, or 01 pppp where the parameters take five bits */
			const uint32_t plen = n >> s.p;
			for (uint32_t j = 0; j < (1u << s.p); ++j) {
				const unsigned k = s.k[j];
				bw.put(k, flac_k_width(bits));
				for (uint32_t i = j ? j * plen : s.order; i < (j + 1) * plen; ++i) {
					const uint32_t u = flac_zigzag(s.type == FLAC_LPC ? resid_lpc(c, s.q, s.order, s.shift, i) : resid(c, s.order, i));
					bw.zeros(u >> k);
					bw.put((1u << k) | (u & ((1u << k) - 1)), k + 1);
				}
			}
		}
	}
	const size_t body = (bw.pos + 7) / 8;
	if (body + 2 != d.bytes) return 0; /* (the analysis and the writer disagree: never) */
	uint32_t crc = 0;
	for (size_t i = 0; i < body; ++i) crc = flac_crc16_update(crc, out[i]);
	out[body] = (uint8_t)(crc >> 8); out[body + 1] = (uint8_t)crc;
	return d.bytes;
}

size_t flac_encode_block(const int16_t *x, uint32_t n, int channels, uint32_t block_frames, uint32_t frame_number, uint8_t *out, size_t cap) {
	return flac_encode_block_lpc(x, n, channels, block_frames, frame_number, 0, out, cap);
}

size_t flac_encode_block_lpc(const int16_t *x, uint32_t n, int channels, uint32_t block_frames, uint32_t frame_number, uint32_t max_lpc_order,
		uint8_t *out, size_t cap) {
	using namespace sauflac;
	const uint32_t B = flac_block_frames(block_frames);
	if (!x || !B || !n || n > B || (channels != 1 && channels != 2) || frame_number > FLAC_MAX_BLOCKS || max_lpc_order > FLAC_LPC_MAX) return 0;
	const std::vector<int32_t> s(x, x + (size_t)n * (size_t)channels);
	return flac_encode_block_any(s.data(), n, (unsigned)channels, B, frame_number, 16, max_lpc_order, out, cap);
}

/* ---- 24 bits and float-fed encoders (include/saugns_amd.h, FLAC, "24 bits") ---- */
size_t flac_header_bits(uint32_t srate, int channels, uint32_t block_frames, int bits, const FlacInfo *info, uint8_t *out, size_t cap) {
	if (!sauflac::flac_bits_ok(bits)) return 0;
	const size_t got = flac_header(srate, channels, block_frames, info, out, cap);
	if (got == 42 && out && cap >= 42 && bits == 24) { /* bits per sample - 1: the low bit of byte 20, the high nibble of byte 21 */
		out[20] = (uint8_t)((out[20] & 0xfeu) | (23u >> 4));
		out[21] = (uint8_t)((out[21] & 0x0fu) | ((23u & 0xfu) << 4));
	}
	return got;
}

bool flac_quantize(const float *x, size_t n, float gain, int bits, int32_t *out) {
	if (!sauflac::flac_bits_ok(bits) || (n && (!x || !out))) return false;
	for (size_t i = 0; i < n; ++i) {
		const float y = x[i] * gain; /* one f32 multiply, as flac_quant_kernel's */
		out[i] = bits == 24 ? saudev::pcm24(y) : (int32_t)saudev::pcm16(y);
	}
	return true;
}

/* ---- MD5 (include/saugns_amd.h, FLAC, "MD5"): what flac_md5_kernel makes of a stream's samples, with sau_md5.h's steps ---- */
size_t flac_header_md5(uint32_t srate, int channels, uint32_t block_frames, int bits, const FlacInfo *info, const uint8_t md5[16],
		uint8_t *out, size_t cap) {
	const size_t got = flac_header_bits(srate, channels, block_frames, bits, info, out, cap);
	if (got == 42 && out && cap >= 42 && md5) memcpy(out + 26, md5, 16);
	return got;
}

bool flac_md5(const int32_t *x, size_t n, int bits, uint8_t out[16]) {
	using namespace saumd5;
	if (!sauflac::flac_bits_ok(bits) || !out || (n && !x)) return false;
	const int32_t lo = bits == 24 ? -(1 << 23) : -32768, hi = bits == 24 ? (1 << 23) - 1 : 32767;
	for (size_t i = 0; i < n; ++i)
		if (x[i] < lo || x[i] > hi) return false;
	const auto at = [x](unsigned long long i) -> int32_t { return x[i]; };
	const unsigned long long total = (unsigned long long)n * (bits == 24 ? 3 : 2), whole = total / 64;
	uint32_t s[4], w[16];
	md5_init(s);
	for (unsigned long long c = 0; c <= whole; ++c) { /* the last round: what is left, and the padding */
		for (unsigned k = 0; k < 16; ++k) w[k] = bits == 24 ? md5_word24(at, 16 * c + k, n) : md5_word16(at, 16 * c + k, n);
		if (c < whole) md5_chunk(s, w);
		else md5_finish(s, w, total);
	}
	md5_digest(s, out);
	return true;
}

size_t flac_encode_block_s32(const int32_t *x, uint32_t n, int channels, uint32_t block_frames, uint32_t frame_number, int bits,
		uint32_t max_lpc_order, uint8_t *out, size_t cap) {
	using namespace sauflac;
	const uint32_t B = flac_block_frames(block_frames);
	if (!x || !B || !n || n > B || (channels != 1 && channels != 2) || frame_number > FLAC_MAX_BLOCKS || !flac_bits_ok(bits) ||
	    max_lpc_order > FLAC_LPC_MAX || (bits == 24 && max_lpc_order)) return 0;
	const size_t cnt = (size_t)n * (size_t)channels;
	const int32_t lo = bits == 24 ? FLAC_S24_MIN : -32768, hi = bits == 24 ? FLAC_S24_MAX : 32767;
	for (size_t i = 0; i < cnt; ++i)
		if (x[i] < lo || x[i] > hi) return 0;
	return flac_encode_block_any(x, n, (unsigned)channels, B, frame_number, (unsigned)bits, max_lpc_order, out, cap);
}

/* LPC at 24 bits: the one entry point that runs flac_encode_block_any's LPC mode on 24-bit samples; flac_encode_block_s32 keeps
 * refusing (24, M > 0) */
size_t flac_encode_block_lpc24(const int32_t *x, uint32_t n, int channels, uint32_t block_frames, uint32_t frame_number, uint32_t max_lpc_order,
		uint8_t *out, size_t cap) {
	using namespace sauflac;
	const uint32_t B = flac_block_frames(block_frames);
	if (!x || !B || !n || n > B || (channels != 1 && channels != 2) || frame_number > FLAC_MAX_BLOCKS || max_lpc_order > FLAC_LPC_MAX) return 0;
	const size_t cnt = (size_t)n * (size_t)channels;
	for (size_t i = 0; i < cnt; ++i)
		if (x[i] < FLAC_S24_MIN || x[i] > FLAC_S24_MAX) return 0;
	return flac_encode_block_any(x, n, (unsigned)channels, B, frame_number, 24, max_lpc_order, out, cap, true);
}

/* ---- the decoder (include/saugns_amd.h, FLAC, "Verify"; the arithmetic is sau_flac_dec.h's, which flac_decode_kernel uses
 * too): the one frame that begins at data ---- */
size_t flac_decode_block(const uint8_t *data, size_t len, int channels, uint32_t block_frames, int bits, uint32_t frame_number, int32_t *out,
		size_t cap_frames, uint32_t *n_out, int *status_out) {
	using namespace sauflac;
	const uint32_t B = flac_block_frames(block_frames);
	if (n_out) *n_out = 0;
	if (!status_out) return 0;
	*status_out = FLAC_DEC_BAD_ARGUMENT;
	if ((len && !data) || !B || (channels != 1 && channels != 2) || !flac_bits_ok(bits) || frame_number > FLAC_MAX_BLOCKS || !n_out ||
	    (cap_frames && !out)) return 0;
	std::vector<int32_t> ch((size_t)B * 2);
	FlacDecFrame f;
	/* (one pass: flac_decode_frame writes no frame at or behind cap_frames, and nothing is promised about out on a failure) */
	const int st = flac_decode_frame(data, len, (uint32_t)channels, B, (unsigned)bits, frame_number, ch.data(), ch.data() + B, &f, out, cap_frames);
	if (st == FLAC_DEC_OK && cap_frames < f.n) return 0;
	*status_out = st;
	if (st != FLAC_DEC_OK) return 0;
	*n_out = f.n;
	return f.bytes;
}

/* ---- dither and noise shaping (include/saugns_amd.h, section "Dither and noise shaping"; the arithmetic is sau_dither.h's,
 * which the kernels use too): what a quantiser makes of one row's frames [first_frame, first_frame + frames) ---- */
bool dither_quantize(const float *x, size_t frames, int channels, float gain, const saudither::DitherSpec *spec, uint64_t row,
		uint64_t first_frame, double *history, int16_t *out, uint64_t *clipped) {
	using namespace saudither;
	if ((channels != 1 && channels != 2) || !spec || !dither_spec_ok(*spec) || !(gain >= -FLT_MAX && gain <= FLT_MAX) ||
	    (frames && (!x || !out))) return false;
	if (clipped) clipped[0] = clipped[1] = 0;
	const unsigned ch = (unsigned)channels, T = spec->taps;
	if (dither_spec_plain(*spec)) { /* the existing rounding: nothing is clamped after it, and no state moves */
		for (size_t i = 0; i < frames * ch; ++i) out[i] = saudev::pcm16(x[i] * gain);
		return true;
	}
	const uint64_t seed_r = dither_row_seed(spec->seed, row);
	for (unsigned c = 0; c < ch; ++c) {
		double e[DITHER_TAPS_MAX] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
		if (history) memcpy(e, history + (size_t)c * DITHER_TAPS_MAX, sizeof e);
		uint64_t clips = 0;
		for (size_t i = 0; i < frames; ++i) {
			const double s = dither_lsb(dither_scale(x[i * ch + c], gain));
			const float d = spec->dither ? dither_tpdf(seed_r, first_frame + i, c) : 0.f;
			bool cl;
			out[i * ch + c] = (int16_t)dither_step(spec->coef, T, e, s, d, cl);
			clips += cl ? 1 : 0;
		}
		if (history) memcpy(history + (size_t)c * DITHER_TAPS_MAX, e, sizeof e);
		if (clipped) clipped[c] = clips;
	}
	return true;
}

} /* namespace sauengine */
