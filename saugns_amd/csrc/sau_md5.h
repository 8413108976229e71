/* sau_md5.h -- the MD5 (RFC 1321) of a FLAC stream's unencoded samples (RFC 9639 section 8.2; include/saugns_amd.h, section
 * "FLAC", paragraph "MD5"), shared by the host restatement (tables.cpp: flac_md5) and the kernels (k_md5.h) the way sau_flac.h
 * is: the initial state, one chunk of 16 message words, how samples become message words, and the final padding. All of it is
 * 32-bit integer arithmetic, so host and device agree by construction; what differs between them is only who fetches the
 * samples. The message is the samples in stream order, channels interleaved, each as a signed little-endian integer of 2
 * bytes (16 bits per sample) or 3 bytes (24). */
#ifndef SAU_MD5_H
#define SAU_MD5_H
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SAU_MD5_HD __host__ __device__ inline
#else
#define SAU_MD5_HD static inline
#endif

namespace saumd5 {

constexpr uint32_t MD5_A0 = 0x67452301u, MD5_B0 = 0xefcdab89u, MD5_C0 = 0x98badcfeu, MD5_D0 = 0x10325476u;

SAU_MD5_HD void md5_init(uint32_t s[4]) { s[0] = MD5_A0; s[1] = MD5_B0; s[2] = MD5_C0; s[3] = MD5_D0; }

SAU_MD5_HD uint32_t md5_rotl(uint32_t x, unsigned s) { return (x << s) | (x >> (32u - s)); }

/* One step: a = b + ((a + f(b, c, d) + w + t) <<< s). Every caller passes the word and the literals t and s of its step, so
 * the word index and the rotate count are compile-time constants: nothing here indexes registers at run time. */
#define SAU_MD5_FF(b, c, d) (((b) & (c)) | (~(b) & (d)))
#define SAU_MD5_GG(b, c, d) (((d) & (b)) | (~(d) & (c)))
#define SAU_MD5_HH(b, c, d) ((b) ^ (c) ^ (d))
#define SAU_MD5_II(b, c, d) ((c) ^ ((b) | ~(d)))
#define SAU_MD5_STEP(f, a, b, c, d, k, s, t) a = b + md5_rotl(a + f(b, c, d) + w[k] + (uint32_t)(t), s)

/* the 64 steps over the chunk w[16], added into state[4] */
SAU_MD5_HD void md5_chunk(uint32_t state[4], const uint32_t w[16]) {
	uint32_t a = state[0], b = state[1], c = state[2], d = state[3];
	SAU_MD5_STEP(SAU_MD5_FF, a, b, c, d,  0,  7, 0xd76aa478u); SAU_MD5_STEP(SAU_MD5_FF, d, a, b, c,  1, 12, 0xe8c7b756u);
	SAU_MD5_STEP(SAU_MD5_FF, c, d, a, b,  2, 17, 0x242070dbu); SAU_MD5_STEP(SAU_MD5_FF, b, c, d, a,  3, 22, 0xc1bdceeeu);
	SAU_MD5_STEP(SAU_MD5_FF, a, b, c, d,  4,  7, 0xf57c0fafu); SAU_MD5_STEP(SAU_MD5_FF, d, a, b, c,  5, 12, 0x4787c62au);
	SAU_MD5_STEP(SAU_MD5_FF, c, d, a, b,  6, 17, 0xa8304613u); SAU_MD5_STEP(SAU_MD5_FF, b, c, d, a,  7, 22, 0xfd469501u);
	SAU_MD5_STEP(SAU_MD5_FF, a, b, c, d,  8,  7, 0x698098d8u); SAU_MD5_STEP(SAU_MD5_FF, d, a, b, c,  9, 12, 0x8b44f7afu);
	SAU_MD5_STEP(SAU_MD5_FF, c, d, a, b, 10, 17, 0xffff5bb1u); SAU_MD5_STEP(SAU_MD5_FF, b, c, d, a, 11, 22, 0x895cd7beu);
	SAU_MD5_STEP(SAU_MD5_FF, a, b, c, d, 12,  7, 0x6b901122u); SAU_MD5_STEP(SAU_MD5_FF, d, a, b, c, 13, 12, 0xfd987193u);
	SAU_MD5_STEP(SAU_MD5_FF, c, d, a, b, 14, 17, 0xa679438eu); SAU_MD5_STEP(SAU_MD5_FF, b, c, d, a, 15, 22, 0x49b40821u);

	SAU_MD5_STEP(SAU_MD5_GG, a, b, c, d,  1,  5, 0xf61e2562u); SAU_MD5_STEP(SAU_MD5_GG, d, a, b, c,  6,  9, 0xc040b340u);
	SAU_MD5_STEP(SAU_MD5_GG, c, d, a, b, 11, 14, 0x265e5a51u); SAU_MD5_STEP(SAU_MD5_GG, b, c, d, a,  0, 20, 0xe9b6c7aau);
	SAU_MD5_STEP(SAU_MD5_GG, a, b, c, d,  5,  5, 0xd62f105du); SAU_MD5_STEP(SAU_MD5_GG, d, a, b, c, 10,  9, 0x02441453u);
	SAU_MD5_STEP(SAU_MD5_GG, c, d, a, b, 15, 14, 0xd8a1e681u); SAU_MD5_STEP(SAU_MD5_GG, b, c, d, a,  4, 20, 0xe7d3fbc8u);
	SAU_MD5_STEP(SAU_MD5_GG, a, b, c, d,  9,  5, 0x21e1cde6u); SAU_MD5_STEP(SAU_MD5_GG, d, a, b, c, 14,  9, 0xc33707d6u);
	SAU_MD5_STEP(SAU_MD5_GG, c, d, a, b,  3, 14, 0xf4d50d87u); SAU_MD5_STEP(SAU_MD5_GG, b, c, d, a,  8, 20, 0x455a14edu);
	SAU_MD5_STEP(SAU_MD5_GG, a, b, c, d, 13,  5, 0xa9e3e905u); SAU_MD5_STEP(SAU_MD5_GG, d, a, b, c,  2,  9, 0xfcefa3f8u);
	SAU_MD5_STEP(SAU_MD5_GG, c, d, a, b,  7, 14, 0x676f02d9u); SAU_MD5_STEP(SAU_MD5_GG, b, c, d, a, 12, 20, 0x8d2a4c8au);

	SAU_MD5_STEP(SAU_MD5_HH, a, b, c, d,  5,  4, 0xfffa3942u); SAU_MD5_STEP(SAU_MD5_HH, d, a, b, c,  8, 11, 0x8771f681u);
	SAU_MD5_STEP(SAU_MD5_HH, c, d, a, b, 11, 16, 0x6d9d6122u); SAU_MD5_STEP(SAU_MD5_HH, b, c, d, a, 14, 23, 0xfde5380cu);
	SAU_MD5_STEP(SAU_MD5_HH, a, b, c, d,  1,  4, 0xa4beea44u); SAU_MD5_STEP(SAU_MD5_HH, d, a, b, c,  4, 11, 0x4bdecfa9u);
	SAU_MD5_STEP(SAU_MD5_HH, c, d, a, b,  7, 16, 0xf6bb4b60u); SAU_MD5_STEP(SAU_MD5_HH, b, c, d, a, 10, 23, 0xbebfbc70u);
	SAU_MD5_STEP(SAU_MD5_HH, a, b, c, d, 13,  4, 0x289b7ec6u); SAU_MD5_STEP(SAU_MD5_HH, d, a, b, c,  0, 11, 0xeaa127fau);
	SAU_MD5_STEP(SAU_MD5_HH, c, d, a, b,  3, 16, 0xd4ef3085u); SAU_MD5_STEP(SAU_MD5_HH, b, c, d, a,  6, 23, 0x04881d05u);
	SAU_MD5_STEP(SAU_MD5_HH, a, b, c, d,  9,  4, 0xd9d4d039u); SAU_MD5_STEP(SAU_MD5_HH, d, a, b, c, 12, 11, 0xe6db99e5u);
	SAU_MD5_STEP(SAU_MD5_HH, c, d, a, b, 15, 16, 0x1fa27cf8u); SAU_MD5_STEP(SAU_MD5_HH, b, c, d, a,  2, 23, 0xc4ac5665u);

	SAU_MD5_STEP(SAU_MD5_II, a, b, c, d,  0,  6, 0xf4292244u); SAU_MD5_STEP(SAU_MD5_II, d, a, b, c,  7, 10, 0x432aff97u);
	SAU_MD5_STEP(SAU_MD5_II, c, d, a, b, 14, 15, 0xab9423a7u); SAU_MD5_STEP(SAU_MD5_II, b, c, d, a,  5, 21, 0xfc93a039u);
	SAU_MD5_STEP(SAU_MD5_II, a, b, c, d, 12,  6, 0x655b59c3u); SAU_MD5_STEP(SAU_MD5_II, d, a, b, c,  3, 10, 0x8f0ccc92u);
	SAU_MD5_STEP(SAU_MD5_II, c, d, a, b, 10, 15, 0xffeff47du); SAU_MD5_STEP(SAU_MD5_II, b, c, d, a,  1, 21, 0x85845dd1u);
	SAU_MD5_STEP(SAU_MD5_II, a, b, c, d,  8,  6, 0x6fa87e4fu); SAU_MD5_STEP(SAU_MD5_II, d, a, b, c, 15, 10, 0xfe2ce6e0u);
	SAU_MD5_STEP(SAU_MD5_II, c, d, a, b,  6, 15, 0xa3014314u); SAU_MD5_STEP(SAU_MD5_II, b, c, d, a, 13, 21, 0x4e0811a1u);
	SAU_MD5_STEP(SAU_MD5_II, a, b, c, d,  4,  6, 0xf7537e82u); SAU_MD5_STEP(SAU_MD5_II, d, a, b, c, 11, 10, 0xbd3af235u);
	SAU_MD5_STEP(SAU_MD5_II, c, d, a, b,  2, 15, 0x2ad7d2bbu); SAU_MD5_STEP(SAU_MD5_II, b, c, d, a,  9, 21, 0xeb86d391u);
	state[0] += a; state[1] += b; state[2] += c; state[3] += d;
}
#undef SAU_MD5_STEP
#undef SAU_MD5_FF
#undef SAU_MD5_GG
#undef SAU_MD5_HH
#undef SAU_MD5_II

/* Message word `w` of a sequence of samples, counted from the sequence's first sample; `at(i)` gives sample i as an int32
 * and is asked only for i < n, the others count as zero bytes. 16 bits: the samples 2w and 2w + 1. 24 bits: the word covers
 * the bytes 4w .. 4w + 3, which begin 4w mod 3 bytes into sample 4w / 3 and end in the next one. */
template <class At>
SAU_MD5_HD uint32_t md5_word16(const At &at, unsigned long long w, unsigned long long n) {
	const unsigned long long i = 2 * w;
	const uint32_t lo = i < n ? (uint32_t)at(i) & 0xffffu : 0u, hi = i + 1 < n ? (uint32_t)at(i + 1) & 0xffffu : 0u;
	return lo | (hi << 16);
}
template <class At>
SAU_MD5_HD uint32_t md5_word24(const At &at, unsigned long long w, unsigned long long n) {
	const unsigned long long i = (4 * w) / 3;
	const unsigned off = (unsigned)((4 * w) % 3);
	const uint64_t lo = i < n ? (uint32_t)at(i) & 0xffffffu : 0u, hi = i + 1 < n ? (uint32_t)at(i + 1) & 0xffffffu : 0u;
	return (uint32_t)((lo | (hi << 24)) >> (8 * off));
}

/* The end of a message of `total` bytes, of which the last total mod 64 lie in w[16] with zeros behind them: the byte 0x80,
 * zeros and the length in bits as 64 bits, low word first. One chunk when total mod 64 < 56, else two. */
SAU_MD5_HD void md5_finish(uint32_t state[4], uint32_t w[16], unsigned long long total) {
	const unsigned used = (unsigned)(total & 63u);
	const unsigned long long bits = total << 3;
	/* (a select per word in place of w[used >> 2] |= ...: no run-time index) */
	for (unsigned k = 0; k < 16; ++k) w[k] |= (used >> 2) == k ? 0x80u << (8 * (used & 3u)) : 0u;
	if (used >= 56) {
		md5_chunk(state, w);
		for (unsigned k = 0; k < 14; ++k) w[k] = 0;
	}
	w[14] = (uint32_t)bits; w[15] = (uint32_t)(bits >> 32);
	md5_chunk(state, w);
}

/* the digest's 16 bytes: the state's words, low byte first */
SAU_MD5_HD void md5_digest(const uint32_t state[4], uint8_t out[16]) {
	for (unsigned i = 0; i < 16; ++i) out[i] = (uint8_t)(state[i >> 2] >> (8 * (i & 3u)));
}

} /* namespace saumd5 */
#endif
