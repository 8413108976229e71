/* TEST INFRASTRUCTURE: the FLAC decoder's arithmetic (saugns_amd/csrc/sau_flac_dec.h over sau_flac.h, host code only) under
 * -fsanitize=address,undefined, as a program of its own (tests/test_flac_verify_sanitize.py builds and runs it once). The same
 * source is what flac_decode_kernel runs, so this is where its reader is shown to be bounded.
 *   main FILE   FILE holds records: u32 channels, B, bits, number, flips (0 or 1), len, then len bytes -- valid frames that the
 *               library's encoders made. For each: the frame decodes; every proper prefix (without flips: every 61st) gives LENGTH;
 *               with flips, every single flipped bit gives a status other than OK; then seeded random mutations of it, and at the end seeded random byte
 *               strings under every (channels, B, bits). Every input sits in a heap buffer of exactly its length, and so do the
 *               channel arrays (B samples each), so a read or a write one byte out is the sanitizer's to report.
 * Exit status 0 and a line of counts, or a message and 2 .. 5 for a wrong status; the sanitizers abort on their own findings. */
#include "../../saugns_amd/csrc/sau_flac_dec.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

using namespace sauflac;

static unsigned long long g_decodes = 0;
static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() { /* xorshift64* */
	g_rng ^= g_rng >> 12; g_rng ^= g_rng << 25; g_rng ^= g_rng >> 27;
	return (uint32_t)((g_rng * 0x2545f4914f6cdd1dull) >> 32);
}

/* one decode of exactly `len` bytes from a heap buffer of that size */
static int decode(const uint8_t *src, size_t len, uint32_t channels, uint32_t B, unsigned bits, uint32_t number, uint32_t *n_out) {
	uint8_t *buf = (uint8_t *)malloc(len ? len : 1);
	if (len) memcpy(buf, src, len);
	if (!len) { free(buf); buf = (uint8_t *)malloc(0); } /* (a buffer with no byte to read) */
	int32_t *ch0 = (int32_t *)malloc(B * sizeof(int32_t)), *ch1 = (int32_t *)malloc(B * sizeof(int32_t));
	int32_t *out = (int32_t *)malloc((size_t)B * channels * sizeof(int32_t));
	FlacDecFrame f;
	const int st = flac_decode_frame(buf, len, channels, B, bits, number, ch0, ch1, &f, out, B);
	if (n_out) *n_out = f.n;
	free(out); free(ch1); free(ch0); free(buf);
	++g_decodes;
	return st;
}

int main(int argc, char **argv) {
	if (argc < 2) { fprintf(stderr, "usage: %s FILE\n", argv[0]); return 1; }
	FILE *fp = fopen(argv[1], "rb");
	if (!fp) { fprintf(stderr, "cannot open %s\n", argv[1]); return 1; }
	unsigned frames = 0;
	for (;;) {
		uint32_t h[6];
		if (fread(h, 4, 6, fp) != 6) break;
		const uint32_t channels = h[0], B = h[1], bits = h[2], number = h[3], flips = h[4], len = h[5];
		if ((channels != 1 && channels != 2) || !flac_block_frames(B) || B != flac_block_frames(B) || !flac_bits_ok((int)bits) || len > (1u << 20)) {
			fprintf(stderr, "bad record\n"); return 1;
		}
		std::vector<uint8_t> fr(len);
		if (len && fread(fr.data(), 1, len, fp) != len) { fprintf(stderr, "short record\n"); return 1; }
		++frames;
		uint32_t n = 0;
		if (decode(fr.data(), len, channels, B, bits, number, &n) != FLAC_DEC_OK) { fprintf(stderr, "frame %u does not decode\n", frames); return 2; }
		for (uint32_t cut = 0; cut < len; cut += flips ? 1 : 61) { /* (a long frame without flips: a sample of its prefixes) */
			const int st = decode(fr.data(), cut, channels, B, bits, number, nullptr);
			if (st != FLAC_DEC_LENGTH) { fprintf(stderr, "frame %u cut at %u: status %d, not LENGTH\n", frames, cut, st); return 3; }
		}
		if (flips)
			for (uint32_t bit = 0; bit < 8 * len; ++bit) {
				fr[bit >> 3] ^= (uint8_t)(0x80u >> (bit & 7));
				const int st = decode(fr.data(), len, channels, B, bits, number, nullptr);
				fr[bit >> 3] ^= (uint8_t)(0x80u >> (bit & 7));
				if (st == FLAC_DEC_OK) { fprintf(stderr, "frame %u with bit %u flipped decodes\n", frames, bit); return 4; }
			}
		/* mutations: a few bytes replaced, sometimes the length changed too; any status will do */
		for (unsigned t = 0; t < 300; ++t) {
			std::vector<uint8_t> m(fr);
			const unsigned changes = 1 + rnd() % 4;
			for (unsigned c = 0; c < changes && !m.empty(); ++c) m[rnd() % m.size()] = (uint8_t)rnd();
			if (rnd() % 4 == 0) m.resize(rnd() % (m.size() + 1));
			(void)decode(m.data(), m.size(), channels, B, bits, rnd() % 3 ? number : rnd(), nullptr);
		}
	}
	fclose(fp);
	if (!frames) { fprintf(stderr, "no frames\n"); return 5; }
	/* random byte strings, half of them behind a plausible start so that the subframes are reached */
	static const uint32_t Bs[5] = {256, 512, 1024, 2048, 4096};
	for (unsigned t = 0; t < 6000; ++t) {
		const uint32_t channels = 1 + rnd() % 2, B = Bs[rnd() % 5], bits = rnd() % 2 ? 24 : 16, number = rnd() % 200;
		std::vector<uint8_t> m(rnd() % 400);
		for (size_t i = 0; i < m.size(); ++i) m[i] = (uint8_t)(rnd() % 3 ? rnd() : 0);
		if (t % 2 == 0) {
			uint8_t head[16];
			const uint32_t n = t % 4 ? B : 1 + rnd() % 255;
			static const uint32_t as[4] = {1, 8, 9, 10};
			const uint32_t hl = flac_frame_header(n, B, channels == 1 ? 0 : as[rnd() % 4], number, bits, head);
			for (uint32_t i = 0; i < hl && i < m.size(); ++i) m[i] = head[i];
		}
		(void)decode(m.data(), m.size(), channels, B, bits, number, nullptr);
	}
	printf("ok: %u frames, %llu decodes\n", frames, g_decodes);
	return 0;
}
