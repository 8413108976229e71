/* sau_flac_dec.h -- the FLAC decoder's arithmetic (include/saugns_amd.h, section "FLAC", paragraph "Verify"), shared by the host
 * restatement (tables.cpp: flac_decode_block) and the kernel (k_flac_dec.h) the way sau_flac.h is shared by the encoders: a
 * bounded bit reader, the frame header, the subframes, the inverses of the zigzag, of the FIXED and LPC residuals and of the
 * stereo assignments, the padding and the range check. It decodes exactly the frames this library's encoders can emit and
 * refuses everything else. Host and device run the same statements on the same bytes, so they agree on the status as well as
 * on the samples; what differs between them is only who walks the data-parallel parts.
 *
 * The statuses, one enum (FlacDecStatus). The checks run in stream order and the first failure wins:
 *   OK
 *   LENGTH    the data ends inside the frame: any read behind `len`, the two CRC-16 bytes included. Only the first
 *             flac_frame_bound(B, channels, bits) bytes are ever looked at -- no frame of these encoders is longer --, so a
 *             frame that would run on behind them ends in LENGTH too.
 *   SYNC      the first two bytes are not FF F8.
 *   HEADER    the block size code is not 0111 and not the code of B; the sample rate code is not 0000; the channel assignment is
 *             not one of 0, 1, 8, 9, 10 or does not go with `channels` (0 with 1; the others with 2); the sample size code is not
 *             that of `bits` (100, 110); the reserved bit; and, behind the number, a code 0111 whose n is not below B.
 *   NUMBER    the frame number: a lead byte 10xxxxxx or 1111111x, a continuation byte that is not 10xxxxxx, a form longer than
 *             the shortest, or a number other than the expected one.
 *   CRC8      the header's CRC-8.
 *   SUBFRAME  per subframe: the padding bit; a type other than CONSTANT, VERBATIM, FIXED of order 0 .. 4 or LPC of order 1 .. 8,
 *             a FIXED order above n, an LPC subframe in a block with n != B; the wasted-bits flag; behind an LPC subframe's
 *             warm-up samples a precision field other than 1011 or a negative shift (the five bits hold 0 .. 15 otherwise).
 *   RESIDUAL  the coding method is not the width's own (00 at 16 bits, 01 at 24); a partition order above 4, or above 0 where
 *             n != B; a Rice parameter above 14 (16 bits, four bits each) or 30 (24 bits, five bits each), the escape among
 *             them; a code whose u does not fit 32 bits.
 *   PADDING   a bit between the last subframe and the next byte boundary is not 0.
 *   CRC16     the frame's CRC-16.
 *   RANGE     a restored L or R (or the one channel) does not fit `bits`.
 *   MISMATCH  verify only: the frame decoded, but not to the block's samples, length or size.
 * FLAC_DEC_BAD_ARGUMENT stands outside that list, for the host entry point's argument checks.
 *
 * Memory safety. FlacBits knows the bits it may read, and every read goes through flac_dec_read, flac_dec_unary or -- behind a
 * check of the whole run -- flac_dec_peek; no byte at or behind `len` is ever touched. Every loop advances the position or a
 * counter bounded by n <= B: the unary run of a Rice code ends at the frame's last bit at the latest. Samples are written at
 * indices below n only, and n <= B is settled by the header before any subframe is read. Restoration is done in unsigned
 * arithmetic (it wraps, as a corrupt frame may make it), so no input has undefined behaviour. */
#ifndef SAU_FLAC_DEC_H
#define SAU_FLAC_DEC_H
#include "sau_flac.h"

namespace sauflac {

enum FlacDecStatus : int {
	FLAC_DEC_OK = 0, FLAC_DEC_LENGTH = 1, FLAC_DEC_SYNC = 2, FLAC_DEC_HEADER = 3, FLAC_DEC_NUMBER = 4, FLAC_DEC_CRC8 = 5,
	FLAC_DEC_SUBFRAME = 6, FLAC_DEC_RESIDUAL = 7, FLAC_DEC_PADDING = 8, FLAC_DEC_CRC16 = 9, FLAC_DEC_RANGE = 10,
	FLAC_DEC_MISMATCH = 11, FLAC_DEC_BAD_ARGUMENT = 255
};

/* ---- the bit reader: MSB first over (p, bits / 8 bytes); pos <= bits always ---- */
struct FlacBits {
	const uint8_t *p;
	uint32_t bits;   /* 8 * len: at most 8 * flac_frame_bound(4096, 2, 24) */
	uint32_t pos;
};
SAU_FLAC_HD FlacBits flac_dec_bits(const uint8_t *p, uint64_t len, uint32_t channels, uint32_t B, unsigned bits) {
	const uint32_t bound = flac_frame_bound(B, channels, bits);
	FlacBits r;
	r.p = p; r.bits = 8 * (len < bound ? (uint32_t)len : bound); r.pos = 0;
	return r;
}
/* w (1 .. 32) bits at pos; the caller has seen that pos + w <= r.bits, so only bytes below len are loaded */
SAU_FLAC_HD uint32_t flac_dec_peek(const FlacBits &r, uint32_t pos, unsigned w) {
	const uint32_t b0 = pos >> 3, sh = pos & 7u, nb = (sh + w + 7) >> 3; /* at most 5 bytes */
	uint64_t x = 0;
	for (uint32_t i = 0; i < nb; ++i) x = (x << 8) | r.p[b0 + i];
	return (uint32_t)((x >> (8 * nb - sh - w)) & ((1ull << w) - 1));
}
/* w (0 .. 32) bits; false, and nothing moves, where they are not all there */
SAU_FLAC_HD bool flac_dec_read(FlacBits &r, unsigned w, uint32_t *v) {
	if (w > r.bits - r.pos) return false;
	*v = w ? flac_dec_peek(r, r.pos, w) : 0;
	r.pos += w;
	return true;
}
/* the zeros ahead of the next one bit, which is consumed; false where the data ends first. Every turn moves pos forward. */
SAU_FLAC_HD bool flac_dec_unary(FlacBits &r, uint32_t *zeros) {
	uint32_t z = 0;
	for (;;) {
		const uint32_t left = r.bits - r.pos;
		if (!left) return false;
		const unsigned w = left < 32 ? left : 32;
		const uint32_t v = flac_dec_peek(r, r.pos, w);
		if (!v) { r.pos += w; z += w; continue; }
		const unsigned lead = (unsigned)__builtin_clz(v) - (32 - w);
		r.pos += lead + 1;
		*zeros = z + lead;
		return true;
	}
}
/* the two's complement value of the low w (1 .. 32) bits */
SAU_FLAC_HD int32_t flac_dec_signed(uint32_t v, unsigned w) { return (int32_t)(v << (32 - w)) >> (32 - w); }
/* the inverse of flac_zigzag */
SAU_FLAC_HD int32_t flac_unzigzag(uint32_t u) { return (int32_t)((u >> 1) ^ (0u - (u & 1u))); }

/* What the parse leaves of a subframe, and of a frame. A FIXED or LPC subframe's channel array then holds the warm-up samples
 * and, from `order` on, the residuals; a CONSTANT one its sample at index 0; a VERBATIM one nothing: its samples stand at bit
 * `at` of the frame, bps bits each, and are read from there (flac_dec_verbatim). */
struct FlacDecSub {
	uint8_t type;     /* FLAC_CONSTANT, _VERBATIM, _FIXED, _LPC */
	uint8_t order;    /* FIXED: 0 .. 4; LPC: 1 .. 8 */
	uint8_t shift;    /* LPC: 0 .. 15 */
	uint8_t bps;      /* bits, or bits + 1 for a side channel */
	uint32_t at;      /* VERBATIM: where the samples begin */
	int16_t q[FLAC_LPC_MAX]; /* LPC: the coefficients, q[0] the most recent sample's */
};
struct FlacDecFrame {
	uint32_t n;       /* frames in the block */
	uint32_t bytes;   /* of the whole frame, CRC-16 included */
	uint32_t assign;  /* the channel assignment's four bits */
	uint32_t crc16;   /* the two bytes behind the padding */
	FlacDecSub sub[2];
};

/* the side channel among an assignment's two */
SAU_FLAC_HD unsigned flac_dec_bps(uint32_t assign, unsigned c, unsigned bits) {
	return ((assign == 8 && c == 1) || (assign == 9 && c == 0) || (assign == 10 && c == 1)) ? bits + 1 : bits;
}

/* the frame header from the sync code to the CRC-8: n and the assignment */
SAU_FLAC_HD int flac_dec_header(FlacBits &r, uint32_t channels, uint32_t B, unsigned bits, uint32_t number, FlacDecFrame *f) {
	uint32_t a, b;
	if (!flac_dec_read(r, 8, &a)) return FLAC_DEC_LENGTH;
	if (a != 0xffu) return FLAC_DEC_SYNC;
	if (!flac_dec_read(r, 8, &b)) return FLAC_DEC_LENGTH;
	if (b != 0xf8u) return FLAC_DEC_SYNC;
	if (!flac_dec_read(r, 8, &a)) return FLAC_DEC_LENGTH;
	const uint32_t code = a >> 4;
	if (code != 7 && !(code >= 8 && code <= 12 && (256u << (code - 8)) == B)) return FLAC_DEC_HEADER;
	if (a & 15u) return FLAC_DEC_HEADER;
	if (!flac_dec_read(r, 8, &a)) return FLAC_DEC_LENGTH;
	const uint32_t assign = a >> 4;
	if (channels == 1 ? assign != 0 : !(assign == 1 || assign == 8 || assign == 9 || assign == 10)) return FLAC_DEC_HEADER;
	if (((a >> 1) & 7u) != (bits == 24 ? 6u : 4u) || (a & 1u)) return FLAC_DEC_HEADER;
	f->assign = assign;
	if (!flac_dec_read(r, 8, &a)) return FLAC_DEC_LENGTH;
	uint32_t num = a, ulen = 1;
	if (a >= 0x80u) {
		ulen = (uint32_t)__builtin_clz(~(a << 24)); /* the lead byte's ones (a < 0xff: not 32) */
		if (a >= 0xfeu || ulen < 2) return FLAC_DEC_NUMBER;
		num = a & (0x7fu >> ulen);
		for (uint32_t i = 1; i < ulen; ++i) {
			if (!flac_dec_read(r, 8, &b)) return FLAC_DEC_LENGTH;
			if ((b >> 6) != 2u) return FLAC_DEC_NUMBER;
			num = (num << 6) | (b & 0x3fu);
		}
		if (flac_utf8_len(num) != ulen) return FLAC_DEC_NUMBER;
	}
	if (num != number) return FLAC_DEC_NUMBER;
	uint32_t n = B;
	if (code == 7) {
		if (!flac_dec_read(r, 16, &a)) return FLAC_DEC_LENGTH;
		n = a + 1;
		if (n >= B) return FLAC_DEC_HEADER;
	}
	f->n = n;
	const uint32_t head = r.pos >> 3; /* at most 13 */
	if (!flac_dec_read(r, 8, &a)) return FLAC_DEC_LENGTH;
	uint32_t crc = 0;
	for (uint32_t i = 0; i < head; ++i) crc = flac_crc8_update(crc, r.p[i]);
	return crc == a ? FLAC_DEC_OK : FLAC_DEC_CRC8;
}

/* the coded residuals behind a FIXED or LPC subframe's warm-up samples, into v[o .. n) */
SAU_FLAC_HD int flac_dec_residuals(FlacBits &r, uint32_t n, uint32_t B, unsigned bits, unsigned o, int32_t *v) {
	uint32_t a;
	if (!flac_dec_read(r, 2, &a)) return FLAC_DEC_LENGTH;
	if (a != (bits == 24 ? 1u : 0u)) return FLAC_DEC_RESIDUAL;
	uint32_t p;
	if (!flac_dec_read(r, 4, &p)) return FLAC_DEC_LENGTH;
	if (p > 4 || (p && n != B)) return FLAC_DEC_RESIDUAL;
	const unsigned kw = flac_k_width(bits), kmax = flac_nk(bits) - 1;
	uint32_t i = o;
	for (uint32_t j = 0; j < (1u << p); ++j) {
		uint32_t k;
		if (!flac_dec_read(r, kw, &k)) return FLAC_DEC_LENGTH;
		if (k > kmax) return FLAC_DEC_RESIDUAL;
		const uint32_t end = (j + 1) * (n >> p); /* (n >> p >= 16 > o where p > 0; o <= n where p == 0) */
		for (; i < end; ++i) {
			uint32_t z, low;
			if (!flac_dec_unary(r, &z) || !flac_dec_read(r, k, &low)) return FLAC_DEC_LENGTH;
			if (z > (0xffffffffu >> k)) return FLAC_DEC_RESIDUAL;
			v[i] = flac_unzigzag((z << k) | low);
		}
	}
	return FLAC_DEC_OK;
}

/* one subframe: its record, and in v[0 .. n) what the record's comment says */
SAU_FLAC_HD int flac_dec_subframe(FlacBits &r, uint32_t n, uint32_t B, unsigned bits, unsigned bps, int32_t *v, FlacDecSub *s) {
	uint32_t a;
	if (!flac_dec_read(r, 8, &a)) return FLAC_DEC_LENGTH;
	if (a & 0x80u) return FLAC_DEC_SUBFRAME;
	const uint32_t t = (a >> 1) & 63u;
	s->order = 0; s->shift = 0; s->bps = (uint8_t)bps; s->at = 0;
	for (unsigned j = 0; j < FLAC_LPC_MAX; ++j) s->q[j] = 0;
	if (t == 0) s->type = FLAC_CONSTANT;
	else if (t == 1) s->type = FLAC_VERBATIM;
	else if (t >= 8 && t <= 12 && t - 8 <= n) { s->type = FLAC_FIXED; s->order = (uint8_t)(t - 8); }
	else if (t >= 32 && t < 32 + FLAC_LPC_MAX && n == B) { s->type = FLAC_LPC; s->order = (uint8_t)(t - 31); }
	else return FLAC_DEC_SUBFRAME;
	if (a & 1u) return FLAC_DEC_SUBFRAME;
	if (s->type == FLAC_CONSTANT) {
		if (!flac_dec_read(r, bps, &a)) return FLAC_DEC_LENGTH;
		v[0] = flac_dec_signed(a, bps);
		return FLAC_DEC_OK;
	}
	if (s->type == FLAC_VERBATIM) {
		if ((uint64_t)bps * n > r.bits - r.pos) return FLAC_DEC_LENGTH;
		s->at = r.pos;
		r.pos += bps * n;
		return FLAC_DEC_OK;
	}
	const unsigned o = s->order;
	for (unsigned i = 0; i < o; ++i) {
		if (!flac_dec_read(r, bps, &a)) return FLAC_DEC_LENGTH;
		v[i] = flac_dec_signed(a, bps);
	}
	if (s->type == FLAC_LPC) {
		if (!flac_dec_read(r, 4, &a)) return FLAC_DEC_LENGTH;
		if (a != FLAC_LPC_PREC - 1) return FLAC_DEC_SUBFRAME;
		if (!flac_dec_read(r, 5, &a)) return FLAC_DEC_LENGTH;
		if (a > 15) return FLAC_DEC_SUBFRAME; /* (a negative shift) */
		s->shift = (uint8_t)a;
		for (unsigned j = 0; j < o; ++j) {
			if (!flac_dec_read(r, FLAC_LPC_PREC, &a)) return FLAC_DEC_LENGTH;
			s->q[j] = (int16_t)flac_dec_signed(a, FLAC_LPC_PREC);
		}
	}
	return flac_dec_residuals(r, n, B, bits, o, v);
}

/* Everything that is serial: the header, the subframes into ch0 and ch1 (room for B samples each; ch1 is not touched in
 * mono), the padding, and the two bytes of the CRC-16, which is left to the caller to hold against the frame's
 * (flac_dec_crc16 on the host). */
SAU_FLAC_HD int flac_dec_parse(FlacBits &r, uint32_t channels, uint32_t B, unsigned bits, uint32_t number, int32_t *ch0, int32_t *ch1,
		FlacDecFrame *f) {
	f->n = 0; f->bytes = 0; f->assign = 0; f->crc16 = 0;
	int st = flac_dec_header(r, channels, B, bits, number, f);
	if (st != FLAC_DEC_OK) return st;
	for (unsigned c = 0; c < channels; ++c) {
		st = flac_dec_subframe(r, f->n, B, bits, flac_dec_bps(f->assign, c, bits), c ? ch1 : ch0, &f->sub[c]);
		if (st != FLAC_DEC_OK) return st;
	}
	uint32_t a;
	if (!flac_dec_read(r, (8 - (r.pos & 7u)) & 7u, &a)) return FLAC_DEC_LENGTH; /* (never: bits is a multiple of 8) */
	if (a) return FLAC_DEC_PADDING;
	if (!flac_dec_read(r, 16, &f->crc16)) return FLAC_DEC_LENGTH;
	f->bytes = r.pos >> 3;
	return FLAC_DEC_OK;
}
/* the CRC-16 of the frame's bytes ahead of its last two, one after another */
SAU_FLAC_HD uint32_t flac_dec_crc16(const FlacBits &r, const FlacDecFrame &f) {
	uint32_t crc = 0;
	for (uint32_t i = 0; i + 2 < f.bytes; ++i) crc = flac_crc16_update(crc, r.p[i]);
	return crc;
}

/* sample i of a VERBATIM subframe (the parse has seen that all n are there) */
SAU_FLAC_HD int32_t flac_dec_verbatim(const FlacBits &r, const FlacDecSub &s, uint32_t i) {
	return flac_dec_signed(flac_dec_peek(r, s.at + s.bps * i, s.bps), s.bps);
}
/* The restoration of a CONSTANT, FIXED or LPC subframe in place, one sample after another. FIXED is the inverse of
 * flac_residual; LPC that of flac_lpc_residual with the 32-bit sum at 16 bits and the 64-bit sum at 24 (the header's step 6
 * and "LPC at 24 bits"). Unsigned arithmetic throughout: where the encoder's did not overflow, neither does this. */
SAU_FLAC_HD void flac_dec_restore(const FlacDecSub &s, uint32_t n, unsigned bits, int32_t *v) {
	if (s.type == FLAC_CONSTANT) { for (uint32_t i = 1; i < n; ++i) v[i] = v[0]; return; }
	const unsigned o = s.order;
	if (s.type == FLAC_FIXED) {
		for (uint32_t i = o; i < n; ++i) {
			const uint32_t r = (uint32_t)v[i];
			const uint32_t s1 = o > 0 ? (uint32_t)v[i - 1] : 0, s2 = o > 1 ? (uint32_t)v[i - 2] : 0, s3 = o > 2 ? (uint32_t)v[i - 3] : 0,
					s4 = o > 3 ? (uint32_t)v[i - 4] : 0;
			uint32_t x;
			switch (o) {
			case 0: x = r; break;
			case 1: x = r + s1; break;
			case 2: x = r + 2 * s1 - s2; break;
			case 3: x = r + 3 * s1 - 3 * s2 + s3; break;
			default: x = r + 4 * s1 - 6 * s2 + 4 * s3 - s4; break;
			}
			v[i] = (int32_t)x;
		}
		return;
	}
	if (s.type != FLAC_LPC) return;
	if (bits == 24) {
		for (uint32_t i = o; i < n; ++i) {
			uint64_t sum = 0;
			for (unsigned j = 0; j < o; ++j) sum += (uint64_t)((int64_t)s.q[j] * (int64_t)v[i - 1 - j]); /* (below 2^44 in size) */
			v[i] = (int32_t)((uint32_t)v[i] + (uint32_t)(uint64_t)((int64_t)sum >> s.shift));
		}
	} else {
		for (uint32_t i = o; i < n; ++i) {
			uint32_t sum = 0;
			for (unsigned j = 0; j < o; ++j) sum += (uint32_t)s.q[j] * (uint32_t)v[i - 1 - j];
			v[i] = (int32_t)((uint32_t)v[i] + (uint32_t)((int32_t)sum >> s.shift));
		}
	}
}
/* the stereo inverses: from the two subframes' samples to L and R, in 64 bits (a and b are any int32) */
SAU_FLAC_HD void flac_dec_stereo(uint32_t assign, int32_t a, int32_t b, int64_t *L, int64_t *R) {
	switch (assign) {
	case 8: *L = a; *R = (int64_t)a - b; break;                 /* left, side */
	case 9: *L = (int64_t)a + b; *R = b; break;                 /* side, right */
	case 10: {                                                  /* mid, side: m = (a << 1) | (b & 1) */
		const int64_t m = ((int64_t)a * 2) | (b & 1);
		*L = (m + b) >> 1; *R = (m - b) >> 1;
		break;
	}
	default: *L = a; *R = b; break;                             /* L, R; mono: a alone */
	}
}
SAU_FLAC_HD bool flac_dec_fits(int64_t x, unsigned bits) { return x >= -(1ll << (bits - 1)) && x < (1ll << (bits - 1)); }

/* One frame from its first byte on, by one thread: ch0, ch1 as in flac_dec_parse; out[n * channels] interleaved where the
 * status is OK (out may be NULL: the status alone). f->n and f->bytes are the frame's. */
SAU_FLAC_HD int flac_decode_frame(const uint8_t *data, uint64_t len, uint32_t channels, uint32_t B, unsigned bits, uint32_t number, int32_t *ch0,
		int32_t *ch1, FlacDecFrame *f, int32_t *out, uint64_t cap_frames) {
	FlacBits r = flac_dec_bits(data, len, channels, B, bits);
	int st = flac_dec_parse(r, channels, B, bits, number, ch0, ch1, f);
	if (st != FLAC_DEC_OK) return st;
	if (flac_dec_crc16(r, *f) != f->crc16) return FLAC_DEC_CRC16;
	for (unsigned c = 0; c < channels; ++c) {
		int32_t *v = c ? ch1 : ch0;
		if (f->sub[c].type == FLAC_VERBATIM) { for (uint32_t i = 0; i < f->n; ++i) v[i] = flac_dec_verbatim(r, f->sub[c], i); }
		else flac_dec_restore(f->sub[c], f->n, bits, v);
	}
	for (uint32_t i = 0; i < f->n; ++i) {
		int64_t L, R;
		flac_dec_stereo(f->assign, ch0[i], channels == 2 ? ch1[i] : 0, &L, &R);
		if (!flac_dec_fits(L, bits) || (channels == 2 && !flac_dec_fits(R, bits))) return FLAC_DEC_RANGE;
		if (out && i < cap_frames) { out[(uint64_t)i * channels] = (int32_t)L; if (channels == 2) out[(uint64_t)i * channels + 1] = (int32_t)R; }
	}
	return FLAC_DEC_OK;
}

} /* namespace sauflac */
#endif
