/* k_flac_dec.h -- the FLAC decoder on the device: part of hip_backend.hip (inside namespace sauhip), behind k_flac.h. The format
 * and the statuses are stated in include/saugns_amd.h, section "FLAC", paragraph "Verify"; the arithmetic, the bit reader and the
 * order of the checks are sau_flac_dec.h's, which the host restatement (tables.cpp: flac_decode_block) runs too -- there is no
 * second reader here, so what bounds the host's reads bounds the kernel's.
 *   flac_decode_kernel<W, VERIFY>  grid (jobs) x 256: a workgroup owns one frame, the job of flac_write_kernel whose bytes lie at
 *       out + out_off + off. W is the width, FlacS16 or FlacS32, as in k_flac.h.
 *       1. the frame's bytes -- no more than the frame bound of (B, channels, bits), whatever the record says -- into LDS, a byte
 *          per lane, consecutive lanes consecutive bytes;
 *       2. thread 0 parses: header and CRC-8, then the subframes bit by bit (a code's place depends on every code before it),
 *          leaving warm-up samples and residuals in the channels' LDS arrays and the record of each subframe (FlacDecFrame, in
 *          LDS: its fields are picked by index); VERBATIM samples are only located, not read;
 *       3. all threads: the CRC-16 as flac_write_kernel makes it -- a run of bytes per thread, advanced over what follows
 *          (flac_crc16_advance), XORed;
 *       4. restoration: VERBATIM samples are read and CONSTANT ones spread by all threads; a FIXED or LPC channel is restored by
 *          lane 0 of wave c, so the two channels of a stereo frame run side by side on two waves;
 *       5. all threads: the stereo inverse and the range check, then either the store (the decode form: samples, status and n per
 *          job) or the compare with the block's original samples (the verify form), which are read straight from the fed row or
 *          the pending buffer -- the frames W::stage reads --, consecutive lanes consecutive frames, never staged.
 *       The verify form takes the expected n from the feed's plan (FlacRow) and the expected size from the frame's record; the
 *       expected number is block0 + j in both. Per row it adds to a count of blocks and of bad blocks and takes the 64-bit
 *       atomicMin of (block number << 8) | status: integer atomics only, so the record depends on no order.
 * LDS: channels * B samples of 4 bytes and the frame bound rounded up to a word; 57364 bytes at 24 bits, B = 4096, stereo, with
 * under 200 bytes of static LDS beside them: below the 64 KiB of a workgroup. Nothing is indexed at run time in registers. */
#ifndef SAU_K_FLAC_DEC_H
#define SAU_K_FLAC_DEC_H

struct FlacVerifyRec { /* per row, since the last reset */
	unsigned long long blocks, bad_blocks;
	unsigned long long first; /* the least (block number << 8) | status of a bad block; all ones: none */
};
static_assert(sizeof(FlacVerifyRec) == 24, "FlacVerifyRec is fetched as it stands");

struct FlacDecArgs {
	int32_t *samples;        /* decode form: [jobs][B * channels], interleaved; NULL: not stored */
	uint32_t *job_status;    /* [jobs], may be NULL */
	uint32_t *job_n;         /* [jobs], may be NULL: the frame's n where the status is OK, else 0 */
	FlacVerifyRec *rec;      /* [n_rows], may be NULL */
};

/* frame `rel` of the row's feed, counted from the row's frame block0 * B: what W::stage would stage */
template <typename W>
__device__ __forceinline__ void flac_dec_original(const FlacParams &P, const FlacRow &d, const unsigned row, const unsigned long long rel, int32_t &l, int32_t &r) {
	typedef typename W::sample_t T;
	const T *xrow = (const T *)((const char *)P.rows + P.row_pitch * row);
	const T *pend = (const T *)P.pend + P.pend_pitch * row;
	const T *src = rel < d.pend ? pend + rel * P.channels : xrow + (rel - d.pend) * P.channels;
	l = src[0];
	r = P.channels == 2 ? src[1] : 0;
}

template <typename W, bool VERIFY>
__global__ __launch_bounds__(FLAC_THREADS) void flac_decode_kernel(const FlacParams P, const FlacDecArgs A) {
	extern __shared__ uint32_t flac_lds[];
	__shared__ FlacDecFrame s_fr;
	__shared__ int s_status;
	__shared__ uint32_t s_crc, s_flags;
	int32_t *s_v = (int32_t *)flac_lds;
	uint8_t *s_b = (uint8_t *)(flac_lds + P.B * P.channels);
	const unsigned tid = threadIdx.x, job = blockIdx.x, row = flac_find_row(P.desc, P.n_rows, job);
	const FlacRow d = P.desc[row];
	const unsigned j = job - d.job0;
	if (j >= d.n_blocks) return; /* (never; uniform) */
	const uint32_t n_plan = j == d.n_blocks - 1 ? d.last_n : P.B;
	const uint32_t number = (uint32_t)(d.block0 + j);
	const uint32_t fd_bytes = P.frames[job].bytes, fd_off = P.frames[job].off;
	const uint32_t bound = flac_frame_bound(P.B, P.channels, W::BITS);
	const uint32_t len = fd_bytes < bound ? fd_bytes : bound; /* (what LDS has room for: a frame is never longer) */
	const uint8_t *src = P.out + d.out_off + fd_off;
	for (uint32_t b = tid; b < len; b += FLAC_THREADS) s_b[b] = src[b];
	if (tid == 0) { s_crc = 0; s_flags = 0; }
	__syncthreads();
	FlacBits rd = flac_dec_bits(s_b, len, P.channels, P.B, W::BITS);
	if (tid == 0) s_status = flac_dec_parse(rd, P.channels, P.B, W::BITS, number, s_v, s_v + P.B, &s_fr);
	__syncthreads();
	int status = s_status; /* (the same for the whole workgroup, and so is everything that branches on it) */
	const uint32_t n = s_fr.n;
	if (status == FLAC_DEC_OK) {
		const uint32_t body = s_fr.bytes - 2; /* (bytes <= len: the parse read them all) */
		const uint32_t run = (body + FLAC_THREADS - 1) / FLAC_THREADS, b0 = tid * run, b1 = b0 + run < body ? b0 + run : body;
		uint32_t crc = 0;
		for (uint32_t b = b0; b < b1; ++b) crc = flac_crc16_update(crc, s_b[b]);
		crc = b0 < body ? flac_crc16_advance(crc, body - b1) : 0;
		for (int m = 1; m < 64; m <<= 1) crc ^= __shfl_xor(crc, m);
		if ((tid & 63) == 0) atomicXor(&s_crc, crc);
		__syncthreads();
		if (s_crc != s_fr.crc16) status = FLAC_DEC_CRC16;
	}
	if (status == FLAC_DEC_OK) {
		for (unsigned c = 0; c < P.channels; ++c) {
			const FlacDecSub &s = s_fr.sub[c];
			int32_t *v = s_v + c * P.B;
			if (s.type == FLAC_VERBATIM) { for (uint32_t i = tid; i < n; i += FLAC_THREADS) v[i] = flac_dec_verbatim(rd, s, i); }
			else if (s.type == FLAC_CONSTANT) { const int32_t x = v[0]; for (uint32_t i = tid + 1; i < n; i += FLAC_THREADS) v[i] = x; }
		}
		const unsigned wave = tid >> 6;
		if ((tid & 63) == 0 && wave < P.channels && (s_fr.sub[wave].type == FLAC_FIXED || s_fr.sub[wave].type == FLAC_LPC))
			flac_dec_restore(s_fr.sub[wave], n, W::BITS, s_v + wave * P.B);
		__syncthreads();
		const bool same = !VERIFY || (n == n_plan && s_fr.bytes == fd_bytes);
		uint32_t flags = 0; /* 1: beyond the bits; 2: not the original */
		for (uint32_t i = tid; i < n; i += FLAC_THREADS) {
			int64_t L, R;
			flac_dec_stereo(s_fr.assign, s_v[i], P.channels == 2 ? s_v[P.B + i] : 0, &L, &R);
			if (!flac_dec_fits(L, W::BITS) || (P.channels == 2 && !flac_dec_fits(R, W::BITS))) flags |= 1u;
			if (VERIFY) {
				if (same) { /* (n is the plan's: frame i is inside what the analysis read) */
					int32_t ol, orr;
					flac_dec_original<W>(P, d, row, (unsigned long long)j * P.B + i, ol, orr);
					if (L != ol || (P.channels == 2 && R != orr)) flags |= 2u;
				}
			} else if (A.samples) {
				int32_t *dst = A.samples + ((size_t)job * P.B + i) * P.channels;
				dst[0] = (int32_t)L;
				if (P.channels == 2) dst[1] = (int32_t)R;
			}
		}
		if (!same) flags |= 2u;
		if (flags) atomicOr(&s_flags, flags);
		__syncthreads();
		if (s_flags & 1u) status = FLAC_DEC_RANGE;
		else if (s_flags & 2u) status = FLAC_DEC_MISMATCH;
	}
	if (tid == 0) {
		if (A.job_status) A.job_status[job] = (uint32_t)status;
		if (A.job_n) A.job_n[job] = status == FLAC_DEC_OK ? n : 0; /* (as the host restatement's *n_out) */
		if (A.rec) {
			atomicAdd(&A.rec[row].blocks, 1ull);
			if (status != FLAC_DEC_OK) {
				atomicAdd(&A.rec[row].bad_blocks, 1ull);
				atomicMin(&A.rec[row].first, ((unsigned long long)number << 8) | (unsigned long long)status);
			}
		}
	}
}

#endif
