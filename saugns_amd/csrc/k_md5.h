/* k_md5.h -- the MD5 of a FLAC encoder's unencoded samples (include/saugns_amd.h, section "FLAC", paragraph "MD5"): part of
 * hip_backend.hip (inside namespace sauhip), behind k_flac.h, none of whose kernels it changes. The arithmetic is sau_md5.h's,
 * which the host restatement (tables.cpp: flac_md5) uses too.
 *   flac_md5_kernel, flac_md5_wide_kernel (int32 samples: 24 bits)    grid (rows) x 64: a wave owns a row. MD5 is one serial
 *       chain per row -- a chunk's 64 steps need the state the chunk before left --, so the rows are what runs side by side.
 *       The wave walks the samples of the blocks this feed completes for its row, addressed as flac_stage addresses them: the
 *       pending frames first, then the fed row. A pass is 64 message words, one per lane, four chunks: lane l fetches and packs
 *       word 64 pass + l (neighbouring lanes read neighbouring samples), and the next pass's word is fetched before this pass's
 *       steps begin, so a fetch has four chunks' steps to arrive in. For each chunk the 16 words go from their lanes to every
 *       lane (a cross-lane read at a constant offset from the chunk's first lane), and all lanes take the 64 steps on equal
 *       values: in vector registers a step is four or five instructions (a bit-select, a three-operand add, a rotate, an
 *       add), in scalar ones about twice that, and one wave alone issues either kind at the same pace.
 *       The running state (four words per row) lies in device memory and is carried across feeds. A whole block is a multiple
 *       of 64 bytes (the smallest block is 256 frames), so nothing but a finish's short block ends inside a chunk, and no
 *       partial chunk is ever carried. On a finish the wave hashes what is left with the padding behind it (md5_finish, with
 *       the stream's byte count from the host) and stores the digest; that happens for a row that completes no block, too. */
#ifndef SAU_K_MD5_H
#define SAU_K_MD5_H

using namespace saumd5;

struct FlacMd5Row { /* (uploaded as it stands) */
	unsigned long long total; /* the stream's bytes of unencoded samples with this feed in: read on a finish */
};
static_assert(sizeof(FlacMd5Row) == 8, "FlacMd5Row is uploaded as it stands");

struct FlacMd5Params {
	const void *rows;         /* the rows the analysis reads: int16, or int32 for the wide kernel */
	size_t row_pitch;         /* bytes between them */
	const FlacRow *desc;      /* [n_rows] (launch_plan.h) */
	const void *pend;         /* [n_rows][pend_pitch], as FlacParams::pend */
	size_t pend_pitch;        /* samples */
	const FlacMd5Row *md5;    /* [n_rows] */
	uint32_t *state;          /* [n_rows][4] */
	uint32_t *digest;         /* [n_rows][4]: written on a finish */
	uint32_t B, channels, n_rows, finish;
};

template <class T>
__device__ __forceinline__ void flac_md5_row(const FlacMd5Params &P) {
	const unsigned row = blockIdx.x, lane = threadIdx.x;
	if (row >= P.n_rows) return;
	const FlacRow d = P.desc[row];
	const T *xrow = (const T *)((const char *)P.rows + P.row_pitch * row);
	const T *pend = (const T *)P.pend + P.pend_pitch * row;
	const unsigned long long n_pend = (unsigned long long)d.pend * P.channels;
	/* the samples of the blocks this feed completes, counted from the row's frame block0 * B */
	const unsigned long long n = d.n_blocks ? ((unsigned long long)(d.n_blocks - 1) * P.B + d.last_n) * P.channels : 0;
	const unsigned long long whole = n * (sizeof(T) == 4 ? 3 : 2) / 64; /* chunks; one more on a finish: the rest and the padding */
	const unsigned long long chunks = whole + (P.finish ? 1 : 0);
	const auto at = [&](unsigned long long i) -> int32_t { return i < n_pend ? pend[i] : xrow[i - n_pend]; };
	const auto word = [&](unsigned long long w) -> uint32_t { return sizeof(T) == 4 ? md5_word24(at, w, n) : md5_word16(at, w, n); };

	uint32_t s[4];
	for (int i = 0; i < 4; ++i) s[i] = P.state[4 * row + i];
	uint32_t cur = chunks ? word(lane) : 0u;
	for (unsigned long long c0 = 0; c0 < chunks; c0 += 4) {
		const uint32_t nxt = c0 + 4 < chunks ? word((c0 + 4) * 16 + lane) : 0u;
#pragma unroll 1
		for (unsigned c = 0; c < 4; ++c) {
			if (c0 + c >= chunks) break;
			uint32_t w[16];
			for (unsigned k = 0; k < 16; ++k) w[k] = (uint32_t)__shfl((int)cur, (int)(c * 16 + k));
			if (c0 + c < whole) md5_chunk(s, w);
			else md5_finish(s, w, P.md5[row].total);
		}
		cur = nxt;
	}
	if (lane < 4) {
		const uint32_t v = lane == 0 ? s[0] : lane == 1 ? s[1] : lane == 2 ? s[2] : s[3];
		P.state[4 * row + lane] = v;
		if (P.finish) P.digest[4 * row + lane] = v; /* (the digest's bytes are the words' low bytes first: the device's order) */
	}
}

__global__ void __launch_bounds__(64) flac_md5_kernel(const FlacMd5Params P) { flac_md5_row<int16_t>(P); }
__global__ void __launch_bounds__(64) flac_md5_wide_kernel(const FlacMd5Params P) { flac_md5_row<int32_t>(P); }

#endif
