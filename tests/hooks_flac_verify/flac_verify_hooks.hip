/* TEST INFRASTRUCTURE: the product's flac_decode_kernel (saugns_amd/csrc/k_flac_dec.h), both forms and both widths, over frames
 * and expected samples the test supplies (tests/test_gpu_flac_verify.py). The kernel is the product's source, included the way
 * hip_backend.hip includes it and compiled for gfx950 with the product's flags; nothing of the product's objects is linked.
 *   sauAmd_flac_verify_hook_run  rows as a feed's plan describes them -- row r completes n_blocks[r] blocks from block0[r] on, the
 *       last of last_n[r] frames --, their jobs numbered row after row; job k's frame is data[off[k] .. off[k] + len[k]). The
 *       decode form (verify == 0) leaves samples[k][B * channels]; the verify form holds frame i of row r's job j against
 *       expect[r][(j * B + i) * channels ..], rows expect_pitch samples apart. Either way status[k], n[k], and per row
 *       rec[r] = {blocks, bad_blocks, (first bad block << 8) | status, or all ones}. 1, or 0 when an argument or a HIP call failed. */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <type_traits>
#include <vector>
#include "../../saugns_amd/csrc/sau_dev_ops.h"
#include "../../saugns_amd/csrc/k_wave_scan.h"
#include "../../saugns_amd/csrc/launch_plan.h"
#include "../../saugns_amd/csrc/sau_flac_dec.h"

#define HOOK extern "C" __attribute__((visibility("default")))

namespace fvk {
using namespace saudev;
using namespace sauplan;
#include "../../saugns_amd/csrc/k_common.h"
#include "../../saugns_amd/csrc/k_flac.h"
#include "../../saugns_amd/csrc/k_flac_dec.h"

template <typename T>
struct Dev {
	T *p = nullptr;
	~Dev() { if (p) (void)hipFree(p); }
	bool put(const T *src, size_t n) {
		if (hipMalloc((void **)&p, (n ? n : 1) * sizeof(T)) != hipSuccess) return false;
		return !n || hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice) == hipSuccess;
	}
	bool zero(size_t n) { return hipMalloc((void **)&p, (n ? n : 1) * sizeof(T)) == hipSuccess && hipMemset(p, 0, (n ? n : 1) * sizeof(T)) == hipSuccess; }
	bool get(T *dst, size_t n) { return !n || hipMemcpy(dst, p, n * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess; }
};

template <typename W>
static bool run(int verify, uint32_t channels, uint32_t B, uint32_t n_rows, const uint64_t *block0, const uint32_t *n_blocks, const uint32_t *last_n,
		const uint8_t *data, size_t data_len, const uint32_t *off, const uint32_t *len, const int32_t *expect, size_t expect_pitch,
		uint32_t *status, uint32_t *n_out, int32_t *samples, uint64_t *rec_out) {
	typedef typename W::sample_t T;
	std::vector<FlacRow> rows(n_rows);
	uint32_t jobs = 0;
	for (uint32_t r = 0; r < n_rows; ++r) {
		if (!n_blocks[r] || !last_n[r] || last_n[r] > B) return false;
		memset((void *)&rows[r], 0, sizeof(FlacRow));
		rows[r].block0 = block0[r]; rows[r].n_blocks = n_blocks[r]; rows[r].last_n = last_n[r]; rows[r].job0 = jobs;
		jobs += n_blocks[r];
	}
	std::vector<FlacFrameDesc> fd(jobs);
	memset((void *)fd.data(), 0, jobs * sizeof(FlacFrameDesc));
	for (uint32_t k = 0; k < jobs; ++k) {
		if ((size_t)off[k] + len[k] > data_len) return false;
		fd[k].off = off[k]; fd[k].bytes = len[k];
	}
	std::vector<T> ex;
	if (verify) { /* every job's frames have to lie inside its expected row */
		ex.resize((size_t)n_rows * expect_pitch);
		for (uint32_t r = 0; r < n_rows; ++r)
			if (((size_t)(n_blocks[r] - 1) * B + last_n[r]) * channels > expect_pitch) return false;
		for (size_t i = 0; i < ex.size(); ++i) ex[i] = (T)expect[i];
	}
	std::vector<FlacVerifyRec> rec(n_rows, FlacVerifyRec{0, 0, ~0ull});
	Dev<FlacRow> d_rows; Dev<FlacFrameDesc> d_fd; Dev<uint8_t> d_data; Dev<T> d_ex; Dev<uint32_t> d_status, d_n; Dev<int32_t> d_samples;
	Dev<FlacVerifyRec> d_rec;
	const size_t n_samples = verify ? 0 : (size_t)jobs * B * channels;
	if (!d_rows.put(rows.data(), n_rows) || !d_fd.put(fd.data(), jobs) || !d_data.put(data, data_len) || !d_ex.put(ex.data(), ex.size()) ||
	    !d_status.zero(jobs) || !d_n.zero(jobs) || !d_samples.zero(n_samples) || !d_rec.put(rec.data(), n_rows)) return false;
	FlacParams P;
	memset((void *)&P, 0, sizeof P);
	P.rows = d_ex.p; P.row_pitch = expect_pitch * sizeof(T); P.desc = d_rows.p;
	P.pend = d_ex.p; P.pend_pitch = 0; /* (no row has pending frames) */
	P.frames = d_fd.p; P.out = d_data.p;
	P.B = B; P.channels = channels; P.n_rows = n_rows; P.jobs = jobs;
	FlacDecArgs A;
	A.samples = verify ? nullptr : d_samples.p; A.job_status = d_status.p; A.job_n = d_n.p; A.rec = d_rec.p;
	const size_t lds = plan_flac_decode_lds(B, channels, W::BITS);
	if (!lds) return false;
	if (verify) hipLaunchKernelGGL((flac_decode_kernel<W, true>), dim3(jobs), dim3(FLAC_THREADS), lds, 0, P, A);
	else hipLaunchKernelGGL((flac_decode_kernel<W, false>), dim3(jobs), dim3(FLAC_THREADS), lds, 0, P, A);
	if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return false;
	if (!d_status.get(status, jobs) || !d_n.get(n_out, jobs) || !d_rec.get(rec.data(), n_rows)) return false;
	if (!verify && samples && !d_samples.get(samples, n_samples)) return false;
	for (uint32_t r = 0; r < n_rows; ++r) { rec_out[3 * r] = rec[r].blocks; rec_out[3 * r + 1] = rec[r].bad_blocks; rec_out[3 * r + 2] = rec[r].first; }
	return true;
}
} /* namespace fvk */

HOOK int sauAmd_flac_verify_hook_run(int bits, int verify, uint32_t channels, uint32_t block_frames, uint32_t n_rows, const uint64_t *block0,
		const uint32_t *n_blocks, const uint32_t *last_n, const uint8_t *data, size_t data_len, const uint32_t *off, const uint32_t *len,
		const int32_t *expect, size_t expect_pitch, uint32_t *status, uint32_t *n_out, int32_t *samples, uint64_t *rec_out) {
	const uint32_t B = sauflac::flac_block_frames(block_frames);
	if (!B || block_frames == 0 || (channels != 1 && channels != 2) || !n_rows || n_rows > sauflac::FLAC_MAX_ROWS || !block0 || !n_blocks ||
	    !last_n || !data || !off || !len || !status || !n_out || !rec_out || (verify && !expect)) return 0;
	if (bits == 16)
		return fvk::run<fvk::FlacS16>(verify, channels, B, n_rows, block0, n_blocks, last_n, data, data_len, off, len, expect, expect_pitch, status,
			n_out, samples, rec_out) ? 1 : 0;
	if (bits == 24)
		return fvk::run<fvk::FlacS32>(verify, channels, B, n_rows, block0, n_blocks, last_n, data, data_len, off, len, expect, expect_pitch, status,
			n_out, samples, rec_out) ? 1 : 0;
	return 0;
}
