/* decimate_hooks.cpp -- TEST INFRASTRUCTURE: the decimator (saugns_amd/csrc/k_decimate.h) over rows the test supplies, for
 * tests/test_gpu_decimate_rows.py. Backend::decimate reads the last float run's rows and Engine::run_decimated always renders
 * them first, so crafted material -- NaN, infinities, full scale, subnormals, poison behind a stream's end, frame counts of any
 * residue -- reaches decimate_kernel and decimate_carry_kernel only through here.
 * Nothing of the product is changed for it: the hook makes the HIP backend itself, makes the batch over it
 * (sauamd_internal::make_batch_over; the engine owns the backend from then on) and keeps the Backend * it made, so it talks
 * to the backend beside the engine. The engine is never told about the decimation; such a batch is used for nothing else. */
#include "../../saugns_amd/csrc/capi_internal.h"
#include "../../saugns_amd/csrc/hip_backend.h"
#include <hip/hip_runtime_api.h>
#include <vector>

#define HOOK extern "C" __attribute__((visibility("default")))

namespace {
struct DecimRows {
	sauAmdBatch *batch;
	sauengine::Backend *be; /* the batch's engine's: not ours to delete */
	size_t n;
};
bool fail(const std::string &err) { sauamd_internal::set_last_error("decimate hook", err); return false; }
}

HOOK void *sauAmd_decimate_rows_create(const sauProgram *const *prgs, size_t n, uint32_t srate) {
	std::string err;
	sauengine::Backend *be = sauhip::create_hip_backend(err);
	if (!be) { fail(err); return nullptr; }
	sauAmdBatch *b = sauamd_internal::make_batch_over(prgs, n, srate, be); /* (a failure has deleted the backend and reported) */
	if (!b) return nullptr;
	return new DecimRows{b, be, n};
}

HOOK void sauAmd_decimate_rows_destroy(void *h) {
	DecimRows *d = (DecimRows *)h;
	if (!d) return;
	sauAmd_destroy_Batch(d->batch);
	delete d;
}

/* one float run of `frames` frames, not fetched: it sizes the rows and leaves them float, which decimate() demands */
HOOK bool sauAmd_decimate_rows_prime(void *h, size_t frames, int stereo) {
	DecimRows *d = (DecimRows *)h;
	std::vector<char> more(d->n); /* (bool[n]) */
	std::vector<size_t> lens(d->n);
	return sauAmd_Batch_run_f32(d->batch, nullptr, frames, stereo != 0, (bool *)more.data(), lens.data());
}

HOOK bool sauAmd_decimate_rows_begin(void *h, int factor, int stereo) {
	DecimRows *d = (DecimRows *)h;
	std::string err;
	return d->be->begin_decimation(factor, stereo != 0, err) || fail(err);
}

/* rows: n host rows, row_floats floats apart, of buf_len * factor * channels floats each -- all of them are copied over the
 * batch's float rows, what lies behind frames_hi[s] included. out: n rows, out_bytes bytes apart, of buf_len * channels samples
 * (float32, or int16 as out_f32 is 0) */
HOOK bool sauAmd_decimate_rows_run(void *h, const float *rows, size_t row_floats, const uint32_t *frames_hi, uint32_t buf_len, int factor,
		int stereo, int out_f32, int swap_bytes, void *out, size_t out_bytes) {
	DecimRows *d = (DecimRows *)h;
	std::string err;
	const size_t ch = stereo ? 2 : 1, floats = (size_t)buf_len * (size_t)factor * ch;
	const size_t bytes = (size_t)buf_len * ch * (out_f32 ? sizeof(float) : sizeof(int16_t));
	if (factor < 1 || row_floats < floats || out_bytes < bytes) return fail("bad argument");
	if (!sauAmd_Batch_sync(d->batch)) return false;
	const size_t pitch = sauAmd_Batch_device_pcm_pitch(d->batch);
	if (floats * sizeof(float) > pitch || !sauAmd_Batch_device_pcm_f32(d->batch, 0)) return fail("the batch's rows are not float32, or shorter than the run");
	for (size_t s = 0; s < d->n && floats; ++s) {
		const float *dev = sauAmd_Batch_device_pcm_f32(d->batch, s);
		const hipError_t e = hipMemcpy((void *)dev, rows + s * row_floats, floats * sizeof(float), hipMemcpyHostToDevice);
		if (e != hipSuccess) return fail(std::string("hipMemcpy: ") + hipGetErrorString(e));
	}
	if (!d->be->decimate(frames_hi, buf_len, factor, stereo != 0, out_f32 ? sauengine::SF_F32 : sauengine::SF_S16, swap_bytes != 0, err))
		return fail(err);
	for (size_t s = 0; s < d->n && bytes; ++s)
		if (!(d->be->fetch_decimated_async((uint32_t)s, (char *)out + s * out_bytes, bytes, 0, err) && d->be->wait_fetch(0, err)))
			return fail(err);
	return true;
}
