/* capi_internal.h -- what the test-hook library (tests/hooks/test_hooks.cpp -> tests/hooks/libsaugns_amd_hooks.so) reaches
 * of capi.cpp and sndout.cpp beside the C ABI. Hidden visibility: none of this is an export of libsaugns_amd.so. The hook
 * library links the product's own objects and adds the entry points tests/ use to run the host control plane over an
 * injected backend (tests/seqexec) and to probe the device-compiled arithmetic; the product library has none of them
 * (VERDICT r04 item 9). */
#ifndef SAU_CAPI_INTERNAL_H
#define SAU_CAPI_INTERNAL_H
#include "../../include/saugns_amd.h"
#include "engine.h"
#include <functional>
#include <string>

namespace sauamd_internal {
/* sau_create_Generator / sauAmd_create_Batch over a caller-supplied backend (owned by the object made; NULL: the HIP one) */
sauGenerator *make_generator(const sauProgram *prg, uint32_t srate, sauengine::Backend *injected);
sauAmdBatch *make_batch_over(const sauProgram *const *prgs, size_t n, uint32_t srate, sauengine::Backend *injected, int device = -1);
/* how often a call of another size or channel layout took this generator's read-ahead back (capi.cpp: generator_rewind) */
unsigned generator_rewinds(const sauGenerator *g);
/* sauAmd_render_file's body (sndout.cpp) */
bool render_file(const sauProgram *prg, uint32_t srate, const char *path, int format, int channels,
		sauengine::Backend *injected, uint64_t *frames_out, std::string &err);
/* sauAmd_render_file_normalized's body (sndout.cpp). The two passes run on two engines, each over a backend of its own:
 * make_backend is asked once per pass (NULL with err: that pass cannot run) and the engine made over it owns what it returns. */
bool render_file_normalized(const sauProgram *prg, uint32_t srate, const char *path, int format, int channels, float target_peak,
		const std::function<sauengine::Backend *(std::string &)> &make_backend, uint64_t *frames_out, sauAmdLevels *levels_out,
		std::string &err);
/* sauAmd_render_file_oversampled's body (sndout.cpp). make_backend is asked once, after the arguments have been looked at
 * (NULL with err: the render cannot run); the engine made over what it returns owns it. */
bool render_file_oversampled(const sauProgram *prg, uint32_t srate, int factor, const char *path, int format, int channels,
		const std::function<sauengine::Backend *(std::string &)> &make_backend, uint64_t *frames_out, std::string &err);
/* sauAmd_render_file_loudness's body (sndout.cpp). As render_file_normalized: two passes, two engines, make_backend asked once
 * per pass -- after the arguments have been looked at, so a bad argument asks for none. */
bool render_file_loudness(const sauProgram *prg, uint32_t srate, const char *path, int format, int channels, double target_lufs,
		float max_true_peak, const std::function<sauengine::Backend *(std::string &)> &make_backend, uint64_t *frames_out,
		sauAmdLoudness *loud_out, float *gain_out, std::string &err);
/* sauAmd_render_file_loudness_limited's body (sndout.cpp). As render_file_loudness: two passes, two engines, make_backend asked
 * once per pass -- after the arguments have been looked at, so a bad argument asks for none. */
bool render_file_loudness_limited(const sauProgram *prg, uint32_t srate, const char *path, int format, int channels, double target_lufs,
		float max_true_peak, const std::function<sauengine::Backend *(std::string &)> &make_backend, uint64_t *frames_out,
		sauAmdLoudness *loud_out, float *gain_out, sauAmdLimiterStats *stats_out, std::string &err);
/* sauAmd_render_spectrum's body (sndout.cpp). make_backend is asked once, after the arguments have been looked at (NULL with
 * err: the render cannot run); the engine made over what it returns owns it. */
bool render_spectrum(const sauProgram *prg, uint32_t srate, int factor, int channels, unsigned log2n, uint32_t hop,
		const std::function<sauengine::Backend *(std::string &)> &make_backend, double *power_out, uint64_t *segments_out,
		uint64_t *frames_out, std::string &err);
/* sauAmd_render_file_flac's body (sndout.cpp). make_backend is asked once, after the arguments have been looked at (NULL with
 * err: the render cannot run); the engine made over what it returns owns it. A backend without an encoder is refused before
 * the file is created. */
bool render_file_flac(const sauProgram *prg, uint32_t srate, const char *path, int channels, uint32_t block_frames,
		const std::function<sauengine::Backend *(std::string &)> &make_backend, uint64_t *frames_out, sauAmdFlacInfo *info_out,
		std::string &err);
/* sauAmd_render_file_flac_lpc's body: the same with the LPC mode's max_lpc_order (0: render_file_flac) */
bool render_file_flac_lpc(const sauProgram *prg, uint32_t srate, const char *path, int channels, uint32_t block_frames, uint32_t max_lpc_order,
		const std::function<sauengine::Backend *(std::string &)> &make_backend, uint64_t *frames_out, sauAmdFlacInfo *info_out,
		std::string &err);
/* sauAmd_render_file_flac_f32's body (sndout.cpp): as render_file_flac_lpc, over float runs and a float-fed encoder of `bits` */
bool render_file_flac_f32(const sauProgram *prg, uint32_t srate, const char *path, int channels, uint32_t block_frames, int bits,
		uint32_t max_lpc_order, float gain, const std::function<sauengine::Backend *(std::string &)> &make_backend, uint64_t *frames_out,
		sauAmdFlacInfo *info_out, std::string &err);
/* sauAmd_render_file_flac_loudness's body (sndout.cpp). As render_file_loudness and render_file_loudness_limited: two passes, two
 * engines, make_backend asked once per pass -- after the arguments have been looked at, so a bad argument asks for none. */
bool render_file_flac_loudness(const sauProgram *prg, uint32_t srate, const char *path, int channels, uint32_t block_frames, int bits,
		uint32_t max_lpc_order, double target_lufs, float max_true_peak, bool limited,
		const std::function<sauengine::Backend *(std::string &)> &make_backend, uint64_t *frames_out, sauAmdLoudness *loud_out,
		float *gain_out, sauAmdLimiterStats *stats_out, sauAmdFlacInfo *info_out, std::string &err);
/* sauAmd_render_file_flac_lpc24's and sauAmd_render_file_flac_loudness_lpc24's bodies (sndout.cpp): the two above at 24 bits over
 * Backend::create_flac_lpc24's encoder, max_lpc_order 0 .. 8 */
bool render_file_flac_lpc24(const sauProgram *prg, uint32_t srate, const char *path, int channels, uint32_t block_frames,
		uint32_t max_lpc_order, float gain, const std::function<sauengine::Backend *(std::string &)> &make_backend, uint64_t *frames_out,
		sauAmdFlacInfo *info_out, std::string &err);
bool render_file_flac_loudness_lpc24(const sauProgram *prg, uint32_t srate, const char *path, int channels, uint32_t block_frames,
		uint32_t max_lpc_order, double target_lufs, float max_true_peak, bool limited,
		const std::function<sauengine::Backend *(std::string &)> &make_backend, uint64_t *frames_out, sauAmdLoudness *loud_out,
		float *gain_out, sauAmdLimiterStats *stats_out, sauAmdFlacInfo *info_out, std::string &err);
/* the thread's sauAmd_last_error text (capi.cpp), with the line on stderr */
void set_last_error(const char *where, const std::string &err);
} /* namespace sauamd_internal */
#endif
