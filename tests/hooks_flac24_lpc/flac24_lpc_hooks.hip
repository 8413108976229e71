/* TEST INFRASTRUCTURE: step 5b of "LPC at 24 bits" (include/saugns_amd.h, FLAC; sau_flac.h: flac_lpc_guard) as a known-answer
 * probe, on the host and as hipcc compiles it for gfx950 with the product's flags. Nothing of the product's objects is linked:
 * the function is the header's.
 *   sauAmd_kat_flac_lpc_guard_host    out[v] = flac_lpc_guard(mask[v], q[v], shift[v], bps[v]) for n vectors; q[v] is
 *                                     [(m - 1) * 8 + j], shift[v] is [m - 1]
 *   sauAmd_kat_flac_lpc_guard_device  the same on the device, as flac_analyze_lpc (k_flac.h) calls it: workgroups of 256,
 *                                     lane 0 of each of the four waves takes one vector, whose q and shift lie in LDS laid out
 *                                     like that kernel's FlacLpcLds; 1, or 0 when a HIP call failed */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../saugns_amd/csrc/sau_flac.h"

#define HOOK extern "C" __attribute__((visibility("default")))

using namespace sauflac;

HOOK int sauAmd_kat_flac_lpc_guard_host(const uint32_t *mask, const int16_t *q, const uint8_t *shift, const uint32_t *bps, uint32_t n, uint32_t *out) {
	if (n && (!mask || !q || !shift || !bps || !out)) return 0;
	for (uint32_t v = 0; v < n; ++v)
		out[v] = flac_lpc_guard(mask[v], q + (size_t)v * FLAC_LPC_MAX * FLAC_LPC_MAX, shift + (size_t)v * FLAC_LPC_MAX, bps[v]);
	return 1;
}

struct KatGuardLds {
	int16_t q[4][FLAC_LPC_MAX * FLAC_LPC_MAX];
	uint8_t shift[4][FLAC_LPC_MAX];
	uint32_t mask[4];
};
__global__ __launch_bounds__(256) void kat_flac_lpc_guard_kernel(const uint32_t *mask, const int16_t *q, const uint8_t *shift, const uint32_t *bps,
		uint32_t n, uint32_t *out) {
	__shared__ KatGuardLds L;
	const unsigned c = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const uint32_t v = blockIdx.x * 4 + c;
	if (v < n) {
		L.q[c][lane] = q[(size_t)v * 64 + lane];
		if (lane < FLAC_LPC_MAX) L.shift[c][lane] = shift[(size_t)v * FLAC_LPC_MAX + lane];
	}
	__syncthreads();
	if (lane == 0 && v < n) L.mask[c] = flac_lpc_guard(mask[v], L.q[c], L.shift[c], bps[v]);
	__syncthreads();
	if (lane == 0 && v < n) out[v] = L.mask[c];
}

HOOK int sauAmd_kat_flac_lpc_guard_device(const uint32_t *mask, const int16_t *q, const uint8_t *shift, const uint32_t *bps, uint32_t n, uint32_t *out) {
	if (!n) return 1;
	if (!mask || !q || !shift || !bps || !out) return 0;
	const size_t nb[5] = {n * sizeof(uint32_t), (size_t)n * 64 * sizeof(int16_t), (size_t)n * 8, n * sizeof(uint32_t), n * sizeof(uint32_t)};
	const void *src[5] = {mask, q, shift, bps, out};
	void *d[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
	bool ok = true;
	for (int i = 0; i < 5 && ok; ++i)
		ok = hipMalloc(&d[i], nb[i]) == hipSuccess && hipMemcpy(d[i], src[i], nb[i], hipMemcpyHostToDevice) == hipSuccess;
	if (ok) {
		hipLaunchKernelGGL(kat_flac_lpc_guard_kernel, dim3((n + 3) / 4), dim3(256), 0, 0, (const uint32_t *)d[0], (const int16_t *)d[1],
			(const uint8_t *)d[2], (const uint32_t *)d[3], n, (uint32_t *)d[4]);
		ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess;
	}
	ok = ok && hipMemcpy(out, d[4], nb[4], hipMemcpyDeviceToHost) == hipSuccess;
	for (int i = 0; i < 5; ++i)
		if (d[i]) (void)hipFree(d[i]);
	return ok ? 1 : 0;
}
