/* hip_backend.hip -- gfx950 kernels and the HIP backend of the generator.
 *
 * One translation unit (the kernels share parameter blocks and inlined helpers), in parts:
 *   k_common.h      parameter blocks of the block loop, wave-level helpers (DPP scans, look-back words)
 *   k_block_loop.h  render_kernel<W,T,V>
 *   k_fast_types.h  FastParams, FastInfo, constants of the time-parallel path
 *   k_analyze.h     analyze_kernel
 *   k_decode.h      FastStep / FastLine / FastAux / ChainDesc, scan_kernel, decode_kernel
 *   k_fast_voice.h  fast_voice, fast_kernel<T,SCAN>, repair_kernel<T>
 *   k_chain.h       chain_kernel
 *   k_finish.h      finalize_kernel, mix_kernel, mix_few_kernel (int16 and float32 forms), event_kernel
 *   k_levels.h      levels_kernel, levels_finish_kernel (level metering), requant_kernel (the normalised file writer)
 *   k_decimate.h    decimate_kernel, decimate_carry_kernel (oversampled rendering: the decimating FIR and its history)
 *   k_loudness.h    loud_chunk_kernel, loud_scan_kernel, truepeak_kernel, loud_finish_kernel, loud_carry_kernel (BS.1770 loudness, true peak)
 *   k_limiter.h     lim_env_kernel, lim_gain_kernel, lim_finish_kernel, lim_carry_kernel (the look-ahead true-peak limiter)
 *   k_spectrum.h    spec_segment_kernel, spec_finish_kernel, spec_carry_kernel (Welch power spectra of fed rows)
 *   k_flac.h        flac_analyze_kernel, flac_scan_kernel, flac_write_kernel, flac_carry_kernel (FLAC frames of fed rows, built
 *                   for int16 and for int32 samples: FlacS16, FlacS32; the <.., true> builds of the first and the third
 *                   hold the LPC mode), flac_quant_kernel (a float-fed encoder's rows)
 *   k_flac_dec.h    flac_decode_kernel (a frame of the encoder's back into samples, stored or held against the originals: the
 *                   verify mode; opt-in)
 *   k_md5.h         flac_md5_kernel, flac_md5_wide_kernel (the MD5 of an encoder's unencoded samples, a wave per row; opt-in)
 *   k_dither.h      dither_flat_kernel, dither_shape_kernel (the 16-bit quantiser stage: TPDF dither, error-feedback noise shaping)
 *   launch_plan.h   (plain C++, no HIP) the tuning switches and every decision about a segment's launches: rows per pass, LDS
 *                   budgets, builds, grids, tasks, chain chunks, the mixer -- a plan per segment, testable without a GPU
 *   mix_overlap.h   (plain C++, no HIP) where the main stream waits for a final mixer that runs on the side stream
 *   (this file)     buffer and stream pools, table sets, the kernel lookup, HipBackendImpl: render() carries a plan out,
 *                   stage by stage in the launch order of DESIGN.md 2
 *
 * Work decomposition (DESIGN.md "Kernels"):
 *   render_kernel<W,T>  one workgroup (W waves) per live voice.  The voice's
 *       operator states (256 B each) and all block buffers live in LDS for
 *       the whole segment; Hermite coefficient tables of the wave types in
 *       use are staged into LDS once per workgroup.  Time runs in blocks of
 *       W*(64T-1) samples; inside a block every lane owns T consecutive
 *       samples, so the differentiator's "previous sample" is in-lane except
 *       at lane boundaries (one cross-lane shuffle) and wave boundaries (one
 *       overlapping halo sample per wave instead of an exchange).  Phase
 *       accumulation is an exact integer prefix scan (wave shuffles + one LDS
 *       exchange).  The only serial code is the feedback recurrence of
 *       self-modulating operators and the rare dphase==0 fill-forward.
 *       Each voice's carrier block goes to HBM once (f32 [voice][frame]).
 *   mix_kernel  one thread per output frame sums the voices of its stream in
 *       ascending voice order (the reference's f32 accumulation order,
 *       generator.c:749-788) and writes int16 PCM (795-825) -- or, on a float32
 *       run (engine.h: SampleFormat), the sum as it stands.
 *   event_kernel  applies operator updates to the state in HBM.
 *
 * Arithmetic: sau_dev_math.h, compiled with -ffp-contract=off.
 */
#include <hip/hip_runtime.h>
#include "hip_backend.h"
#include "launch_plan.h"
#include "sau_dev_ops.h"
#include "sau_md5.h"
#include "sau_flac_dec.h"
#include <float.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

namespace sauhip {

using namespace saudev;
using sauengine::BackendConfig;
using sauengine::tune_env;
using sauengine::SegmentDesc;
using namespace sauplan;

/* ------------------------------------------------------------------------ */
/* device side                                                              */
/* ------------------------------------------------------------------------ */
#include "k_common.h"
#include "k_block_loop.h"
#include "k_fast_types.h"
#include "k_analyze.h"
#include "k_decode.h"
#include "k_fast_voice.h"
#include "k_chain.h"
#include "k_finish.h"
#include "k_levels.h"
#include "k_decimate.h"
#include "k_loudness.h"
#include "k_limiter.h"
#include "k_spectrum.h"
#include "k_flac.h"
#include "k_md5.h"
#include "k_flac_dec.h"
#include "k_dither.h"
static_assert(MISC_BYTES == sizeof(Misc), "launch_plan.h plans the block loop's LDS with this size");

/* ------------------------------------------------------------------------ */
/* host side                                                                */
/* ------------------------------------------------------------------------ */

#define HIP_OK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { \
	err = std::string(#call) + ": " + hipGetErrorString(e_); return false; } } while (0)

/* Device and page-locked buffers are recycled through a process-wide pool: a host that renders one
 * script after another (saugns.c:583-621 once per script) would otherwise pay about twenty
 * hipMalloc/hipFree pairs, each a device-wide synchronisation, per generator. Blocks are handed
 * back only after the owning stream has drained (the destructor and grow() see to that). */
class BufPool {
public:
	static BufPool &get() { static BufPool *g = new BufPool; return *g; } /* never destroyed: HIP may be gone by then */
	static size_t bucket(size_t bytes) {
		size_t b = 4096;
		while (b * 2 <= bytes) b <<= 1;
		const size_t q = b / 8; /* eight size classes per octave */
		return (bytes + q - 1) / q * q;
	}
	void *take(bool pinned, size_t bytes) {
		int dev = 0;
		(void)hipGetDevice(&dev);
		std::lock_guard<std::mutex> lk(mu_);
		auto &m = pinned ? pin_ : dev_[dev & 15];
		auto it = m.find(bytes);
		if (it == m.end()) return nullptr;
		void *q = it->second;
		m.erase(it);
		(pinned ? held_pin_ : held_dev_) -= bytes;
		return q;
	}
	/* false: the pool is full, the caller frees the block */
	bool give(bool pinned, void *q, size_t bytes) {
		int dev = 0;
		(void)hipGetDevice(&dev);
		std::lock_guard<std::mutex> lk(mu_);
		size_t &held = pinned ? held_pin_ : held_dev_;
		/* what the pool may keep between generators: 64 GiB of the 288 GB of HBM, 1 GiB page-locked;
		 * SAU_AMD_POOL_MB / SAU_AMD_PINNED_POOL_MB set other caps (0: keep nothing) */
		static const size_t cap_dev = env_mb("SAU_AMD_POOL_MB", (size_t)64 << 10);
		static const size_t cap_pin = env_mb("SAU_AMD_PINNED_POOL_MB", (size_t)1 << 10);
		if (held + bytes > (pinned ? cap_pin : cap_dev)) return false;
		(pinned ? pin_ : dev_[dev & 15]).emplace(bytes, q);
		held += bytes;
		return true;
	}
	/* an allocation has failed: give the runtime back everything the pool holds for this device (or of page-locked memory) */
	size_t trim(bool pinned) {
		int dev = 0;
		(void)hipGetDevice(&dev);
		std::multimap<size_t, void *> out;
		{
			std::lock_guard<std::mutex> lk(mu_);
			out.swap(pinned ? pin_ : dev_[dev & 15]);
			for (auto &b : out) (pinned ? held_pin_ : held_dev_) -= b.first;
		}
		size_t n = 0;
		for (auto &b : out) { if (pinned) (void)hipHostFree(b.second); else (void)hipFree(b.second); n += b.first; }
		return n;
	}
private:
	static size_t env_mb(const char *name, size_t def_mb) {
		const char *v = getenv(name);
		return (v ? (size_t)atoll(v) : def_mb) << 20;
	}
	std::mutex mu_;
	std::multimap<size_t, void *> dev_[16], pin_;
	size_t held_dev_ = 0, held_pin_ = 0;
};

/* Streams too: creating one sets up a hardware queue, milliseconds on this runtime. */
class StreamPool {
public:
	static StreamPool &get() { static StreamPool *g = new StreamPool; return *g; }
	/* `kind` 1: the streams feedback chains run on (created with high priority: see chain_stream_) */
	hipStream_t take(int dev, int kind = 0) {
		std::lock_guard<std::mutex> lk(mu_);
		auto &v = free_[kind & 1][dev & 15];
		if (v.empty()) return nullptr;
		hipStream_t s = v.back();
		v.pop_back();
		return s;
	}
	void give(int dev, hipStream_t s, int kind = 0) {
		std::lock_guard<std::mutex> lk(mu_);
		auto &v = free_[kind & 1][dev & 15];
		if (v.size() < 8) v.push_back(s); else (void)hipStreamDestroy(s);
	}
private:
	std::mutex mu_;
	std::vector<hipStream_t> free_[2][16];
};

/* Launches of the single-pass running-sum build whose voices have waves in more than one workgroup wait for each
 * other's sums across workgroups. One such launch alone always finishes (its workgroups are dispatched in order and
 * a voice's lie next to each other, so what a blocked workgroup waits for is the next to get a CU), two at once
 * from different generators could hold each other's CUs: within the process they take turns, through an event
 * chain per device. (Launches whose voices each sit inside one workgroup need none of this.) */
class SpreadLaunchOrder {
public:
	static SpreadLaunchOrder &get() { static SpreadLaunchOrder *g = new SpreadLaunchOrder; return *g; }
	/* `launch` enqueues the kernel on `stream`; it runs after the device's previous such launch has finished */
	template <typename F> bool ordered(int dev, hipStream_t stream, F launch) {
		std::lock_guard<std::mutex> lk(mu_);
		Dev &d = dev_[dev & 15];
		if (d.last && hipStreamWaitEvent(stream, d.last, 0) != hipSuccess) return false;
		if (!launch()) return false;
		hipEvent_t &e = d.ring[d.next++ & 63];
		if (!e && hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return false;
		if (hipEventRecord(e, stream) != hipSuccess) return false;
		d.last = e; /* (a wait captures the event's state when it is enqueued: re-recording it 64 launches on is harmless) */
		return true;
	}
private:
	struct Dev { hipEvent_t ring[64] = {}; hipEvent_t last = nullptr; unsigned next = 0; };
	std::mutex mu_;
	Dev dev_[16];
};

static void *pool_alloc(bool pinned, size_t &bytes, std::string &err) {
	bytes = BufPool::bucket(bytes);
	void *q = BufPool::get().take(pinned, bytes);
	if (q) return q;
	hipError_t e = pinned ? hipHostMalloc(&q, bytes, hipHostMallocDefault) : hipMalloc(&q, bytes);
	if (e != hipSuccess) {
		/* The failed call's error stays the thread's "last error" (successful calls do not clear it on this runtime):
		 * consume it, or the hipGetLastError() checks behind later launches report this allocation against them -- a
		 * caller that has a way on without the block (the block loop in place of the chains' rows) would fail anyway.
		 * Then once more with the pool's idle blocks given back to the runtime. */
		(void)hipGetLastError();
		if (BufPool::get().trim(pinned)) {
			e = pinned ? hipHostMalloc(&q, bytes, hipHostMallocDefault) : hipMalloc(&q, bytes);
			if (e == hipSuccess) return q;
			(void)hipGetLastError();
		}
		err = std::string(pinned ? "hipHostMalloc: " : "hipMalloc: ") + hipGetErrorString(e);
		return nullptr;
	}
	return q;
}
static void pool_free(bool pinned, void *q, size_t bytes) {
	if (!q) return;
	if (!BufPool::get().give(pinned, q, bytes)) { if (pinned) (void)hipHostFree(q); else (void)hipFree(q); }
}

/* hipFuncSetAttribute(MaxDynamicSharedMemorySize) is per device and kernel, remembered here per (kernel, device): generators
 * driven from different host threads share the slots, so check-then-raise runs under one lock (values only ever grow) */
static std::mutex &attr_mutex() { static std::mutex *m = new std::mutex; return *m; }
static bool raise_lds_attr(const void *fn, size_t lds, int dev, std::string &err) {
	static std::map<std::pair<const void *, int>, size_t> *slots = new std::map<std::pair<const void *, int>, size_t>;
	std::lock_guard<std::mutex> lk(attr_mutex());
	size_t &configured = (*slots)[std::make_pair(fn, dev & 15)];
	if (lds > configured) {
		hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
		if (e != hipSuccess) { err = std::string("hipFuncSetAttribute: ") + hipGetErrorString(e); return false; }
		configured = lds;
	}
	return true;
}

/* Which instantiation a launch takes: the one place that names them. A (build, rows, form) without an instantiation is
 * NULL -- an error for the caller, never another kernel beside slots laid out for `rows`.
 * fast_kernel builds -- 0: closed-form phases only; 1: every kind of running-sum voice; 2: single-pass (look-back) voices;
 * 3: voices with feedback chains and nothing to scan (4, 5 or 6 rows per pass; 6 spills 170 VGPRs and is still the fastest on
 * config 5 -- 52.3 against 53.1 ms per step at 5; the 8-row instantiation, 298 spilled, is gone since round 4, like the full
 * build's 8-row one). Forms: wide table blocks in LDS (k_fast_types.h: FkTab -- the closed-form build at 6, 8, 10 and 12 rows,
 * the look-back build at 8: round 5, where the lean buffer numbering leaves LDS for them), the look-back build that mixes
 * few-voice streams (round 6: FastParams.tail_ok), the builds with the loop tails of `cub` R segments, the inner launch of the
 * 12-row build (k_fast_voice.h: INNER), its lane-major form (k_fast_group_lm.h) and that form for launches of one table
 * (round 10: fk_entry's TAB0; only in a -DFK_LM_TAB0=1 build -- by default every launch takes the form that adds the table's base),
 * and the lane-major form for launches of wave oscillators with constant amplitude only (round 11: fast_kernel's WONLY).
 * (The table's order is the order the instantiations take in the code object.) */
enum : unsigned { FK_WIDE = 1, FK_TAIL = 2, FK_CUB = 4, FK_INNER = 8, FK_LANEMAJOR = 16, FK_TAB0 = 32, FK_WONLY = 64 };
static const void *fast_kernel_fn(int build, uint32_t rows, unsigned form) {
	struct Entry { int build; uint32_t rows; unsigned form; const void *fn; };
#define FK(build, form, ...) {build, FK_ROWS(__VA_ARGS__), form, (const void *)fast_kernel<__VA_ARGS__>}
#define FK_ROWS(rows, ...) rows
	static const Entry table[] = {
		FK(0, 0, 2, 0), FK(0, 0, 4, 0), FK(0, 0, 5, 0), FK(0, 0, 6, 0), FK(0, 0, 8, 0),
		FK(1, 0, 2, 1), FK(1, 0, 4, 1),
		FK(2, 0, 2, 2), FK(2, 0, 4, 2), FK(2, 0, 5, 2), FK(2, 0, 6, 2), FK(2, 0, 8, 2),
		FK(3, 0, 4, 3), FK(3, 0, 5, 3), FK(3, 0, 6, 3),
		FK(0, FK_WIDE, 6, 0, false, true), FK(0, FK_WIDE, 8, 0, false, true), FK(0, FK_WIDE, 10, 0, false, true), FK(0, FK_WIDE, 12, 0, false, true),
		FK(2, FK_WIDE | FK_TAIL, 8, 2, false, true, true), FK(2, FK_WIDE, 8, 2, false, true), FK(2, FK_TAIL, 8, 2, false, false, true),
		FK(2, FK_CUB, (int)FAST_CUB_ROWS, 2, true),
		FK(0, FK_WIDE | FK_INNER | FK_LANEMAJOR, 12, 0, false, true, false, true, true), FK(0, FK_WIDE | FK_INNER, 12, 0, false, true, false, true),
#if FK_LM_TAB0
		FK(0, FK_WIDE | FK_INNER | FK_LANEMAJOR | FK_TAB0, 12, 0, false, true, false, true, true, true),
#endif
#if FK_LM_WONLY
		FK(0, FK_WIDE | FK_INNER | FK_LANEMAJOR | FK_WONLY, 12, 0, false, true, false, true, true, false, true),
#endif
		FK(0, FK_CUB, (int)FAST_CUB_ROWS, 0, true)};
#undef FK
#undef FK_ROWS
	for (const Entry &e : table)
		if (e.build == build && e.rows == rows && e.form == form) return e.fn;
	return nullptr;
}
#if FK_LM_TAB0
/* fk_entry's TAB0 form reads the table at LDS address 0: only while the kernel has no static __shared__ ahead of its dynamic block */
static bool tab0_kernel_ok(const void *fn) {
	static const bool ok = [&] { hipFuncAttributes a; return fn && hipFuncGetAttributes(&a, fn) == hipSuccess && a.sharedSizeBytes == 0; }();
	return ok;
}
#endif
static const void *repair_kernel_fn(uint32_t rows, bool wide) {
	if (wide)
		return rows == 12 ? (const void *)repair_kernel<12, true> : rows == 10 ? (const void *)repair_kernel<10, true>
		     : rows == 8 ? (const void *)repair_kernel<8, true> : rows == 6 ? (const void *)repair_kernel<6, true> : nullptr;
	return rows == 8 ? (const void *)repair_kernel<8> : rows == 6 ? (const void *)repair_kernel<6> : rows == 5 ? (const void *)repair_kernel<5>
	     : rows == 4 ? (const void *)repair_kernel<4> : rows == 2 ? (const void *)repair_kernel<2> : nullptr;
}
/* render_kernel<W, T, V, HB>: W waves x T frames per lane on one voice, or V single-wave teams, or (HB) block buffers in HBM */
static const void *render_kernel_fn(uint32_t W, uint32_t T, uint32_t V, bool HB) {
	struct Entry { uint32_t W, T, V; bool HB; const void *fn; };
#define RK(W, T, V, HB) {W, T, V, HB, (const void *)render_kernel<W, T, V, HB>}
	static const Entry table[] = {
		RK(1, 4, 8, false), RK(1, 3, 8, false), RK(1, 2, 8, false), RK(1, 1, 8, false),
		RK(1, 4, 16, false), RK(1, 3, 16, false), RK(1, 2, 16, false), RK(1, 1, 16, false),
		RK(1, 1, 1, true), RK(1, 1, 1, false), RK(4, 4, 1, false), RK(8, 2, 1, false)};
#undef RK
	for (const Entry &e : table)
		if (e.W == W && e.T == T && e.V == V && e.HB == HB) return e.fn;
	return nullptr;
}

template <typename T, bool PINNED> struct PoolBuf {
	T *p = nullptr;
	size_t cap = 0, bytes = 0;
	PoolBuf() = default;
	PoolBuf(const PoolBuf &) = delete;
	PoolBuf &operator=(const PoolBuf &) = delete;
	~PoolBuf() { release(); }
	/* growing replaces the block: the caller has drained the stream that used the old one */
	bool ensure(size_t n, std::string &err, bool keep = false) {
		if (n <= cap) return true;
		size_t nbytes = (n + n / 4 + 16) * sizeof(T);
		T *q = (T *)pool_alloc(PINNED, nbytes, err);
		if (!q) return false;
		if (keep && p && cap) {
			hipError_t e = PINNED ? (memcpy(q, p, cap * sizeof(T)), hipSuccess)
			                      : hipMemcpy(q, p, cap * sizeof(T), hipMemcpyDeviceToDevice);
			if (e != hipSuccess) { err = hipGetErrorString(e); return false; }
		}
		if (p) { (void)hipDeviceSynchronize(); pool_free(PINNED, p, bytes); }
		p = q; bytes = nbytes; cap = nbytes / sizeof(T);
		return true;
	}
	void release() { pool_free(PINNED, p, bytes); p = nullptr; cap = 0; bytes = 0; }
};
template <typename T> using DevBuf = PoolBuf<T, false>;
template <typename T> using PinBuf = PoolBuf<T, true>; /* page-locked staging for async copies */

/* Hermite coefficient tables (sau/wave.h:127-141 evaluated per table entry) are a function of the
 * PILUTs alone: built and uploaded once per device and table set, shared by every generator. */
struct TableSet {
	int dev;
	std::vector<float> piluts;
	WaveConst wconst[12];
	HerpC23 *c23;
	HerpC01 *c01;
	WaveConst *wc;
};
static const TableSet *shared_tables(const float *piluts, const WaveConst *wconst, std::string &err) {
	static std::mutex mu;
	static std::vector<TableSet *> sets;
	int dev = 0;
	(void)hipGetDevice(&dev);
	std::lock_guard<std::mutex> lk(mu);
	for (const TableSet *t : sets)
		if (t->dev == dev && !memcmp(t->piluts.data(), piluts, (size_t)12 * WAVE_LEN * sizeof(float)) &&
		    !memcmp(t->wconst, wconst, sizeof t->wconst))
			return t;
	std::vector<HerpC23> h23((size_t)12 * WAVE_LEN);
	std::vector<HerpC01> h01((size_t)12 * WAVE_LEN);
	for (uint32_t wv = 0; wv < 12; ++wv)
		for (uint32_t i = 0; i < WAVE_LEN; ++i) {
			if (!herp_c1_scalable(piluts + (size_t)wv * WAVE_LEN, i)) {
				err = "wave table has slopes below 2^-100: unsupported";
				return nullptr;
			}
			herp_coeffs(piluts + (size_t)wv * WAVE_LEN, i,
					h23[(size_t)wv * WAVE_LEN + i], h01[(size_t)wv * WAVE_LEN + i]);
		}
	TableSet *t = new TableSet;
	t->dev = dev;
	t->piluts.assign(piluts, piluts + (size_t)12 * WAVE_LEN);
	memcpy(t->wconst, wconst, sizeof t->wconst);
	t->c23 = nullptr; t->c01 = nullptr; t->wc = nullptr;
	hipError_t e = hipMalloc((void **)&t->c23, h23.size() * sizeof(HerpC23));
	if (e == hipSuccess) e = hipMalloc((void **)&t->c01, h01.size() * sizeof(HerpC01));
	if (e == hipSuccess) e = hipMalloc((void **)&t->wc, 12 * sizeof(WaveConst));
	if (e == hipSuccess) e = hipMemcpy(t->c23, h23.data(), h23.size() * sizeof(HerpC23), hipMemcpyHostToDevice);
	if (e == hipSuccess) e = hipMemcpy(t->c01, h01.data(), h01.size() * sizeof(HerpC01), hipMemcpyHostToDevice);
	if (e == hipSuccess) e = hipMemcpy(t->wc, wconst, 12 * sizeof(WaveConst), hipMemcpyHostToDevice);
	if (e != hipSuccess) {
		err = std::string("wave tables: ") + hipGetErrorString(e);
		(void)hipFree(t->c23); (void)hipFree(t->c01); (void)hipFree(t->wc);
		delete t;
		return nullptr;
	}
	sets.push_back(t); /* generators keep plain pointers: sets live as long as the process (0.6 MB each) */
	return t;
}

int device_count() {
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess) return 0;
	return n;
}

bool device_pci_bus_id(int dev, char *buf, int len) {
	if (!buf || len < 16) return false;
	buf[0] = 0;
	return hipDeviceGetPCIBusId(buf, len, dev) == hipSuccess;
}

class HipBackendImpl : public HipBackend {
public:
	explicit HipBackendImpl(int device = -1) : want_dev_(device) {}
	/* every entry point runs on this backend's device, whatever the host thread's current one is
	 * (another generator on another GPU, torch.cuda.set_device): allocations, the pools (keyed by
	 * the current device) and launches all follow it */
	void use_device() { (void)hipSetDevice(dev_); }

	/* ---- the final mixer's side stream (mix_overlap.h has the rules; launch_mixer puts the mixer there) ----
	 * Every override of Backend joins the pending mixer as its first action -- join_mixer(), a wait on the main stream, nothing
	 * the host blocks on -- so that a method added later is ordered behind the mixer by default. Those that do not:
	 *   render                         asks the tracker at the points mix_overlap.h names
	 *   upload_plans, apply_updates    write plans and operator records, which no mixer reads
	 *   reserve_frames, set_format     join only when they change something (the rows' size, the samples' format)
	 *   zero_pcm                       joins once it knows that it has frames to clear
	 *   chain_rows_budget, alloc_host, free_host, wait_fetch   touch nothing on the device that a mixer uses */
	/* the main stream waits for mixer `t` (0: for nothing); `where`: for SAU_AMD_OVERLAP_REPORT */
	bool wait_mixer(uint64_t t, const char *where, std::string &err) {
		if (!t) return true;
		hipEvent_t done = mix_done_[MixOverlapTracker::slot(t)];
		if (overlap_report_) { /* (had it finished already? asked only for the report) */
			const bool was_done = hipEventQuery(done) == hipSuccess;
			report_waits_ += std::string(" ") + where + ":" + std::to_string(t) + (was_done ? ":done" : ":busy");
		}
		HIP_OK(hipStreamWaitEvent(stream_, done, 0));
		return true;
	}
	bool join_mixer(const char *where, std::string &err) { return wait_mixer(mixo_.join(), where, err); }
	void join_mixer_quiet(const char *where) { std::string e; (void)join_mixer(where, e); }
	bool ensure_mix_stream(std::string &err) {
		if (mix_ready_) return true;
		/* from the chain streams' pool, high priority as they are: a queue of another priority is never the main stream's
		 * (launch_chains), and two streams on one hardware queue would run the mixer behind the set-up launches after all */
		if (!mix_stream_) mix_stream_ = StreamPool::get().take(dev_, 1);
		if (!mix_stream_) {
			int lo = 0, hi = 0;
			(void)hipDeviceGetStreamPriorityRange(&lo, &hi);
			HIP_OK(hipStreamCreateWithPriority(&mix_stream_, hipStreamNonBlocking, hi));
		}
		for (uint32_t i = 0; i < MIXO_RING; ++i) { /* (a call that failed midway is taken up where it stopped) */
			if (!mix_fork_[i]) HIP_OK(hipEventCreateWithFlags(&mix_fork_[i], hipEventDisableTiming));
			if (!mix_done_[i]) HIP_OK(hipEventCreateWithFlags(&mix_done_[i], hipEventDisableTiming));
		}
		mix_ready_ = true;
		return true;
	}

	~HipBackendImpl() override {
		use_device();
		/* the buffers go back to the pool (member destructors): nothing may still be using them */
		if (stream_) { join_mixer_quiet("destroy"); (void)hipStreamSynchronize(stream_); }
		if (mix_stream_) { (void)hipStreamSynchronize(mix_stream_); StreamPool::get().give(dev_, mix_stream_, 1); }
		for (uint32_t i = 0; i < MIXO_RING; ++i) {
			if (mix_fork_[i]) (void)hipEventDestroy(mix_fork_[i]);
			if (mix_done_[i]) (void)hipEventDestroy(mix_done_[i]);
		}
		if (chain_stream_) { (void)hipStreamSynchronize(chain_stream_); StreamPool::get().give(dev_, chain_stream_, 1); }
		for (hipEvent_t e : chain_ev_) (void)hipEventDestroy(e);
		for (int i = 0; i < 4; ++i) if (fetch_ev_[i]) (void)hipEventDestroy(fetch_ev_[i]);
		if (after_ev_) (void)hipEventDestroy(after_ev_);
		for (auto &e : events_) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
		if (stream_) StreamPool::get().give(dev_, stream_); /* drained above */
	}

	bool init(const BackendConfig &cfg, std::string &err) override {
		cfg_ = cfg;
		int dev = 0;
		const char *env = getenv("SAU_AMD_DEVICE");
		if (want_dev_ >= 0) dev = want_dev_; /* (sauAmd_create_Batch_on: the caller's choice goes before the environment's) */
		else if (env) dev = atoi(env);
		if (dev < 0 || dev >= device_count()) { err = "no HIP device " + std::to_string(dev) + " (" + std::to_string(device_count()) + " visible)"; return false; }
		HIP_OK(hipSetDevice(dev));
		dev_ = dev;
		stream_ = StreamPool::get().take(dev);
		if (!stream_) HIP_OK(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
		static std::mutex prop_mu;
		static size_t dev_lds[16]; /* per device: hipGetDeviceProperties costs a millisecond */
		static uint32_t dev_cus[16];
		static size_t dev_free[16]; /* bytes free when the process first opened the device: the chain rows' budget follows it */
		{
			std::lock_guard<std::mutex> lk(prop_mu);
			if (!dev_lds[dev & 15]) {
				hipDeviceProp_t prop;
				HIP_OK(hipGetDeviceProperties(&prop, dev));
				dev_lds[dev & 15] = prop.maxSharedMemoryPerMultiProcessor ? prop.maxSharedMemoryPerMultiProcessor
				                                                          : prop.sharedMemPerBlock;
				dev_cus[dev & 15] = prop.multiProcessorCount > 0 ? (uint32_t)prop.multiProcessorCount : FK_GRID;
				size_t mfree = 0, mtotal = 0; /* the budget of the feedback chains' rows follows what this device has free */
				if (hipMemGetInfo(&mfree, &mtotal) == hipSuccess) dev_free[dev & 15] = mfree;
			}
			free_hint_ = dev_free[dev & 15];
			tun_ = tuning_from_env(tune_env);
			lim_ = device_limits(dev_lds[dev & 15], dev_cus[dev & 15], tun_); /* (launch_plan.h: what the device's CUs mean for grids and queues) */
		}
		debug_ = getenv("SAU_AMD_DEBUG") != nullptr;
		inmix_report_ = tune_env("SAU_AMD_INMIX_REPORT") != nullptr;
		inner_report_ = tune_env("SAU_AMD_INNER_REPORT") != nullptr; /* (tests: which form the inner launch took) */
		overlap_report_ = tune_env("SAU_AMD_OVERLAP_REPORT") != nullptr; /* (tests: where the final mixer ran and what waited for it) */
		if (!ops_.ensure(cfg.op_count ? cfg.op_count : 1, err)) return false;
		HIP_OK(hipMemsetAsync(ops_.p, 0, ops_.cap * sizeof(DevOp), stream_));
		tables_ = shared_tables(cfg.piluts, cfg.wconst, err);
		if (!tables_) return false;
		memcpy(wconst_, cfg.wconst, sizeof wconst_);
		return true;
	}

	bool reserve_frames(uint32_t max_frames, bool /* stereo: the rows have room for it either way */, std::string &err) override {
		use_device();
		if (!join_mixer("reserve_frames", err)) return false; /* (the rows and the PCM block are sized anew) */
		HIP_OK(hipStreamSynchronize(stream_));
		row_stride_ = (max_frames + 63) & ~63u;
		pcm_row_ = (size_t)row_stride_ * 2; /* room for stereo */
		/* (not cleared: every frame of a run is written by a mixer or cleared by zero_pcm, and no frame behind a run's
		 * length is ever handed out -- until round 6 a memset here, 32 us for a config-4 batch's 677 MB) */
		if (!pcm_.ensure(pcm_row_ * cfg_.n_streams * pcm_units(), err)) return false;
		sets_[0].vout_rows = sets_[1].vout_rows = 0; /* re-sized on the next render */
		return true;
	}

	/* The PCM block holds a row of pcm_row_ samples per stream in the format of the run at hand: int16, or float32 (engine.h:
	 * SampleFormat) at twice the bytes. A run of the other format than the last one says so first; the block grows (and may
	 * move) when the float rows do not fit it -- every MixStream record is then sent again, its row pointer has changed. */
	size_t pcm_units() const { return pcm_f32_ ? 2 : 1; } /* int16 units per sample */
	size_t pcm_pitch() const { return pcm_row_ * pcm_units() * sizeof(int16_t); } /* bytes from a stream's row to the next one's */
	char *pcm_at(uint32_t stream) const { return (char *)pcm_.p + pcm_pitch() * stream; }
	bool set_format(sauengine::SampleFormat fmt, std::string &err) override {
		use_device();
		const bool f32 = fmt == sauengine::SF_F32;
		if (f32 == pcm_f32_) return true;
		/* (no wait for the host: the last run's copies out of the rows and this run's stores are in order on the main stream --
		 * behind the last run's mixer, which is joined here -- and a block that moves is freed only once the device has
		 * drained -- DevBuf::ensure) */
		if (!join_mixer("set_format", err)) return false;
		pcm_f32_ = f32;
		if (pcm_row_ && !pcm_.ensure(pcm_row_ * cfg_.n_streams * pcm_units(), err)) { pcm_f32_ = !f32; return false; }
		return true;
	}

	/* Host data for the device goes through a page-locked arena and asynchronous copies on the
	 * generator's stream: the copies are ordered behind the kernels still reading the old
	 * contents, and the host goes on to prepare the next segment instead of waiting (a script
	 * with many events is a chain of short segments). The arena is reused from its start once
	 * the stream has drained. */
	void *stage(const void *src, size_t bytes, std::string &err) {
		const size_t need = (bytes + 63) & ~(size_t)63;
		if (arena_used_ + need > arena_.cap) {
			hipError_t e = hipStreamSynchronize(stream_);
			if (e != hipSuccess) { err = std::string("hipStreamSynchronize: ") + hipGetErrorString(e); return nullptr; }
			arena_used_ = 0;
			const size_t want = need > ((size_t)4 << 20) ? need : ((size_t)4 << 20);
			if (want > arena_.cap && !arena_.ensure(want, err)) return nullptr;
		}
		void *p = arena_.p + arena_used_;
		arena_used_ += need;
		memcpy(p, src, bytes);
		return p;
	}
	bool send(void *dst, const void *src, size_t bytes, std::string &err) {
		if (!bytes) return true;
		void *h = stage(src, bytes, err);
		if (!h) return false;
		HIP_OK(hipMemcpyAsync(dst, h, bytes, hipMemcpyHostToDevice, stream_));
		return true;
	}

	bool upload_plans(const Step *steps, const FastIds *fast_ids, size_t n_steps, const uint32_t *op_ids,
			size_t n_ids, std::string &err) override {
		use_device();
		if (!steps_.ensure(n_steps ? n_steps : 1, err) || !op_ids_.ensure(n_ids ? n_ids : 1, err) ||
		    !fast_ids_.ensure(n_steps ? 2 * n_steps : 1, err))
			return false;
		n_steps_total_ = (uint32_t)n_steps;
		return send(steps_.p, steps, n_steps * sizeof(Step), err) &&
			send(fast_ids_.p, fast_ids, 2 * n_steps * sizeof(FastIds), err) &&
			send(op_ids_.p, op_ids, n_ids * sizeof(uint32_t), err);
	}

	bool apply_updates(const OpUpdate *recs, size_t n, std::string &err) override {
		use_device();
		if (!n) return true;
		if (!recs_.ensure(n, err) || !send(recs_.p, recs, n * sizeof(OpUpdate), err)) return false;
		hipLaunchKernelGGL(event_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, stream_,
				ops_.p, recs_.p, (uint32_t)n, tables_->wc);
		HIP_OK(hipGetLastError());
		return true;
	}

	/* (SAU_AMD_POISON, tests) every stream's whole row, the frames behind the run's length included: those are never handed out
	 * and must still read 0x5a5a afterwards. On the one stream, so behind the previous run's fetch_pcm_async copies. */
	bool poison_run(uint32_t frames, bool stereo, std::string &err) override {
		(void)frames; (void)stereo;
		use_device();
		if (!join_mixer("poison_run", err)) return false;
		/* (a float row then reads 0x5a5a5a5a = 1.5e16 per sample: no mix of voices comes near it) */
		if (pcm_.p) HIP_OK(hipMemsetD16Async((hipDeviceptr_t)pcm_.p, 0x5a5a, pcm_row_ * cfg_.n_streams * pcm_units(), stream_));
		return true;
	}

	bool zero_pcm(uint32_t first_stream, uint32_t n_streams, uint32_t first_frame, uint32_t n_frames, bool stereo,
			std::string &err) override {
		use_device();
		if (!pcm_.p || !n_streams || !n_frames) return true;
		if (!join_mixer("zero_pcm", err)) return false;
		const size_t fb = (stereo ? 2 : 1) * pcm_units() * sizeof(int16_t); /* bytes per frame (zero bytes are +0.0f too) */
		char *at = pcm_at(first_stream) + (size_t)first_frame * fb;
		if (n_streams == 1) HIP_OK(hipMemsetAsync(at, 0, (size_t)n_frames * fb, stream_));
		else HIP_OK(hipMemset2DAsync(at, pcm_pitch(), 0, (size_t)n_frames * fb, n_streams, stream_));
		return true;
	}

	/* kind: 0 block-loop kernel, 1 mixer, 2 time-parallel kernel, 3 analyze/finalize */
	struct TimedPair { hipEvent_t a, b; int kind; bool used; };

	/* One render() call: the segment, what launch_plan.h decided for it, and the parameter blocks the stages fill. */
	struct Job {
		const SegmentDesc &seg;
		PlanInputs in;
		BlockLoopPlan bl;
		FastPlan fk;
		RenderParams rp;
		FastParams fp;
		FastParams cfp;       /* the closed-form launch of a split segment (also what the cub build and repair_kernel run with there) */
		bool launched = true; /* false: some launch of the time-parallel path failed (err says which) */
		bool tail_live = false;  /* this segment's look-back launch mixes few-voice streams: mix_few_kernel looks at the set's tail_ok */
		bool inmix_live = false; /* this segment's closed-form launch mixes: mix_kernel looks at the control words */
		uint32_t early_mixed_blocks = 0; /* 256-frame blocks of this segment that early launches have mixed */
		uint32_t block_grid = 1;
		MixOverlap mode = MIXO_OFF; /* where the segment's final mixer runs (launch_plan.h: plan_mix_overlap) */
		uint32_t set = 0;           /* which of the two sets of records the segment's launches use: segment n, set n mod 2 */
		uint32_t block = 0;         /* ... and which block of voice and pan rows: 0, or with rows of its own the set's */
		TimedPair *tf = nullptr;
		explicit Job(const SegmentDesc &s) : seg(s) { memset(&rp, 0, sizeof rp); memset(&fp, 0, sizeof fp); }
	};

	/* What is launched when. The decisions are launch_plan.h's; the stages below carry them out in this order. */
	bool render(const SegmentDesc &seg, std::string &err) override {
		use_device();
		if (!seg.n_voices) return true;
		++acc_launches_; /* segments rendered */
		Job j(seg);
		j.in.f32 = seg.format == sauengine::SF_F32; /* (a float run: set_format has sized the rows) */
		if (j.in.f32 != pcm_f32_) { err = "a segment of another sample format than the run announced"; return false; }
		if (j.in.f32 && seg.swap_bytes) { err = "float32 samples are not byte-swapped"; return false; }
		j.in.row_stride = row_stride_; j.in.pcm_row = pcm_row_; j.in.chain_budget = chain_rows_budget();
		for (uint32_t s = 0; s < seg.n_streams; ++s) { /* (what the plans read of the streams) */
			if (seg.streams[s].write_len > j.in.max_write) j.in.max_write = seg.streams[s].write_len;
			if (seg.streams[s].n_voices > j.in.max_rows) j.in.max_rows = seg.streams[s].n_voices;
		}
		j.fk = plan_fast(seg, tun_, lim_, j.in);
		if (!begin_overlap(j, err)) return false;
		j.bl = plan_block_loop(seg, tun_, lim_);
		if (!j.bl.ok) { err = "voice too large for one workgroup's LDS (block buffers + operator states)"; return false; }
		if (!ensure_rows(j, err) || !upload_descriptors(j, err)) return false;
		/* ---- time-parallel path first; the block loop continues after it ---- */
		if (!prepare_fast(j, err) || !prepare_chains(j, err)) return false;
		fill_tables(j);
		if (!launch_analyze(j, err)) return false;
		if (j.fk.use_fast) {
			if (!launch_decode(j, err)) return false;
			if (j.fk.main_build == 2 && !launch_split(j, err)) return false;
			if (j.fp.scan ? !launch_sums_and_chains(j, err) : !launch_closed_form(j, err)) return false;
			if (!launch_cub(j, err)) return false;
			if (!j.launched) return false;
			if (!launch_repair(j, err)) return false;
			if (j.tf) (void)hipEventRecord(j.tf->b, stream_);
		}
		if (!launch_finalize(j, err)) return false;
		if (!launch_block_loop(j, err)) return false;
		return launch_mixer(j, err);
	}

	/* The segment's set and mode, its block of rows, and the first of its waits: nothing of set s is written before the last mixer
	 * that read set s has finished (two segments ago, normally: no wait then). */
	bool begin_overlap(Job &j, std::string &err) {
		const SegmentDesc &seg = j.seg;
		j.set = mixo_.begin_segment();
		const size_t rows_bytes = ((size_t)seg.n_voices + seg.n_pan_rows) * row_stride_ * sizeof(float);
		j.mode = plan_mix_overlap(tun_, j.in, j.fk, rows_bytes, second_refused_);
		if (j.mode == MIXO_ALTERNATE && j.set == 1 && !second_rows(j)) j.mode = MIXO_SHARED;
		j.block = MixOverlapTracker::block_of(j.mode, j.set);
		if (j.mode != MIXO_OFF && !ensure_mix_stream(err)) return false;
		return wait_mixer(mixo_.before_records(j.set), "records", err);
	}
	/* The second block of voice and pan rows, on the first segment that would use it (and when a later one needs more). When the
	 * device does not give it -- pool_alloc has then consumed the failed call's error -- the two sets share the first block from
	 * here on, for good on this backend. (SAU_AMD_MIX_OVERLAP_FAIL, tests: refused without asking.) */
	bool second_rows(Job &j) {
		const SegmentDesc &seg = j.seg;
		MixSet &R = sets_[1];
		const size_t nv = (size_t)seg.n_voices * row_stride_, np = (size_t)seg.n_pan_rows * row_stride_;
		if (R.vout.p && seg.n_voices <= R.vout_rows && np <= R.pan.cap) return true;
		std::string why = "refused by SAU_AMD_MIX_OVERLAP_FAIL";
		bool ok = !tun_.mix_overlap_fail;
		if (ok && (seg.n_voices > R.vout_rows || !R.vout.p)) {
			if (R.vout.p) { /* (a block that grows is replaced: nothing may still read the old one) */
				join_mixer_quiet("second_rows");
				(void)hipStreamSynchronize(stream_);
			}
			ok = R.vout.ensure(nv, why);
			if (ok) R.vout_rows = seg.n_voices;
		}
		if (ok && np) ok = R.pan.ensure(np, why);
		if (!ok) {
			second_refused_ = true;
			/* (shared rows for good: what was had of the second block goes back. No mixer reads it -- one that did was joined when
			 * it grew, and a fresh block has had none -- and the main stream's launches on it are drained first) */
			if (R.vout.p || R.pan.p) { join_mixer_quiet("second_rows"); (void)hipStreamSynchronize(stream_); (void)hipStreamSynchronize(mix_stream_ ? mix_stream_ : stream_); }
			R.vout.release(); R.pan.release(); R.vout_rows = 0;
			if (debug_) fprintf(stderr, "saugns_amd: no second block of %zu bytes of voice rows (%s): the final mixer's two sets share one\n", nv * sizeof(float), why.c_str());
		}
		return ok;
	}
	/* before the first launch (or memset) of the segment that writes voice or pan rows: the last mixer that read this block */
	bool rows_hazard(Job &j, std::string &err) { return wait_mixer(mixo_.before_rows(j.block), "rows", err); }
	/* before the first launch of the segment that reads or writes PCM: the last mixer */
	bool pcm_hazard(std::string &err) { return wait_mixer(mixo_.before_pcm(), "pcm", err); }

	/* voice rows, pan rows, per-row and per-stream records */
	bool ensure_rows(Job &j, std::string &err) {
		const SegmentDesc &seg = j.seg;
		MixSet &S = sets_[j.set], &R = sets_[j.block];
		if (!voices_.ensure(seg.n_voices, err) || !S.vinfo.ensure(seg.n_voices, err)) return false;
		if (seg.n_voices > R.vout_rows || !R.vout.p) {
			if (!join_mixer("ensure_rows", err)) return false; /* (the block is replaced: its last mixer with everything else) */
			HIP_OK(hipStreamSynchronize(stream_));
			if (!R.vout.ensure((size_t)seg.n_voices * row_stride_, err)) return false;
			R.vout_rows = seg.n_voices;
		}
		if (seg.n_pan_rows && !R.pan.ensure((size_t)seg.n_pan_rows * row_stride_, err)) return false;
		/* (SAU_AMD_POISON, tests) the voice and pan rows before the segment's first launch, with a finite value (about 0.32: a
		 * NaN may come out of the float-to-int16 clamp as 0 and hide the very frames this is meant to show). Nothing in them
		 * outlives a segment: every kernel that reads a row (the mixers, the launches that mix tiles themselves) reads what this
		 * segment's launches stored in it, and what a feedback chain carries over lives in chain_rows_, not here. */
		if (tun_.poison) {
			if (!wait_mixer(mixo_.before_rows(j.block), "poison", err)) return false;
			HIP_OK(hipMemsetD32Async((hipDeviceptr_t)R.vout.p, 0x3ea5a5a5, (size_t)seg.n_voices * row_stride_, stream_));
			if (seg.n_pan_rows) HIP_OK(hipMemsetD32Async((hipDeviceptr_t)R.pan.p, 0x3ea5a5a5, (size_t)seg.n_pan_rows * row_stride_, stream_));
		}
		return S.mstreams.ensure(seg.n_streams, err);
	}

	/* The voice and stream descriptors go through page-locked staging that is reused once the previous segment's copies have
	 * left it. In steady state (no event between two segments) the descriptors repeat: upload only changes. */
	bool upload_descriptors(Job &j, std::string &err) {
		const SegmentDesc &seg = j.seg;
		MixSet &S = sets_[j.set];
		ms_host_.resize(seg.n_streams);
		for (uint32_t s = 0; s < seg.n_streams; ++s) {
			MixStream &m = ms_host_[s];
			memset(&m, 0, sizeof m);
			m.first_row = seg.streams[s].first_voice;
			m.n_rows = seg.streams[s].n_voices;
			m.amp_scale = seg.streams[s].amp_scale;
			m.write_len = seg.streams[s].write_len;
			m.pcm = (int16_t *)pcm_at(s); /* (a row of floats on a float run: the mixers' float forms read it so) */
		}
		const bool same_voices = voices_sent_.size() == seg.n_voices && voices_dev_ == voices_.p &&
			memcmp(voices_sent_.data(), seg.voices, seg.n_voices * sizeof(VoiceDesc)) == 0;
		const bool same_ms = S.ms_sent.size() == seg.n_streams && S.ms_dev == S.mstreams.p &&
			memcmp(S.ms_sent.data(), ms_host_.data(), seg.n_streams * sizeof(MixStream)) == 0;
		if (!same_voices) {
			if (!send(voices_.p, seg.voices, seg.n_voices * sizeof(VoiceDesc), err)) return false;
			voices_sent_.assign(seg.voices, seg.voices + seg.n_voices);
			voices_dev_ = voices_.p;
		}
		if (!same_ms) {
			if (!send(S.mstreams.p, ms_host_.data(), seg.n_streams * sizeof(MixStream), err)) return false;
			S.ms_sent = ms_host_;
			S.ms_dev = S.mstreams.p;
		}
		return true;
	}

	/* the time-parallel path's buffers and its parameter block, but for the chains and the tables */
	bool prepare_fast(Job &j, std::string &err) {
		const SegmentDesc &seg = j.seg;
		const FastPlan &k = j.fk;
		FastParams &fp = j.fp;
		MixSet &S = sets_[j.set], &R = sets_[j.block];
		const size_t n_lists = (size_t)FAST_LISTS * seg.n_voices * k.fmax_steps;
		if (!finfo_.ensure(seg.n_voices, err) || !fdone_.ensure(seg.n_voices, err) ||
		    !worklist_.ensure(seg.n_voices, err) || !S.work_count.ensure(4, err) ||
		    !fsteps_.ensure(n_lists * sizeof(FastStep), err) || !flines_.ensure(n_lists * sizeof(FastLine), err) ||
		    !faux_.ensure(n_lists * sizeof(FastAux), err)) return false;
		fp.voices = voices_.p; fp.steps = steps_.p; fp.fast_ids = fast_ids_.p; fp.op_ids = op_ids_.p; fp.ops = ops_.p;
		fp.vout = R.vout.p; fp.pan = R.pan.p; fp.info = finfo_.p; fp.fast_done = fdone_.p;
		fp.worklist = worklist_.p; fp.work_count = S.work_count.p; fp.vinfo = S.vinfo.p;
		fp.g_c23 = tables_->c23; fp.g_c01 = tables_->c01; fp.fsteps = (FastStep *)fsteps_.p; fp.flines = (FastLine *)flines_.p; fp.faux = (FastAux *)faux_.p;
		fp.row_stride = row_stride_; fp.n_voices = seg.n_voices; fp.n_fast = k.n_fast;
		fp.seq_enable = k.seq_ok ? 1u : 0u; fp.ids_full_ofs = n_steps_total_;
		fp.scan = nullptr; fp.scan_groups = k.scan_groups; fp.mode = 0;
		if (tun_.xcd_queues && lim_.eight_xcds) { /* the closed-form launch's task queues, one per XCD (k_fast_types.h) */
			if (!S.inmix_ctl.ensure(INMIX_WORDS, err)) return false;
			fp.inmix = S.inmix_ctl.p;
		}
		if (k.scan) {
			if (!scan_.ensure((size_t)seg.n_voices * FAST_MAX_SCAN * k.scan_groups, err)) return false;
			fp.scan = scan_.p;
		}
		if (k.look) {
			if (k.look_words_real || !k.look_inside) {
				/* look-back words: valid for this segment's epoch only, so a fresh block starts out zeroed */
				const unsigned long long *before = look_.p;
				if (!look_.ensure(k.look_words, err)) return false;
				if (look_.p != before || look_epoch_ >= (1u << 30) - 1) {
					HIP_OK(hipMemsetAsync(look_.p, 0, look_.cap * sizeof(unsigned long long), stream_));
					look_epoch_ = 0;
				}
				fp.look_epoch = ++look_epoch_;
			} else if (!look_.p && !look_.ensure(64, err)) {
				return false; /* (a token block: the kernel forms row addresses from it and never reads them) */
			}
			fp.look = look_.p;
		}
		if (!pass_flags_.p) {
			if (!pass_flags_.ensure(FAST_FLAGS, err)) return false;
			HIP_OK(hipMemsetAsync(pass_flags_.p, 0, pass_flags_.cap * sizeof(uint32_t), stream_));
		}
		fp.pass_flags = pass_flags_.p;
		fp.sum_levels = k.sum_levels;
		if (!repair_.ensure((size_t)seg.n_voices * FAST_REPAIR_WORDS, err)) return false;
		fp.repair = repair_.p;
		fp.repair_on = tun_.repair ? 1u : 0u;
		fp.max_ops = seg.max_ops; fp.max_steps = k.fmax_steps; fp.np = 64; fp.rows = k.rows; fp.rows_multi = k.rows_multi;
		fp.enable = k.use_fast ? 1u : 0u;
		if (k.inc_rows) {
			if (!inc_rows_.ensure((size_t)seg.n_inc_rows * 2 * k.inc_stride + 64, err)) return false;
			fp.inc_rows = inc_rows_.p; fp.inc_stride = k.inc_stride; fp.n_inc_rows = seg.n_inc_rows;
		}
		if (k.split_cf) {
			if (!vlists_.ensure((size_t)2 * seg.n_voices, err)) return false;
			fp.vlists = vlists_.p; fp.split_cf = 1; fp.rows_cf = k.rows_cf;
			fp.look_words_real = k.look_words_real && fp.look ? 1u : 0u;
		}
		fp.cub_ok = k.cub_ok ? 1u : 0u;
		memcpy(fp.wc, wconst_, sizeof wconst_);
		return true;
	}

	/* The chains' rows are the one large allocation that depends on how long the engine cut the segment. When the device
	 * cannot give them (a smaller or fuller GPU than the budget assumed, several engines on it) this segment's
	 * feedback voices take the block loop -- slow, exact -- and later segments are cut at CHAIN_SEG again
	 * (ADVICE r03). SAU_AMD_CHAIN_ROWS_FAIL (tests) makes the first such allocation of an engine fail -- by not
	 * asking, or ("real") by asking hipMalloc for 64 TiB, which fails the way a full device does and
	 * leaves its error behind as the thread's last one. */
	bool prepare_chains(Job &j, std::string &err) {
		const SegmentDesc &seg = j.seg;
		FastPlan &k = j.fk;
		FastParams &fp = j.fp;
		if (k.chains) {
			std::string rows_err;
			const size_t rows_need = (size_t)seg.n_chain_rows * 2 * k.chain_stride + 64;
			const char *rft = chain_rows_failed_once_ ? nullptr : tune_env("SAU_AMD_CHAIN_ROWS_FAIL");
			const bool rows_fail_test = rft && strcmp(rft, "real") != 0;
			if (rows_fail_test || !chain_rows_.ensure((rft && !rows_fail_test) ? (size_t)1 << 44 : rows_need, rows_err)) {
				chain_rows_failed_once_ = true;
				++chain_rows_failures_; /* (this backend's budget halves: Backend::chain_rows_budget) */
				if (debug_) fprintf(stderr, "saugns_amd: %zu bytes of chain rows not available (%s): block loop for this segment\n",
						rows_need * sizeof(float), rows_err.c_str());
				k.drop_chains();
			}
		}
		if (k.chains) {
			if (!chain_desc_.ensure(seg.n_chain_slots, err) ||
			    !fplines_.ensure((size_t)FAST_LISTS * seg.n_voices * k.fmax_steps * sizeof(FastLine), err)) return false;
			/* (lanes that belong to no voice -- the engine begins every kind of R feedback chain on a wave of its own -- must read
			 * as unused: analyze_kernel clears the descriptors of the voices' lanes only) */
			if (seg.chain_rows_padded) HIP_OK(hipMemsetAsync(chain_desc_.p, 0, (size_t)seg.n_chain_slots * sizeof(ChainDesc), stream_));
			fp.chain_rows = chain_rows_.p; fp.chain_stride = k.chain_stride; fp.n_chain_rows = seg.n_chain_rows; fp.n_chain_slots = seg.n_chain_slots;
			fp.chain_desc = chain_desc_.p; fp.fplines = (FastLine *)fplines_.p;
			fp.chain_inline = tun_.chain_inline ? 1u : 0u;
			fp.chain_early_ok = tun_.chain_early ? 1u : 0u;
			memcpy(fp.ctab_of_wave, k.ctabs.tab_of_wave, sizeof fp.ctab_of_wave);
			memcpy(fp.cwave_of_tab, k.ctabs.wave_of_tab, sizeof fp.cwave_of_tab);
			fp.n_ctabs = k.ctabs.n;
		}
		fp.lean_on = k.lean_on ? 1u : 0u;
		fp.rows_lean = k.rows_lean;
		return true;
	}

	void fill_tables(Job &j) {
		memcpy(j.fp.tab_of_wave, j.fk.tabs.tab_of_wave, sizeof j.fp.tab_of_wave);
		memcpy(j.fp.wave_of_tab, j.fk.tabs.wave_of_tab, sizeof j.fp.wave_of_tab);
		j.fp.n_tabs = j.fk.tabs.n;
	}

	/* a wave per voice: the voice's operator records and plan staged in LDS for lane 0's chain of dependent reads
	 * (k_analyze.h; round 6 -- a thread per voice on the records in HBM took 25-53 us per segment). Voices with more
	 * records or steps than 48 KiB hold are analysed on the records in HBM (SAU_AMD_ANALYZE_NO_LDS: all of them) */
	bool launch_analyze(Job &j, std::string &err) {
		const SegmentDesc &seg = j.seg;
		(void)err;
		TimedPair *ta = timing_on_ ? new_pair(3) : nullptr;
		if (ta) (void)hipEventRecord(ta->a, stream_);
		uint32_t lo = seg.max_ops, ls = seg.max_steps;
		size_t albytes = (size_t)lo * sizeof(DevOp) + (size_t)ls * sizeof(Step) + (size_t)lo * sizeof(uint32_t);
		if (albytes > 48 * 1024 || !tun_.analyze_lds) { lo = 0; ls = 0; albytes = 0; }
		hipLaunchKernelGGL(analyze_kernel, dim3(seg.n_voices), dim3(64), albytes, stream_, j.fp, lo, ls);
		if (ta) (void)hipEventRecord(ta->b, stream_);
		return true;
	}
	bool launch_decode(Job &j, std::string &err) {
		hipLaunchKernelGGL(decode_kernel, dim3(j.seg.n_voices), dim3(64), 0, stream_, j.fp);
		if (!wait_for_predecessor(err)) return false; /* (sauAmd_Batch_order_after: the rendering kernels from here on) */
		j.tf = timing_on_ ? new_pair(2) : nullptr;
		if (j.tf) (void)hipEventRecord(j.tf->a, stream_);
		return true;
	}

	/* One launch of a fast_kernel build. `cf`: over the closed-form voices' buffers only; `prm`: another block than j.fp.
	 * (rows per pass 2, 4, 5, 6, 8; the full build never runs at more than 4: its 5- and 6-row slots stand in with 4's;
	 * the lean build has 4, 5 or 6) */
	bool launch_build(Job &j, std::string &err, int build, uint32_t rows, uint32_t grid, const FastParams *prm = nullptr, bool cf = false,
			bool wide = false) {
		if (!rows_hazard(j, err)) return false; /* (every build stores rows) */
		if (build == 1 && rows > 4) rows = 4;
		if (build == 3) rows = rows < 5 ? 4 : rows > 6 ? 6 : rows;
		/* (the look-back build that mixes few-voice streams: round 6, FastParams.tail_ok) */
		const void *fn = fast_kernel_fn(build, rows, (wide ? FK_WIDE : 0u) | (build == 2 && j.tail_live ? FK_TAIL : 0u));
		if (!fn) {
			err = "internal error: no fast_kernel build with " + std::to_string(rows) + " rows per pass in this form";
			return false;
		}
		const size_t lds = j.fk.launch_lds(build, rows, wide, cf);
		void *args[] = {(void *)(prm ? prm : &j.fp)};
		if (!raise_lds_attr(fn, lds, dev_, err)) return false;
		HIP_OK(hipLaunchKernel(fn, dim3(grid), dim3(1024), args, lds, stream_));
		return true;
	}
	/* a pass of the main build over the segment (and, for the chains' two passes, of the lean build before it) */
	void launch_fast(Job &j, std::string &err, uint32_t mode, uint32_t grid = 0) {
		FastParams &fp = j.fp;
		if (!grid) grid = j.fk.grid;
		fp.mode = mode;
		if (fp.lean_on && fp.chain_rows && (mode == fp.sum_levels + 1 || mode == fp.sum_levels + 2) &&
		    !launch_build(j, err, 3, fp.rows_lean, grid))
			j.launched = false;
		if (j.fk.main_build == 2) { /* what the single-pass build leaves out: returns at once when there is none */
			fp.only_multi = 1;
			if (!launch_build(j, err, 1, j.fk.rows_multi, grid)) j.launched = false;
			fp.only_multi = 0;
		} else if (!launch_build(j, err, j.fk.main_build, j.fk.rows, grid, nullptr, false, j.fk.wide_cf)) {
			j.launched = false;
		}
	}

	/* A split segment: two launches over analyze_kernel's lists -- the closed-form voices, then the look-back voices -- or
	 * both kinds in one (duo_kernel). */
	bool launch_split(Job &j, std::string &err) {
		const SegmentDesc &seg = j.seg;
		const FastPlan &k = j.fk;
		FastParams &fp = j.fp, &cfp = j.cfp;
		MixSet &S = sets_[j.set];
		if (k.tailmix) {
			if (!S.tail_ok.ensure(seg.n_streams, err)) return false;
			fp.tail_ok = S.tail_ok.p; fp.inmix_stream = S.mstreams.p;
			fp.tail_flags = (seg.stereo ? 1u : 0u) | (seg.swap_bytes ? 2u : 0u);
			fp.tail_pcm_offset = seg.pcm_offset;
			hipLaunchKernelGGL(tailmix_kernel, dim3((seg.n_streams + 63) / 64), dim3(64), 0, stream_, fp, seg.n_streams);
			j.tail_live = true;
		}
		if (!rows_hazard(j, err)) return false;
		if (j.tail_live && !pcm_hazard(err)) return false; /* (the look-back launch stores those streams' PCM) */
		cfp = fp;
		cfp.n_fast = k.n_fast_cf; cfp.rows = k.rows_cf; cfp.mode = 0; cfp.only_multi = 0;
		if (getenv("SAU_AMD_DEBUG_DUO"))
			fprintf(stderr, "[sau-amd] duo %d: enabled %d look %d words_real %u FT %u rows_cf %u cub_ok %u tail %d may_scan %u of %u voices, lds %zu of %zu\n",
					(int)k.duo, (int)tun_.duo, fp.look != nullptr, fp.look_words_real, k.rows, k.rows_cf, fp.cub_ok, (int)j.tail_live, seg.n_may_scan, seg.n_voices,
					k.launch_lds(2, k.rows, false) + 1024, lim_.lds_limit);
		cfp.dyn_chunks = k.tasks_cf.dyn_chunks; cfp.dyn_static = k.tasks_cf.dyn_static;
		if (!k.duo && !launch_build(j, err, 0, k.rows_cf, k.grid_cf, &cfp, true, k.wide_cf)) j.launched = false;
		fp.mode = fp.sum_levels + 1; fp.only_multi = 0; fp.look_wpv = k.look_wpv; fp.look_groups = k.groups;
		fp.look_wpv_flags = k.look_wpv_flags;
		if (k.duo) {
			const size_t dlds = k.launch_lds(2, k.rows, false);
			if (!raise_lds_attr((const void *)duo_kernel, dlds, dev_, err)) return false;
			auto go = [&]() -> bool {
				void *da[] = {(void *)&fp, (void *)&cfp};
				return hipLaunchKernel((const void *)duo_kernel, dim3(lim_.fk_grid), dim3(1024), da, dlds, stream_) == hipSuccess;
			};
			/* (its look-back waves wait for sums across workgroups: in turn with other such launches of the process) */
			if (!SpreadLaunchOrder::get().ordered(dev_, stream_, go)) j.launched = false;
		} else if (fp.look) {
			if (k.look_inside) { /* (every voice within one workgroup: no waits across workgroups) */
				if (!launch_build(j, err, 2, k.rows, k.grid_look, nullptr, false, k.wide_look)) j.launched = false;
			} else if (!SpreadLaunchOrder::get().ordered(dev_, stream_, [&]() { return launch_build(j, err, 2, k.rows, k.grid_look, nullptr, false, k.wide_look); })) {
				j.launched = false;
			}
			if (fp.cub_ok) { /* look-back voices with the loop tails of `cub` R segments: the build with that code, same lists */
				const void *ck2 = fast_kernel_fn(2, FAST_CUB_ROWS, FK_CUB);
				const size_t lds2 = k.launch_lds(2, FAST_CUB_ROWS, false);
				if (!raise_lds_attr(ck2, lds2, dev_, err)) return false;
				auto go = [&]() -> bool {
					void *a2[] = {(void *)&fp};
					return hipLaunchKernel(ck2, dim3(k.grid_look), dim3(1024), a2, lds2, stream_) == hipSuccess;
				};
				if (k.look_inside ? !go() : !SpreadLaunchOrder::get().ordered(dev_, stream_, go)) j.launched = false;
			}
		}
		return true;
	}

	/* Some voice may have running-sum phases: sums per row group, their prefixes, final pass.
	 * (With look-back only voices that have, or may get, feedback chains still take sum passes.) */
	bool launch_sums_and_chains(Job &j, std::string &err) {
		const SegmentDesc &seg = j.seg;
		FastParams &fp = j.fp;
		if (!rows_hazard(j, err)) return false;
		if (fp.chain_rows && fp.chain_early_ok && !launch_early_chains(j, err)) return false;
		for (uint32_t pass = 1; pass <= fp.sum_levels && (!fp.look || seg.n_chain_rows); ++pass) {
			launch_fast(j, err, pass);
			hipLaunchKernelGGL(scan_kernel, dim3(seg.n_voices), dim3(64), 0, stream_, fp);
		}
		if (!fp.chain_rows) { launch_fast(j, err, fp.sum_levels + 1); return true; }
		return launch_chains(j, err);
	}

	/* chains that sums or other chains' inputs depend on, fed from their own lines: whole segment, before
	 * anything else (FastInfo.early); returns at once when analyze_kernel found none */
	bool launch_early_chains(Job &j, std::string &err) {
		FastParams &fp = j.fp;
		const uint32_t cgrid = j.fk.chain_grid;
		const size_t clds = chain_alone_lds((size_t)fp.n_ctabs * CHAIN_TAB_BYTES + CHAIN_IO_BYTES, cgrid);
		if (!raise_lds_attr((const void *)chain_kernel, clds, dev_, err)) return false;
		fp.chain_early = 1; fp.range_mode = 0;
		hipLaunchKernelGGL(chain_kernel, dim3(cgrid), dim3(192), clds, stream_, fp);
		/* R feedback: a chain wave and a feeder wave per 64 chains (k_chain.h) */
		const size_t rlds = chain_alone_lds(RCHAIN_LDS_BYTES, cgrid);
		if (!raise_lds_attr((const void *)rchain_kernel, rlds, dev_, err)) return false;
		hipLaunchKernelGGL(rchain_kernel, dim3(cgrid), dim3(RCHAIN_THREADS), rlds, stream_, fp);
		fp.chain_early = 0;
		return true;
	}

	/* The chains' inputs, the chains themselves (lanes = voices), the final pass -- pipelined over
	 * chunks of the segment: chain_kernel occupies one CU per 64 chains for frames x chain latency,
	 * so it runs on a stream of its own while, on the other CUs, the chain-input pass prepares the
	 * chunks after it and the final pass finishes the chunks before it. (The chunks: launch_plan.h, chain_chunk_bounds.) */
	bool launch_chains(Job &j, std::string &err) {
		const FastPlan &k = j.fk;
		FastParams &fp = j.fp;
		const uint32_t cgrid = k.chain_grid, n_chunks = k.chunks.n;
		const size_t clds = chain_alone_lds((size_t)fp.n_ctabs * CHAIN_TAB_BYTES + CHAIN_IO_BYTES, cgrid);
		if (!raise_lds_attr((const void *)chain_kernel, clds, dev_, err)) return false;
		TimedPair *tc = nullptr; /* counted with the block loop it replaces */
		if (n_chunks == 1) {
			tc = timing_on_ ? new_pair(0) : nullptr;
			fp.range_mode = 0;
			launch_fast(j, err, fp.sum_levels + 2);
			if (tc) (void)hipEventRecord(tc->a, stream_);
			hipLaunchKernelGGL(chain_kernel, dim3(cgrid), dim3(192), clds, stream_, fp);
			if (tc) (void)hipEventRecord(tc->b, stream_);
			launch_fast(j, err, fp.sum_levels + 1);
			return true;
		}
		if (!chain_stream_) {
			chain_stream_ = StreamPool::get().take(dev_, 1);
			if (!chain_stream_) {
				/* High priority, for the sake of the hardware queue it gets: the runtime maps streams onto a
				 * handful of queues (four per priority), and a second generator's two streams of ordinary priority
				 * landed on ONE -- its chains and its passes then ran one after the other, 76 ms for a config-5
				 * step instead of 45 (profiles/r05_c5_pipelined_trace.txt). Queues of another priority are others:
				 * a generator's chain stream never shares its main stream's. (The chain wave is also what the
				 * step's time hangs on.) */
				int lo = 0, hi = 0;
				(void)hipDeviceGetStreamPriorityRange(&lo, &hi);
				HIP_OK(hipStreamCreateWithPriority(&chain_stream_, hipStreamNonBlocking, hi));
			}
		}
		while (chain_ev_.size() < 2 * (size_t)n_chunks) {
			hipEvent_t e;
			HIP_OK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
			chain_ev_.push_back(e);
		}
		tc = timing_on_ ? new_pair(0) : nullptr;
		const uint32_t *cb = k.chunks.cb;
		auto set_range = [&](FastParams &q, uint32_t mode, uint32_t c) {
			q.range_mode = mode; q.f_lo = cb[c]; q.f_hi = c + 1 == n_chunks ? 0xffffffffu : cb[c + 1];
		};
		for (uint32_t c = 0; c < n_chunks; ++c) { /* inputs of chunk c, then its chains on the other stream */
			set_range(fp, 1, c);
			fp.range_last = c + 1 == n_chunks;
			launch_fast(j, err, fp.sum_levels + 2, k.pass_grid);
			HIP_OK(hipEventRecord(chain_ev_[2 * c], stream_));
			HIP_OK(hipStreamWaitEvent(chain_stream_, chain_ev_[2 * c], 0));
			FastParams cp = fp;
			set_range(cp, 1, c);
			if (tc && c == 0) (void)hipEventRecord(tc->a, chain_stream_);
			hipLaunchKernelGGL(chain_kernel, dim3(cgrid), dim3(192), clds, chain_stream_, cp);
			if (tc && c + 1 == n_chunks) (void)hipEventRecord(tc->b, chain_stream_);
			HIP_OK(hipEventRecord(chain_ev_[2 * c + 1], chain_stream_));
		}
		/* the mixer follows the final passes chunk by chunk (launch_plan.h: early_mix) */
		uint32_t mixed_blocks = 0;
		if (k.early_mix) hipLaunchKernelGGL(premix_kernel, dim3((j.seg.n_voices + 63) / 64), dim3(64), 0, stream_, fp);
		for (uint32_t c = 0; c < n_chunks; ++c) { /* the final pass follows the chains chunk by chunk */
			HIP_OK(hipStreamWaitEvent(stream_, chain_ev_[2 * c + 1], 0));
			set_range(fp, 2, c);
			fp.range_last = c + 1 == n_chunks;
			launch_fast(j, err, fp.sum_levels + 1, c + 1 == n_chunks ? k.grid : k.pass_grid);
			if (k.early_mix && c + 1 < n_chunks && cb[c + 1] > 512) {
				const uint32_t hi = (cb[c + 1] - 512) / 256;
				if (hi > mixed_blocks) {
					if (!pcm_hazard(err)) return false; /* (an early launch writes PCM on the main stream) */
					MixParams mp = mix_params(j);
					mp.blk_lo = mixed_blocks; mp.blk_hi = hi;
					TimedPair *tm = timing_on_ ? new_pair(1) : nullptr;
					if (tm) (void)hipEventRecord(tm->a, stream_);
					hipLaunchKernelGGL((j.in.f32 ? mix_kernel_f32 : mix_kernel), dim3(hi - mixed_blocks, j.seg.n_streams), dim3(256), 0, stream_, mp);
					if (tm) (void)hipEventRecord(tm->b, stream_);
					mixed_blocks = hi;
				}
			}
		}
		j.early_mixed_blocks = mixed_blocks;
		fp.range_mode = 0; fp.f_lo = 0; fp.f_hi = 0; fp.range_last = 0;
		return true;
	}

	/* Closed-form voices only: tasks dealt out by a counter or the XCDs' queues, the launch's own mixing, and the 12-row build as
	 * edge and inner launches (launch_plan.h: plan_closed_form). */
	bool launch_closed_form(Job &j, std::string &err) {
		const SegmentDesc &seg = j.seg;
		const FastPlan &k = j.fk;
		FastParams &fp = j.fp;
		fp.dyn_chunks = k.tasks.dyn_chunks; fp.dyn_static = k.tasks.dyn_static; fp.dyn_small = k.tasks.dyn_small;
		if (k.queues) {
			fp.inmix_flags = k.inmix_flags;
			fp.inmix_div_s = k.div.s; fp.inmix_div_m = k.div.m;
			if (k.inmix) {
				fp.inmix_stream = sets_[j.set].mstreams.p;
				fp.inmix_pcm_offset = seg.pcm_offset;
				hipLaunchKernelGGL(premix_kernel, dim3((seg.n_voices + 63) / 64), dim3(64), 0, stream_, fp);
				j.inmix_live = true;
			}
		}
		if (k.inner != INNER_NONE) {
			const bool lm = k.inner == INNER_LANE_MAJOR;
#if FK_LM_TAB0
			const bool tab0 = lm && k.inner_tab0 && tab0_kernel_ok(fast_kernel_fn(0, 12, FK_WIDE | FK_INNER | FK_LANEMAJOR | FK_TAB0)); /* (one table: the instantiation whose table address is the index alone) */
#else
			const bool tab0 = false;
#endif
			/* (wave oscillators with constant amplitude only, by the planner's word: the instantiation that holds nothing else. A
			 * one-table build's launches of one table keep that instantiation: it is an A/B build, and has no third copy) */
			const bool wonly = FK_LM_WONLY && lm && k.inner_wonly && !tab0;
			const void *ik = fast_kernel_fn(0, 12, FK_WIDE | FK_INNER | (lm ? FK_LANEMAJOR : 0u) | (tab0 ? FK_TAB0 : 0u) | (wonly ? FK_WONLY : 0u));
			if (!ik) { err = "no inner instantiation of fast_kernel for this form"; return false; }
			const size_t lds = k.inner_lds();
			FastParams ep = fp;
			ep.mode = 0; ep.edge_only = 1; ep.dyn_static = 1; ep.dyn_chunks = 2; ep.dyn_small = 0; ep.inmix_flags = 0; /* (two tasks a voice: its first group, its last) */
			/* (the edge launch stores rows and no PCM: with rows of its own it runs beside the last segment's mixer, as
			 * analyze_kernel, decode_kernel and premix_kernel before it do either way -- launch_build has the rows' wait) */
			if (!launch_build(j, err, 0, k.rows, k.grid_edge, &ep, false, true)) j.launched = false;
			fp.mode = 0;
			void *iargs[] = {(void *)&fp};
			if (!raise_lds_attr(ik, lds, dev_, err)) return false;
			if (fp.inmix_flags && !pcm_hazard(err)) return false; /* (the inner launch mixes tiles into the PCM itself) */
			HIP_OK(hipLaunchKernel(ik, dim3(k.grid), dim3(1024), iargs, lds, stream_));
			if (inner_report_) fprintf(stderr, "[sau-amd] inner: %s, %u voices, %u tables%s\n", lm ? "lane-major" : "row-major", seg.n_voices, k.tabs.n, tab0 ? ", tab0" : wonly ? ", wonly" : "");
		} else {
			/* (a closed-form segment that did not take the two launches, and what kept it from them) */
			if (inner_report_) fprintf(stderr, "[sau-amd] inner: none (rows %u, wide %d, chunks %u), %u voices\n", k.rows, k.wide_cf ? 1 : 0, fp.dyn_chunks, seg.n_voices);
			if (fp.inmix_flags && (!rows_hazard(j, err) || !pcm_hazard(err))) return false;
			launch_fast(j, err, 0);
		}
		fp.dyn_chunks = 0; fp.inmix_flags = 0; fp.dyn_small = 0;
		return true;
	}

	/* closed-form voices with the loop tails of `cub` R segments (FastInfo.cub): the build with that code,
	 * FAST_CUB_ROWS rows per pass, fixed strides over the same voices as the closed-form launch; returns at
	 * once when analyze_kernel found none */
	bool launch_cub(Job &j, std::string &err) {
		if (!j.fp.cub_ok) return true;
		const FastPlan &k = j.fk;
		FastParams q = k.main_build == 2 ? j.cfp : j.fp;
		q.n_fast = k.n_fast_cf; q.rows = FAST_CUB_ROWS; q.mode = 0; q.only_multi = 0;
		q.dyn_chunks = k.tasks_cub.dyn_chunks; q.dyn_static = k.tasks_cub.dyn_static;
		const size_t qlds = k.launch_lds(0, FAST_CUB_ROWS, false, true);
		const void *ck = fast_kernel_fn(0, FAST_CUB_ROWS, FK_CUB);
		if (!raise_lds_attr(ck, qlds, dev_, err)) return false;
		void *qargs[] = {(void *)&q};
		if (!rows_hazard(j, err)) return false;
		HIP_OK(hipLaunchKernel(ck, dim3(k.grid_cub), dim3(1024), qargs, qlds, stream_));
		return true;
	}

	/* row groups noted for a second evaluation: returns at once when there are none */
	/* (only closed-form voices note any: with split launches they run at rows_cf rows per pass, in cfp's layout) */
	bool launch_repair(Job &j, std::string &err) {
		const FastPlan &k = j.fk;
		const size_t rlds = k.launch_lds(0, k.rows_repair, k.wide_cf, k.main_build == 2);
		FastParams rpar = k.main_build == 2 ? j.cfp : j.fp;
		rpar.mode = 0;
		const void *rk = repair_kernel_fn(k.rows_repair, k.wide_cf);
		if (!rk) {
			err = "internal error: no repair_kernel build with " + std::to_string(k.rows_repair) + " rows per pass in this form";
			return false;
		}
		if (!raise_lds_attr(rk, rlds, dev_, err)) return false;
		j.fp.mode = 0;
		void *rargs[] = {(void *)&rpar};
		if (!rows_hazard(j, err)) return false;
		HIP_OK(hipLaunchKernel(rk, dim3(k.grid_repair), dim3(1024), rargs, rlds, stream_));
		return true;
	}

	bool launch_finalize(Job &j, std::string &err) {
		const SegmentDesc &seg = j.seg;
		TimedPair *tz = timing_on_ ? new_pair(3) : nullptr;
		if (tz) (void)hipEventRecord(tz->a, stream_);
		hipLaunchKernelGGL(finalize_kernel, dim3((unsigned)(((size_t)seg.n_voices * j.fp.max_ops * 8 + 63) / 64)), dim3(64), 0,
				stream_, j.fp);
		if (tz) (void)hipEventRecord(tz->b, stream_);
		HIP_OK(hipGetLastError());
		if (debug_ && j.fk.use_fast) {
			(void)hipStreamSynchronize(stream_);
			FastInfo fi0;
			(void)hipMemcpy(&fi0, finfo_.p, sizeof fi0, hipMemcpyDeviceToHost);
			fprintf(stderr, "[sau-amd] fast: voice 0 total %u H %u bail %u steps %u seq %u; n_fast %u rows %u\n",
					fi0.total, fi0.H, fi0.bail, fi0.n_fsteps, fi0.seq, j.fk.n_fast, j.fk.rows);
			std::vector<FastStep> fs(fi0.n_fsteps < 64 ? fi0.n_fsteps : 64);
			if (!fs.empty()) (void)hipMemcpy(fs.data(), fsteps_.p, fs.size() * sizeof(FastStep), hipMemcpyDeviceToHost);
			for (size_t i = 0; i < fs.size(); ++i)
				fprintf(stderr, "[sau-amd]   step %zu kind %u flags %#x which %u dep %u out %d pm %d fpm %d amp %d aux %d type %#x inc %u ac %g fc %g ramp %u\n",
						i, fs[i].kind & 0xff, (fs[i].kind >> 8) & 0xff, (fs[i].kind >> 16) & 0xff, fs[i].kind >> 24,
						(int)fs[i].out_off, (int)fs[i].pm_off, (int)fs[i].fpm_off, (int)fs[i].amp_off, (int)fs[i].aux_off,
						fs[i].type, fs[i].inc, fs[i].ac, fs[i].fc, fs[i].ramp);
		}
		return true;
	}

	/* the block loop continues where the time-parallel path stopped (fast_done), over the device-built work list */
	bool launch_block_loop(Job &j, std::string &err) {
		const SegmentDesc &seg = j.seg;
		const BlockLoopPlan &b = j.bl;
		RenderParams &rp = j.rp;
		rp.team_bytes = (uint32_t)b.team_bytes;
		memcpy(rp.tab_of_wave, b.tabs.tab_of_wave, sizeof rp.tab_of_wave);
		memcpy(rp.wave_of_tab, b.tabs.wave_of_tab, sizeof rp.wave_of_tab);
		rp.voices = voices_.p; rp.steps = steps_.p; rp.op_ids = op_ids_.p; rp.ops = ops_.p;
		rp.vout = sets_[j.block].vout.p; rp.pan = sets_[j.block].pan.p; rp.vinfo = sets_[j.set].vinfo.p;
		rp.g_c23 = tables_->c23; rp.g_c01 = tables_->c01;
		rp.row_stride = row_stride_; rp.seg_len = seg.len;
		rp.n_slots = seg.n_slots; rp.max_ops = seg.max_ops; rp.n_tabs = b.tabs.n;
		rp.max_steps = seg.max_steps; rp.n_main = seg.n_main;
		memcpy(rp.wc, wconst_, sizeof wconst_);
		rp.fast_done = fdone_.p; rp.worklist = worklist_.p; rp.work_count = sets_[j.set].work_count.p;
		j.block_grid = b.grid(seg, j.fk.use_fast);
		if (b.HB) {
			const size_t stride = ((size_t)seg.n_slots * 64 * sizeof(float) + (size_t)seg.max_ops * sizeof(DevOp) +
				(size_t)seg.max_steps * sizeof(Step) + 255) / 256 * 256 / sizeof(float);
			if (stride > 0xffffffffu) { err = "voice too large (block buffers + operator records beyond 16 GiB)"; return false; }
			if (!big_slots_.ensure((size_t)j.block_grid * stride, err)) return false;
			rp.big_slots = big_slots_.p; rp.big_stride = (uint32_t)stride;
		}
		if (!wait_for_predecessor(err)) return false; /* (a segment without the time-parallel path) */
		if (!rows_hazard(j, err)) return false;
		TimedPair *tp = timing_on_ ? new_pair(0) : nullptr;
		if (tp) (void)hipEventRecord(tp->a, stream_);
		const void *fn = render_kernel_fn(b.W, b.T, b.V, b.HB);
		if (!fn) { err = "internal error: no render_kernel build of this geometry"; return false; }
		if (!raise_lds_attr(fn, b.lds, dev_, err)) return false;
		void *args[] = {(void *)&rp};
		HIP_OK(hipLaunchKernel(fn, dim3(j.block_grid), dim3(64 * b.W * b.V), args, b.lds, stream_));
		HIP_OK(hipGetLastError());
		if (tp) (void)hipEventRecord(tp->b, stream_);
		if (debug_) debug_dump("after render", j);
		return true;
	}

	/* The segment's last mixer launch: on the side stream, behind a fork recorded on the main stream after the block loop, so that
	 * the next segment's analyze_kernel, decode_kernel, premix_kernel (and, with rows of its own, the edge launch) run beside it --
	 * they are small grids waiting on latency, the mixer is HBM-bound, and they need finalize_kernel's state of this segment, nothing
	 * of the mixer's. What it reads is kept apart by the two sets of records (and blocks of rows), what it writes by the waits of
	 * mix_overlap.h. (Round 3 had a mixer beside the whole next segment, persistent or not, and measured no gain: nothing runs
	 * beside the rendering launches, which fill every CU's registers. This one asks for the set-up launches' time alone; the
	 * figures are in profiles/r09_mix_overlap_ab.json.) MIXO_OFF: on the main stream, behind the segment's kernels. */
	bool launch_mixer(Job &j, std::string &err) {
		const SegmentDesc &seg = j.seg;
		const uint32_t max_write = j.in.max_write;
		const Mixer which = plan_mixer(seg, tun_, j.in, pcm_pitch(), j.inmix_live, j.early_mixed_blocks);
		if (which == MIX_NONE) { report_overlap(j, 0, false); return true; }
		MixSet &S = sets_[j.set];
		MixParams mp = mix_params(j);
		/* (frames an early launch has mixed are skipped when the device says those results stand: k_finish.h) */
		mp.early_blocks = j.early_mixed_blocks;
		mp.inmix = j.inmix_live ? S.inmix_ctl.p : nullptr; /* (the closed-form launch has mixed tiles itself: mix_kernel takes what is left) */
		mp.tail_ok = j.tail_live ? S.tail_ok.p : nullptr; /* (the look-back launch has mixed some streams itself: mix_few_kernel leaves them) */
		/* (the pair first: new_pair may drain its pool, which joins the pending mixer -- nothing of this mixer exists yet) */
		TimedPair *tm = timing_on_ ? new_pair(1) : nullptr;
		hipStream_t ms = stream_;
		/* The tracker learns of the mixer only once its done event is recorded (mixer_launched below): until then no join can
		 * take the ticket for waited-for, and a launch that fails on the way leaves no ticket without an event behind. */
		const uint64_t ticket = j.mode == MIXO_OFF ? 0 : mixo_.next_ticket();
		if (!ticket) {
			if (!wait_mixer(mixo_.before_pcm(), "mixer", err)) return false; /* (an earlier segment's may still be on the side stream) */
		} else {
			hipEvent_t fork = mix_fork_[MixOverlapTracker::slot(ticket)];
			HIP_OK(hipEventRecord(fork, stream_));
			HIP_OK(hipStreamWaitEvent(mix_stream_, fork, 0));
			ms = mix_stream_;
		}
		if (tm) (void)hipEventRecord(tm->a, ms);
		switch (which) {
		case MIX_FEW_F32: hipLaunchKernelGGL(mix_few_kernel_f32, dim3((max_write + 1023) / 1024, seg.n_streams), dim3(256), 0, ms, mp); break;
		case MIX_F32: hipLaunchKernelGGL(mix_kernel_f32, dim3((max_write + 255) / 256, seg.n_streams), dim3(256), 0, ms, mp); break;
		case MIX_FEW: hipLaunchKernelGGL(mix_few_kernel, dim3((max_write + 1023) / 1024, seg.n_streams), dim3(256), 0, ms, mp); break;
		case MIX_64: hipLaunchKernelGGL(mix_kernel64, dim3((max_write + 63) / 64, seg.n_streams), dim3(64), 0, ms, mp); break;
		default: hipLaunchKernelGGL(mix_kernel, dim3((max_write + 255) / 256, seg.n_streams), dim3(256), 0, ms, mp); break;
		}
		HIP_OK(hipGetLastError());
		if (tm) (void)hipEventRecord(tm->b, ms);
		if (ticket) {
			HIP_OK(hipEventRecord(mix_done_[MixOverlapTracker::slot(ticket)], mix_stream_));
			if (mixo_.mixer_launched(j.set, j.block) != ticket) { err = "internal error: the final mixer's ticket changed under its launch"; return false; }
		}
		report_overlap(j, ticket, true);
		if (mp.inmix && inmix_report_) report_inmix(mp, seg.n_voices, max_write);
		return true;
	}

	/* (SAU_AMD_OVERLAP_REPORT, tests: a line per segment -- its mode and set, its mixer's ticket (0: on the main stream, or none),
	 * and every wait for a mixer issued since the last line, each as where:ticket:done|busy -- had that mixer finished when the
	 * wait was issued) */
	void report_overlap(const Job &j, uint64_t ticket, bool mixer) {
		if (!overlap_report_) return;
		fprintf(stderr, "[sau-amd] overlap: mode %s set %u block %u mixer %s ticket %llu waits%s\n",
				j.mode == MIXO_ALTERNATE ? "alternate" : j.mode == MIXO_SHARED ? "shared" : "off", j.set, j.block,
				!mixer ? "none" : ticket ? "side" : "main", (unsigned long long)ticket, report_waits_.empty() ? " -" : report_waits_.c_str());
		report_waits_.clear();
	}

	/* (SAU_AMD_INMIX_REPORT, tests: what the launch mixed itself) */
	void report_inmix(const MixParams &mp, uint32_t n_voices, uint32_t max_write) {
		std::vector<uint32_t> h(INMIX_WORDS);
		uint32_t g[2] = {0, 0};
		(void)hipStreamSynchronize(stream_);
		(void)hipMemcpy(h.data(), mp.inmix, INMIX_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost);
		(void)hipMemcpy(g, mp.guard, sizeof g, hipMemcpyDeviceToHost);
		const uint32_t nch = h[INMIX_NCH] < INMIX_MAX_CHUNKS ? h[INMIX_NCH] : INMIX_MAX_CHUNKS, tpc = h[INMIX_TPC];
		uint32_t tiles = 0, whole = 0, all = 0;
		for (uint32_t k = 0; k < nch; ++k) {
			/* (the chunk's tiles: a regular chunk's, or a short one's at the end -- k_fast_types.h: INMIX_NCH1) */
			uint32_t lo_f = k * h[INMIX_CF], hi_f = lo_f + h[INMIX_CF];
			if (k >= h[INMIX_NCH1]) { lo_f = h[INMIX_BASE] + (k - h[INMIX_NCH1]) * h[INMIX_CFS]; hi_f = lo_f + h[INMIX_CFS]; }
			else if (hi_f > h[INMIX_BASE]) hi_f = h[INMIX_BASE];
			if (hi_f > max_write) hi_f = max_write;
			const uint32_t tk = hi_f > lo_f ? (hi_f - lo_f + INMIX_TILE - 1) / INMIX_TILE : 0u;
			uint32_t c = 0;
			for (uint32_t j = 0; j < tk && j < tpc && j < INMIX_MAX_TPC; ++j) c += (h[INMIX_CHUNK + INMIX_LINE * k + INMIX_BITS + (j >> 5)] >> (j & 31u)) & 1u;
			tiles += c; whole += c == tk ? 1u : 0u; all += tk;
		}
		fprintf(stderr, "[sau-amd] inmix: voices %u frames %u chunks %u x %u frames, tiles %u of %u, chunks mixed whole %u, guard %u %u\n",
				n_voices, max_write, nch, h[INMIX_CF], tiles, all, whole, g[0], g[1]);
	}

	/* everything a mixer of this segment dereferences but the PCM: the segment's set of records and its block of rows */
	MixParams mix_params(const Job &j) {
		const SegmentDesc &seg = j.seg;
		const MixSet &S = sets_[j.set], &R = sets_[j.block];
		MixParams mp;
		mp.streams = S.mstreams.p; mp.vout = R.vout.p; mp.pan = R.pan.p; mp.vinfo = S.vinfo.p;
		mp.row_stride = row_stride_; mp.pcm_offset = seg.pcm_offset;
		mp.stereo = seg.stereo ? 1 : 0;
		mp.swap_bytes = seg.swap_bytes ? 1 : 0;
		mp.blk_lo = 0; mp.blk_hi = 0; mp.early_blocks = 0; mp.guard = S.work_count.p; mp.inmix = nullptr; mp.tail_ok = nullptr;
		return mp;
	}

	bool fetch_pcm(uint32_t stream, int16_t *dst, uint32_t frames, bool stereo, std::string &err) override {
		if (pcm_f32_) { err = "the last run's samples are float32"; return false; }
		return fetch_units(stream, dst, (size_t)frames * (stereo ? 2 : 1), err);
	}
	bool fetch_pcm_f32(uint32_t stream, float *dst, uint32_t frames, bool stereo, std::string &err) override {
		if (!pcm_f32_) { err = "the last run's samples are int16"; return false; }
		return fetch_units(stream, (int16_t *)dst, (size_t)frames * (stereo ? 2 : 1) * 2, err);
	}
	/* n int16 units (a float sample is two) from the start of the stream's row */
	bool fetch_units(uint32_t stream, int16_t *dst, const size_t n, std::string &err) {
		use_device();
		if (!join_mixer("fetch_pcm", err)) return false;
		/* the caller's memory is pageable: a device copy straight into it costs milliseconds of
		 * pinning per call, so the PCM goes through a page-locked block (unless dst is one) */
		const bool pinned = host_blocks_.count(dst) != 0;
		if (!pinned && !h_pcm_.ensure(n, err)) return false;
		HIP_OK(hipMemcpyAsync(pinned ? dst : h_pcm_.p, pcm_at(stream), n * sizeof(int16_t),
				hipMemcpyDeviceToHost, stream_));
		HIP_OK(hipStreamSynchronize(stream_));
		if (!pinned) memcpy(dst, h_pcm_.p, n * sizeof(int16_t));
		return true;
	}

	/* output stage: copies into page-locked memory queue behind the mixer and
	 * ahead of the next run's kernels on the one stream */
	bool fetch_pcm_async(uint32_t stream, int16_t *dst, uint32_t frames, bool stereo, int slot,
			std::string &err) override {
		if (pcm_f32_) { err = "the last run's samples are float32"; return false; }
		return fetch_bytes_async(stream, dst, (size_t)frames * (stereo ? 2 : 1) * sizeof(int16_t), slot, err);
	}
	bool fetch_pcm_f32_async(uint32_t stream, float *dst, uint32_t frames, bool stereo, int slot,
			std::string &err) override {
		if (!pcm_f32_) { err = "the last run's samples are int16"; return false; }
		return fetch_bytes_async(stream, dst, (size_t)frames * (stereo ? 2 : 1) * sizeof(float), slot, err);
	}
	bool fetch_bytes_async(uint32_t stream, void *dst, size_t bytes, int slot, std::string &err) {
		slot &= 3;
		use_device();
		if (!join_mixer("fetch_pcm_async", err)) return false;
		if (!fetch_ev_[slot]) HIP_OK(hipEventCreateWithFlags(&fetch_ev_[slot], hipEventDisableTiming));
		hipStream_t cs = stream_;
		HIP_OK(hipMemcpyAsync(dst, pcm_at(stream), bytes, hipMemcpyDeviceToHost, cs));
		HIP_OK(hipEventRecord(fetch_ev_[slot], cs));
		return true;
	}
	bool wait_fetch(int slot, std::string &err) override {
		slot &= 3;
		if (fetch_ev_[slot]) HIP_OK(hipEventSynchronize(fetch_ev_[slot]));
		return true;
	}
	void *alloc_host(size_t bytes) override {
		use_device();
		std::string err;
		void *p = pool_alloc(true, bytes, err);
		if (p) host_blocks_[p] = bytes;
		return p;
	}
	void free_host(void *p) override {
		use_device();
		auto it = host_blocks_.find(p);
		if (it == host_blocks_.end()) return;
		(void)hipStreamSynchronize(stream_);
		pool_free(true, p, it->second);
		host_blocks_.erase(it);
	}

	/* ---- level metering (k_levels.h; the geometry is launch_plan.h's plan_levels) ---- */
	bool begin_metering(std::string &err) override {
		use_device();
		if (!join_mixer("begin_metering", err)) return false;
		if (lev_acc_.p) return true;
		if (!lev_acc_.ensure(cfg_.n_streams, err)) return false;
		HIP_OK(hipMemsetAsync(lev_acc_.p, 0, (size_t)cfg_.n_streams * sizeof(LevelsAcc), stream_));
		return true;
	}
	/* the two launches of one measurement, on the backend's stream */
	bool launch_levels(LevelsParams lp, const LevelsPlan &plan, std::string &err) {
		if (!plan.blocks) lp.parts = nullptr; /* (rows without a sample: the records are all there is to write) */
		else {
			if (!lev_parts_.ensure(plan.parts, err)) return false;
			lp.parts = lev_parts_.p;
			lp.blocks = plan.blocks;
			if (lp.f32) hipLaunchKernelGGL(levels_kernel<float>, dim3(plan.blocks, plan.rows), dim3(LEVELS_THREADS), 0, stream_, lp);
			else hipLaunchKernelGGL(levels_kernel<int16_t>, dim3(plan.blocks, plan.rows), dim3(LEVELS_THREADS), 0, stream_, lp);
			HIP_OK(hipGetLastError());
		}
		hipLaunchKernelGGL(levels_finish_kernel, dim3(plan.finish_grid), dim3(64), 0, stream_, lp);
		HIP_OK(hipGetLastError());
		return true;
	}
	bool measure_streams(const uint32_t *frames, bool stereo, sauengine::SampleFormat format, std::string &err) override {
		use_device();
		if (!join_mixer("measure_streams", err)) return false;
		const bool f32 = format == sauengine::SF_F32;
		if (!lev_acc_.p) { err = "level metering has not begun"; return false; }
		if (f32 != pcm_f32_ || !pcm_.p) { err = "no rows of that sample format to measure"; return false; }
		uint32_t longest = 0;
		for (uint32_t s = 0; s < cfg_.n_streams; ++s) {
			if (frames[s] > row_stride_) { err = "frames beyond the streams' rows"; return false; }
			if (frames[s] > longest) longest = frames[s];
		}
		if (!longest) return true; /* every stream has ended: nothing to add */
		const LevelsPlan plan = plan_levels(longest, stereo ? 2 : 1, cfg_.n_streams);
		if (!plan.ok) { err = "too many streams for one level measurement"; return false; }
		if (!lev_frames_.ensure(cfg_.n_streams, err) || !send(lev_frames_.p, frames, (size_t)cfg_.n_streams * sizeof(uint32_t), err)) return false;
		LevelsParams lp;
		memset((void *)&lp, 0, sizeof lp);
		lp.rows = pcm_.p; lp.pitch = pcm_pitch(); /* (rows start on 256 bytes: reserve_frames) */
		lp.row_frames = lev_frames_.p;
		lp.channels = stereo ? 2 : 1;
		lp.acc = lev_acc_.p; lp.n_rows = cfg_.n_streams; lp.f32 = f32 ? 1 : 0; lp.accumulate = 1;
		return launch_levels(lp, plan, err);
	}
	static void levels_out(const LevelsAcc &a, sauengine::Levels &o) {
		o.frames = a.frames;
		for (int c = 0; c < 2; ++c) {
			/* int16 runs: one conversion, here (a batch of int16 runs alone has fpeak and fsum +0: max and sum leave the int16 part as it is) */
			const float ip = (float)a.ipeak[c] / 32767.0f;
			o.peak[c] = a.fpeak[c] > ip ? a.fpeak[c] : ip;
			o.sum_sq[c] = a.fsum[c] + (double)a.isum[c] / (32767.0 * 32767.0);
			o.over[c] = a.over[c]; o.full_scale[c] = a.full[c]; o.nonfinite[c] = a.nonf[c];
		}
	}
	bool read_records(const LevelsAcc *dev, size_t n, sauengine::Levels *out, std::string &err) {
		std::vector<LevelsAcc> h(n);
		HIP_OK(hipMemcpyAsync(h.data(), dev, n * sizeof(LevelsAcc), hipMemcpyDeviceToHost, stream_));
		HIP_OK(hipStreamSynchronize(stream_));
		for (size_t i = 0; i < n; ++i) levels_out(h[i], out[i]);
		return true;
	}
	bool read_levels(sauengine::Levels *out, bool reset, std::string &err) override {
		use_device();
		if (!join_mixer("read_levels", err)) return false;
		if (!lev_acc_.p) { memset((void *)out, 0, sizeof(sauengine::Levels) * cfg_.n_streams); return true; }
		if (!read_records(lev_acc_.p, cfg_.n_streams, out, err)) return false;
		if (reset) HIP_OK(hipMemsetAsync(lev_acc_.p, 0, (size_t)cfg_.n_streams * sizeof(LevelsAcc), stream_));
		return true;
	}
	bool measure_rows(const void *rows, size_t pitch, size_t n_rows, sauengine::SampleFormat format, size_t frames, bool stereo,
			sauengine::Levels *out, std::string &err) override {
		use_device();
		if (!join_mixer("measure_rows", err)) return false;
		const bool f32 = format == sauengine::SF_F32;
		const size_t ch = stereo ? 2 : 1, size = f32 ? sizeof(float) : sizeof(int16_t);
		if (!n_rows) return true;
		if (!rows || ((uintptr_t)rows & 15u) || (pitch & 15u) || !out) { err = "bad argument: rows and pitch_bytes must be multiples of 16"; return false; }
		if (frames > SIZE_MAX / 8 || (n_rows > 1 && frames * ch * size > pitch)) { err = "bad argument: rows longer than their pitch"; return false; }
		if (frames) { /* the rows are read by a kernel: they have to lie inside one allocation of this device */
			hipPointerAttribute_t at;
			memset((void *)&at, 0, sizeof at);
			if (hipPointerGetAttributes(&at, rows) != hipSuccess) { (void)hipGetLastError(); err = "bad argument: rows is not device memory"; return false; }
			if (at.type != hipMemoryTypeDevice || at.device != dev_) { err = "bad argument: rows must be memory of the batch's device"; return false; }
			hipDeviceptr_t base = nullptr;
			size_t span = 0;
			if (hipMemGetAddressRange(&base, &span, (hipDeviceptr_t)rows) != hipSuccess) { (void)hipGetLastError(); err = "bad argument: rows is not device memory"; return false; }
			size_t need = 0;
			const bool wraps = __builtin_mul_overflow(pitch, n_rows - 1, &need) || __builtin_add_overflow(need, frames * ch * size, &need);
			const size_t ofs = (size_t)((const char *)rows - (const char *)base);
			if (wraps || ofs > span || need > span - ofs) { err = "bad argument: the rows reach beyond their allocation"; return false; }
		}
		const LevelsPlan plan = plan_levels(frames, (uint32_t)ch, n_rows);
		if (!plan.ok) { err = "bad argument: too many rows (65535 at most) or frames for one level measurement"; return false; }
		if (!lev_out_.ensure(n_rows, err)) return false;
		LevelsParams lp;
		memset((void *)&lp, 0, sizeof lp);
		lp.rows = rows; lp.pitch = pitch; lp.row_frames = nullptr; lp.frames = frames;
		lp.channels = (uint32_t)ch;
		lp.acc = lev_out_.p; lp.n_rows = (uint32_t)n_rows; lp.f32 = f32 ? 1 : 0; lp.accumulate = 0;
		return launch_levels(lp, plan, err) && read_records(lev_out_.p, n_rows, out, err);
	}
	bool requantize(uint32_t stream, uint32_t frames, bool stereo, float gain, sauengine::SampleFormat out, bool swap_bytes,
			std::string &err) override {
		use_device();
		if (!join_mixer("requantize", err)) return false;
		if (!pcm_f32_ || !pcm_.p) { err = "the last run's samples are not float32"; return false; }
		if (stream >= cfg_.n_streams || frames > row_stride_) { err = "frames beyond the stream's row"; return false; }
		const bool f32 = out == sauengine::SF_F32;
		if (f32 && swap_bytes) { err = "float32 samples are not byte-swapped"; return false; }
		const size_t n = (size_t)frames * (stereo ? 2 : 1);
		if (!n) return true;
		if (!requant_.ensure(n * (f32 ? sizeof(float) : sizeof(int16_t)), err)) return false;
		RequantParams rq;
		rq.src = (const float *)pcm_at(stream); rq.dst = requant_.p; rq.n = n; rq.gain = gain; rq.swap_bytes = swap_bytes ? 1 : 0;
		const dim3 grid((unsigned)((n + 1023) / 1024));
		if (f32) hipLaunchKernelGGL(requant_kernel<float>, grid, dim3(256), 0, stream_, rq);
		else hipLaunchKernelGGL(requant_kernel<int16_t>, grid, dim3(256), 0, stream_, rq);
		HIP_OK(hipGetLastError());
		return true;
	}
	/* (the next run's requant_kernel is ordered behind this copy on the one stream: one buffer serves both host slots) */
	bool fetch_requant_async(void *dst, size_t bytes, int slot, std::string &err) override {
		slot &= 3;
		use_device();
		if (!join_mixer("fetch_requant_async", err)) return false;
		if (bytes > requant_.bytes) { err = "more bytes than were requantised"; return false; }
		if (!fetch_ev_[slot]) HIP_OK(hipEventCreateWithFlags(&fetch_ev_[slot], hipEventDisableTiming));
		HIP_OK(hipMemcpyAsync(dst, requant_.p, bytes, hipMemcpyDeviceToHost, stream_));
		HIP_OK(hipEventRecord(fetch_ev_[slot], stream_));
		return true;
	}

	/* ---- the decimator (k_decimate.h; the geometry is launch_plan.h's plan_decimate) ---- */
	bool begin_decimation(int factor, bool stereo, std::string &err) override {
		use_device();
		if (!join_mixer("begin_decimation", err)) return false;
		const DecimPlan plan = plan_decimate(0, factor, stereo ? 2 : 1, cfg_.n_streams, sizeof(float));
		if (!plan.ok) { err = "bad argument"; return false; }
		const size_t hist = (size_t)cfg_.n_streams * plan.hist_floats;
		if (!decim_hist_.ensure(hist, err) || !decim_taps_.ensure(plan.taps, err) || !decim_frames_.ensure(cfg_.n_streams, err)) return false;
		HIP_OK(hipMemsetAsync(decim_hist_.p, 0, hist * sizeof(float), stream_)); /* (behind the last sequence's kernels on the one stream) */
		std::vector<double> h(plan.taps);
		if (sauengine::decimator_taps(factor, h.data(), h.size()) != plan.taps) { err = "bad argument"; return false; }
		if (!send(decim_taps_.p, h.data(), h.size() * sizeof(double), err)) return false;
		decim_factor_ = factor; decim_stereo_ = stereo;
		return true;
	}
	template <int K, typename OutT> void launch_decimate(const DecimPlan &plan, const DecimParams &dp, bool stereo) {
		const dim3 grid(plan.tiles, plan.streams), block(DECIM_THREADS);
		if (stereo) hipLaunchKernelGGL((decimate_kernel<K, OutT, 2>), grid, block, 0, stream_, dp, (const double *)decim_taps_.p);
		else hipLaunchKernelGGL((decimate_kernel<K, OutT, 1>), grid, block, 0, stream_, dp, (const double *)decim_taps_.p);
	}
	bool decimate(const uint32_t *frames_hi, uint32_t buf_len, int factor, bool stereo, sauengine::SampleFormat out_fmt, bool swap_bytes,
			std::string &err) override {
		use_device();
		if (!join_mixer("decimate", err)) return false;
		if (!decim_hist_.p || factor != decim_factor_ || stereo != decim_stereo_) { err = "decimation has not begun"; return false; }
		const bool f32 = out_fmt == sauengine::SF_F32;
		if (f32 && swap_bytes) { err = "float32 samples are not byte-swapped"; return false; }
		const uint32_t ch = stereo ? 2 : 1;
		const DecimPlan plan = plan_decimate(buf_len, factor, ch, cfg_.n_streams, f32 ? sizeof(float) : sizeof(int16_t));
		if (!plan.ok) { err = "bad argument"; return false; }
		const unsigned long long n_hi = (unsigned long long)buf_len * (unsigned)factor;
		bool any = false;
		for (uint32_t s = 0; s < cfg_.n_streams; ++s) {
			if (frames_hi[s] > n_hi || frames_hi[s] > row_stride_) { err = "frames beyond the streams' rows"; return false; }
			any = any || frames_hi[s] != 0;
		}
		if (any && (!pcm_f32_ || !pcm_.p)) { err = "the last run's samples are not float32"; return false; }
		decim_out_f32_ = f32; decim_out_pitch_ = plan.out_pitch; decim_out_bytes_ = (size_t)buf_len * ch * (f32 ? sizeof(float) : sizeof(int16_t));
		if (!plan.tiles) return true; /* no output frame: nothing to launch, and the history stands */
		if (!decim_out_.ensure(plan.out_pitch * cfg_.n_streams, err)) return false;
		if (!send(decim_frames_.p, frames_hi, (size_t)cfg_.n_streams * sizeof(uint32_t), err)) return false;
		DecimParams dp;
		memset((void *)&dp, 0, sizeof dp);
		dp.rows = (const float *)pcm_.p; dp.row_pitch = pcm_f32_ ? pcm_pitch() : 0; /* (rows start on 256 bytes: reserve_frames) */
		dp.frames = decim_frames_.p; dp.hist = decim_hist_.p;
		dp.out = decim_out_.p; dp.out_pitch = plan.out_pitch;
		dp.buf_len = buf_len; dp.swap_bytes = swap_bytes ? 1 : 0;
		switch (factor * 2 + (f32 ? 1 : 0)) {
		case 5: launch_decimate<2, float>(plan, dp, stereo); break;
		case 4: launch_decimate<2, int16_t>(plan, dp, stereo); break;
		case 9: launch_decimate<4, float>(plan, dp, stereo); break;
		case 8: launch_decimate<4, int16_t>(plan, dp, stereo); break;
		case 17: launch_decimate<8, float>(plan, dp, stereo); break;
		default: launch_decimate<8, int16_t>(plan, dp, stereo); break;
		}
		HIP_OK(hipGetLastError());
		/* behind decimate_kernel on the one stream: every read of the old history has finished */
		hipLaunchKernelGGL(decimate_carry_kernel, dim3(plan.streams), dim3(DECIM_CARRY_THREADS), 0, stream_, dp, plan.hist_floats, ch, n_hi);
		HIP_OK(hipGetLastError());
		return true;
	}
	/* (the next run's decimate_kernel is ordered behind this copy on the one stream) */
	bool fetch_decimated_async(uint32_t stream, void *dst, size_t bytes, int slot, std::string &err) override {
		slot &= 3;
		use_device();
		if (!join_mixer("fetch_decimated_async", err)) return false;
		if (stream >= cfg_.n_streams || bytes > decim_out_bytes_ || (bytes && !decim_out_.p)) { err = "more bytes than were decimated"; return false; }
		if (!fetch_ev_[slot]) HIP_OK(hipEventCreateWithFlags(&fetch_ev_[slot], hipEventDisableTiming));
		if (bytes) {
			const char *src = (const char *)decim_out_.p + decim_out_pitch_ * stream;
			if (host_blocks_.count(dst)) HIP_OK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream_));
			else { /* pageable memory: through the page-locked block, as fetch_pcm goes */
				if (!h_pcm_.ensure((bytes + 1) / 2, err)) return false;
				HIP_OK(hipMemcpyAsync(h_pcm_.p, src, bytes, hipMemcpyDeviceToHost, stream_));
				HIP_OK(hipStreamSynchronize(stream_));
				memcpy(dst, h_pcm_.p, bytes);
			}
		}
		HIP_OK(hipEventRecord(fetch_ev_[slot], stream_));
		return true;
	}
	const float *device_decimated_f32(uint32_t stream) override {
		join_mixer_quiet("device_decimated");
		return decim_out_.p && decim_out_f32_ && decim_out_bytes_ && stream < cfg_.n_streams ? (const float *)((const char *)decim_out_.p + decim_out_pitch_ * stream) : nullptr;
	}
	size_t device_decimated_pitch() override { join_mixer_quiet("device_decimated"); return decim_out_.p && decim_out_bytes_ ? decim_out_pitch_ : 0; }

	/* ---- loudness and true peak (k_loudness.h; the geometry is launch_plan.h's plan_loudness) ---- */
	/* the records of a set of rows: the batch's streams, or the foreign rows of one measure_loudness_rows call */
	struct LoudSet {
		DevBuf<LoudState> state;
		DevBuf<unsigned long long> pos;
		DevBuf<double> E;
		DevBuf<uint32_t> peak;
		DevBuf<float> hist;
		std::vector<uint64_t> pos_h; /* the host's copy of pos: what E has to hold is known without asking the device */
		size_t e_cap = 0;            /* hops E holds per row */
		uint32_t rows = 0, channels = 0;
	};
	bool loud_setup(uint32_t srate, std::string &err) {
		if (loud_rate_ == srate) return true;
		double f[10], m[16];
		if (!sauengine::loudness_filter(srate, f)) { err = "bad argument: loudness metering needs a rate of 2560 Hz or more"; return false; }
		sauengine::loudness_chunk_map(f, LOUD_CHUNK, m);
		loud_f_ = LoudFilter{f[0], f[1], f[2], f[3], f[4], f[5], f[6], f[7], f[8], f[9]};
		for (int r = 0; r < 4; ++r) for (int k = 0; k < 4; ++k) loud_m_.m[r][k] = m[4 * r + k];
		if (!loud_taps_.p) {
			double g[TP_TAPS];
			if (sauengine::truepeak_taps(g, TP_TAPS) != TP_TAPS || !loud_taps_.ensure(TP_TAPS, err) || !send(loud_taps_.p, g, sizeof g, err)) return false;
		}
		loud_rate_ = srate;
		return true;
	}
	bool loud_clear(LoudSet &L, std::string &err) {
		HIP_OK(hipMemsetAsync(L.state.p, 0, (size_t)L.rows * 2 * sizeof(LoudState), stream_));
		HIP_OK(hipMemsetAsync(L.pos.p, 0, (size_t)L.rows * sizeof(unsigned long long), stream_));
		HIP_OK(hipMemsetAsync(L.peak.p, 0, (size_t)L.rows * 2 * sizeof(uint32_t), stream_));
		HIP_OK(hipMemsetAsync(L.hist.p, 0, (size_t)L.rows * TP_LEAD * 2 * sizeof(float), stream_));
		if (L.e_cap) HIP_OK(hipMemsetAsync(L.E.p, 0, L.e_cap * L.rows * 2 * sizeof(double), stream_));
		L.pos_h.assign(L.rows, 0);
		L.channels = 0;
		return true;
	}
	bool loud_make(LoudSet &L, size_t rows, std::string &err) {
		if (L.rows != rows && L.E.p) { /* (E is [hop][row][2]: another number of rows is another block) */
			HIP_OK(hipStreamSynchronize(stream_));
			L.E.release();
			L.e_cap = 0;
		}
		L.rows = (uint32_t)rows;
		if (!L.state.ensure(rows * 2, err) || !L.pos.ensure(rows, err) || !L.peak.ensure(rows * 2, err) || !L.hist.ensure(rows * TP_LEAD * 2, err)) return false;
		return loud_clear(L, err);
	}
	/* E grows by reallocation on the backend's stream: the hops so far are copied, the rest is cleared, and the old block goes
	 * back to the pool once the stream has drained. [hop][row][2]: the rows' hops so far are a prefix of the block. */
	bool loud_grow(LoudSet &L, size_t need, std::string &err) {
		if (need <= L.e_cap) return true;
		const size_t want = need + need / 2 + 32, per = (size_t)L.rows * 2;
		DevBuf<double> nb;
		if (!nb.ensure(want * per, err)) return false;
		if (L.e_cap) HIP_OK(hipMemcpyAsync(nb.p, L.E.p, L.e_cap * per * sizeof(double), hipMemcpyDeviceToDevice, stream_));
		HIP_OK(hipMemsetAsync(nb.p + L.e_cap * per, 0, (want - L.e_cap) * per * sizeof(double), stream_));
		if (L.E.p) { HIP_OK(hipStreamSynchronize(stream_)); L.E.release(); }
		L.E.p = nb.p; L.E.cap = nb.cap; L.E.bytes = nb.bytes;
		nb.p = nullptr; nb.cap = 0; nb.bytes = 0;
		L.e_cap = want;
		return true;
	}
	/* the launches of one measurement, on the backend's stream: frames[r] frames of row r */
	bool loud_measure(LoudSet &L, const void *rows, size_t pitch, const uint32_t *frames, uint32_t ch, std::string &err) {
		uint32_t longest = 0;
		for (uint32_t r = 0; r < L.rows; ++r) if (frames[r] > longest) longest = frames[r];
		if (!longest) return true; /* no row has a frame: nothing changes */
		const LoudPlan plan = plan_loudness(longest, ch, L.rows, loud_rate_);
		if (!plan.ok) { err = "bad argument: too many rows (65535 at most) for one loudness measurement"; return false; }
		size_t need = 0;
		for (uint32_t r = 0; r < L.rows; ++r) {
			const size_t h = (size_t)((L.pos_h[r] + frames[r]) / plan.hop) + 1; /* (the hop the row's end lies in: loud_finish_kernel loads it) */
			if (h > need) need = h;
		}
		if (!loud_grow(L, need, err)) return false;
		const size_t lanes = (size_t)L.rows * 2 * plan.chunks;
		if (!loud_z_.ensure(lanes, err) || !loud_s_.ensure(lanes, err) || !loud_parts_.ensure(lanes * 2, err) ||
		    !loud_tp_parts_.ensure((size_t)L.rows * plan.tiles * 2, err) || !loud_frames_.ensure(L.rows, err) ||
		    !send(loud_frames_.p, frames, (size_t)L.rows * sizeof(uint32_t), err))
			return false;
		LoudParams lp;
		memset((void *)&lp, 0, sizeof lp);
		lp.rows = (const float *)rows; lp.row_pitch = pitch; lp.frames = loud_frames_.p;
		lp.channels = ch; lp.n_rows = L.rows; lp.hop = plan.hop; lp.chunk_cap = plan.chunks; lp.tile_cap = plan.tiles;
		lp.state = L.state.p; lp.pos = L.pos.p; lp.zstate = loud_z_.p; lp.sstate = loud_s_.p; lp.parts = loud_parts_.p;
		lp.E = L.E.p; lp.e_cap = (uint32_t)(L.e_cap > 0xffffffffull ? 0xffffffffull : L.e_cap);
		lp.tp_parts = loud_tp_parts_.p; lp.peak = L.peak.p; lp.hist = L.hist.p;
		const dim3 cgrid(plan.chunk_grid, plan.rows), tgrid(plan.tiles, plan.rows);
		if (ch == 2) hipLaunchKernelGGL((loud_chunk_kernel<2, 0>), cgrid, dim3(LOUD_THREADS), 0, stream_, lp, loud_f_);
		else hipLaunchKernelGGL((loud_chunk_kernel<1, 0>), cgrid, dim3(LOUD_THREADS), 0, stream_, lp, loud_f_);
		HIP_OK(hipGetLastError());
		hipLaunchKernelGGL(loud_scan_kernel, dim3(plan.lane_grid), dim3(64), 0, stream_, lp, loud_m_);
		HIP_OK(hipGetLastError());
		if (ch == 2) hipLaunchKernelGGL((loud_chunk_kernel<2, 1>), cgrid, dim3(LOUD_THREADS), 0, stream_, lp, loud_f_);
		else hipLaunchKernelGGL((loud_chunk_kernel<1, 1>), cgrid, dim3(LOUD_THREADS), 0, stream_, lp, loud_f_);
		HIP_OK(hipGetLastError());
		if (ch == 2) hipLaunchKernelGGL(truepeak_kernel<2>, tgrid, dim3(TP_THREADS), 0, stream_, lp, (const double *)loud_taps_.p);
		else hipLaunchKernelGGL(truepeak_kernel<1>, tgrid, dim3(TP_THREADS), 0, stream_, lp, (const double *)loud_taps_.p);
		HIP_OK(hipGetLastError());
		/* behind both on the one stream: every partial record is written, every read of the old history has finished */
		hipLaunchKernelGGL(loud_finish_kernel, dim3((plan.rows + 63) / 64), dim3(64), 0, stream_, lp);
		HIP_OK(hipGetLastError());
		hipLaunchKernelGGL(loud_carry_kernel, dim3(plan.rows), dim3(64), 0, stream_, lp);
		HIP_OK(hipGetLastError());
		for (uint32_t r = 0; r < L.rows; ++r) L.pos_h[r] += frames[r];
		L.channels = ch;
		return true;
	}
	/* wait for the stream; the rows' records -- gated hops, peaks with the tail covered in the copy -- and, where asked for,
	 * the complete hops of every row, [row][hops][2] with `hops_stride` hops per row */
	bool loud_read(LoudSet &L, sauengine::Loudness *out, std::vector<double> *hops_out, size_t *hops_stride, std::string &err) {
		const size_t per = (size_t)L.rows * 2;
		const uint32_t hop = loud_rate_ / 10, ch = L.channels ? L.channels : 1;
		size_t max_hops = 0;
		for (uint32_t r = 0; r < L.rows; ++r) { const size_t h = (size_t)(L.pos_h[r] / hop); if (h > max_hops) max_hops = h; }
		std::vector<double> E(max_hops * per);
		std::vector<uint32_t> peak(per);
		std::vector<float> hist((size_t)L.rows * TP_LEAD * 2);
		if (max_hops) HIP_OK(hipMemcpyAsync(E.data(), L.E.p, E.size() * sizeof(double), hipMemcpyDeviceToHost, stream_));
		HIP_OK(hipMemcpyAsync(peak.data(), L.peak.p, per * sizeof(uint32_t), hipMemcpyDeviceToHost, stream_));
		HIP_OK(hipMemcpyAsync(hist.data(), L.hist.p, hist.size() * sizeof(float), hipMemcpyDeviceToHost, stream_));
		HIP_OK(hipStreamSynchronize(stream_));
		double g[TP_TAPS];
		(void)sauengine::truepeak_taps(g, TP_TAPS);
		if (hops_out) { hops_out->assign((size_t)L.rows * max_hops * 2, 0.0); *hops_stride = max_hops; }
		std::vector<double> mine;
		for (uint32_t r = 0; r < L.rows; ++r) {
			const size_t nh = (size_t)(L.pos_h[r] / hop);
			mine.assign(nh * 2, 0.0);
			for (size_t h = 0; h < nh; ++h) { mine[2 * h] = E[h * per + (size_t)r * 2]; mine[2 * h + 1] = E[h * per + (size_t)r * 2 + 1]; }
			if (!sauengine::loudness_gate(mine.data(), nh, hop, (int)ch, &out[r])) { err = "bad argument"; return false; }
			out[r].frames = L.pos_h[r];
			uint32_t pk[2] = {peak[(size_t)r * 2], peak[(size_t)r * 2 + 1]};
			if (L.pos_h[r]) sauengine::truepeak_tail(hist.data() + (size_t)r * TP_LEAD * 2, (int)ch, g, pk);
			memcpy(out[r].true_peak, pk, sizeof pk);
			if (hops_out && nh) memcpy(hops_out->data() + (size_t)r * max_hops * 2, mine.data(), nh * 2 * sizeof(double));
		}
		return true;
	}
	bool begin_loudness(std::string &err) override {
		use_device();
		if (!join_mixer("begin_loudness", err)) return false;
		if (loud_own_.state.p) return true;
		return loud_setup(cfg_.srate, err) && loud_make(loud_own_, cfg_.n_streams, err);
	}
	bool measure_loudness(const uint32_t *frames, bool stereo, std::string &err) override {
		use_device();
		if (!join_mixer("measure_loudness", err)) return false;
		if (!loud_own_.state.p) { err = "loudness metering has not begun"; return false; }
		if (!pcm_f32_ || !pcm_.p) { err = "the last run's samples are not float32"; return false; }
		for (uint32_t s = 0; s < cfg_.n_streams; ++s)
			if (frames[s] > row_stride_) { err = "frames beyond the streams' rows"; return false; }
		if (!loud_setup(cfg_.srate, err)) return false; /* (a measure_loudness_rows call at another rate has been in between) */
		return loud_measure(loud_own_, pcm_.p, pcm_pitch(), frames, stereo ? 2 : 1, err); /* (rows start on 256 bytes: reserve_frames) */
	}
	bool read_loudness(sauengine::Loudness *out, bool reset, std::string &err) override {
		use_device();
		if (!join_mixer("read_loudness", err)) return false;
		if (!loud_own_.state.p) { err = "loudness metering has not begun"; return false; }
		if (!loud_setup(cfg_.srate, err) || !loud_read(loud_own_, out, nullptr, nullptr, err)) return false;
		return !reset || loud_clear(loud_own_, err);
	}
	bool read_loudness_hops(uint32_t stream, double *out, size_t cap, size_t *n_hops, std::string &err) override {
		use_device();
		if (!join_mixer("read_loudness_hops", err)) return false;
		if (!loud_own_.state.p || stream >= cfg_.n_streams) { err = "loudness metering has not begun"; return false; }
		const uint32_t hop = cfg_.srate / 10;
		const size_t nh = (size_t)(loud_own_.pos_h[stream] / hop), per = (size_t)loud_own_.rows * 2;
		*n_hops = nh;
		if (!out || cap < nh || !nh) return true;
		/* (the stream's two doubles of every hop: a strided copy, in order behind the measurements on the one stream) */
		HIP_OK(hipMemcpy2DAsync(out, 2 * sizeof(double), loud_own_.E.p + (size_t)stream * 2, per * sizeof(double), 2 * sizeof(double), nh,
				hipMemcpyDeviceToHost, stream_));
		HIP_OK(hipStreamSynchronize(stream_));
		return true;
	}
	bool measure_loudness_rows(const void *rows, size_t pitch, size_t n_rows, size_t frames, bool stereo, uint32_t srate,
			sauengine::Loudness *out, double *hops_out, size_t hops_cap, std::string &err) override {
		use_device();
		if (!join_mixer("measure_loudness_rows", err)) return false;
		const size_t ch = stereo ? 2 : 1, size = sizeof(float);
		if (!n_rows) return true;
		if (!rows || ((uintptr_t)rows & 15u) || (pitch & 15u) || !out) { err = "bad argument: rows and pitch_bytes must be multiples of 16"; return false; }
		if (frames > 0xffffffffull || (n_rows > 1 && frames * ch * size > pitch)) { err = "bad argument: rows longer than their pitch, or than 32 bits of frames"; return false; }
		if (srate < LOUD_MIN_RATE || n_rows > LOUD_MAX_ROWS) { err = "bad argument: a rate below 2560 Hz, or more than 65535 rows"; return false; }
		if (frames) { /* the rows are read by kernels: they have to lie inside one allocation of this device */
			hipPointerAttribute_t at;
			memset((void *)&at, 0, sizeof at);
			if (hipPointerGetAttributes(&at, rows) != hipSuccess) { (void)hipGetLastError(); err = "bad argument: rows is not device memory"; return false; }
			if (at.type != hipMemoryTypeDevice || at.device != dev_) { err = "bad argument: rows must be memory of the batch's device"; return false; }
			hipDeviceptr_t base = nullptr;
			size_t span = 0;
			if (hipMemGetAddressRange(&base, &span, (hipDeviceptr_t)rows) != hipSuccess) { (void)hipGetLastError(); err = "bad argument: rows is not device memory"; return false; }
			size_t need = 0;
			const bool wraps = __builtin_mul_overflow(pitch, n_rows - 1, &need) || __builtin_add_overflow(need, frames * ch * size, &need);
			const size_t ofs = (size_t)((const char *)rows - (const char *)base);
			if (wraps || ofs > span || need > span - ofs) { err = "bad argument: the rows reach beyond their allocation"; return false; }
		}
		const size_t nh = frames / (srate / 10);
		if (hops_out && hops_cap < n_rows * nh * 2) hops_out = nullptr; /* (nothing is written when the capacity does not suffice) */
		if (!loud_setup(srate, err) || !loud_make(loud_rows_, n_rows, err)) return false;
		loud_rows_.channels = (uint32_t)ch;
		const std::vector<uint32_t> fr(n_rows, (uint32_t)frames);
		std::vector<double> hops;
		size_t stride = 0;
		const bool ok = loud_measure(loud_rows_, rows, pitch, fr.data(), (uint32_t)ch, err) &&
			loud_read(loud_rows_, out, hops_out ? &hops : nullptr, &stride, err);
		if (ok && hops_out && !hops.empty()) memcpy(hops_out, hops.data(), hops.size() * sizeof(double)); /* (equal rows: stride == nh) */
		return ok;
	}

	/* ---- the limiter (k_limiter.h; the geometry is launch_plan.h's plan_limit) ---- */
	/* the window and the true-peak taps of the rate at hand (a limit_rows call at another rate may have been in between) */
	bool lim_setup(uint32_t srate, std::string &err) {
		if (!lim_taps_.p) {
			double g[TP_TAPS];
			if (sauengine::truepeak_taps(g, TP_TAPS) != TP_TAPS || !lim_taps_.ensure(TP_TAPS, err) || !send(lim_taps_.p, g, sizeof g, err)) return false;
		}
		if (lim_rate_ == srate) return true;
		std::vector<double> h(sauengine::limiter_window(srate, nullptr, 0));
		if (h.empty() || sauengine::limiter_window(srate, h.data(), h.size()) != h.size()) { err = "bad argument"; return false; }
		if (!lim_win_.ensure(2 * LIM_A_MAX + 1, err) || !send(lim_win_.p, h.data(), h.size() * sizeof(double), err)) return false;
		lim_rate_ = srate;
		return true;
	}
	/* the launches of one pass, on the backend's stream; lp carries rows, frames, history, output, statistics and base */
	template <typename OutT> void lim_launch_gain(const LimitPlan &plan, const LimParams &lp, bool stereo) {
		const dim3 grid(plan.tiles, plan.streams), block(LIM_THREADS);
		if (stereo) hipLaunchKernelGGL((lim_gain_kernel<OutT, 2>), grid, block, 0, stream_, lp, (const double *)lim_win_.p);
		else hipLaunchKernelGGL((lim_gain_kernel<OutT, 1>), grid, block, 0, stream_, lp, (const double *)lim_win_.p);
	}
	bool lim_launch(const LimitPlan &plan, LimParams &lp, bool stereo, bool f32, std::string &err) {
		const size_t sc = plan.scratch_pitch * plan.streams, parts = (size_t)plan.tiles * plan.streams;
		if (!lim_s_.ensure(sc, err) || !lim_r_.ensure(sc, err) || !lim_part_min_.ensure(parts, err) || !lim_part_cnt_.ensure(parts, err)) return false;
		lp.s = lim_s_.p; lp.r = lim_r_.p; lp.scratch_pitch = plan.scratch_pitch;
		lp.part_min = lim_part_min_.p; lp.part_cnt = lim_part_cnt_.p;
		lp.env_n = plan.env_n; lp.A = plan.A; lp.hist_frames = plan.hist_frames; lp.tiles = plan.tiles; lp.n_streams = plan.streams;
		const dim3 egrid(plan.env_tiles, plan.streams), block(LIM_THREADS);
		if (stereo) hipLaunchKernelGGL(lim_env_kernel<2>, egrid, block, 0, stream_, lp, (const double *)lim_taps_.p);
		else hipLaunchKernelGGL(lim_env_kernel<1>, egrid, block, 0, stream_, lp, (const double *)lim_taps_.p);
		HIP_OK(hipGetLastError());
		if (f32) lim_launch_gain<float>(plan, lp, stereo);
		else lim_launch_gain<int16_t>(plan, lp, stereo);
		HIP_OK(hipGetLastError());
		hipLaunchKernelGGL(lim_finish_kernel, dim3(plan.streams), dim3(64), 0, stream_, lp);
		HIP_OK(hipGetLastError());
		return true;
	}
	bool lim_clear_stats(LimStats *dst, size_t n, std::string &err) {
		const std::vector<LimStats> empty(n, LimStats{0, 0, 1.0});
		return send(dst, empty.data(), n * sizeof(LimStats), err);
	}
	bool begin_limiting(bool stereo, std::string &err) override {
		use_device();
		if (!join_mixer("begin_limiting", err)) return false;
		const LimitPlan plan = plan_limit(0, cfg_.srate, stereo ? 2 : 1, cfg_.n_streams, sizeof(float));
		if (!plan.ok) { err = "bad argument"; return false; }
		const size_t hist = (size_t)cfg_.n_streams * plan.hist_frames * 2;
		if (!lim_hist_[0].ensure(hist, err) || !lim_hist_[1].ensure(hist, err) || !lim_frames_.ensure(cfg_.n_streams, err)) return false;
		if (!lim_stats_.p) {
			if (!lim_stats_.ensure(cfg_.n_streams, err) || !lim_clear_stats(lim_stats_.p, cfg_.n_streams, err)) return false;
		}
		lim_cur_ = 0;
		HIP_OK(hipMemsetAsync(lim_hist_[0].p, 0, hist * sizeof(float), stream_)); /* (behind the last sequence's kernels on the one stream) */
		lim_on_ = true; lim_stereo_ = stereo;
		return true;
	}
	bool limit(const uint32_t *frames, uint32_t buf_len, float pre_gain, float ceiling, bool stereo, sauengine::SampleFormat out_fmt,
			bool swap_bytes, std::string &err) override {
		use_device();
		if (!join_mixer("limit", err)) return false;
		if (!lim_on_ || stereo != lim_stereo_) { err = "limiting has not begun"; return false; }
		if (!sauengine::limiter_param_ok(pre_gain) || !sauengine::limiter_param_ok(ceiling)) { err = "bad argument"; return false; }
		const bool f32 = out_fmt == sauengine::SF_F32;
		if (f32 && swap_bytes) { err = "float32 samples are not byte-swapped"; return false; }
		const uint32_t ch = stereo ? 2 : 1;
		const LimitPlan plan = plan_limit(buf_len, cfg_.srate, ch, cfg_.n_streams, f32 ? sizeof(float) : sizeof(int16_t));
		if (!plan.ok) { err = "bad argument"; return false; }
		bool any = false;
		for (uint32_t s = 0; s < cfg_.n_streams; ++s) {
			if (frames[s] > buf_len || frames[s] > row_stride_) { err = "frames beyond the streams' rows"; return false; }
			any = any || frames[s] != 0;
		}
		if (any && (!pcm_f32_ || !pcm_.p)) { err = "the last run's samples are not float32"; return false; }
		lim_out_f32_ = f32; lim_out_pitch_ = plan.out_pitch; lim_out_bytes_ = (size_t)buf_len * ch * (f32 ? sizeof(float) : sizeof(int16_t));
		if (!plan.tiles) return true; /* no output frame: nothing to launch, and the history stands */
		if (!lim_setup(cfg_.srate, err) || !lim_out_.ensure(plan.out_pitch * cfg_.n_streams, err)) return false;
		if (!send(lim_frames_.p, frames, (size_t)cfg_.n_streams * sizeof(uint32_t), err)) return false;
		LimParams lp;
		memset((void *)&lp, 0, sizeof lp);
		lp.rows = (const float *)pcm_.p; lp.row_pitch = pcm_f32_ ? pcm_pitch() : 0;
		lp.frames = lim_frames_.p;
		lp.hist = lim_hist_[lim_cur_].p; lp.hist_next = lim_hist_[lim_cur_ ^ 1].p;
		lp.out = lim_out_.p; lp.out_pitch = plan.out_pitch;
		lp.stats = lim_stats_.p;
		lp.base = -(long long)plan.D - 2 * (long long)plan.A; /* output 0 is the sequence's frame (run's first) - D */
		lp.n_out = buf_len; lp.run_frames = buf_len; lp.swap_bytes = swap_bytes ? 1 : 0;
		lp.pre_gain = pre_gain; lp.ceiling = ceiling;
		if (!lim_launch(plan, lp, stereo, f32, err)) return false;
		hipLaunchKernelGGL(lim_carry_kernel, dim3((plan.hist_frames * ch + LIM_THREADS - 1) / LIM_THREADS, plan.streams), dim3(LIM_THREADS), 0,
				stream_, lp, ch);
		HIP_OK(hipGetLastError());
		lim_cur_ ^= 1;
		return true;
	}
	/* (the next run's kernels are ordered behind this copy on the one stream) */
	bool fetch_limited_async(uint32_t stream, void *dst, size_t bytes, int slot, std::string &err) override {
		slot &= 3;
		use_device();
		if (!join_mixer("fetch_limited_async", err)) return false;
		if (stream >= cfg_.n_streams || bytes > lim_out_bytes_ || (bytes && !lim_out_.p)) { err = "more bytes than were limited"; return false; }
		if (!fetch_ev_[slot]) HIP_OK(hipEventCreateWithFlags(&fetch_ev_[slot], hipEventDisableTiming));
		if (bytes) {
			const char *src = (const char *)lim_out_.p + lim_out_pitch_ * stream;
			if (host_blocks_.count(dst)) HIP_OK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream_));
			else { /* pageable memory: through the page-locked block, as fetch_pcm goes */
				if (!h_pcm_.ensure((bytes + 1) / 2, err)) return false;
				HIP_OK(hipMemcpyAsync(h_pcm_.p, src, bytes, hipMemcpyDeviceToHost, stream_));
				HIP_OK(hipStreamSynchronize(stream_));
				memcpy(dst, h_pcm_.p, bytes);
			}
		}
		HIP_OK(hipEventRecord(fetch_ev_[slot], stream_));
		return true;
	}
	const float *device_limited_f32(uint32_t stream) override {
		join_mixer_quiet("device_limited");
		return lim_out_.p && lim_out_f32_ && lim_out_bytes_ && stream < cfg_.n_streams ? (const float *)((const char *)lim_out_.p + lim_out_pitch_ * stream) : nullptr;
	}
	size_t device_limited_pitch() override { join_mixer_quiet("device_limited"); return lim_out_.p && lim_out_bytes_ ? lim_out_pitch_ : 0; }
	bool read_limiter_stats(sauengine::LimiterStats *out, bool reset, std::string &err) override {
		use_device();
		if (!join_mixer("read_limiter_stats", err)) return false;
		if (!lim_stats_.p) { err = "limiting has not begun"; return false; }
		HIP_OK(hipMemcpyAsync(out, lim_stats_.p, (size_t)cfg_.n_streams * sizeof(LimStats), hipMemcpyDeviceToHost, stream_));
		HIP_OK(hipStreamSynchronize(stream_));
		return !reset || lim_clear_stats(lim_stats_.p, cfg_.n_streams, err);
	}
	/* is [p, p + pitch * (n_rows - 1) + row_bytes) inside one allocation of this device? (the rows are read or written by kernels) */
	bool lim_rows_inside(const void *p, size_t pitch, size_t n_rows, size_t row_bytes, const char *what, std::string &err) {
		hipPointerAttribute_t at;
		memset((void *)&at, 0, sizeof at);
		if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); err = std::string("bad argument: ") + what + " is not device memory"; return false; }
		if (at.type != hipMemoryTypeDevice || at.device != dev_) { err = std::string("bad argument: ") + what + " must be memory of the batch's device"; return false; }
		hipDeviceptr_t base = nullptr;
		size_t span = 0;
		if (hipMemGetAddressRange(&base, &span, (hipDeviceptr_t)p) != hipSuccess) { (void)hipGetLastError(); err = std::string("bad argument: ") + what + " is not device memory"; return false; }
		size_t need = 0;
		const bool wraps = __builtin_mul_overflow(pitch, n_rows - 1, &need) || __builtin_add_overflow(need, row_bytes, &need);
		const size_t ofs = (size_t)((const char *)p - (const char *)base);
		if (wraps || ofs > span || need > span - ofs) { err = std::string("bad argument: ") + what + " reaches beyond its allocation"; return false; }
		return true;
	}
	bool limit_rows(const void *rows, size_t pitch, size_t n_rows, size_t frames, bool stereo, uint32_t srate, float pre_gain, float ceiling,
			void *out_rows, size_t out_pitch, sauengine::LimiterStats *stats_out, std::string &err) override {
		use_device();
		if (!join_mixer("limit_rows", err)) return false;
		const size_t ch = stereo ? 2 : 1, row_bytes = frames * ch * sizeof(float);
		if (!sauengine::limiter_param_ok(pre_gain) || !sauengine::limiter_param_ok(ceiling) || !srate) { err = "bad argument"; return false; }
		if (!rows || !out_rows || ((uintptr_t)rows & 15u) || (pitch & 15u) || ((uintptr_t)out_rows & 15u) || (out_pitch & 15u)) {
			err = "bad argument: rows, out_rows and their pitches must be multiples of 16"; return false;
		}
		if (frames > 0xffffffffull - 4 * LIM_A_MAX || (n_rows > 1 && (row_bytes > pitch || row_bytes > out_pitch))) {
			err = "bad argument: rows longer than their pitch, or than 32 bits of frames"; return false;
		}
		if (n_rows > LIM_MAX_STREAMS) { err = "bad argument: more than 65535 rows"; return false; }
		for (size_t r = 0; stats_out && r < n_rows; ++r) stats_out[r] = sauengine::LimiterStats{0, 0, 1.0};
		if (!n_rows || !frames) return true;
		if (!lim_rows_inside(rows, pitch, n_rows, row_bytes, "rows", err) || !lim_rows_inside(out_rows, out_pitch, n_rows, row_bytes, "out_rows", err)) return false;
		{ /* the two sets of rows may not share a byte: a tile's input reaches into its neighbours' output */
			const uintptr_t a0 = (uintptr_t)rows, a1 = a0 + pitch * (n_rows - 1) + row_bytes, b0 = (uintptr_t)out_rows, b1 = b0 + out_pitch * (n_rows - 1) + row_bytes;
			if (a0 < b1 && b0 < a1) { err = "bad argument: out_rows overlaps rows"; return false; }
		}
		const LimitPlan plan = plan_limit(frames, srate, (uint32_t)ch, n_rows, sizeof(float));
		if (!plan.ok) { err = "bad argument"; return false; }
		if (!lim_setup(srate, err) || !lim_rows_frames_.ensure(n_rows, err) || !lim_rows_stats_.ensure(n_rows, err)) return false;
		const std::vector<uint32_t> fr(n_rows, (uint32_t)frames);
		if (!send(lim_rows_frames_.p, fr.data(), n_rows * sizeof(uint32_t), err) || !lim_clear_stats(lim_rows_stats_.p, n_rows, err)) return false;
		LimParams lp;
		memset((void *)&lp, 0, sizeof lp);
		lp.rows = (const float *)rows; lp.row_pitch = pitch;
		lp.frames = lim_rows_frames_.p;
		lp.out = out_rows; lp.out_pitch = out_pitch;
		lp.stats = lim_rows_stats_.p;
		lp.base = -2 * (long long)plan.A; /* output 0 is the rows' frame 0: the delay is dropped */
		lp.n_out = (uint32_t)frames; lp.run_frames = (uint32_t)frames;
		lp.pre_gain = pre_gain; lp.ceiling = ceiling;
		if (!lim_launch(plan, lp, stereo, true, err)) return false;
		std::vector<LimStats> st(n_rows);
		HIP_OK(hipMemcpyAsync(st.data(), lim_rows_stats_.p, n_rows * sizeof(LimStats), hipMemcpyDeviceToHost, stream_));
		HIP_OK(hipStreamSynchronize(stream_));
		if (stats_out) memcpy((void *)stats_out, st.data(), n_rows * sizeof(LimStats));
		return true;
	}

	/* ---- the spectrum meter (k_spectrum.h; the geometry is launch_plan.h's plan_spectrum) ----
	 * A meter is records of its own on this backend's device and stream: sums, the group at hand, the pending frames (two
	 * buffers: spec_carry_kernel moves from one into the other). Where a row stands is kept on the host -- the frame counts
	 * of a feed are host values -- and every feed uploads what the kernels need of it (SpecRow). */
	class Spectrum : public sauengine::SpectrumMeter {
	public:
		Spectrum(HipBackendImpl *be, size_t n_rows, uint32_t channels, unsigned log2n, uint32_t hop)
			: be_(be), n_(n_rows), ch_(channels), L_(log2n), N_(1u << log2n), bins_((1u << log2n) / 2 + 1), hop_(hop), pos_(n_rows, 0) {}
		~Spectrum() override { /* the buffers go back to the pool (member destructors): nothing may still be using them */
			be_->use_device();
			if (be_->stream_) { be_->join_mixer_quiet("spectrum"); (void)hipStreamSynchronize(be_->stream_); }
		}
		size_t n_rows() const override { return n_; }
		uint32_t channels() const override { return ch_; }
		uint32_t log2n() const override { return L_; }
		bool init(std::string &err) {
			const SpectrumPlan plan = plan_spectrum(L_, hop_, ch_, n_, nullptr);
			if (!plan.ok) { err = "bad argument"; return false; }
			const size_t sums = n_ * plan.sum_pitch, pend = n_ * plan.pend_pitch;
			if (!total_.ensure(sums, err) || !acc_.ensure(sums, err) || !pend_[0].ensure(pend, err) || !pend_[1].ensure(pend, err) ||
			    !desc_.ensure(n_, err) || !win_.ensure(N_, err) || !tw_.ensure(N_, err))
				return false;
			std::vector<double> t(N_);
			if (sauengine::spectrum_window(L_, t.data(), N_) != N_ || !be_->send(win_.p, t.data(), N_ * sizeof(double), err)) return false;
			if (sauengine::spectrum_twiddles(L_, t.data(), N_) != N_ || !be_->send(tw_.p, t.data(), N_ * sizeof(double), err)) return false;
			return clear(err);
		}
		bool clear(std::string &err) {
			if (!be_->join_mixer("spectrum_clear", err)) return false;
			HIP_OK(hipMemsetAsync(total_.p, 0, n_ * bins_ * ch_ * sizeof(double), be_->stream_)); /* (+0.0; behind the last feed's kernels) */
			std::fill(pos_.begin(), pos_.end(), 0);
			return true;
		}
		/* sgram: feed()'s segment kernel also writes every segment's (float)p[k] there (spectrum_rows: rows from empty records) */
		bool feed_into(const void *rows, size_t pitch, const uint32_t *frames, float *sgram, size_t sgram_segs, std::string &err) {
			be_->use_device();
			if (!be_->join_mixer("spectrum_feed", err)) return false; /* (the rows fed may be the batch's PCM) */
			if (!rows || !frames || ((uintptr_t)rows & 15u) || (pitch & 15u)) { err = "bad argument: rows and pitch_bytes must be multiples of 16"; return false; }
			uint32_t longest = 0;
			for (size_t r = 0; r < n_; ++r) longest = frames[r] > longest ? frames[r] : longest;
			if (!longest) return true; /* nothing changes, and the rows are not looked at */
			const size_t row_bytes = (size_t)longest * ch_ * sizeof(float);
			if (n_ > 1 && row_bytes > pitch) { err = "bad argument: rows longer than their pitch"; return false; }
			/* the rows are read by kernels: they have to lie inside one allocation of this device */
			if (!be_->lim_rows_inside(rows, pitch, n_, row_bytes, "rows", err)) return false;
			std::vector<SpecRow> d(n_);
			for (size_t r = 0; r < n_; ++r) d[r] = plan_spectrum_row(pos_[r], frames[r], N_, hop_);
			const SpectrumPlan plan = plan_spectrum(L_, hop_, ch_, n_, d.data());
			if (!plan.ok) { err = "bad argument: too many frames for one feed"; return false; }
			if (plan.scratch && !part_.ensure(plan.scratch, err)) return false;
			if (!be_->send(desc_.p, d.data(), n_ * sizeof(SpecRow), err)) return false;
			SpecParams sp;
			memset((void *)&sp, 0, sizeof sp);
			sp.rows = (const float *)rows; sp.row_pitch = pitch; sp.desc = desc_.p;
			sp.pend = pend_[cur_].p; sp.pend_next = pend_[cur_ ^ 1].p; sp.pend_pitch = plan.pend_pitch;
			sp.acc = acc_.p; sp.total = total_.p; sp.part = part_.p;
			sp.sgram = sgram; sp.sgram_segs = sgram_segs;
			sp.win = win_.p; sp.tw = (const double2 *)tw_.p;
			sp.hop = hop_; sp.channels = ch_; sp.max_groups = plan.max_groups;
			hipStream_t st = be_->stream_;
			if (plan.max_groups) {
				const dim3 grid(plan.max_groups, plan.rows, ch_), block(SPEC_THREADS);
				switch (L_) {
				case 8: hipLaunchKernelGGL(spec_segment_kernel<8>, grid, block, plan.lds_bytes, st, sp); break;
				case 9: hipLaunchKernelGGL(spec_segment_kernel<9>, grid, block, plan.lds_bytes, st, sp); break;
				case 10: hipLaunchKernelGGL(spec_segment_kernel<10>, grid, block, plan.lds_bytes, st, sp); break;
				case 11: hipLaunchKernelGGL(spec_segment_kernel<11>, grid, block, plan.lds_bytes, st, sp); break;
				default: hipLaunchKernelGGL(spec_segment_kernel<12>, grid, block, plan.lds_bytes, st, sp); break;
				}
				HIP_OK(hipGetLastError());
				hipLaunchKernelGGL(spec_finish_kernel, dim3((bins_ + SPEC_THREADS - 1) / SPEC_THREADS, plan.rows, ch_), block, 0, st, sp, bins_);
				HIP_OK(hipGetLastError());
			}
			hipLaunchKernelGGL(spec_carry_kernel, dim3((uint32_t)((plan.pend_pitch + SPEC_THREADS - 1) / SPEC_THREADS), plan.rows), dim3(SPEC_THREADS), 0, st, sp);
			HIP_OK(hipGetLastError());
			cur_ ^= 1;
			for (size_t r = 0; r < n_; ++r) pos_[r] += frames[r];
			return true;
		}
		bool feed(const void *rows, size_t pitch, const uint32_t *frames, std::string &err) override {
			return feed_into(rows, pitch, frames, nullptr, 0, err);
		}
		bool read(double *power_out, uint64_t *segments_out, bool reset, std::string &err) override {
			be_->use_device();
			if (!be_->join_mixer("spectrum_read", err)) return false;
			const size_t sums = n_ * bins_ * ch_;
			std::vector<double> acc(sums);
			HIP_OK(hipMemcpyAsync(power_out, total_.p, sums * sizeof(double), hipMemcpyDeviceToHost, be_->stream_));
			HIP_OK(hipMemcpyAsync(acc.data(), acc_.p, sums * sizeof(double), hipMemcpyDeviceToHost, be_->stream_));
			HIP_OK(hipStreamSynchronize(be_->stream_));
			for (size_t r = 0; r < n_; ++r) {
				const uint64_t S = sauengine::spectrum_segments(pos_[r], N_, hop_);
				segments_out[r] = S;
				if (S % SPEC_GROUP) /* the group at hand, in the copy: the device state is untouched */
					for (size_t k = r * bins_ * ch_; k < (r + 1) * bins_ * ch_; ++k) power_out[k] = power_out[k] + acc[k];
			}
			return !reset || clear(err);
		}
	private:
		HipBackendImpl *be_;
		size_t n_;
		uint32_t ch_, L_, N_, bins_, hop_;
		std::vector<uint64_t> pos_; /* per row: frames fed so far */
		DevBuf<double> total_, acc_, part_, win_, tw_;
		DevBuf<float> pend_[2];
		DevBuf<SpecRow> desc_;
		int cur_ = 0;
	};
	sauengine::SpectrumMeter *create_spectrum(size_t n_rows, uint32_t channels, unsigned log2n, uint32_t hop, std::string &err) override {
		use_device();
		if (!join_mixer("create_spectrum", err)) return nullptr;
		if (!sauengine::spectrum_params_ok((int)channels, log2n, hop) || !n_rows) { err = "bad argument"; return nullptr; }
		if (n_rows > SPEC_MAX_ROWS) { err = "bad argument: more than 65535 rows"; return nullptr; }
		Spectrum *m = new Spectrum(this, n_rows, channels, log2n, hop);
		if (!m->init(err)) { delete m; return nullptr; }
		return m;
	}
	bool spectrum_rows(const void *rows, size_t pitch, size_t n_rows, size_t frames, uint32_t channels, unsigned log2n, uint32_t hop,
			double *power_out, uint64_t *segments_out, float *spectrogram_out, size_t spectrogram_cap, std::string &err) override {
		use_device();
		if (!join_mixer("spectrum_rows", err)) return false;
		if (!sauengine::spectrum_params_ok((int)channels, log2n, hop) || !n_rows || !power_out || !segments_out) { err = "bad argument"; return false; }
		if (!rows || ((uintptr_t)rows & 15u) || (pitch & 15u)) { err = "bad argument: rows and pitch_bytes must be multiples of 16"; return false; }
		if (n_rows > SPEC_MAX_ROWS || frames > 0xffffffffull) { err = "bad argument: more than 65535 rows, or than 32 bits of frames"; return false; }
		const uint32_t N = 1u << log2n, bins = N / 2 + 1;
		const uint64_t S = sauengine::spectrum_segments(frames, N, hop);
		size_t sg = 0;
		if (spectrogram_out && (__builtin_mul_overflow((size_t)S, (size_t)bins * channels, &sg) || __builtin_mul_overflow(sg, n_rows, &sg) || sg > spectrogram_cap)) {
			err = "bad argument: the spectrogram needs more floats than spectrogram_cap"; return false;
		}
		Spectrum m(this, n_rows, channels, log2n, hop);
		if (!m.init(err)) return false;
		if (spectrogram_out && sg && !spec_gram_.ensure(sg, err)) return false;
		const std::vector<uint32_t> fr(n_rows, (uint32_t)frames);
		if (!m.feed_into(rows, pitch, fr.data(), spectrogram_out && sg ? spec_gram_.p : nullptr, (size_t)S, err)) return false;
		if (!m.read(power_out, segments_out, false, err)) return false;
		if (spectrogram_out && sg) HIP_OK(hipMemcpy(spectrogram_out, spec_gram_.p, sg * sizeof(float), hipMemcpyDeviceToHost));
		return true;
	}

	/* ---- the FLAC encoder (k_flac.h; the geometry is launch_plan.h's plan_flac) ----
	 * An encoder is streams of its own on this backend's device and stream: the pending frames (two buffers, as the spectrum
	 * meter's), a running record per row, and the output of every feed not yet read -- one block of device memory per feed with
	 * room for its worst case, in which a row's frames lie back to back from the row's offset on. Where a row stands is kept on
	 * the host. The unread total that the 1 GiB rule counts is the feeds' worst cases until a read has fetched the sizes. */
	class Flac : public sauengine::FlacEncoder {
	public:
		/* f32: a float-fed encoder of `bits` per sample (feed_f32); else the int16-fed one (bits 16) */
		Flac(HipBackendImpl *be, size_t n_rows, uint32_t channels, uint32_t block_frames, uint32_t max_lpc_order, bool f32 = false, uint32_t bits = 16)
			: be_(be), n_(n_rows), ch_(channels), B_(sauflac::flac_block_frames(block_frames)), M_(max_lpc_order), f32_(f32), bits_(bits),
			  pos_(n_rows, 0), blocks_(n_rows, 0) {
			/* (tests: another limit of unread bytes than 1 GiB) */
			if (const char *v = sauengine::tune_env("SAU_AMD_FLAC_UNREAD_MAX")) { const long long x = atoll(v); if (x > 0) limit_ = (uint64_t)x; }
		}
		~Flac() override { /* the buffers go back to the pool (member destructors): nothing may still be using them */
			be_->use_device();
			if (be_->stream_) { be_->join_mixer_quiet("flac"); (void)hipStreamSynchronize(be_->stream_); }
		}
		size_t n_rows() const override { return n_; }
		uint32_t channels() const override { return ch_; }
		uint32_t block_frames() const override { return B_; }
		uint32_t bits() const override { return bits_; }
		bool init(std::string &err) {
			const FlacPlan plan = plan_flac(B_, ch_, n_, nullptr, bits_);
			if (!plan.ok) { err = "bad argument"; return false; }
			const size_t pend = n_ * plan.pend_pitch * (bits_ == 24 ? 2 : 1); /* (int16 units: the wide kernels' pending samples are int32) */
			if (!pend_[0].ensure(pend, err) || !pend_[1].ensure(pend, err) || !desc_.ensure(n_, err) || !stats_.ensure(n_, err)) return false;
			if (f32_ && !qdesc_.ensure(n_, err)) return false;
			return clear(err);
		}
		/* new streams: behind a read, which has waited for the stream */
		bool clear(std::string &err) {
			if (!be_->join_mixer("flac_clear", err)) return false;
			HIP_OK(hipMemsetAsync(stats_.p, 0, n_ * sizeof(FlacStats), be_->stream_));
			if (md5_on_ && !md5_reset(err)) return false;
			if (verify_on_ && !verify_reset(err)) return false;
			std::fill(pos_.begin(), pos_.end(), 0);
			std::fill(blocks_.begin(), blocks_.end(), 0);
			closed_ = false;
			return true;
		}
		/* MD5 (k_md5.h): a running state of four words and a digest per row, and the row's byte count for a finish */
		bool set_md5(bool on, std::string &err) override {
			be_->use_device();
			if (closed_) { err = "bad argument: the streams are not at their start (read with reset first)"; return false; }
			for (size_t r = 0; r < n_; ++r)
				if (pos_[r]) { err = "bad argument: the streams are not at their start (read with reset first)"; return false; }
			if (on) {
				if (!md5_state_.ensure(4 * n_, err) || !md5_digest_.ensure(4 * n_, err) || !md5_desc_.ensure(n_, err)) return false;
				if (!be_->join_mixer("flac_set_md5", err) || !md5_reset(err)) return false;
			}
			md5_on_ = on;
			return true;
		}
		bool md5(uint8_t *out, std::string &err) override {
			be_->use_device();
			if (!md5_on_ || !closed_ || !out) { err = !out ? "bad argument" : !md5_on_ ? "bad argument: MD5 is off (set_md5)" : "bad argument: the streams are not finished"; return false; }
			if (!be_->join_mixer("flac_md5", err)) return false;
			HIP_OK(hipStreamSynchronize(be_->stream_));
			HIP_OK(hipMemcpy(out, md5_digest_.p, 16 * n_, hipMemcpyDeviceToHost));
			return true;
		}
		/* the verify mode (k_flac_dec.h): a record of three words per row */
		bool set_verify(bool on, std::string &err) override {
			be_->use_device();
			if (closed_) { err = "bad argument: the streams are not at their start (read with reset first)"; return false; }
			for (size_t r = 0; r < n_; ++r)
				if (pos_[r]) { err = "bad argument: the streams are not at their start (read with reset first)"; return false; }
			if (on) {
				if (!verify_rec_.ensure(n_, err)) return false;
				if (!be_->join_mixer("flac_set_verify", err) || !verify_reset(err)) return false;
			}
			verify_on_ = on;
			return true;
		}
		bool verify(sauengine::FlacVerify *out, std::string &err) override {
			be_->use_device();
			if (!verify_on_ || !out) { err = !out ? "bad argument" : "bad argument: verify is off (set_verify)"; return false; }
			if (!be_->join_mixer("flac_verify", err)) return false;
			HIP_OK(hipStreamSynchronize(be_->stream_));
			std::vector<FlacVerifyRec> rec(n_);
			HIP_OK(hipMemcpy(rec.data(), verify_rec_.p, n_ * sizeof(FlacVerifyRec), hipMemcpyDeviceToHost));
			for (size_t r = 0; r < n_; ++r) {
				const bool bad = rec[r].bad_blocks != 0;
				out[r].blocks = rec[r].blocks; out[r].bad_blocks = rec[r].bad_blocks;
				out[r].first_bad_block = bad ? rec[r].first >> 8 : 0;
				out[r].first_status = bad ? (uint32_t)(rec[r].first & 0xffu) : 0; out[r].pad_ = 0;
			}
			return true;
		}
		bool feed(const void *rows, size_t pitch, const uint32_t *frames, bool finish, std::string &err) override {
			if (f32_) { err = "bad argument: this encoder is fed float rows (feed_f32)"; return false; }
			return feed_any(rows, pitch, frames, nullptr, finish, err);
		}
		bool feed_f32(const void *rows, size_t pitch, const uint32_t *frames, const float *gains, bool finish, std::string &err) override {
			if (!f32_) { err = "bad argument: this encoder is fed int16 rows (feed)"; return false; }
			return feed_any(rows, pitch, frames, gains, finish, err);
		}
		/* a float-fed encoder's feed differs in what it asks of the rows, and in the quantiser ahead of the other kernels, which
		 * then read the encoder's own rows; every refusal comes before anything is queued or changed */
		bool feed_any(const void *rows, size_t pitch, const uint32_t *frames, const float *gains, bool finish, std::string &err) {
			be_->use_device();
			if (!be_->join_mixer("flac_feed", err)) return false; /* (the rows fed may be the batch's PCM) */
			const uintptr_t align = f32_ ? 3u : 15u;
			if (!rows || !frames || ((uintptr_t)rows & align) || (pitch & align)) {
				err = f32_ ? "bad argument: rows and pitch_bytes must be multiples of 4" : "bad argument: rows and pitch_bytes must be multiples of 16";
				return false;
			}
			for (size_t r = 0; f32_ && gains && r < n_; ++r)
				if (!(gains[r] >= -FLT_MAX && gains[r] <= FLT_MAX)) { err = "bad argument: a gain is not finite"; return false; }
			if (closed_) { err = "bad argument: the streams are finished (read with reset first)"; return false; }
			uint32_t longest = 0;
			for (size_t r = 0; r < n_; ++r) longest = frames[r] > longest ? frames[r] : longest;
			if (!longest && !finish) return true; /* nothing changes, and the rows are not looked at */
			if (longest) {
				const size_t row_bytes = (size_t)longest * ch_ * (f32_ ? sizeof(float) : sizeof(int16_t));
				if (n_ > 1 && row_bytes > pitch) { err = "bad argument: rows longer than their pitch"; return false; }
				/* the rows are read by kernels: they have to lie inside one allocation of this device */
				if (!be_->lim_rows_inside(rows, pitch, n_, row_bytes, "rows", err)) return false;
			}
			const bool wide = bits_ == 24;
			std::vector<FlacRow> d(n_);
			for (size_t r = 0; r < n_; ++r) d[r] = plan_flac_row(pos_[r], frames[r], B_, finish);
			const FlacPlan plan = plan_flac(B_, ch_, n_, d.data(), bits_);
			if (!plan.ok) { err = "bad argument: too many frames for one feed, or for one stream"; return false; }
			if (bound_ + plan.worst > limit_) { err = "bad argument: the unread output could pass its limit (read first)"; return false; }
			std::unique_ptr<Chunk> c;
			if (plan.jobs) {
				c.reset(new Chunk);
				if (!frames_.ensure(plan.jobs, err) || !c->out.ensure(plan.out_bytes, err) || !c->row_bytes.ensure(n_, err)) return false;
				c->off.resize(n_);
				for (size_t r = 0; r < n_; ++r) c->off[r] = d[r].out_off;
			}
			/* a float-fed encoder's own rows: as long as the feed's longest row, on a pitch that is a multiple of 256 */
			const size_t q_pitch = ((size_t)longest * ch_ * (wide ? sizeof(int32_t) : sizeof(int16_t)) + 255) & ~(size_t)255;
			if (f32_ && longest && !qrows_.ensure(n_ * q_pitch, err)) return false;
			if (!be_->send(desc_.p, d.data(), n_ * sizeof(FlacRow), err)) return false;
			const bool md5_now = md5_on_ && (plan.jobs || finish); /* (a finish that completes no block still pads) */
			if (md5_now) {
				std::vector<FlacMd5Row> m(n_);
				for (size_t r = 0; r < n_; ++r) m[r].total = (pos_[r] + frames[r]) * ch_ * (wide ? 3 : 2);
				if (!be_->send(md5_desc_.p, m.data(), n_ * sizeof(FlacMd5Row), err)) return false;
			}
			hipStream_t st = be_->stream_;
			if (f32_ && longest) {
				std::vector<FlacQuantRow> q(n_);
				for (size_t r = 0; r < n_; ++r) { q[r].n = (unsigned long long)frames[r] * ch_; q[r].gain = gains ? gains[r] : 1.0f; q[r].pad_ = 0; }
				if (!be_->send(qdesc_.p, q.data(), n_ * sizeof(FlacQuantRow), err)) return false;
				FlacQuantParams qp;
				qp.src = (const float *)rows; qp.src_pitch = pitch; qp.dst = qrows_.p; qp.dst_pitch = q_pitch; qp.rows = qdesc_.p;
				/* thread 0 of a row takes the samples ahead of the first 16-byte boundary, every other thread four */
				const dim3 grid((uint32_t)(((unsigned long long)longest * ch_ / 4 + 2 + 255) / 256), (uint32_t)n_);
				if (wide) hipLaunchKernelGGL(flac_quant_kernel<int32_t>, grid, dim3(256), 0, st, qp);
				else hipLaunchKernelGGL(flac_quant_kernel<int16_t>, grid, dim3(256), 0, st, qp);
				HIP_OK(hipGetLastError());
				rows = qrows_.p; pitch = q_pitch;
			}
			FlacParams fp;
			memset((void *)&fp, 0, sizeof fp);
			fp.rows = rows; fp.row_pitch = pitch; fp.desc = desc_.p;
			fp.pend = pend_[cur_].p; fp.pend_next = pend_[cur_ ^ 1].p; fp.pend_pitch = plan.pend_pitch;
			fp.frames = frames_.p; fp.stats = stats_.p;
			fp.B = B_; fp.channels = ch_; fp.n_rows = (uint32_t)n_; fp.jobs = plan.jobs; fp.max_lpc = M_;
			if (plan.jobs) { fp.out = c->out.p; fp.row_bytes = c->row_bytes.p; }
			FlacMd5Params mp; /* (reads what the analysis reads: the rows at hand and the pending frames ahead of the carry) */
			memset((void *)&mp, 0, sizeof mp);
			mp.rows = rows; mp.row_pitch = pitch; mp.desc = desc_.p; mp.pend = pend_[cur_].p; mp.pend_pitch = plan.pend_pitch;
			mp.md5 = md5_desc_.p; mp.state = md5_state_.p; mp.digest = md5_digest_.p;
			mp.B = B_; mp.channels = ch_; mp.n_rows = (uint32_t)n_; mp.finish = finish ? 1 : 0;
			/* the feed's launches at one width (k_flac.h: FlacS16, FlacS32); flac_scan_kernel is the same for both */
			auto launch = [&](auto w, auto md5_kernel) -> bool {
				typedef decltype(w) W;
				if (plan.jobs) {
					/* (max_lpc_order 0 runs the kernels without the LPC mode's code: the encoder as it was before that mode) */
					auto analyze = flac_analyze_kernel<W, false>, write = flac_write_kernel<W, false>;
					if (M_) { analyze = flac_analyze_kernel<W, true>; write = flac_write_kernel<W, true>; }
					hipLaunchKernelGGL(analyze, dim3(plan.jobs), dim3(plan.analyze_threads), plan.analyze_lds, st, fp);
					HIP_OK(hipGetLastError());
					hipLaunchKernelGGL(flac_scan_kernel, dim3(plan.rows), dim3(FLAC_THREADS), 0, st, fp);
					HIP_OK(hipGetLastError());
					hipLaunchKernelGGL(write, dim3(plan.jobs), dim3(FLAC_THREADS), plan.write_lds, st, fp);
					HIP_OK(hipGetLastError());
				}
				if (verify_on_ && plan.jobs) { /* behind the writer, ahead of the carry: the rows and the pending frames are the analysis' */
					FlacDecArgs da;
					memset((void *)&da, 0, sizeof da);
					da.rec = verify_rec_.p;
					hipLaunchKernelGGL((flac_decode_kernel<W, true>), dim3(plan.jobs), dim3(FLAC_THREADS), plan_flac_decode_lds(B_, ch_, bits_), st, fp, da);
					HIP_OK(hipGetLastError());
				}
				if (md5_now) {
					hipLaunchKernelGGL(md5_kernel, dim3(plan.rows), dim3(64), 0, st, mp);
					HIP_OK(hipGetLastError());
				}
				if (!finish) { /* (behind a finish nothing is pending) */
					hipLaunchKernelGGL(flac_carry_kernel<W>, dim3((uint32_t)((plan.pend_pitch + FLAC_THREADS - 1) / FLAC_THREADS), plan.rows), dim3(FLAC_THREADS), 0, st, fp);
					HIP_OK(hipGetLastError());
					cur_ ^= 1;
				}
				return true;
			};
			if (!(wide ? launch(FlacS32(), flac_md5_wide_kernel) : launch(FlacS16(), flac_md5_kernel))) return false;
			for (size_t r = 0; r < n_; ++r) { pos_[r] += frames[r]; blocks_[r] += d[r].n_blocks; }
			if (c) chunks_.push_back(std::move(c));
			bound_ += plan.worst;
			closed_ = finish;
			return true;
		}
		bool read(uint8_t *const *bufs, const size_t *caps, size_t *bytes_out, sauengine::FlacInfo *info_out, bool reset, std::string &err) override {
			be_->use_device();
			if (!be_->join_mixer("flac_read", err)) return false;
			if (!bytes_out || (bufs && !caps)) { err = "bad argument"; return false; }
			HIP_OK(hipStreamSynchronize(be_->stream_));
			std::vector<uint64_t> total(n_, 0);
			for (auto &c : chunks_) {
				if (c->len.empty()) { /* (fetched once: a read that consumes nothing may come again) */
					c->len.resize(n_);
					HIP_OK(hipMemcpy(c->len.data(), c->row_bytes.p, n_ * sizeof(uint32_t), hipMemcpyDeviceToHost));
				}
				for (size_t r = 0; r < n_; ++r) total[r] += c->len[r];
			}
			std::vector<FlacStats> st(n_);
			HIP_OK(hipMemcpy(st.data(), stats_.p, n_ * sizeof(FlacStats), hipMemcpyDeviceToHost));
			uint64_t all = 0;
			for (size_t r = 0; r < n_; ++r) {
				all += total[r];
				if (bufs && total[r] && (!bufs[r] || caps[r] < total[r])) { err = "bad argument: a buffer is too small for its row's bytes"; return false; }
			}
			if (bufs) {
				std::vector<size_t> at(n_, 0);
				for (auto &c : chunks_)
					for (size_t r = 0; r < n_; ++r)
						if (c->len[r]) {
							HIP_OK(hipMemcpyAsync(bufs[r] + at[r], c->out.p + c->off[r], c->len[r], hipMemcpyDeviceToHost, be_->stream_));
							at[r] += c->len[r];
						}
				HIP_OK(hipStreamSynchronize(be_->stream_));
				chunks_.clear();
				bound_ = 0;
			} else
				bound_ = all; /* (the sizes are known now) */
			for (size_t r = 0; r < n_; ++r) {
				bytes_out[r] = (size_t)total[r];
				if (info_out) {
					info_out[r].frames = pos_[r]; info_out[r].blocks = blocks_[r]; info_out[r].bytes = st[r].bytes;
					info_out[r].min_frame_bytes = st[r].min_bytes; info_out[r].max_frame_bytes = st[r].max_bytes;
				}
			}
			if (reset) { /* new streams: what is pending or unread goes */
				chunks_.clear();
				bound_ = 0;
				return clear(err);
			}
			return true;
		}
	private:
		/* every row's running state back to MD5's initial value, on the stream */
		bool md5_reset(std::string &err) {
			std::vector<uint32_t> s(4 * n_);
			for (size_t r = 0; r < n_; ++r) saumd5::md5_init(&s[4 * r]);
			return be_->send(md5_state_.p, s.data(), s.size() * sizeof(uint32_t), err);
		}
		/* every row's record back to nothing checked, on the stream */
		bool verify_reset(std::string &err) {
			const FlacVerifyRec none = {0, 0, ~0ull};
			const std::vector<FlacVerifyRec> rec(n_, none);
			return be_->send(verify_rec_.p, rec.data(), n_ * sizeof(FlacVerifyRec), err);
		}
		struct Chunk { /* one feed's output */
			DevBuf<uint8_t> out;
			DevBuf<uint32_t> row_bytes;  /* [rows]: flac_scan_kernel's word on them */
			std::vector<uint32_t> off;   /* [rows]: where a row's frames begin in `out` */
			std::vector<uint32_t> len;   /* [rows]: row_bytes on the host, once a read has fetched them */
		};
		HipBackendImpl *be_;
		size_t n_;
		uint32_t ch_, B_, M_;
		bool f32_;                           /* fed float rows (feed_f32), quantised into qrows_ */
		uint32_t bits_;                      /* 16, or 24: the wide kernels */
		std::vector<uint64_t> pos_, blocks_; /* per row: frames fed, blocks made */
		std::vector<std::unique_ptr<Chunk>> chunks_;
		uint64_t bound_ = 0, limit_ = sauflac::FLAC_MAX_UNREAD;
		bool closed_ = false;
		DevBuf<int16_t> pend_[2];
		DevBuf<FlacRow> desc_;
		DevBuf<FlacStats> stats_;
		DevBuf<FlacFrameDesc> frames_;
		DevBuf<unsigned char> qrows_;        /* a float-fed encoder's quantised rows of the feed at hand */
		DevBuf<FlacQuantRow> qdesc_;
		bool md5_on_ = false;                /* set_md5: flac_md5_kernel runs behind the write kernel */
		DevBuf<uint32_t> md5_state_, md5_digest_; /* [rows][4] each */
		DevBuf<FlacMd5Row> md5_desc_;
		bool verify_on_ = false;             /* set_verify: flac_decode_kernel<W, true> runs behind the write kernel */
		DevBuf<FlacVerifyRec> verify_rec_;   /* [rows] */
		int cur_ = 0;
	};
	sauengine::FlacEncoder *create_flac(size_t n_rows, uint32_t channels, uint32_t block_frames, std::string &err) override {
		return create_flac_lpc(n_rows, channels, block_frames, 0, err);
	}
	sauengine::FlacEncoder *create_flac_lpc(size_t n_rows, uint32_t channels, uint32_t block_frames, uint32_t max_lpc_order, std::string &err) override {
		use_device();
		if (!join_mixer("create_flac", err)) return nullptr;
		if (!sauengine::flac_params_ok((int)channels, block_frames) || !n_rows || max_lpc_order > sauflac::FLAC_LPC_MAX) { err = "bad argument"; return nullptr; }
		if (n_rows > sauflac::FLAC_MAX_ROWS) { err = "bad argument: more than 65535 rows"; return nullptr; }
		Flac *e = new Flac(this, n_rows, channels, block_frames, max_lpc_order);
		if (!e->init(err)) { delete e; return nullptr; }
		return e;
	}
	sauengine::FlacEncoder *create_flac_f32(size_t n_rows, uint32_t channels, uint32_t block_frames, int bits, uint32_t max_lpc_order, std::string &err) override {
		return create_flac_float(n_rows, channels, block_frames, bits, max_lpc_order, false, err);
	}
	/* the float-fed encoder of 24 bits in the LPC mode (the header's "LPC at 24 bits"); order 0 is create_flac_f32's encoder */
	sauengine::FlacEncoder *create_flac_lpc24(size_t n_rows, uint32_t channels, uint32_t block_frames, uint32_t max_lpc_order, std::string &err) override {
		return create_flac_float(n_rows, channels, block_frames, 24, max_lpc_order, true, err);
	}
	/* (lpc24: asked for through create_flac_lpc24 -- create_flac_f32 keeps refusing an order at 24 bits) */
	sauengine::FlacEncoder *create_flac_float(size_t n_rows, uint32_t channels, uint32_t block_frames, int bits, uint32_t max_lpc_order, bool lpc24,
			std::string &err) {
		use_device();
		if (!join_mixer("create_flac", err)) return nullptr;
		if (!sauengine::flac_params_ok((int)channels, block_frames) || !n_rows || !sauflac::flac_bits_ok(bits) || max_lpc_order > sauflac::FLAC_LPC_MAX) { err = "bad argument"; return nullptr; }
		if (bits == 24 && max_lpc_order && !lpc24) { err = "bad argument: no LPC mode at 24 bits"; return nullptr; }
		if (n_rows > sauflac::FLAC_MAX_ROWS) { err = "bad argument: more than 65535 rows"; return nullptr; }
		Flac *e = new Flac(this, n_rows, channels, block_frames, max_lpc_order, true, (uint32_t)bits);
		if (!e->init(err)) { delete e; return nullptr; }
		return e;
	}

	/* ---- the quantiser (k_dither.h; the geometry is launch_plan.h's plan_dither) ----
	 * A quantiser is streams of its own on this backend's device and stream: a record per chain (history and clamp counts) and
	 * the int16 rows of the feed at hand. Where a row stands is kept on the host and goes to the kernels with the feed's row
	 * records, so a feed waits for nothing. */
	class Quant : public sauengine::Quantizer {
	public:
		Quant(HipBackendImpl *be, size_t n_rows, uint32_t channels, const saudither::DitherSpec &spec)
			: be_(be), n_(n_rows), ch_(channels), spec_(spec), pos_(n_rows, 0), last_(n_rows, 0) {}
		~Quant() override { /* the buffers go back to the pool (member destructors): nothing may still be using them */
			be_->use_device();
			if (be_->stream_) { be_->join_mixer_quiet("dither"); (void)hipStreamSynchronize(be_->stream_); }
		}
		size_t n_rows() const override { return n_; }
		uint32_t channels() const override { return ch_; }
		bool init(std::string &err) {
			if (!plan_dither(spec_.taps, ch_, n_, 0).ok) { err = "bad argument"; return false; }
			if (!chains_.ensure(n_ * ch_, err) || !desc_.ensure(n_, err)) return false;
			return clear(err);
		}
		bool clear(std::string &err) {
			if (!be_->join_mixer("dither_clear", err)) return false;
			HIP_OK(hipMemsetAsync(chains_.p, 0, n_ * ch_ * sizeof(saudither::DitherChain), be_->stream_));
			std::fill(pos_.begin(), pos_.end(), 0);
			return true;
		}
		/* every refusal comes before anything is queued or changed */
		bool feed(const void *rows, size_t pitch, const uint32_t *frames, const float *gains, std::string &err) override {
			be_->use_device();
			if (!be_->join_mixer("dither_feed", err)) return false; /* (the rows fed may be the batch's PCM) */
			if (!rows || !frames || ((uintptr_t)rows & 3u) || (pitch & 3u)) { err = "bad argument: rows and pitch_bytes must be multiples of 4"; return false; }
			for (size_t r = 0; gains && r < n_; ++r)
				if (!(gains[r] >= -FLT_MAX && gains[r] <= FLT_MAX)) { err = "bad argument: a gain is not finite"; return false; }
			uint32_t longest = 0;
			for (size_t r = 0; r < n_; ++r) longest = frames[r] > longest ? frames[r] : longest;
			if (!longest) { std::fill(last_.begin(), last_.end(), 0); return true; } /* nothing changes, and the rows are not looked at */
			const size_t row_bytes = (size_t)longest * ch_ * sizeof(float);
			if (n_ > 1 && row_bytes > pitch) { err = "bad argument: rows longer than their pitch"; return false; }
			/* the rows are read by kernels: they have to lie inside one allocation of this device */
			if (!be_->lim_rows_inside(rows, pitch, n_, row_bytes, "rows", err)) return false;
			const DitherPlan plan = plan_dither(spec_.taps, ch_, n_, longest);
			if (!plan.ok) { err = "bad argument"; return false; }
			if (!out_.ensure(n_ * plan.out_pitch, err)) return false;
			std::vector<DitherRow> d(n_);
			for (size_t r = 0; r < n_; ++r) {
				d[r].first = pos_[r]; d[r].seed_r = saudither::dither_row_seed(spec_.seed, r);
				d[r].frames = frames[r]; d[r].gain = gains ? gains[r] : 1.0f;
			}
			if (!be_->send(desc_.p, d.data(), n_ * sizeof(DitherRow), err)) return false;
			DitherParams dp;
			memset((void *)&dp, 0, sizeof dp);
			dp.src = (const float *)rows; dp.src_pitch = pitch; dp.dst = (int16_t *)out_.p; dp.dst_pitch = plan.out_pitch;
			dp.rows = desc_.p; dp.chains = chains_.p; dp.n_rows = (uint32_t)n_; dp.channels = ch_;
			dp.dither = spec_.dither; dp.plain = saudither::dither_spec_plain(spec_) ? 1 : 0;
			for (unsigned j = 0; j < saudither::DITHER_TAPS_MAX; ++j) dp.coef[j] = j < spec_.taps ? spec_.coef[j] : 0.0;
			if (plan.shaped) hipLaunchKernelGGL(dither_shape_kernel, dim3(plan.shape_waves), dim3(DITHER_CHAINS), 0, be_->stream_, dp);
			else hipLaunchKernelGGL(dither_flat_kernel, dim3(plan.flat_grid_x, plan.rows), dim3(256), 0, be_->stream_, dp);
			HIP_OK(hipGetLastError());
			for (size_t r = 0; r < n_; ++r) { pos_[r] += frames[r]; last_[r] = frames[r]; }
			pitch_ = plan.out_pitch;
			return true;
		}
		const int16_t *rows() const override { return pitch_ ? (const int16_t *)out_.p : nullptr; }
		size_t pitch() const override { return pitch_; }
		bool read(int16_t *const *bufs, std::string &err) override {
			be_->use_device();
			if (!be_->join_mixer("dither_read", err)) return false;
			if (!bufs) { err = "bad argument"; return false; }
			for (size_t r = 0; r < n_; ++r)
				if (last_[r] && !bufs[r]) { err = "bad argument: no buffer for a row with frames"; return false; }
			for (size_t r = 0; r < n_; ++r)
				if (last_[r]) HIP_OK(hipMemcpyAsync(bufs[r], out_.p + pitch_ * r, (size_t)last_[r] * ch_ * sizeof(int16_t), hipMemcpyDeviceToHost, be_->stream_));
			HIP_OK(hipStreamSynchronize(be_->stream_));
			return true;
		}
		/* (the next feed's kernel is ordered behind this copy on the one stream: one set of rows serves both host slots) */
		bool fetch_async(void *dst, size_t bytes, int slot, std::string &err) override {
			slot &= 3;
			be_->use_device();
			if (!be_->join_mixer("dither_fetch_async", err)) return false;
			if (bytes > (size_t)last_[0] * ch_ * sizeof(int16_t)) { err = "more bytes than were quantised"; return false; }
			if (!be_->fetch_ev_[slot]) HIP_OK(hipEventCreateWithFlags(&be_->fetch_ev_[slot], hipEventDisableTiming));
			HIP_OK(hipMemcpyAsync(dst, out_.p, bytes, hipMemcpyDeviceToHost, be_->stream_));
			HIP_OK(hipEventRecord(be_->fetch_ev_[slot], be_->stream_));
			return true;
		}
		bool stats(sauengine::DitherStats *out, bool reset, std::string &err) override {
			be_->use_device();
			if (!be_->join_mixer("dither_stats", err)) return false;
			HIP_OK(hipStreamSynchronize(be_->stream_));
			if (out) {
				std::vector<saudither::DitherChain> c(n_ * ch_);
				HIP_OK(hipMemcpy(c.data(), chains_.p, c.size() * sizeof(saudither::DitherChain), hipMemcpyDeviceToHost));
				for (size_t r = 0; r < n_; ++r) {
					out[r].frames = pos_[r];
					out[r].clipped[0] = c[r * ch_].clipped;
					out[r].clipped[1] = ch_ == 2 ? c[r * ch_ + 1].clipped : 0;
				}
			}
			return reset ? clear(err) : true;
		}
	private:
		HipBackendImpl *be_;
		size_t n_;
		uint32_t ch_;
		saudither::DitherSpec spec_;
		std::vector<uint64_t> pos_;          /* per row: frames fed */
		std::vector<uint32_t> last_;         /* per row: frames of the last feed */
		size_t pitch_ = 0;
		DevBuf<saudither::DitherChain> chains_;
		DevBuf<DitherRow> desc_;
		DevBuf<unsigned char> out_;          /* the int16 rows of the feed at hand */
	};
	sauengine::Quantizer *create_quantizer(size_t n_rows, uint32_t channels, const saudither::DitherSpec &spec, std::string &err) override {
		use_device();
		if (!join_mixer("create_quantizer", err)) return nullptr;
		if (!n_rows || (channels != 1 && channels != 2) || !saudither::dither_spec_ok(spec)) { err = "bad argument"; return nullptr; }
		if (n_rows > saudither::DITHER_MAX_ROWS) { err = "bad argument: more than 65535 rows"; return nullptr; }
		Quant *q = new Quant(this, n_rows, channels, spec);
		if (!q->init(err)) { delete q; return nullptr; }
		return q;
	}

	/* (whoever reads the rows through these pointers orders itself behind the main stream -- sync(), stream_handle() -- and so
	 * behind the last mixer, joined here) */
	const int16_t *device_pcm(uint32_t stream) override { join_mixer_quiet("device_pcm"); return pcm_.p && !pcm_f32_ ? (const int16_t *)pcm_at(stream) : nullptr; }
	const float *device_pcm_f32(uint32_t stream) override { join_mixer_quiet("device_pcm"); return pcm_.p && pcm_f32_ ? (const float *)pcm_at(stream) : nullptr; }
	size_t device_pcm_pitch() override { join_mixer_quiet("device_pcm"); return pcm_.p ? pcm_pitch() : 0; }

	bool sync(std::string &err) override {
		use_device();
		if (!join_mixer("sync", err)) return false;
		HIP_OK(hipStreamSynchronize(stream_));
		arena_used_ = 0; /* every staged copy has left the arena */
		return true;
	}
	/* the operator records are all the state a generator has on the device (everything else is per segment): a copy of them
	 * on the generator's stream, behind the kernels of the run before and ahead of those of the run after */
	bool save_state(int slot, std::string &err) override {
		slot &= 3;
		use_device();
		if (!join_mixer("save_state", err)) return false;
		if (!ops_snap_[slot].ensure(ops_.cap, err)) return false;
		HIP_OK(hipMemcpyAsync(ops_snap_[slot].p, ops_.p, ops_.cap * sizeof(DevOp), hipMemcpyDeviceToDevice, stream_));
		return true;
	}
	bool load_state(int slot, std::string &err) override {
		slot &= 3;
		use_device();
		if (!join_mixer("load_state", err)) return false;
		if (!ops_snap_[slot].p || ops_snap_[slot].cap < ops_.cap) { err = "no operator state was saved under this slot"; return false; }
		HIP_OK(hipMemcpyAsync(ops_.p, ops_snap_[slot].p, ops_.cap * sizeof(DevOp), hipMemcpyDeviceToDevice, stream_));
		return true;
	}

	void timing(double *render_ms, double *mix_ms, uint64_t *launches, bool reset) override {
		if (!timing_on_) { timing_on_ = true; }
		use_device();
		join_mixer_quiet("timing"); /* (its pair of events is on the side stream) */
		(void)hipStreamSynchronize(stream_);
		drain_pairs();
		if (render_ms) *render_ms = acc_ms_[0] + acc_ms_[2];
		if (mix_ms) *mix_ms = acc_ms_[1];
		if (launches) *launches = acc_launches_;
		if (reset) { acc_ms_[0] = acc_ms_[1] = acc_ms_[2] = acc_ms_[3] = 0; acc_launches_ = 0; }
	}

	size_t chain_rows_budget() override { return sauengine::chain_rows_budget(free_hint_, chain_rows_failures_); }
	/* (what the caller orders behind this stream is behind the last mixer too -- the last one launched when this is called: a
	 * host asks again after every run whose rows it reads on the device, include/saugns_amd.h) */
	void *stream_handle() override { use_device(); join_mixer_quiet("stream_handle"); return (void *)stream_; }
	bool order_after(HipBackend *before, std::string &err) override {
		HipBackendImpl *o = static_cast<HipBackendImpl *>(before);
		if (o == this) return true;
		if (o->dev_ != dev_) { err = "sauAmd_Batch_order_after: the two batches are on different devices"; return false; }
		use_device();
		if (!after_ev_) HIP_OK(hipEventCreateWithFlags(&after_ev_, hipEventDisableTiming));
		/* (everything of `before` ends on its main stream: its chain stream's work is joined there by the final passes, its last
		 * mixer's here) */
		if (!o->join_mixer("order_after", err)) return false;
		HIP_OK(hipEventRecord(after_ev_, o->stream_));
		after_pending_ = true;
		return true;
	}
	/* (render(): ahead of the first kernel that does real work -- after analyze_kernel and decode_kernel) */
	bool wait_for_predecessor(std::string &err) {
		if (!after_pending_) return true;
		after_pending_ = false;
		HIP_OK(hipStreamWaitEvent(stream_, after_ev_, 0));
		return true;
	}
	void set_timing(int level) override { use_device(); join_mixer_quiet("set_timing"); timing_on_ = level > 0; timing_level_ = level; }

	void timing_ex(double *out4, uint64_t *segments, bool reset) override {
		if (!timing_on_) timing_on_ = true;
		use_device();
		join_mixer_quiet("timing");
		(void)hipStreamSynchronize(stream_);
		drain_pairs();
		/* out: time-parallel kernel, block-loop kernel, mixer, analyze+finalize (ms) */
		out4[0] = acc_ms_[2]; out4[1] = acc_ms_[0]; out4[2] = acc_ms_[1]; out4[3] = acc_ms_[3];
		if (segments) *segments = acc_launches_;
		if (reset) { acc_ms_[0] = acc_ms_[1] = acc_ms_[2] = acc_ms_[3] = 0; acc_launches_ = 0; }
	}

	void debug_dump(const char *what, const Job &j) {
		const SegmentDesc &seg = j.seg;
		const uint32_t block_grid = j.block_grid;
		const MixSet &S = sets_[j.set];
		(void)hipStreamSynchronize(stream_);
		uint32_t n = cfg_.op_count < 8 ? cfg_.op_count : 8;
		std::vector<DevOp> h(n);
		(void)hipMemcpy(h.data(), ops_.p, n * sizeof(DevOp), hipMemcpyDeviceToHost);
		fprintf(stderr, "[sau-amd] %s: seg len %u off %u voices %u slots %u\n", what, seg.len,
				seg.pcm_offset, seg.n_voices, seg.n_slots);
		for (uint32_t v = 0; v < seg.n_voices && v < 4; ++v)
			fprintf(stderr, "  voice %u: run_len %u plan %u+%u ops %u+%u\n", v, seg.voices[v].run_len,
					seg.voices[v].plan_ofs, seg.voices[v].plan_len, seg.voices[v].ops_ofs, seg.voices[v].nops);
		{
			uint32_t wc = 0;
			(void)hipMemcpy(&wc, S.work_count.p, 4, hipMemcpyDeviceToHost);
			{ /* voices the time-parallel path did not finish */
				std::vector<FastInfo> all(seg.n_voices);
				(void)hipMemcpy(all.data(), finfo_.p, all.size() * sizeof(FastInfo), hipMemcpyDeviceToHost);
				uint32_t shown = 0;
				for (size_t v = 0; v < all.size() && shown < 16; ++v)
					if (all[v].bail || all[v].total < seg.voices[v].run_len) {
						uint32_t dbg = 0;
						(void)hipMemcpy(&dbg, repair_.p + v * FAST_REPAIR_WORDS + 1, 4, hipMemcpyDeviceToHost);
						fprintf(stderr, "  voice %zu: fast total %u of %u, bail %u, H %u, seq %u; last unresolved hold: lane p_min+%u row %u step %u group %u (mod 4096)\n", v, all[v].total,
								seg.voices[v].run_len, all[v].bail, all[v].H, all[v].seq, dbg >> 24, (dbg >> 20) & 15, (dbg >> 12) & 255, dbg & 0xfff);
						++shown;
					}
			}
			std::vector<VoiceOut> vi(seg.n_voices < 4 ? seg.n_voices : 4);
			std::vector<uint32_t> fd(vi.size());
			std::vector<FastInfo> fi(vi.size());
			(void)hipMemcpy(vi.data(), S.vinfo.p, vi.size() * sizeof(VoiceOut), hipMemcpyDeviceToHost);
			(void)hipMemcpy(fd.data(), fdone_.p, fd.size() * 4, hipMemcpyDeviceToHost);
			(void)hipMemcpy(fi.data(), finfo_.p, fi.size() * sizeof(FastInfo), hipMemcpyDeviceToHost);
			float v8[8] = {0};
			(void)hipMemcpy(v8, sets_[j.block].vout.p, sizeof v8, hipMemcpyDeviceToHost);
			fprintf(stderr, "  work_count %u block_grid %u; row0: %g %g %g %g %g %g\n", wc, block_grid, v8[0], v8[1],
					v8[2], v8[3], v8[4], v8[5]);
			for (size_t v = 0; v < vi.size(); ++v)
				fprintf(stderr, "  vinfo %zu: pan %g has_pan %u valid %u prow %u | fast total %u H %u bail %u done %u\n", v,
						vi[v].pan_const, vi[v].has_pan, vi[v].valid_len, vi[v].pan_row, fi[v].total, fi[v].H,
						fi[v].bail, fd[v]);
		}
		for (uint32_t i = 0; i < n; ++i) {
			const DevOp &o = h[i];
			fprintf(stderr, "  op %u: time %u flags %#x type %u wave %u phase %u prev_s %g fb %g\n", i, o.time,
					o.flags, o.type, o.wave, o.phase, o.prev_s, o.fb_s);
			for (int l = 0; l < 6; ++l)
				if (o.line[l].flags || o.line[l].v0 != 0.f)
					fprintf(stderr, "     line %d: v0 %g vt %g pos %u end %u type %u flags %#x\n", l,
							o.line[l].v0, o.line[l].vt, o.line[l].pos, o.line[l].end, o.line[l].type,
							o.line[l].flags);
		}
	}

private:
	TimedPair *new_pair(int kind) {
		if (timing_level_ == 1 && kind != 2) return nullptr; /* level 1: dominant kernel only */
		if (n_used_ == events_.size()) {
			if (events_.size() >= 4096) { join_mixer_quiet("timing"); (void)hipStreamSynchronize(stream_); drain_pairs(); }
			else {
				TimedPair p; p.kind = 0; p.used = false;
				if (hipEventCreate(&p.a) != hipSuccess || hipEventCreate(&p.b) != hipSuccess) return nullptr;
				events_.push_back(p);
			}
		}
		TimedPair *p = &events_[n_used_++];
		p->kind = kind; p->used = true;
		return p;
	}
	void drain_pairs() {
		for (size_t i = 0; i < n_used_; ++i) {
			float ms = 0;
			if (hipEventElapsedTime(&ms, events_[i].a, events_[i].b) == hipSuccess) {
				acc_ms_[events_[i].kind & 3] += ms;
			}
		}
		n_used_ = 0;
	}

	BackendConfig cfg_;
	hipStream_t stream_ = nullptr;
	Tuning tun_;       /* the tuning switches as the environment had them when the backend was created (launch_plan.h) */
	DeviceLimits lim_; /* ... and what the rules need to know of the device */
	bool debug_ = false;
	bool inner_report_ = false; /* SAU_AMD_INNER_REPORT: which form the closed-form launch took, a line on stderr per such segment (tests) */
	bool inmix_report_ = false; /* SAU_AMD_INMIX_REPORT: what the launch mixed itself, likewise (tests) */
	uint32_t row_stride_ = 0;
	size_t pcm_row_ = 0;   /* samples per stream's row (room for stereo) */
	bool pcm_f32_ = false; /* the rows hold float32 samples: the run at hand, or the last one, is a float run (set_format) */
	WaveConst wconst_[12];
	DevBuf<DevOp> ops_;
	DevBuf<DevOp> ops_snap_[4]; /* save_state() */
	DevBuf<Step> steps_;
	DevBuf<FastIds> fast_ids_; /* [2][n_steps_total_]: without / with frequency blocks */
	uint32_t n_steps_total_ = 0;
	DevBuf<uint32_t> op_ids_;
	DevBuf<VoiceDesc> voices_;
	/* What a mixer reads, but for the PCM: voice rows, pan rows, per-row records, stream records, the guard words, the control
	 * words of a launch that mixes tiles itself, the streams a look-back launch has mixed. Two sets, segment n's launches on set
	 * n mod 2, so that a segment's final mixer can still be reading its set while the next segment's launches fill the other
	 * (launch_mixer). The rows are the one large member: set 1 has a block of its own only while plan_mix_overlap says so
	 * (MIXO_ALTERNATE) and the device gave it; otherwise both sets' segments use set 0's (Job.block). */
	struct MixSet {
		DevBuf<float> vout, pan;
		DevBuf<VoiceOut> vinfo;
		DevBuf<MixStream> mstreams;
		DevBuf<uint32_t> work_count; /* four words: [0] the block loop's work list, [1] premix_kernel's verdict -- the mixers' guard */
		DevBuf<uint32_t> inmix_ctl;
		DevBuf<uint32_t> tail_ok;    /* [stream]: the look-back launch mixes this stream itself (k_fast_types.h: FastParams.tail_ok) */
		uint32_t vout_rows = 0;
		std::vector<MixStream> ms_sent;
		const void *ms_dev = nullptr;
	};
	MixSet sets_[2];
	MixOverlapTracker mixo_;       /* where the main stream waits for a mixer on the side stream (mix_overlap.h) */
	hipStream_t mix_stream_ = nullptr;
	bool mix_ready_ = false;       /* the side stream and every event of the two rings are there */
	hipEvent_t mix_fork_[MIXO_RING] = {}, mix_done_[MIXO_RING] = {}; /* per ticket: recorded on the main stream ahead of the mixer, on the side stream behind it */
	bool second_refused_ = false;  /* the second block of rows was not to be had: shared rows for good */
	bool overlap_report_ = false;  /* SAU_AMD_OVERLAP_REPORT: a line on stderr per segment (tests) */
	std::string report_waits_;
	DevBuf<int16_t> pcm_;
	DevBuf<OpUpdate> recs_;
	const TableSet *tables_ = nullptr;
	PinBuf<int16_t> h_pcm_; /* fetch_pcm() staging */
	PinBuf<unsigned char> arena_; /* stage() */
	size_t arena_used_ = 0;
	std::vector<VoiceDesc> voices_sent_;   /* what the device copies hold */
	std::vector<MixStream> ms_host_;
	const void *voices_dev_ = nullptr;
	std::deque<TimedPair> events_; /* (a deque: pairs handed out stay where they are while more are added) */
	size_t n_used_ = 0;
	bool timing_on_ = false;
	double acc_ms_[4] = {0, 0, 0, 0};
	uint64_t acc_launches_ = 0;
	int timing_level_ = 2;
	DevBuf<FastInfo> finfo_;
	DevBuf<uint32_t> fdone_, worklist_;
	DevBuf<float> big_slots_;     /* block buffers of render_kernel<1, 1, 1, true>: [workgroup][slot][64] */
	DevBuf<unsigned char> fsteps_, flines_, faux_;
	DevBuf<unsigned long long> scan_;
	DevBuf<uint32_t> pass_flags_, repair_;
	hipEvent_t fetch_ev_[4] = {nullptr, nullptr, nullptr, nullptr}; /* per host slot of the drop-in generator's read-ahead */
	int dev_ = 0;
	int want_dev_ = -1; /* the device the creator asked for (-1: SAU_AMD_DEVICE, else 0) */
	std::map<void *, size_t> host_blocks_; /* alloc_host() blocks and their pool sizes */
	DevBuf<unsigned long long> look_;
	uint32_t look_epoch_ = 0;
	DevBuf<uint32_t> inc_rows_;
	hipStream_t chain_stream_ = nullptr;
	std::vector<hipEvent_t> chain_ev_;
	DevBuf<float> chain_rows_;
	bool chain_rows_failed_once_ = false;
	unsigned chain_rows_failures_ = 0; /* allocations of rows that failed on this backend */
	size_t free_hint_ = 0;             /* bytes free on the device when the process first opened it */
	DevBuf<ChainDesc> chain_desc_;
	DevBuf<unsigned char> fplines_;
	hipEvent_t after_ev_ = nullptr; /* order_after() */
	bool after_pending_ = false;
	/* level metering: the streams' running records, one measurement's partial records and frame counts, the records of
	 * foreign rows (measure_rows), and the normalised writer's requantised row -- all from the pool, none there until asked for */
	DevBuf<LevelsAcc> lev_acc_, lev_out_;
	DevBuf<LevelsPart> lev_parts_;
	DevBuf<uint32_t> lev_frames_;
	DevBuf<unsigned char> requant_;
	/* the decimator: the streams' histories, the taps of the sequence at hand, a run's frame counts and its output rows -- all
	 * from the pool, none there until a decimated run asks for them */
	DevBuf<float> decim_hist_;
	DevBuf<double> decim_taps_;
	DevBuf<uint32_t> decim_frames_;
	DevBuf<unsigned char> decim_out_;
	int decim_factor_ = 0;
	bool decim_stereo_ = false, decim_out_f32_ = false;
	/* loudness: the streams' records and those of one measure_loudness_rows call, one measurement's scratch (the chunks' zero-state
	 * results, their start states, their hop sums, the tiles' peaks, the rows' frame counts), the true-peak taps, and the filter
	 * and chunk map of the rate at hand -- all from the pool, none there until asked for */
	LoudSet loud_own_, loud_rows_;
	DevBuf<LoudState> loud_z_, loud_s_;
	DevBuf<double> loud_parts_, loud_taps_;
	DevBuf<uint32_t> loud_tp_parts_, loud_frames_;
	LoudFilter loud_f_;
	LoudMap loud_m_;
	uint32_t loud_rate_ = 0;
	/* the limiter: the streams' histories (two buffers: lim_carry_kernel moves from one into the other), a run's frame counts and
	 * output rows, the streams' statistics, one pass's scratch (s, r, the tiles' records), the window of the rate at hand and the
	 * true-peak taps, and what one limit_rows call needs -- all from the pool, none there until a limited run asks for them */
	DevBuf<float> lim_hist_[2];
	DevBuf<uint32_t> lim_frames_, lim_rows_frames_, lim_part_cnt_;
	DevBuf<unsigned char> lim_out_;
	DevBuf<LimStats> lim_stats_, lim_rows_stats_;
	DevBuf<double> lim_s_, lim_r_, lim_part_min_, lim_win_, lim_taps_;
	int lim_cur_ = 0;
	uint32_t lim_rate_ = 0;
	bool lim_on_ = false, lim_stereo_ = false, lim_out_f32_ = false;
	size_t lim_out_pitch_ = 0, lim_out_bytes_ = 0; /* of the last limited run: between the rows, and of a row's frames */
	DevBuf<float> spec_gram_; /* spectrum_rows: one call's spectrogram, from the pool, not there until asked for */
	size_t decim_out_pitch_ = 0, decim_out_bytes_ = 0; /* of the last decimated run: between the rows, and of a row's frames */
	DevBuf<uint32_t> vlists_;   /* [2][n_voices]: analyze_kernel's lists of closed-form and look-back voices (split launches) */
	/* A chain kernel's workgroup is three waves on a latency-bound recurrence. SAU_AMD_CHAIN_ALONE=1 (a tuning switch): while a
	 * launch has no more workgroups than the device has CUs, each asks for more than half a CU's LDS and so gets a CU of its own.
	 * Measured without effect -- R feedback banks of 8 / 64 / 1024 / 4096 voices 521 571 501 427 ns per frame with it, 486-511
	 * 574-609 484-501 426 without, config 5 45.96-46.06 against 45.77-46.00 ms: the workgroups do not slow each other; what varies
	 * from run to run on a nearly idle device (one voice: 324-418 ns) is not the placement. Off. */
	size_t chain_alone_lds(size_t need, uint32_t grid) const {
		if (!tun_.chain_alone || grid > lim_.cus || need * 2 > lim_.lds_limit) return need;
		const size_t half = lim_.lds_limit / 2 + 1024;
		return need > half ? need : half;
	}
};

HipBackend *create_hip_backend(std::string &err, int device) {
	if (device_count() <= 0) {
		err = "no HIP device available (this backend has no CPU fallback)";
		return nullptr;
	}
	return new HipBackendImpl(device);
}

} /* namespace sauhip */

