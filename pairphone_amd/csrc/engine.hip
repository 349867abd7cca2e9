/*
 * engine.hip -- host side of the MI355X MELPe-1200 engine: the C ABI
 * (include/melpe.h drop-in, include/melpe_batch.h batched), the engine
 * object, stream and event plumbing, staging for the host calls, and device
 * table upload.  Host code only: this file defines no kernel and launches
 * none itself.
 *
 * Every kernel lives in a k_*.hip translation unit next to its kl_*
 * launcher, compiled in parallel (pairphone_amd/build.py) and linked into
 * libmelpe_amd.so:
 *   k_npp.hip    melpe_n, and the NPP half of melpe_a (melpe/melpe.c:94-96)
 *   k_ana.hip    the analysis half of melpe_a (melpe/melpe.c:97-98)
 *   k_dec.hip    melpe_s (melpe/melpe.c:102-107), and the synthesis from
 *                parameter rows
 *   k_state.hip  reset, init, parameter sharing, the test-signal generator
 *                and the lane-order sort
 *   k_line.hip   voice crypt, the VAD, the VAD-framed stream format, the
 *                modem and the receive loop
 * and the rest that kern.h lists; launch.h declares what this file calls in
 * them.
 * Execution model: one lane per channel (kern.h).  Per-channel
 * state lives in HBM (EncState / DecState), the codebooks in the constant
 * tables of each TU whose kernels read them (uploaded once per device).
 */
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include <initializer_list>
#include <string>
#include <mutex>
#include <vector>

#include "kern.h"
#include "synth.h"
#include "voice_crypt.h"
#include "vad.h"
#include "stream_fmt.h"
#include "ops_eval.h"
#include "dsp_eval_modes.h"
#include "ana_eval_modes.h"
#include "modem.h"
#include "rxline.h"
#include "../../include/melpe.h"
#include "../../include/melpe_batch.h"

/* ------------------------------------------------------------------ */
/* embedded constant tables (oracle/dump_tables.py output)            */
/* ------------------------------------------------------------------ */
#if !defined(__HIP_DEVICE_COMPILE__)
__asm__(".section .rodata\n"
	".balign 16\n"
	".global melpe_tables_blob\n"
	"melpe_tables_blob:\n"
	".incbin \"" MELPE_TABLES_BIN "\"\n"
	".global melpe_tables_blob_end\n"
	"melpe_tables_blob_end:\n"
	".previous\n");
#endif
extern "C" const unsigned char melpe_tables_blob[];
extern "C" const unsigned char melpe_tables_blob_end[];

static thread_local std::string g_err;

static int fail(const char *what, hipError_t e)
{
	g_err = std::string(what) + ": " + hipGetErrorString(e);
	return -1;
}

static int fail_msg(const std::string &m)
{
	g_err = m;
	return -2;
}

#define HIPCHK(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) return fail(#expr, _e); } while (0)

/* Every entry point that selects a device restores the caller's current
 * device on return, so a multi-GPU host process (or torch's default device)
 * never sees its current device move under it. */
struct DevGuard {
	int prev = -1;
	hipError_t err = hipSuccess;
	explicit DevGuard(int dev)
	{
		int cur = -1;
		if (hipGetDevice(&cur) == hipSuccess && cur == dev)
			return;
		err = hipSetDevice(dev);
		prev = cur;
	}
	~DevGuard()
	{
		if (prev >= 0)
			hipSetDevice(prev);
	}
};
#define DEVGUARD(dev) DevGuard _dg(dev); HIPCHK(_dg.err)

/* device staging of the engine-less *_host calls (VAD, voice crypt): one
 * buffer per device, grown on demand and kept, instead of a hipMalloc /
 * hipFree pair per call */
struct HostStage {
	std::mutex mu;
	void *p = nullptr;
	size_t n = 0;
};
static HostStage g_stage[64];

static int stage_get(int dev, size_t bytes, void **out)
{
	if (dev < 0 || dev >= 64)
		return fail_msg("bad device index");
	HostStage &h = g_stage[dev];
	if (h.n < bytes) {
		if (h.p)
			HIPCHK(hipFree(h.p));
		h.p = nullptr;
		h.n = 0;
		HIPCHK(hipMalloc(&h.p, bytes));
		h.n = bytes;
	}
	*out = h.p;
	return 0;
}

/* The lane order (MELPE_BIN, default on): k_state.hip has the sort and what
 * its classes are, launch.h the buffers of one order (BinBuf); here, their
 * host bookkeeping. */

/* what a kernel is launched with: b's order and live count when the order is
 * used, nulls (identity lanes + mask) when it is not */
struct LaneOrder {
	const int *perm, *nlive;
};
static LaneOrder bin_order(const BinBuf &b, bool on)
{
	return {on ? b.perm : nullptr, on ? (const int *) (b.ctl + 2 * NBIN) : nullptr};
}

static hipError_t bin_alloc(BinBuf *b, int channels)
{
	size_t pb = sizeof(int) * (size_t) channels, cb = sizeof(unsigned) * (2 * NBIN + 4);
	const size_t kb = sizeof(uint16_t) * (size_t) channels;
	char *p = nullptr;
	hipError_t er = hipMalloc(&p, pb + cb + kb);
	if (er != hipSuccess)
		return er;
	er = hipEventCreateWithFlags(&b->done, hipEventDisableTiming);
	if (er != hipSuccess) {
		hipFree(p);
		return er;
	}
	b->perm = (int *) p;
	b->ctl = (unsigned *) (p + pb);
	b->key = (uint16_t *) (p + pb + cb);
	return hipMemset(b->ctl, 0, cb);
}

static bool bin_enabled(void)
{
	static const bool on = env_int("MELPE_BIN", 1) != 0;
	return on;
}

/* the part of a sort that depends on no record: s waits for the kernel that
 * read b's previous order when that ran on another stream, then the class
 * counters are zeroed.  bin_launch does it itself unless told that the
 * caller already has (ana_launch, for the second order: the zeroing is a
 * dispatch of its own, and issued only after k_enc_ana it queued 2 ms behind
 * the resident NPP and analysis waves, profiles/r07_new_kernel_stats.txt). */
static hipError_t bin_prepare(BinBuf &b, hipStream_t s)
{
	hipError_t er;
	if (b.used && b.last != s && (er = hipStreamWaitEvent(s, b.done, 0)) != hipSuccess)
		return er;
	return hipMemsetAsync(b.ctl, 0, sizeof(unsigned) * NBIN, s);
}

/* sorts the live channels of `rec` (records of `stride` bytes) into b.perm on
 * stream s by the class `key` gives them; *on: whether the order is used
 * (false: identity lanes + mask) */
static hipError_t bin_launch(int order, BinBuf &b, const void *rec, size_t stride, int off_par,
			     int off_uv, const uint8_t *active, int n, hipStream_t s, bool *on,
			     int key = KEY_PITCH, bool prepared = false)
{
	*on = !(order == 0 || (order < 0 && !bin_enabled()));
	if (!*on)
		return hipSuccess;
	hipError_t er;
	if (!prepared && (er = bin_prepare(b, s)) != hipSuccess)
		return er;
	return (hipError_t) kl_bin_sort(key, (const char *) rec, stride, off_par, off_uv, active, n, b, s);
}

/* after the kernel that reads b's order, on the same stream */
static hipError_t bin_release(BinBuf &b, hipStream_t s)
{
	b.last = s;
	b.used = true;
	return hipEventRecord(b.done, s);
}

/* k_enc_ana_mw holds two workgroups (of 4 waves, 64 channels) per CU, so it
 * keeps every workgroup resident up to 512 of them */
#define MW_MAX_CHANNELS (512 * WAVE)
/* the two-wave decoder (k_decode2) by default up to this many channels per
 * engine: 2,048 waves (two per SIMD) at 65,536 channels, where the lane
 * decoder has one wave per SIMD */
#define DEC2_MAX_CHANNELS (1024 * WAVE)

struct melpe_engine {
	int device = 0;
	int channels = 0;
	hipStream_t stream = nullptr;	/* the device's engine stream (g_dev_stream), shared */
	hipEvent_t ev0 = nullptr, ev1 = nullptr;
	hipEvent_t ev_in = nullptr, ev_out = nullptr;	/* engine_call's hops to and from the engine stream */
	hipEvent_t ev_host = nullptr;	/* host_finish: the end of a host call's own work */
	hipEvent_t ev_pin = nullptr, ev_npp = nullptr;	/* pipe_step's hops to / from cin */
	EncState *d_enc = nullptr;
	DecState *d_dec = nullptr;
	synth_state *d_syn = nullptr;
	int16_t *d_pcm = nullptr;	/* staging for *_host calls */
	unsigned char *d_bits = nullptr;
	uint8_t *d_mask = nullptr;
	uint8_t *d_rxmask = nullptr;	/* melpe_rx_line_dev: the decoder's mask of the slot in hand */
	int16_t *d_npp = nullptr;	/* staging of melpe_npp_host, grown on demand */
	BinBuf bin_enc, bin_dec;	/* pitch-class lane order of k_enc_ana / k_decode */
	BinBuf bin_enc2;	/* voicing-pattern lane order of k_enc_quant / k_enc_harm / k_enc_tail */
	int lane_order = -1;	/* 1 on, 0 off, -1 the MELPE_BIN default */
	int ana_waves = 0;	/* waves per 64 channels in k_enc_ana(_mw); 0: by channel count */
	uint32_t *d_lq = nullptr;	/* k_enc_ana_mw's lsf_vq score rows (engine_reserve) */
	int dec_waves = 0;	/* waves per 64 channels of the decoder; 0: by channel count */
	uint32_t *d_hb = nullptr;	/* k_decode2's hand-over buffers (engine_reserve) */
	/* the live-count mapping (ana_launch): a superframe with at most this
	 * many live channels runs the multi-wave kernel (0: off) */
	int mw_live_max = MW_MAX_CHANNELS;
	size_t scratch_need = 0;	/* bytes of scratch the largest launch takes */
	int16_t *d_res = nullptr;	/* the split lane analysis' windowed residuals (C x NF x LPC_FRAME) */
	/* one event per stream this engine's *_dev calls have used, recorded
	 * after each call: the host-side calls wait on these (engine_wait)
	 * instead of the whole device */
	std::vector<std::pair<hipStream_t, hipEvent_t>> marks;
	std::recursive_mutex mu;	/* guards marks and the BinBuf bookkeeping */
	size_t npp_bytes = 0;
	float last_ms = 0.f;
	/* the host-fed pipeline (melpe_encode_host_async): two device slots;
	 * call k uses slot k & 1 -- its H2D on `cin`, its kernels on the
	 * engine stream, its D2H on `cout`, so superframe k's kernels overlap
	 * the copies of k - 1 and k + 1 */
	struct Slot {
		int16_t *pcm = nullptr;
		unsigned char *bits = nullptr;
		uint8_t *mask = nullptr;
		hipEvent_t loaded = nullptr, done = nullptr, freed = nullptr;
		bool used = false;
	} slot[2];
	hipStream_t cin = nullptr, cout = nullptr;
	/* pipe_step's decoder stream and its hop back */
	hipStream_t cdec = nullptr;
	hipEvent_t ev_dec = nullptr;
	long async_calls = 0;
	hipStream_t own = nullptr;	/* melpe_engine_set_own_stream */
};

/*
 * Waves per 64 channels of the analysis kernel.  Lane-per-channel (1) needs
 * about four waves per SIMD to hide its scratch latency; below that the
 * channel count leaves SIMDs idle or alone, and the multi-wave kernel
 * (k_enc_ana_mw, ana_mw.h) spreads each channel's independent chains over
 * 4 waves instead.  melpe_engine_set_ana_waves(1 or 4) overrides the
 * automatic choice.
 */
static int ana_waves_for(melpe_engine *e)
{
	if (e->ana_waves == 1 || e->ana_waves == 4)
		return e->ana_waves;
	/* k_enc_ana_mw holds two workgroups (of 4 waves) per CU, so it keeps
	 * every workgroup resident up to 512 of them: 32,768 channels */
	long groups = (e->channels + WAVE - 1) / WAVE;
	return groups <= 512 ? 4 : 1;
}

/* after_sort: recorded on s between the lane-order sort and the analysis
 * kernels (melpe_encode_pipe_dev starts the next superframe's NPP there, so
 * that the analysis' waves are dispatched first and the NPP's fill the
 * slots they free) */
static int ana_launch(melpe_engine *e, const int16_t *d_sp, uint8_t *d_bits, const uint8_t *d_act,
		      hipStream_t s, hipEvent_t after_sort = nullptr)
{
	BinBuf &b = e->bin_enc;
	bool on;
	hipError_t er = bin_launch(e->lane_order, b, e->d_enc, sizeof(EncState),
				   (int) (offsetof(EncState, a) + offsetof(EncAna, par)),
				   (int) (offsetof(EncState, a) + offsetof(EncAna, qpar) + offsetof(QuantParam, uv_flag)),
				   d_act, e->channels, s, &on);
	if (er != hipSuccess)
		return (int) er;
	LaneOrder o = bin_order(b, on);
	int nw = ana_waves_for(e);
	AnaGate all;
	all.tag = (int *) (b.ctl + 2 * NBIN + 1);
	/* Above MW_MAX_CHANNELS the engine runs the lane kernels -- unless few
	 * channels are live (ragged streams, BASELINE config 5).  The live count
	 * is on the device (the lane-order sort counted it), so the choice is
	 * made there: both mappings are enqueued, each gated on the count, and
	 * the one whose range holds it runs (the other's waves leave at once).
	 * No host readback, so host run-ahead cannot make the choice stale.
	 * Either mapping gives the same bits (the four-wave kernel grid-strides
	 * over every live slot). */
	bool dual = nw == 1 && on && e->ana_waves == 0 && e->mw_live_max > 0;
	/* An engine small enough for the four-wave kernel alone takes the same
	 * dual path once the caller has set the live count at which the lane
	 * kernels take over below its channel count
	 * (melpe_engine_set_mw_live_max; the default, MW_MAX_CHANNELS, never
	 * is). */
	if (nw == 4 && on && e->ana_waves == 0 && e->mw_live_max > 0 && e->mw_live_max < e->channels) {
		dual = true;
		nw = 1;
	}
	/* the second order's counters are zeroed here, beside the first sort
	 * and ahead of after_sort, while the GPU is not yet full of the next
	 * superframe's NPP */
	BinBuf &b2 = e->bin_enc2;
	if (on && nw == 1 && (er = bin_prepare(b2, s)) != hipSuccess)
		return (int) er;
	if (after_sort && (er = hipEventRecord(after_sort, s)) != hipSuccess)
		return (int) er;
	AnaGate lane = all, mw = all;
	if (dual) {
		lane.lo = e->mw_live_max;
		mw.hi = e->mw_live_max;
	}
	int rc = 0;
	if (dual || nw == 4)
		rc = kl_enc_ana_mw(e->d_enc, d_sp, d_bits, d_act, e->channels, o.perm, o.nlive, e->d_lq, mw, s);
	if (rc == 0 && nw == 1) {
		/* lane-per-channel analysis up to sc_ana (k_ana.hip), the
		 * quantisers (k_quant.hip), the Fourier magnitudes with a wave per
		 * channel, then the packing (k_harm.hip) */
		rc = kl_enc_ana(e->d_enc, d_sp, d_act, e->channels, o.perm, o.nlive, e->d_res, lane, s);
		/* The second lane order.  What follows sc_ana branches on the
		 * superframe's voicing pattern (lsf_vq's codebooks and searches,
		 * quant_fsmag, the residual loop), which the first order cannot
		 * know: it sorts by the previous superframe, and this one's
		 * pattern exists only once k_enc_ana has written par[].uv_flag.
		 * So the live channels are sorted again here, by that pattern, and
		 * the three kernels below run on this order.  The live count is
		 * the first sort's (same mask), so the gate decides alike; when
		 * the four-wave kernel ran, the sort is wasted and they stand
		 * down. */
		if (rc == 0 && on) {
			bool on2;
			rc = (int) bin_launch(1, b2, e->d_enc, sizeof(EncState),
					      (int) (offsetof(EncState, a) + offsetof(EncAna, par)), 0, d_act,
					      e->channels, s, &on2, KEY_VOICING, true);
			o = bin_order(b2, true);
		}
		if (rc == 0)
			rc = kl_enc_quant(e->d_enc, e->d_res, d_act, e->channels, o.perm, o.nlive, lane, s);
		if (rc == 0)
			rc = kl_enc_harm(e->d_enc, e->d_res, d_act, e->channels, o.perm, o.nlive, lane, s);
		if (rc == 0)
			rc = kl_enc_tail(e->d_enc, d_bits, d_act, e->channels, o.perm, o.nlive, lane, s);
		if (rc == 0 && on)
			rc = (int) bin_release(b2, s);
	}
	if (rc == 0 && on)
		rc = (int) bin_release(b, s);
	return rc;
}

/* Waves per 64 channels of the decoder: 1 = one lane per channel
 * (k_decode); 2 = the two-wave decoder (k_decode2), for channel counts that
 * leave SIMDs idle in lane mode.  melpe_engine_set_dec_waves(1 or 2)
 * overrides the automatic choice. */
static int dec_waves_for(melpe_engine *e)
{
	int nw = e->dec_waves;
	if (nw != 1 && nw != 2)
		nw = e->channels <= DEC2_MAX_CHANNELS ? 2 : 1;
	return nw == 2 && e->d_hb ? 2 : 1;
}

/* One superframe of the decoder family (k_dec.hip) from either source: the
 * lane order in the decoder's BinBuf, the mapping choice and the hand-over
 * buffers are the same for both.  The sort key follows the source: the
 * channel words decode in the order of the records' previous superframe
 * (KEY_PITCH), the parameter rows in the order of the rows themselves
 * (KEY_ROWS: the tensor is the "record", one row of 180 bytes per channel). */
static int dec_launch(melpe_engine *e, int16_t *d_sp, DecSrc src, const uint8_t *d_act, hipStream_t s)
{
	BinBuf &b = e->bin_dec;
	bool on;
	hipError_t er = src.rows ? bin_launch(e->lane_order, b, src.in, sizeof(MelpParam) * NF, 0, 0, d_act,
					      e->channels, s, &on, KEY_ROWS)
				 : bin_launch(e->lane_order, b, e->d_dec, sizeof(DecState),
					      (int) offsetof(DecState, par),
					      (int) (offsetof(DecState, qpar) + offsetof(QuantParam, uv_flag)),
					      d_act, e->channels, s, &on);
	if (er != hipSuccess)
		return (int) er;
	const LaneOrder o = bin_order(b, on);
	int rc = kl_dec(dec_waves_for(e), src, e->d_dec, d_sp, d_act, e->channels, o.perm, o.nlive, e->d_hb, s);
	if (rc == 0 && on)
		rc = (int) bin_release(b, s);
	return rc;
}

/* the two sources (launch.h DecSrc) */
static DecSrc src_bits(const void *d_bits)
{
	return {0, d_bits, nullptr};
}
static DecSrc src_rows(const void *d_par, uint8_t *d_status)
{
	return {1, d_par, d_status};
}

static std::mutex g_dev_mu;
static bool g_dev_ready[64];
/* One stream per device for every engine's own work (create's warm-ups and
 * the host-buffer calls).  The runtime holds kernel scratch per hardware
 * queue and keeps it between dispatches; engines each on a stream of their
 * own end up on every hardware queue the process has, each holding the
 * scratch of the largest codec launch it ran, and together they can exhaust
 * the device's scratch pool (a later launch then aborts its queue with
 * HSA_STATUS_ERROR_OUT_OF_RESOURCES).  Sharing one stream keeps that to one
 * queue plus the callers' own streams. */
static hipStream_t g_dev_stream[64];

static int ensure_device_tables(int dev)
{
	std::lock_guard<std::mutex> lk(g_dev_mu);
	if (dev < 0 || dev >= 64)
		return fail_msg("bad device index");
	if (g_dev_ready[dev])
		return 0;
	size_t bytes = (size_t) (melpe_tables_blob_end - melpe_tables_blob);
	if (bytes != sizeof(int16_t) * MELPE_TABLE_WORDS)
		return fail_msg("embedded table blob has the wrong size");
	DEVGUARD(dev);
#define TU_UPLOAD(name) melpe_tu_##name##_upload,
	int (*up[])(const void *, size_t) = {MELPE_TU_LIST(TU_UPLOAD)};
#undef TU_UPLOAD
	for (auto f : up)
		if (int rc = f(melpe_tables_blob, bytes))
			return fail("table upload", (hipError_t) rc);
	if (hipError_t er = hipStreamCreateWithFlags(&g_dev_stream[dev], hipStreamNonBlocking))
		return fail("engine stream", er);

	g_dev_ready[dev] = true;
	return 0;
}

/* what melpe_last_kernel_ms reports of a call: nothing (the previous timed
 * call stands), resolved lazily when it is asked for, or waited for here */
enum Timing { TIME_NONE, TIME_LAZY, TIME_SYNC };

/* runs `launches` (which enqueue on s) between the engine's two timing
 * events; a failed launch leaves the previous timing */
template <class F> static int timed(melpe_engine *e, hipStream_t s, Timing t, F &&launches)
{
	if (t == TIME_NONE)
		return launches();
	hipEventRecord(e->ev0, s);
	if (int rc = launches())
		return rc;
	hipEventRecord(e->ev1, s);
	if (t == TIME_SYNC) {
		hipEventSynchronize(e->ev1);
		hipEventElapsedTime(&e->last_ms, e->ev0, e->ev1);
	} else {
		e->last_ms = -1.f;	/* resolved lazily in melpe_last_kernel_ms */
	}
	return 0;
}

/* after enqueueing this engine's work on stream s (engine_call records it on
 * every exit of a call, error paths included, so a later host-side wait also
 * covers the work a failed call left in flight).  A stream's event is
 * reused; at most MAX_MARKS streams
 * are tracked, beyond that the oldest mark is waited for and recycled. */
#define MAX_MARKS 16
static int engine_mark(melpe_engine *e, hipStream_t s)
{
	for (auto &m : e->marks)
		if (m.first == s) {
			HIPCHK(hipEventRecord(m.second, s));
			return 0;
		}
	if (e->marks.size() >= MAX_MARKS) {
		auto m = e->marks.front();
		e->marks.erase(e->marks.begin());
		HIPCHK(hipEventSynchronize(m.second));
		HIPCHK(hipEventDestroy(m.second));
	}
	hipEvent_t ev;
	HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
	e->marks.emplace_back(s, ev);
	HIPCHK(hipEventRecord(ev, s));
	return 0;
}

/* the host waits for every call of this engine already enqueued, on any
 * stream (not for other engines or unrelated work on the device).  The
 * engines' shared stream needs no wait of its own: every call that enqueues
 * on it synchronises it before returning. */
static int engine_wait(melpe_engine *e)
{
	std::lock_guard<std::recursive_mutex> lk(e->mu);
	for (auto &m : e->marks)
		HIPCHK(hipEventSynchronize(m.second));
	return 0;
}
#define ENGINE_WAIT(e) do { if (int _r = engine_wait(e)) return _r; } while (0)
/* a host-side call (the *_host calls, reset, export / import, synth_seed)
 * holds the engine's lock for its whole body: it stages data through the
 * engine's shared buffers (d_mask, d_pcm, d_bits, d_npp), which another
 * thread's call on the same engine would otherwise overwrite or reallocate
 * under it.  (The lock is recursive: ENGINE_WAIT and engine_call take it
 * again inside.) */
#define HOST_LOCK(e) std::lock_guard<std::recursive_mutex> _host_lk((e)->mu)
/* the host waits for the work this call enqueued on the engine stream (an
 * event recorded after it), not for work other engines enqueue later */
static int host_finish(melpe_engine *e)
{
	HIPCHK(hipEventRecord(e->ev_host, e->stream));
	HIPCHK(hipEventSynchronize(e->ev_host));
	return 0;
}
#define HOST_FINISH(e) do { if (int _r = host_finish(e)) return _r; } while (0)
/*
 * One *_dev call of an engine on the caller's stream `user`.  It holds the
 * engine's lock (the host-side bookkeeping -- marks, the lane-order buffers
 * -- is shared by the calls of every thread), runs `launches(s)` with the
 * stream to enqueue on, timed as `t` asks, and records the caller's stream's
 * mark on every exit, error exits included.
 *
 * The call's kernels run on the device's engine stream, ordered after the
 * caller's stream and before its later work (two event hops).  The runtime
 * holds kernel scratch per hardware queue; the codec kernels' is reserved on
 * the engine stream's queue at create (engine_reserve), and a second queue
 * running them would hold its own -- at 14 GB per queue for the analysis
 * kernels two queues exceed the runtime's threshold and it reclaims one
 * queue's scratch to grant the other's, hundreds of ms per launch.
 *
 * An entry point returns this call's result, so a failed hop back (the
 * caller's later work would not be ordered after the kernels) is reported;
 * after failed launches the hop and the mark are made all the same, and the
 * launches' error stands.
 */
template <class F> static int engine_call(melpe_engine *e, hipStream_t user, Timing t, F &&launches)
{
	DEVGUARD(e->device);
	std::lock_guard<std::recursive_mutex> lk(e->mu);
	hipStream_t run = user;
	if (user != e->stream && hipEventRecord(e->ev_in, user) == hipSuccess &&
	    hipStreamWaitEvent(e->stream, e->ev_in, 0) == hipSuccess)
		run = e->stream;
	const int rc = timed(e, run, t, [&] { return launches(run); });
	std::string err;
	if (rc)
		err = g_err;
	hipError_t hop = hipSuccess;
	if (run != user && (hop = hipEventRecord(e->ev_out, run)) == hipSuccess)
		hop = hipStreamWaitEvent(user, e->ev_out, 0);
	const int mark = engine_mark(e, user);
	if (rc) {
		g_err = err;
		return rc;
	}
	if (hop != hipSuccess)
		return fail("the hop from the engine stream back to the caller's", hop);
	return mark;
}

static const uint8_t *stage_mask(melpe_engine *e, const uint8_t *mask_host, int *rc)
{
	*rc = 0;
	if (!mask_host)
		return nullptr;
	hipError_t er = hipMemcpyAsync(e->d_mask, mask_host, (size_t) e->channels,
				       hipMemcpyHostToDevice, e->stream);
	if (er != hipSuccess)
		*rc = fail("hipMemcpyAsync(mask)", er);
	return e->d_mask;
}

/* one buffer of a *_host call and its device staging.  XFER_IN_MASKED: up
 * only when the call has a mask, so that inactive channels keep the caller's
 * data when the buffer comes back down.  A null host pointer: no transfer. */
enum { XFER_IN = 1, XFER_IN_MASKED = 2, XFER_OUT = 4 };
struct Xfer {
	const void *host;
	void *dev;
	size_t bytes;
	int dir;
};

/* The engine's staged host call: under the engine's lock and after every
 * call of the engine already enqueued, the mask and the uploads, then
 * `launches(mask, s)` as one synchronously timed engine_call, the
 * downloads, and the wait -- all on the engine stream, in list order. */
template <class F>
static int engine_host_call(melpe_engine *e, const uint8_t *active, std::initializer_list<Xfer> xs, F &&launches)
{
	DEVGUARD(e->device);
	HOST_LOCK(e);
	ENGINE_WAIT(e);
	int rc;
	const uint8_t *m = stage_mask(e, active, &rc);
	if (rc)
		return rc;
	for (const Xfer &x : xs)
		if (x.host && ((x.dir & XFER_IN) || ((x.dir & XFER_IN_MASKED) && active)))
			HIPCHK(hipMemcpyAsync(x.dev, x.host, x.bytes, hipMemcpyHostToDevice, e->stream));
	if ((rc = engine_call(e, e->stream, TIME_SYNC, [&](hipStream_t s) { return launches(m, s); })))
		return rc;
	for (const Xfer &x : xs)
		if (x.host && (x.dir & XFER_OUT))
			HIPCHK(hipMemcpyAsync((void *) x.host, x.dev, x.bytes, hipMemcpyDeviceToHost, e->stream));
	return host_finish(e);
}

/* The engine-less staged host call (VAD, voice crypt, link): under the
 * current device's stage mutex, xs[i].dev is carved from the device's stage
 * buffer (each part rounded up to 4 bytes; null where the host pointer is),
 * then the uploads, `dev_call()` on the null stream, and the downloads, with
 * synchronous copies. */
template <class F> static int stage_host_call(const char *who, Xfer *xs, int n, F &&dev_call)
{
	size_t total = 0;
	for (int i = 0; i < n; i++)
		total += (xs[i].bytes + 3) & ~(size_t) 3;
	int dev = 0;
	HIPCHK(hipGetDevice(&dev));
	std::lock_guard<std::mutex> lk(g_stage[dev & 63].mu);
	char *d = nullptr;
	if (int r = stage_get(dev, total, (void **) &d))
		return r;
	for (int i = 0; i < n; i++) {
		xs[i].dev = xs[i].host ? d : nullptr;
		d += (xs[i].bytes + 3) & ~(size_t) 3;
	}
	hipError_t he;
	for (int i = 0; i < n; i++)
		if (xs[i].dev && (xs[i].dir & XFER_IN) &&
		    (he = hipMemcpy(xs[i].dev, xs[i].host, xs[i].bytes, hipMemcpyHostToDevice)) != hipSuccess)
			return fail((std::string(who) + ": upload").c_str(), he);
	if (int rc = dev_call())
		return rc;
	for (int i = 0; i < n; i++)
		if (xs[i].dev && (xs[i].dir & XFER_OUT) &&
		    (he = hipMemcpy((void *) xs[i].host, xs[i].dev, xs[i].bytes, hipMemcpyDeviceToHost)) != hipSuccess)
			return fail((std::string(who) + ": download").c_str(), he);
	return 0;
}

/* the VAD, modem and link state records hold 32-bit words */
static int state_aligned(const char *who, const void *d_state)
{
	if ((uintptr_t) d_state & 3)
		return fail_msg(std::string(who) + ": state must be 4-byte aligned");
	return 0;
}

static int vad_launch(void *d_state, const void *d_sp, void *d_votes, void *d_gate, const void *d_active,
		      int channels, hipStream_t s)
{
	if (int rc = kl_vad((VadState *) d_state, (const int16_t *) d_sp, (uint8_t *) d_votes, (uint8_t *) d_gate,
			    (const uint8_t *) d_active, channels, s))
		return fail("vad_launch", (hipError_t) rc);
	return 0;
}

/*
 * The engine's side streams, made at the first call that needs them: cout
 * and cin (the host-fed pipeline's copies; the pipelined calls' NPP and VAD
 * run on cin) and, with `dec`, cdec (melpe_duplex_pipe_dev's decode) and its
 * event.  The runtime spreads streams over the process's hardware queues in
 * the order they are made, so they are made in one place: cout, cin, then
 * cdec.  Each queue's scratch is reserved here as engine_warm does on the
 * engine stream's: the NPP kernel's on cin (only that kernel and the VAD run
 * there besides copies), the decoder kernels' on cdec.
 *
 * All of it under the engine's lock, into locals: the engine's fields are
 * assigned only once every warm-up has run and been waited for, so no call
 * of another thread ever sees a stream whose queue has no scratch yet, and a
 * failure leaves the engine as it was.
 */
static int engine_streams(melpe_engine *e, bool dec)
{
	std::lock_guard<std::recursive_mutex> lk(e->mu);
	const bool side = !e->cin;
	dec = dec && !e->cdec;
	if (!side && !dec)
		return 0;
	DEVGUARD(e->device);
	hipStream_t cout = nullptr, cin = nullptr, cdec = nullptr;
	hipEvent_t ev_dec = nullptr;
	hipError_t er = hipSuccess;
	const char *what = nullptr;
#define STREAM_STEP(expr) if (er == hipSuccess && (er = (hipError_t) (expr)) != hipSuccess) what = #expr
	if (side) {
		STREAM_STEP(hipStreamCreateWithFlags(&cout, hipStreamNonBlocking));
		STREAM_STEP(hipStreamCreateWithFlags(&cin, hipStreamNonBlocking));
		STREAM_STEP(kl_npp_warm(e->channels, cin));
		STREAM_STEP(hipStreamSynchronize(cin));
	}
	if (dec) {
		STREAM_STEP(hipEventCreateWithFlags(&ev_dec, hipEventDisableTiming));
		STREAM_STEP(hipStreamCreateWithFlags(&cdec, hipStreamNonBlocking));
		STREAM_STEP(kl_dec_warm(1, 0, e->channels, cdec));
		if (e->d_hb)
			STREAM_STEP(kl_dec_warm(2, 0, e->channels, cdec));
		STREAM_STEP(hipStreamSynchronize(cdec));
	}
#undef STREAM_STEP
	if (er != hipSuccess) {
		for (hipStream_t s : {cout, cin, cdec})
			if (s)
				hipStreamDestroy(s);
		if (ev_dec)
			hipEventDestroy(ev_dec);
		return fail(what, er);
	}
	if (side) {
		e->cout = cout;
		e->cin = cin;
	}
	if (dec) {
		e->ev_dec = ev_dec;
		e->cdec = cdec;
	}
	return 0;
}

/*
 * The pipelined step behind melpe_encode_pipe_dev, melpe_duplex_pipe_dev and
 * melpe_tx_pipe_dev, on three queues: this superframe's analysis on the
 * engine stream, and once its lane-order sort is done (ev_pin: after the
 * caller's work too, which the engine stream waited for, and so that the
 * analysis' waves, the longest, are dispatched first and the others fill the
 * slots they free) the decode on cdec and the next superframe's VAD and NPP
 * on cin.  The NPP touches only the records' NppState and the next PCM, the
 * analysis only their EncAna and this PCM, the VAD its own state; the
 * encoder and decoder halves of a record and their lane-order buffers
 * (bin_enc and bin_enc2, bin_dec) are disjoint.  The hop back to the caller covers all
 * three; melpe_last_kernel_ms reports the analysis.
 */
struct PipeNext {	/* the next superframe, or none */
	void *sp;
	const void *mask;	/* the NPP's mask: with a VAD the gate it writes */
	void *vad, *votes;	/* the VAD to run first (or null): its state and votes */
	const void *active;	/* the VAD's mask */
};
struct PipeDec {	/* a decode, or none */
	void *sp;
	const void *bits, *active;
};

static int pipe_step(melpe_engine *e, void *d_bits, const void *d_sp, const void *d_active, const PipeNext *nx,
		     const PipeDec *dc, hipStream_t user)
{
	if (nx || dc)
		if (int rc = engine_streams(e, dc != nullptr))
			return rc;
	return engine_call(e, user, TIME_NONE, [&](hipStream_t s) {
		const int rc = timed(e, s, TIME_LAZY, [&] {
			HIPCHK((hipError_t) ana_launch(e, (const int16_t *) d_sp, (uint8_t *) d_bits,
						       (const uint8_t *) d_active, s, (nx || dc) ? e->ev_pin : nullptr));
			return 0;
		});
		if (rc)
			return rc;
		if (dc) {
			HIPCHK(hipStreamWaitEvent(e->cdec, e->ev_pin, 0));
			HIPCHK((hipError_t) dec_launch(e, (int16_t *) dc->sp, src_bits(dc->bits),
						       (const uint8_t *) dc->active, e->cdec));
			HIPCHK(hipEventRecord(e->ev_dec, e->cdec));
		}
		if (nx) {
			HIPCHK(hipStreamWaitEvent(e->cin, e->ev_pin, 0));
			if (nx->vad)
				if (int r = vad_launch(nx->vad, nx->sp, nx->votes, (void *) nx->mask, nx->active,
						       e->channels, e->cin))
					return r;
			HIPCHK((hipError_t) kl_enc_npp(e->d_enc, (int16_t *) nx->sp, (const uint8_t *) nx->mask,
						       e->channels, e->cin));
			HIPCHK(hipEventRecord(e->ev_npp, e->cin));
			HIPCHK(hipStreamWaitEvent(s, e->ev_npp, 0));
		}
		if (dc)
			HIPCHK(hipStreamWaitEvent(s, e->ev_dec, 0));
		return 0;
	});
}

extern "C" {

const char *melpe_last_error(void)
{
	return g_err.c_str();
}

/*
 * What the engine's launches need beyond its records, had at create so a
 * shortage fails here and not mid-stream:
 * - the analysis hand-over buffers (the split lane analysis' residuals; the
 *   multi-wave kernel's score rows up to its 512 resident workgroups);
 * - the private-segment scratch of every codec kernel (the lane kernels
 *   hold ~27 KB per lane): the runtime sizes a queue's scratch by the
 *   dispatches it sees, so each kernel is dispatched once on the engine's
 *   stream with the grid of a real launch over the engine's channels and
 *   no live channel (every lane exits at once), and waited for.  (Scratch
 *   is held per hardware queue: a caller's own stream may map to another
 *   queue, whose first dispatch reserves it again.)
 * engine_warm is the second half, engine_reserve the first and then both.
 */
static int engine_warm(melpe_engine *e)
{
	hipError_t er;
	const int mw = e->channels < MW_MAX_CHANNELS ? e->channels : MW_MAX_CHANNELS;
	int (*warm[])(int, hipStream_t) = {kl_npp_warm, kl_ana_warm, kl_quant_warm, kl_harm_warm, kl_ana_mw_warm};
	for (auto f : warm)
		if ((er = (hipError_t) f(f == kl_ana_mw_warm ? mw : e->channels, e->stream)) != hipSuccess)
			return fail("melpe_engine: codec kernel scratch could not be reserved", er);
	/* the decoder family, each mapping the engine has: the channel words'
	 * kernel always; the parameter rows' runs the same call tree less the
	 * channel read, and is warmed only if its frame should come out larger */
	for (int waves = 1; waves <= (e->d_hb ? 2 : 1); waves++)
		for (int rows = 0; rows < 2; rows++)
			if ((!rows || kl_dec_private(waves, 1) > kl_dec_private(waves, 0)) &&
			    (er = (hipError_t) kl_dec_warm(waves, rows, e->channels, e->stream)) != hipSuccess)
				return fail("melpe_engine: codec kernel scratch could not be reserved", er);
	if ((er = hipStreamSynchronize(e->stream)) != hipSuccess)
		return fail("melpe_engine: codec kernel scratch could not be reserved", er);
	return 0;
}

static int engine_reserve(melpe_engine *e)
{
	DEVGUARD(e->device);
	hipError_t er;
	if ((er = hipMalloc(&e->d_res, sizeof(int16_t) * NF * LPC_FRAME * (size_t) e->channels)) != hipSuccess) {
		e->d_res = nullptr;
		return fail("melpe_engine_create: analysis residual buffer", er);
	}
	if ((er = hipMalloc(&e->d_lq, sizeof(uint32_t) * kl_enc_ana_mw_lq_words(e->channels))) != hipSuccess) {
		e->d_lq = nullptr;
		return fail("melpe_engine_create: multi-wave score rows", er);
	}
	/* (one size whichever the source: k_decode2 and k_synth_par2 share the buffers) */
	if (e->channels <= DEC2_MAX_CHANNELS &&
	    (er = hipMalloc(&e->d_hb, sizeof(uint32_t) * kl_dec2_hb_words(e->channels))) != hipSuccess) {
		e->d_hb = nullptr;
		return fail("melpe_engine_create: two-wave decoder hand-over buffers", er);
	}
	const int mw = e->channels < MW_MAX_CHANNELS ? e->channels : MW_MAX_CHANNELS;
	/* The runtime keeps a queue's scratch between dispatches only below its
	 * scratch limit threshold; above it the allocation is made for the
	 * dispatch and given back.  Raise the threshold (never lower it) to
	 * what this engine's largest launch needs: private bytes per lane x 64
	 * lanes x the waves of the launch that can be resident at once (lane
	 * kernels: one per 64 channels; the four-wave kernel: 4 per group, at
	 * most 512 groups; the wave-per-channel kernels k_enc_npp / k_npp and
	 * k_enc_harm: one per channel, up to the device's resident waves). */
	{
		size_t lane = kl_ana_private() > kl_harm_private() ? kl_ana_private() : kl_harm_private();
		if (kl_quant_private() > lane)
			lane = kl_quant_private();
		/* (k_parse's frame, the record's excitation side, is far below
		 * the decoder's: it never sets the maximum and needs no warm-up) */
		size_t dec_lane = kl_dec_private(1, 0) > kl_parse_private() ? kl_dec_private(1, 0) : kl_parse_private();
		/* (nor does the receive loop's, the demodulator's window plus a
		 * link record: melpe_rx_line_private_bytes) */
		if (kl_rx_line_private() > dec_lane)
			dec_lane = kl_rx_line_private();
		/* the synthesis from rows: the decoder's frame without the channel
		 * read's (engine_warm warms it only if it is the larger) */
		if (kl_dec_private(1, 1) > dec_lane)
			dec_lane = kl_dec_private(1, 1);
		const size_t dec2_lane = kl_dec_private(2, 0) > kl_dec_private(2, 1) ? kl_dec_private(2, 0)
										     : kl_dec_private(2, 1);
		const size_t per_wave = (lane > dec_lane ? lane : dec_lane) * WAVE;
		const size_t mw_wave = kl_ana_mw_private() * WAVE;
		const size_t ww = kl_npp_private() > kl_harm_wave_private() ? kl_npp_private() : kl_harm_wave_private();
		const size_t waves = (size_t) (e->channels + WAVE - 1) / WAVE;
		const size_t mw_waves = 4 * (size_t) ((mw + WAVE - 1) / WAVE);
		size_t resident = (size_t) e->channels;
		hipDeviceProp_t prop;
		if (hipGetDeviceProperties(&prop, e->device) == hipSuccess) {
			const size_t r = (size_t) prop.multiProcessorCount * (size_t) (prop.maxThreadsPerMultiProcessor / WAVE);
			if (r > 0 && r < resident)
				resident = r;
		}
		size_t need = per_wave * waves;
		if (mw_wave * mw_waves > need)
			need = mw_wave * mw_waves;
		if (e->d_hb && dec2_lane * WAVE * 2 * waves > need)
			need = dec2_lane * WAVE * 2 * waves;
		if (ww * WAVE * resident > need)
			need = ww * WAVE * resident;
		size_t cur = 0, mx = 0;
		if (hipDeviceGetLimit(&cur, hipExtLimitScratchCurrent) == hipSuccess &&
		    hipDeviceGetLimit(&mx, hipExtLimitScratchMax) == hipSuccess && need > cur) {
			if (need > mx)
				return fail_msg("melpe_engine_create: the codec kernels' scratch exceeds the "
						"device's scratch limit (fewer channels per engine)");
			if ((er = hipDeviceSetLimit(hipExtLimitScratchCurrent, need)) != hipSuccess)
				return fail("melpe_engine_create: raising the scratch limit", er);
		}
		e->scratch_need = need;
	}
	return engine_warm(e);
}

int melpe_engine_create(melpe_engine **out, int device, int channels)
{
	if (!out || channels <= 0)
		return fail_msg("melpe_engine_create: bad arguments");
	int ndev = 0;
	HIPCHK(hipGetDeviceCount(&ndev));
	if (device < 0 || device >= ndev)
		return fail_msg("melpe_engine_create: no such HIP device");
	int rc = ensure_device_tables(device);
	if (rc)
		return rc;
	DEVGUARD(device);
	melpe_engine *e = new melpe_engine();
	e->device = device;
	e->channels = channels;
	hipError_t er = hipSuccess;
	const char *what = nullptr;
#define CREATE_STEP(expr) if (er == hipSuccess && (er = (expr)) != hipSuccess) what = #expr
	e->stream = g_dev_stream[device];
	CREATE_STEP(hipEventCreate(&e->ev0));
	CREATE_STEP(hipEventCreate(&e->ev1));
	CREATE_STEP(hipEventCreateWithFlags(&e->ev_in, hipEventDisableTiming));
	CREATE_STEP(hipEventCreateWithFlags(&e->ev_out, hipEventDisableTiming));
	CREATE_STEP(hipEventCreateWithFlags(&e->ev_host, hipEventDisableTiming));
	CREATE_STEP(hipEventCreateWithFlags(&e->ev_pin, hipEventDisableTiming));
	CREATE_STEP(hipEventCreateWithFlags(&e->ev_npp, hipEventDisableTiming));
	CREATE_STEP(hipMalloc(&e->d_enc, sizeof(EncState) * (size_t) channels));
	CREATE_STEP(hipMalloc(&e->d_dec, sizeof(DecState) * (size_t) channels));
	CREATE_STEP(hipMalloc(&e->d_syn, sizeof(synth_state) * (size_t) channels));
	CREATE_STEP(hipMalloc(&e->d_pcm, sizeof(int16_t) * MELPE_SF_SAMPLES * (size_t) channels));
	CREATE_STEP(hipMalloc(&e->d_bits, (size_t) MELPE_SF_BYTES * channels));
	CREATE_STEP(hipMalloc(&e->d_mask, (size_t) channels));
	CREATE_STEP(hipMalloc(&e->d_rxmask, (size_t) channels));
	CREATE_STEP(bin_alloc(&e->bin_enc, channels));
	CREATE_STEP(bin_alloc(&e->bin_dec, channels));
	CREATE_STEP(bin_alloc(&e->bin_enc2, channels));
#undef CREATE_STEP
	if (er != hipSuccess) {
		int r = fail(what, er);
		melpe_engine_destroy(e);	/* frees whatever was allocated */
		return r;
	}
	int r = melpe_engine_reset(e, nullptr, 3);
	if (r == 0)
		r = engine_reserve(e);
	if (r) {
		std::string m = g_err;
		melpe_engine_destroy(e);
		g_err = m;
		return r;
	}
	*out = e;
	return 0;
}

int melpe_engine_set_own_stream(melpe_engine *e, int on)
{
	if (!e)
		return fail_msg("melpe_engine_set_own_stream: null engine");
	DEVGUARD(e->device);
	HOST_LOCK(e);
	ENGINE_WAIT(e);
	HIPCHK(hipStreamSynchronize(e->stream));
	if (on && !e->own) {
		HIPCHK(hipStreamCreateWithFlags(&e->own, hipStreamNonBlocking));
		e->stream = e->own;
		/* the new queue's scratch, had here and not mid-stream */
		if (int rc = engine_warm(e)) {
			e->stream = g_dev_stream[e->device];
			hipStreamDestroy(e->own);
			e->own = nullptr;
			return rc;
		}
	} else if (!on && e->own) {
		e->stream = g_dev_stream[e->device];
		HIPCHK(hipStreamDestroy(e->own));
		e->own = nullptr;
	}
	return 0;
}

int melpe_engine_set_lane_order(melpe_engine *e, int on)
{
	if (!e)
		return fail_msg("melpe_engine_set_lane_order: null engine");
	std::lock_guard<std::recursive_mutex> lk(e->mu);
	e->lane_order = on ? 1 : 0;
	return 0;
}

int melpe_engine_set_mw_live_max(melpe_engine *e, int live_max)
{
	if (!e || live_max < 0)
		return fail_msg("melpe_engine_set_mw_live_max: a live-channel count >= 0");
	std::lock_guard<std::recursive_mutex> lk(e->mu);
	e->mw_live_max = live_max;
	return 0;
}

int melpe_engine_last_ana_waves(melpe_engine *e)
{
	if (!e)
		return fail_msg("melpe_engine_last_ana_waves: no engine");
	DEVGUARD(e->device);
	ENGINE_WAIT(e);
	int v = 0;
	HIPCHK(hipMemcpy(&v, e->bin_enc.ctl + 2 * NBIN + 1, sizeof(int), hipMemcpyDeviceToHost));
	return v;
}

int melpe_engine_set_dec_waves(melpe_engine *e, int waves)
{
	if (!e || !(waves == 0 || waves == 1 || waves == 2))
		return fail_msg("melpe_engine_set_dec_waves: waves must be 0 (auto), 1 or 2");
	if (waves == 2 && !e->d_hb)
		return fail_msg("melpe_engine_set_dec_waves: the two-wave decoder is available up to "
				"65,536 channels per engine");
	std::lock_guard<std::recursive_mutex> lk(e->mu);
	e->dec_waves = waves;
	return 0;
}

int melpe_engine_set_ana_waves(melpe_engine *e, int waves)
{
	if (!e || !(waves == 0 || waves == 1 || waves == 4))
		return fail_msg("melpe_engine_set_ana_waves: waves must be 0 (auto), 1 or 4");
	std::lock_guard<std::recursive_mutex> lk(e->mu);
	e->ana_waves = waves;
	return 0;
}

int melpe_engine_destroy(melpe_engine *e)
{
	if (!e)
		return 0;
	DevGuard dg(e->device);
	/* this engine's enqueued calls, not the whole shared stream */
	engine_wait(e);
	hipFree(e->d_npp);
	hipFree(e->d_enc);
	hipFree(e->d_dec);
	hipFree(e->d_syn);
	hipFree(e->d_pcm);
	hipFree(e->d_bits);
	hipFree(e->d_mask);
	hipFree(e->d_rxmask);
	hipFree(e->bin_enc.perm);
	hipFree(e->bin_dec.perm);
	hipFree(e->bin_enc2.perm);
	hipFree(e->d_lq);
	hipFree(e->d_hb);
	hipFree(e->d_res);
	for (auto &m : e->marks)
		hipEventDestroy(m.second);
	if (e->bin_enc.done)
		hipEventDestroy(e->bin_enc.done);
	if (e->bin_dec.done)
		hipEventDestroy(e->bin_dec.done);
	if (e->bin_enc2.done)
		hipEventDestroy(e->bin_enc2.done);
	if (e->ev0)
		hipEventDestroy(e->ev0);
	if (e->ev1)
		hipEventDestroy(e->ev1);
	if (e->ev_in)
		hipEventDestroy(e->ev_in);
	if (e->ev_out)
		hipEventDestroy(e->ev_out);
	if (e->ev_host)
		hipEventDestroy(e->ev_host);
	if (e->ev_pin)
		hipEventDestroy(e->ev_pin);
	if (e->ev_npp)
		hipEventDestroy(e->ev_npp);
	for (auto &sl : e->slot) {
		hipFree(sl.pcm);
		hipFree(sl.bits);
		hipFree(sl.mask);
		for (hipEvent_t ev : {sl.loaded, sl.done, sl.freed})
			if (ev)
				hipEventDestroy(ev);
	}
	if (e->own)
		hipStreamDestroy(e->own);
	if (e->cin)
		hipStreamDestroy(e->cin);
	if (e->cout)
		hipStreamDestroy(e->cout);
	if (e->cdec)
		hipStreamDestroy(e->cdec);
	if (e->ev_dec)
		hipEventDestroy(e->ev_dec);
	delete e;
	return 0;
}

int melpe_engine_channels(const melpe_engine *e)
{
	return e ? e->channels : 0;
}

int melpe_engine_reset_dev(melpe_engine *e, const void *d_mask, int which, void *hip_stream)
{
	if (!e || which < 1 || which > 3)
		return fail_msg("melpe_engine_reset_dev: bad arguments");
	return engine_call(e, (hipStream_t) hip_stream, TIME_NONE, [&](hipStream_t s) {
		if (int rc = kl_reset(e->d_enc, e->d_dec, (const uint8_t *) d_mask, e->channels, which, s))
			return fail("melpe_engine_reset_dev", (hipError_t) rc);
		return 0;
	});
}

int melpe_engine_reset(melpe_engine *e, const uint8_t *mask_host, int which)
{
	if (!e || which < 1 || which > 3)
		return fail_msg("melpe_engine_reset: bad arguments");
	DEVGUARD(e->device);
	HOST_LOCK(e);
	/* ordered after every *_dev call of this engine already enqueued, on
	 * any stream: those read and write the same channel records */
	ENGINE_WAIT(e);
	int rc;
	const uint8_t *m = stage_mask(e, mask_host, &rc);
	if (rc)
		return rc;
	if ((rc = kl_reset(e->d_enc, e->d_dec, m, e->channels, which, e->stream)))
		return fail("melpe_engine_reset", (hipError_t) rc);
	HOST_FINISH(e);
	return 0;
}

/* melpe_npp_dev / melpe_npp_host / melpe_n: `frames` frames per channel at `stride` samples */
static int npp_args_ok(int frames, int stride)
{
	if (frames <= 0 || stride < frames * MELPE_FRAME_SAMPLES)
		return fail_msg("melpe_npp: bad frames/stride");
	return 0;
}

int melpe_npp_dev(melpe_engine *e, void *d_sp, int frames, int stride, const void *d_active,
		  void *hip_stream)
{
	if (!e || !d_sp)
		return fail_msg("melpe_npp_dev: null argument");
	if (int rc = npp_args_ok(frames, stride))
		return rc;
	return engine_call(e, (hipStream_t) hip_stream, TIME_LAZY, [&](hipStream_t s) {
		HIPCHK((hipError_t) kl_npp(e->d_enc, (int16_t *) d_sp, frames, stride, (const uint8_t *) d_active,
					   e->channels, 1, s));
		return 0;
	});
}

int melpe_npp_host(melpe_engine *e, int16_t *sp, int frames, int stride, const uint8_t *active)
{
	if (!e || !sp || stride <= 0)
		return fail_msg("melpe_npp_host: bad arguments");
	if (int rc = npp_args_ok(frames, stride))
		return rc;
	DEVGUARD(e->device);
	HOST_LOCK(e);
	/* the staging buffer is grown before the staged call, under the same
	 * lock and once nothing enqueued reads the old one any more */
	ENGINE_WAIT(e);
	const size_t bytes = sizeof(int16_t) * (size_t) stride * e->channels;
	if (e->npp_bytes < bytes) {
		HIPCHK(hipFree(e->d_npp));
		e->d_npp = nullptr;
		e->npp_bytes = 0;
		HIPCHK(hipMalloc(&e->d_npp, bytes));
		e->npp_bytes = bytes;
	}
	return engine_host_call(e, active, {{sp, e->d_npp, bytes, XFER_IN | XFER_OUT}},
				[&](const uint8_t *m, hipStream_t s) {
		HIPCHK((hipError_t) kl_npp(e->d_enc, e->d_npp, frames, stride, m, e->channels, 1, s));
		return 0;
	});
}

/* melpe_a of every channel: the NPP in place, then the analysis */
static int encode_kernels(melpe_engine *e, void *d_bits, void *d_sp, const void *d_act, hipStream_t s)
{
	HIPCHK((hipError_t) kl_enc_npp(e->d_enc, (int16_t *) d_sp, (const uint8_t *) d_act, e->channels, s));
	HIPCHK((hipError_t) ana_launch(e, (const int16_t *) d_sp, (uint8_t *) d_bits, (const uint8_t *) d_act, s));
	return 0;
}

int melpe_encode_dev(melpe_engine *e, void *d_bits, void *d_sp, const void *d_active,
		     void *hip_stream)
{
	if (!e || !d_bits || !d_sp)
		return fail_msg("melpe_encode_dev: null argument");
	return engine_call(e, (hipStream_t) hip_stream, TIME_LAZY,
			   [&](hipStream_t s) { return encode_kernels(e, d_bits, d_sp, d_active, s); });
}

int melpe_encode_npp_dev(melpe_engine *e, void *d_sp, const void *d_active, void *hip_stream)
{
	if (!e || !d_sp)
		return fail_msg("melpe_encode_npp_dev: null argument");
	return engine_call(e, (hipStream_t) hip_stream, TIME_NONE, [&](hipStream_t s) {
		HIPCHK((hipError_t) kl_enc_npp(e->d_enc, (int16_t *) d_sp, (const uint8_t *) d_active,
					       e->channels, s));
		return 0;
	});
}

int melpe_encode_ana_dev(melpe_engine *e, void *d_bits, const void *d_sp, const void *d_active,
			 void *hip_stream)
{
	if (!e || !d_bits || !d_sp)
		return fail_msg("melpe_encode_ana_dev: null argument");
	return engine_call(e, (hipStream_t) hip_stream, TIME_NONE, [&](hipStream_t s) {
		HIPCHK((hipError_t) ana_launch(e, (const int16_t *) d_sp, (uint8_t *) d_bits,
					       (const uint8_t *) d_active, s));
		return 0;
	});
}

int melpe_encode_pipe_dev(melpe_engine *e, void *d_bits, const void *d_sp, const void *d_active,
			  void *d_sp_next, const void *d_active_next, void *hip_stream)
{
	if (!e || !d_bits || !d_sp)
		return fail_msg("melpe_encode_pipe_dev: null argument");
	if (d_sp_next == d_sp)
		return fail_msg("melpe_encode_pipe_dev: the next superframe's PCM must be another buffer");
	const PipeNext nx = {d_sp_next, d_active_next, nullptr, nullptr, nullptr};
	return pipe_step(e, d_bits, d_sp, d_active, d_sp_next ? &nx : nullptr, nullptr, (hipStream_t) hip_stream);
}

int melpe_duplex_pipe_dev(melpe_engine *e, void *d_bits, const void *d_sp, const void *d_active,
			  void *d_sp_next, const void *d_active_next, void *d_dec_sp,
			  const void *d_dec_bits, const void *d_dec_active, void *hip_stream)
{
	if (!e || !d_bits || !d_sp || (d_dec_bits && !d_dec_sp))
		return fail_msg("melpe_duplex_pipe_dev: null argument");
	if (d_sp_next == d_sp)
		return fail_msg("melpe_duplex_pipe_dev: the next superframe's PCM must be another buffer");
	if (d_dec_bits && (d_dec_bits == d_bits || d_dec_sp == d_sp || d_dec_sp == d_sp_next))
		return fail_msg("melpe_duplex_pipe_dev: the decode's buffers must differ from the encode's");
	const PipeNext nx = {d_sp_next, d_active_next, nullptr, nullptr, nullptr};
	const PipeDec dc = {d_dec_sp, d_dec_bits, d_dec_active};
	return pipe_step(e, d_bits, d_sp, d_active, d_sp_next ? &nx : nullptr, d_dec_bits ? &dc : nullptr,
			 (hipStream_t) hip_stream);
}

int melpe_encode_host(melpe_engine *e, unsigned char *bits, int16_t *sp, const uint8_t *active)
{
	if (!e || !bits || !sp)
		return fail_msg("melpe_encode_host: null argument");
	const size_t pb = sizeof(int16_t) * BLOCK * (size_t) e->channels, bb = (size_t) 11 * e->channels;
	return engine_host_call(e, active,
				{{sp, e->d_pcm, pb, XFER_IN | XFER_OUT}, {bits, e->d_bits, bb, XFER_IN_MASKED | XFER_OUT}},
				[&](const uint8_t *m, hipStream_t s) { return encode_kernels(e, e->d_bits, e->d_pcm, m, s); });
}

/* the host-fed pipeline's buffers and streams, made at its first call */
static int async_setup(melpe_engine *e)
{
	if (e->slot[0].pcm)
		return engine_streams(e, false);
	const size_t pb = sizeof(int16_t) * BLOCK * (size_t) e->channels, bb = (size_t) 11 * e->channels;
	for (auto &sl : e->slot) {
		HIPCHK(hipMalloc(&sl.pcm, pb));
		HIPCHK(hipMalloc(&sl.bits, bb));
		HIPCHK(hipMalloc(&sl.mask, (size_t) e->channels));
		for (hipEvent_t *ev : {&sl.loaded, &sl.done, &sl.freed})
			HIPCHK(hipEventCreateWithFlags(ev, hipEventDisableTiming));
	}
	return engine_streams(e, false);
}

int melpe_encode_host_async(melpe_engine *e, unsigned char *bits, int16_t *sp, const uint8_t *active)
{
	if (!e || !bits || !sp)
		return fail_msg("melpe_encode_host_async: null argument");
	DEVGUARD(e->device);
	HOST_LOCK(e);
	if (int rc = async_setup(e))
		return rc;
	const size_t pb = sizeof(int16_t) * BLOCK * (size_t) e->channels, bb = (size_t) 11 * e->channels;
	melpe_engine::Slot &sl = e->slot[e->async_calls & 1];
	/* the slot's previous superframe has left the device (its D2H) */
	if (sl.used)
		HIPCHK(hipStreamWaitEvent(e->cin, sl.freed, 0));
	/* (the copies touch only the slot; the kernels below are ordered after
	 * the engine's earlier calls by the engine stream itself) */
	if (active)
		HIPCHK(hipMemcpyAsync(sl.mask, active, (size_t) e->channels, hipMemcpyHostToDevice, e->cin));
	HIPCHK(hipMemcpyAsync(sl.pcm, sp, pb, hipMemcpyHostToDevice, e->cin));
	if (active)	/* inactive channels keep the caller's bits */
		HIPCHK(hipMemcpyAsync(sl.bits, bits, bb, hipMemcpyHostToDevice, e->cin));
	HIPCHK(hipEventRecord(sl.loaded, e->cin));
	/* the kernels on the engine stream, after the slot's H2D */
	HIPCHK(hipStreamWaitEvent(e->stream, sl.loaded, 0));
	HIPCHK((hipError_t) kl_enc_npp(e->d_enc, sl.pcm, active ? sl.mask : nullptr, e->channels, e->stream));
	HIPCHK((hipError_t) ana_launch(e, sl.pcm, sl.bits, active ? sl.mask : nullptr, e->stream));
	HIPCHK(hipEventRecord(sl.done, e->stream));
	/* the NPP output (melpe_a's in-place side effect) and the bits back */
	HIPCHK(hipStreamWaitEvent(e->cout, sl.done, 0));
	HIPCHK(hipMemcpyAsync(sp, sl.pcm, pb, hipMemcpyDeviceToHost, e->cout));
	HIPCHK(hipMemcpyAsync(bits, sl.bits, bb, hipMemcpyDeviceToHost, e->cout));
	HIPCHK(hipEventRecord(sl.freed, e->cout));
	sl.used = true;
	e->async_calls++;
	/* later calls of this engine (and engine_wait) are ordered after this
	 * one's last copy */
	return engine_mark(e, e->cout);
}

int melpe_encode_host_wait(melpe_engine *e)
{
	if (!e)
		return fail_msg("melpe_encode_host_wait: null argument");
	DEVGUARD(e->device);
	HOST_LOCK(e);
	for (auto &sl : e->slot)
		if (sl.used)
			HIPCHK(hipEventSynchronize(sl.freed));
	return 0;
}

int melpe_decode_dev(melpe_engine *e, void *d_sp, const void *d_bits, const void *d_active,
		     void *hip_stream)
{
	if (!e || !d_sp || !d_bits)
		return fail_msg("melpe_decode_dev: null argument");
	return engine_call(e, (hipStream_t) hip_stream, TIME_LAZY, [&](hipStream_t s) {
		HIPCHK((hipError_t) dec_launch(e, (int16_t *) d_sp, src_bits(d_bits), (const uint8_t *) d_active, s));
		return 0;
	});
}

int melpe_decode_host(melpe_engine *e, int16_t *sp, const unsigned char *bits,
		      const uint8_t *active)
{
	if (!e || !bits || !sp)
		return fail_msg("melpe_decode_host: null argument");
	const size_t pb = sizeof(int16_t) * BLOCK * (size_t) e->channels, bb = (size_t) 11 * e->channels;
	return engine_host_call(e, active,
				{{bits, e->d_bits, bb, XFER_IN}, {sp, e->d_pcm, pb, XFER_IN_MASKED | XFER_OUT}},
				[&](const uint8_t *m, hipStream_t s) {
		HIPCHK((hipError_t) dec_launch(e, e->d_pcm, src_bits(e->d_bits), m, s));
		return 0;
	});
}

/* The codec parameters as tensors (k_par.hip): the tap on the records of the
 * last melpe_a / melpe_s, and the parse-only decoder.  which: 0 = encoder
 * tap, 1 = decoder tap, 2 = parse (d_bits in). */
#define PAR_ROW_BYTES (sizeof(int16_t) * MELPE_PAR_WORDS * NF)
#define QPAR_ROW_BYTES (sizeof(int16_t) * MELPE_QPAR_WORDS)

static int params_kernels(melpe_engine *e, int which, void *d_par, void *d_qpar, const void *d_bits,
			  const void *d_active, hipStream_t s)
{
	const uint8_t *d_act = (const uint8_t *) d_active;
	uint32_t *par = (uint32_t *) d_par;
	if (which == 0)
		HIPCHK((hipError_t) kl_par_tap((const char *) e->d_enc, sizeof(EncState),
					       offsetof(EncState, a) + offsetof(EncAna, par), par, (uint32_t *) d_qpar,
					       d_act, e->channels, s));
	else if (which == 1)
		HIPCHK((hipError_t) kl_par_tap((const char *) e->d_dec, sizeof(DecState), offsetof(DecState, par), par,
					       nullptr, d_act, e->channels, s));
	else
		HIPCHK((hipError_t) kl_parse(e->d_dec, par, (const uint8_t *) d_bits, d_act, e->channels, s));
	return 0;
}

static int params_dev(melpe_engine *e, int which, void *d_par, void *d_qpar, const void *d_bits,
		      const void *d_active, void *hip_stream)
{
	if (((uintptr_t) d_par | (uintptr_t) d_qpar) & 3)
		return fail_msg("melpe parameter rows: device buffers must be 4-byte aligned");
	return engine_call(e, (hipStream_t) hip_stream, TIME_LAZY, [&](hipStream_t s) {
		return params_kernels(e, which, d_par, d_qpar, d_bits, d_active, s);
	});
}

int melpe_encode_params_dev(melpe_engine *e, void *d_par, void *d_qpar, const void *d_active,
			    void *hip_stream)
{
	if (!e || !d_par)
		return fail_msg("melpe_encode_params_dev: null argument");
	return params_dev(e, 0, d_par, d_qpar, nullptr, d_active, hip_stream);
}

int melpe_decode_params_dev(melpe_engine *e, void *d_par, const void *d_active, void *hip_stream)
{
	if (!e || !d_par)
		return fail_msg("melpe_decode_params_dev: null argument");
	return params_dev(e, 1, d_par, nullptr, nullptr, d_active, hip_stream);
}

int melpe_parse_dev(melpe_engine *e, void *d_par, const void *d_bits, const void *d_active,
		    void *hip_stream)
{
	if (!e || !d_par || !d_bits)
		return fail_msg("melpe_parse_dev: null argument");
	return params_dev(e, 2, d_par, nullptr, d_bits, d_active, hip_stream);
}

/* the host forms stage the rows in d_pcm (C x 1,080 bytes: a channel's par
 * row is 180 bytes, its qpar row 60, the qpar rows after all par rows) */
static int params_host(melpe_engine *e, int which, int16_t *par, int16_t *qpar, const unsigned char *bits,
		       const uint8_t *active)
{
	static_assert(PAR_ROW_BYTES + QPAR_ROW_BYTES <= sizeof(int16_t) * MELPE_SF_SAMPLES && PAR_ROW_BYTES % 4 == 0,
		      "the rows fit the PCM staging buffer");
	const size_t pb = PAR_ROW_BYTES * (size_t) e->channels, qb = QPAR_ROW_BYTES * (size_t) e->channels;
	char *d_par = (char *) e->d_pcm, *d_qpar = qpar ? d_par + pb : nullptr;
	return engine_host_call(e, active,
				{{bits, e->d_bits, (size_t) 11 * e->channels, XFER_IN},
				 {par, d_par, pb, XFER_IN_MASKED | XFER_OUT},
				 {qpar, d_qpar, qb, XFER_IN_MASKED | XFER_OUT}},
				[&](const uint8_t *m, hipStream_t s) {
		return params_kernels(e, which, d_par, d_qpar, e->d_bits, m, s);
	});
}

int melpe_encode_params_host(melpe_engine *e, int16_t *par, int16_t *qpar, const uint8_t *active)
{
	if (!e || !par)
		return fail_msg("melpe_encode_params_host: null argument");
	return params_host(e, 0, par, qpar, nullptr, active);
}

int melpe_decode_params_host(melpe_engine *e, int16_t *par, const uint8_t *active)
{
	if (!e || !par)
		return fail_msg("melpe_decode_params_host: null argument");
	return params_host(e, 1, par, nullptr, nullptr, active);
}

int melpe_parse_host(melpe_engine *e, int16_t *par, const unsigned char *bits, const uint8_t *active)
{
	if (!e || !par || !bits)
		return fail_msg("melpe_parse_host: null argument");
	return params_host(e, 2, par, nullptr, bits, active);
}

/* The synthesis from parameter rows (k_dec.hip RowsIn): d_par (C x 3 x 30 int16,
 * read only) in, d_sp (C x 540) and d_status (C bytes, optional) out */
int melpe_synth_params_dev(melpe_engine *e, void *d_sp, const void *d_par, void *d_status, const void *d_active,
			   void *hip_stream)
{
	if (!e || !d_sp || !d_par)
		return fail_msg("melpe_synth_params_dev: null argument");
	if ((uintptr_t) d_par & 3)
		return fail_msg("melpe_synth_params_dev: the parameter rows must be 4-byte aligned");
	return engine_call(e, (hipStream_t) hip_stream, TIME_LAZY, [&](hipStream_t s) {
		HIPCHK((hipError_t) dec_launch(e, (int16_t *) d_sp, src_rows(d_par, (uint8_t *) d_status),
					       (const uint8_t *) d_active, s));
		return 0;
	});
}

/* the host form stages the rows and the status bytes in the analysis'
 * residual buffer (C x 1,200 bytes, in use only inside an encode call) */
int melpe_synth_params_host(melpe_engine *e, int16_t *sp, const int16_t *par, uint8_t *status,
			    const uint8_t *active)
{
	if (!e || !sp || !par)
		return fail_msg("melpe_synth_params_host: null argument");
	static_assert(PAR_ROW_BYTES + 1 <= sizeof(int16_t) * NF * LPC_FRAME && PAR_ROW_BYTES % 4 == 0,
		      "the rows and the status bytes fit the residual buffer");
	const size_t pb = sizeof(int16_t) * BLOCK * (size_t) e->channels, rb = PAR_ROW_BYTES * (size_t) e->channels;
	char *d_par = (char *) e->d_res;
	uint8_t *d_status = status ? (uint8_t *) d_par + rb : nullptr;
	return engine_host_call(e, active,
				{{par, d_par, rb, XFER_IN},
				 {sp, e->d_pcm, pb, XFER_IN_MASKED | XFER_OUT},
				 {status, d_status, (size_t) e->channels, XFER_IN_MASKED | XFER_OUT}},
				[&](const uint8_t *m, hipStream_t s) {
		HIPCHK((hipError_t) dec_launch(e, e->d_pcm, src_rows(d_par, d_status), m, s));
		return 0;
	});
}

/* private-segment bytes per lane of the synthesis kernels (diagnostics):
 * waves = 1 k_synth_par, 2 k_synth_par2 */
int melpe_synth_params_private_bytes(int waves)
{
	return (int) kl_dec_private(waves == 2 ? 2 : 1, 1);
}

/* 2400 bps mode (codec2400.h): NPP of one 180-sample frame at RATE2400
 * (k_npp, melpe/npp.c:180-184 first-call branch), then analysis + 54-bit
 * packing (k_enc24); decode = channel read + synthesis of one frame */
static int encode24_kernels(melpe_engine *e, void *d_bits, void *d_sp, const void *d_act, hipStream_t s)
{
	HIPCHK((hipError_t) kl_npp(e->d_enc, (int16_t *) d_sp, 1, MELPE_FRAME_SAMPLES, (const uint8_t *) d_act,
				   e->channels, 0, s));
	HIPCHK((hipError_t) kl_enc24(e->d_enc, (const int16_t *) d_sp, (uint8_t *) d_bits, (const uint8_t *) d_act,
				     e->channels, s));
	return 0;
}

static int decode24_kernels(melpe_engine *e, void *d_sp, const void *d_bits, const void *d_act, hipStream_t s)
{
	HIPCHK((hipError_t) kl_dec24(e->d_dec, (int16_t *) d_sp, (const uint8_t *) d_bits, (const uint8_t *) d_act,
				     e->channels, s));
	return 0;
}

int melpe_encode2400_dev(melpe_engine *e, void *d_bits, void *d_sp, const void *d_active,
			 void *hip_stream)
{
	if (!e || !d_bits || !d_sp)
		return fail_msg("melpe_encode2400_dev: null argument");
	return engine_call(e, (hipStream_t) hip_stream, TIME_LAZY,
			   [&](hipStream_t s) { return encode24_kernels(e, d_bits, d_sp, d_active, s); });
}

int melpe_decode2400_dev(melpe_engine *e, void *d_sp, const void *d_bits, const void *d_active,
			 void *hip_stream)
{
	if (!e || !d_sp || !d_bits)
		return fail_msg("melpe_decode2400_dev: null argument");
	return engine_call(e, (hipStream_t) hip_stream, TIME_LAZY,
			   [&](hipStream_t s) { return decode24_kernels(e, d_sp, d_bits, d_active, s); });
}

int melpe_encode2400_host(melpe_engine *e, unsigned char *bits, int16_t *sp, const uint8_t *active)
{
	if (!e || !bits || !sp)
		return fail_msg("melpe_encode2400_host: null argument");
	const size_t pb = sizeof(int16_t) * MELPE_FRAME_SAMPLES * (size_t) e->channels;
	const size_t bb = (size_t) MELPE_R24_BYTES * e->channels;
	return engine_host_call(e, active,
				{{sp, e->d_pcm, pb, XFER_IN | XFER_OUT}, {bits, e->d_bits, bb, XFER_IN_MASKED | XFER_OUT}},
				[&](const uint8_t *m, hipStream_t s) { return encode24_kernels(e, e->d_bits, e->d_pcm, m, s); });
}

int melpe_decode2400_host(melpe_engine *e, int16_t *sp, const unsigned char *bits,
			  const uint8_t *active)
{
	if (!e || !bits || !sp)
		return fail_msg("melpe_decode2400_host: null argument");
	const size_t pb = sizeof(int16_t) * MELPE_FRAME_SAMPLES * (size_t) e->channels;
	const size_t bb = (size_t) MELPE_R24_BYTES * e->channels;
	return engine_host_call(e, active,
				{{bits, e->d_bits, bb, XFER_IN}, {sp, e->d_pcm, pb, XFER_IN_MASKED | XFER_OUT}},
				[&](const uint8_t *m, hipStream_t s) { return decode24_kernels(e, e->d_pcm, e->d_bits, m, s); });
}

/* per-channel state records (checkpoint / migration between engines) */
static int state_geom(melpe_engine *e, int which, int first, int count, size_t *rec,
		      char **base)
{
	if (!e || (which != 1 && which != 2) || first < 0 || count < 0 ||
	    first + (long) count > e->channels)
		return fail_msg("melpe_engine_state: bad arguments");
	*rec = which == 1 ? sizeof(EncState) : sizeof(DecState);
	*base = which == 1 ? (char *) e->d_enc : (char *) e->d_dec;
	return 0;
}

long melpe_engine_state_bytes(int which)
{
	return which == 1 ? (long) sizeof(EncState) : which == 2 ? (long) sizeof(DecState) : -1;
}

int melpe_engine_export(melpe_engine *e, int which, int first, int count, void *host_out)
{
	size_t rec;
	char *base;
	if (int r = state_geom(e, which, first, count, &rec, &base))
		return r;
	if (!host_out && count)
		return fail_msg("melpe_engine_export: null buffer");
	DEVGUARD(e->device);
	HOST_LOCK(e);
	ENGINE_WAIT(e);
	HIPCHK(hipMemcpy(host_out, base + rec * first, rec * count, hipMemcpyDeviceToHost));
	return 0;
}

int melpe_engine_import(melpe_engine *e, int which, int first, int count, const void *host_in)
{
	size_t rec;
	char *base;
	if (int r = state_geom(e, which, first, count, &rec, &base))
		return r;
	if (!host_in && count)
		return fail_msg("melpe_engine_import: null buffer");
	const uint32_t want = which == 1 ? ENC_REC_FMT : DEC_REC_FMT;
	const size_t tag = which == 1 ? offsetof(EncState, fmt) : offsetof(DecState, fmt);
	for (int k = 0; k < count; k++) {
		uint32_t f;
		memcpy(&f, (const char *) host_in + rec * k + tag, sizeof f);
		if (f != want)
			return fail_msg("melpe_engine_import: record " + std::to_string(k) +
					" is not a state record of this library's layout");
	}
	DEVGUARD(e->device);
	HOST_LOCK(e);
	ENGINE_WAIT(e);
	HIPCHK(hipMemcpy(base + rec * first, host_in, rec * count, hipMemcpyHostToDevice));
	return 0;
}

int melpe_synth_seed(melpe_engine *e, uint32_t run_seed, uint32_t first_channel)
{
	if (!e)
		return fail_msg("null engine");
	DEVGUARD(e->device);
	HOST_LOCK(e);
	if (int rc = kl_synth_seed(e->d_syn, run_seed, first_channel, e->channels, e->stream))
		return fail("melpe_synth_seed", (hipError_t) rc);
	HOST_FINISH(e);
	return 0;
}

int melpe_synth_dev(melpe_engine *e, void *d_sp, int samples, void *hip_stream)
{
	if (!e || !d_sp || samples <= 0)
		return fail_msg("melpe_synth_dev: bad arguments");
	return engine_call(e, (hipStream_t) hip_stream, TIME_NONE, [&](hipStream_t s) {
		if (int rc = kl_synth(e->d_syn, (int16_t *) d_sp, samples, e->channels, s))
			return fail("melpe_synth_dev", (hipError_t) rc);
		return 0;
	});
}

int melpe_synth_host(uint32_t run_seed, uint32_t channel, int16_t *out, int samples)
{
	synth_state st;
	synth_init(&st, synth_mix(run_seed, channel));
	synth_block(&st, out, samples);
	return 0;
}

int melpe_debug_encode_stage(melpe_engine *e, void *d_sp, int upto)
{
	if (!e || !d_sp)
		return fail_msg("melpe_debug_encode_stage: null argument");
	DEVGUARD(e->device);
	HIPCHK((hipError_t) kl_enc_npp(e->d_enc, (int16_t *) d_sp, nullptr, e->channels, e->stream));
	if (upto > 0)
		HIPCHK((hipError_t) kl_enc_ana_dbg(e->d_enc, (int16_t *) d_sp, e->channels, upto,
						   e->stream));
	HIPCHK(hipStreamSynchronize(e->stream));
	return 0;
}

#define MELPE_PROF_SLOTS_ABI 256	/* ops.h MELPE_PROF_SLOTS of the profiling build */

int melpe_prof_read(uint64_t *out, int n)
{
	uint64_t acc[MELPE_PROF_SLOTS_ABI] = {0};
#define TU_PROF(name) melpe_tu_##name##_prof,
	int (*rd[])(uint64_t *) = {MELPE_TU_LIST(TU_PROF)};
#undef TU_PROF
	for (auto f : rd)
		if (f(acc))
			return fail_msg("not a profiling build (-DMELPE_PROF)");
	for (int i = 0; i < n && i < MELPE_PROF_SLOTS_ABI; i++)
		out[i] = acc[i];
	return MELPE_PROF_SLOTS_ABI;
}

double melpe_last_kernel_ms(const melpe_engine *ce)
{
	melpe_engine *e = (melpe_engine *) ce;
	if (!e)
		return 0.0;
	if (e->last_ms < 0.f) {
		if (hipEventSynchronize(e->ev1) != hipSuccess ||
		    hipEventElapsedTime(&e->last_ms, e->ev0, e->ev1) != hipSuccess)
			e->last_ms = 0.f;
	}
	return e->last_ms;
}

/* ------------------------------------------------------------------ */
/* single-stream drop-in (include/melpe.h)                            */
/* ------------------------------------------------------------------ */

static melpe_engine *g_single = nullptr;
static bool g_single_rate1200 = false;	/* melpe_i sets rate = RATE1200 */
static bool g_single_rate2400 = false;	/* melpe_i2 sets rate = RATE2400 */
static bool g_single_npp_started = false;	/* npp's static first_time has fired */

static melpe_engine *single_engine(void)
{
	if (!g_single) {
		if (melpe_engine_create(&g_single, 0, 1)) {
			fprintf(stderr, "libmelpe_amd: no usable GPU: %s\n", g_err.c_str());
			abort();
		}
	}
	return g_single;
}

void melpe_n(short *sp)
{
	melpe_engine *e = single_engine();
	DevGuard dg(e->device);
	/* npp reads 256 samples only on its very first call (from melpe_n or
	 * melpe_a) and only when rate == RATE1200 (melpe/npp.c:176-179);
	 * every other call reads the caller's 180 */
	size_t n = (!g_single_npp_started && g_single_rate1200) ? 256 : 180;
	int16_t *d = e->d_pcm;
	if (dg.err != hipSuccess ||
	    hipMemcpy(d, sp, sizeof(int16_t) * n, hipMemcpyHostToDevice) != hipSuccess ||
	    engine_call(e, e->stream, TIME_SYNC, [&](hipStream_t s) {
		    HIPCHK((hipError_t) kl_npp(e->d_enc, d, 1, 256, nullptr, e->channels, g_single_rate1200 ? 1 : 0, s));
		    return 0;
	    }) ||
	    hipMemcpy(sp, d, sizeof(int16_t) * 180, hipMemcpyDeviceToHost) != hipSuccess) {
		fprintf(stderr, "libmelpe_amd: melpe_n failed: %s\n", g_err.c_str());
		abort();
	}
	g_single_npp_started = true;
}

int melpe_single_reset(void)
{
	melpe_engine *e = single_engine();
	g_single_rate1200 = false;
	g_single_rate2400 = false;
	g_single_npp_started = false;
	return melpe_engine_reset(e, nullptr, 3);
}

/* melp_ana_init + melp_syn_init, and the rate the later calls run at */
static void single_init(const char *who, bool rate2400)
{
	melpe_engine *e = single_engine();
	DevGuard dg(e->device);
	if (kl_melpe_i(e->d_enc, e->d_dec, e->stream) || hipStreamSynchronize(e->stream) != hipSuccess) {
		fprintf(stderr, "libmelpe_amd: %s failed\n", who);
		abort();
	}
	g_single_rate1200 = !rate2400;
	g_single_rate2400 = rate2400;
}

void melpe_i(void)
{
	single_init("melpe_i", false);
}

/* melpe_i2 / melpe_al: the 2400 bps entry points the reference declares
 * (melpe/melpe.c:57-58) but never defines.  melpe_i2 = melpe_i at RATE2400
 * (melp_ana_init + melp_syn_init, one-frame blocks); melpe_al = melpe_a's
 * body for one 180-sample frame: npp in place, analysis, 7 bytes out.
 * After melpe_i2, melpe_s decodes one 7-byte frame into 180 samples (the
 * reference's synthesis() at RATE2400). */
void melpe_i2(void)
{
	single_init("melpe_i2", true);
}

void melpe_al(unsigned char *buf, short *sp)
{
	melpe_engine *e = single_engine();
	if (!g_single_rate2400) {
		fprintf(stderr, "libmelpe_amd: melpe_al needs melpe_i2 first\n");
		abort();
	}
	if (melpe_encode2400_host(e, buf, sp, nullptr)) {
		fprintf(stderr, "libmelpe_amd: melpe_al failed: %s\n", g_err.c_str());
		abort();
	}
	g_single_npp_started = true;
}

void melpe_a(unsigned char *buf, short *sp)
{
	melpe_engine *e = single_engine();
	if (melpe_encode_host(e, buf, sp, nullptr)) {
		fprintf(stderr, "libmelpe_amd: melpe_a failed: %s\n", g_err.c_str());
		abort();
	}
	g_single_npp_started = true;
}

void melpe_s(short *sp, unsigned char *buf)
{
	melpe_engine *e = single_engine();
	DevGuard dg(e->device);
	/* after melpe_i2, synthesis() at RATE2400: 7 bytes -> 180 samples */
	const bool r24 = g_single_rate2400;
	int rc = kl_share_params(e->d_enc, e->d_dec, 0, e->stream) ||
		 (r24 ? melpe_decode2400_host(e, sp, buf, nullptr) : melpe_decode_host(e, sp, buf, nullptr));
	if (!rc) {
		rc = kl_share_params(e->d_enc, e->d_dec, 1, e->stream) || hipStreamSynchronize(e->stream) != hipSuccess;
	}
	if (rc) {
		fprintf(stderr, "libmelpe_amd: melpe_s%s failed: %s\n", r24 ? " (2400)" : "", g_err.c_str());
		abort();
	}
}


int melpe_modem_state_bytes(void)
{
	return (int) sizeof(ModemState);
}

static int modem_state_ok(const void *d_state, int channels)
{
	if (!d_state || channels <= 0)
		return fail_msg("modem: bad arguments");
	return state_aligned("modem", d_state);
}

int melpe_modem_reset_dev(void *d_state, int channels, const void *d_mask, void *hip_stream)
{
	if (int r = modem_state_ok(d_state, channels))
		return r;
	if (int rc = kl_modem_reset((ModemState *) d_state, (const uint8_t *) d_mask, channels, (hipStream_t) hip_stream))
		return fail("melpe_modem_reset_dev", (hipError_t) rc);
	return 0;
}

/* the same records written on the host (no GPU): what a caller uploads */
int melpe_modem_reset_host(void *state, int channels)
{
	if (!state || channels <= 0 || ((uintptr_t) state & 3))
		return fail_msg("melpe_modem_reset_host: bad arguments");
	for (int c = 0; c < channels; c++)
		modem_reset((ModemState *) state + c);
	return 0;
}

int melpe_modulate_dev(void *d_state, const void *d_pkts, void *d_pcm, int channels, int packets,
		       const void *d_active, void *hip_stream)
{
	if (int r = modem_state_ok(d_state, channels))
		return r;
	if (!d_pkts || !d_pcm || packets <= 0 || ((uintptr_t) d_pcm & 3))
		return fail_msg("melpe_modulate_dev: bad arguments (pcm must be 4-byte aligned)");
	long waves = (long) channels * packets;
	if ((waves + 3) / 4 > 0x7fffffffL)
		return fail_msg("melpe_modulate_dev: too many packets");
	if (int rc = kl_modulate((ModemState *) d_state, (const uint8_t *) d_pkts, (int16_t *) d_pcm, channels, packets,
				 (const uint8_t *) d_active, (hipStream_t) hip_stream))
		return fail("melpe_modulate_dev", (hipError_t) rc);
	return 0;
}

int melpe_demodulate_dev(void *d_state, const void *d_pcm, long stride, void *d_pos, void *d_data,
			 void *d_out, void *d_ret, int channels, int calls, const void *d_active,
			 void *hip_stream)
{
	if (int r = modem_state_ok(d_state, channels))
		return r;
	if (!d_pcm || !d_pos || !d_data || calls <= 0 || stride < MODEM_LOOKAHEAD ||
	    ((uintptr_t) d_pos & 3) || ((uintptr_t) d_ret & 3))
		return fail_msg("melpe_demodulate_dev: bad arguments");
	if (int rc = kl_demodulate((ModemState *) d_state, (const int16_t *) d_pcm, stride, (int32_t *) d_pos,
				   (uint8_t *) d_data, (uint8_t *) d_out, (int32_t *) d_ret, channels, calls,
				   (const uint8_t *) d_active, (hipStream_t) hip_stream))
		return fail("melpe_demodulate_dev", (hipError_t) rc);
	return 0;
}

int melpe_ops_eval_dev(int op, const void *d_a, const void *d_b, const void *d_c, void *d_out,
		       long n, void *hip_stream)
{
	if (op < 0 || op >= MELPE_OPS_EVAL_COUNT || !d_a || !d_out || n <= 0 ||
	    (n + 255) / 256 > 0x7fffffffL)
		return fail_msg("melpe_ops_eval_dev: bad arguments");
	if (int rc = kl_ops_eval(op, (const int64_t *) d_a, (const int32_t *) d_b, (const int32_t *) d_c,
				 (int64_t *) d_out, n, (hipStream_t) hip_stream))
		return fail("melpe_ops_eval_dev", (hipError_t) rc);
	return 0;
}

int melpe_divide_s_sweep_dev(void *d_digest, void *hip_stream)
{
	if (!d_digest)
		return fail_msg("melpe_divide_s_sweep_dev: null argument");
	if (int rc = kl_divide_s_sweep((uint64_t *) d_digest, (hipStream_t) hip_stream))
		return fail("melpe_divide_s_sweep_dev", (hipError_t) rc);
	return 0;
}

int melpe_helpers_eval_dev(int mode, const void *d_src, const void *d_args, void *d_out, int n,
			   void *hip_stream)
{
	if (!d_src || !d_args || !d_out || n < 0 || mode < 0 || mode > 8)
		return fail_msg("melpe_helpers_eval_dev: bad arguments");
	if (n == 0)
		return 0;
	if (int rc = kl_helpers_eval(mode, (const int16_t *) d_src, (const int32_t *) d_args, (int32_t *) d_out, n,
				     (hipStream_t) hip_stream))
		return fail("melpe_helpers_eval_dev", (hipError_t) rc);
	return 0;
}

/* the tables of every TU on the caller's current device (the path engine
 * creation takes), for the engine-less self-tests that read them */
static int current_device_tables(void)
{
	int dev = 0;
	HIPCHK(hipGetDevice(&dev));
	return ensure_device_tables(dev);
}

int melpe_dsp_eval_dev(int mode, const void *d_in, const void *d_args, void *d_out, int n,
		       void *hip_stream)
{
	if (!d_in || !d_args || !d_out || n < 0 || mode < 0 || mode >= DE_MODE_COUNT)
		return fail_msg("melpe_dsp_eval_dev: bad arguments");
	if (n == 0)
		return 0;
	if (int rc = current_device_tables())
		return rc;
	if (int rc = kl_dsp_eval(mode, (const int16_t *) d_in, (const int32_t *) d_args, (int32_t *) d_out, n,
				 (hipStream_t) hip_stream))
		return fail("melpe_dsp_eval_dev", (hipError_t) rc);
	return 0;
}

int melpe_ana_eval_dev(int mode, const void *d_in, const void *d_args, void *d_out, int n,
		       void *hip_stream)
{
	if (!d_in || !d_args || !d_out || n < 0 || mode < 0 || mode >= AE_MODE_COUNT)
		return fail_msg("melpe_ana_eval_dev: bad arguments");
	if (n == 0)
		return 0;
	if (int rc = current_device_tables())
		return rc;
	if (int rc = kl_ana_eval(mode, (const int16_t *) d_in, (const int32_t *) d_args, (int32_t *) d_out, n,
				 (hipStream_t) hip_stream))
		return fail("melpe_ana_eval_dev", (hipError_t) rc);
	return 0;
}

int melpe_ana_scalar_dev(int mode, const void *d_args, void *d_out, long n, void *hip_stream)
{
	if (!d_args || !d_out || n < 0 || n > 0x7fffffffL || mode < 0 || mode >= AE_SCALAR_COUNT)
		return fail_msg("melpe_ana_scalar_dev: bad arguments");
	if (n == 0)
		return 0;
	if (int rc = current_device_tables())
		return rc;
	if (int rc = kl_ana_scalar(mode, (const int32_t *) d_args, (int32_t *) d_out, n, (hipStream_t) hip_stream))
		return fail("melpe_ana_scalar_dev", (hipError_t) rc);
	return 0;
}

int melpe_dsp_scalar_dev(int mode, int lds_tables, const void *d_args, void *d_out, long n,
			 void *hip_stream)
{
	/* n within int: either form's grid (256 or 64 cases per block) fits */
	if (!d_args || !d_out || n < 0 || n > 0x7fffffffL || mode < 0 || mode >= DE_SCALAR_COUNT ||
	    (lds_tables && mode > DE_SCALAR_LDS_LAST))
		return fail_msg("melpe_dsp_scalar_dev: bad arguments");
	if (n == 0)
		return 0;
	if (int rc = current_device_tables())
		return rc;
	int rc = lds_tables ? kl_dsp_scalar_lds(mode, (const int32_t *) d_args, (int32_t *) d_out, n,
						(hipStream_t) hip_stream)
			    : kl_dsp_scalar(mode, (const int32_t *) d_args, (int32_t *) d_out, n,
					    (hipStream_t) hip_stream);
	if (rc)
		return fail("melpe_dsp_scalar_dev", (hipError_t) rc);
	return 0;
}

int melpe_dsp_wave_dev(int mode, const void *d_in, const void *d_args, void *d_out, int n,
		       void *hip_stream)
{
	if (!d_in || !d_args || !d_out || n < 0 || mode < 0 || mode >= DE_WAVE_COUNT)
		return fail_msg("melpe_dsp_wave_dev: bad arguments");
	if (n == 0)
		return 0;
	if (int rc = current_device_tables())
		return rc;
	int rc = mode == DE_WAVE_FIND_HARM
			 ? kl_dsp_wave_harm((const int16_t *) d_in, (const int32_t *) d_args, (int32_t *) d_out, n,
					    (hipStream_t) hip_stream)
			 : kl_dsp_wave_fft(mode, (const int16_t *) d_in, (const int32_t *) d_args,
					   (int32_t *) d_out, n, (hipStream_t) hip_stream);
	if (rc)
		return fail("melpe_dsp_wave_dev", (hipError_t) rc);
	return 0;
}

int melpe_voice_crypt_dev(void *d_pkts, const void *d_counters, const void *d_keys,
			  const void *d_invert, int channels, int packets, int dir,
			  void *hip_stream)
{
	if (!d_pkts || !d_counters || !d_keys || channels <= 0 || packets <= 0 ||
	    (dir != 0 && dir != 1))
		return fail_msg("melpe_voice_crypt_dev: bad arguments");
	if (((uintptr_t) d_keys & 15) || ((uintptr_t) d_counters & 3))
		return fail_msg("melpe_voice_crypt_dev: keys must be 16-byte and counters "
				"4-byte aligned");
	long n = (long) channels * packets;
	long blocks = (n + 255) / 256;
	if (blocks > 0x7fffffffL)
		return fail_msg("melpe_voice_crypt_dev: too many packets");
	if (int rc = kl_voice_crypt((unsigned char *) d_pkts, (const uint32_t *) d_counters, (const uint4 *) d_keys,
				    (const uint8_t *) d_invert, channels, packets, dir, (hipStream_t) hip_stream))
		return fail("melpe_voice_crypt_dev", (hipError_t) rc);
	return 0;
}

int melpe_voice_crypt_host(unsigned char *pkts, const uint32_t *counters,
			   const unsigned char *keys, const uint8_t *invert, int channels,
			   int packets, int dir)
{
	if (!pkts || !counters || !keys || channels <= 0 || packets <= 0)
		return fail_msg("melpe_voice_crypt_host: bad arguments");
	const size_t n = (size_t) channels;
	/* the keys first: 16-byte aligned at the head of the stage buffer */
	Xfer x[] = {{keys, nullptr, n * VC_KEY_BYTES, XFER_IN},
		    {counters, nullptr, n * 4, XFER_IN},
		    {invert, nullptr, n, XFER_IN},
		    {pkts, nullptr, n * packets * VC_PKT_BYTES, XFER_IN | XFER_OUT}};
	return stage_host_call("melpe_voice_crypt_host", x, 4, [&] {
		return melpe_voice_crypt_dev(x[3].dev, x[1].dev, x[0].dev, x[2].dev, channels, packets, dir, nullptr);
	});
}


/* the link's packet layer (k_link.hip, link.h) */
#define LINK_STATE_BYTES 256

int melpe_link_state_bytes(void)
{
	return LINK_STATE_BYTES;
}

/* argument errors, refused before any HIP call */
static int link_args(const char *who, const void *state, const void *pkts, const void *ret, int channels,
		     int packets, bool dev)
{
	const std::string w(who);
	if (channels <= 0 || packets <= 0)
		return fail_msg(w + ": channels and packets must be positive");
	if (!state)
		return fail_msg(w + ": null state pointer");
	if (!pkts)
		return fail_msg(w + ": null packet pointer");
	if (!ret)
		return fail_msg(w + ": null return-value pointer");
	if (int rc = state_aligned(who, state))
		return rc;
	if (dev && (((uintptr_t) pkts & 3) || ((uintptr_t) ret & 3)))
		return fail_msg(w + ": packets and return values must be 4-byte aligned");
	if ((long) channels * packets > 0x7fffffffL / VC_PKT_BYTES)
		return fail_msg(w + ": too many packets");
	return 0;
}

int melpe_link_tx_dev(void *d_state, void *d_pkts, const void *d_voiced, void *d_ret, int channels,
		      int packets, const void *d_active, void *hip_stream)
{
	if (int rc = link_args("melpe_link_tx_dev", d_state, d_pkts, d_ret, channels, packets, true))
		return rc;
	if (int rc = kl_link_tx((LinkState *) d_state, (uint8_t *) d_pkts, (const uint8_t *) d_voiced, (int32_t *) d_ret,
				(const uint8_t *) d_active, channels, packets, (hipStream_t) hip_stream))
		return fail("melpe_link_tx_dev", (hipError_t) rc);
	return 0;
}

int melpe_link_rx_dev(void *d_state, void *d_pkts, void *d_ret, void *d_voice, int channels, int packets,
		      const void *d_active, void *hip_stream)
{
	if (int rc = link_args("melpe_link_rx_dev", d_state, d_pkts, d_ret, channels, packets, true))
		return rc;
	if (int rc = kl_link_rx((LinkState *) d_state, (uint8_t *) d_pkts, (int32_t *) d_ret, (uint8_t *) d_voice,
				(const uint8_t *) d_active, channels, packets, (hipStream_t) hip_stream))
		return fail("melpe_link_rx_dev", (hipError_t) rc);
	return 0;
}

/* host buffers: one staged upload per tensor, the same kernels, and back.
 * flag = voiced (TX, in) or voice (RX, out), C x K bytes, optional */
static int link_host(bool tx, void *state, unsigned char *pkts, uint8_t *flag, int32_t *ret, int channels,
		     int packets, const uint8_t *active)
{
	const char *who = tx ? "melpe_link_tx_host" : "melpe_link_rx_host";
	if (int rc = link_args(who, state, pkts, ret, channels, packets, false))
		return rc;
	const size_t n = (size_t) channels * packets;
	/* an inactive or refused channel keeps its outputs: ret (and RX voice) go up too */
	Xfer x[] = {{state, nullptr, (size_t) channels * LINK_STATE_BYTES, XFER_IN | XFER_OUT},
		    {ret, nullptr, n * 4, XFER_IN | XFER_OUT},
		    {pkts, nullptr, n * VC_PKT_BYTES, XFER_IN | XFER_OUT},
		    {flag, nullptr, n, tx ? XFER_IN : XFER_IN | XFER_OUT},
		    {active, nullptr, (size_t) channels, XFER_IN}};
	return stage_host_call(who, x, 5, [&] {
		return tx ? melpe_link_tx_dev(x[0].dev, x[2].dev, x[3].dev, x[1].dev, channels, packets, x[4].dev, nullptr)
			  : melpe_link_rx_dev(x[0].dev, x[2].dev, x[1].dev, x[3].dev, channels, packets, x[4].dev,
					      nullptr);
	});
}

int melpe_link_tx_host(void *state, unsigned char *pkts, const uint8_t *voiced, int32_t *ret, int channels,
		       int packets, const uint8_t *active)
{
	return link_host(true, state, pkts, (uint8_t *) voiced, ret, channels, packets, active);
}

int melpe_link_rx_host(void *state, unsigned char *pkts, int32_t *ret, uint8_t *voice, int channels,
		       int packets, const uint8_t *active)
{
	return link_host(false, state, pkts, voice, ret, channels, packets, active);
}

int melpe_golay_sweep_dev(void *d_enc, void *d_digest, void *hip_stream)
{
	if (!d_enc || !d_digest)
		return fail_msg("melpe_golay_sweep_dev: null argument");
	if (((uintptr_t) d_enc & 3) || ((uintptr_t) d_digest & 7))
		return fail_msg("melpe_golay_sweep_dev: misaligned argument");
	if (int rc = kl_golay_sweep((uint32_t *) d_enc, (uint64_t *) d_digest, (hipStream_t) hip_stream))
		return fail("melpe_golay_sweep_dev", (hipError_t) rc);
	return 0;
}

int melpe_vad_state_bytes(void)
{
	return (int) sizeof(VadState);
}

int melpe_vad_reset_dev(void *d_state, int channels, const void *d_mask, void *hip_stream)
{
	if (!d_state || channels <= 0)
		return fail_msg("melpe_vad_reset_dev: bad arguments");
	if (int rc = state_aligned("melpe_vad_reset_dev", d_state))
		return rc;
	if (int rc = kl_vad_reset((VadState *) d_state, (const uint8_t *) d_mask, channels, (hipStream_t) hip_stream))
		return fail("melpe_vad_reset_dev", (hipError_t) rc);
	return 0;
}

int melpe_vad_dev(void *d_state, const void *d_sp, void *d_votes, int channels,
		  const void *d_active, void *hip_stream)
{
	if (!d_state || !d_sp || !d_votes || channels <= 0)
		return fail_msg("melpe_vad_dev: bad arguments");
	if (int rc = state_aligned("melpe_vad_dev", d_state))
		return rc;
	return vad_launch(d_state, d_sp, d_votes, nullptr, d_active, channels, (hipStream_t) hip_stream);
}

int melpe_vad_host(unsigned char *state, const int16_t *sp, uint8_t *votes, int channels,
		   const uint8_t *active)
{
	if (!state || !sp || !votes || channels <= 0)
		return fail_msg("melpe_vad_host: bad arguments");
	const size_t n = (size_t) channels;
	/* an inactive channel keeps its votes: they go up too */
	Xfer x[] = {{state, nullptr, sizeof(VadState) * n, XFER_IN | XFER_OUT},
		    {sp, nullptr, sizeof(int16_t) * MELPE_SF_SAMPLES * n, XFER_IN},
		    {votes, nullptr, n, XFER_IN | XFER_OUT},
		    {active, nullptr, n, XFER_IN}};
	return stage_host_call("melpe_vad_host", x, 4, [&] {
		return melpe_vad_dev(x[0].dev, x[1].dev, x[2].dev, channels, x[3].dev, nullptr);
	});
}


int melpe_tx_dev(melpe_engine *e, void *d_vad_state, void *d_bits, void *d_sp, void *d_votes,
		 void *d_gate, const void *d_active, void *hip_stream)
{
	if (!e || !d_vad_state || !d_bits || !d_sp || !d_votes || !d_gate)
		return fail_msg("melpe_tx_dev: bad arguments");
	if (int rc = state_aligned("melpe_tx_dev", d_vad_state))
		return rc;
	DEVGUARD(e->device);
	if (int rc = vad_launch(d_vad_state, d_sp, d_votes, d_gate, d_active, e->channels, (hipStream_t) hip_stream))
		return rc;
	return melpe_encode_dev(e, d_bits, d_sp, d_gate, hip_stream);
}

/* the first half of melpe_tx_dev: the VAD gate and the NPP of the channels
 * it opens (the analysis follows in melpe_tx_pipe_dev or
 * melpe_encode_ana_dev with the gate as the mask) */
int melpe_tx_npp_dev(melpe_engine *e, void *d_vad_state, void *d_sp, void *d_votes, void *d_gate,
		     const void *d_active, void *hip_stream)
{
	if (!e || !d_vad_state || !d_sp || !d_votes || !d_gate)
		return fail_msg("melpe_tx_npp_dev: bad arguments");
	if (int rc = state_aligned("melpe_tx_npp_dev", d_vad_state))
		return rc;
	DEVGUARD(e->device);
	if (int rc = vad_launch(d_vad_state, d_sp, d_votes, d_gate, d_active, e->channels, (hipStream_t) hip_stream))
		return rc;
	return melpe_encode_npp_dev(e, d_sp, d_gate, hip_stream);
}

/* the TX front end pipelined like melpe_encode_pipe_dev: superframe k's
 * analysis on the engine stream (gated by d_gate, which melpe_tx_npp_dev or
 * the previous call wrote), and once its lane-order sort is done, on cin,
 * superframe k + 1's VAD (votes and gate out) and the NPP of the channels
 * it opens.  The VAD state is the VAD's alone, so a sequence tx_npp(0),
 * tx_pipe(0, 1), ..., tx_pipe(K-1, NULL) gives the bits, votes, gates and
 * NPP output of K melpe_tx_dev calls. */
int melpe_tx_pipe_dev(melpe_engine *e, void *d_vad_state, void *d_bits, const void *d_sp, const void *d_gate,
		      void *d_sp_next, void *d_votes_next, void *d_gate_next, const void *d_active_next,
		      void *hip_stream)
{
	if (!e || !d_vad_state || !d_bits || !d_sp || !d_gate ||
	    (d_sp_next && (!d_votes_next || !d_gate_next)))
		return fail_msg("melpe_tx_pipe_dev: bad arguments");
	if (int rc = state_aligned("melpe_tx_pipe_dev", d_vad_state))
		return rc;
	if (d_sp_next == d_sp || (d_sp_next && d_gate_next == d_gate))
		return fail_msg("melpe_tx_pipe_dev: the next superframe's buffers must be other buffers");
	const PipeNext nx = {d_sp_next, d_gate_next, d_vad_state, d_votes_next, d_active_next};
	return pipe_step(e, d_bits, d_sp, d_gate, d_sp_next ? &nx : nullptr, nullptr, (hipStream_t) hip_stream);
}


int melpe_stream_pack(const unsigned char *bits, const uint8_t *votes, uint8_t *last,
		      unsigned char *out, uint8_t *lens, int channels, const uint8_t *active)
{
	if (!bits || !votes || !last || !out || !lens || channels <= 0)
		return fail_msg("melpe_stream_pack: bad arguments");
	for (int c = 0; c < channels; c++) {
		const unsigned char *b = bits + (size_t) c * MELPE_SF_BYTES;
		unsigned char *o = out + (size_t) c * MELPE_SF_BYTES;
		lens[c] = (uint8_t) sfmt_frame_len(!active || active[c], votes[c]);
		if (lens[c])
			last[c] = sfmt_pack(b, votes[c], last[c], o);
	}
	return 0;
}

long melpe_stream_unpack(const unsigned char *stream, long nbytes, unsigned char *bits,
			 uint8_t *voiced, long max_sf)
{
	if (!stream || nbytes < 0 || !bits || !voiced || max_sf < 0)
		return fail_msg("melpe_stream_unpack: bad arguments");
	long pos = 0, k = 0;
	while (pos < nbytes && k < max_sf) {	/* melpe_dec.c:33-48 */
		unsigned char *b = bits + (size_t) k * MELPE_SF_BYTES;
		unsigned len = sfmt_rx_len(stream[pos], (unsigned long) (nbytes - pos));
		if (len == SFMT_TRUNCATED)
			return fail_msg("melpe_stream_unpack: truncated voiced frame");
		if (len == 1)
			memset(b, 0, MELPE_SF_BYTES);
		else
			sfmt_unswap(stream + pos, b);
		voiced[k++] = len != 1;
		pos += len;
	}
	return k;
}

long melpe_stream_pack_work_bytes(int channels)
{
	if (channels <= 0)
		return fail_msg("melpe_stream_pack_work_bytes: bad arguments");
	return (long) (sizeof(uint32_t) * kl_stream_pack_work_words(channels));
}

int melpe_stream_pack_dev(const void *d_bits, const void *d_votes, void *d_last, void *d_out,
			  void *d_offs, void *d_work, int channels, const void *d_active,
			  void *hip_stream)
{
	if (!d_bits || !d_votes || !d_last || !d_out || !d_offs || !d_work || channels <= 0)
		return fail_msg("melpe_stream_pack_dev: bad arguments");
	if (((uintptr_t) d_offs & 3) || ((uintptr_t) d_work & 3))
		return fail_msg("melpe_stream_pack_dev: offs and work must be 4-byte aligned");
	if ((long) channels * SFMT_BYTES > 0xffffffffL)
		return fail_msg("melpe_stream_pack_dev: the offsets of so many channels exceed 32 bits");
	if (int rc = kl_stream_pack((const unsigned char *) d_bits, (const uint8_t *) d_votes, (uint8_t *) d_last,
				    (unsigned char *) d_out, (uint32_t *) d_offs, (uint32_t *) d_work, channels,
				    (const uint8_t *) d_active, (hipStream_t) hip_stream))
		return fail("melpe_stream_pack_dev", (hipError_t) rc);
	return 0;
}

/* melpe_dec.c:33-49 on every channel: the parse (one lane per channel), the
 * zero fill of the silent channels' PCM, then the engine's decode with the
 * parse's `voiced` as its mask */
int melpe_rx_stream_dev(melpe_engine *e, const void *d_stream, const void *d_pos, const void *d_end,
			void *d_pos_next, void *d_sp, void *d_bits, void *d_voiced, void *d_lens,
			const void *d_active, void *hip_stream)
{
	if (!e || !d_stream || !d_pos || !d_end || !d_sp || !d_bits || !d_voiced || !d_lens)
		return fail_msg("melpe_rx_stream_dev: null argument");
	if (((uintptr_t) d_pos & 3) || ((uintptr_t) d_end & 3) || ((uintptr_t) d_pos_next & 3) ||
	    ((uintptr_t) d_sp & 7))
		return fail_msg("melpe_rx_stream_dev: pos, end and pos_next must be 4-byte and "
				"sp 8-byte aligned");
	const int n = e->channels;
	return engine_call(e, (hipStream_t) hip_stream, TIME_LAZY, [&](hipStream_t s) {
		if (int rc = kl_stream_parse((const unsigned char *) d_stream, (const uint32_t *) d_pos,
					     (const uint32_t *) d_end, (uint32_t *) d_pos_next, (unsigned char *) d_bits,
					     (uint8_t *) d_voiced, (uint8_t *) d_lens, (uint2 *) d_sp,
					     (const uint8_t *) d_active, n, s))
			return fail("melpe_rx_stream_dev", (hipError_t) rc);
		HIPCHK((hipError_t) dec_launch(e, (int16_t *) d_sp, src_bits(d_bits), (const uint8_t *) d_voiced, s));
		return 0;
	});
}

/* the receive loop (k_rx_line, rxline.h) */
int melpe_rx_line_state_bytes(void)
{
	return (int) sizeof(RxLineState);
}

int melpe_rx_line_private_bytes(void)
{
	return (int) kl_rx_line_private();
}

/* argument errors, refused before any HIP call */
static int rx_line_args(const char *who, const melpe_engine *e, const void *modem, const void *link,
			const void *rx, const void *pcm, long stride, const void *pos, const void *data,
			const void *sp, const void *bits, const void *voice, const void *info,
			const void *count, int calls, int slots, bool dev)
{
	const std::string w(who);
	if (calls <= 0 || stride < MODEM_LOOKAHEAD)
		return fail_msg(w + ": calls must be positive and stride at least one call's 1,080 samples");
	if (slots < calls / 15 + 2 || slots > 255)
		return fail_msg(w + ": slots must be at least calls / 15 + 2 (and at most 255)");
	if (!modem || !link || !rx)
		return fail_msg(w + ": null state pointer");
	if (!pcm || !pos || !data || !sp || !bits || !voice || !info || !count)
		return fail_msg(w + ": null buffer pointer");
	if (((uintptr_t) modem & 3) || ((uintptr_t) link & 3) || ((uintptr_t) rx & 3))
		return fail_msg(w + ": state records must be 4-byte aligned");
	if (dev && (((uintptr_t) sp & 7) || ((uintptr_t) pos & 3) || ((uintptr_t) info & 3) || ((uintptr_t) pcm & 1)))
		return fail_msg(w + ": sp must be 8-byte, pos and info 4-byte aligned");
	if (!e)
		return fail_msg(w + ": null engine");
	return 0;
}

int melpe_rx_line_dev(melpe_engine *e, void *d_modem_state, void *d_link_state, void *d_rx_state,
		      const void *d_pcm, long stride, void *d_pos, void *d_data, void *d_sp, void *d_bits,
		      void *d_voice, void *d_info, void *d_count, int calls, int slots, const void *d_active,
		      void *hip_stream)
{
	if (int rc = rx_line_args("melpe_rx_line_dev", e, d_modem_state, d_link_state, d_rx_state, d_pcm, stride,
				  d_pos, d_data, d_sp, d_bits, d_voice, d_info, d_count, calls, slots, true))
		return rc;
	const int n = e->channels;
	const uint8_t *act = (const uint8_t *) d_active, *voice = (const uint8_t *) d_voice;
	const uint8_t *count = (const uint8_t *) d_count;
	return engine_call(e, (hipStream_t) hip_stream, TIME_LAZY, [&](hipStream_t s) {
		if (int rc = kl_rx_line((ModemState *) d_modem_state, (LinkState *) d_link_state,
					(RxLineState *) d_rx_state, (const int16_t *) d_pcm, stride, (int32_t *) d_pos,
					(uint8_t *) d_data, (uint2 *) d_sp, (uint8_t *) d_bits, (uint8_t *) d_voice,
					(uint32_t *) d_info, (uint8_t *) d_count, n, calls, slots, act, s))
			return fail("melpe_rx_line_dev", (hipError_t) rc);
		/* slot by slot, as the channel's decoder state carries from block to block */
		for (int j = 0; j < slots; j++) {
			if (int rc = kl_rx_line_mask(e->d_rxmask, voice, count, act, n, j, s))
				return fail("melpe_rx_line_dev", (hipError_t) rc);
			HIPCHK((hipError_t) dec_launch(e, (int16_t *) d_sp + (size_t) j * n * MELPE_SF_SAMPLES,
						       src_bits((const uint8_t *) d_bits + (size_t) j * n * MELPE_SF_BYTES),
						       e->d_rxmask, s));
		}
		return 0;
	});
}

/* host buffers: one staged upload per tensor (outputs too, so that rows the
 * call does not write keep the caller's bytes), the same launches, and back */
int melpe_rx_line_host(melpe_engine *e, void *modem_state, void *link_state, void *rx_state, const int16_t *pcm,
		       long stride, int32_t *pos, uint8_t *data, int16_t *sp, unsigned char *bits, uint8_t *voice,
		       uint8_t *info, uint8_t *count, int calls, int slots, const uint8_t *active)
{
	if (int rc = rx_line_args("melpe_rx_line_host", e, modem_state, link_state, rx_state, pcm, stride, pos, data,
				  sp, bits, voice, info, count, calls, slots, false))
		return rc;
	DEVGUARD(e->device);
	const size_t n = (size_t) e->channels, rows = n * (size_t) slots;
	/* sp first: the stage buffer's start is its only 8-byte aligned part */
	Xfer x[] = {{sp, nullptr, rows * MELPE_SF_SAMPLES * sizeof(int16_t), XFER_IN | XFER_OUT},
		    {modem_state, nullptr, n * sizeof(ModemState), XFER_IN | XFER_OUT},
		    {link_state, nullptr, n * LINK_STATE_BYTES, XFER_IN | XFER_OUT},
		    {rx_state, nullptr, n * sizeof(RxLineState), XFER_IN | XFER_OUT},
		    {pos, nullptr, n * sizeof(int32_t), XFER_IN | XFER_OUT},
		    {info, nullptr, rows * RXL_INFO_BYTES, XFER_IN | XFER_OUT},
		    {pcm, nullptr, n * (size_t) stride * sizeof(int16_t), XFER_IN},
		    {data, nullptr, n * 12, XFER_IN | XFER_OUT},
		    {bits, nullptr, rows * MELPE_SF_BYTES, XFER_IN | XFER_OUT},
		    {voice, nullptr, rows, XFER_IN | XFER_OUT},
		    {count, nullptr, n, XFER_IN | XFER_OUT},
		    {active, nullptr, n, XFER_IN}};
	return stage_host_call("melpe_rx_line_host", x, 12, [&] {
		return melpe_rx_line_dev(e, x[1].dev, x[2].dev, x[3].dev, x[6].dev, stride, x[4].dev, x[7].dev,
					 x[0].dev, x[8].dev, x[9].dev, x[5].dev, x[10].dev, calls, slots, x[11].dev,
					 nullptr);
	});
}

}  // extern "C"
