/*
 * k_ana.hip -- the analysis half of melpe_a (melpe/melpe.c:97-98:
 * analysis() + the 11-byte frame): dc removal, melp_ana per frame and
 * sc_ana, one lane per channel, reading the NPP output k_enc_npp left in the
 * caller's PCM.  The quantisers are in k_quant.hip, the Fourier magnitudes
 * and the channel packing in k_harm.hip.
 */
#define MELPE_PROG_PRIO	/* progprio.h: ANA_CKPT */
#include "kern.h"

MELPE_TU(ana)

/* the lane's frame: the analysis state only (not the NPP state), whose
 * live prefix moves in and out (state.h ENC_ANA_LIVE), and the PCM block */
struct AnaLane {
	uint8_t guard[FLAT_GUARD_BYTES];
	EncAna S;
	int16_t x[BLOCK];
};

#if defined(MELPE_WAVE_TIMES)
/* diagnostics (tools/wave_times.py): each wave's start and end on the
 * chip-wide 100 MHz counter, to see how the launch's waves finish */
__device__ unsigned long long g_wave_t[2 * 16384];
/* the wave's placement: HW_ID (wave, SIMD, CU, SH, SE) and XCC_ID */
__device__ unsigned g_wave_hw[2 * 16384];
extern "C" int kl_wave_times(unsigned long long *out, int n)
{
	return (int) hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wave_t), sizeof(unsigned long long) * n);
}
extern "C" int kl_wave_hw(unsigned *out, int n)
{
	return (int) hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wave_hw), sizeof(unsigned) * n);
}
#define WT_START() const unsigned long long wt0_ = __builtin_amdgcn_s_memrealtime()
#define WT_END()                                                                         \
	do {                                                                             \
		if (threadIdx.x == 0 && blockIdx.x < 16384) {                            \
			g_wave_t[2 * blockIdx.x] = wt0_;                                 \
			g_wave_t[2 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime(); \
			g_wave_hw[2 * blockIdx.x] = __builtin_amdgcn_s_getreg((31 << 11) | 4);  \
			g_wave_hw[2 * blockIdx.x + 1] = __builtin_amdgcn_s_getreg((31 << 11) | 20); \
		}                                                                        \
	} while (0)
#else
#define WT_START() (void) 0
#define WT_END() (void) 0
#endif

/* The split form of the analysis (encoder.h analysis_a1): the three frames
 * and sc_ana.  The quantisers that follow branch on the voicing pattern
 * sc_ana leaves, so they run in a kernel of their own (k_quant.hip) on waves
 * sorted by that pattern; the residuals they make come from speech the
 * history shift drops, so that span goes out to the channel's row of res
 * first, from every lane alike.  The Fourier magnitudes and the packing,
 * which writes the bits, are in k_harm.hip.
 * MODE is a name tag only: the profiles and the tools that read them key on
 * the symbol k_enc_ana<1>.  `bits` is unused and keeps the argument layout. */
template <int MODE>
__global__ __launch_bounds__(WAVE, MELPE_ENC_WAVES) void k_enc_ana(EncState *enc, const int16_t *sp, uint8_t *bits,
						  const uint8_t *active, int n, const int *perm,
						  const int *nlive, int16_t *res, AnaGate gate, int prio)
{
	static_assert(MODE == 1, "the unsplit analysis (MODE 0) is gone");
	/* lane g runs channel perm[g] when the engine ordered the live channels
	 * by pitch class (engine.hip, MELPE_BIN), else channel g under the mask;
	 * the whole launch stands down unless the live count is the gate's
	 * (engine.hip ana_launch enqueues this and the four-wave kernel) */
	WT_START();
	int c = blockIdx.x * WAVE + threadIdx.x;
	if (perm) {
		const int L = *nlive;
		if (!gate.open(L))
			return;
		gate.mark(c == 0 && L > 0, 1);	/* no live channel: the tag stays 0 */
		if (c >= L)
			return;
		/* progprio.h: the counter is the sort's control word nlive[2] */
		PP_BEGIN(prio ? (unsigned *) (nlive + 2) : nullptr, (L + WAVE - 1) / WAVE);
		c = perm[c];
	} else {
		PP_BEGIN(nullptr, 1);
		gate.mark(c == 0, 1);
		if (c >= n || (active && !active[c]))
			return;
	}
	AnaLane L;
	PIN_FRAME(L);
	constexpr size_t nb = ENC_ANA_LIVE;
	static_assert(offsetof(AnaLane, S) % 16 == 0, "the record copy is in 16-byte pieces");
	static_assert((offsetof(AnaLane, S) + offsetof(EncAna, hpspeech) + sizeof(int16_t) * ANA_XSPAN_BEG) % 16 == 0,
		      "and so is the span copy");
	lane_copy_x4(&L.S, &enc[c].a, nb);
	lane_copy(L.x, sp + (size_t) c * BLOCK, sizeof(int16_t) * BLOCK);
	analysis_a1(&L.S, L.x);
	lane_copy_x4(res + (size_t) c * NF * LPC_FRAME, &L.S.hpspeech[ANA_XSPAN_BEG], ANA_XSPAN_BYTES);
	ana_shift(&L.S);
	lane_copy_x4(&enc[c].a, &L.S, nb);
	WT_END();
}

/* debug aid: analysis cut after `upto` stages (0 = nothing) */
__global__ __launch_bounds__(WAVE, MELPE_ENC_WAVES) void k_enc_ana_dbg(EncState *enc, const int16_t *sp, int n, int upto)
{
	int c = blockIdx.x * WAVE + threadIdx.x;
	PP_BEGIN(nullptr, 1);
	if (c >= n || upto <= 0)
		return;
	AnaLane L;
	PIN_FRAME(L);
	lane_copy(&L.S, &enc[c].a, ENC_ANA_LIVE);
	lane_copy(L.x, sp + (size_t) c * BLOCK, sizeof(int16_t) * BLOCK);
	analysis_upto(&L.S, L.x, upto);
	lane_copy(&enc[c].a, &L.S, ENC_ANA_LIVE);
}

/* MELPE_ANA_PRIO=0: no progress-driven priority (progprio.h), for A/Bs */
static int ana_prio_mode(void)
{
	static const int v = env_int("MELPE_ANA_PRIO", 1) != 0;
	return v;
}

/* the launch of k_enc_ana<1>, a lane per channel over `lanes` channels: the
 * real one (n = lanes) and the warm-up (n = 0: every lane exits at once) */
static int launch_ana(int lanes, EncState *enc, const int16_t *sp, const uint8_t *active, int n, const int *perm,
		      const int *nlive, int16_t *res, AnaGate gate, int prio, hipStream_t s)
{
	k_enc_ana<1><<<grid_for(lanes), WAVE, 0, s>>>(enc, sp, nullptr, active, n, perm, nlive, res, gate, prio);
	return (int) hipGetLastError();
}

extern "C" int kl_enc_ana(EncState *enc, const int16_t *sp, const uint8_t *active, int n, const int *perm,
			  const int *nlive, int16_t *res, AnaGate gate, hipStream_t s)
{
	return launch_ana(n, enc, sp, active, n, perm, nlive, res, gate, ana_prio_mode(), s);
}

extern "C" int kl_enc_ana_dbg(EncState *enc, const int16_t *sp, int n, int upto, hipStream_t s)
{
	k_enc_ana_dbg<<<grid_for(n), WAVE, 0, s>>>(enc, sp, n, upto);
	return (int) hipGetLastError();
}

/* the larger of the two analysis kernels: melpe_debug_encode_stage runs
 * k_enc_ana_dbg on the engine stream too, and its frame is the larger */
extern "C" size_t kl_ana_private(void)
{
	const size_t x = private_bytes((const void *) k_enc_ana<1>), y = private_bytes((const void *) k_enc_ana_dbg);
	return x > y ? x : y;
}

extern "C" int kl_ana_warm(int n, hipStream_t s)
{
	return launch_ana(n, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, AnaGate{}, 0, s);
}
