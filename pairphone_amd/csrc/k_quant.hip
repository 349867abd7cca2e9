/*
 * k_quant.hip -- the quantisers of melpe_a between sc_ana and the Fourier
 * magnitudes (melpe/melp_ana.c:164-233: lsf_vq, pitch_vq, gain_vq, the
 * jitter and bandpass quantisers, and the last voiced frame's windowed
 * residual of the quantised LSFs), one lane per channel.
 *
 * lsf_vq branches on the superframe's voicing pattern, and a wave pays the
 * union of its lanes' branches: every codebook scan runs once per distinct
 * codebook among the 64 lanes.  The pattern exists only after sc_ana, so the
 * lane analysis stops there (k_ana.hip), the engine sorts the live channels
 * by the pattern (engine.hip, the second lane order), and this kernel runs
 * with waves of one pattern each.  Each channel's arithmetic is analysis_q's
 * (encoder.h), the same statements the unsplit analysis runs.
 */
#include "kern.h"

MELPE_TU(quant)

/* minimum resident waves per SIMD k_enc_quant is compiled for: one wave per
 * 64 channels, four per SIMD at 262,144 channels, as the lane analysis */
#ifndef MELPE_QUANT_WAVES
#define MELPE_QUANT_WAVES 4
#endif

/* the lane's frame: the record's layout, of which only the ranges below and
 * the residual span of hpspeech are filled, and sigbuf as working storage */
struct QuantLane {
	uint8_t guard[FLAT_GUARD_BYTES];
	EncAna S;
};

/* res: the channel's row of NF x LPC_FRAME samples.  In: the pre-shift
 * speech span k_enc_ana exported at its start (ANA_XSPAN_*).  Out: the
 * last voiced frame's windowed residual at last * LPC_FRAME, for k_enc_harm.
 * The rows overlap the span, so the span is taken into the lane's frame
 * whole before analysis_q writes its row. */
__global__ __launch_bounds__(WAVE, MELPE_QUANT_WAVES) void k_enc_quant(EncState *enc, int16_t *res,
									const uint8_t *active, int n,
									const int *perm, const int *nlive,
									AnaGate gate)
{
	int c = blockIdx.x * WAVE + threadIdx.x;
	if (perm) {
		const int L = *nlive;
		if (!gate.open(L) || c >= L)
			return;
		c = perm[c];
	} else if (c >= n || (active && !active[c])) {
		return;
	}
	QuantLane L;
	PIN_FRAME(L);
	/* par + qpar, and pvq_prev_uv_flag .. qplsp, widened to dwords (the
	 * extra int16 at either end goes back unchanged) */
	constexpr size_t o = offsetof(EncAna, par), e = offsetof(EncAna, voicedEn);
	constexpr size_t o2 = offsetof(EncAna, pvq_prev_uv_flag) & ~(size_t) 3;
	constexpr size_t e2 = (offsetof(EncAna, fsm_prev_uv) + 3) & ~(size_t) 3;
	static_assert(o % 4 == 0 && e % 4 == 0, "the quantisers' record ranges are dword copies");
	static_assert((offsetof(QuantLane, S) + offsetof(EncAna, hpspeech) + sizeof(int16_t) * ANA_XSPAN_BEG) % 16 == 0 &&
			      ANA_XSPAN_BYTES % 16 == 0,
		      "the span copy is in 16-byte pieces");
	EncAna *R = &enc[c].a;
	int16_t *row = res + (size_t) c * NF * LPC_FRAME;
	lane_copy((char *) &L.S + o, (const char *) R + o, e - o);
	lane_copy((char *) &L.S + o2, (const char *) R + o2, e2 - o2);
	lane_copy_x4(&L.S.hpspeech[ANA_XSPAN_BEG], row, ANA_XSPAN_BYTES);
	analysis_q(&L.S, row);
	lane_copy((char *) R + o, (const char *) &L.S + o, e - o);
	lane_copy((char *) R + o2, (const char *) &L.S + o2, e2 - o2);
}

/* the launch of k_enc_quant, a lane per channel over `lanes` channels (real:
 * n = lanes; warm-up: n = 0, every lane exits at once) */
static int launch_quant(int lanes, EncState *enc, int16_t *res, const uint8_t *active, int n,
			const int *perm, const int *nlive, AnaGate gate, hipStream_t s)
{
	k_enc_quant<<<grid_for(lanes), WAVE, 0, s>>>(enc, res, active, n, perm, nlive, gate);
	return (int) hipGetLastError();
}

extern "C" int kl_enc_quant(EncState *enc, int16_t *res, const uint8_t *active, int n, const int *perm,
			    const int *nlive, AnaGate gate, hipStream_t s)
{
	return launch_quant(n, enc, res, active, n, perm, nlive, gate, s);
}

extern "C" size_t kl_quant_private(void)
{
	return private_bytes((const void *) k_enc_quant);
}

extern "C" int kl_quant_warm(int n, hipStream_t s)
{
	return launch_quant(n, nullptr, nullptr, nullptr, 0, nullptr, nullptr, AnaGate{}, s);
}
