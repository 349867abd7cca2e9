/*
 * launch.h -- the one declaration of everything engine.hip calls in the
 * kernel translation units: each TU's table upload and stage-timer readout
 * (kern.h MELPE_TU) and the kl_* launchers defined next to the kernels.
 * engine.hip includes it and so does the TU that defines each function (the
 * codec TUs through kern.h), so a definition that disagrees with its
 * declaration fails to compile instead of linking silently.
 *
 * Only pointers to the record types appear here, so the header names them
 * and leaves their definitions to state.h, kern.h and link.h.
 */
#ifndef MELPE_LAUNCH_H
#define MELPE_LAUNCH_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace mlp {
struct EncState;
struct DecState;
}
struct AnaGate;
struct LinkState;

/* the translation units that carry their own copy of the constant tables:
 * MELPE_TU(name) in the TU's .hip is the one definition site, this list the
 * one place that names them all (tests/test_abi.py holds the two equal) */
#define MELPE_TU_LIST(X) X(eng) X(npp) X(ana) X(quant) X(anamw) X(harm) X(dec) X(r24) X(dspeval) X(anaeval) X(par)

extern "C" {

#define MELPE_TU_DECL(name)                                      \
	int melpe_tu_##name##_upload(const void *blob, size_t bytes); \
	int melpe_tu_##name##_prof(uint64_t *acc);
MELPE_TU_LIST(MELPE_TU_DECL)
#undef MELPE_TU_DECL

/* k_npp.hip */
int kl_npp(mlp::EncState *enc, int16_t *sp, int frames, int stride, const uint8_t *active, int n,
	   int rate1200, hipStream_t s);
int kl_enc_npp(mlp::EncState *enc, int16_t *sp, const uint8_t *active, int n, hipStream_t s);
int kl_dsp_scalar_lds(int mode, const int32_t *args, int32_t *out, long n, hipStream_t s);
int kl_dsp_wave_fft(int mode, const int16_t *in, const int32_t *args, int32_t *out, int n, hipStream_t s);

/* k_ana.hip: the lane analysis up to sc_ana; res receives the speech span
 * the quantisers' residuals are made from */
int kl_enc_ana(mlp::EncState *enc, const int16_t *sp, const uint8_t *active, int n, const int *perm,
	       const int *nlive, int16_t *res, AnaGate gate, hipStream_t s);
int kl_enc_ana_dbg(mlp::EncState *enc, const int16_t *sp, int n, int upto, hipStream_t s);

/* k_quant.hip: the quantisers after sc_ana; res in (the span), out (each
 * voiced frame's windowed residual) */
int kl_enc_quant(mlp::EncState *enc, int16_t *res, const uint8_t *active, int n, const int *perm,
		 const int *nlive, AnaGate gate, hipStream_t s);

/* k_harm.hip */
int kl_enc_harm(mlp::EncState *enc, const int16_t *res, const uint8_t *active, int n, const int *perm,
		const int *nlive, AnaGate gate, hipStream_t s);
int kl_enc_tail(mlp::EncState *enc, uint8_t *bits, const uint8_t *active, int n, const int *perm,
		const int *nlive, AnaGate gate, hipStream_t s);
int kl_dsp_wave_harm(const int16_t *in, const int32_t *args, int32_t *out, int n, hipStream_t s);

/* k_ana_mw.hip */
int kl_enc_ana_mw(mlp::EncState *enc, const int16_t *sp, uint8_t *bits, const uint8_t *active, int n,
		  const int *perm, const int *nlive, uint32_t *lqbuf, AnaGate gate, hipStream_t s);
size_t kl_enc_ana_mw_lq_words(int n);

/* k_dec.hip: the decoder family.  The source of a superframe's parameters
 * is the channel words (rows 0: in = bits, C x 11) or a tensor of parameter
 * rows (rows 1: in = C x 3 x 30 int16, read only; status: C bytes or null).
 * kl_dec runs it with `waves` waves per 64 channels: 1, a lane per channel
 * (k_decode / k_synth_par), or 2 (k_decode2 / k_synth_par2, through hbuf:
 * kl_dec2_hb_words(n) dwords, whichever the source). */
struct DecSrc {
	int rows;
	const void *in;
	uint8_t *status;
};
int kl_dec(int waves, DecSrc src, mlp::DecState *dec, int16_t *sp, const uint8_t *active, int n,
	   const int *perm, const int *nlive, uint32_t *hbuf, hipStream_t s);
size_t kl_dec2_hb_words(int n);

/* k_r24.hip */
int kl_enc24(mlp::EncState *enc, const int16_t *sp, uint8_t *bits, const uint8_t *active, int n,
	     hipStream_t s);
int kl_dec24(mlp::DecState *dec, int16_t *sp, const uint8_t *bits, const uint8_t *active, int n,
	     hipStream_t s);

/* k_dsp_eval.hip: the function-level parity test (dsp_eval.h), lane and
 * blob-table scalar modes; the wave forms are next to the code they test */
int kl_dsp_eval(int mode, const int16_t *in, const int32_t *args, int32_t *out, int n, hipStream_t s);
int kl_dsp_scalar(int mode, const int32_t *args, int32_t *out, long n, hipStream_t s);

/* k_ana_eval.hip: the function-level parity test of the pitch and voicing
 * analysis (ana_eval.h) */
int kl_ana_eval(int mode, const int16_t *in, const int32_t *args, int32_t *out, int n, hipStream_t s);
int kl_ana_scalar(int mode, const int32_t *args, int32_t *out, long n, hipStream_t s);

/* k_par.hip: the parameter tap (rec + c * stride + off is channel c's
 * par[0]) and the parse-only decoder, rows as dwords */
int kl_par_tap(const char *rec, size_t stride, size_t off, uint32_t *par, uint32_t *qpar,
	       const uint8_t *active, int n, hipStream_t s);
int kl_parse(mlp::DecState *dec, uint32_t *par, const uint8_t *bits, const uint8_t *active, int n,
	     hipStream_t s);

/* k_link.hip: the link's packet layer and the Golay sweep */
int kl_link_tx(LinkState *st, uint8_t *pkts, const uint8_t *voiced, int32_t *ret, const uint8_t *active,
	       int channels, int packets, hipStream_t s);
int kl_link_rx(LinkState *st, uint8_t *pkts, int32_t *ret, uint8_t *voice, const uint8_t *active,
	       int channels, int packets, hipStream_t s);
int kl_golay_sweep(uint32_t *enc, uint64_t *digest, hipStream_t s);

/* Scratch reservation (engine.hip engine_reserve / engine_warm): a kernel's
 * private-segment bytes per lane, and its warm-up -- the real launch over n
 * channels with null pointers and no live channel, so that every lane exits
 * at once and the runtime reserves what the real launch will need. */
size_t kl_npp_private(void);
size_t kl_ana_private(void);
size_t kl_quant_private(void);
size_t kl_harm_private(void);	/* k_enc_tail, lane per channel */
size_t kl_harm_wave_private(void);	/* k_enc_harm, wave per channel */
size_t kl_ana_mw_private(void);
size_t kl_dec_private(int waves, int rows);	/* the decoder family's kernel for (waves, DecSrc.rows) */
size_t kl_parse_private(void);
int kl_npp_warm(int n, hipStream_t s);
int kl_ana_warm(int n, hipStream_t s);
int kl_quant_warm(int n, hipStream_t s);
int kl_harm_warm(int n, hipStream_t s);
int kl_ana_mw_warm(int n, hipStream_t s);
int kl_dec_warm(int waves, int rows, int n, hipStream_t s);

}

#endif
