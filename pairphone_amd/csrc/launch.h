/*
 * launch.h -- the one declaration of everything engine.hip calls in the
 * kernel translation units: each table-carrying TU's table upload and
 * stage-timer readout (kern.h MELPE_TU) and the kl_* launchers defined next
 * to the kernels.  engine.hip holds no device code: every kernel it runs is
 * reached through one of these.  engine.hip includes this header and so does
 * the TU that defines each function (through kern.h, or directly), so a
 * definition that disagrees with its declaration fails to compile instead of
 * linking silently.
 *
 * Only pointers to the record types appear here, so the header names them
 * and leaves their definitions to state.h, kern.h, link.h, vad.h, modem.h,
 * rxline.h and synth.h.
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
struct VadState;
struct ModemState;
struct RxLineState;
struct synth_state;

/* the translation units that carry their own copy of the constant tables:
 * MELPE_TU(name) in the TU's .hip is the one definition site, this list the
 * one place that names them all (tests/test_abi.py holds the two equal) */
#define MELPE_TU_LIST(X) X(npp) X(ana) X(quant) X(anamw) X(harm) X(dec) X(r24) X(dspeval) X(anaeval) X(par)

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
/* the basic operators (ops_eval.h) and the stream / correlator helpers
 * (helpers_eval.h) */
int kl_ops_eval(int op, const int64_t *a, const int32_t *b, const int32_t *c, int64_t *out, long n,
		hipStream_t s);
int kl_divide_s_sweep(uint64_t *digest, hipStream_t s);
int kl_helpers_eval(int mode, const int16_t *src, const int32_t *args, int32_t *out, int n, hipStream_t s);

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

/* k_line.hip: the line side -- voice crypt, VAD, the stream format, the
 * modem and the receive loop.  Kernels that always run together share a
 * launcher: the pack's three scan passes (work: kl_stream_pack_work_words
 * dwords), the parse and the zero fill of the silent channels' rows of sp,
 * Modulate and its state update, the receive loop and the zero fill of the
 * slots that hold no voice. */
int kl_voice_crypt(unsigned char *pkts, const uint32_t *counters, const uint4 *keys, const uint8_t *invert,
		   int channels, int packets, int dir, hipStream_t s);
int kl_vad(VadState *st, const int16_t *sp, uint8_t *votes, uint8_t *gate, const uint8_t *active, int channels,
	   hipStream_t s);
int kl_vad_reset(VadState *st, const uint8_t *mask, int channels, hipStream_t s);
size_t kl_stream_pack_work_words(int channels);
int kl_stream_pack(const unsigned char *bits, const uint8_t *votes, uint8_t *last, unsigned char *out,
		   uint32_t *offs, uint32_t *work, int channels, const uint8_t *active, hipStream_t s);
int kl_stream_parse(const unsigned char *stream, const uint32_t *pos, const uint32_t *end, uint32_t *pos_next,
		    unsigned char *bits, uint8_t *voiced, uint8_t *lens, uint2 *sp, const uint8_t *active,
		    int channels, hipStream_t s);
int kl_modem_reset(ModemState *st, const uint8_t *mask, int channels, hipStream_t s);
int kl_modulate(ModemState *st, const uint8_t *pkts, int16_t *pcm, int channels, int packets,
		const uint8_t *active, hipStream_t s);
int kl_demodulate(ModemState *st, const int16_t *pcm, long stride, int32_t *pos, uint8_t *data, uint8_t *out,
		  int32_t *ret, int channels, int calls, const uint8_t *active, hipStream_t s);
int kl_rx_line(ModemState *st, LinkState *lk, RxLineState *rx, const int16_t *pcm, long stride, int32_t *pos,
	       uint8_t *data, uint2 *sp, uint8_t *bits, uint8_t *voice, uint32_t *info, uint8_t *count,
	       int channels, int calls, int slots, const uint8_t *active, hipStream_t s);
int kl_rx_line_mask(uint8_t *mask, const uint8_t *voice, const uint8_t *count, const uint8_t *active,
		    int channels, int j, hipStream_t s);
size_t kl_rx_line_private(void);

/* k_state.hip: the engine's own kernels on the channel records */
int kl_reset(mlp::EncState *enc, mlp::DecState *dec, const uint8_t *mask, int n, int which, hipStream_t s);
int kl_melpe_i(mlp::EncState *enc, mlp::DecState *dec, hipStream_t s);
int kl_share_params(mlp::EncState *enc, mlp::DecState *dec, int dir, hipStream_t s);
int kl_synth_seed(synth_state *syn, uint32_t seed, uint32_t ch0, int n, hipStream_t s);
int kl_synth(synth_state *syn, int16_t *out, int samples, int n, hipStream_t s);
/* the lane-order sort: the live channels of `rec` (records of `stride`
 * bytes) counted, scanned and scattered into b.perm by the class that `key`
 * gives them.  The three kernels take the engine's BinBuf by value and use
 * its device pointers; the event and stream fields are engine.hip's host
 * bookkeeping (bin_prepare / bin_release). */
#define NBIN 640	/* room for the 4 x 142 = 568 pitch classes (progprio.h and AnaGate index past it) */
#define KEY_PITCH 0	/* the record's previous superframe: voiced frames x last pitch */
#define KEY_VOICING 1	/* the voicing pattern k_enc_ana's sc_ana left in par[0..2] */
#define KEY_ROWS 2	/* a tensor of parameter rows: voiced frames x the last frame's pitch */
struct BinBuf {
	int *perm = nullptr;	/* [C] lane -> channel */
	uint16_t *key = nullptr;	/* [C] class of each channel (NOT_LIVE: not live) */
	/* [0, NBIN) counts, [NBIN, 2 NBIN) next slot of each class, [2 NBIN]
	 * the live count, [2 NBIN + 1] the mapping the last analysis launch ran
	 * (AnaGate tag: 1 lane, 4 four-wave; 0 none yet), [2 NBIN + 2] the
	 * launch's progress counter (k_ana.hip ana_ckpt) */
	unsigned *ctl = nullptr;
	/* The buffers are one per engine and direction, but *_dev calls may
	 * come on different streams: the sort of a call waits for the kernel
	 * that read the previous call's order (its stream recorded `done`). */
	hipEvent_t done = nullptr;
	hipStream_t last = nullptr;
	bool used = false;
};
int kl_bin_sort(int key, const char *rec, size_t stride, int off_par, int off_uv, const uint8_t *active, int n,
		BinBuf b, hipStream_t s);

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
