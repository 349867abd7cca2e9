/*
 * dsp_eval_modes.h -- the mode list and case layout of the function-level
 * parity test of the DSP and math library (dsp_eval.h).  Plain preprocessor
 * text: the device kernels, the host build, the checker (oracle/ref_dsp.c,
 * a C program) and tests/test_device_dsp.py (which parses the two lists)
 * all read the ids from here.
 *
 * Vector modes: one case is a row of DE_IN int16 (`b`: coefficients, filter
 * memories, and the signal with its history, at the offsets the arguments
 * give), DE_ARGS int32 arguments (`a`) and DE_OUT int32 results: the return
 * values in o[0 .. DE_RET) and then the whole row as the call left it, so
 * everything the function writes -- and anything it should not have
 * written -- is compared.
 *
 *   b[0 .. DE_DATA)        coefficients and memories (per mode, below)
 *   b[DE_DATA .. DE_IN)    signals, at offsets taken from the arguments
 *
 * Scalar modes: one case is four int32 arguments and one int32 result.
 */
#ifndef MELPE_DSP_EVAL_MODES_H
#define MELPE_DSP_EVAL_MODES_H

#define DE_IN 1168	/* int16 per case */
#define DE_ARGS 8	/* int32 per case */
#define DE_RET 8	/* return values in front of the row dump */
#define DE_OUT (DE_RET + DE_IN)	/* int32 per case */
#define DE_DATA 128	/* first int16 of the signal area */

/* X(id, name).  Arguments a[0..7], row b; offsets are int16 indices into b.
 *
 *  0 L_v_inner   (b+a0, b+a1, n=a2, qa=a3, qb=a4, qout=a5) -> o[0]
 *  1 L_v_magsq   (b+a0, n=a2, qa=a3, qout=a5) -> o[0]
 *  2 zerflt_Q    in=b+a0 (history b[a0-order .. a0)), coeff=b[0..order],
 *                out=b+a1, order=a2, n=a3, qc=a4
 *  3 iir_2nd_s   in=b+a0, out=b+a1, n=a2; den=b[0..3) num=b[3..6)
 *                din=b[6..8) dout=b[8..10)
 *  4 iir_2nd_d   the same; din=b[6..8) dhi=b[8..10) dlo=b[10..12)
 *  5 iir3_s      x=b+a0 in place, n=a2, snap=a3; den=b[0..9) num=b[9..18)
 *                din=b[18..24) dout=b[24..30)
 *  6 iir3_s_io   in=b+a0, out=b+a1, n=a2, same tables; every f(i, y) is
 *                stored at b[a3 + i]
 *  7 iir3_d      in=b+a0, out=b+a1, n=a2; den=b[0..9) num=b[9..18)
 *                din=b[18..24) dhi=b[24..30) dlo=b[30..36)
 *  8 iir3_d_batched  the same (a0 even, n a multiple of 36)
 *  9 iir2_d      x=b+a0 in place, n=a2; filter 1 den=b[0..3) num=b[3..6)
 *                din=b[6..8) dhi=b[8..10) dlo=b[10..12); filter 2 the same
 *                at b[12..24)
 * 10 envelope    in=b+a0, out=b+a1 (history b[a1-2], b[a1-1]), n=a2,
 *                prev_in=a3
 * 11 envelope_e  the same, lsh=a4; energy -> o[0] (low), o[1] (high)
 * 12 lpc_syn     x=b+a0, y=b+a1 (memory b[a1-order .. a1)), a=b[0..order),
 *                order=a2, n=a3
 * 13 cfft        256 complex points at b[DE_DATA ..), halvings -> o[0]
 * 14 fft_npp     the same, dir=a0
 * 15 rfft        512 real points at b[DE_DATA ..), 1024 shorts out
 * 16 rfft_pk     the same through the packed form (the input's max |x|
 *                taken as find_harm_fft takes it)
 * 17 find_harm   in=b+a0, len=a1, pitch=a2, fsmag=b[0..NUM_HARM)
 * 18 lpc_acor    in=b+a0, win=b+a1, r=b[0..order], order=a2, n=a3,
 *                hf_corr=a4
 * 19 lpc_schr    r=b[0..10], lpc=b[16..26), alpha -> o[0]
 * 20 lpc_pred2lsp  lpc=b[0..10), lsf=b[16..26)
 * 21 lpc_lsp2pred  lsf=b[0..10) (clamped in place), lpc=b[16..26)
 * 22 lsp2pred10  lsf_sort10 + lsp2pred10, the same layout
 * 23 lpc_clmp    lsp=b[0..order), delta=a0, order=a1
 * 24 lpc_pred2refl  lpc=b[0..10), energy -> o[0], *refc -> o[1]
 */
#define DE_MODES(X) \
	X(0, L_v_inner) X(1, L_v_magsq) X(2, zerflt_Q) X(3, iir_2nd_s) X(4, iir_2nd_d) \
	X(5, iir3_s) X(6, iir3_s_io) X(7, iir3_d) X(8, iir3_d_batched) X(9, iir2_d) \
	X(10, envelope) X(11, envelope_e) X(12, lpc_syn) X(13, cfft) X(14, fft_npp) \
	X(15, rfft) X(16, rfft_pk) X(17, find_harm) X(18, lpc_acor) X(19, lpc_schr) \
	X(20, lpc_pred2lsp) X(21, lpc_lsp2pred) X(22, lsp2pred10) X(23, lpc_clmp) \
	X(24, lpc_pred2refl)
#define DE_MODE_COUNT 25

/* S(id, name, call on int32 a, b, c, d) */
#define DE_SCALAR_MODES(S) \
	S(0, log10_fxp, log10_fxp((int16_t) a, (int16_t) b)) \
	S(1, pow10_fxp, pow10_fxp((int16_t) a, (int16_t) b)) \
	S(2, sqrt_fxp, sqrt_fxp((int16_t) a, (int16_t) b)) \
	S(3, L_log10_fxp, L_log10_fxp(a, (int16_t) b)) \
	S(4, L_sqrt_fxp, L_sqrt_fxp(a, (int16_t) b)) \
	S(5, L_pow_fxp, L_pow_fxp(a, (int16_t) b, (int16_t) c, (int16_t) d)) \
	S(6, sin_fxp, sin_fxp((int16_t) a)) \
	S(7, cos_fxp, cos_fxp((int16_t) a)) \
	S(8, sqrt_Q15, sqrt_Q15((int16_t) a)) \
	S(9, add_shr, add_shr((int16_t) a, (int16_t) b)) \
	S(10, interp_scalar, interp_scalar((int16_t) a, (int16_t) b, (int16_t) c)) \
	S(11, L_divider2, L_divider2(a, b, (int16_t) c, (int16_t) d))
#define DE_SCALAR_COUNT 12
/* modes 0 .. DE_SCALAR_LDS_LAST read the log / pow tables: they also run from
 * the LDS copy of the tables, as the NPP kernels stage it (k_npp.hip) */
#define DE_SCALAR_LDS_LAST 5

/* Wave modes, one wavefront per case: a row of DE_WV_IN int16, 4 int32
 * arguments, DE_WV_OUT int32 results (DE_RET return values, then the row).
 *
 *  0 wv_cfft256   256 complex points in the row, halvings -> o[0]
 *  1 wv_fft_npp   the same, dir = a0
 *  2 wv_find_harm 256 real points in b[0..256) (zero past the frame),
 *                 pitch = a0; fsmag -> b[256 .. 256 + NUM_HARM)
 */
#define DE_WV_IN 512
#define DE_WV_OUT (DE_RET + DE_WV_IN)
#define DE_WAVE_MODES(X) X(0, wv_cfft256) X(1, wv_fft_npp) X(2, wv_find_harm)
#define DE_WAVE_FIND_HARM 2
#define DE_WAVE_COUNT 3

#endif
