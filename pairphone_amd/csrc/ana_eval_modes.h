/*
 * ana_eval_modes.h -- the mode list and case layout of the function-level
 * parity test of the encoder's pitch and voicing analysis (ana_eval.h).
 * Plain preprocessor text: the device kernel, the host build, the checker
 * (oracle/ref_ana.c, a C program) and tests/test_device_ana.py (which parses
 * the list) all read the ids from here.
 *
 * One case is a row of AE_IN int16 (`row`, in global memory), AE_ARGS int32
 * arguments (`a`) and AE_OUT int32 results: AE_RET return values and then the
 * private window b[0 .. AE_WIN) as the last call left it, so everything the
 * function writes -- and anything it should not have written -- is compared.
 *
 * Stateless modes: b is a copy of row[0 .. AE_WIN); offsets in the arguments
 * are int16 indices into b.  The values of the one call go to r[0 ..).
 *
 * Stateful modes: a case is K = a[0] consecutive calls from the state of a
 * fresh process; call k reads its inputs from row[k * stride .. (k + 1) *
 * stride) into b[0 .. stride) (one reused window) and writes its values to
 * r[k * AE_CALL .. (k + 1) * AE_CALL), so a state error of call k shows in
 * call k + 1.
 *
 * r[AE_INFO]: what only this implementation has (the `exact` flag);
 * the checker leaves it zero.  r[AE_MARK] = -1: the case was refused
 * (ae_args_ok), nothing run.
 */
#ifndef MELPE_ANA_EVAL_MODES_H
#define MELPE_ANA_EVAL_MODES_H

#define AE_IN 2688	/* int16 per case */
#define AE_WIN 832	/* int16 of the private window */
#define AE_ARGS 8	/* int32 per case */
#define AE_CALL 20	/* values per call */
#define AE_KMAX 8	/* calls per case, at most */
#define AE_INFO 160
#define AE_MARK 161
#define AE_RET 162	/* return values in front of the window dump */
#define AE_OUT (AE_RET + AE_WIN)	/* int32 per case */
#define AE_PAD 16	/* int16 kept between a signal and either end of b */
#define AE_PW 321	/* a pitch window: PITCH_FR samples, the signal pointer at + AE_PC */
#define AE_PC 160

/* the forms of the pit_lib modes (the argument `form`):
 *  0  f_pitch_scale on the window, then the function with exact = false
 *  1  the same with the flag f_pitch_scale gives
 *  2  as bpvc_band0: window energy e <= LW_MAX -> the unscaled window with
 *     exact = true and lsh = norm_l(e) >> 1 (the window scaled afterwards,
 *     for the dump); else form 1 */
#define AE_FORMS 3

/* X(id, name).  Arguments a[0..7]; w = b + a0 is a pitch window.
 *
 *  0 f_pitch_scale  (out=b+a1, in=b+a0, len=a2, extra=a3): shift -> r[0],
 *                   the exact flag -> r[AE_INFO]
 *  1 find_pitch     f_pitch_scale(w, w, AE_PW), then find_pitch(w + AE_PC,
 *                   lower=a2, upper=a3, len=a4), form=a1: ip -> r[0],
 *                   pcorr -> r[1], the shift -> r[2]
 *  2 frac_pch       f_pitch_scale(w, w, AE_PW), then frac_pch(w + AE_PC,
 *                   fpitch=a2, range=a3, PITCHMIN, PITCHMAX, PITCHMIN_Q7,
 *                   PITCHMAX_Q7, lmin=a4), form=a1: fpitch -> r[0],
 *                   pcorr -> r[1], the shift -> r[2]
 *  3 gain_ana       (b+a0, pitch=a1, minlen=a2, maxlen=a3) -> r[0]
 *  4 trackPitch     (pitch=a1, the PitTrack at b+a0: pit[8], weight[8],
 *                   cost[8]) -> r[0]
 *  5 pitLookahead   (a1 + 1 PitTracks from b+a0, num=a1) -> r[0]; the costs
 *                   it writes are in the dump
 *  6 pitch_ana      K=a0 calls, stride 2 * AE_PW + 2: speech window, resid
 *                   window (the pointers at + AE_PC), pest, pavg: pitch ->
 *                   r[c], pcorr -> r[c+1] (c = AE_CALL * k)
 *  7 p_avg_update   K=a0 calls, stride 4: pitch, pcorr, pthresh -> r[c]
 *  8 bpvc_ana       K=a0 calls, stride 184: 180 new samples (speech[-19 ..
 *                   161) of the reference's argument), fpitch[0..2):
 *                   bpvc[0..5) -> r[c .. c+5), pitch -> r[c+5]
 *  9 pitchAuto      K=a0 calls, stride 92: 90 new samples: pit[8] -> r[c ..
 *                   c+8), weight[8] -> r[c+8 .. c+16), classStat.pitch ->
 *                   r[c+16], corx -> r[c+17]
 * 10 classify       K=a0 calls, stride 244: inbuf[-65 .. 155), autocorr[17],
 *                   then the previous subframe's zeroCrosRate and subEnergy,
 *                   this one's pitch and corx, and voicedEn, silenceEn as
 *                   they stand before the call (set from the second call
 *                   on; the first call initialises them): classy, subEnergy,
 *                   zeroCrosRate, peakiness, corx, pitch -> r[c .. c+6),
 *                   voicedEn, silenceEn, voicedCnt -> r[c+6 .. c+9)
 */
#define AE_MODES(X) \
	X(0, f_pitch_scale) X(1, find_pitch) X(2, frac_pch) X(3, gain_ana) X(4, trackPitch) \
	X(5, pitLookahead) X(6, pitch_ana) X(7, p_avg_update) X(8, bpvc_ana) X(9, pitchAuto) \
	X(10, classify)
#define AE_MODE_COUNT 11
#define AE_FIRST_STATEFUL 6
#define AE_STRIDE_PITCH_ANA 644
#define AE_STRIDE_P_AVG 4
#define AE_STRIDE_BPVC 184
#define AE_STRIDE_PAUTO 92
#define AE_STRIDE_CLASSIFY 244
#define AE_CLS_BACK 65	/* inbuf[0] is the 65th sample of a classify call */
#define AE_CLS_SPAN 220

/* Scalar modes, the pitch tracker's scalars: one case is four int32
 * arguments and one int32 result.  S(id, name, call on int32 a, b, c, d) */
#define AE_SCALAR_MODES(S) \
	S(0, ratio, ratio((int16_t) a, (int16_t) b)) \
	S(1, L_ratio, L_ratio((int16_t) a, b)) \
	S(2, updateEn, updateEn((int16_t) a, (int16_t) b, (int16_t) c)) \
	S(3, multiCheck, multiCheck((int16_t) a, (int16_t) b))
#define AE_SCALAR_COUNT 4

#endif
