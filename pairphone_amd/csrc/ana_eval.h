/*
 * ana_eval.h -- one function of the encoder's pitch and voicing analysis
 * (analysis.h), or one sequence of calls of it, selected by `mode`, on one
 * case, for the function-level parity test: k_ana_eval.hip runs it one lane
 * per case on the lane's private window, hostemu.cpp (emu_ana_eval) runs the
 * host build, oracle/ref_ana.c calls the reference's own functions on the
 * same rows, and tests/test_device_ana.py requires the three to be equal.
 *
 * The modes and the case layout are in ana_eval_modes.h.  These are the
 * functions whose gfx950 form is no transcription of the reference's but a
 * set of equivalence claims (one 64-bit energy for the running margin test,
 * plain packed sums where the window's energy fits 32 bits, samples shifted
 * as they are read, lag blocks of 8 and 12, fused window passes).
 */
#ifndef MELPE_ANA_EVAL_H
#define MELPE_ANA_EVAL_H

#include "codec.h"
#include "ana_eval_modes.h"

namespace mlp {

/* a scalar of the pitch tracker on (a, b, c, d) */
MD int32_t ae_scalar(int mode, int32_t a, int32_t b, int32_t c, int32_t d)
{
	switch (mode) {
#define AE_S(id, name, call) case id: return (int32_t) (call);
	AE_SCALAR_MODES(AE_S)
#undef AE_S
	default: return 0;
	}
}

/* b[off - back .. off + len) lies inside the window, AE_PAD from either end */
MD bool ae_span(int32_t off, int32_t back, int32_t len)
{
	return len >= 0 && len <= AE_WIN && back >= 0 && back <= AE_WIN && off >= AE_PAD + back &&
	       off <= AE_WIN - AE_PAD - len;
}

MD bool ae_seq(const int32_t *a, int stride)
{
	return a[0] >= 1 && a[0] <= AE_KMAX && a[0] * stride <= AE_IN && stride <= AE_WIN;
}

MD bool ae_pitch_q7(int32_t p)
{
	return p >= PITCHMIN_Q7 && p <= PITCHMAX_Q7;
}

/* n PitTracks of pitches the tracker can hold (positive lags, so that ratio's
 * division is defined) */
MD bool ae_tracks_ok(const int16_t *p, int n)
{
	for (int t = 0; t < n; t++)
		for (int k = 0; k < NODE; k++)
			if (p[3 * NODE * t + k] < 1 || p[3 * NODE * t + k] > 255)
				return false;
	return true;
}

/* every access of the case stays inside its window or its row (a case that
 * would not is refused: r[AE_MARK] = -1, nothing run).  The pit_lib modes
 * keep to the codec's own domain -- lags and pitches in [PITCHMIN,
 * PITCHMAX], lengths up to PITCHMAX -- inside which every read of find_pitch
 * and frac_pch lies in w[0 .. AE_PW). */
MD bool ae_args_ok(int mode, const int32_t *a, const int16_t *row)
{
	switch (mode) {
	case 0:
		return a[2] <= PITCH_FR && ae_span(a[0], 0, a[2]) && ae_span(a[1], 0, a[2]) && a[3] >= 0 &&
		       (a[0] == a[1] || a[0] + a[2] <= a[1] || a[1] + a[2] <= a[0]);
	case 1:
		return ae_span(a[0], 0, AE_PW) && a[1] >= 0 && a[1] < AE_FORMS && a[2] >= PITCHMIN &&
		       a[2] <= a[3] && a[3] <= PITCHMAX && a[4] >= 1 && a[4] <= PITCHMAX;
	case 2:
		return ae_span(a[0], 0, AE_PW) && a[1] >= 0 && a[1] < AE_FORMS && ae_pitch_q7(a[2]) &&
		       (a[3] == 0 || a[3] == 5) && a[4] >= 1 && a[4] <= PITCHMAX;
	case 3:
		/* the window is shorter than minlen + pitch + 2 samples */
		return ae_pitch_q7(a[1]) && a[2] >= 0 && a[2] <= 200 && a[3] >= 1 && a[3] <= 400 &&
		       ae_span(a[0], (a[2] + (a[1] >> 7) + 4) / 2, (a[2] + (a[1] >> 7) + 4) / 2);
	case 4:
		return ae_span(a[0], 0, 3 * NODE) && a[1] > 0 && ae_tracks_ok(row + a[0], 1);
	case 5:
		return a[1] >= 0 && a[1] < TRACK_NUM && ae_span(a[0], 0, 3 * NODE * (a[1] + 1)) &&
		       ae_tracks_ok(row + a[0], a[1] + 1);
	case 6:
		if (!ae_seq(a, AE_STRIDE_PITCH_ANA))
			return false;
		for (int k = 0; k < a[0]; k++)
			if (!ae_pitch_q7(row[k * AE_STRIDE_PITCH_ANA + 2 * AE_PW]))
				return false;
		return true;
	case 7:
		return ae_seq(a, AE_STRIDE_P_AVG);
	case 8:
		if (!ae_seq(a, AE_STRIDE_BPVC))
			return false;
		for (int k = 0; k < a[0]; k++)
			if (!ae_pitch_q7(row[k * AE_STRIDE_BPVC + FRAME]) ||
			    !ae_pitch_q7(row[k * AE_STRIDE_BPVC + FRAME + 1]))
				return false;
		return true;
	case 9:
		return ae_seq(a, AE_STRIDE_PAUTO);
	case 10:
		if (!ae_seq(a, AE_STRIDE_CLASSIFY))
			return false;
		for (int k = 0; k < a[0]; k++) {
			const int16_t p = row[k * AE_STRIDE_CLASSIFY + AE_CLS_SPAN + 17 + 2];
			if (p < MINPITCH || p > MAXPITCH)
				return false;
		}
		return true;
	default:
		return false;
	}
}

/* the window's energy as f_pitch_scale adds it up: sum of L_mult(x, x) */
MD int64_t ae_energy(const int16_t *w, int n)
{
	int64_t e = 0;
	for (int i = 0; i < n; i++)
		e += L_mult(w[i], w[i]);
	return e;
}

/* find_pitch (fp) or frac_pch on the pitch window w in the form a[1] */
MD void ae_pit_lib(bool fp, int16_t *w, const int32_t *a, int32_t *r)
{
	bool ex = false;
	int lsh = 0;
	Word16 sc = 0, pcorr = 0, ret;
	const int16_t *sig = w + AE_PC;
	bool unscaled = false;
	if (a[1] == 2) {
		const int64_t e = ae_energy(w, AE_PW);
		if (e <= (int64_t) LW_MAX_) {
			lsh = shr(norm_l((Word32) e), 1);
			ex = true;
			unscaled = true;
		}
	}
	if (!unscaled) {
		sc = f_pitch_scale(w, w, AE_PW, &ex);
		if (a[1] == 0)
			ex = false;
	}
	if (fp)
		ret = find_pitch(sig, &pcorr, (Word16) a[2], (Word16) a[3], (Word16) a[4], ex, lsh);
	else
		ret = frac_pch(sig, &pcorr, (Word16) a[2], (Word16) a[3], PITCHMIN, PITCHMAX, PITCHMIN_Q7,
			       PITCHMAX_Q7, (Word16) a[4], ex, lsh);
	if (unscaled)
		sc = f_pitch_scale(w, w, AE_PW);
	r[0] = ret;
	r[1] = pcorr;
	r[2] = sc;
	r[AE_INFO] = ex;
}

/* one call's inputs from the case's row into the window */
MD void ae_fetch(int16_t *b, const int16_t *src, int n)
{
	for (int i = 0; i < n; i++)
		b[i] = src[i];
}

/* mode on the case: b the private window (AE_WIN int16, dword-aligned), row
 * the case's AE_IN int16 as given, E zeroed state (the statics of a fresh
 * process), arguments a, return values r[0 .. AE_RET) (zeroed) */
MD void ae_eval(int mode, const int16_t *row, int16_t *b, EncAna *E, const int32_t *a, int32_t *r)
{
	if (!ae_args_ok(mode, a, row)) {
		r[AE_MARK] = -1;
		return;
	}
	if (mode < AE_FIRST_STATEFUL)
		for (int k = 0; k < AE_WIN; k++)
			b[k] = row[k];
	switch (mode) {
	case 0: {
		bool ex = false;
		r[0] = f_pitch_scale(b + a[1], b + a[0], a[2], &ex, (int64_t) a[3]);
		r[AE_INFO] = ex;
		break;
	}
	case 1:
		ae_pit_lib(true, b + a[0], a, r);
		break;
	case 2:
		ae_pit_lib(false, b + a[0], a, r);
		break;
	case 3:
		r[0] = gain_ana(b + a[0], (Word16) a[1], (Word16) a[2], (Word16) a[3]);
		break;
	case 4:
		r[0] = trackPitch((Word16) a[1], reinterpret_cast<const PitTrack *>(b + a[0]));
		break;
	case 5:
		r[0] = pitLookahead(reinterpret_cast<PitTrack *>(b + a[0]), a[1]);
		break;
	case 6:
		for (int k = 0; k < a[0]; k++) {
			ae_fetch(b, row + k * AE_STRIDE_PITCH_ANA, AE_STRIDE_PITCH_ANA);
			Word16 pcorr = 0;
			r[k * AE_CALL] = pitch_ana(E, b + AE_PC, b + AE_PW + AE_PC, b[2 * AE_PW], b[2 * AE_PW + 1],
						   &pcorr);
			r[k * AE_CALL + 1] = pcorr;
		}
		break;
	case 7:
		for (int k = 0; k < a[0]; k++) {
			ae_fetch(b, row + k * AE_STRIDE_P_AVG, AE_STRIDE_P_AVG);
			r[k * AE_CALL] = p_avg_update(E, b[0], b[1], b[2]);
		}
		break;
	case 8:
		for (int k = 0; k < a[0]; k++) {
			ae_fetch(b, row + k * AE_STRIDE_BPVC, AE_STRIDE_BPVC);
			int16_t bpvc[NUM_BANDS] = {0, 0, 0, 0, 0};
			Word16 pitch = 0;
			/* the argument's [PITCH_FR - FRAME - PITCHMAX] is b[0] */
			bpvc_ana(E, b - (PITCH_FR - FRAME - PITCHMAX), b + FRAME, bpvc, &pitch);
			for (int i = 0; i < NUM_BANDS; i++)
				r[k * AE_CALL + i] = bpvc[i];
			r[k * AE_CALL + NUM_BANDS] = pitch;
		}
		break;
	case 9:
		for (int k = 0; k < a[0]; k++) {
			ae_fetch(b, row + k * AE_STRIDE_PAUTO, AE_STRIDE_PAUTO);
			PitTrack *pt = &E->pitTrack[0];
			ClassParam *cs = &E->classStat[0];
			pitchAuto(E, b, pt, cs);
			for (int i = 0; i < NODE; i++) {
				r[k * AE_CALL + i] = pt->pit[i];
				r[k * AE_CALL + NODE + i] = pt->weight[i];
			}
			r[k * AE_CALL + 2 * NODE] = cs->pitch;
			r[k * AE_CALL + 2 * NODE + 1] = cs->corx;
		}
		break;
	case 10:
		for (int k = 0; k < a[0]; k++) {
			ae_fetch(b, row + k * AE_STRIDE_CLASSIFY, AE_STRIDE_CLASSIFY);
			const int16_t *x = b + AE_CLS_SPAN + 17;
			ClassParam *cs = &E->classStat[1];
			cs[-1].zeroCrosRate = x[0];
			cs[-1].subEnergy = x[1];
			cs->pitch = x[2];
			cs->corx = x[3];
			if (k > 0) {
				E->voicedEn = x[4];
				E->silenceEn = x[5];
			}
			classify(E, b + AE_CLS_BACK, cs, b + AE_CLS_SPAN);
			int32_t *o = r + k * AE_CALL;
			o[0] = cs->classy;
			o[1] = cs->subEnergy;
			o[2] = cs->zeroCrosRate;
			o[3] = cs->peakiness;
			o[4] = cs->corx;
			o[5] = cs->pitch;
			o[6] = E->voicedEn;
			o[7] = E->silenceEn;
			o[8] = E->voicedCnt;
		}
		break;
	default:
		break;
	}
}

}  // namespace mlp

#endif
