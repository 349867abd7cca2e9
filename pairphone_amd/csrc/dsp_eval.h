/*
 * dsp_eval.h -- one function of the DSP and math library (dsp.h, the
 * find_harm part of analysis.h) selected by `mode`, on one case, for the
 * function-level parity test: k_dsp_eval.hip runs it one lane per case on
 * the lane's private copy of the row, hostemu.cpp (emu_dsp_eval) runs the
 * host build, oracle/ref_dsp.c calls the reference's own functions on the
 * same rows, and tests/test_device_dsp.py requires the three to be equal.
 *
 * The modes and the case layout are in dsp_eval_modes.h.  These are the
 * functions whose gfx950 form is a restructuring of the reference's
 * (blocked FIRs, fused cascades, deferred divisions, packed FFT), each with
 * several dispatch arms that only built inputs reach.
 */
#ifndef MELPE_DSP_EVAL_H
#define MELPE_DSP_EVAL_H

#include "codec.h"
#include "dsp_eval_modes.h"

namespace mlp {

/* a scalar math function on (a, b, c, d) */
MD int32_t de_scalar(int mode, int32_t a, int32_t b, int32_t c, int32_t d)
{
	/* the logarithms index their table with the argument's top bits: a
	 * negative argument is outside the reference's domain (and the table) */
	if ((mode == 0 || (mode >= 2 && mode <= 5)) && a < 0)
		return 0;
	switch (mode) {
#define DE_S(id, name, call) case id: return (int32_t) (call);
	DE_SCALAR_MODES(DE_S)
#undef DE_S
	default: return 0;
	}
}

/* b[off - back .. off + len) lies in the signal area */
MD bool de_span(int32_t off, int32_t back, int32_t len)
{
	return len >= 0 && len <= DE_IN && back >= 0 && back <= DE_IN && off >= DE_DATA + back &&
	       off <= DE_IN - len;
}

/* every access of the case stays inside its row (the kernel refuses a case
 * that would not: r[DE_RET - 1] = -1, nothing run) */
MD bool de_args_ok(int mode, const int32_t *a)
{
	switch (mode) {
	case 0:
		return de_span(a[0], 0, a[2]) && de_span(a[1], 0, a[2]);
	case 1:
		return de_span(a[0], 0, a[2]);
	case 2:
		return a[2] >= 0 && a[2] < DE_DATA && de_span(a[0], a[2], a[3]) && de_span(a[1], 0, a[3]);
	case 3: case 4: case 7:
		return de_span(a[0], 0, a[2]) && de_span(a[1], 0, a[2]);
	case 5:
		return de_span(a[0], 0, a[2]) && a[3] >= 0 && a[3] < (a[2] > 0 ? a[2] : 1) && a[3] % 4 == 0;
	case 6:
		return de_span(a[0], 0, a[2]) && de_span(a[1], 0, a[2]) && de_span(a[3], 0, a[2]);
	case 8:
		return de_span(a[0], 0, a[2]) && de_span(a[1], 0, a[2]) && a[0] % 2 == 0 && a[2] % 36 == 0;
	case 9:
		return de_span(a[0], 0, a[2]);
	case 10:
		return de_span(a[0], 0, a[2]) && de_span(a[1], 2, a[2]);
	case 11:
		return de_span(a[0], 0, a[2]) && de_span(a[1], 2, a[2]) && a[4] >= 0 && a[4] <= 14;
	case 12:
		return a[2] >= 1 && a[2] <= 16 && de_span(a[0], 0, a[3]) && de_span(a[1], a[2], a[3]);
	case 13: case 14: case 15: case 16:
		return true;
	case 17:
		return a[1] >= 1 && a[1] <= 512 && de_span(a[0], 0, a[1]) && a[2] >= 20 * 128 && a[2] <= 160 * 128;
	case 18:
		return (a[2] == 10 || a[2] == 16) && a[3] >= 1 && a[3] <= 200 && de_span(a[0], 0, a[3]) &&
		       de_span(a[1], 0, a[3]);
	case 19: case 20: case 21: case 22: case 24:
		return true;
	case 23:
		return a[1] >= 2 && a[1] <= DE_DATA;
	default:
		return false;
	}
}

/* mode on the row b (in place), arguments a, return values r[0 .. DE_RET) */
MD void de_eval(int mode, int16_t *b, const int32_t *a, int32_t *r)
{
	if (!de_args_ok(mode, a)) {
		r[DE_RET - 1] = -1;
		return;
	}
	switch (mode) {
	case 0:
		r[0] = L_v_inner(b + a[0], b + a[1], a[2], (int16_t) a[3], (int16_t) a[4], (int16_t) a[5]);
		break;
	case 1:
		r[0] = L_v_magsq(b + a[0], a[2], (int16_t) a[3], (int16_t) a[5]);
		break;
	case 2:
		zerflt_Q(b + a[0], b, b + a[1], a[2], a[3], (Word16) a[4]);
		break;
	case 3:
		iir_2nd_s(b + a[0], b, b + 3, b + a[1], b + 6, b + 8, a[2]);
		break;
	case 4:
		iir_2nd_d(b + a[0], b, b + 3, b + a[1], b + 6, b + 8, b + 10, a[2]);
		break;
	case 5:
		iir3_s(b + a[0], b, b + 9, b + 18, b + 24, a[2], a[3]);
		break;
	case 6: {
		int16_t *seen = b + a[3];
		iir3_s_io(b + a[0], b + a[1], b, b + 9, b + 18, b + 24, a[2],
			  [&](int i, int16_t y) { seen[i] = y; });
		break;
	}
	case 7:
		iir3_d(b + a[0], b + a[1], b, b + 9, b + 18, b + 24, b + 30, a[2]);
		break;
	case 8:
		iir3_d_batched(b + a[0], b + a[1], b, b + 9, b + 18, b + 24, b + 30, a[2]);
		break;
	case 9:
		iir2_d(b + a[0], b, b + 3, b + 6, b + 8, b + 10, b + 12, b + 15, b + 18, b + 20, b + 22, a[2]);
		break;
	case 10:
		envelope(b + a[0], (int16_t) a[3], b + a[1], a[2]);
		break;
	case 11: {
		int64_t e = envelope_e(b + a[0], (int16_t) a[3], b + a[1], a[2], a[4]);
		r[0] = (int32_t) (uint32_t) e;
		r[1] = (int32_t) (e >> 32);
		break;
	}
	case 12:
		lpc_syn(b + a[0], b + a[1], b, a[2], a[3]);
		break;
	case 13:
		r[0] = cfft(b + DE_DATA, 256);
		break;
	case 14:
		r[0] = fft_npp(b + DE_DATA, (Word16) a[0]);
		break;
	case 15:
		rfft(b + DE_DATA, 512);
		break;
	case 16: {
		uint32_t hb[512];
		int16_t *d = b + DE_DATA;
		Word16 mx = 0;
		for (int k = 0; k < 256; k++) {
			hb[k] = pk(d[2 * k], d[2 * k + 1]);
			mx = pk_amax(hb[k], mx);
		}
		for (int k = 256; k < 512; k++)
			hb[k] = 0;
		rfft_pk(hb, 512, mx);
		for (int k = 0; k < 512; k++) {
			d[2 * k] = pk_re(hb[k]);
			d[2 * k + 1] = pk_im(hb[k]);
		}
		break;
	}
	case 17:
		find_harm(b + a[0], b, (Word16) a[2], NUM_HARM, a[1]);
		break;
	case 18:
		lpc_acor(b + a[0], b + a[1], b, (Word16) a[4], a[2], a[3]);
		break;
	case 19:
		r[0] = lpc_schr(b, b + 16, 10);
		break;
	case 20:
		lpc_pred2lsp(b, b + 16, 10);
		break;
	case 21:
		lpc_lsp2pred(b, b + 16, 10);
		break;
	case 22:
		lsf_sort10(b);
		lsp2pred10(b, b + 16);
		break;
	case 23:
		lpc_clmp(b, (Word16) a[0], a[1]);
		break;
	case 24: {
		int16_t refc = 0;
		r[0] = lpc_pred2refl(b, &refc, 10);
		r[1] = refc;
		break;
	}
	default:
		break;
	}
}

}  // namespace mlp

#endif
