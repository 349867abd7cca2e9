/*
 * ref_dsp.c -- the REFERENCE's own DSP and math functions on the cases of
 * the function-level parity test (TEST INFRASTRUCTURE ONLY): the checker of
 * pairphone_amd/csrc/dsp_eval.h, same mode ids and case layout
 * (dsp_eval_modes.h).  It calls the reference's functions and restates none
 * of them; its static functions (lsp_to_freq, lpc_refl2pred) are reached
 * through their public callers lpc_pred2lsp and lpc_schr.
 *
 * A stand-alone program, not a library: the reference is built with its
 * asserts live (L_divider2's preconditions), and an assert must end this
 * process, not the test runner's.
 *
 *   ref_dsp v <mode> <n> <in> <out>   vector modes: <in> holds n rows of
 *       DE_IN int16, then n rows of DE_ARGS int32; <out> n rows of DE_OUT
 *       int32
 *   ref_dsp s <mode> <n> <in> <out>   scalar modes: n x 4 int32 -> n int32
 *   ref_dsp w <mode> <n> <in> <out>   wave modes: n rows of DE_WV_IN int16,
 *       then n x 4 int32 -> n rows of DE_WV_OUT int32
 *
 * For the device-only fused forms the expected value is the sequence of
 * reference calls the fused form's comment claims to equal (three in-place
 * iir_2nd_s passes for iir3_s, and so on).
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>

#include "sc1200.h"
#include "mathhalf.h"
#include "math_lib.h"
#include "mat_lib.h"
#include "dsp_sub.h"
#include "lpc_lib.h"
#include "fft_lib.h"
#include "fs_lib.h"
#include "dsp_eval_modes.h"

static int32_t scalar(int mode, int32_t a, int32_t b, int32_t c, int32_t d)
{
	switch (mode) {
#define DE_S(id, name, call) case id: return (int32_t) (call);
	DE_SCALAR_MODES(DE_S)
#undef DE_S
	}
	return 0;
}

/* three cascaded single-precision sections, one after the other, in place */
static void iir3_s_ref(int16_t *x, int16_t *out, int16_t *b, int n)
{
	int s;
	iir_2nd_s(x, b, b + 9, out, b + 18, b + 24, (int16_t) n);
	for (s = 1; s < 3; s++)
		iir_2nd_s(out, b + 3 * s, b + 9 + 3 * s, out, b + 18 + 2 * s, b + 24 + 2 * s, (int16_t) n);
}

static void iir3_d_ref(int16_t *x, int16_t *out, int16_t *b, int n)
{
	int s;
	iir_2nd_d(x, b, b + 9, out, b + 18, b + 24, b + 30, (int16_t) n);
	for (s = 1; s < 3; s++)
		iir_2nd_d(out, b + 3 * s, b + 9 + 3 * s, out, b + 18 + 2 * s, b + 24 + 2 * s,
			  b + 30 + 2 * s, (int16_t) n);
}

static void vector(int mode, int16_t *b, const int32_t *a, int32_t *r)
{
	int i;
	switch (mode) {
	case 0:
		r[0] = L_v_inner(b + a[0], b + a[1], (int16_t) a[2], (int16_t) a[3], (int16_t) a[4],
				 (int16_t) a[5]);
		break;
	case 1:
		r[0] = L_v_magsq(b + a[0], (int16_t) a[2], (int16_t) a[3], (int16_t) a[5]);
		break;
	case 2:
		zerflt_Q(b + a[0], b, b + a[1], (int16_t) a[2], (int16_t) a[3], (int16_t) a[4]);
		break;
	case 3:
		iir_2nd_s(b + a[0], b, b + 3, b + a[1], b + 6, b + 8, (int16_t) a[2]);
		break;
	case 4:
		iir_2nd_d(b + a[0], b, b + 3, b + a[1], b + 6, b + 8, b + 10, (int16_t) a[2]);
		break;
	case 5: {
		/* snap > 0: filter the first part, save the memories, filter
		 * the rest, restore (melp_ana.c:324-346) */
		int16_t keep[12];
		if (a[3] > 0) {
			iir3_s_ref(b + a[0], b + a[0], b, a[3]);
			memcpy(keep, b + 18, sizeof keep);
			iir3_s_ref(b + a[0] + a[3], b + a[0] + a[3], b, a[2] - a[3]);
			memcpy(b + 18, keep, sizeof keep);
		} else {
			iir3_s_ref(b + a[0], b + a[0], b, a[2]);
		}
		break;
	}
	case 6:
		iir3_s_ref(b + a[0], b + a[1], b, a[2]);
		memmove(b + a[3], b + a[1], sizeof(int16_t) * a[2]);
		break;
	case 7:
	case 8:
		iir3_d_ref(b + a[0], b + a[1], b, a[2]);
		break;
	case 9:
		iir_2nd_d(b + a[0], b, b + 3, b + a[0], b + 6, b + 8, b + 10, (int16_t) a[2]);
		iir_2nd_d(b + a[0], b + 12, b + 15, b + a[0], b + 18, b + 20, b + 22, (int16_t) a[2]);
		break;
	case 10:
		envelope(b + a[0], (int16_t) a[3], b + a[1], (int16_t) a[2]);
		break;
	case 11: {
		/* the input scaled up by 2^lsh (the caller's precondition: no
		 * sample overflows), envelope, and the energy of what it wrote */
		int16_t tmp[DE_IN];
		int64_t e = 0;
		for (i = 0; i < a[2]; i++)
			tmp[i] = (int16_t) (b[a[0] + i] * (1 << a[4]));
		envelope(tmp, (int16_t) a[3], b + a[1], (int16_t) a[2]);
		for (i = 0; i < a[2]; i++)
			e += melpe_L_mult(b[a[1] + i], b[a[1] + i]);
		r[0] = (int32_t) (uint32_t) e;
		r[1] = (int32_t) (e >> 32);
		break;
	}
	case 12:
		lpc_syn(b + a[0], b + a[1], b, (int16_t) a[2], (int16_t) a[3]);
		break;
	case 13:
		r[0] = cfft(b + DE_DATA, 256);
		break;
	case 14:
		r[0] = fft_npp(b + DE_DATA, (int16_t) a[0]);
		break;
	case 15:
	case 16:
		rfft(b + DE_DATA, 512);
		break;
	case 17:
		find_harm(b + a[0], b, (int16_t) a[2], NUM_HARM, (int16_t) a[1]);
		break;
	case 18:
		lpc_acor(b + a[0], b + a[1], b, (int16_t) a[4], (int16_t) a[2], (int16_t) a[3]);
		break;
	case 19:
		r[0] = lpc_schr(b, b + 16, 10);
		break;
	case 20:
		lpc_pred2lsp(b, b + 16, 10);
		break;
	case 21:
	case 22:
		lpc_lsp2pred(b, b + 16, 10);
		break;
	case 23:
		lpc_clmp(b, (int16_t) a[0], (int16_t) a[1]);
		break;
	case 24: {
		int16_t refc = 0;
		r[0] = lpc_pred2refl(b, &refc, 10);
		r[1] = refc;
		break;
	}
	}
}

static void wave(int mode, int16_t *b, const int32_t *a, int32_t *r)
{
	switch (mode) {
	case 0:
		r[0] = cfft(b, 256);
		break;
	case 1:
		r[0] = fft_npp(b, (int16_t) a[0]);
		break;
	case 2:
		find_harm(b, b + 256, (int16_t) a[0], NUM_HARM, 256);
		break;
	}
}

static void *load(const char *path, size_t bytes)
{
	FILE *f = fopen(path, "rb");
	void *p = malloc(bytes ? bytes : 1);
	if (!f || !p || fread(p, 1, bytes, f) != bytes) {
		fprintf(stderr, "ref_dsp: cannot read %zu bytes of %s\n", bytes, path);
		exit(2);
	}
	fclose(f);
	return p;
}

int main(int argc, char **argv)
{
	if (argc != 6) {
		fprintf(stderr, "usage: ref_dsp v|s|w <mode> <n> <in> <out>\n");
		return 2;
	}
	const char kind = argv[1][0];
	const int mode = atoi(argv[2]);
	const long n = atol(argv[3]);
	long i;
	int k;
	FILE *fo;
	int32_t *out;
	size_t out_words;

	fs_init();	/* the FFT's twiddle tables (melp_ana_init does this) */
	if (kind == 's') {
		const int32_t *a = load(argv[4], sizeof(int32_t) * 4 * n);
		out_words = n;
		out = calloc(out_words ? out_words : 1, sizeof(int32_t));
		for (i = 0; i < n; i++)
			out[i] = scalar(mode, a[4 * i], a[4 * i + 1], a[4 * i + 2], a[4 * i + 3]);
	} else {
		const int wv = kind == 'w';
		const int nin = wv ? DE_WV_IN : DE_IN, nargs = wv ? 4 : DE_ARGS;
		const int nout = DE_RET + nin;
		char *raw = load(argv[4], (sizeof(int16_t) * nin + sizeof(int32_t) * nargs) * n);
		const int16_t *in = (const int16_t *) raw;
		const int32_t *args = (const int32_t *) (raw + sizeof(int16_t) * nin * n);
		out_words = (size_t) nout * n;
		out = calloc(out_words ? out_words : 1, sizeof(int32_t));
		for (i = 0; i < n; i++) {
			int16_t b[DE_IN];
			int32_t a[DE_ARGS], *o = out + (size_t) nout * i;
			memcpy(b, in + (size_t) nin * i, sizeof(int16_t) * nin);
			memcpy(a, args + (size_t) nargs * i, sizeof(int32_t) * nargs);
			if (wv)
				wave(mode, b, a, o);
			else
				vector(mode, b, a, o);
			for (k = 0; k < nin; k++)
				o[DE_RET + k] = b[k];
		}
	}
	fo = fopen(argv[5], "wb");
	if (!fo || fwrite(out, sizeof(int32_t), out_words, fo) != out_words) {
		fprintf(stderr, "ref_dsp: cannot write %s\n", argv[5]);
		return 2;
	}
	fclose(fo);
	return 0;
}
