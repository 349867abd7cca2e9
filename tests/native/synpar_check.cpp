/*
 * synpar_check.cpp -- the synthesis from parameter rows is total: the host
 * build of decoder.h synth_superframe (row admission, then melp_syn) on
 * 100,000 superframes of uniformly random int16 rows and on the all-0x8000,
 * all-0x7FFF, all-zero and all-(-1) rows, on a few channels of carried state.
 * Built with -fsanitize=address,undefined (tests/test_synth_params.py), so an
 * index outside a table or a frame, a shift out of range or a signed overflow
 * anywhere under melp_syn fails the run; a loop that does not end fails the
 * test's time limit.  Prints a hash of every sample and status byte.
 *
 *   synpar_check <melpe_tables.bin> [superframes]
 *
 * Word w of superframe j is the top 16 bits of splitmix64(SEED + 90 j + w);
 * from superframe `superframes` on, for a fifth as many, the uv_flag words keep
 * only their low bit.  tests/test_synth_params_dev.py regenerates rows of both
 * parts from the same formula and runs them on the GPU.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "codec.h"

using namespace mlp;

#define SEED 0x53594e50ull	/* "SYNP" */
#define CHANNELS 4

static uint64_t splitmix64(uint64_t x)
{
	x += 0x9e3779b97f4a7c15ull;
	x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
	x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
	return x ^ (x >> 31);
}

static uint64_t h = 0xcbf29ce484222325ull;
static void fold(const void *p, size_t n)
{
	for (size_t i = 0; i < n; i++)
		h = (h ^ ((const uint8_t *) p)[i]) * 0x100000001b3ull;
}

int main(int argc, char **argv)
{
	if (argc < 2)
		return 2;
	FILE *f = fopen(argv[1], "rb");
	if (!f || fread(g_tab, sizeof(int16_t), MELPE_TABLE_WORDS, f) != MELPE_TABLE_WORDS)
		return 2;
	fclose(f);
	derive_all(&g_der);
	derive_lspgrid(g_der.lsp_cos, g_lspgrid);
	const long total = argc > 2 ? atol(argv[2]) : 100000;

	/* each record and each PCM block in a heap block of its own size */
	DecState *D[CHANNELS];
	for (int c = 0; c < CHANNELS; c++) {
		D[c] = (DecState *) aligned_alloc(16, sizeof(DecState));
		dec_reset(D[c]);
	}
	int16_t *out = (int16_t *) malloc(sizeof(int16_t) * BLOCK);
	MelpParam *rows = (MelpParam *) malloc(sizeof(MelpParam) * NF);
	long clamped = 0;
	const int16_t fills[4] = {(int16_t) 0x8000, 0x7fff, 0, -1};
	/* A uniformly random uv_flag is nonzero 65,535 times in 65,536, and the
	 * head then overwrites the frame's pitch, jitter and magnitudes; so
	 * total / 5 more superframes follow whose uv_flag words keep only their
	 * low bit, which sends full-range values down the voiced paths too */
	const long extra = total / 5;
	for (long j = 0; j < total + extra + 4 * CHANNELS; j++) {
		int16_t *w = (int16_t *) rows;
		for (int k = 0; k < NF * 30; k++) {
			if (j >= total + extra) {
				w[k] = fills[(j - total - extra) / CHANNELS];
				continue;
			}
			w[k] = (int16_t) (splitmix64(SEED + 90ull * (uint64_t) j + k) >> 48);
			if (j >= total && k % 30 == 19)
				w[k] &= 1;
		}
		uint8_t st = 2;
		synth_superframe(D[j % CHANNELS], rows, out, &st);
		if (st > 1)
			return 3;
		clamped += st;
		fold(out, sizeof(int16_t) * BLOCK);
		fold(&st, 1);
	}
	for (int c = 0; c < CHANNELS; c++) {
		fold(D[c], sizeof(DecState));
		free(D[c]);
	}
	free(out);
	free(rows);
	printf("OK %ld superframes, %ld clamped, hash %016llx\n", total + extra + 4 * CHANNELS, clamped, (unsigned long long) h);
	return 0;
}
