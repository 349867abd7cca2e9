/*
 * ref_synpar.c -- drives the REFERENCE's synthesis() with its own build switch
 * SKIP_CHANNEL on, for tests/golden/make_synpar_golden.py (dev container only).
 *
 * melpe/sc1200.h:53 defines SKIP_CHANNEL FALSE; with it TRUE, synthesis()
 * (melpe/melp_syn.c:110-146) leaves out low_rate_chn_read, keeps erase = FALSE
 * and runs melp_syn on whatever melp_par[3] holds.  The header is guarded, so
 * it is included here first, the switch redefined, and melp_syn.c then compiled
 * where it lies, by inclusion; nothing of it is copied.  Everything else comes
 * from libmelpe_ref.a: this file defines melp_syn.c's two external functions,
 * so the archive's own melp_syn.o is never pulled in.
 * make_synpar_golden.py builds this into oracle/_ref/ref_synpar.
 *
 * One process = one channel (the codec's statics are per process).
 *
 *   ref_synpar in out
 *     in:  K x 90 int16, the three rows of each superframe
 *     out: per superframe 540 int16 of speech, then melp_par[3] as
 *          synthesis() left it (90 int16)
 */
#include "sc1200.h"
#undef SKIP_CHANNEL
#define SKIP_CHANNEL TRUE
#include "melp_syn.c"

#include <stdio.h>
#include <string.h>

void melpe_i(void);

int main(int argc, char **argv)
{
	if (argc != 3)
		return 1;
	FILE *fi = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
	if (!fi || !out)
		return 2;
	int16_t rows[NF * 30], sp[BLOCK];
	if (sizeof(struct melp_param) != 60 || sizeof(melp_par[0]) * NF != sizeof rows)
		return 3;
	melpe_i();
	while (fread(rows, sizeof rows, 1, fi) == 1) {
		memcpy(melp_par, rows, sizeof rows);
		synthesis(melp_par, sp);
		fwrite(sp, sizeof sp, 1, out);
		fwrite(melp_par, sizeof rows, 1, out);
	}
	fclose(fi);
	fclose(out);
	return 0;
}
