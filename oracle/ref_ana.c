/*
 * ref_ana.c -- the REFERENCE's own pitch and voicing analysis functions on
 * the cases of the function-level parity test (TEST INFRASTRUCTURE ONLY): the
 * checker of pairphone_amd/csrc/ana_eval.h, same mode ids and case layout
 * (ana_eval_modes.h).  It calls the reference's functions and restates none
 * of them; its static functions are reached through their public callers
 * (double_chk and double_ver through pitch_ana; lpfilt, ivfilt and corPeak
 * through pitchAuto; zeroCrosCount, bandEn and frac_cor through classify).
 *
 *   ref_ana v <mode> <n> <in> <out>   <in> holds n rows of AE_IN int16, then
 *       n rows of AE_ARGS int32; <out> n rows of AE_OUT int32
 *   ref_ana s <mode> <n> <in> <out>   scalar modes: n x 4 int32 -> n int32
 *
 * pitch_ana, p_avg_update, bpvc_ana, pitchAuto and classify keep their state
 * in function-scope statics behind a firstTime flag, which nothing outside
 * can set or reset:
 * every case of a stateful mode runs in a child process of its own (fork),
 * which sends its row back through a pipe.  A child that dies (a live assert
 * of the reference, a signal) ends the run: non-zero exit, the case index on
 * stderr.
 *
 * For the forms only the device has (exact sums, samples shifted as they are
 * read) the expected value is the sequence of reference calls the form's
 * comment claims to equal: f_pitch_scale, then the function.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include <unistd.h>
#include <sys/types.h>
#include <sys/wait.h>

#include "sc1200.h"
#include "mathhalf.h"
#include "math_lib.h"
#include "mat_lib.h"
#include "dsp_sub.h"
#include "pit_lib.h"
#include "melp_sub.h"
#include "cprv.h"
#include "pitch.h"
#include "global.h"
#include "ana_eval_modes.h"

static int32_t scalar(int mode, int32_t a, int32_t b, int32_t c, int32_t d)
{
	switch (mode) {
#define AE_S(id, name, call) case id: return (int32_t) (call);
	AE_SCALAR_MODES(AE_S)
#undef AE_S
	}
	return 0;
}

/* one case: row as given, o[0 .. AE_RET) zeroed; fills o */
static void run_case(int mode, const int16_t *row, const int32_t *a, int32_t *o)
{
	int16_t b[AE_WIN];
	int16_t pcorr = 0;
	int k, i;

	memset(b, 0, sizeof b);
	if (mode < AE_FIRST_STATEFUL)
		memcpy(b, row, sizeof b);
	switch (mode) {
	case 0:
		o[0] = f_pitch_scale(b + a[1], b + a[0], (int16_t) a[2]);
		break;
	case 1:
		o[2] = f_pitch_scale(b + a[0], b + a[0], AE_PW);
		o[0] = find_pitch(b + a[0] + AE_PC, &pcorr, (int16_t) a[2], (int16_t) a[3], (int16_t) a[4]);
		o[1] = pcorr;
		break;
	case 2:
		o[2] = f_pitch_scale(b + a[0], b + a[0], AE_PW);
		o[0] = frac_pch(b + a[0] + AE_PC, &pcorr, (int16_t) a[2], (int16_t) a[3], PITCHMIN, PITCHMAX,
				PITCHMIN_Q7, PITCHMAX_Q7, (int16_t) a[4]);
		o[1] = pcorr;
		break;
	case 3:
		o[0] = gain_ana(b + a[0], (int16_t) a[1], (int16_t) a[2], (int16_t) a[3]);
		break;
	case 4:
		o[0] = trackPitch((int16_t) a[1], (pitTrackParam *) (b + a[0]));
		break;
	case 5:
		o[0] = pitLookahead((pitTrackParam *) (b + a[0]), (int16_t) a[1]);
		break;
	case 6:
		for (k = 0; k < a[0]; k++) {
			memcpy(b, row + k * AE_STRIDE_PITCH_ANA, sizeof(int16_t) * AE_STRIDE_PITCH_ANA);
			o[k * AE_CALL] = pitch_ana(b + AE_PC, b + AE_PW + AE_PC, b[2 * AE_PW], b[2 * AE_PW + 1],
						   &pcorr);
			o[k * AE_CALL + 1] = pcorr;
		}
		break;
	case 7:
		for (k = 0; k < a[0]; k++) {
			memcpy(b, row + k * AE_STRIDE_P_AVG, sizeof(int16_t) * AE_STRIDE_P_AVG);
			o[k * AE_CALL] = p_avg_update(b[0], b[1], b[2]);
		}
		break;
	case 8:
		for (k = 0; k < a[0]; k++) {
			int16_t bpvc[NUM_BANDS] = { 0, 0, 0, 0, 0 };
			int16_t pitch = 0;
			memcpy(b, row + k * AE_STRIDE_BPVC, sizeof(int16_t) * AE_STRIDE_BPVC);
			bpvc_ana(b - (PITCH_FR - FRAME - PITCHMAX), b + FRAME, bpvc, &pitch);
			for (i = 0; i < NUM_BANDS; i++)
				o[k * AE_CALL + i] = bpvc[i];
			o[k * AE_CALL + NUM_BANDS] = pitch;
		}
		break;
	case 9:
		for (k = 0; k < a[0]; k++) {
			pitTrackParam pt;
			classParam cs;
			memset(&pt, 0, sizeof pt);
			memset(&cs, 0, sizeof cs);
			memcpy(b, row + k * AE_STRIDE_PAUTO, sizeof(int16_t) * AE_STRIDE_PAUTO);
			pitchAuto(b, &pt, &cs);
			for (i = 0; i < NODE; i++) {
				o[k * AE_CALL + i] = pt.pit[i];
				o[k * AE_CALL + NODE + i] = pt.weight[i];
			}
			o[k * AE_CALL + 2 * NODE] = cs.pitch;
			o[k * AE_CALL + 2 * NODE + 1] = cs.corx;
		}
		break;
	case 10:
		for (k = 0; k < a[0]; k++) {
			classParam cs[2];
			const int16_t *x = b + AE_CLS_SPAN + 17;
			int32_t *q = o + k * AE_CALL;
			memset(cs, 0, sizeof cs);
			memcpy(b, row + k * AE_STRIDE_CLASSIFY, sizeof(int16_t) * AE_STRIDE_CLASSIFY);
			cs[0].zeroCrosRate = x[0];
			cs[0].subEnergy = x[1];
			cs[1].pitch = x[2];
			cs[1].corx = x[3];
			if (k > 0) {
				voicedEn = x[4];
				silenceEn = x[5];
			}
			classify(b + AE_CLS_BACK, &cs[1], b + AE_CLS_SPAN);
			q[0] = cs[1].classy;
			q[1] = cs[1].subEnergy;
			q[2] = cs[1].zeroCrosRate;
			q[3] = cs[1].peakiness;
			q[4] = cs[1].corx;
			q[5] = cs[1].pitch;
			q[6] = voicedEn;
			q[7] = silenceEn;
			q[8] = voicedCnt;
		}
		break;
	}
	for (k = 0; k < AE_WIN; k++)
		o[AE_RET + k] = b[k];
}

/* run_case in a child process; 0 when the whole row came back */
static int run_forked(int mode, const int16_t *row, const int32_t *a, int32_t *o)
{
	int fd[2], status = 0;
	size_t got = 0;
	const size_t want = sizeof(int32_t) * AE_OUT;
	pid_t pid;

	if (pipe(fd) != 0)
		return -1;
	fflush(NULL);
	pid = fork();
	if (pid < 0)
		return -1;
	if (pid == 0) {
		size_t put = 0;
		close(fd[0]);
		run_case(mode, row, a, o);
		while (put < want) {
			ssize_t w = write(fd[1], (const char *) o + put, want - put);
			if (w <= 0)
				_exit(3);
			put += (size_t) w;
		}
		_exit(0);
	}
	close(fd[1]);
	while (got < want) {
		ssize_t r = read(fd[0], (char *) o + got, want - got);
		if (r <= 0)
			break;
		got += (size_t) r;
	}
	close(fd[0]);
	if (waitpid(pid, &status, 0) != pid)
		return -1;
	return (got == want && WIFEXITED(status) && WEXITSTATUS(status) == 0) ? 0 : -1;
}

static void *load(const char *path, size_t bytes)
{
	FILE *f = fopen(path, "rb");
	void *p = malloc(bytes ? bytes : 1);
	if (!f || !p || fread(p, 1, bytes, f) != bytes) {
		fprintf(stderr, "ref_ana: cannot read %zu bytes of %s\n", bytes, path);
		exit(2);
	}
	fclose(f);
	return p;
}

int main(int argc, char **argv)
{
	if (argc != 6) {
		fprintf(stderr, "usage: ref_ana v|s <mode> <n> <in> <out>\n");
		return 2;
	}
	const int mode = atoi(argv[2]);
	const long n = atol(argv[3]);
	long i;
	argv++;	/* argv[3], argv[4]: <in>, <out> */
	if (argv[0][0] == 's') {
		const int32_t *sa = load(argv[3], sizeof(int32_t) * 4 * n);
		int32_t *so = calloc(n ? n : 1, sizeof(int32_t));
		FILE *fs;
		if (mode < 0 || mode >= AE_SCALAR_COUNT || !so) {
			fprintf(stderr, "ref_ana: bad scalar mode %d\n", mode);
			return 2;
		}
		for (i = 0; i < n; i++)
			so[i] = scalar(mode, sa[4 * i], sa[4 * i + 1], sa[4 * i + 2], sa[4 * i + 3]);
		fs = fopen(argv[4], "wb");
		if (!fs || fwrite(so, sizeof(int32_t), n, fs) != (size_t) n) {
			fprintf(stderr, "ref_ana: cannot write %s\n", argv[4]);
			return 2;
		}
		fclose(fs);
		return 0;
	}
	char *raw = load(argv[3], (sizeof(int16_t) * AE_IN + sizeof(int32_t) * AE_ARGS) * n);
	const int16_t *in = (const int16_t *) raw;
	const int32_t *args = (const int32_t *) (raw + sizeof(int16_t) * AE_IN * n);
	const size_t out_words = (size_t) AE_OUT * n;
	int32_t *out = calloc(out_words ? out_words : 1, sizeof(int32_t));
	FILE *fo;

	if (mode < 0 || mode >= AE_MODE_COUNT || !out) {
		fprintf(stderr, "ref_ana: bad mode %d\n", mode);
		return 2;
	}
	for (i = 0; i < n; i++) {
		int32_t *o = out + (size_t) AE_OUT * i;
		if (mode < AE_FIRST_STATEFUL) {
			run_case(mode, in + (size_t) AE_IN * i, args + (size_t) AE_ARGS * i, o);
		} else if (run_forked(mode, in + (size_t) AE_IN * i, args + (size_t) AE_ARGS * i, o) != 0) {
			fprintf(stderr, "ref_ana: mode %d, case %ld: the child process died\n", mode, i);
			return 3;
		}
	}
	fo = fopen(argv[4], "wb");
	if (!fo || fwrite(out, sizeof(int32_t), out_words, fo) != out_words) {
		fprintf(stderr, "ref_ana: cannot write %s\n", argv[4]);
		return 2;
	}
	fclose(fo);
	return 0;
}
