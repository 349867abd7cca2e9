/*
 * hostemu.cpp -- host build of the engine's DEVICE sources, for CPU-side
 * tests only (tests/test_hostemu.py).  It runs the very same per-channel
 * code that the HIP kernels run (ops.h .. codec headers compiled with g++
 * instead of hipcc), one channel after another, so the kernel logic can be
 * checked against the reference oracle in a container without a GPU.
 *
 * NOT part of the product: libmelpe_amd.so never loads it, and nothing in
 * pairphone_amd/ imports it.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "codec.h"
#if !defined(MELPE_OPCOUNT)	/* the census counts the reference's serial order */
#include "ana_mw.h"
#endif
#include "helpers_eval.h"
#include "dsp_eval.h"
#include "ana_eval.h"
#include "codec2400.h"
#include "voice_crypt.h"
#include "link.h"
#include "vad.h"
#include "modem.h"
#include "rxline.h"

using namespace mlp;

struct emu_engine {
	int channels;
	std::vector<EncState> enc;
	std::vector<DecState> dec;
};

static NppScratch g_npp_scratch;

#if defined(MELPE_EXACT_STATS)
extern "C" { long melpe_exact_stats[6] = {0, 0, 0, 0, 0, 0}; }
#endif

#if defined(MELPE_OPCOUNT)
extern "C" {
uint64_t melpe_opcount[64];
uint64_t melpe_stagecount[64];
int melpe_opstage;
int melpe_opdepth;
}
#endif

extern "C" {

int emu_load_tables(const char *path)
{
	FILE *f = fopen(path, "rb");
	if (!f)
		return -1;
	size_t n = fread(g_tab, sizeof(int16_t), MELPE_TABLE_WORDS, f);
	fclose(f);
	if (n != MELPE_TABLE_WORDS)
		return -2;
	derive_all(&g_der);
	derive_lspgrid(g_der.lsp_cos, g_lspgrid);
	return 0;
}

emu_engine *emu_create(int channels)
{
	emu_engine *e = new emu_engine();
	e->channels = channels;
	e->enc.resize(channels);
	e->dec.resize(channels);
	for (int c = 0; c < channels; c++) {
		enc_reset(&e->enc[c]);
		dec_reset(&e->dec[c]);
	}
	return e;
}

void emu_destroy(emu_engine *e)
{
	delete e;
}

int emu_npp(emu_engine *e, int16_t *sp, int frames, int stride, int rate1200)
{
	for (int c = 0; c < e->channels; c++)
		for (int f = 0; f < frames; f++) {
			int16_t *x = sp + (size_t) c * stride + f * NPP_HOP;
			npp_frame(&e->enc[c].npp, &g_npp_scratch, x, x, rate1200 != 0);
		}
	return 0;
}

/* melpe_a on every channel: sp (C x 540) in/out, bits (C x 11) out */
int emu_encode(emu_engine *e, unsigned char *bits, int16_t *sp)
{
	for (int c = 0; c < e->channels; c++) {
		encode_superframe(&e->enc[c], &g_npp_scratch, sp + (size_t) c * BLOCK);
		for (int k = 0; k < 11; k++)
			bits[c * 11 + k] = e->enc[c].a.chbuf[k];
	}
	return 0;
}

/* the two halves of melpe_a, as the GPU runs them (k_enc_npp, k_enc_ana) */
int emu_encode_npp(emu_engine *e, int16_t *sp)
{
	for (int c = 0; c < e->channels; c++) {
		int16_t *x = sp + (size_t) c * BLOCK;
		for (int f = 0; f < NF; f++)
			npp_frame(&e->enc[c].npp, &g_npp_scratch, x + f * FRAME, x + f * FRAME);
	}
	return 0;
}

/* the split lane analysis as k_enc_ana / k_enc_quant / k_enc_harm /
 * k_enc_tail run it, each part on a frame of its own that holds what the
 * kernel is handed and a pattern everywhere else, with the Fourier
 * magnitudes from the scalar find_harm on the written residuals (the wave
 * kernel's own arithmetic is checked on the GPU) */
int emu_encode_ana_split(emu_engine *e, unsigned char *bits, const int16_t *sp)
{
	static int16_t res[NF * LPC_FRAME];
	static EncAna L;	/* the lane's private copy (k_ana.hip AnaLane) */
	static EncAna Q;	/* k_quant.hip QuantLane */
	/* the record ranges k_enc_quant moves: par + qpar, pvq_prev_uv_flag ..
	 * qplsp (the kernel widens the second to dwords; here it is exact) */
	const size_t o = offsetof(EncAna, par), n = offsetof(EncAna, voicedEn) - o;
	const size_t o2 = offsetof(EncAna, pvq_prev_uv_flag), n2 = offsetof(EncAna, fsm_prev_uv) - o2;
	for (int c = 0; c < e->channels; c++) {
		EncAna *E = &L, *R = &e->enc[c].a;
		/* k_enc_ana.  The live prefix in, the working storage a pattern
		 * (state.h): nothing may read it before writing it */
		memcpy(E, R, ENC_ANA_LIVE);
		memset((char *) E + ENC_ANA_LIVE, 0x5a + (c & 7), sizeof(EncAna) - ENC_ANA_LIVE);
		analysis_a1(E, sp + (size_t) c * BLOCK);
		/* the residual span goes out through the channel's row of res,
		 * whose tail it leaves alone */
		for (int k = 0; k < NF * LPC_FRAME; k++)
			res[k] = (int16_t) 0x5a5a;
		memcpy(res, &E->hpspeech[ANA_RES_BEG], sizeof(int16_t) * (ANA_RES_END - ANA_RES_BEG));
		ana_shift(E);
		memcpy(R, E, ENC_ANA_LIVE);
		/* k_enc_quant.  Its record ranges and the span in, the rest a
		 * pattern; the span is taken whole before any row is written */
		E = &Q;
		memset(E, 0xa5 - (c & 7), sizeof(EncAna));
		memcpy((char *) E + o, (const char *) R + o, n);
		memcpy((char *) E + o2, (const char *) R + o2, n2);
		memcpy(&E->hpspeech[ANA_RES_BEG], res, sizeof(int16_t) * (ANA_RES_END - ANA_RES_BEG));
		for (int k = 0; k < NF * LPC_FRAME; k++)
			res[k] = (int16_t) 0x5a5a;	/* every row but frame last's stays unread */
		analysis_q(E, res);
		memcpy((char *) R + o, (const char *) E + o, n);
		memcpy((char *) R + o2, (const char *) E + o2, n2);
		/* k_enc_harm and k_enc_tail, on the record: the unvoiced frames'
		 * 8192s and frame last's magnitudes; the other voiced frames' stay
		 * as the record holds them */
		E = R;
		for (int i = 0; i < NF; i++)
			if (E->par[i].uv_flag)
				v_set(E->par[i].fs_mag, 8192, NUM_HARM);
		const int last = fsmag_last(E->par);
		if (last >= 0)
			find_harm(&res[last * LPC_FRAME], E->par[last].fs_mag, E->par[last].pitch, NUM_HARM,
				  LPC_FRAME);
		analysis_b(E);
		for (int k = 0; k < 11; k++)
			bits[c * 11 + k] = E->chbuf[k];
	}
	return 0;
}

int emu_encode_ana(emu_engine *e, unsigned char *bits, const int16_t *sp)
{
	for (int c = 0; c < e->channels; c++) {
		analysis(&e->enc[c].a, sp + (size_t) c * BLOCK);
		for (int k = 0; k < 11; k++)
			bits[c * 11 + k] = e->enc[c].a.chbuf[k];
	}
	return 0;
}

/* the analysis in the reference's literal order, every voiced frame's
 * Fourier magnitudes computed, cut after `upto` stages (encoder.h
 * analysis_upto, what k_enc_ana_dbg runs): the independent form the product
 * forms above are compared with */
int emu_encode_ana_upto(emu_engine *e, unsigned char *bits, const int16_t *sp, int upto)
{
	for (int c = 0; c < e->channels; c++) {
		analysis_upto(&e->enc[c].a, sp + (size_t) c * BLOCK, upto);
		for (int k = 0; k < 11; k++)
			bits[c * 11 + k] = e->enc[c].a.chbuf[k];
	}
	return 0;
}

/* where the tests find fields in an exported encoder record (EncState), in
 * bytes: the analysis state, its live prefix's length, par[0], par's stride,
 * uv_flag within a par, fsm_prev_uv and chbuf within the analysis state;
 * returns how many there are */
int emu_enc_layout(long *out, int n)
{
	const long v[] = {(long) offsetof(EncState, a),       (long) ENC_ANA_LIVE,
			  (long) offsetof(EncAna, par),       (long) sizeof(MelpParam),
			  (long) offsetof(MelpParam, uv_flag), (long) offsetof(EncAna, fsm_prev_uv),
			  (long) offsetof(EncAna, chbuf)};
	const int m = (int) (sizeof v / sizeof v[0]);
	for (int i = 0; i < n && i < m; i++)
		out[i] = v[i];
	return m;
}

/* the live prefix of channel c's analysis state (ENC_ANA_LIVE bytes) */
long emu_enc_live(emu_engine *e, int c, unsigned char *out)
{
	memcpy(out, &e->enc[c].a, ENC_ANA_LIVE);
	return (long) ENC_ANA_LIVE;
}

#if !defined(MELPE_OPCOUNT)
/* the multi-wave analysis (ana_mw.h) as k_enc_ana_mw runs it: nw physical
 * waves, each with its own private copy of the record, phase by phase (the
 * barriers), the exchange block and the HBM record the only shared data;
 * each wave writes back the state groups of its virtual waves */
struct HostXch {
	int16_t w[XS_WORDS];
	int16_t get(int k) const { return w[k]; }
	void put(int k, int16_t v) { w[k] = v; }
};

/* lsf_vq's per-channel score row (HBM on the GPU) */
struct HostDb {
	uint32_t v[LQ_ROW];
	uint32_t get(int u) const { return v[u]; }
	void put(int u, uint32_t x) { v[u] = x; }
};

int emu_encode_ana_mw(emu_engine *e, unsigned char *bits, const int16_t *sp, int nw)
{
	if (nw < 1 || nw > MW_NV)
		return -1;
	std::vector<EncAna> W(nw);
	for (int c = 0; c < e->channels; c++) {
		EncAna &rec = e->enc[c].a;
		const int16_t *x = sp + (size_t) c * BLOCK;
		HostXch xc;
		memset(&xc, 0x5a, sizeof xc);	/* nothing may read a slot before it is written */
		static HostDb db;
		memset(&db, 0xa5, sizeof db);
		AnaMwTmp tmp[MW_NV];
		for (int w = 0; w < nw; w++) {
			memset(&W[w], 0xa5 + w, sizeof(EncAna));	/* uncopied bytes: a pattern */
			ana_mw_copy_in(&W[w], &rec, w, nw);
			ana_mw_begin(&W[w], x);
		}
		for (int p = 0; p < MW_PHASES; p++)
			for (int w = 0; w < nw; w++)
				for (int v = w; v < MW_NV; v += nw)
					ana_mw_phase(&W[w], &rec, xc, db, tmp[v], v, p);
		for (int w = 0; w < nw; w++)
			for (int v = w; v < MW_NV; v += nw) {
				size_t off[2], len[2];
				int n = ana_mw_owned(v, off, len);
				for (int k = 0; k < n; k++)
					memcpy((char *) &rec + off[k], (const char *) &W[w] + off[k], len[k]);
			}
		for (int k = 0; k < 11; k++)
			bits[c * 11 + k] = rec.chbuf[k];
	}
	return 0;
}
#endif

/* host build of the helper self-test (helpers_eval.h), same layout as
 * melpe_helpers_eval_dev */
int emu_helpers_eval(int mode, const int16_t *src, const int32_t *args, int32_t *out, int n)
{
	for (int i = 0; i < n; i++) {
		alignas(4) int16_t buf[HE_N];
		memcpy(buf, src + (size_t) i * HE_N, sizeof buf);
		int32_t *o = out + (size_t) i * HE_OUT;
		memset(o, 0, sizeof(int32_t) * HE_OUT);
		he_eval(mode, buf, args[4 * i], args[4 * i + 1], args[4 * i + 2], o);
	}
	return 0;
}

/* host build of the function-level parity test (dsp_eval.h), same layouts
 * as melpe_dsp_eval_dev / melpe_dsp_scalar_dev */
int emu_dsp_eval(int mode, const int16_t *in, const int32_t *args, int32_t *out, int n)
{
	if (mode < 0 || mode >= DE_MODE_COUNT)
		return -1;
	for (int i = 0; i < n; i++) {
		alignas(4) int16_t b[DE_IN];
		int32_t r[DE_RET] = {0};
		memcpy(b, in + (size_t) i * DE_IN, sizeof b);
		de_eval(mode, b, args + (size_t) i * DE_ARGS, r);
		int32_t *o = out + (size_t) i * DE_OUT;
		for (int k = 0; k < DE_RET; k++)
			o[k] = r[k];
		for (int k = 0; k < DE_IN; k++)
			o[DE_RET + k] = b[k];
	}
	return 0;
}

/* host build of the analysis parity test (ana_eval.h), same layouts as
 * melpe_ana_eval_dev */
int emu_ana_eval(int mode, const int16_t *in, const int32_t *args, int32_t *out, int n)
{
	if (mode < 0 || mode >= AE_MODE_COUNT)
		return -1;
	for (int i = 0; i < n; i++) {
		alignas(4) int16_t b[AE_WIN] = {0};
		int32_t r[AE_RET] = {0};
		EncAna E;
		memset(&E, 0, sizeof E);
		ae_eval(mode, in + (size_t) i * AE_IN, b, &E, args + (size_t) i * AE_ARGS, r);
		int32_t *o = out + (size_t) i * AE_OUT;
		for (int k = 0; k < AE_RET; k++)
			o[k] = r[k];
		for (int k = 0; k < AE_WIN; k++)
			o[AE_RET + k] = b[k];
	}
	return 0;
}

int emu_ana_scalar(int mode, const int32_t *args, int32_t *out, long n)
{
	if (mode < 0 || mode >= AE_SCALAR_COUNT)
		return -1;
	for (long i = 0; i < n; i++)
		out[i] = ae_scalar(mode, args[4 * i], args[4 * i + 1], args[4 * i + 2], args[4 * i + 3]);
	return 0;
}

int emu_dsp_scalar(int mode, const int32_t *args, int32_t *out, long n)
{
	if (mode < 0 || mode >= DE_SCALAR_COUNT)
		return -1;
	for (long i = 0; i < n; i++)
		out[i] = de_scalar(mode, args[4 * i], args[4 * i + 1], args[4 * i + 2], args[4 * i + 3]);
	return 0;
}

/* melpe_s on every channel: bits (C x 11) in, sp (C x 540) out */
int emu_decode(emu_engine *e, int16_t *sp, const unsigned char *bits)
{
	for (int c = 0; c < e->channels; c++) {
		DecState *D = &e->dec[c];
		memcpy(D->chbuf, bits + c * 11, 11);
		decode_superframe(D, sp + (size_t) c * BLOCK);
	}
	return 0;
}

/* the parse-only decoder as k_parse runs it (decoder.h parse_superframe):
 * bits (C x 11) in, melp_par as melpe_s leaves it (C x 3 x 30 int16) out.
 * The lane's copy holds the excitation side of the record only; the rest is
 * a pattern, which must come back untouched. */
int emu_parse(emu_engine *e, int16_t *par_out, const unsigned char *bits)
{
	static DecState W;
	for (int c = 0; c < e->channels; c++) {
		DecState *D = &e->dec[c];
		memset(&W, 0x5a + (c & 7), sizeof W);
		memcpy(&W, D, DEC_B_BEG);
		memcpy(W.chbuf, bits + (size_t) c * 11, 11);
		parse_superframe(&W);
		for (size_t k = DEC_B_BEG; k < sizeof W; k++)
			if (((const unsigned char *) &W)[k] != (unsigned char) (0x5a + (c & 7)))
				return -1;
		memcpy(D, &W, DEC_B_BEG);
		memcpy(par_out + (size_t) c * NF * 30, D->par, sizeof(D->par));
	}
	return 0;
}

#if !defined(MELPE_OPCOUNT)
}	/* extern "C": a template follows */

/* the two-wave decoder (decoder.h dec2_phase) as k_decode2 runs it: wave A
 * and wave B each on a private copy of the record, phase by phase, the two
 * hand-over buffers the only shared data; each writes back its own side */
struct HostHb {
	uint32_t *v;
	uint32_t get(int k) const { return v[k]; }
	void put(int k, uint32_t x) const { v[k] = x; }
};

/* the source of a superframe's parameters, as the kernels' (k_dec.hip BitsIn /
 * RowsIn): wave A takes channel c's input, wave B's copy of that field is a
 * pattern -- B never reads the channel or the rows */
struct HostBits {
	static constexpr bool ROWS = false;
	const unsigned char *bits;
	void take(DecState *A, DecState *B, int c) const
	{
		memcpy(A->chbuf, bits + c * 11, 11);
		memset(B->chbuf, 0xa5, 11);
	}
	void done(int, uint8_t) const {}
};

struct HostRows {
	static constexpr bool ROWS = true;
	const int16_t *par;
	uint8_t *status;
	void take(DecState *A, DecState *B, int c) const
	{
		memcpy(A->par, par + (size_t) c * NF * 30, sizeof(A->par));
		memset(B->par, 0xa5, sizeof(B->par));
	}
	void done(int c, uint8_t st) const
	{
		if (status)
			status[c] = st;
	}
};

template <class In>
static int emu_two(emu_engine *e, int16_t *sp, const In in)
{
	static uint32_t hb[2][HB_WORDS];
	static DecState W[2];
	for (int c = 0; c < e->channels; c++) {
		DecState *D = &e->dec[c];
		memset(hb, 0x5a, sizeof hb);	/* nothing may read a word before it is written */
		for (int r = 0; r < 2; r++)
			W[r] = *D;
		in.take(&W[0], &W[1], c);
		uint8_t st = 0;
		int16_t *out = sp + (size_t) c * BLOCK;
		for (int p = 0; p < DEC2_PHASES; p++)
			for (int r = 0; r < 2; r++)
				dec2_phase<HostHb, In::ROWS>(&W[r], out, HostHb{hb[0]}, HostHb{hb[1]}, r, p, W[r].par, &st);
		memcpy(D, &W[0], DEC_B_BEG);
		memcpy((char *) D + DEC_B_BEG, (const char *) &W[1] + DEC_B_BEG, sizeof(DecState) - DEC_B_BEG);
		in.done(c, st);
	}
	return 0;
}

extern "C" {

int emu_decode2(emu_engine *e, int16_t *sp, const unsigned char *bits)
{
	return emu_two(e, sp, HostBits{bits});
}

/* the two-wave synthesis from rows as k_synth_par2 runs it: wave A takes and
 * admits the rows (dec2_phase<Hb, true>) */
int emu_synth_params2(emu_engine *e, int16_t *sp, const int16_t *par, uint8_t *status)
{
	return emu_two(e, sp, HostRows{par, status});
}
#endif

/* synthesis() with SKIP_CHANNEL on every channel as k_synth_par runs it
 * (decoder.h synth_superframe): par (C x 3 x 30, read only) in, sp (C x 540)
 * and status (C bytes, may be null) out */
int emu_synth_params(emu_engine *e, int16_t *sp, const int16_t *par, uint8_t *status)
{
	for (int c = 0; c < e->channels; c++) {
		MelpParam rows[NF];
		uint8_t st = 0;
		memcpy(rows, par + (size_t) c * NF * 30, sizeof rows);
		synth_superframe(&e->dec[c], rows, sp + (size_t) c * BLOCK, &st);
		if (status)
			status[c] = st;
	}
	return 0;
}

/* The channel reader's rows before melp_syn's parameter head: emu_parse
 * (parse_superframe's steps, on the engine's records) with melp_par captured
 * between low_rate_chn_read and the head.  bits (C x 11) in; par (C x 3 x 30)
 * the pre-head rows and erase (C bytes) the reader's erasure flag out.  The
 * engine is a reader of its own: it advances as a parse-only decoder does. */
int emu_read_rows(emu_engine *e, int16_t *par_out, uint8_t *erase, const unsigned char *bits)
{
	for (int c = 0; c < e->channels; c++) {
		DecState *D = &e->dec[c];
		memcpy(D->chbuf, bits + (size_t) c * 11, 11);
		D->erase = low_rate_chn_read(D);
		memcpy(par_out + (size_t) c * NF * 30, D->par, sizeof(D->par));
		erase[c] = (uint8_t) (D->erase != 0);
		for (int i = 0; i < NF; i++) {
			syn_par_head<false>(D, &D->par[i]);
			D->prev_par = D->par[i];
		}
	}
	return 0;
}

/* the admission alone (decoder.h syn_row_admit) on n frame rows in place;
 * changed[i] = whether row i was clamped */
int emu_row_admit(int16_t *rows, uint8_t *changed, long n)
{
	for (long i = 0; i < n; i++)
		changed[i] = (uint8_t) syn_row_admit((MelpParam *) (rows + i * 30));
	return 0;
}

/* per-superframe debug view of channel c: melp_par (3 x 30 int16) and
 * quant_par (30 int16), in the layout oracle/ref_tool.c dumps */
int emu_enc_params(emu_engine *e, int c, int16_t *out)
{
	const EncAna *E = &e->enc[c].a;
	memcpy(out, E->par, sizeof(E->par));
	const QuantParam *q = &E->qpar;
	int16_t *w = out + 90;
	int k = 0;
	w[k++] = q->pitch_index;
	for (int i = 0; i < NF; i++)
		for (int j = 0; j < MAX_LSF_STAGE; j++)
			w[k++] = q->lsf_index[i][j];
	for (int i = 0; i < NUM_GAINFR; i++)
		w[k++] = q->gain_index[i];
	for (int i = 0; i < NF; i++)
		w[k++] = q->jit_index[i];
	for (int i = 0; i < NF; i++)
		w[k++] = q->bpvc_index[i];
	w[k++] = q->fs_index;
	for (int i = 0; i < NF; i++)
		w[k++] = q->uv_flag[i];
	for (int i = 0; i < MSVQ_STAGES; i++)
		w[k++] = q->msvq_index[i];
	w[k++] = q->fsvq_index;
	return k;
}

/* the single-stream engine's melp_par / quant_par / chbuf hand-over around
 * melpe_s (k_state.hip k_share_params), channel 0 */
int emu_share(emu_engine *e, int dir)
{
	EncAna *E = &e->enc[0].a;
	DecState *D = &e->dec[0];
	if (dir == 0) {
		memcpy(D->par, E->par, sizeof(D->par));
		D->qpar = E->qpar;
	} else {
		memcpy(E->par, D->par, sizeof(E->par));
		E->qpar = D->qpar;
		memcpy(E->chbuf, D->chbuf, 11);
	}
	return 0;
}

/* decoder's melp_par of channel c after the last superframe (3 x 30 int16) */
int emu_dec_params(emu_engine *e, int c, int16_t *out)
{
	memcpy(out, e->dec[c].par, sizeof(e->dec[c].par));
	return 90;
}

/* basic-op census (count build only): copies and clears the counters;
 * returns the number of ops, or -1 in a normal build */
int emu_opcount(uint64_t *out, int n)
{
#if defined(MELPE_OPCOUNT)
	for (int i = 0; i < n && i < 64; i++) {
		out[i] = melpe_opcount[i];
		melpe_opcount[i] = 0;
	}
	return 37;
#else
	(void) out;
	(void) n;
	return -1;
#endif
}

/* per-stage census (count build only): ops attributed to the innermost
 * PROF_SCOPE stage (index k+1; 0 = outside any stage); copies and clears */
int emu_stagecount(uint64_t *out, int n)
{
#if defined(MELPE_OPCOUNT)
	for (int i = 0; i < n && i < 64; i++) {
		out[i] = melpe_stagecount[i];
		melpe_stagecount[i] = 0;
	}
	return 64;
#else
	(void) out;
	(void) n;
	return -1;
#endif
}

const char *emu_op_names(void)
{
	return MELPE_OP_NAMES;
}


/* host build of the voice-frame crypt (voice_crypt.h), same layout as
 * melpe_voice_crypt_host */
int emu_voice_crypt(unsigned char *pkts, const uint32_t *counters, const unsigned char *keys,
		    const uint8_t *invert, int channels, int packets, int dir)
{
	for (int c = 0; c < channels; c++) {
		uint32_t key[4];
		memcpy(key, keys + 16 * (size_t) c, 16);
		for (int k = 0; k < packets; k++)
			vc_apply(pkts + ((size_t) c * packets + k) * VC_PKT_BYTES,
				 counters[c] + (uint32_t) k, key, dir, invert ? invert[c] : 0);
	}
	return 0;
}

/* host build of the link's packet layer (link.h), same layout and statuses
 * as melpe_link_tx_host / melpe_link_rx_host */
int emu_link_tx(unsigned char *state, unsigned char *pkts, const uint8_t *voiced, int32_t *ret,
		int channels, int packets, const uint8_t *active)
{
	LinkState *st = (LinkState *) state;
	for (int c = 0; c < channels; c++) {
		if (active && !active[c])
			continue;
		for (int k = 0; k < packets; k++) {
			const size_t i = (size_t) c * packets + k;
			ret[i] = link_make_ctr(&st[c], pkts + i * VC_PKT_BYTES, voiced ? voiced[i] : 0);
		}
	}
	return 0;
}

int emu_link_rx(unsigned char *state, unsigned char *pkts, int32_t *ret, uint8_t *voice, int channels,
		int packets, const uint8_t *active)
{
	LinkState *st = (LinkState *) state;
	for (int c = 0; c < channels; c++) {
		if (active && !active[c])
			continue;
		LinkRx R;
		link_rx_load(&R, &st[c]);
		for (int k = 0; k < packets; k++) {
			const size_t i = (size_t) c * packets + k;
			int r = LINK_STAGE;
			if (R.step >= 5) {
				uint64_t lo, hi;
				bool wr;
				link_pkt_load(pkts + i * VC_PKT_BYTES, &lo, &hi);
				r = link_process_ctr(&R, &lo, &hi, &wr);
				if (wr)
					link_pkt_store(pkts + i * VC_PKT_BYTES, lo, hi);
			}
			ret[i] = r;
			if (voice)
				voice[i] = r == -3;
		}
		if (R.step >= 5)
			link_rx_store(&st[c], &R);
	}
	return 0;
}

unsigned emu_golay_encode(unsigned m)
{
	return fec_golay2412_encode_symbol(m);
}

unsigned emu_golay_decode(unsigned r)
{
	return fec_golay2412_decode_symbol(r);
}

/* the sweep of melpe_golay_sweep_dev on the host */
int emu_golay_sweep(uint32_t *enc, uint64_t *digest)
{
	for (uint32_t m = 0; m < 4096; m++)
		enc[m] = fec_golay2412_encode_symbol(m);
	for (uint32_t b = 0; b < 256; b++) {
		uint64_t h = 0;
		for (uint32_t v = b << 16; v < (b + 1) << 16; v++)
			h += (uint64_t) fec_golay2412_decode_symbol(v) * ((uint64_t) v * 0x9E3779B97F4A7C15ull + 1u);
		digest[b] = h;
	}
	return 0;
}

#if defined(MELPE_OPCOUNT)
uint64_t melpe_vad_ops;
int melpe_vad_depth;
#endif

/* VAD basic-op census since the last call (count build only; else 0) */
uint64_t emu_vad_opcount(void)
{
#if defined(MELPE_OPCOUNT)
	uint64_t n = melpe_vad_ops;
	melpe_vad_ops = 0;
	return n;
#else
	return 0;
#endif
}

int emu_vad_state_bytes(void)
{
	return (int) sizeof(VadState);
}

/* host build of k_vad: `nsf` superframes of C channels, sp C x (nsf*540),
 * votes C x nsf, state C records (zeroed by the caller = vad2_reset) */
int emu_vad(unsigned char *state, const int16_t *sp, uint8_t *votes, int channels, int nsf)
{
	VadState *st = (VadState *) state;
	for (int c = 0; c < channels; c++)
		for (int k = 0; k < nsf; k++)
			votes[(size_t) c * nsf + k] = (uint8_t) va_superframe(
				sp + ((size_t) c * nsf + k) * 540, &st[c]);
	return 0;
}

/* 2400 bps mode (codec2400.h): sp C x 180 in/out (NPP at RATE2400, then
 * analysis), bits C x 7 out; decode bits C x 7 -> sp C x 180 */
int emu_encode2400(emu_engine *e, unsigned char *bits, int16_t *sp)
{
	for (int c = 0; c < e->channels; c++) {
		EncState *S = &e->enc[c];
		int16_t *x = sp + (size_t) c * FRAME;
		npp_frame(&S->npp, &g_npp_scratch, x, x, false);
		analysis24(&S->a, x);
		memcpy(bits + (size_t) c * R24_BYTES, S->a.chbuf, R24_BYTES);
	}
	return 0;
}

int emu_decode2400(emu_engine *e, int16_t *sp, const unsigned char *bits)
{
	for (int c = 0; c < e->channels; c++) {
		DecState *D = &e->dec[c];
		memcpy(D->chbuf, bits + (size_t) c * R24_BYTES, R24_BYTES);
		decode_frame24(D, sp + (size_t) c * FRAME);
	}
	return 0;
}

/* raw state records (test diagnostics): which 1 = EncState, 2 = DecState */
long emu_state_bytes(int which)
{
	return which == 1 ? (long) sizeof(EncState) : (long) sizeof(DecState);
}

int emu_export(emu_engine *e, int which, int c, void *out)
{
	if (which == 1)
		memcpy(out, &e->enc[c], sizeof(EncState));
	else
		memcpy(out, &e->dec[c], sizeof(DecState));
	return 0;
}

/* host build of the modem (modem.h) */
int emu_modem_state_bytes(void)
{
	return (int) sizeof(ModemState);
}

void emu_modem_reset(unsigned char *state, int channels)
{
	for (int c = 0; c < channels; c++)
		modem_reset((ModemState *) state + c);
}

/* pkts C x K x 11 -> pcm C x K x 3240 */
int emu_modulate(unsigned char *state, const uint8_t *pkts, int16_t *pcm, int channels, int packets)
{
	for (int c = 0; c < channels; c++) {
		ModemState *S = (ModemState *) state + c;
		for (int k = 0; k < packets; k++) {
			const uint8_t *d = pkts + ((size_t) c * packets + k) * 11;
			int16_t *o = pcm + ((size_t) c * packets + k) * MODEM_PKT_SAMPLES;
			int prev = S->lastb;
			for (int t = 0; t < MODEM_BITS; t++) {
				int b = modem_tx_bit(d, t);
				for (int ii = 0; ii < 36; ii++)
					o[t * 36 + ii] = modem_sample(b, prev, S->vadtr, ii);
				prev = b;
			}
			S->lastb = prev;
			S->vadtr ^= 1;
		}
	}
	return 0;
}

/* `calls` Demodulate calls per channel on pcm C x stride from pos[c];
 * data C x 12 in/out, out C x calls x 12, ret C x calls */
int emu_demodulate(unsigned char *state, const int16_t *pcm, long stride, int32_t *pos,
		   uint8_t *data, uint8_t *out, int32_t *ret, int channels, int calls)
{
	for (int c = 0; c < channels; c++) {
		ModemState *S = (ModemState *) state + c;
		for (int k = 0; k < calls; k++) {
			int32_t r = -1;
			if (pos[c] >= 0 && pos[c] + MODEM_LOOKAHEAD <= stride) {
				r = modem_demod(S, pcm + (size_t) c * stride + pos[c], data + 12 * (size_t) c);
				pos[c] += r;
			}
			for (int i = 0; i < 12; i++)
				out[((size_t) c * calls + k) * 12 + i] = data[12 * (size_t) c + i];
			ret[(size_t) c * calls + k] = r;
			if (r < 0)
				break;
		}
	}
	return 0;
}

/* host build of the receive loop (rxline.h), same layout as
 * melpe_rx_line_host: per active channel `calls` Demodulate calls with the
 * ready-block step between them, then slot by slot melpe_s or 540 zeros on
 * the engine's decoder records */
int emu_rx_line_state_bytes(void)
{
	return (int) sizeof(RxLineState);
}

int emu_rx_line(emu_engine *e, unsigned char *modem_state, unsigned char *link_state, unsigned char *rx_state,
		const int16_t *pcm, long stride, int32_t *pos, uint8_t *data, int16_t *sp, unsigned char *bits,
		uint8_t *voice, uint8_t *info, uint8_t *count, int calls, int slots, const uint8_t *active)
{
	const int C = e->channels;
	if (slots < calls / 15 + 2 || slots > 255)
		return -1;
	for (int c = 0; c < C; c++) {
		if (active && !active[c])
			continue;
		ModemState *S = (ModemState *) modem_state + c;
		LinkState *lk = (LinkState *) link_state + c;
		RxLineState *rx = (RxLineState *) rx_state + c;
		uint8_t *d = data + 12 * (size_t) c;
		int n = 0;
		for (int k = 0; k < calls; k++) {
			if (pos[c] < 0 || pos[c] + MODEM_LOOKAHEAD > stride)
				break;
			pos[c] += modem_demod(S, pcm + (size_t) c * stride + pos[c], d);
			if (!(d[11] & 0x80))
				continue;
			const RxLineEvent ev = rxline_block(d, lk, &rx->fber, &rx->fau);
			rx->blocks++;
			if (n < slots) {
				const size_t row = (size_t) n * C + c;
				uint32_t w[2];
				memcpy(bits + row * VC_PKT_BYTES, d, VC_PKT_BYTES);
				voice[row] = ev.kind == RXL_KIND_VOICE;
				rxline_info(&ev, k, &w[0], &w[1]);
				memcpy(info + row * RXL_INFO_BYTES, w, RXL_INFO_BYTES);
				n++;
			}
			d[11] = 0;
		}
		count[c] = (uint8_t) n;
		for (int j = 0; j < n; j++) {
			const size_t row = (size_t) j * C + c;
			int16_t *out = sp + row * BLOCK;
			if (voice[row]) {
				memcpy(e->dec[c].chbuf, bits + row * VC_PKT_BYTES, VC_PKT_BYTES);
				decode_superframe(&e->dec[c], out);
			} else {
				memset(out, 0, sizeof(int16_t) * BLOCK);
			}
		}
	}
	return 0;
}

}  // extern "C"
