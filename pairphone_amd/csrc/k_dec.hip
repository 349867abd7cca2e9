/*
 * k_dec.hip -- the decoder family: one superframe of synthesis and postfilter
 * per active channel on the channel's decoder record, from either source of
 * parameters:
 *   BitsIn  melpe_s (melpe/melpe.c:102-107): the channel word is read
 *           (decoder.h decode_superframe) -- k_decode, k_decode2
 *   RowsIn  synthesis() of melpe/melp_syn.c:110-146 with the reference's
 *           SKIP_CHANNEL switch on: a [C, 3, 30] tensor of MELP parameters
 *           takes the channel word's place (decoder.h synth_superframe /
 *           dec2_phase<Hb, true>) -- k_synth_par, k_synth_par2
 * in either mapping: one lane per channel (dec_lane) or two waves per 64
 * channels (dec_two).  Each frame is written once, over the source; the four
 * kernels are its instances.
 */
#define MELPE_IDFT_LDS	/* realIDFT's table from LDS (decoder.h) */
#define MELPE_PROG_PRIO	/* progprio.h: DEC_CKPT in k_decode */
#include "kern.h"
#include "../../include/melpe_batch.h"

MELPE_TU(dec)

/* up to four waves per block share one LDS copy of the realIDFT table;
 * dec_launch picks the widest block that still gives every CU four blocks */
#define DEC_BLOCK 256
#define ROW_BYTES (sizeof(MelpParam) * NF)

static_assert(sizeof(MelpParam) == 2 * MELPE_PAR_WORDS, "the public row size (melpe_batch.h)");
static_assert(ROW_BYTES % 4 == 0 && offsetof(DecState, par) % 4 == 0, "rows move as dwords");

struct DecLane {
	uint8_t guard[FLAT_GUARD_BYTES];
	DecState S;
	int16_t out[BLOCK];
};
static_assert(sizeof(DecState) % 16 == 0 && offsetof(DecLane, S) % 16 == 0, "16-byte record copy");

/*
 * The source of a superframe's parameters, by value: take() brings channel
 * c's input into the lane's record, run() is the lane frame's superframe,
 * done() reports the admission status.  The members are MM (ops.h): inlined
 * by attribute like the codec's whole call tree, not by the optimiser's leave
 * -- left out of line, run() costs k_decode 192 bytes of scratch per lane.
 *
 * Progress-driven priority (progprio.h) belongs to BitsIn alone, as before
 * the two sources shared this file: synth_superframe holds no DEC_CKPT
 * (decoder.h), and a RowsIn kernel never runs PP_BEGIN, so it references
 * neither the counter nor its LDS words.
 */
struct BitsIn {
	static constexpr bool ROWS = false;
	const uint8_t *bits;	/* C x 11 */
	MM void take(DecState *S, int c) const
	{
		for (int k = 0; k < 11; k++)
			S->chbuf[k] = bits[(size_t) c * 11 + k];
	}
	MM void run(DecState *S, int16_t *out, uint8_t *) const { decode_superframe(S, out); }
	MM void done(int, uint8_t) const {}
};

/* The lane's 180-byte row is read straight from the tensor into the record's
 * par[]: it is 16% of the record's bytes in the same per-lane access pattern,
 * and under a permuted lane order the 64 rows of a wave are no contiguous run
 * that LDS staging could coalesce. */
struct RowsIn {
	static constexpr bool ROWS = true;
	const char *par;	/* C x 3 x 30 int16, read only */
	uint8_t *status;	/* C bytes, or null */
	MM void take(DecState *S, int c) const { lane_copy(S->par, par + (size_t) c * ROW_BYTES, ROW_BYTES); }
	MM void run(DecState *S, int16_t *out, uint8_t *st) const { synth_superframe(S, S->par, out, st); }
	MM void done(int c, uint8_t st) const
	{
		if (status)
			status[c] = st;
	}
};

/* every lane of the block, before its barrier */
__device__ __forceinline__ void idft_lds_fill(void)
{
	for (int len = 1; len <= PITCHMAX; len++)
		for (int i = threadIdx.x; i < len; i += blockDim.x)
			s_idft_cos[((len - 1) * len) / 2 + i] = g_der.idft_cos[len][i];
}

/* The lane frame: one lane per channel. */
template <class In>
__device__ __forceinline__ void dec_lane(DecState *dec, int16_t *sp, const In in, const uint8_t *active, int n,
					 const int *perm, const int *nlive, int prio)
{
	idft_lds_fill();
	if constexpr (!In::ROWS) {
		/* progprio.h: the counter is the sort's control word nlive[2] */
		if (perm)
			PP_BEGIN(prio ? (unsigned *) (nlive + 2) : nullptr, (*nlive + WAVE - 1) / WAVE);
		else
			PP_BEGIN(nullptr, 1);
	}
	__syncthreads();
	/* lane g runs channel perm[g] when the engine ordered the live
	 * channels (engine.hip, MELPE_BIN) */
	int c = blockIdx.x * blockDim.x + threadIdx.x;
	if (perm) {
		if (c >= *nlive)
			return;
		c = perm[c];
	} else if (c >= n || (active && !active[c])) {
		return;
	}
	DecLane L;
	PIN_FRAME(L);
	lane_copy_x4(&L.S, &dec[c], sizeof(DecState));
	in.take(&L.S, c);
	uint8_t st = 0;
	in.run(&L.S, L.out, &st);
	lane_copy_x4(&dec[c], &L.S, sizeof(DecState));
	lane_copy(sp + (size_t) c * BLOCK, L.out, sizeof(int16_t) * BLOCK);
	in.done(c, st);
}

__global__ __launch_bounds__(DEC_BLOCK, MELPE_DEC_WAVES) void k_decode(DecState *dec, int16_t *sp,
						      const uint8_t *bits, const uint8_t *active, int n,
						      const int *perm, const int *nlive, int prio)
{
	dec_lane(dec, sp, BitsIn{bits}, active, n, perm, nlive, prio);
}

__global__ __launch_bounds__(DEC_BLOCK, MELPE_DEC_WAVES) void k_synth_par(DecState *dec, int16_t *sp,
							  const char *par, uint8_t *status,
							  const uint8_t *active, int n, const int *perm,
							  const int *nlive)
{
	dec_lane(dec, sp, RowsIn{par, status}, active, n, perm, nlive, 0);
}

/*
 * The two-wave frame (decoder.h melp_syn_a / melp_syn_b): for channel
 * counts that leave SIMDs idle in lane mode (32,768 channels are 512 waves
 * for 1,024 SIMDs), each group of 64 channels gets two waves, lane t of both
 * on channel t, each wave on its own private copy of the record.  Wave A
 * takes the source in and synthesises each frame's excitation (the parameter
 * interpolation, harm_syn_pitch / realIDFT); wave B runs the synthesis
 * filters, scale_adj, the dispersion FIR and the postfilter one frame
 * behind, on what A handed over through a coalesced HBM buffer (word k of
 * lane t at k * 64 + t, two frame buffers per group).  A workgroup holds
 * DEC2_GROUPS groups sharing one LDS copy of the realIDFT table (only A
 * reads it).  Each wave writes back its own side of the record (state.h
 * DEC_B_BEG); A writes the status, B the PCM.
 */
#ifndef DEC2_GROUPS
#define DEC2_GROUPS 2
#endif
#define DEC2_BLOCK (2 * WAVE * DEC2_GROUPS)

struct HbG {
	uint32_t *p;
	__device__ uint32_t get(int k) const { return p[(size_t) k * WAVE]; }
	__device__ void put(int k, uint32_t v) const { p[(size_t) k * WAVE] = v; }
};

template <class In>
__device__ __forceinline__ void dec_two(DecState *dec, int16_t *sp, const In in, const uint8_t *active, int n,
					const int *perm, const int *nlive, uint32_t *hbuf)
{
	idft_lds_fill();
	if constexpr (!In::ROWS)
		PP_BEGIN(nullptr, 1);	/* no checkpoint is on its path; kept off all the same */
	__syncthreads();
	const int w = threadIdx.x / WAVE, t = threadIdx.x % WAVE;
	const int grp = blockIdx.x * DEC2_GROUPS + (w >> 1), role = w & 1;
	int c = grp * WAVE + t;
	bool live;
	if (perm) {
		live = c < *nlive;
		c = live ? perm[c] : 0;
	} else {
		live = c < n && (!active || active[c]);
	}
	DecLane L;
	PIN_FRAME(L);
	uint8_t st = 0;
	if (live) {
		lane_copy_x4(&L.S, &dec[c], sizeof(DecState));
		if (role == 0)
			in.take(&L.S, c);
	}
	const HbG hb0{hbuf + (size_t) (2 * grp) * HB_WORDS * WAVE + t};
	const HbG hb1{hbuf + (size_t) (2 * grp + 1) * HB_WORDS * WAVE + t};
	for (int p = 0; p < DEC2_PHASES; p++) {
		if (live)
			dec2_phase<HbG, In::ROWS>(&L.S, L.out, hb0, hb1, role, p, L.S.par, &st);
		__syncthreads();
	}
	if (live) {
		if (role == 0) {
			lane_copy_x4(&dec[c], &L.S, DEC_B_BEG);
			in.done(c, st);
		} else {
			lane_copy_x4((char *) &dec[c] + DEC_B_BEG, (const char *) &L.S + DEC_B_BEG,
				     sizeof(DecState) - DEC_B_BEG);
			lane_copy(sp + (size_t) c * BLOCK, L.out, sizeof(int16_t) * BLOCK);
		}
	}
}

__global__ __launch_bounds__(DEC2_BLOCK, MELPE_DEC_WAVES) void k_decode2(DecState *dec, int16_t *sp,
							const uint8_t *bits, const uint8_t *active, int n,
							const int *perm, const int *nlive, uint32_t *hbuf)
{
	dec_two(dec, sp, BitsIn{bits}, active, n, perm, nlive, hbuf);
}

__global__ __launch_bounds__(DEC2_BLOCK, MELPE_DEC_WAVES) void k_synth_par2(DecState *dec, int16_t *sp,
							    const char *par, uint8_t *status,
							    const uint8_t *active, int n, const int *perm,
							    const int *nlive, uint32_t *hbuf)
{
	dec_two(dec, sp, RowsIn{par, status}, active, n, perm, nlive, hbuf);
}

/* MELPE_DEC_PRIO=0: no progress-driven priority (progprio.h), for A/Bs */
static int dec_prio_mode(void)
{
	static const int v = env_int("MELPE_DEC_PRIO", 1) != 0;
	return v;
}

static unsigned dec2_grid(int n)
{
	const int per = WAVE * DEC2_GROUPS;
	return (unsigned) ((n + per - 1) / per);
}

/* hand-over buffer of a two-wave launch over n channels, in dwords */
extern "C" size_t kl_dec2_hb_words(int n)
{
	return (size_t) dec2_grid(n) * DEC2_GROUPS * 2 * HB_WORDS * WAVE;
}

/* the launch of the family's kernel for (waves, src) over `slots` channels:
 * the real one (n = slots) and the warm-up (n = 0: every lane exits at once,
 * or no lane is live).  The lane frame runs in the widest block that still
 * gives every CU four blocks. */
static int dec_launch(int waves, DecSrc src, int slots, DecState *dec, int16_t *sp, const uint8_t *active, int n,
		      const int *perm, const int *nlive, uint32_t *hbuf, hipStream_t s)
{
	const size_t lds = IDFT_LDS_WORDS * sizeof(int16_t);
	const uint8_t *bits = (const uint8_t *) src.in;
	const char *par = (const char *) src.in;
	if (waves == 2) {
		const unsigned g = dec2_grid(slots);
		if (src.rows)
			k_synth_par2<<<g, DEC2_BLOCK, lds, s>>>(dec, sp, par, src.status, active, n, perm, nlive, hbuf);
		else
			k_decode2<<<g, DEC2_BLOCK, lds, s>>>(dec, sp, bits, active, n, perm, nlive, hbuf);
	} else {
		int b = DEC_BLOCK;
		while (b > WAVE && (slots + b - 1) / b < 1024)
			b /= 2;
		const unsigned g = (unsigned) ((slots + b - 1) / b);
		if (src.rows)
			k_synth_par<<<g, b, lds, s>>>(dec, sp, par, src.status, active, n, perm, nlive);
		else
			k_decode<<<g, b, lds, s>>>(dec, sp, bits, active, n, perm, nlive, dec_prio_mode());
	}
	return (int) hipGetLastError();
}

extern "C" int kl_dec(int waves, DecSrc src, DecState *dec, int16_t *sp, const uint8_t *active, int n,
		      const int *perm, const int *nlive, uint32_t *hbuf, hipStream_t s)
{
	if (n <= 0)
		return 0;
	return dec_launch(waves, src, n, dec, sp, active, n, perm, nlive, hbuf, s);
}

extern "C" size_t kl_dec_private(int waves, int rows)
{
	return private_bytes(waves == 2 ? (rows ? (const void *) k_synth_par2 : (const void *) k_decode2)
					: (rows ? (const void *) k_synth_par : (const void *) k_decode));
}

extern "C" int kl_dec_warm(int waves, int rows, int n, hipStream_t s)
{
	return dec_launch(waves, DecSrc{rows, nullptr, nullptr}, n, nullptr, nullptr, nullptr, 0, nullptr, nullptr,
			  nullptr, s);
}
