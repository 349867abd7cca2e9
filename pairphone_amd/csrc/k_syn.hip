/*
 * k_syn.hip -- synthesis() of melpe/melp_syn.c:110-146 with the reference's
 * SKIP_CHANNEL switch on: per active channel, three frames of melp_syn on the
 * channel's decoder record from a [C, 3, 30] tensor of MELP parameters instead
 * of a channel word (decoder.h synth_superframe / dec2_phase<Hb, true>).
 *
 * The two kernels mirror k_dec.hip's: k_synth_par, one lane per channel, and
 * k_synth_par2, two waves per 64 channels (wave A takes and admits the rows
 * and synthesises the excitation, wave B filters one frame behind).  The lane's
 * 180-byte row is read straight from the tensor into the record's par[]: it is
 * 16% of the record's bytes in the same per-lane access pattern, and under a
 * permuted lane order the 64 rows of a wave are no contiguous run that LDS
 * staging could coalesce.
 */
#define MELPE_IDFT_LDS	/* realIDFT's table from LDS (decoder.h) */
#include "kern.h"
#include "../../include/melpe_batch.h"

MELPE_TU(syn)

#define SYN_BLOCK 256	/* as k_decode's DEC_BLOCK */
#define ROW_BYTES (sizeof(MelpParam) * NF)

static_assert(sizeof(MelpParam) == 2 * MELPE_PAR_WORDS, "the public row size (melpe_batch.h)");
static_assert(ROW_BYTES % 4 == 0 && offsetof(DecState, par) % 4 == 0, "rows move as dwords");

struct SynLane {
	uint8_t guard[FLAT_GUARD_BYTES];
	DecState S;
	int16_t out[BLOCK];
};

__global__ __launch_bounds__(SYN_BLOCK, MELPE_DEC_WAVES) void k_synth_par(DecState *dec, int16_t *sp,
							  const char *par, uint8_t *status,
							  const uint8_t *active, int n, const int *perm,
							  const int *nlive)
{
	for (int len = 1; len <= PITCHMAX; len++)
		for (int i = threadIdx.x; i < len; i += blockDim.x)
			s_idft_cos[((len - 1) * len) / 2 + i] = g_der.idft_cos[len][i];
	__syncthreads();
	int c = blockIdx.x * blockDim.x + threadIdx.x;
	if (perm) {
		if (c >= *nlive)
			return;
		c = perm[c];
	} else if (c >= n || (active && !active[c])) {
		return;
	}
	SynLane L;
	PIN_FRAME(L);
	static_assert(sizeof(DecState) % 16 == 0 && offsetof(SynLane, S) % 16 == 0, "16-byte record copy");
	lane_copy_x4(&L.S, &dec[c], sizeof(DecState));
	lane_copy(L.S.par, par + (size_t) c * ROW_BYTES, ROW_BYTES);
	uint8_t st;
	synth_superframe(&L.S, L.S.par, L.out, &st);
	lane_copy_x4(&dec[c], &L.S, sizeof(DecState));
	lane_copy(sp + (size_t) c * BLOCK, L.out, sizeof(int16_t) * BLOCK);
	if (status)
		status[c] = st;
}

/* the launch of k_synth_par over `lanes` channels, blocks sized as
 * k_decode's: the real one (n = lanes) and the warm-up (n = 0) */
static int launch_synth(int lanes, DecState *dec, int16_t *sp, const char *par, uint8_t *status,
			const uint8_t *active, int n, const int *perm, const int *nlive, hipStream_t s)
{
	int b = SYN_BLOCK;
	while (b > WAVE && (lanes + b - 1) / b < 1024)
		b /= 2;
	k_synth_par<<<(lanes + b - 1) / b, b, IDFT_LDS_WORDS * sizeof(int16_t), s>>>(dec, sp, par, status, active, n,
										    perm, nlive);
	return (int) hipGetLastError();
}

extern "C" int kl_synth_par(DecState *dec, int16_t *sp, const void *par, uint8_t *status, const uint8_t *active,
			    int n, const int *perm, const int *nlive, hipStream_t s)
{
	if (n <= 0)
		return 0;
	return launch_synth(n, dec, sp, (const char *) par, status, active, n, perm, nlive, s);
}

/* The two-wave form, laid out as k_decode2 (k_dec.hip): group, roles, the
 * hand-over buffers (the engine's d_hb, sized by kl_decode2_hb_words) and the
 * write-back of each side of the record by the wave that owns it. */
#ifndef DEC2_GROUPS
#define DEC2_GROUPS 2
#endif
#define SYN2_BLOCK (2 * WAVE * DEC2_GROUPS)

struct HbG {
	uint32_t *p;
	__device__ uint32_t get(int k) const { return p[(size_t) k * WAVE]; }
	__device__ void put(int k, uint32_t v) const { p[(size_t) k * WAVE] = v; }
};

__global__ __launch_bounds__(SYN2_BLOCK, MELPE_DEC_WAVES) void k_synth_par2(DecState *dec, int16_t *sp,
							    const char *par, uint8_t *status,
							    const uint8_t *active, int n, const int *perm,
							    const int *nlive, uint32_t *hbuf)
{
	for (int len = 1; len <= PITCHMAX; len++)
		for (int i = threadIdx.x; i < len; i += blockDim.x)
			s_idft_cos[((len - 1) * len) / 2 + i] = g_der.idft_cos[len][i];
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
	SynLane L;
	PIN_FRAME(L);
	uint8_t st = 0;
	if (live) {
		lane_copy_x4(&L.S, &dec[c], sizeof(DecState));
		if (role == 0)
			lane_copy(L.S.par, par + (size_t) c * ROW_BYTES, ROW_BYTES);
	}
	const HbG hb0{hbuf + (size_t) (2 * grp) * HB_WORDS * WAVE + t};
	const HbG hb1{hbuf + (size_t) (2 * grp + 1) * HB_WORDS * WAVE + t};
	for (int p = 0; p < DEC2_PHASES; p++) {
		if (live)
			dec2_phase<HbG, true>(&L.S, L.out, hb0, hb1, role, p, L.S.par, &st);
		__syncthreads();
	}
	if (live) {
		if (role == 0) {
			lane_copy_x4(&dec[c], &L.S, DEC_B_BEG);
			if (status)
				status[c] = st;
		} else {
			lane_copy_x4((char *) &dec[c] + DEC_B_BEG, (const char *) &L.S + DEC_B_BEG,
				     sizeof(DecState) - DEC_B_BEG);
			lane_copy(sp + (size_t) c * BLOCK, L.out, sizeof(int16_t) * BLOCK);
		}
	}
}

static unsigned syn2_grid(int n)
{
	const int per = WAVE * DEC2_GROUPS;
	return (unsigned) ((n + per - 1) / per);
}

/* hand-over dwords a launch over n channels indexes (the engine checks it
 * against the decoder's buffer) */
extern "C" size_t kl_synth_par2_hb_words(int n)
{
	return (size_t) syn2_grid(n) * DEC2_GROUPS * 2 * HB_WORDS * WAVE;
}

static int launch_synth2(int slots, DecState *dec, int16_t *sp, const char *par, uint8_t *status,
			 const uint8_t *active, int n, const int *perm, const int *nlive, uint32_t *hbuf,
			 hipStream_t s)
{
	k_synth_par2<<<syn2_grid(slots), SYN2_BLOCK, IDFT_LDS_WORDS * sizeof(int16_t), s>>>(dec, sp, par, status,
											    active, n, perm, nlive, hbuf);
	return (int) hipGetLastError();
}

extern "C" int kl_synth_par2(DecState *dec, int16_t *sp, const void *par, uint8_t *status, const uint8_t *active,
			     int n, const int *perm, const int *nlive, uint32_t *hbuf, hipStream_t s)
{
	if (n <= 0)
		return 0;
	return launch_synth2(n, dec, sp, (const char *) par, status, active, n, perm, nlive, hbuf, s);
}

extern "C" size_t kl_syn_private(void)
{
	return private_bytes((const void *) k_synth_par);
}

extern "C" size_t kl_syn2_private(void)
{
	return private_bytes((const void *) k_synth_par2);
}

extern "C" int kl_syn_warm(int n, hipStream_t s)
{
	return launch_synth(n, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, s);
}

extern "C" int kl_syn2_warm(int n, hipStream_t s)
{
	return launch_synth2(n, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, s);
}
