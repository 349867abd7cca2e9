/*
 * k_state.hip -- the engine's own kernels on the channel records: reset,
 * melpe_i, the parameter sharing of the single-stream drop-in, the synthetic
 * test-signal generator (synth.h), and the lane-order sort.  None of them
 * reads the codec's constant tables, so the TU carries no copy of them (no
 * MELPE_TU).
 */
#include "kern.h"
#define SYN_FN __host__ __device__ static inline
#include "synth.h"

/* ------------------------------------------------------------------ */
/* small kernels: reset, init, parameter sharing, test-signal synth   */
/* ------------------------------------------------------------------ */

__global__ __launch_bounds__(WAVE) void k_reset(EncState *enc, DecState *dec,
						 const uint8_t *mask, int n, int which)
{
	int c = blockIdx.x * WAVE + threadIdx.x;
	if (c >= n || (mask && !mask[c]))
		return;
	if (which & 1)
		enc_reset(&enc[c]);
	if (which & 2)
		dec_reset(&dec[c]);
}

/* melpe_i on channel 0 of the single-stream engine: melp_ana_init +
 * melp_syn_init (melpe/melpe.c:72-88) */
__global__ void k_melpe_i(EncState *enc, DecState *dec)
{
	if (threadIdx.x == 0) {
		enc_melpe_i(&enc->a);
		dec_melpe_i(dec);
	}
}

/* The reference's analysis and synthesis share melp_par, quant_par and chbuf
 * (melpe/global.c:27-39).  For the single-stream drop-in the engine keeps
 * them in EncState and hands them to the decoder around each melpe_s, so an
 * interleaved melpe_a / melpe_s sequence sees exactly the reference's
 * process-global state.  dir 0: encoder -> decoder, 1: decoder -> encoder. */
__global__ void k_share_params(EncState *enc, DecState *dec, int dir)
{
	if (threadIdx.x != 0)
		return;
	EncAna *a = &enc->a;
	if (dir == 0) {
		for (int i = 0; i < NF; i++)
			dec->par[i] = a->par[i];
		dec->qpar = a->qpar;
	} else {
		for (int i = 0; i < NF; i++)
			a->par[i] = dec->par[i];
		a->qpar = dec->qpar;
		for (int k = 0; k < 11; k++)
			a->chbuf[k] = dec->chbuf[k];
	}
}

__global__ __launch_bounds__(WAVE) void k_synth_seed(synth_state *s, uint32_t seed,
						      uint32_t ch0, int n)
{
	int c = blockIdx.x * WAVE + threadIdx.x;
	if (c < n)
		synth_init(&s[c], synth_mix(seed, ch0 + (uint32_t) c));
}

__global__ __launch_bounds__(WAVE) void k_synth(synth_state *s, int16_t *out, int samples, int n)
{
	int c = blockIdx.x * WAVE + threadIdx.x;
	if (c >= n)
		return;
	synth_state st = s[c];
	synth_block(&st, out + (size_t) c * samples, samples);
	s[c] = st;
}

/*
 * Lane order by pitch class (MELPE_BIN, default on).
 *
 * k_enc_ana and k_decode run one channel per lane, and their loops follow
 * each channel's own pitch period and voicing: a synthesis period costs
 * O(L^2) in realIDFT and a frame holds 180/L of them, the analysis windows
 * and harmonic counts follow the pitch, and unvoiced frames take other
 * branches.  A wave pays the slowest of its 64 channels in every such loop.
 * So before each launch the live channels are counting-sorted into 568
 * classes -- voiced frames of the channel's last superframe (0..3) x its last
 * pitch in 1-sample steps -- and lane g of the kernel runs channel perm[g];
 * lanes at or past the live count exit at once, so a ragged mask also packs
 * the live channels into the fewest waves.  Each channel's arithmetic is
 * untouched (the order only decides which channels share a wave), so the
 * output is the same bit for bit; the order within a class follows the
 * atomics and is not reproducible, which nothing depends on.
 */
#define BIN_PITCHES 142	/* pitch classes: 20 .. 161 samples in 1-sample steps */
static_assert(4 * BIN_PITCHES <= NBIN, "every class has a counter");
#define NOT_LIVE 0xffff	/* the key of a channel that is not live */
static_assert(NBIN < NOT_LIVE, "class ids and the not-live mark must fit the uint16 keys");

/* the class of one record, from its last superframe: the voiced frames
 * (quant_par uv_flag, 0 = voiced) and the pitch (Q7) of its last frame, in
 * 1-sample steps.  Coarser steps (2, 3, 5 samples) and the mean pitch lost
 * to this key in round 5 on MI355X at 262,144 channels, two runs each
 * (profiles/r05_s_keys.txt): k_decode 8.52 -> 8.39 ms and the analysis
 * 31.11 -> 31.01 ms from the 3-sample key to this one. */
__device__ __forceinline__ int bin_class(const char *rec, int off_par, int off_uv)
{
	const int16_t *uv = (const int16_t *) (rec + off_uv);
	const int nv = (uv[0] == 0) + (uv[1] == 0) + (uv[2] == 0);
	int b = (*(const int16_t *) (rec + off_par + (NF - 1) * sizeof(MelpParam)) >> 7) - 20;
	b = b < 0 ? 0 : (b > BIN_PITCHES - 1 ? BIN_PITCHES - 1 : b);
	return nv * BIN_PITCHES + b;
}

/* The second lane order of the encoder (KEY_VOICING): the class of a record
 * is the voicing pattern of the superframe being encoded, the uv_flags of
 * par[0..2] as k_enc_ana's sc_ana left them (quant.h lsf_uvc: frame 0 in bit
 * 2), 8 classes.  lsf_vq, quant_fsmag and the residual loop branch on it. */
__device__ __forceinline__ int bin_class_uvc(const char *rec, int off_par)
{
	const MelpParam *par = (const MelpParam *) (rec + off_par);
	return (par[0].uv_flag ? 4 : 0) | (par[1].uv_flag ? 2 : 0) | (par[2].uv_flag ? 1 : 0);
}

/* The lane order of the synthesis from parameter rows (KEY_ROWS): there
 * the superframe being synthesised is known before the launch, so the class
 * is cut by it, not by the previous one as bin_class must for k_decode -- the
 * voiced frames among the rows' uv_flags and the pitch the last frame will be
 * synthesised with (an unvoiced frame runs at UV_PITCH_Q7, decoder.h
 * syn_par_head), in 1-sample steps.  The rows are read as the caller left
 * them, before admission: any value lands in a class. */
__device__ __forceinline__ int bin_class_rows(const char *row)
{
	const MelpParam *par = (const MelpParam *) row;
	const int nv = (par[0].uv_flag == 0) + (par[1].uv_flag == 0) + (par[2].uv_flag == 0);
	int b = ((par[NF - 1].uv_flag ? UV_PITCH_Q7 : par[NF - 1].pitch) >> 7) - 20;
	b = b < 0 ? 0 : (b > BIN_PITCHES - 1 ? BIN_PITCHES - 1 : b);
	return nv * BIN_PITCHES + b;
}

template <int KEY>
__global__ __launch_bounds__(256) void k_bin_count(const char *rec, size_t stride, int off_par,
						   int off_uv, const uint8_t *active, int n, BinBuf b)
{
	__shared__ unsigned cnt[NBIN];
	for (int k = threadIdx.x; k < NBIN; k += blockDim.x)
		cnt[k] = 0;
	__syncthreads();
	int c = blockIdx.x * blockDim.x + threadIdx.x;
	if (c < n) {
		int k = NOT_LIVE;
		if (!active || active[c]) {
			k = KEY == KEY_VOICING ? bin_class_uvc(rec + (size_t) c * stride, off_par)
			    : KEY == KEY_ROWS  ? bin_class_rows(rec + (size_t) c * stride + off_par)
					       : bin_class(rec + (size_t) c * stride, off_par, off_uv);
			atomicAdd(&cnt[k], 1u);
		}
		b.key[c] = (uint16_t) k;
	}
	__syncthreads();
	for (int k = threadIdx.x; k < NBIN; k += blockDim.x)
		if (cnt[k])
			atomicAdd(&b.ctl[k], cnt[k]);
}

__global__ void k_bin_scan(BinBuf b)
{
	if (threadIdx.x == 0) {
		unsigned acc = 0;
		for (int k = 0; k < NBIN; k++) {
			b.ctl[NBIN + k] = acc;
			acc += b.ctl[k];
		}
		b.ctl[2 * NBIN] = acc;
		b.ctl[2 * NBIN + 1] = 0;	/* the mapping tag: the launch that runs sets it */
		b.ctl[2 * NBIN + 2] = 0;	/* the lane kernels' progress counter (k_ana.hip ana_ckpt) */
	}
}

__global__ __launch_bounds__(256) void k_bin_scatter(int n, BinBuf b)
{
	__shared__ unsigned cnt[NBIN], base[NBIN];
	for (int k = threadIdx.x; k < NBIN; k += blockDim.x)
		cnt[k] = 0;
	__syncthreads();
	int c = blockIdx.x * blockDim.x + threadIdx.x;
	int k = c < n ? b.key[c] : NOT_LIVE;
	unsigned r = 0;
	if (k != NOT_LIVE)
		r = atomicAdd(&cnt[k], 1u);
	__syncthreads();
	for (int j = threadIdx.x; j < NBIN; j += blockDim.x)
		if (cnt[j])
			base[j] = atomicAdd(&b.ctl[NBIN + j], cnt[j]);
	__syncthreads();
	if (k != NOT_LIVE)
		b.perm[base[k] + r] = c;
}

/* ------------------------------------------------------------------ */
/* launchers (launch.h)                                                */
/* ------------------------------------------------------------------ */

extern "C" int kl_reset(EncState *enc, DecState *dec, const uint8_t *mask, int n, int which, hipStream_t s)
{
	k_reset<<<grid_for(n), WAVE, 0, s>>>(enc, dec, mask, n, which);
	return (int) hipGetLastError();
}

extern "C" int kl_melpe_i(EncState *enc, DecState *dec, hipStream_t s)
{
	k_melpe_i<<<1, WAVE, 0, s>>>(enc, dec);
	return (int) hipGetLastError();
}

extern "C" int kl_share_params(EncState *enc, DecState *dec, int dir, hipStream_t s)
{
	k_share_params<<<1, WAVE, 0, s>>>(enc, dec, dir);
	return (int) hipGetLastError();
}

extern "C" int kl_synth_seed(synth_state *syn, uint32_t seed, uint32_t ch0, int n, hipStream_t s)
{
	k_synth_seed<<<grid_for(n), WAVE, 0, s>>>(syn, seed, ch0, n);
	return (int) hipGetLastError();
}

extern "C" int kl_synth(synth_state *syn, int16_t *out, int samples, int n, hipStream_t s)
{
	k_synth<<<grid_for(n), WAVE, 0, s>>>(syn, out, samples, n);
	return (int) hipGetLastError();
}

extern "C" int kl_bin_sort(int key, const char *rec, size_t stride, int off_par, int off_uv,
			   const uint8_t *active, int n, BinBuf b, hipStream_t s)
{
	unsigned g = (unsigned) ((n + 255) / 256);
	if (key == KEY_VOICING)
		k_bin_count<KEY_VOICING><<<g, 256, 0, s>>>(rec, stride, off_par, off_uv, active, n, b);
	else if (key == KEY_ROWS)
		k_bin_count<KEY_ROWS><<<g, 256, 0, s>>>(rec, stride, off_par, off_uv, active, n, b);
	else
		k_bin_count<KEY_PITCH><<<g, 256, 0, s>>>(rec, stride, off_par, off_uv, active, n, b);
	MELPE_CHK(hipGetLastError());
	k_bin_scan<<<1, WAVE, 0, s>>>(b);
	MELPE_CHK(hipGetLastError());
	k_bin_scatter<<<g, 256, 0, s>>>(n, b);
	return (int) hipGetLastError();
}
