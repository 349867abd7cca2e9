/*
 * k_line.hip -- the line side, between the codec's bits and the line
 * samples: the voice-frame crypt (voice_crypt.h), the VAD (vad.h), the
 * VAD-framed stream format (stream_fmt.h), the modem (modem.h) and the
 * receive loop (rxline.h).  None of these kernels reads the codec's constant
 * tables, so the TU carries no copy of them (no MELPE_TU), like k_link.hip;
 * kern.h is included for the lane conventions (WAVE, the frame guard, the
 * 16-byte copies).
 */
#include "kern.h"
#include "voice_crypt.h"
#include "vad.h"
#include "stream_fmt.h"
#define MODEM_FN __host__ __device__ static inline
#include "modem.h"
#include "rxline.h"
#include "../../include/melpe_batch.h"

/* VoiceEnc / VoiceDec (crp.c:986-1027, voice_crypt.h), one lane per packet:
 * packet k of channel c is pkts[(c*K + k)*11 ..], its counter counters[c] + k
 * (cnt_out / cnt_in advance by one per packet, crp.c:805), its key the
 * channel's 16 bytes keys[c*16 ..] */
__global__ __launch_bounds__(256) void k_voice_crypt(unsigned char *pkts, const uint32_t *counters,
						     const uint4 *keys, const uint8_t *invert,
						     int channels, int packets, int dir)
{
	long i = blockIdx.x * (long) blockDim.x + threadIdx.x;
	if (i >= (long) channels * packets)
		return;
	int c = (int) (i / packets), k = (int) (i - (long) c * packets);
	uint4 kv = keys[c];
	uint32_t key[4] = {kv.x, kv.y, kv.z, kv.w};
	unsigned char *p = pkts + i * VC_PKT_BYTES;
	unsigned char b[VC_PKT_BYTES];
#pragma unroll
	for (int j = 0; j < VC_PKT_BYTES; j++)
		b[j] = p[j];
	vc_apply(b, counters[c] + (uint32_t) k, key, dir, invert ? invert[c] : 0);
#pragma unroll
	for (int j = 0; j < VC_PKT_BYTES; j++)
		p[j] = b[j];
}


/* VAD of one superframe per channel (vad.h): the six vad2 windows of
 * tx.c:234-239 on the channel's 540 samples; votes[c] = their sum */
__global__ __launch_bounds__(WAVE) void k_vad(VadState *st, const int16_t *sp, uint8_t *votes,
					      uint8_t *gate, const uint8_t *active, int channels)
{
	int c = blockIdx.x * blockDim.x + threadIdx.x;
	if (c >= channels)
		return;
	if (active && !active[c]) {
		if (gate)
			gate[c] = 0;
		return;
	}
	VadState s = st[c];
	int n = va_superframe(sp + (size_t) c * MELPE_SF_SAMPLES, &s);
	st[c] = s;
	votes[c] = (uint8_t) n;
	if (gate)	/* tx.c:242-244: encoded when any window voted */
		gate[c] = n > 0;
}

__global__ __launch_bounds__(WAVE) void k_vad_reset(VadState *st, const uint8_t *mask, int channels)
{
	int c = blockIdx.x * blockDim.x + threadIdx.x;
	if (c >= channels || (mask && !mask[c]))
		return;
	VadState z;
	memset(&z, 0, sizeof z);
	st[c] = z;
}

/*
 * The VAD-framed stream format on the device (stream_fmt.h).
 *
 * melpe_stream_pack_dev compacts one superframe's frames across channels:
 * channel c's frame of len(c) = 11, 1 or 0 bytes goes to out[offs[c] ..],
 * offs = the exclusive prefix sum of len.  The scan is three launches, so no
 * workgroup ever waits for another: k_stream_len writes each block's total
 * to work[], k_stream_scan (one block) turns work[] into the blocks' bases,
 * tile after tile of STREAM_BLOCK totals with a running carry, and
 * k_stream_scatter scans its block again, adds the block's base and writes
 * the frames.  Lengths are recomputed from votes and active in both passes,
 * not stored.
 */
#define STREAM_BLOCK 256
static_assert(STREAM_BLOCK % WAVE == 0 && WAVE == 64, "the scans below are written for wave64");

/* inclusive prefix sum over the wave's 64 lanes, on the DPP lane network:
 * row_shr:1,2,4,8 scan each row of 16 lanes (bound_ctrl: a lane shifted in
 * from outside the row reads 0), row_bcast:15 adds a row's total to the next
 * row (rows 1 and 3), row_bcast:31 adds the lower half's total to rows 2 and
 * 3.  Every lane of the wave must be active. */
__device__ static inline unsigned wave_scan_incl(unsigned v)
{
	v += (unsigned) __builtin_amdgcn_update_dpp(0, (int) v, 0x111, 0xf, 0xf, true);
	v += (unsigned) __builtin_amdgcn_update_dpp(0, (int) v, 0x112, 0xf, 0xf, true);
	v += (unsigned) __builtin_amdgcn_update_dpp(0, (int) v, 0x114, 0xf, 0xf, true);
	v += (unsigned) __builtin_amdgcn_update_dpp(0, (int) v, 0x118, 0xf, 0xf, true);
	v += (unsigned) __builtin_amdgcn_update_dpp(0, (int) v, 0x142, 0xa, 0xf, false);
	v += (unsigned) __builtin_amdgcn_update_dpp(0, (int) v, 0x143, 0xc, 0xf, false);
	return v;
}

/* exclusive prefix sum of v over the block's STREAM_BLOCK lanes, *total =
 * their sum; called by every lane of the block.  A caller that loops
 * synchronises the block before the next call (wsum is reused). */
__device__ static inline unsigned block_scan_excl(unsigned v, unsigned *total)
{
	__shared__ unsigned wsum[STREAM_BLOCK / WAVE];
	const unsigned inc = wave_scan_incl(v);
	const int w = threadIdx.x / WAVE;
	if ((threadIdx.x & (WAVE - 1)) == WAVE - 1)
		wsum[w] = inc;
	__syncthreads();
	unsigned base = 0, t = 0;
#pragma unroll
	for (int k = 0; k < STREAM_BLOCK / WAVE; k++) {
		const unsigned s = wsum[k];
		base += k < w ? s : 0u;
		t += s;
	}
	*total = t;
	return base + inc - v;
}

__global__ __launch_bounds__(STREAM_BLOCK) void k_stream_len(const uint8_t *votes, const uint8_t *active,
							     uint32_t *work, int channels)
{
	const long c = blockIdx.x * (long) STREAM_BLOCK + threadIdx.x;
	const unsigned len = c < channels ? sfmt_frame_len(!active || active[c], votes[c]) : 0u;
	unsigned total;
	block_scan_excl(len, &total);
	if (threadIdx.x == 0)
		work[blockIdx.x] = total;
}

__global__ __launch_bounds__(STREAM_BLOCK) void k_stream_scan(uint32_t *work, unsigned nb)
{
	unsigned carry = 0;
	for (unsigned t0 = 0; t0 < nb; t0 += STREAM_BLOCK) {	/* uniform: every lane runs every tile */
		const unsigned i = t0 + threadIdx.x;
		const unsigned v = i < nb ? work[i] : 0u;
		unsigned total;
		const unsigned ex = block_scan_excl(v, &total);
		if (i < nb)
			work[i] = carry + ex;
		carry += total;
		__syncthreads();
	}
}

__global__ __launch_bounds__(STREAM_BLOCK) void k_stream_scatter(const unsigned char *bits, const uint8_t *votes,
								 uint8_t *last, unsigned char *out, uint32_t *offs,
								 const uint32_t *work, int channels,
								 const uint8_t *active)
{
	const long c = blockIdx.x * (long) STREAM_BLOCK + threadIdx.x;
	const bool in = c < channels;
	const unsigned vote = in ? votes[c] : 0u;
	const unsigned len = in ? sfmt_frame_len(!active || active[c], vote) : 0u;
	unsigned total;
	const unsigned off = work[blockIdx.x] + block_scan_excl(len, &total);
	if (!in)
		return;
	offs[c] = off;
	if (c == channels - 1)
		offs[channels] = off + len;
	if (len)	/* off + len <= the total <= channels * 11, out's capacity */
		last[c] = sfmt_pack(bits + c * SFMT_BYTES, vote, last[c], out + off);
}

/* melpe_dec.c:33-49, the parse of one frame per channel: channel c's frame
 * starts at stream[pos[c]] and its stream ends at end[c].  pos_next may be
 * pos itself (a lane touches only its own slot), hence no restrict. */
__global__ __launch_bounds__(STREAM_BLOCK) void k_stream_parse(const unsigned char *stream, const uint32_t *pos,
							       const uint32_t *end, uint32_t *pos_next,
							       unsigned char *bits, uint8_t *voiced, uint8_t *lens,
							       const uint8_t *active, int channels)
{
	const long c = blockIdx.x * (long) STREAM_BLOCK + threadIdx.x;
	if (c >= channels)
		return;
	const uint32_t p = pos[c];
	unsigned len = 0;
	if ((!active || active[c]) && p < end[c]) {
		const unsigned char *f = stream + p;
		unsigned char *b = bits + c * SFMT_BYTES;
		len = sfmt_rx_len(f[0], end[c] - p);
		if (len == 1) {
#pragma unroll
			for (int j = 0; j < SFMT_BYTES; j++)
				b[j] = 0;
		} else if (len == SFMT_BYTES) {
			sfmt_unswap(f, b);
		}
	}
	lens[c] = (uint8_t) len;
	voiced[c] = len == SFMT_BYTES;
	if (pos_next)
		pos_next[c] = p + (len == SFMT_TRUNCATED ? 0u : len);
}

/* melpe_dec.c:37: 540 zero samples for the channels the parse found silent,
 * one wave per channel, 8 bytes per lane and store */
static_assert(MELPE_SF_SAMPLES * sizeof(int16_t) % sizeof(uint2) == 0, "a channel's PCM row in 8-byte words");
__global__ __launch_bounds__(STREAM_BLOCK) void k_stream_zero(uint2 *sp, const uint8_t *lens, int channels)
{
	const int words = (int) (MELPE_SF_SAMPLES * sizeof(int16_t) / sizeof(uint2));
	const long c = blockIdx.x * (long) (STREAM_BLOCK / WAVE) + threadIdx.x / WAVE;
	if (c >= channels || lens[c] != 1)
		return;
	uint2 *row = sp + c * words;
	for (int i = threadIdx.x & (WAVE - 1); i < words; i += WAVE)
		row[i] = make_uint2(0u, 0u);
}

/* Modulate (modem.h, modem/modem.c:136): one wave per (channel, packet).
 * The packet's starting state follows from the channel's state at launch:
 * the previous bit is the last bit of the previous packet (its parity bit
 * 89) and the muting flag alternates per packet.  Lane pairs of samples are
 * stored as dwords: coalesced 6,480-byte rows per packet. */
__global__ __launch_bounds__(256) void k_modulate(ModemState *st, const uint8_t *pkts, int16_t *pcm,
						  int channels, int packets, const uint8_t *active)
{
	long w = blockIdx.x * 4L + threadIdx.x / WAVE;
	int lane = threadIdx.x % WAVE;
	if (w >= (long) channels * packets)
		return;
	int c = (int) (w / packets), k = (int) (w - (long) c * packets);
	if (active && !active[c])
		return;
	const uint8_t *d = pkts + w * 11;
	int prev0 = k ? modem_tx_bit(d - 11, MODEM_BITS - 1) : st[c].lastb;
	int vad = st[c].vadtr ^ (k & 1);
	uint32_t *o = (uint32_t *) (pcm + w * MODEM_PKT_SAMPLES);
	for (int q = lane; q < MODEM_PKT_SAMPLES / 2; q += WAVE) {
		int s0 = 2 * q, t = s0 / 36, ii = s0 - 36 * t;
		int b = modem_tx_bit(d, t);
		int prev = t ? modem_tx_bit(d, t - 1) : prev0;
		uint32_t lo = (uint16_t) modem_sample(b, prev, vad, ii);
		uint32_t hi = (uint16_t) modem_sample(b, prev, vad, ii + 1);
		o[q] = lo | (hi << 16);
	}
}

/* the state update of a whole modulate launch, after k_modulate has read it */
__global__ __launch_bounds__(WAVE) void k_modulate_state(ModemState *st, const uint8_t *pkts,
							 int channels, int packets, const uint8_t *active)
{
	int c = blockIdx.x * WAVE + threadIdx.x;
	if (c >= channels || (active && !active[c]))
		return;
	st[c].lastb = modem_tx_bit(pkts + ((long) c * packets + packets - 1) * 11, MODEM_BITS - 1);
	st[c].vadtr ^= packets & 1;
}

/* Demodulate (modem.h, modem/modem.c:186): one lane per channel, `calls`
 * successive calls as rx.c:294-297 makes them (pos advances by the return
 * value, data persists); a call that would read past the channel's stride
 * returns -1 and stops the channel.
 *
 * Each lane reads its own row, so a direct read of the stream is a 2-byte
 * load whose 64 lanes touch 64 different rows -- ~1,900 of them per call.
 * Instead the samples of up to DEMOD_CALLS calls are staged once into the
 * lane's private segment with 16-byte loads, and the calls read them from
 * there, where the hardware interleaves the 64 lanes' copies per dword: the
 * same-index reads of a wave are one contiguous 256-byte access. */
#define DEMOD_CALLS 15	/* calls per staged window (one packet time) */
#define DEMOD_ADV_MAX (MODEM_BLOCK_SAMPLES + 8)	/* a call's largest return (q <= 8) */
#define DEMOD_WIN (((DEMOD_CALLS - 1) * DEMOD_ADV_MAX + MODEM_LOOKAHEAD + 8 + 7) & ~7)

struct DemodLane {
	uint8_t guard[FLAT_GUARD_BYTES];
	ModemState S;
	alignas(16) int16_t w[DEMOD_WIN];
};

/* w[sh + i] = src[i], i < n, where sh = the samples before src in its
 * 16-byte line: whole lines by dwordx4 (each starts at or after the line
 * that holds src[0], and ends at or before src[n]), the last partial line
 * sample by sample, so nothing past src[n - 1] is read */
__device__ __forceinline__ int demod_stage(int16_t *w, const int16_t *src, int n)
{
	const int sh = (int) (((uintptr_t) src & 15) >> 1);
	/* pointer arithmetic on src (not an integer cast) keeps the global
	 * address space, so these are global_ loads, not FLAT */
	const v4u32 *g = (const v4u32 *) (src - sh);
	v4u32 *d = (v4u32 *) w;
	const int full = (sh + n) >> 3;
	int k = 0;
	for (; k + 8 <= full; k += 8) {	/* eight loads in flight, then the stores */
		v4u32 t[8];
#pragma unroll
		for (int j = 0; j < 8; j++)
			t[j] = g[k + j];
#pragma unroll
		for (int j = 0; j < 8; j++)
			d[k + j] = t[j];
	}
	for (; k < full; k++)
		d[k] = g[k];
	for (int i = full * 8 - sh; i < n; i++)
		w[sh + i] = src[i];
	return sh;
}

/* `calls` successive calls of one lane on its staged window, from sample
 * offset p of its row x; after(k, r) runs after call k with its return value
 * (-1: the call would have read past the row, and the lane stops).  Returns
 * the offset after the last call. */
template <class F>
__device__ __forceinline__ int32_t demod_calls(DemodLane &L, const int16_t *x, long stride, int32_t p,
						uint8_t *d, int calls, F &&after)
{
	int32_t r = 0;
	for (int k0 = 0; k0 < calls && r >= 0; k0 += DEMOD_CALLS) {
		const int nk = calls - k0 < DEMOD_CALLS ? calls - k0 : DEMOD_CALLS;
		/* the window: from p, the lookahead of the chunk's last call at
		 * the largest advance per call, never past the row */
		long base = 0;
		if (p >= 0 && p + MODEM_LOOKAHEAD <= stride) {
			long end = (long) p + (long) (nk - 1) * DEMOD_ADV_MAX + MODEM_LOOKAHEAD;
			if (end > stride)
				end = stride;
			base = p - demod_stage(L.w, x + p, (int) (end - p));
		}
		for (int k = k0; k < k0 + nk; k++) {
			r = -1;
			if (p >= 0 && p + MODEM_LOOKAHEAD <= stride) {
				r = modem_demod(&L.S, L.w + (p - base), d);
				p += r;
			}
			after(k, r);
			if (r < 0)
				break;
		}
	}
	return p;
}

__global__ __launch_bounds__(WAVE) void k_demodulate(ModemState *st, const int16_t *pcm, long stride,
						     int32_t *pos, uint8_t *data, uint8_t *out,
						     int32_t *ret, int channels, int calls,
						     const uint8_t *active)
{
	int c = blockIdx.x * WAVE + threadIdx.x;
	if (c >= channels || (active && !active[c]))
		return;
	DemodLane L;
	PIN_FRAME(L);
	L.S = st[c];
	uint8_t d[12];
	for (int i = 0; i < 12; i++)
		d[i] = data[12L * c + i];
	const int32_t p = demod_calls(L, pcm + (long) c * stride, stride, pos[c], d, calls, [&](int k, int32_t r) {
		if (out)
			for (int i = 0; i < 12; i++)
				out[((long) c * calls + k) * 12 + i] = d[i];
		if (ret)
			ret[(long) c * calls + k] = r;
	});
	st[c] = L.S;
	pos[c] = p;
	for (int i = 0; i < 12; i++)
		data[12L * c + i] = d[i];
}

/*
 * The receive loop (rx.c:294-361, rxline.h): k_demodulate's lane and window,
 * with the ready-block step run inside the call loop on the lane's buf --
 * the fber update, ProcessCtr on the channel's link record (loaded at the
 * event and stored after it: its 32 soft bits would otherwise sit in the
 * lane's registers through every Demodulate call), the fau update -- and the
 * block handed out into the channel's next slot.  Lanes of a wave reach their
 * events at different calls, so the wave may run the branch in every
 * iteration; no lane waits on another, and every loop is bounded by `calls`
 * or a constant.
 *
 * Outputs are slot-major (slot j = rows j * channels ...).  A lane writes the
 * bytes of its own rows only: an 11-byte bits row as the bytes up to its
 * first dword boundary, whole dwords, and the bytes after the last; the
 * 8-byte info row as two dwords; nothing at or past `slots`.
 */
typedef uint32_t rxl_u32a __attribute__((__may_alias__));

__device__ __forceinline__ void rxl_store_bits(uint8_t *row, const uint8_t *d)
{
	const int head = (int) ((4 - ((uintptr_t) row & 3)) & 3);
	int i = 0;
	for (; i < head; i++)
		row[i] = d[i];
	for (; i + 4 <= VC_PKT_BYTES; i += 4)
		*(rxl_u32a *) (row + i) = (uint32_t) d[i] | ((uint32_t) d[i + 1] << 8) |
					  ((uint32_t) d[i + 2] << 16) | ((uint32_t) d[i + 3] << 24);
	for (; i < VC_PKT_BYTES; i++)
		row[i] = d[i];
}

__global__ __launch_bounds__(WAVE) void k_rx_line(ModemState *st, LinkState *lk, RxLineState *rx,
						  const int16_t *pcm, long stride, int32_t *pos, uint8_t *data,
						  uint8_t *bits, uint8_t *voice, uint32_t *info, uint8_t *count,
						  int channels, int calls, int slots, const uint8_t *active)
{
	int c = blockIdx.x * WAVE + threadIdx.x;
	if (c >= channels || (active && !active[c]))
		return;
	DemodLane L;
	PIN_FRAME(L);
	L.S = st[c];
	uint8_t d[12];
	for (int i = 0; i < 12; i++)
		d[i] = data[12L * c + i];
	float fber = rx[c].fber, fau = rx[c].fau;
	uint32_t blocks = rx[c].blocks;
	int n = 0;	/* blocks handed out by this launch */
	const int32_t p = demod_calls(L, pcm + (long) c * stride, stride, pos[c], d, calls, [&](int k, int32_t r) {
		if (r < 0 || !(d[11] & 0x80))
			return;
		const RxLineEvent ev = rxline_block(d, &lk[c], &fber, &fau);
		blocks++;
		if (n < slots) {
			const long row = (long) n * channels + c;
			rxl_store_bits(bits + row * VC_PKT_BYTES, d);
			voice[row] = ev.kind == RXL_KIND_VOICE;
			uint32_t w0, w1;
			rxline_info(&ev, k, &w0, &w1);
			info[2 * row] = w0;
			info[2 * row + 1] = w1;
			n++;
		}
		d[11] = 0;	/* rx.c:361: the block is taken, the output slot being free */
	});
	st[c] = L.S;
	pos[c] = p;
	for (int i = 0; i < 12; i++)
		data[12L * c + i] = d[i];
	rx[c].fber = fber;
	rx[c].fau = fau;
	rx[c].blocks = blocks;
	count[c] = (uint8_t) n;
}

/* after k_rx_line: 540 zero samples for every slot that holds a block which
 * is not voice (rx.c:360), one wave per (slot, channel) */
__global__ __launch_bounds__(STREAM_BLOCK) void k_rx_line_zero(uint2 *sp, const uint8_t *voice,
								 const uint8_t *count, const uint8_t *active,
								 int channels, int slots)
{
	const int words = (int) (MELPE_SF_SAMPLES * sizeof(int16_t) / sizeof(uint2));
	const long w = blockIdx.x * (long) (STREAM_BLOCK / WAVE) + threadIdx.x / WAVE;
	if (w >= (long) slots * channels)
		return;
	const int j = (int) (w / channels), c = (int) (w - (long) j * channels);
	if ((active && !active[c]) || j >= count[c] || voice[w])
		return;
	uint2 *row = sp + w * words;
	for (int i = threadIdx.x & (WAVE - 1); i < words; i += WAVE)
		row[i] = make_uint2(0u, 0u);
}

/* the decoder's mask of slot j: the channels whose block j is voice */
__global__ __launch_bounds__(STREAM_BLOCK) void k_rx_line_mask(uint8_t *mask, const uint8_t *voice,
								 const uint8_t *count, const uint8_t *active,
								 int channels, int j)
{
	const long c = blockIdx.x * (long) STREAM_BLOCK + threadIdx.x;
	if (c >= channels)
		return;
	mask[c] = (!active || active[c]) && j < count[c] && voice[(long) j * channels + c];
}

__global__ __launch_bounds__(WAVE) void k_modem_reset(ModemState *st, const uint8_t *mask, int channels)
{
	int c = blockIdx.x * WAVE + threadIdx.x;
	if (c >= channels || (mask && !mask[c]))
		return;
	ModemState z;
	modem_reset(&z);
	st[c] = z;
}

/* ------------------------------------------------------------------ */
/* launchers (launch.h)                                                */
/* ------------------------------------------------------------------ */

/* blocks of STREAM_BLOCK lanes (or, with per = STREAM_BLOCK / WAVE, of that
 * many waves) that cover n */
static inline unsigned stream_blocks(long n, long per = STREAM_BLOCK)
{
	return (unsigned) ((n + per - 1) / per);
}

extern "C" int kl_voice_crypt(unsigned char *pkts, const uint32_t *counters, const uint4 *keys,
			      const uint8_t *invert, int channels, int packets, int dir, hipStream_t s)
{
	const long n = (long) channels * packets;
	k_voice_crypt<<<(unsigned) ((n + 255) / 256), 256, 0, s>>>(pkts, counters, keys, invert, channels, packets, dir);
	return (int) hipGetLastError();
}

extern "C" int kl_vad(VadState *st, const int16_t *sp, uint8_t *votes, uint8_t *gate, const uint8_t *active,
		      int channels, hipStream_t s)
{
	k_vad<<<grid_for(channels), WAVE, 0, s>>>(st, sp, votes, gate, active, channels);
	return (int) hipGetLastError();
}

extern "C" int kl_vad_reset(VadState *st, const uint8_t *mask, int channels, hipStream_t s)
{
	k_vad_reset<<<grid_for(channels), WAVE, 0, s>>>(st, mask, channels);
	return (int) hipGetLastError();
}

extern "C" size_t kl_stream_pack_work_words(int channels)
{
	return stream_blocks(channels);
}

extern "C" int kl_stream_pack(const unsigned char *bits, const uint8_t *votes, uint8_t *last, unsigned char *out,
			      uint32_t *offs, uint32_t *work, int channels, const uint8_t *active, hipStream_t s)
{
	const unsigned nb = stream_blocks(channels);
	k_stream_len<<<nb, STREAM_BLOCK, 0, s>>>(votes, active, work, channels);
	MELPE_CHK(hipGetLastError());
	k_stream_scan<<<1, STREAM_BLOCK, 0, s>>>(work, nb);
	MELPE_CHK(hipGetLastError());
	k_stream_scatter<<<nb, STREAM_BLOCK, 0, s>>>(bits, votes, last, out, offs, work, channels, active);
	return (int) hipGetLastError();
}

extern "C" int kl_stream_parse(const unsigned char *stream, const uint32_t *pos, const uint32_t *end,
			       uint32_t *pos_next, unsigned char *bits, uint8_t *voiced, uint8_t *lens,
			       uint2 *sp, const uint8_t *active, int channels, hipStream_t s)
{
	k_stream_parse<<<stream_blocks(channels), STREAM_BLOCK, 0, s>>>(stream, pos, end, pos_next, bits, voiced, lens,
									active, channels);
	MELPE_CHK(hipGetLastError());
	k_stream_zero<<<stream_blocks(channels, STREAM_BLOCK / WAVE), STREAM_BLOCK, 0, s>>>(sp, lens, channels);
	return (int) hipGetLastError();
}

extern "C" int kl_modem_reset(ModemState *st, const uint8_t *mask, int channels, hipStream_t s)
{
	k_modem_reset<<<grid_for(channels), WAVE, 0, s>>>(st, mask, channels);
	return (int) hipGetLastError();
}

extern "C" int kl_modulate(ModemState *st, const uint8_t *pkts, int16_t *pcm, int channels, int packets,
			   const uint8_t *active, hipStream_t s)
{
	const long waves = (long) channels * packets;
	k_modulate<<<(unsigned) ((waves + 3) / 4), 256, 0, s>>>(st, pkts, pcm, channels, packets, active);
	MELPE_CHK(hipGetLastError());
	k_modulate_state<<<grid_for(channels), WAVE, 0, s>>>(st, pkts, channels, packets, active);
	return (int) hipGetLastError();
}

extern "C" int kl_demodulate(ModemState *st, const int16_t *pcm, long stride, int32_t *pos, uint8_t *data,
			     uint8_t *out, int32_t *ret, int channels, int calls, const uint8_t *active,
			     hipStream_t s)
{
	k_demodulate<<<grid_for(channels), WAVE, 0, s>>>(st, pcm, stride, pos, data, out, ret, channels, calls, active);
	return (int) hipGetLastError();
}

extern "C" int kl_rx_line(ModemState *st, LinkState *lk, RxLineState *rx, const int16_t *pcm, long stride,
			  int32_t *pos, uint8_t *data, uint2 *sp, uint8_t *bits, uint8_t *voice, uint32_t *info,
			  uint8_t *count, int channels, int calls, int slots, const uint8_t *active, hipStream_t s)
{
	k_rx_line<<<grid_for(channels), WAVE, 0, s>>>(st, lk, rx, pcm, stride, pos, data, bits, voice, info, count,
						      channels, calls, slots, active);
	MELPE_CHK(hipGetLastError());
	k_rx_line_zero<<<stream_blocks((long) slots * channels, STREAM_BLOCK / WAVE), STREAM_BLOCK, 0, s>>>(
		sp, voice, count, active, channels, slots);
	return (int) hipGetLastError();
}

extern "C" int kl_rx_line_mask(uint8_t *mask, const uint8_t *voice, const uint8_t *count, const uint8_t *active,
			       int channels, int j, hipStream_t s)
{
	k_rx_line_mask<<<stream_blocks(channels), STREAM_BLOCK, 0, s>>>(mask, voice, count, active, channels, j);
	return (int) hipGetLastError();
}

extern "C" size_t kl_rx_line_private(void)
{
	return private_bytes((const void *) k_rx_line);
}
