/*
 * k_link.hip -- the work-stage packet layer on the device (link.h): MakeCtr
 * for C channels x K packets (k_link_tx), ProcessCtr (k_link_rx), and the
 * Golay(24,12) self-test sweep (k_golay_sweep).
 *
 * Packets are 11-byte rows, C x K x 11, so a lane's row is not dword-aligned.
 * Both kernels move them between HBM and LDS as dwords (the tensor is 4-byte
 * aligned) and let the lanes pick their bytes out of LDS.  Only bytes of
 * packets a lane rewrote are stored: a dword that lies wholly in rewritten
 * packets goes out as a dword, one that straddles a packet that was not
 * rewritten (an inactive channel's, a refused one's, a control packet on RX)
 * goes out as the rewritten bytes alone.
 */
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "link.h"
#include "launch.h"

typedef uint32_t u32_may_alias __attribute__((__may_alias__));

/* dword j of the packet tensor, whose last dword may be cut short by the
 * tensor's end (`total` bytes) */
__device__ __forceinline__ uint32_t pk_load(const uint8_t *base, size_t off, size_t total)
{
	if (off + 4 <= total)
		return *(const u32_may_alias *) (base + off);
	uint32_t v = 0;
	for (int b = 0; b < 4; b++)
		if (off + b < total)
			v |= (uint32_t) base[off + b] << (8 * b);
	return v;
}

/*
 * TX: one lane per (channel, packet).  Packet k of a channel carries counter
 * cnt_out + 1 + k, so the packets of a call are independent; every lane
 * reads its channel's record and none writes it (k_link_tx_state does, after
 * this kernel).  A block owns TXB consecutive packets = TXB * 11 contiguous
 * bytes, a whole number of dwords.
 */
#define TXB 256
#define TX_DW (TXB * VC_PKT_BYTES / 4)
static_assert(TXB * VC_PKT_BYTES % 4 == 0, "a block's packets are whole dwords");

__global__ __launch_bounds__(TXB) void k_link_tx(const LinkState *st, uint8_t *pkts, const uint8_t *voiced,
						 int32_t *ret, const uint8_t *active, int channels, int packets)
{
	__shared__ uint32_t sh[TX_DW];
	__shared__ uint8_t mod[TXB];
	const int t = threadIdx.x;
	const size_t n = (size_t) channels * packets;
	const size_t first = (size_t) blockIdx.x * TXB;
	const size_t total = n * VC_PKT_BYTES, base = first * VC_PKT_BYTES;
	const int here = (int) (n - first < TXB ? n - first : TXB);	/* packets of this block */

	for (int j = t; j < TX_DW; j += TXB)
		if (base + 4 * (size_t) j < total)
			sh[j] = pk_load(pkts, base + 4 * (size_t) j, total);
	mod[t] = 0;
	__syncthreads();

	if (t < here) {
		const size_t i = first + t;
		const int c = (int) (i / packets), k = (int) (i - (size_t) c * packets);
		if (!active || active[c]) {
			const LinkState *S = &st[c];
			const int step = S->step;
			const uint64_t cnt = (uint64_t) S->cnt_out + 1u + (uint64_t) k;
			int r;
			if (step < 6) {
				r = LINK_STAGE;
			} else if (cnt > LINK_CNT_MAX) {
				r = LINK_REKEY;
			} else {
				uint64_t a0, a1, s0, s1, lo, hi;
				link_key_lanes(S->akey, &a0, &a1);
				link_key_lanes(S->skey, &s0, &s1);
				uint8_t *p = (uint8_t *) sh + t * VC_PKT_BYTES;
				link_pkt_load(p, &lo, &hi);
				r = link_tx_packet((uint32_t) cnt, step, voiced && (voiced[i] & 1), a0, a1, s0, s1,
						   &lo, &hi);
				link_pkt_store(p, lo, hi);
				mod[t] = 1;
			}
			ret[i] = r;
		}
	}
	__syncthreads();

	for (int j = t; j < TX_DW; j += TXB) {
		const size_t off = base + 4 * (size_t) j;
		if (off >= total)
			break;
		const int p0 = 4 * j / VC_PKT_BYTES, p1 = (4 * j + 3) / VC_PKT_BYTES;
		if (off + 4 <= total && mod[p0] && mod[p1]) {
			*(u32_may_alias *) (pkts + off) = sh[j];
		} else {
			for (int b = 0; b < 4; b++) {
				const int p = (4 * j + b) / VC_PKT_BYTES;
				if (p < here && mod[p])
					pkts[off + b] = (uint8_t) (sh[j] >> (8 * b));
			}
		}
	}
}

/* the single writer of the records after k_link_tx: cnt_out advances by the
 * packets that were built (those up to the call-time limit) */
__global__ __launch_bounds__(64) void k_link_tx_state(LinkState *st, const uint8_t *active, int channels,
						      int packets)
{
	const int c = blockIdx.x * 64 + threadIdx.x;
	if (c >= channels || (active && !active[c]))
		return;
	const uint32_t cnt = st[c].cnt_out;
	if (st[c].step < 6 || cnt >= LINK_CNT_MAX)
		return;
	const uint32_t room = LINK_CNT_MAX - cnt;
	st[c].cnt_out = cnt + (room < (uint32_t) packets ? room : (uint32_t) packets);
}

/*
 * RX: one lane per channel, its K packets in order: the counter, fcrc and the
 * soft bits carry from packet to packet, so the record stays in registers for
 * the whole loop.  A block is one wave.  The wave's packets go through LDS in
 * tiles of up to RX_TILE packets per channel: channel l's tile is RX_TILE * 11
 * bytes of its row, fetched as the dwords that cover it into RX_STRIDE dwords
 * of LDS (odd, so the lanes' byte reads spread over the banks), consecutive
 * threads on consecutive dwords.
 */
#define RX_TILE 8
#define RX_COVER ((RX_TILE * VC_PKT_BYTES + 3 + 3) / 4)	/* dwords covering a tile at any alignment */
#define RX_STRIDE (RX_COVER | 1)

__global__ __launch_bounds__(64) void k_link_rx(LinkState *st, uint8_t *pkts, int32_t *ret, uint8_t *voice,
						const uint8_t *active, int channels, int packets)
{
	__shared__ uint32_t sh[64 * RX_STRIDE];
	__shared__ uint8_t mod[64 * RX_TILE];
	const int t = threadIdx.x;
	const int c0 = blockIdx.x * 64;
	const int c = c0 + t;
	const int nch = channels - c0 < 64 ? channels - c0 : 64;	/* channels of this wave */
	const size_t total = (size_t) channels * packets * VC_PKT_BYTES;
	bool live = c < channels && (!active || active[c]);
	LinkRx R;
	if (live) {
		link_rx_load(&R, &st[c]);
		live = R.step >= 5;
		if (!live)
			for (int k = 0; k < packets; k++) {
				ret[(size_t) c * packets + k] = LINK_STAGE;
				if (voice)
					voice[(size_t) c * packets + k] = 0;
			}
	}
	const unsigned long long livemask = __ballot(live);

	for (int k0 = 0; k0 < packets; k0 += RX_TILE) {
		const int kn = packets - k0 < RX_TILE ? packets - k0 : RX_TILE;
		const int seg = kn * VC_PKT_BYTES;	/* bytes of a channel's tile */
		/* fetch: dword w of channel ch's cover */
		for (int e = t; e < nch * RX_COVER; e += 64) {
			const int ch = e / RX_COVER, w = e - ch * RX_COVER;
			const size_t g0 = ((size_t) (c0 + ch) * packets + k0) * VC_PKT_BYTES;
			const size_t off = (g0 & ~(size_t) 3) + 4 * (size_t) w;
			if (((livemask >> ch) & 1) && off < g0 + seg && off < total)
				sh[ch * RX_STRIDE + w] = pk_load(pkts, off, total);
		}
		for (int e = t; e < 64 * RX_TILE; e += 64)
			mod[e] = 0;
		__syncthreads();

		if (live) {
			const size_t g0 = ((size_t) c * packets + k0) * VC_PKT_BYTES;
			uint8_t *row = (uint8_t *) (sh + t * RX_STRIDE) + (g0 & 3);
			for (int k = 0; k < kn; k++) {
				uint64_t lo, hi;
				bool wr;
				link_pkt_load(row + k * VC_PKT_BYTES, &lo, &hi);
				const int r = link_process_ctr(&R, &lo, &hi, &wr);
				if (wr) {
					link_pkt_store(row + k * VC_PKT_BYTES, lo, hi);
					mod[t * RX_TILE + k] = 1;
				}
				ret[(size_t) c * packets + k0 + k] = r;
				if (voice)
					voice[(size_t) c * packets + k0 + k] = r == -3;
			}
		}
		__syncthreads();

		/* store the bytes of rewritten packets */
		for (int e = t; e < nch * RX_COVER; e += 64) {
			const int ch = e / RX_COVER, w = e - ch * RX_COVER;
			if (!((livemask >> ch) & 1))
				continue;
			const size_t g0 = ((size_t) (c0 + ch) * packets + k0) * VC_PKT_BYTES;
			const size_t off = (g0 & ~(size_t) 3) + 4 * (size_t) w;
			if (off >= g0 + seg)
				continue;
			const int rel = (int) (off - g0);	/* -3 .. seg - 1: the dword's first byte in the tile */
			const uint32_t v = sh[ch * RX_STRIDE + w];
			const bool whole = rel >= 0 && rel + 4 <= seg;
			if (whole && mod[ch * RX_TILE + rel / VC_PKT_BYTES] &&
			    mod[ch * RX_TILE + (rel + 3) / VC_PKT_BYTES]) {
				*(u32_may_alias *) (pkts + off) = v;
			} else {
				for (int b = 0; b < 4; b++) {
					const int rb = rel + b;
					if (rb >= 0 && rb < seg && mod[ch * RX_TILE + rb / VC_PKT_BYTES])
						pkts[off + b] = (uint8_t) (v >> (8 * b));
				}
			}
		}
		__syncthreads();
	}
	if (live)
		link_rx_store(&st[c], &R);
}

/*
 * The Golay code over its whole domain: thread v < 4,096 also writes the
 * codeword of v; thread i sums decode(v) * (v * 0x9E3779B97F4A7C15 + 1) over
 * 256 received words v of bucket b = v >> 16 and the block adds the partial
 * sums into digest[b] (256 blocks of 256 threads, one bucket each).  Sums
 * are mod 2^64, so their order does not matter.
 */
__global__ __launch_bounds__(256) void k_golay_sweep(uint32_t *enc, uint64_t *digest)
{
	__shared__ uint64_t part[256];
	const int t = threadIdx.x;
	const uint32_t b = blockIdx.x;
	if (b < 16)
		enc[b * 256 + t] = fec_golay2412_encode_symbol(b * 256 + t);
	uint64_t h = 0;
	for (int j = 0; j < 256; j++) {
		const uint32_t v = (b << 16) | ((uint32_t) j << 8) | (uint32_t) t;
		h += (uint64_t) fec_golay2412_decode_symbol(v) * ((uint64_t) v * 0x9E3779B97F4A7C15ull + 1u);
	}
	part[t] = h;
	__syncthreads();
	for (int s = 128; s > 0; s >>= 1) {
		if (t < s)
			part[t] += part[t + s];
		__syncthreads();
	}
	if (t == 0)
		digest[b] = part[0];
}

extern "C" int kl_link_tx(LinkState *st, uint8_t *pkts, const uint8_t *voiced, int32_t *ret,
			  const uint8_t *active, int channels, int packets, hipStream_t s)
{
	const size_t n = (size_t) channels * packets;
	k_link_tx<<<(unsigned) ((n + TXB - 1) / TXB), TXB, 0, s>>>(st, pkts, voiced, ret, active, channels, packets);
	k_link_tx_state<<<(unsigned) ((channels + 63) / 64), 64, 0, s>>>(st, active, channels, packets);
	return (int) hipGetLastError();
}

extern "C" int kl_link_rx(LinkState *st, uint8_t *pkts, int32_t *ret, uint8_t *voice, const uint8_t *active,
			  int channels, int packets, hipStream_t s)
{
	k_link_rx<<<(unsigned) ((channels + 63) / 64), 64, 0, s>>>(st, pkts, ret, voice, active, channels, packets);
	return (int) hipGetLastError();
}

extern "C" int kl_golay_sweep(uint32_t *enc, uint64_t *digest, hipStream_t s)
{
	k_golay_sweep<<<256, 256, 0, s>>>(enc, digest);
	return (int) hipGetLastError();
}
