/*
 * link.h -- PairPhone's work-stage packet layer: MakeCtr (crp.c:789-838, what
 * MakePkt is at step 6 and above, tx.c:269) and ProcessCtr (crp.c:842-982,
 * what ProcessPkt is at step 5 and above, rx.c:340), with EncodeBlock /
 * DecodeBlock (crp.c:331-426), UpdateSoftBits / AssembleSoftBits
 * (crp.c:430-455) and VoiceEnc / VoiceDec (voice_crypt.h).
 *
 * One LinkState per channel holds the file statics of crp.c:73-88 these
 * functions read or write (layout: include/melpe_batch.h).  A packet is held
 * as two integers, lo = bytes 0..7 and hi = bytes 8..10 (little-endian), so
 * the header is lo & 0xff, the three Golay words are 24-bit fields and the
 * polarity bit is bit 16 of hi.
 *
 * The reference's scratch array udata reaches the state in one place: a
 * block with an uncorrectable Golay word leaves DecodeBlock early, and the
 * crc8 that drives fcrc (crp.c:873-875) is then taken over the bytes decoded
 * so far plus whatever the previous call left in udata[0..5] -- a decoded
 * control block or, after voice, the first bytes of the gamma.  Those stale
 * bytes are pseudo-random, which is what keeps fcrc averaging 0 on voice (a
 * zeroed scratch would make every such packet count +4, as a key-exchange
 * packet does, and force a reset within a few hundred voice packets).  So
 * udata[0..5] as the channel's previous ProcessCtr left them are part of the
 * record (`scratch`).  A reference process shares udata between its TX and RX
 * calls; here each direction has its own context, and MakeCtr, which writes
 * udata before it reads it, needs none.  tests/golden/ref_link.c saves and
 * restores the same six bytes around each ProcessPkt.
 *
 * The key-exchange stages are not here.  Where the reference would enter them
 * the calls return a status it never returns: LINK_REKEY instead of ResetCT
 * at the call-time limit (crp.c:808-816), LINK_STAGE at a step the work-stage
 * functions are not called at.
 *
 * Float state rounds as the reference's does: `f *= 0.95` is a double
 * multiply rounded to float, `f += weight` a float add (no contraction: the
 * conversion sits between them).
 *
 * Shared by the GPU kernels (k_link.hip) and the host-emulation build.
 */
#ifndef MELPE_LINK_H
#define MELPE_LINK_H

#include <stdint.h>

#include "voice_crypt.h"
#include "golay.h"

#define LINK_REKEY (-100)
#define LINK_STAGE (-101)
#define LINK_CNT_MAX 65534u	/* crp.c:808, :864 */

struct LinkState {
	uint32_t cnt_out;	/* counter of outgoing packets */
	uint32_t cnt_in;	/* synchronised counter of incoming packets */
	float finv;		/* soft flag of channel inversion (< 0: inverted) */
	float fcrc;		/* soft level of the DH-sequence detector */
	int32_t step;		/* stage of the connection (5..8 here) */
	uint8_t scratch[6];	/* udata[0..5] as the last ProcessCtr left them */
	uint8_t rsv0[6];
	uint8_t skey[32];	/* [0..15] encrypts, [16..31] decrypts */
	uint8_t akey[32];	/* [0..15] our authenticator key, [16..31] theirs */
	float fdata[32];	/* soft bits of the counter delta */
	uint32_t rsv1[8];
};
static_assert(sizeof(LinkState) == 256, "the public record size (melpe_batch.h)");

/* crc8 of crp.c:204-248 (polynomial 0x25, MSB first) over the 4 bytes of v,
 * lowest byte first */
static MELPE_HD inline uint32_t link_crc8_4(uint32_t v)
{
	uint32_t crc = 0;
#pragma unroll
	for (int b = 0; b < 4; b++) {
		crc ^= (v >> (8 * b)) & 0xffu;
#pragma unroll
		for (int i = 0; i < 8; i++)
			crc = ((crc << 1) ^ ((crc & 0x80u) ? 0x25u : 0u)) & 0xffu;
	}
	return crc;
}

/* crc32(0, &g, 1) of crp.c:252-308: the greying mask of tag g */
static MELPE_HD inline uint32_t link_grey_mask(uint32_t g)
{
	uint32_t crc = 0xffffffffu ^ (g & 0xffu);
#pragma unroll
	for (int i = 0; i < 8; i++)
		crc = (crc >> 1) ^ ((crc & 1u) ? 0xedb88320u : 0u);
	return ~crc;
}

/* a 16-byte key as two little-endian lanes */
static MELPE_HD inline void link_key_lanes(const uint8_t *k, uint64_t *a, uint64_t *b)
{
	uint64_t x = 0, y = 0;
#pragma unroll
	for (int i = 0; i < 8; i++) {
		x |= (uint64_t) k[i] << (8 * i);
		y |= (uint64_t) k[8 + i] << (8 * i);
	}
	*a = x;
	*b = y;
}

/*
 * The one sponge call of a packet.  Both uses absorb less than one 72-byte
 * block, so each is one Keccak-f on a padded block (voice_crypt.h):
 *   authenticator (auth != 0): akey16 | skey16 | cnt (2 bytes), pad 0x01 at
 *     byte 34; the tag is the first byte squeezed (crp.c:829-833, :904-908);
 *   gamma: cnt (4 bytes) | skey16, pad 0x01 at byte 20 (crp.c:992-998).
 * The input lanes are selected, the permutation runs once.
 */
static MELPE_HD inline void link_sponge(bool auth, uint32_t cnt, uint64_t a0, uint64_t a1, uint64_t s0,
					uint64_t s1, uint64_t *lo, uint64_t *hi)
{
	uint64_t A[25];
#pragma unroll
	for (int i = 0; i < 25; i++)
		A[i] = 0;
	A[0] = auth ? a0 : ((uint64_t) cnt | (s0 << 32));
	A[1] = auth ? a1 : ((s0 >> 32) | (s1 << 32));
	A[2] = auth ? s0 : ((s1 >> 32) | ((uint64_t) 0x01 << 32));
	A[3] = auth ? s1 : 0;
	A[4] = auth ? ((uint64_t) (cnt & 0xffffu) | ((uint64_t) 0x01 << 16)) : 0;
	A[8] = (uint64_t) 0x80 << 56;
	vc_keccak_f(A);
	*lo = A[0];
	*hi = A[1];
}

/* EncodeBlock (crp.c:331-375) of a control packet: counter sent twice, tag =
 * its 4 LSB, header = authenticator */
static MELPE_HD inline void link_encode_block(uint32_t payload, uint32_t tag, uint32_t header, uint64_t *lo,
					      uint64_t *hi)
{
	tag &= 0xfu;
	if (tag & 1u)
		tag ^= 0xeu;
	payload ^= link_grey_mask(tag);
	const uint32_t w1 = fec_golay2412_encode_symbol(payload & 0xfffu);
	const uint32_t w2 = fec_golay2412_encode_symbol((payload >> 12) & 0xfffu);
	const uint32_t w3 = fec_golay2412_encode_symbol((payload >> 24) | (tag << 8));
	*lo = (uint64_t) (header & 0xffu) | ((uint64_t) w1 << 8) | ((uint64_t) w2 << 32) | ((uint64_t) w3 << 56);
	*hi = (uint64_t) (w3 >> 8);	/* bytes 8, 9; byte 10 = 0 */
}

/* DecodeBlock (crp.c:380-426) into udata[0..3] (*payload), [4] (*tag) and [5]
 * (*header), which come in as the previous call left them: a block that
 * fails at word n returns 0 with only the bytes of the words before n
 * written, still greyed, and the rest stale.  Returns whether the block
 * decoded. */
static MELPE_HD inline bool link_decode_block(uint64_t lo, uint64_t hi, uint32_t *payload, uint32_t *tag,
					      uint32_t *header)
{
	if (hi & 0x10000u) {	/* polarity bit: invert the 80 bits */
		lo = ~lo;
		hi ^= 0xffffu;
	}
	const uint32_t d1 = fec_golay2412_decode_symbol((uint32_t) (lo >> 8) & 0xffffffu);
	const uint32_t d2 = fec_golay2412_decode_symbol((uint32_t) (lo >> 32) & 0xffffffu);
	const uint32_t d3 = fec_golay2412_decode_symbol((uint32_t) (lo >> 56) | ((uint32_t) (hi & 0xffffu) << 8));
	const bool ok1 = !(d1 & GOLAY_FAIL), ok2 = ok1 && !(d2 & GOLAY_FAIL), ok3 = ok2 && !(d3 & GOLAY_FAIL);
	uint32_t p = *payload, t = *tag;
	p = ok1 ? (p & 0xffff0000u) | d1 : p;			/* data[0], data[1] */
	p = ok2 ? (p & 0xff000fffu) | (d2 << 12) : p;		/* data[1] |=, data[2] */
	p = ok3 ? (p & 0x00ffffffu) | ((d3 & 0xffu) << 24) : p;	/* data[3] */
	t = ok3 ? (d3 >> 8) & 0xfu : t;
	if (ok3) {
		p ^= link_grey_mask(t);
		if (t & 1u)
			t ^= 0xeu;
	}
	*payload = p;
	*tag = t;
	*header = ok3 ? (uint32_t) lo & 0xffu : *header;
	return ok3;
}

/* what VoiceDec leaves in udata[0..5]: the gamma's first bytes (crp.c:1021) */
static MELPE_HD inline void link_scratch_gamma(uint64_t glo, uint32_t *u03, uint32_t *u4, uint32_t *u5)
{
	*u03 = (uint32_t) glo;
	*u4 = (uint32_t) (glo >> 32) & 0xffu;
	*u5 = (uint32_t) (glo >> 40) & 0xffu;
}

/* VoiceEnc / VoiceDec's XOR: gamma bytes 0..10 with gamma[10] &= 1; the
 * decrypt side first inverts the 81 bits when finv < 0 (crp.c:1010-1014) */
static MELPE_HD inline void link_apply_gamma(uint64_t *lo, uint64_t *hi, uint64_t glo, uint64_t ghi, bool invert)
{
	ghi &= 0x1ffffu;
	if (invert) {
		glo = ~glo;
		ghi ^= 0x1ffffu;
	}
	*lo ^= glo;
	*hi ^= ghi;
}

/* packet bytes <-> (lo, hi); the store keeps nothing: hi carries byte 10 whole */
static MELPE_HD inline void link_pkt_load(const uint8_t *p, uint64_t *lo, uint64_t *hi)
{
	uint64_t a = 0, b = 0;
#pragma unroll
	for (int i = 0; i < 8; i++)
		a |= (uint64_t) p[i] << (8 * i);
#pragma unroll
	for (int i = 0; i < 3; i++)
		b |= (uint64_t) p[8 + i] << (8 * i);
	*lo = a;
	*hi = b;
}

static MELPE_HD inline void link_pkt_store(uint8_t *p, uint64_t lo, uint64_t hi)
{
#pragma unroll
	for (int i = 0; i < 8; i++)
		p[i] = (uint8_t) (lo >> (8 * i));
#pragma unroll
	for (int i = 0; i < 3; i++)
		p[8 + i] = (uint8_t) (hi >> (8 * i));
}

/*
 * The body of MakeCtr for the packet that carries counter `cnt` (the
 * already incremented cnt_out, <= LINK_CNT_MAX) at stage `step` (>= 6); a0,
 * a1 = akey[0..15], s0, s1 = skey[0..15].  Returns MakeCtr's value.
 */
static MELPE_HD inline int link_tx_packet(uint32_t cnt, int step, bool voiced, uint64_t a0, uint64_t a1,
					  uint64_t s0, uint64_t s1, uint64_t *lo, uint64_t *hi)
{
	const bool voice = voiced && step == 8;
	uint64_t klo, khi;
	link_sponge(!voice, cnt, a0, a1, s0, s1, &klo, &khi);
	if (voice) {
		link_apply_gamma(lo, hi, klo, khi, false);
	} else {
		const uint32_t c16 = cnt & 0xffffu;
		link_encode_block(c16 | (c16 << 16), c16 & 0xfu, (uint32_t) klo & 0xffu, lo, hi);
	}
	return step > 7 ? (int) cnt : -3;
}

/* MakeCtr on a channel's record */
static MELPE_HD inline int link_make_ctr(LinkState *S, uint8_t *pkt, int voiced)
{
	if (S->step < 6)
		return LINK_STAGE;
	if (S->cnt_out >= LINK_CNT_MAX)
		return LINK_REKEY;
	S->cnt_out++;
	uint64_t a0, a1, s0, s1, lo, hi;
	link_key_lanes(S->akey, &a0, &a1);
	link_key_lanes(S->skey, &s0, &s1);
	link_pkt_load(pkt, &lo, &hi);
	const int r = link_tx_packet(S->cnt_out, S->step, (voiced & 1) != 0, a0, a1, s0, s1, &lo, &hi);
	link_pkt_store(pkt, lo, hi);
	return r;
}

/* the part of a record ProcessCtr reads or writes, as values: the RX kernel
 * keeps it in registers over a call's packets (fdata only ever indexed by
 * unrolled constant loops) */
struct LinkRx {
	uint32_t cnt_out, cnt_in;
	float finv, fcrc;
	int32_t step;
	uint32_t u03, u4, u5;		/* udata[0..3], [4], [5] */
	uint64_t a0, a1, s0, s1;	/* akey[16..31], skey[16..31] */
	float fdata[32];
};

static MELPE_HD inline float link_decay(float f)
{
	return (float) ((double) f * 0.95);
}

/* the reset exits of crp.c:856-883 */
static MELPE_HD inline int link_force_reset(LinkRx *R)
{
	R->cnt_out = 65535;
	R->step = 6;
	return 0;
}

/* the sync events' common tail (crp.c:932-944, :962-974) */
static MELPE_HD inline int link_sync(LinkRx *R, int delta)
{
	if (R->step != 8) {	/* initial sync: back and forward */
		if (R->cnt_out < 200)
			R->cnt_out = 201;
		R->step = 8;
	} else if (delta < -1) {
		delta = -1;	/* freeze the counter instead of going back */
	}
	R->cnt_in += (uint32_t) delta;
	R->fcrc = 0;
	return delta;
}

/*
 * ProcessCtr (step >= 5).  *wr is set when the packet was rewritten (voice).
 */
static MELPE_HD inline int link_process_ctr(LinkRx *R, uint64_t *lo, uint64_t *hi, bool *wr)
{
	*wr = false;
	R->cnt_in++;
	if (R->cnt_in == 200 || R->cnt_in > LINK_CNT_MAX)
		return link_force_reset(R);

	bool ctl = link_decode_block(*lo, *hi, &R->u03, &R->u4, &R->u5);
	const uint32_t payload = R->u03, tag = R->u4, header = R->u5;
	const uint32_t c = link_crc8_4(payload);
	R->fcrc = link_decay(R->fcrc);
	R->fcrc += (float) (4 - __builtin_popcount(c ^ header));
	if (R->fcrc > 60.0f)
		return link_force_reset(R);

	const uint32_t u0 = payload & 0xffu, u1 = (payload >> 8) & 0xffu;
	const uint32_t u2 = (payload >> 16) & 0xffu, u3 = payload >> 24;
	/* the tag matches a copy of the counter, and the copies nearly agree */
	if ((u0 & 0xfu) != tag && (u2 & 0xfu) != tag)
		ctl = false;
	if (__builtin_popcount((payload ^ (payload >> 16)) & 0xffffu) > 2)
		ctl = false;
	if (!ctl && R->step != 8)
		return 0;

	const bool inv = R->finv < 0.0f;
	uint64_t klo, khi;
	link_sponge(ctl, R->cnt_in, R->a0, R->a1, R->s0, R->s1, &klo, &khi);
	if (!ctl) {
		link_scratch_gamma(klo, &R->u03, &R->u4, &R->u5);
		link_apply_gamma(lo, hi, klo, khi, inv);
		*wr = true;
		return -3;
	}

	const int au = R->step == 8 ? 8 - __builtin_popcount((header ^ (uint32_t) klo) & 0xffu) : 0;
	/* the far end's counter against ours: forward or back within 32768 */
	int delta = (int) ((u0 | (u1 << 8)) - (R->cnt_in & 0xffffu));
	if (delta > 32767)
		delta -= 65535;
	else if (delta < -32767)
		delta += 65535;
	uint32_t d = (uint32_t) (delta < 0 ? -delta : delta);
	if (delta < 0)
		d += 32768;
	d &= 0xffffu;
	/* UpdateSoftBits(udata + 6, 0, 32, 1): bits 0..15 the delta, bits 16..31
	 * what lies in udata[8..9], our counter (crp.c:903) */
	const uint32_t soft = d | ((R->cnt_in & 0xffffu) << 16);
#pragma unroll
	for (int i = 0; i < 32; i++) {
		R->fdata[i] = link_decay(R->fdata[i]);
		R->fdata[i] += ((soft >> i) & 1u) ? 1.0f : -1.0f;
	}

	/* fast correction: both copies the same and the delta small */
	if (u0 == u2 && u1 == u3 && delta > -255 && delta < 255) {
		if (link_sync(R, delta)) {
#pragma unroll
			for (int i = 0; i < 16; i++)
				R->fdata[i] = 0;
		}
		return au;
	}

	/* slow correction: every bit of the averaged delta is firm */
	const float lim = R->step != 8 ? 10.0f : 17.0f;
	uint32_t avg = 0;
	int firm = 0;
#pragma unroll
	for (int i = 0; i < 16; i++) {
		avg |= R->fdata[i] > 0.0f ? 1u << i : 0u;
		firm += (R->fdata[i] < -lim || R->fdata[i] > lim) ? 1 : 0;
	}
	if (firm == 16) {
		link_sync(R, avg > 32767 ? -(int) (avg & 0x7fffu) : (int) avg);
#pragma unroll
		for (int i = 0; i < 16; i++)
			R->fdata[i] = 0;
	}
	/* a control packet's delta is within two bits of the average; anything
	 * else was voice that happened to look like one */
	if (__builtin_popcount(d ^ avg) < 3 || R->step != 8)
		return au;
	link_sponge(false, R->cnt_in, R->a0, R->a1, R->s0, R->s1, &klo, &khi);
	link_scratch_gamma(klo, &R->u03, &R->u4, &R->u5);
	link_apply_gamma(lo, hi, klo, khi, inv);
	*wr = true;
	return -3;
}

static MELPE_HD inline void link_rx_load(LinkRx *R, const LinkState *S)
{
	R->cnt_out = S->cnt_out;
	R->cnt_in = S->cnt_in;
	R->finv = S->finv;
	R->fcrc = S->fcrc;
	R->step = S->step;
	R->u03 = (uint32_t) S->scratch[0] | ((uint32_t) S->scratch[1] << 8) | ((uint32_t) S->scratch[2] << 16) |
		 ((uint32_t) S->scratch[3] << 24);
	R->u4 = S->scratch[4];
	R->u5 = S->scratch[5];
	link_key_lanes(S->akey + 16, &R->a0, &R->a1);
	link_key_lanes(S->skey + 16, &R->s0, &R->s1);
#pragma unroll
	for (int i = 0; i < 32; i++)
		R->fdata[i] = S->fdata[i];
}

static MELPE_HD inline void link_rx_store(LinkState *S, const LinkRx *R)
{
	S->cnt_out = R->cnt_out;
	S->cnt_in = R->cnt_in;
	S->fcrc = R->fcrc;
	S->step = R->step;
	S->scratch[0] = (uint8_t) R->u03;
	S->scratch[1] = (uint8_t) (R->u03 >> 8);
	S->scratch[2] = (uint8_t) (R->u03 >> 16);
	S->scratch[3] = (uint8_t) (R->u03 >> 24);
	S->scratch[4] = (uint8_t) R->u4;
	S->scratch[5] = (uint8_t) R->u5;
#pragma unroll
	for (int i = 0; i < 32; i++)
		S->fdata[i] = R->fdata[i];
}

#endif
