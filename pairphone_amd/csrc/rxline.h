/*
 * rxline.h -- the body of PairPhone's receive loop between Demodulate and
 * melpe_s (rx.c:298-361) for one channel, with the playback buffer always
 * empty (l_jit_buf = 0): what happens to the demodulator's persistent
 * 12-byte buf when a call has flagged a block ready (buf[11] & 0x80).
 *
 *   lag_flag = buf[11] & 0x40; if set, fber *= 0.99, fber += buf[11] & 0x0F
 *   buf[11] = 0xFE
 *   if lag_flag: ProcessPkt(buf) in place (link.h link_process_ctr at step
 *     >= 5); a value >= 0 is a control packet (fau *= 0.99, fau += value),
 *     -3 is voice (buf[11] = 0xFF)
 *   the caller hands the block out, then buf[11] = 0 (rx.c:361)
 *
 * buf is the buffer the next Demodulate call receives, so a block the
 * demodulator forced out without rewriting it (modem.h, `data[11] |= 0x8F`)
 * would be processed as the previous ProcessPkt left it, plus the lag bits
 * every call since has added to byte 10.  From a reset ModemState that path
 * is unreachable (a frame's 15 calls visit every bit position once and the
 * lag is fixed within a frame, so `j == lag` always fires and sets blk);
 * keeping the packet in place covers it by construction, no test reaches it.
 *
 * fber and fau round as the reference's floats do: a double multiply rounded
 * to float, then a float add (link.h link_decay).
 *
 * Shared by the receive-loop kernel (k_line.hip k_rx_line) and the
 * host-emulation build.
 */
#ifndef MELPE_RXLINE_H
#define MELPE_RXLINE_H

#include <stdint.h>

#include "link.h"

#define RXL_NOLOCK (-102)	/* MELPE_RX_NOLOCK: the block lag was not locked, ProcessPkt not run */
#define RXL_INFO_BYTES 8

/* a block's kind, byte 2 of its info row */
enum { RXL_KIND_NOLOCK = 0, RXL_KIND_CONTROL = 1, RXL_KIND_VOICE = 2, RXL_KIND_STAGE = 3 };

/* the per-channel record of the loop's own statics (rx.c:150-151); layout:
 * include/melpe_batch.h */
struct RxLineState {
	float fber;		/* averaged symbol errors per block */
	float fau;		/* averaged authentication level */
	uint32_t blocks;	/* ready blocks seen */
	uint32_t rsv;
};
static_assert(sizeof(RxLineState) == 16, "the public record size (melpe_batch.h)");

struct RxLineEvent {
	int32_t ret;	/* ProcessPkt's value, LINK_STAGE, or RXL_NOLOCK */
	uint8_t kind;
	uint8_t status;	/* buf[11] as Demodulate left it */
};

static MELPE_HD inline float rxline_decay(float f)
{
	return (float) ((double) f * 0.99);
}

/* rx.c:298-348 on a ready block; buf[11] is left 0xFE (silence) or 0xFF
 * (voice), for the caller to hand out and clear */
static MELPE_HD inline RxLineEvent rxline_block(uint8_t *buf, LinkState *S, float *fber, float *fau)
{
	RxLineEvent ev;
	ev.status = buf[11];
	ev.kind = RXL_KIND_NOLOCK;
	ev.ret = RXL_NOLOCK;
	const bool lag = (buf[11] & 0x40) != 0;
	if (lag) {
		*fber = rxline_decay(*fber);
		*fber += (float) (buf[11] & 0x0F);
	}
	buf[11] = 0xFE;
	if (!lag)
		return ev;
	if (S->step < 5) {	/* a key-exchange stage: the host's, record and packet untouched */
		ev.kind = RXL_KIND_STAGE;
		ev.ret = LINK_STAGE;
		return ev;
	}
	LinkRx R;
	uint64_t lo, hi;
	bool wr;
	link_rx_load(&R, S);
	link_pkt_load(buf, &lo, &hi);
	ev.ret = link_process_ctr(&R, &lo, &hi, &wr);
	if (wr)
		link_pkt_store(buf, lo, hi);
	link_rx_store(S, &R);
	if (ev.ret >= 0) {
		ev.kind = RXL_KIND_CONTROL;
		*fau = rxline_decay(*fau);
		*fau += (float) ev.ret;
	} else {	/* -3 */
		ev.kind = RXL_KIND_VOICE;
		buf[11] = 0xFF;
	}
	return ev;
}

/* a block's info row (melpe_batch.h) as two little-endian dwords */
static MELPE_HD inline void rxline_info(const RxLineEvent *ev, int call, uint32_t *w0, uint32_t *w1)
{
	*w0 = (uint32_t) (call & 0xff) | ((uint32_t) ev->status << 8) | ((uint32_t) ev->kind << 16);
	*w1 = (uint32_t) ev->ret;
}

#endif
