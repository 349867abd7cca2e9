/*
 * ref_rxline.c -- drives the REFERENCE's receive chain for
 * tests/golden/make_rxline_golden.py (dev container only): Demodulate
 * (modem/modem.c), ProcessPkt (crp.c) and melpe_s (libmelpe_ref.a).  crp.c
 * and modem/modem.c are compiled where they lie, by inclusion, so their file
 * statics are reachable; nothing of them is copied.  make_rxline_golden.py
 * builds this into oracle/_ref/ref_rxline.
 *
 * rx.c itself cannot be compiled here (it pulls in the sound devices and the
 * GSM codec), so main() restates the control flow of its rx() between
 * Demodulate and the resampler, rx.c:294-361, with the playback buffer held
 * empty (l_jit_buf = 0) -- and nothing else of it.
 *
 * One process = one channel: the modem's and the codec's statics are per
 * process.  The link statics are restored from the channel's 256-byte record
 * before each ProcessPkt and saved after it, udata[0..5] under the RX-only
 * rule, exactly as tests/golden/ref_link.c does.
 *
 *   ref_rxline in out
 *     in:  int32 N, L; L x (int32 calls, int32 avail); the link record (256
 *          bytes); the receive-loop record (16 bytes); N int16 samples.
 *          Launch l makes up to `calls` Demodulate calls; a call needs 1,080
 *          samples below `avail` (rx.c:246), else the launch ends.
 *     out: per launch int32 count and int32 calls made, then per block 8
 *          bytes info (call index, buf[11] after Demodulate, kind, 0, int32
 *          value), 11 bytes, 1 byte voice, 540 int16; then int32 pos,
 *          buf[12], the modem record, the link record, the receive-loop
 *          record.
 */
#include "crp.c"
#include "modem/modem.c"

#include <stdint.h>

void melpe_i(void);
void melpe_s(short *sp, unsigned char *buf);

#define STAGE (-101)
#define NOLOCK (-102)

struct rec {
	uint32_t cnt_out, cnt_in;
	float finv, fcrc;
	int32_t step;
	uint8_t scratch[6], rsv0[6];
	uint8_t skey[32], akey[32];
	float fdata[32];
	uint32_t rsv1[8];
};

struct rxrec {
	float fber, fau;
	uint32_t blocks, rsv;
};

/* the modem's statics in the layout of include/melpe_batch.h's record */
struct mrec {
	int32_t lastb, vadtr;
	uint32_t r[9], rr, dr;
	int32_t lag, cnt, u, cq;
	float fr[90], fd[90];
	float mlag, qq, f180, falign;
	float ffg[4][36];
	int8_t oldq, blk, lock, align;
};

static void restore(const struct rec *r)
{
	cnt_out = r->cnt_out;
	cnt_in = r->cnt_in;
	finv = r->finv;
	fcrc = r->fcrc;
	step = (char) r->step;
	memcpy(skey, r->skey, 32);
	memcpy(akey, r->akey, 32);
	memcpy(fdata, r->fdata, sizeof(r->fdata));
	memset(udata, 0, sizeof(udata));
	memcpy(udata, r->scratch, 6);
}

static void save(struct rec *r)
{
	memcpy(r->scratch, udata, 6);
	r->cnt_out = cnt_out;
	r->cnt_in = cnt_in;
	r->finv = finv;
	r->fcrc = fcrc;
	r->step = step;
	memcpy(r->skey, skey, 32);
	memcpy(r->akey, akey, 32);
	memcpy(r->fdata, fdata, sizeof(r->fdata));
}

int main(int argc, char **argv)
{
	if (argc != 3)
		return 1;
	FILE *fi = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
	if (!fi || !out || !freopen("/dev/null", "w", stdout))
		return 2;
	int32_t N, L;
	if (fread(&N, 4, 1, fi) != 1 || fread(&L, 4, 1, fi) != 1)
		return 2;
	int32_t *plan = malloc(8 * (size_t) L);
	struct rec lk;
	struct rxrec rx;
	short *pcm = malloc(2 * (size_t) N + 16);
	if (fread(plan, 8, L, fi) != (size_t) L || fread(&lk, sizeof lk, 1, fi) != 1 ||
	    fread(&rx, sizeof rx, 1, fi) != 1 || fread(pcm, 2, N, fi) != (size_t) N)
		return 2;
	fclose(fi);

	static unsigned char buf[12];
	short sp[540];
	float fber = rx.fber, fau = rx.fau;
	int32_t pos = 0;
	melpe_i();
	for (int l = 0; l < L; l++) {
		const int calls = plan[2 * l], avail = plan[2 * l + 1];
		long at = ftell(out);
		int32_t count = 0, made = 0;
		fwrite(&count, 4, 1, out);
		fwrite(&made, 4, 1, out);
		for (int k = 0; k < calls; k++) {
			unsigned char info[8] = {(unsigned char) k, 0, 0xEE, 0, 0, 0, 0, 0};
			int32_t val = NOLOCK;
			char lag_flag;
			int i;
			if (pos + 1080 > avail)
				break;
			i = Demodulate(pcm + pos, buf);
			pos += i;
			made++;
			if (0x80 & buf[11]) {
				info[1] = buf[11];
				info[2] = 0;
				lag_flag = !(!(buf[11] & 0x40));
				if (lag_flag) {
					i = (0x0F & buf[11]);
					fber *= 0.99;
					fber += i;
				}
				buf[11] = 0xFE;
				if (lag_flag) {
					if (lk.step < 5) {	/* the key-exchange stages are not the product's */
						val = STAGE;
						info[2] = 3;
					} else {
						restore(&lk);
						i = ProcessPkt(buf);
						save(&lk);
						val = i;
						if (i >= 0) {
							fau *= 0.99;
							fau += i;
							info[2] = 1;
						} else if (i == -3) {
							buf[11] = 0xFF;
							info[2] = 2;
						} else {
							return 3;
						}
					}
				}
				rx.blocks++;
			}
			if (0x0E & buf[11]) {	/* l_jit_buf <= 180 holds: it is 0 */
				unsigned char voice = 1 & buf[11];
				if (voice)
					melpe_s(sp, buf);
				else
					memset(sp, 0, 1080);
				memcpy(info + 4, &val, 4);
				fwrite(info, 1, 8, out);
				fwrite(buf, 1, 11, out);
				fwrite(&voice, 1, 1, out);
				fwrite(sp, 2, 540, out);
				buf[11] = 0;
				count++;
			}
		}
		long end = ftell(out);
		fseek(out, at, SEEK_SET);
		fwrite(&count, 4, 1, out);
		fwrite(&made, 4, 1, out);
		fseek(out, end, SEEK_SET);
	}
	rx.fber = fber;
	rx.fau = fau;
	struct mrec m;
	memset(&m, 0, sizeof m);
	m.lastb = lastb;
	m.vadtr = vadtr;
	memcpy(m.r, r, sizeof m.r);
	m.rr = rr;
	m.dr = dr;
	m.lag = lag;
	m.cnt = cnt;
	m.u = u;
	m.cq = cq;
	memcpy(m.fr, fr, sizeof m.fr);
	memcpy(m.fd, fd, sizeof m.fd);
	m.mlag = mlag;
	m.qq = qq;
	m.f180 = f180;
	m.falign = falign;
	memcpy(m.ffg, ffg, sizeof m.ffg);
	m.oldq = oldq;
	m.blk = blk;
	m.lock = lock;
	m.align = align;
	fwrite(&pos, 4, 1, out);
	fwrite(buf, 1, 12, out);
	fwrite(&m, sizeof m, 1, out);
	fwrite(&lk, sizeof lk, 1, out);
	fwrite(&rx, sizeof rx, 1, out);
	fclose(out);
	return 0;
}
