/*
 * golay.h -- the extended Golay(24,12) code that protects PairPhone's control
 * packets (crp.c:331-426 EncodeBlock / DecodeBlock call
 * fec/fec_golay2412.c:101-213 three times per packet).
 *
 * The reference multiplies by its generator and parity-check matrices with
 * byte-wise popcount tables and walks the two parity searches with early
 * returns.  Both matrices are [I | P] forms of one 12 x 12 matrix P, so here
 * everything is 12 parities of popc(P[i] & v) with P as immediates:
 *
 *   encode(m)   = (m.P) << 12 | m		(Gt rows 12..23 are unit vectors)
 *   syndrome(r) = (r & 0xfff).P ^ (r >> 12)	(H[i] = 1 << (23 - i) | P[i])
 *
 * and the searches are 12 unrolled popcount tests run from the last row to
 * the first, so the first hit is the one kept.  The result equals the
 * reference for all 2^24 received words (melpe_golay_sweep_dev,
 * tests/test_link.py), its quirks included: step 5 accepts a weight of 2 or 3
 * only (a weight of 0 or 1 falls through to the second search), and 0x1000
 * is returned for an uncorrectable word.
 *
 * Shared by the GPU kernels (k_link.hip) and the host-emulation build.
 */
#ifndef MELPE_GOLAY_H
#define MELPE_GOLAY_H

#include <stdint.h>

#ifndef MELPE_HD
#if defined(__HIPCC__)
#define MELPE_HD __host__ __device__
#else
#define MELPE_HD
#endif
#endif

#define GOLAY_FAIL 0x1000u

/* row i of P (fec/fec_golay2412.c:53-56) */
static MELPE_HD inline uint32_t golay_p(int i)
{
	const uint32_t P[12] = {0x8ed, 0x1db, 0x3b5, 0x769, 0xed1, 0xda3,
				0xb47, 0x68f, 0xd1d, 0xa3b, 0x477, 0xffe};
	return P[i];
}

/* v.P: bit 11 - i = parity(P[i] & v) */
static MELPE_HD inline uint32_t golay_mul_p(uint32_t v)
{
	uint32_t x = 0;
#pragma unroll
	for (int i = 0; i < 12; i++)
		x = (x << 1) | ((uint32_t) __builtin_popcount(golay_p(i) & v) & 1u);
	return x;
}

/* golay2412_parity_search: the first i with w(v ^ P[i]) <= 2.  Returns
 * whether there is one, with its row P[i] and its unit vector 1 << (11 - i) */
static MELPE_HD inline bool golay_search(uint32_t v, uint32_t *row, uint32_t *unit)
{
	bool hit = false;
	uint32_t p = 0, u = 0;
#pragma unroll
	for (int i = 11; i >= 0; i--) {
		const bool h = __builtin_popcount(v ^ golay_p(i)) <= 2;
		hit = hit || h;
		p = h ? golay_p(i) : p;
		u = h ? (0x800u >> i) : u;
	}
	*row = p;
	*unit = u;
	return hit;
}

static MELPE_HD inline uint32_t fec_golay2412_encode_symbol(uint32_t m)
{
	return (golay_mul_p(m) << 12) | (m & 0xfffu);
}

static MELPE_HD inline uint32_t fec_golay2412_decode_symbol(uint32_t r)
{
	const uint32_t s = golay_mul_p(r & 0xfffu) ^ ((r >> 12) & 0xfffu);
	const uint32_t sP = golay_mul_p(s);
	const int ws = __builtin_popcount(s), wsP = __builtin_popcount(sP);
	uint32_t p1, u1, p2, u2;
	const bool t3 = golay_search(s, &p1, &u1), t6 = golay_search(sP, &p2, &u2);
	/* steps 2, 3, 5 and 6 of the reference, the first that applies */
	const uint32_t e2 = (s << 12) & 0xfff000u;
	const uint32_t e3 = ((s ^ p1) << 12) | u1;
	const uint32_t e5 = sP;
	const uint32_t e6 = (u2 << 12) | (sP ^ p2);
	const bool t2 = ws <= 3, t5 = wsP == 2 || wsP == 3;
	const uint32_t e = t2 ? e2 : t3 ? e3 : t5 ? e5 : e6;
	return (t2 || t3 || t5 || t6) ? ((r ^ e) & 0xfffu) : GOLAY_FAIL;
}

#endif
