/*
 * stream_fmt.h -- the VAD-framed stream format of the reference's file
 * codec (melpe_enc.c:55-72 writes it, melpe_dec.c:33-49 reads it): the frame
 * rules in one place.
 *
 * Per superframe a channel writes either
 *   silence: 1 byte, the carried txbuf[0] (the first byte of the channel's
 *            last frame) with bit 1 set (melpe_enc.c:57-59), or
 *   voiced:  its 11 bytes with bytes 0 and 10 swapped (melpe_enc.c:64-70).
 *            Byte 10 of a 1200 bps superframe holds bit 80 only, so the first
 *            byte of a voiced frame never has bit 1 set;
 * and the reader tells them apart by bit 1 of the first byte
 * (melpe_dec.c:35).
 *
 * Shared by the stream kernels (k_line.hip k_stream_*) and the host
 * functions melpe_stream_pack / melpe_stream_unpack.
 */
#ifndef MELPE_STREAM_FMT_H
#define MELPE_STREAM_FMT_H

#include <stdint.h>

#if defined(__HIPCC__)
#define SFMT_FN __host__ __device__ static inline
#else
#define SFMT_FN static inline
#endif

#define SFMT_BYTES 11		/* a voiced frame: one 1200 bps superframe */
#define SFMT_SILENT 2		/* bit 1 of a frame's first byte */
#define SFMT_TRUNCATED 0xFF	/* receive: a voiced frame cut off by the stream's end */

/* bytes a channel writes for one superframe (0: the channel is masked out) */
SFMT_FN unsigned sfmt_frame_len(int active, unsigned vote)
{
	return !active ? 0u : vote ? (unsigned) SFMT_BYTES : 1u;
}

/* writes the frame of one superframe (b: its 11 bytes, vote: its VAD votes,
 * last: the channel's carried byte) to o, sfmt_frame_len(1, vote) bytes;
 * returns the new carried byte */
SFMT_FN uint8_t sfmt_pack(const unsigned char *b, unsigned vote, uint8_t last, unsigned char *o)
{
	if (vote == 0) {	/* melpe_enc.c:57-59: VAD flag on the carried txbuf[0] */
		last |= SFMT_SILENT;
		o[0] = last;
		return last;
	}
	const uint8_t first = b[10];	/* melpe_enc.c:64-70: bytes 0 and 10 swapped */
	o[0] = first;
	for (int j = 1; j < SFMT_BYTES - 1; j++)
		o[j] = b[j];
	o[10] = b[0];
	return first;
}

/* melpe_dec.c:35: a frame is silence when bit 1 of its first byte is set */
SFMT_FN int sfmt_is_silent(unsigned first)
{
	return (first & SFMT_SILENT) != 0;
}

/* the length of the frame that starts with `first` when `avail` (>= 1) bytes
 * of the stream are left: 1, 11, or SFMT_TRUNCATED for a voiced frame that
 * the stream's end cuts off (melpe_dec.c:42 reads its other 10 bytes
 * unchecked; here such a frame is an error of that stream) */
SFMT_FN unsigned sfmt_rx_len(unsigned first, unsigned long avail)
{
	if (sfmt_is_silent(first))
		return 1u;
	return avail >= SFMT_BYTES ? (unsigned) SFMT_BYTES : (unsigned) SFMT_TRUNCATED;
}

/* a voiced frame f back to the superframe's 11 bytes b (the swap undone) */
SFMT_FN void sfmt_unswap(const unsigned char *f, unsigned char *b)
{
	b[0] = f[10];
	for (int j = 1; j < SFMT_BYTES - 1; j++)
		b[j] = f[j];
	b[10] = f[0];
}

#endif
