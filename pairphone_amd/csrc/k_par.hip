/*
 * k_par.hip -- the codec's own description of a superframe as device
 * tensors: melp_par (NF rows of MelpParam, 30 int16 each) and quant_par (30
 * int16, oracle/ref_tool.c dump_quant's order = QuantParam's field order).
 *
 * k_par_tap copies the parameters the last melpe_a / melpe_s left in the
 * channels' records (EncAna::par, qpar / DecState::par) into row tensors.
 * k_parse is melpe_s without the synthesis: the channel read and the head of
 * melp_syn that owns the parameters (decoder.h parse_superframe), bits in,
 * parameter rows out, no PCM.
 */
#include "kern.h"
#include "../../include/melpe_batch.h"

MELPE_TU(par)

#define PAR_DW ((int) (sizeof(MelpParam) * NF / 4))	/* 45 dwords per channel */
#define QPAR_DW ((int) (sizeof(QuantParam) / 4))	/* 15 */
#define TAP_DW (PAR_DW + QPAR_DW)

static_assert(sizeof(MelpParam) == 2 * MELPE_PAR_WORDS && sizeof(QuantParam) == 2 * MELPE_QPAR_WORDS,
	      "the public row sizes (melpe_batch.h)");
static_assert(sizeof(MelpParam) * NF % 4 == 0 && sizeof(QuantParam) % 4 == 0, "rows move as dwords");
static_assert(offsetof(EncAna, qpar) == offsetof(EncAna, par) + sizeof(MelpParam) * NF &&
	      offsetof(DecState, qpar) == offsetof(DecState, par) + sizeof(MelpParam) * NF,
	      "par[NF] and qpar are one contiguous block of a record");
static_assert((offsetof(EncState, a) + offsetof(EncAna, par)) % 4 == 0 && offsetof(DecState, par) % 4 == 0 &&
	      sizeof(EncState) % 4 == 0 && sizeof(DecState) % 4 == 0, "the block is dword-aligned");
static_assert(offsetof(QuantParam, lsf_index) == 2 && offsetof(QuantParam, gain_index) == 26 &&
	      offsetof(QuantParam, jit_index) == 30 && offsetof(QuantParam, bpvc_index) == 36 &&
	      offsetof(QuantParam, fs_index) == 42 && offsetof(QuantParam, uv_flag) == 44 &&
	      offsetof(QuantParam, msvq_index) == 50 && offsetof(QuantParam, fsvq_index) == 58,
	      "QuantParam's field order is dump_quant's word order");

/*
 * The tap.  The block is 240 bytes of a record several KB long, so a lane
 * per channel would touch 64 records for 64 dwords.  Here thread i moves
 * dword i % 60 of channel i / 60: a wave reads 64 consecutive dwords of one
 * or two channels' blocks and writes 64 consecutive dwords of the row
 * tensors (split where a channel's par row ends and its qpar row begins).
 * rec + c * stride + off is channel c's par[0]; qpar NULL = not wanted.
 */
#define TAP_BLOCK 256

__global__ __launch_bounds__(TAP_BLOCK) void k_par_tap(const char *rec, size_t stride, size_t off, uint32_t *par,
						       uint32_t *qpar, const uint8_t *active, int n)
{
	const size_t i = (size_t) blockIdx.x * TAP_BLOCK + threadIdx.x;
	const size_t c = i / TAP_DW;
	const int d = (int) (i % TAP_DW);
	if (c >= (size_t) n || (active && !active[c]))
		return;
	if (d >= PAR_DW && !qpar)
		return;
	const uint32_t v = *(const u32_alias *) (rec + c * stride + off + 4 * (size_t) d);
	if (d < PAR_DW)
		par[c * PAR_DW + d] = v;
	else
		qpar[c * QPAR_DW + (d - PAR_DW)] = v;
}

extern "C" int kl_par_tap(const char *rec, size_t stride, size_t off, uint32_t *par, uint32_t *qpar,
			  const uint8_t *active, int n, hipStream_t s)
{
	if (n <= 0)
		return 0;
	const size_t threads = (size_t) n * TAP_DW;
	k_par_tap<<<(unsigned) ((threads + TAP_BLOCK - 1) / TAP_BLOCK), TAP_BLOCK, 0, s>>>(rec, stride, off, par, qpar,
											   active, n);
	return (int) hipGetLastError();
}

/*
 * The parse kernel: one lane per channel, lane g on channel g (no lane-order
 * sort: the channel read and the parameter head are a few thousand
 * operations with short branches, nothing like the synthesis' per-pitch
 * loops the sort exists for, and the sort would cost a launch of its own).
 * The lane's private frame holds only the excitation side of the record,
 * [0, DEC_B_BEG): everything parse_superframe touches lies there.  A block
 * is one wave; its 64 rows are one contiguous run of the output tensor, so
 * they go through LDS and out as 45 coalesced dword stores per lane (lane
 * l's row at l * 45: the odd stride keeps the LDS writes conflict-free).
 */
struct ParseLane {
	uint8_t guard[FLAT_GUARD_BYTES];
	alignas(16) uint8_t s[DEC_B_BEG];	/* DecState's excitation side */
};
static_assert(offsetof(ParseLane, s) % 16 == 0 && DEC_B_BEG % 16 == 0, "16-byte record copy");
static_assert(offsetof(DecState, chbuf) + 12 <= DEC_B_BEG && offsetof(DecState, rd_prev_gain) < DEC_B_BEG &&
	      offsetof(DecState, prev_par) + sizeof(MelpParam) <= DEC_B_BEG &&
	      offsetof(DecState, noise_gain) < DEC_B_BEG && offsetof(DecState, erase) < DEC_B_BEG,
	      "the parse path's fields lie in the excitation side");

__global__ __launch_bounds__(WAVE) void k_parse(DecState *dec, uint32_t *par, const uint8_t *bits,
						const uint8_t *active, int n)
{
	__shared__ uint32_t rows[WAVE * PAR_DW];
	const int t = threadIdx.x;
	const int c = blockIdx.x * WAVE + t;
	const bool live = c < n && (!active || active[c]);
	if (live) {
		ParseLane L;
		PIN_FRAME(L);
		DecState *D = (DecState *) L.s;
		lane_copy_x4(L.s, &dec[c], DEC_B_BEG);
		for (int k = 0; k < 11; k++)
			D->chbuf[k] = bits[(size_t) c * 11 + k];
		parse_superframe(D);
		lane_copy_x4(&dec[c], L.s, DEC_B_BEG);
		const u32_alias *p = (const u32_alias *) D->par;
		for (int k = 0; k < PAR_DW; k++)
			rows[t * PAR_DW + k] = p[k];
	}
	__syncthreads();
	const unsigned long long m = __ballot(live);
	uint32_t *out = par + (size_t) blockIdx.x * WAVE * PAR_DW;
	for (int k = 0; k < PAR_DW; k++) {
		const int j = k * WAVE + t;
		if ((m >> (j / PAR_DW)) & 1)	/* rows of inactive channels are not written */
			out[j] = rows[j];
	}
}

extern "C" int kl_parse(DecState *dec, uint32_t *par, const uint8_t *bits, const uint8_t *active, int n,
			hipStream_t s)
{
	if (n <= 0)
		return 0;
	k_parse<<<grid_for(n), WAVE, 0, s>>>(dec, par, bits, active, n);
	return (int) hipGetLastError();
}

extern "C" size_t kl_parse_private(void)
{
	return private_bytes((const void *) k_parse);
}
