/*
 * k_ana_eval.hip -- the function-level parity test of the encoder's pitch
 * and voicing analysis on the device (ana_eval.h): built like the codec
 * kernels (the whole call tree inline, its own table upload), so the
 * functions are compiled the way k_enc_ana runs them.
 *
 * k_ana_eval: one lane per case, each on a private window and a private,
 * zeroed analysis state (the codec's lanes work in the private segment, at
 * per-lane offsets), so a wave mixes lanes that take different arms of the
 * same function.  A sequence of calls reads each call's inputs from the
 * case's row in global memory into the one window.
 * k_ana_scalar: the pitch tracker's scalars, one thread per case.
 */
#include "kern.h"
#include "ana_eval.h"

MELPE_TU(anaeval)

/* The lane's analysis state stops where the superframe's speech history and
 * melp_ana's work buffer begin (EncAna's last two members): no mode reads
 * them, and without them the kernel's private segment stays below
 * k_enc_ana's, so the queue's scratch reservation does not grow. */
#define AE_STATE_BYTES offsetof(EncAna, hpspeech)
static_assert(AE_STATE_BYTES % 4 == 0 && offsetof(EncAna, sigbuf) > AE_STATE_BYTES &&
	      offsetof(EncAna, sigbuf) + sizeof(int16_t) * SIG_LENGTH + 16 > sizeof(EncAna),
	      "hpspeech and sigbuf are the members that end EncAna");

__global__ __launch_bounds__(WAVE) void k_ana_eval(int mode, const int16_t *in, const int32_t *args,
						   int32_t *out, int n)
{
	int i = blockIdx.x * WAVE + threadIdx.x;
	if (i >= n)
		return;
	struct {
		uint8_t guard[FLAT_GUARD_BYTES];
		alignas(4) int16_t b[AE_WIN];
		int32_t a[AE_ARGS];
		int32_t r[AE_RET];
		alignas(16) u32_alias E[AE_STATE_BYTES / 4];
	} L;
	PIN_FRAME(L);
	for (int k = 0; k < AE_WIN; k++)
		L.b[k] = 0;
	for (int k = 0; k < AE_ARGS; k++)
		L.a[k] = args[(size_t) i * AE_ARGS + k];
	for (int k = 0; k < AE_RET; k++)
		L.r[k] = 0;
	for (unsigned k = 0; k < AE_STATE_BYTES / 4; k++)
		L.E[k] = 0;
	ae_eval(mode, in + (size_t) i * AE_IN, L.b, reinterpret_cast<EncAna *>(L.E), L.a, L.r);
	int32_t *o = out + (size_t) i * AE_OUT;
	for (int k = 0; k < AE_RET; k++)
		o[k] = L.r[k];
	for (int k = 0; k < AE_WIN; k++)
		o[AE_RET + k] = L.b[k];
}

__global__ __launch_bounds__(256) void k_ana_scalar(int mode, const int32_t *args, int32_t *out, long n)
{
	long i = blockIdx.x * (long) blockDim.x + threadIdx.x;
	if (i >= n)
		return;
	const int32_t *a = args + 4 * i;
	out[i] = ae_scalar(mode, a[0], a[1], a[2], a[3]);
}

extern "C" int kl_ana_scalar(int mode, const int32_t *args, int32_t *out, long n, hipStream_t s)
{
	k_ana_scalar<<<(unsigned) ((n + 255) / 256), 256, 0, s>>>(mode, args, out, n);
	return (int) hipGetLastError();
}

extern "C" int kl_ana_eval(int mode, const int16_t *in, const int32_t *args, int32_t *out, int n,
			   hipStream_t s)
{
	k_ana_eval<<<grid_for(n), WAVE, 0, s>>>(mode, in, args, out, n);
	return (int) hipGetLastError();
}
