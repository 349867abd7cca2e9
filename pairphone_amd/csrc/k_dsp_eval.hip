/*
 * k_dsp_eval.hip -- the function-level parity test of the DSP and math
 * library on the device (dsp_eval.h): built like the codec kernels (the
 * whole call tree inline, its own table upload), so the functions are
 * compiled the way the codec runs them.
 *
 * k_dsp_eval: one lane per case, each on a private copy of its row (the
 * codec's lanes work in the private segment, at per-lane offsets), so a wave
 * mixes lanes that take different arms of the same function and wave-wide
 * predicates (lpc_syn's wave_all) see mixed lanes.
 * k_dsp_scalar: the scalar math functions, one thread per case, tables read
 * from the blob (the LDS copy of the NPP kernels is tested in k_npp.hip).
 */
#include "kern.h"
#include "dsp_eval.h"

MELPE_TU(dspeval)

__global__ __launch_bounds__(WAVE) void k_dsp_eval(int mode, const int16_t *in, const int32_t *args,
						   int32_t *out, int n)
{
	int i = blockIdx.x * WAVE + threadIdx.x;
	if (i >= n)
		return;
	struct {
		uint8_t guard[FLAT_GUARD_BYTES];
		alignas(4) int16_t b[DE_IN];
		int32_t a[DE_ARGS];
		int32_t r[DE_RET];
	} L;
	PIN_FRAME(L);
	for (int k = 0; k < DE_IN; k++)
		L.b[k] = in[(size_t) i * DE_IN + k];
	for (int k = 0; k < DE_ARGS; k++)
		L.a[k] = args[(size_t) i * DE_ARGS + k];
	for (int k = 0; k < DE_RET; k++)
		L.r[k] = 0;
	de_eval(mode, L.b, L.a, L.r);
	int32_t *o = out + (size_t) i * DE_OUT;
	for (int k = 0; k < DE_RET; k++)
		o[k] = L.r[k];
	for (int k = 0; k < DE_IN; k++)
		o[DE_RET + k] = L.b[k];
}

__global__ __launch_bounds__(256) void k_dsp_scalar(int mode, const int32_t *args, int32_t *out, long n)
{
	long i = blockIdx.x * (long) blockDim.x + threadIdx.x;
	if (i >= n)
		return;
	const int32_t *a = args + 4 * i;
	out[i] = de_scalar(mode, a[0], a[1], a[2], a[3]);
}

extern "C" int kl_dsp_eval(int mode, const int16_t *in, const int32_t *args, int32_t *out, int n,
			   hipStream_t s)
{
	k_dsp_eval<<<grid_for(n), WAVE, 0, s>>>(mode, in, args, out, n);
	return (int) hipGetLastError();
}

extern "C" int kl_dsp_scalar(int mode, const int32_t *args, int32_t *out, long n, hipStream_t s)
{
	k_dsp_scalar<<<(unsigned) ((n + 255) / 256), 256, 0, s>>>(mode, args, out, n);
	return (int) hipGetLastError();
}
