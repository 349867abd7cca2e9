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
 * k_ops_eval, k_divide_s_sweep: the basic operators of ops.h (ops_eval.h).
 * k_helpers_eval: the device-only stream and correlator helpers
 * (helpers_eval.h).
 */
#include "kern.h"
#include "dsp_eval.h"
#include "ops_eval.h"
#include "helpers_eval.h"

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

/* device basic-op parity test: out[i] = op(a[i], b[i], c[i]) with the
 * device build of ops.h (ops_eval.h) */
__global__ __launch_bounds__(256) void k_ops_eval(int op, const int64_t *A, const int32_t *B,
						  const int32_t *C, int64_t *out, long n)
{
	long i = blockIdx.x * (long) blockDim.x + threadIdx.x;
	if (i >= n)
		return;
	int64_t a = A[i];
	int32_t b = B ? B[i] : 0, c = C ? C[i] : 0;
	int64_t r = 0;
	switch (op) {
#define OPS_CASE(id, name, call) case id: r = (int64_t) (call); break;
	MELPE_OPS_EVAL_LIST(OPS_CASE)
#undef OPS_CASE
	default: r = 0;
	}
	out[i] = r;
}

/* divide_s over its whole domain, 0 <= num <= den < 2^15 (den >= 1): one
 * thread per denominator sums q(num) * (num * 0x9E3779B97F4A7C15 + 1) over
 * every numerator in uint64 arithmetic -- a digest that any wrong quotient
 * changes (tests/test_device_ops.py forms the same sums from the
 * reference's divide_s) */
__global__ __launch_bounds__(256) void k_divide_s_sweep(uint64_t *digest)
{
	const int den = blockIdx.x * blockDim.x + threadIdx.x + 1;
	if (den > 32767)
		return;
	uint64_t h = 0;
	for (int num = 0; num <= den; num++)
		h += (uint64_t) (uint16_t) divide_s((Word16) num, (Word16) den) *
		     ((uint64_t) num * 0x9E3779B97F4A7C15ull + 1u);
	digest[den - 1] = h;
}

/* device helper self-test (helpers_eval.h): lane i copies its HE_N
 * samples into a private array -- the codec's streams read the private
 * segment, at per-lane alignments -- and runs helper `mode` on it with
 * (a, b, len) = args[4i .. 4i+2], HE_OUT int32 results per lane */
__global__ __launch_bounds__(WAVE) void k_helpers_eval(int mode, const int16_t *src, const int32_t *args,
						       int32_t *out, int n)
{
	int i = blockIdx.x * WAVE + threadIdx.x;
	if (i >= n)
		return;
	struct {
		uint8_t guard[FLAT_GUARD_BYTES];
		int16_t buf[HE_N];
		int32_t o[HE_OUT];
	} L;
	PIN_FRAME(L);
	for (int k = 0; k < HE_N; k++)
		L.buf[k] = src[(size_t) i * HE_N + k];
	for (int k = 0; k < HE_OUT; k++)
		L.o[k] = 0;
	he_eval(mode, L.buf, args[4 * i], args[4 * i + 1], args[4 * i + 2], L.o);
	for (int k = 0; k < HE_OUT; k++)
		out[(size_t) i * HE_OUT + k] = L.o[k];
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

extern "C" int kl_ops_eval(int op, const int64_t *a, const int32_t *b, const int32_t *c, int64_t *out, long n,
			   hipStream_t s)
{
	k_ops_eval<<<(unsigned) ((n + 255) / 256), 256, 0, s>>>(op, a, b, c, out, n);
	return (int) hipGetLastError();
}

extern "C" int kl_divide_s_sweep(uint64_t *digest, hipStream_t s)
{
	k_divide_s_sweep<<<(32767 + 255) / 256, 256, 0, s>>>(digest);
	return (int) hipGetLastError();
}

extern "C" int kl_helpers_eval(int mode, const int16_t *src, const int32_t *args, int32_t *out, int n,
			       hipStream_t s)
{
	k_helpers_eval<<<grid_for(n), WAVE, 0, s>>>(mode, src, args, out, n);
	return (int) hipGetLastError();
}
