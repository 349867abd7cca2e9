"""Function-level parity of the DSP and math library (pairphone_amd/csrc/dsp.h,
npp_wave.h wv_cfft256, k_harm.hip wv_find_harm, analysis.h find_harm) with the
reference's own functions, one function at a time.

Every function is run through pairphone_amd/csrc/dsp_eval.h -- by the host
build (emu_dsp_eval / emu_dsp_scalar: the CPU tests) and on the device
(melpe_dsp_eval_dev, melpe_dsp_scalar_dev, melpe_dsp_wave_dev: the GPU
tests) -- on inputs built to reach every dispatch arm, remainder loop and
guard threshold of the gfx950 forms, and must be bit-equal to what
oracle/_ref/ref_dsp (oracle/ref_dsp.c: the reference's functions, out of
process because its asserts are live) gives for the same cases.  The mode
ids and the case layout are parsed from csrc/dsp_eval_modes.h.  For the
device-only fused forms the expected value is the sequence of reference
calls the form's comment claims to equal.

The reference runs once per mode; CPU and GPU tests share its result.
"""
import ctypes
import functools
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import REF_DIR, ROOT
from test_device_ops import E32, all16, r32, second16

CSRC = os.path.join(ROOT, "pairphone_amd", "csrc")
EMU = os.path.join(ROOT, "build", "libmelpe_hostemu.so")
TABLES = os.path.join(ROOT, "pairphone_amd", "data", "melpe_tables.bin")
REF_DSP = os.path.join(REF_DIR, "ref_dsp")

HDR = open(os.path.join(CSRC, "dsp_eval_modes.h")).read()


def _num(name):
    return int(re.search(r"#define %s (\d+)" % name, HDR).group(1))


def _modes(macro):
    body = HDR[HDR.index("#define %s(" % macro):]
    body = body[:body.index("\n#define", 1)]
    return {m.group(2): int(m.group(1)) for m in re.finditer(r"\b[XS]\((\d+), (\w+)", body)}


DE_IN, DE_ARGS, DE_RET, DE_DATA, DE_WV_IN = (_num(k) for k in ("DE_IN", "DE_ARGS", "DE_RET", "DE_DATA", "DE_WV_IN"))
DE_OUT, DE_WV_OUT = DE_RET + DE_IN, DE_RET + DE_WV_IN
VMODES, SMODES, WMODES = _modes("DE_MODES"), _modes("DE_SCALAR_MODES"), _modes("DE_WAVE_MODES")
LDS_LAST = _num("DE_SCALAR_LDS_LAST")
assert len(VMODES) == _num("DE_MODE_COUNT") and len(SMODES) == _num("DE_SCALAR_COUNT")
assert len(WMODES) == _num("DE_WAVE_COUNT")

N = 512		# lanes per vector mode
LPC_FRAME, PITCH_FR = 200, 321
MIN16, MAX16 = -32768, 32767


def table(name):
    gen = open(os.path.join(CSRC, "tables_gen.h")).read()
    off = int(re.search(r"#define TOFF_%s (\d+)" % name, gen).group(1))
    ln = int(re.search(r"#define TLEN_%s (\d+)" % name, gen).group(1))
    return np.fromfile(TABLES, np.int16)[off:off + ln].copy()


# ---------------------------------------------------------------- reference

def ref_run(kind, mode, inp, args):
    """oracle/_ref/ref_dsp on one mode's cases"""
    assert os.path.exists(REF_DSP), "oracle/_ref/ref_dsp missing: run __graft_entry__.build() where the reference is"
    n = len(args)
    with tempfile.TemporaryDirectory() as tmp:
        fi, fo = os.path.join(tmp, "in"), os.path.join(tmp, "out")
        with open(fi, "wb") as f:
            if inp is not None:
                f.write(np.ascontiguousarray(inp, np.int16).tobytes())
            f.write(np.ascontiguousarray(args, np.int32).tobytes())
        r = subprocess.run([REF_DSP, kind, str(mode), str(n), fi, fo], capture_output=True, text=True)
        assert r.returncode == 0, "ref_dsp %s %d: exit %d %s" % (kind, mode, r.returncode, r.stderr[-300:])
        out = np.fromfile(fo, np.int32)
    return out if kind == "s" else out.reshape(n, -1)


def first_diff(what, got, want, describe=None, where=None):
    """exact equality; the message names the mode, the case and the first
    differing output (where(j): what output j of a case is, e.g. the call of
    a sequence it belongs to)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: shape %s, reference %s" % (what, got.shape, want.shape)
    if np.array_equal(got, want):
        return
    bad = np.argwhere(got != want)
    idx = tuple(int(v) for v in bad[0])
    extra = " [%s]" % describe(idx[0]) if describe else ""
    out = idx[1:] if len(idx) > 1 else ""
    if where and len(idx) == 2:
        out = "%d (%s)" % (idx[1], where(idx[1]))
    pytest.fail("%s: %d outputs differ in %d cases; first: case %d%s output %s = %d, reference %d" % (
        what, len(bad), len(np.unique(bad[:, 0])), idx[0], extra, out, got[idx], want[idx]))


# ------------------------------------------------------------- scalar cases

def _pow2_edges():
    k = np.arange(0, 31, dtype=np.int64)
    v = np.concatenate([2**k - 1, 2**k, 2**k + 1, [2**31 - 1, 0]])
    return np.unique(v[(v >= 0) & (v < 2**31)])


def _x32(g):
    """x >= 0: powers of two with neighbours, test_device_ops' E32, and ~1 M
    edge-weighted random values"""
    edge = np.unique(np.concatenate([_pow2_edges(), E32[E32 >= 0]]))
    rnd = r32(g, 2_000_000)
    return edge, rnd[rnd >= 0]


def _neigh(v):
    return [v - 1, v, v + 1]


# L_pow_fxp(x, power, Q_in, Q_out) as the codec calls it (quant.h:26, :113)
POW_SITES = [(-9830, 19, 11), (22609, 28, 13)]


@functools.lru_cache(maxsize=None)
def scalar_cases(name):
    g = np.random.default_rng(20261019 + SMODES[name])
    z = lambda a: np.zeros(len(a), np.int64)
    if name in ("log10_fxp", "sqrt_fxp", "pow10_fxp"):
        x = all16() if name == "pow10_fxp" else np.arange(0, 32768, dtype=np.int64)
        a, b = (v.ravel() for v in np.meshgrid(x, np.arange(16), indexing="ij"))
        c = d = z(a)
    elif name in ("L_log10_fxp", "L_sqrt_fxp"):
        edge, rnd = _x32(g)
        ea, eb = (v.ravel() for v in np.meshgrid(edge, np.arange(32), indexing="ij"))
        a, b = np.concatenate([ea, rnd]), np.concatenate([eb, g.integers(0, 32, len(rnd))])
        c = d = z(a)
    elif name == "L_pow_fxp":
        edge, rnd = _x32(g)
        combos = np.array([(p, qi, qo) for s in POW_SITES for p in _neigh(s[0]) for qi in _neigh(s[1])
                           for qo in _neigh(s[2])], np.int64)
        ea, ek = (v.ravel() for v in np.meshgrid(edge, np.arange(len(combos)), indexing="ij"))
        k = np.concatenate([ek, g.integers(0, len(combos), len(rnd))])
        a = np.concatenate([ea, rnd])
        b, c, d = combos[k, 0], combos[k, 1], combos[k, 2]
    elif name in ("sin_fxp", "cos_fxp", "sqrt_Q15"):
        a = all16()
        b = c = d = z(a)
    elif name in ("add_shr", "interp_scalar"):
        # the two-operand grid of test_device_ops' add
        a, b = (v.ravel() for v in np.meshgrid(all16(), second16(g), indexing="ij"))
        c = d = z(a)
        if name == "interp_scalar":
            f = np.array([0, 1, 16383, 16384, 32766, 32767], np.int64)
            k = np.arange(len(a)) % 8
            c = np.where(k < 6, f[np.minimum(k, 5)], g.integers(0, 32768, len(a)))
    elif name == "L_divider2":
        M = 2_000_000
        den = r32(g, M)
        # half the numerators a random fraction of the denominator (either
        # sign), so that the asserted precondition holds often
        frac = (np.abs(den) * g.random(M)).astype(np.int64) * np.where(g.random(M) < 0.5, -1, 1)
        num = np.where(g.random(M) < 0.5, frac, r32(g, M))
        nsh, dsh = g.integers(0, 5, M), g.integers(-2, 3, M)
        codec = g.random(M) < 0.5	# the codec's own shifts: (0, 0) and (2, 0)
        nsh = np.where(codec, np.where(g.random(M) < 0.5, 0, 2), nsh)
        dsh = np.where(codec, 0, dsh)
        # the reference's asserted precondition, from the inputs alone:
        # denom != 0 and, after the shifts, L_abs and the halving loop,
        # numer <= denom (math_lib.c:113, :131)
        dd = np.where(dsh >= 0, np.clip(den << np.maximum(dsh, 0), -2**31, 2**31 - 1), den >> np.maximum(-dsh, 0))
        dd = np.minimum(np.abs(dd), 2**31 - 1)
        nn = np.minimum(np.abs(num >> nsh), 2**31 - 1)
        k = np.zeros(M, np.int64)
        for _ in range(17):
            big = dd > 32767
            dd = np.where(big, dd >> 1, dd)
            k += big
        nn >>= k
        ok = (den != 0) & (nn <= dd)
        a, b, c, d = num[ok], den[ok], nsh[ok], dsh[ok]
        sign = (a < 0) * 2 + (b < 0)
        assert all((sign == s).sum() > 50_000 for s in range(4)), "all four sign combinations"
        small = np.abs(np.where(d >= 0, b << np.maximum(d, 0), b >> np.maximum(-d, 0))) <= 32767
        assert small.sum() > 50_000 and (~small).sum() > 50_000, "denominators on both sides of 32767"
    else:
        raise KeyError(name)
    args = np.stack([a, b, c, d], axis=1).astype(np.int32)
    return np.ascontiguousarray(args)


@functools.lru_cache(maxsize=None)
def scalar_want(name):
    return ref_run("s", SMODES[name], None, scalar_cases(name))


def describe_scalar(name):
    args = scalar_cases(name)
    return lambda i: "%s(%s)" % (name, ", ".join(str(v) for v in args[i]))


# ------------------------------------------------------------- vector cases

def signal(g, n, width):
    """per-lane signals from near silence to full scale, every eighth lane on
    the extremes alone (chains that saturate)"""
    amp = np.array([30, 1000, 12000, 32768])[np.arange(n) % 4]
    v = (g.random((n, width)) * 2 - 1) * amp[:, None]
    v = np.clip(np.rint(v), MIN16, MAX16)
    ext = np.arange(n) % 8 == 5
    e = np.where(g.random((n, width)) < 0.5, MIN16, MAX16)
    v[ext] = e[ext]
    return v.astype(np.int16)


def biquads(g, n, k, tables):
    """k sections per lane, den / num triples: the codec's tables on the
    first lanes, then random stable sections (poles r e^{+-j theta}, r < 1,
    in the tables' convention den = -8192, 2 r cos(theta) 8192, -r^2 8192)"""
    den, num = np.zeros((n, 3 * k), np.int64), np.zeros((n, 3 * k), np.int64)
    r = g.uniform(0.3, 0.995, (n, k))
    th = g.uniform(0.05, 3.1, (n, k))
    den[:, 0::3] = -8192
    den[:, 1::3] = np.rint(2 * r * np.cos(th) * 8192)
    den[:, 2::3] = np.rint(-r * r * 8192)
    num[:] = g.integers(-16384, 16385, (n, 3 * k))
    for i in range(n):
        if i % 3 == 0 and tables:
            d, m = tables[(i // 3) % len(tables)]
            den[i], num[i] = d, m
    return den.astype(np.int16), num.astype(np.int16)


def memories(g, n, width, lo=MIN16, hi=MAX16):
    m = g.integers(lo, hi + 1, (n, width))
    full = np.arange(n) % 4 == 3
    m[full] = np.where(g.random((full.sum(), width)) < 0.5, lo, hi)
    return m.astype(np.int16)


def fft_frames(extra_random):
    """the FFT family's inputs, 512 int16 each (256 complex points, or 512
    real ones)"""
    g = np.random.default_rng(77)
    F = [np.zeros(512, np.int64)]
    for v in (32767, -32767, -32768):
        for pos in (0, 1, 256, 511):
            f = np.zeros(512, np.int64)
            f[pos] = v
            F.append(f)
    F += [np.full(512, 32767), np.full(512, -32768)]
    F.append(np.where(np.arange(512) % 2 == 0, 32767, -32768))
    k = np.arange(256)
    for b in (1, 64, 127, 128):	# these grow by two at every stage
        f = np.zeros(512, np.int64)
        f[0::2] = np.rint(32767 * np.cos(2 * np.pi * b * k / 256))
        f[1::2] = np.rint(32767 * np.sin(2 * np.pi * b * k / 256))
        F.append(f)
    for m in (8191, 8192, 16383, 16384, 32767, -32768):	# the guard thresholds
        f = g.integers(-(abs(m) // 4), abs(m) // 4 + 1, 512)
        f[g.integers(0, 512)] = m
        F.append(f)
    # lower levels of the same shapes: guard counts between none and the most
    f = np.zeros(512, np.int64)
    f[3] = 12000
    F.append(f)
    for m in (3, 40, 500, 4000, 8191, 8192, 16383, 16384):
        F.append(np.full(512, m))
    amps = (1, 100, 8191, 16383, 32767)
    for j in range(64 - len(F) + extra_random):
        a = amps[j % len(amps)]
        F.append(g.integers(-a, a + 1, 512))
    return np.clip(np.array(F), MIN16, MAX16).astype(np.int16)


PITCHES = [2560, 2561, 3071, 3072, 4095, 4096, 4607, 4608, 5119, 5120, 5121, 7000, 12800, 20479, 20480]


@functools.lru_cache(maxsize=None)
def vector_cases(name):
    """(rows n x DE_IN int16, args n x DE_ARGS int32)"""
    mode = VMODES[name]
    g = np.random.default_rng(20261019 + 100 * mode)
    n = N
    b = np.zeros((n, DE_IN), np.int16)
    a = np.zeros((n, DE_ARGS), np.int32)
    i = np.arange(n)
    W = DE_IN - DE_DATA
    if name in ("L_v_inner", "L_v_magsq"):
        b[:, DE_DATA:] = signal(g, n, W)
        late = i % 8 == 6	# small terms, then full scale at the end: saturates late
        b[late, DE_DATA:] >>= 9
        ln = np.where(i < 402, i % 201, g.integers(0, 201, n))
        for r in np.nonzero(late)[0]:
            for o in (DE_DATA + (r & 1), DE_DATA + 512 + ((r >> 1) & 1)):
                b[r, o + max(ln[r] - 6, 0):o + ln[r]] = MAX16
        a[:, 0] = DE_DATA + (i & 1)
        a[:, 1] = DE_DATA + 512 + ((i >> 1) & 1)
        a[:, 2] = ln
        a[:, 3] = np.array([0, 1, 7, 15])[g.integers(0, 4, n)]
        a[:, 4] = np.array([0, 1, 7, 15])[g.integers(0, 4, n)]
        a[:, 5] = np.array([0, 1, 15, 16, 30, 31])[g.integers(0, 6, n)]
    elif name == "zerflt_Q":
        orders = np.array([1, 10, 64, 20, 7])[i % 5]
        u = i // 5
        ln = u % 103	# every remainder of the blocks of 4 and 8, and n below one block
        inplace = (u >> 3) & 1
        b[:, DE_DATA:] = signal(g, n, W)
        # Q13-sized coefficients, and every fourth group of lanes at full
        # scale (+-32767: the L_mac / sat_add32 chains saturate sooner)
        cf = signal(np.random.default_rng(5), n, 65).astype(np.int64)
        fs = (u % 4) == 3
        g5 = np.random.default_rng(6)
        pm = np.where(g5.random((n, 65)) < 0.5, -MAX16, MAX16)
        hit = g5.random((n, 65)) < 0.25
        hit[:, 0] = True
        cf = np.where(fs[:, None], np.where(hit, pm, np.maximum(cf, -MAX16)), cf >> 2)
        disp = table("disp_cof")
        for r in range(n):
            if orders[r] == 64 and r % 2 == 0:
                cf[r] = disp
            if r % 3 == 1:	# a MIN16 coefficient: at order 64 the lane leaves zerflt_q_blk8
                cf[r, g.integers(0, orders[r] + 1)] = MIN16
        b[:, :65] = cf
        a[:, 0] = DE_DATA + 64 + (i & 1)
        a[:, 1] = np.where(inplace, a[:, 0], 640 + ((i >> 1) & 1))
        a[:, 2] = orders
        a[:, 3] = ln
        a[:, 4] = np.array([12, 15, 12, 15, 14, 13, 11])[i % 7]
    elif name in ("iir_2nd_s", "iir_2nd_d", "iir3_s", "iir3_s_io", "iir3_d", "iir3_d_batched", "iir2_d"):
        b[:, DE_DATA:] = signal(g, n, W)
        lpf, dc = (table("lpf_den"), table("lpf_num")), (table("dc_den"), table("dc_num"))
        bpf = [(table("bpf_den")[9 * k:9 * k + 9], table("bpf_num")[9 * k:9 * k + 9]) for k in range(5)]
        one = lambda t: [(t[0][3 * k:3 * k + 3], t[1][3 * k:3 * k + 3]) for k in range(3)]
        ln = np.where(i % 3 == 0, 100 + i % 97, i % 97)
        ln[:4] = (180, PITCH_FR, 0, 1)
        a[:, 0] = DE_DATA + 16 + (i & 1)
        rel = (i >> 1) % 3		# in place, disjoint, out below in
        a[:, 1] = np.where(rel == 0, a[:, 0], np.where(rel == 1, 640 + ((i >> 3) & 1), a[:, 0] - 1 - (i >> 3) % 5))
        if name in ("iir_2nd_s", "iir_2nd_d"):
            den, num = biquads(g, n, 1, one(lpf) + one(dc) + [(table("hpf60_den"), table("hpf60_num")),
                                                              (table("lpf3500_den"), table("lpf3500_num"))])
            b[:, 0:3], b[:, 3:6] = den, num
            b[:, 6:10] = memories(g, n, 4)
            if name == "iir_2nd_d":
                b[:, 10:12] = memories(g, n, 2, 0, 0x3fff)
        elif name == "iir2_d":
            den, num = biquads(g, n, 2, [(np.concatenate([table("lpf3500_den"), table("hpf60_den")]),
                                          np.concatenate([table("lpf3500_num"), table("hpf60_num")]))])
            for s in range(2):
                b[:, 12 * s:12 * s + 3], b[:, 12 * s + 3:12 * s + 6] = den[:, 3 * s:3 * s + 3], num[:, 3 * s:3 * s + 3]
                b[:, 12 * s + 6:12 * s + 10] = memories(g, n, 4)
                b[:, 12 * s + 10:12 * s + 12] = memories(g, n, 2, 0, 0x3fff)
            a[:, 1] = a[:, 0]
        else:
            dbl = name in ("iir3_d", "iir3_d_batched")
            den, num = biquads(g, n, 3, [dc] if dbl else [lpf] + bpf)
            b[:, 0:9], b[:, 9:18] = den, num
            b[:, 18:30] = memories(g, n, 12)
            if dbl:
                b[:, 30:36] = memories(g, n, 6, 0, 0x3fff)
            if name == "iir3_s":
                a[:, 1] = a[:, 0]
                # snap 0, or a multiple of 4 below n
                a[:, 3] = np.where((i % 2 == 1) & (ln > 4), 4 * (g.integers(0, 1 << 20, n) % np.maximum((ln - 1) // 4, 1) + 1), 0)
                a[:, 3] = np.where(a[:, 3] < ln, a[:, 3], 0)
            if name == "iir3_s_io":	# in, out and the record of f's calls apart
                a[:, 1] = np.where(rel == 1, 480 + ((i >> 3) & 1), a[:, 1])
                a[:, 3] = 820
            if name == "iir3_d_batched":
                ln = 36 * (i % 6)	# multiples of 36, from 0 to the codec's 180
                a[:, 0] = DE_DATA + 16 + 2 * (i & 1)
                a[:, 1] = np.where(rel == 0, a[:, 0], np.where(rel == 1, 640 + ((i >> 3) & 1), a[:, 0] - 1 - (i >> 3) % 5))
        a[:, 2] = ln
    elif name in ("envelope", "envelope_e"):
        ln = np.where(i % 3 == 0, 100 + i % 97, i % 97)
        ln[:4] = (PITCH_FR, 180, 0, 1)
        b[:, DE_DATA:] = signal(g, n, W)
        a[:, 0] = DE_DATA + 16 + (i & 1)
        rel = (i >> 1) % 3
        a[:, 1] = np.where(rel == 0, a[:, 0], np.where(rel == 1, 640 + ((i >> 3) & 1), a[:, 0] - 1 - (i >> 3) % 5))
        a[:, 2] = ln
        a[:, 3] = memories(g, n, 1)[:, 0]
        if name == "envelope_e":
            # lsh > 0 inside the precondition envelope_e's comment states:
            # no input sample overflows when scaled up by 2^lsh
            lsh = np.where(i % 2 == 0, 0, 1 + (i >> 1) % 4)
            b[:, DE_DATA:] = b[:, DE_DATA:] >> lsh[:, None]
            m = b[:, DE_DATA:].astype(np.int64) << lsh[:, None]
            assert m.min() >= MIN16 and m.max() <= MAX16
            a[:, 4] = lsh
    elif name == "lpc_syn":
        order = np.where(i % 4 == 3, 8, 10)
        u = i // 4
        ln = np.where(u % 2 == 0, u % 40, 16 + u % 61)	# below 16; from 16 up, every remainder of 8
        rel = (i // 2 + i // 8) % 4	# x == y, y below x, y inside (x, x + n), disjoint
        rel = np.where((rel == 2) & (ln < 2), 0, rel)
        b[:, DE_DATA:] = signal(g, n, W)
        cf = signal(np.random.default_rng(9), n, 16).astype(np.int64)
        cf >>= np.array([5, 4, 3, 0])[(i // 8) % 4][:, None]
        # the lower waves hold no MIN16 coefficient (full scale there is
        # +-32767), so every lane's wave_all(dbl) is true and the order-10
        # fast path runs on the device; the upper waves mix lanes with and
        # without one, which moves the whole wave to the other path
        mixed = i >= n // 2
        cf[~mixed] = np.maximum(cf[~mixed], -MAX16)
        for r in np.nonzero(mixed & (i % 5 == 2))[0]:
            cf[r, g.integers(0, order[r])] = MIN16
        b[:, :16] = cf
        x0 = DE_DATA + 32 + (i & 1)
        d = 1 + g.integers(0, 1 << 20, n) % np.maximum(ln - 1, 1)
        a[:, 0] = np.where(rel == 1, x0 + 1 + (i >> 3) % 20, x0)
        a[:, 1] = np.where(rel == 2, x0 + d, np.where(rel == 3, 640 + ((i >> 1) & 1), x0))
        a[:, 2] = order
        a[:, 3] = ln
    elif name in ("cfft", "fft_npp", "rfft", "rfft_pk"):
        F = fft_frames(192)
        n = len(F)
        b, a = np.zeros((n, DE_IN), np.int16), np.zeros((n, DE_ARGS), np.int32)
        b[:, DE_DATA:DE_DATA + 512] = F
        a[:, 0] = np.where(np.arange(n) % 2 == 0, 1, -1)	# fft_npp's direction
    elif name == "find_harm":
        F = fft_frames(0)
        n = 5 * len(F)
        b, a = np.zeros((n, DE_IN), np.int16), np.zeros((n, DE_ARGS), np.int32)
        i = np.arange(n)
        a[:, 1] = np.array([LPC_FRAME, 512, 1, 2, 199])[i // len(F)]
        a[:, 0] = DE_DATA + (i & 1)
        a[:, 2] = np.array(PITCHES)[(i + i // len(F)) % len(PITCHES)]
        for r in range(n):
            b[r, a[r, 0]:a[r, 0] + a[r, 1]] = F[r % len(F)][:a[r, 1]]
    elif name == "lpc_acor":
        win = table("win_cof")
        amp = np.array([0, 1, 3, 10, 40, 200, 1000, 5000, 20000, 32768])[i % 10]
        v = np.clip(np.rint((g.random((n, 200)) * 2 - 1) * amp[:, None]), MIN16, MAX16)
        # coloured frames (a one-pole smoother) on half the lanes: spectra
        # with structure, so that the Schur recursion runs to the end
        sm = v.copy()
        for k in range(1, 200):
            sm[:, k] = 0.9 * sm[:, k - 1] + v[:, k] * 0.4
        v = np.where((i % 2 == 0)[:, None], np.clip(np.rint(sm), MIN16, MAX16), v)
        v[i % 16 == 15] = MAX16
        a[:, 0] = DE_DATA + (i & 1)
        a[:, 1] = 400 + ((i >> 1) & 1)
        a[:, 2] = np.where(i % 3 == 0, 10, 16)
        a[:, 3] = np.where(i % 7 == 6, 1 + i % 199, 200)
        a[:, 4] = np.array([4, 4, 3, 5])[i % 4]
        for r in range(n):
            b[r, a[r, 0]:a[r, 0] + 200] = v[r]
            b[r, a[r, 1]:a[r, 1] + 200] = win
    elif name == "lpc_schr":
        # autocorrelations the reference's lpc_acor produced, and copies with
        # the later lags perturbed (the L_temp > y2[i] break at various i);
        # r[0] > 0 and |r[1]| <= r[0] throughout
        r = vector_want("lpc_acor")[:, DE_RET:DE_RET + 11].astype(np.int64)
        first = np.clip(2 + (i % 9), 2, 10)
        noise = g.integers(-1, 2, (n, 11)) * (2 ** (i % 14))[:, None] * g.integers(1, 4, (n, 11))
        noise[np.arange(11)[None, :] < first[:, None]] = 0
        r = np.where((i % 2 == 1)[:, None], np.clip(r + noise, MIN16, MAX16), r)
        assert (r[:, 0] > 0).all() and (np.abs(r[:, 1]) <= r[:, 0]).all()
        b[:, :11] = r
    elif name == "lpc_pred2lsp":
        schr = vector_want("lpc_schr")[:, DE_RET + 16:DE_RET + 26].astype(np.int64)
        gam = np.cumprod(np.full(10, 0.994))
        kind = i % 4
        amp = np.array([500, 2000, 8000, 32767])[(i // 4) % 4]
        rnd = np.clip(np.rint((g.random((n, 10)) * 2 - 1) * amp[:, None]), MIN16, MAX16)
        p = np.where((kind == 0)[:, None], schr, np.where((kind == 1)[:, None], np.rint(schr * gam), rnd))
        p[(p == 0).all(axis=1), 0] = 1	# the reference divides by zero on the all-zero polynomial
        b[:, :10] = p
    elif name in ("lpc_lsp2pred", "lsp2pred10", "lpc_clmp"):
        base = np.sort(g.integers(1, 32767, (n, 10)), axis=1)
        kind = i % 8
        for r in range(n):
            k = kind[r]
            if k == 1:	# unsorted
                base[r] = g.permutation(base[r])
            elif k == 2:	# reversed: the bubble sort's worst case
                base[r] = base[r][::-1]
            elif k == 3:	# ties
                base[r, g.integers(0, 10, 4)] = base[r, g.integers(0, 10)]
            elif k == 4:	# out of range
                base[r, g.integers(0, 10, 3)] = g.choice([MIN16, -1, 0, MAX16, -20000])
            elif k == 5:	# one pair closer than delta
                j = g.integers(0, 9)
                base[r, j + 1] = base[r, j] + g.integers(0, 400)
            elif k == 6:	# a cluster: several separation passes
                j = g.integers(0, 6)
                base[r, j:j + 4] = base[r, j] + np.sort(g.integers(0, 300, 4))
            elif k == 7:	# crowded at either end
                base[r] = np.sort(g.integers(0, 1500, 10)) + (31000 if r % 16 == 7 else 0)
        b[:, :10] = np.clip(base, MIN16, MAX16)
        a[:, 0] = np.array([409, 0, 408, 410])[(i // 8) % 4]	# the codec's deltas and neighbours
        a[:, 1] = 10
    elif name == "lpc_pred2refl":
        amp = np.array([300, 1500, 4096, 9000])[i % 4]
        p = np.rint((g.random((n, 10)) * 2 - 1) * amp[:, None])
        edge = np.array([4096, -4096, 4095, -4095, 4097, -4097, 5000, -5000, MAX16, MIN16])
        for r in range(0, n, 3):
            p[r, g.integers(0, 10, 2)] = edge[g.integers(0, len(edge), 2)]
        b[:, :10] = np.clip(p, MIN16, MAX16)
    else:
        raise KeyError(name)
    return np.ascontiguousarray(b, np.int16), np.ascontiguousarray(a, np.int32)


@functools.lru_cache(maxsize=None)
def vector_want(name):
    b, a = vector_cases(name)
    return ref_run("v", VMODES[name], b, a)


@functools.lru_cache(maxsize=None)
def wave_cases(name):
    F = fft_frames(0)
    n = len(F)
    assert n == 64
    a = np.zeros((n, 4), np.int32)
    if name == "wv_find_harm":
        # the wave form's contract: 256 points, zero past the frame
        F = np.concatenate([F, F])
        F[:n, LPC_FRAME:] = 0
        F[:, 256:] = 0
        a = np.zeros((2 * n, 4), np.int32)
        a[:, 0] = np.array(PITCHES)[np.arange(2 * n) % len(PITCHES)]
    else:
        a[:, 0] = np.where(np.arange(n) % 2 == 0, 1, -1)
    return np.ascontiguousarray(F, np.int16), a


@functools.lru_cache(maxsize=None)
def wave_want(name):
    b, a = wave_cases(name)
    return ref_run("w", WMODES[name], b, a)


def describe_vector(name):
    a = vector_cases(name)[1]
    return lambda i: "args %s" % list(a[i])


# ------------------------------------------------- what the cases must reach

def test_fft_cases_cover_every_guard_count():
    """the reference's cfft returns every guard count from 0 to the largest
    it returns for full-scale input"""
    want = vector_want("cfft")
    F = vector_cases("cfft")[0][:, DE_DATA:DE_DATA + 512].astype(np.int64)
    full = np.abs(F).max(axis=1) >= 32767
    top = int(want[full, 0].max())
    seen = set(int(v) for v in want[:, 0])
    assert set(range(top + 1)) <= seen, "guard counts %s, full scale reaches %d" % (sorted(seen), top)
    ww = wave_want("wv_cfft256")
    assert set(range(int(ww[:, 0].max()) + 1)) <= set(int(v) for v in ww[:, 0])


def test_lpc_syn_cases_hold_clean_and_mixed_waves():
    """lpc_syn's order-10 fast path is taken by a whole wave or not at all
    (wave_all over the lanes with order 10 and n >= 16): from the inputs, some
    64-lane blocks hold no MIN16 coefficient on those lanes -- with lanes
    that may take the path (x == y, y below x, disjoint) and lanes the
    aliasing test sends away (y inside (x, x + n)) -- and some blocks mix
    lanes with and without one"""
    b, a = vector_cases("lpc_syn")
    clean = mixed = 0
    for w in range(0, len(a), 64):
        aa, bb = a[w:w + 64], b[w:w + 64]
        vote = (aa[:, 2] == 10) & (aa[:, 3] >= 16)
        has = (bb[:, :10] == MIN16).any(axis=1)
        inside = (aa[:, 1] > aa[:, 0]) & (aa[:, 1] < aa[:, 0] + aa[:, 3])
        if not has[vote].any():
            assert (vote & ~inside).sum() >= 8 and (vote & inside).sum() >= 2
            # n >= 16 with every remainder of 8 on lanes that take the path
            clean += 1
        elif has[vote].any() and (~has[vote]).any():
            mixed += 1
    assert clean >= 2 and mixed >= 2, (clean, mixed)
    fast = (a[:256, 2] == 10) & (a[:256, 3] >= 16) & ~((a[:256, 1] > a[:256, 0]) & (a[:256, 1] < a[:256, 0] + a[:256, 3]))
    assert set(range(8)) <= set(int(v) % 8 for v in a[:256, 3][fast]), "every remainder of 8 on the fast path"
    assert (np.abs(b[:256, :10].astype(np.int64))[fast] == MAX16).any(), "full-scale coefficients on the fast path"


def test_zerflt_cases_reach_every_form_at_full_scale():
    """from the inputs: each of zerflt_Q's forms gets lanes with full-scale
    coefficients, and order 64 gets them with and without a MIN16 one"""
    b, a = vector_cases("zerflt_Q")
    full = np.array([(np.abs(b[r, :a[r, 2] + 1].astype(np.int64)) >= MAX16).any() for r in range(len(a))])
    has = np.array([(b[r, :a[r, 2] + 1] == MIN16).any() for r in range(len(a))])
    for order in (1, 10, 64, 20, 7):
        sel = (a[:, 2] == order) & full & (a[:, 3] >= 8)
        assert (sel & ~has).sum() >= 4, order
    assert ((a[:, 2] == 64) & has).sum() >= 8 and ((a[:, 2] == 64) & ~has).sum() >= 8


def test_pred2lsp_cases_cover_both_branches():
    """lsp_to_freq: all roots found / default frequencies, each at least 10%
    of the cases (judged from the reference's output)"""
    lsf = vector_want("lpc_pred2lsp")[:, DE_RET + 16:DE_RET + 26]
    default = np.array([3276, 9829, 16382, 22935, 29488])
    dflt = (lsf[:, 0::2] == default).all(axis=1) | (lsf[:, 1::2] == default).all(axis=1)
    share = dflt.mean()
    assert 0.1 <= share <= 0.9, "default-frequency share %.3f" % share


def test_schr_cases_take_the_break_at_various_orders():
    """lpc_schr's early exit at step i zeroes the reflection coefficients from
    i on, which leaves the predictor's terms from i on at zero
    (lpc_refl2pred): the number of trailing zeros in the reference's output
    tells where the break was taken.  At least three different places."""
    lpc = vector_want("lpc_schr")[:, DE_RET + 16:DE_RET + 26]
    nz = (np.cumsum((lpc != 0)[:, ::-1], axis=1) == 0).sum(axis=1)
    places = set(int(v) for v in nz if 0 < v < 10)
    assert len(places) >= 3, sorted(places)
    assert (nz == 0).mean() >= 0.1, "recursions that run to the end"


# ------------------------------------------------------------------ CPU

@functools.lru_cache(maxsize=None)
def emu():
    lib = ctypes.CDLL(EMU)
    assert lib.emu_load_tables(TABLES.encode()) == 0
    return lib


def ptr(x):
    return x.ctypes.data_as(ctypes.c_void_p)


@pytest.mark.parametrize("name", sorted(VMODES, key=VMODES.get))
def test_hostemu_vector(name):
    b, a = vector_cases(name)
    out = np.zeros((len(a), DE_OUT), np.int32)
    assert emu().emu_dsp_eval(VMODES[name], ptr(b), ptr(a), ptr(out), len(a)) == 0
    first_diff("host build, mode %d %s" % (VMODES[name], name), out, vector_want(name), describe_vector(name))


@pytest.mark.parametrize("name", sorted(SMODES, key=SMODES.get))
def test_hostemu_scalar(name):
    args = scalar_cases(name)
    out = np.zeros(len(args), np.int32)
    assert emu().emu_dsp_scalar(SMODES[name], ptr(args), ptr(out), ctypes.c_long(len(args))) == 0
    first_diff("host build, scalar mode %d %s" % (SMODES[name], name), out, scalar_want(name), describe_scalar(name))


# ------------------------------------------------------------------ GPU

def _device():
    import torch
    from pairphone_amd import load_library
    lib = load_library()
    dev = torch.device("cuda", 0)
    return torch, lib, dev, torch.cuda.current_stream(dev).cuda_stream


def _device_vector(names):
    torch, lib, dev, s = _device()
    for name in names:
        b, a = vector_cases(name)
        db, da = torch.from_numpy(b).to(dev), torch.from_numpy(a).to(dev)
        do = torch.zeros((len(a), DE_OUT), dtype=torch.int32, device=dev)
        rc = lib.melpe_dsp_eval_dev(VMODES[name], db.data_ptr(), da.data_ptr(), do.data_ptr(), len(a), s)
        assert rc == 0, lib.melpe_last_error()
        got = do.cpu().numpy()
        print("%s: %d cases" % (name, len(got)))
        first_diff("device, mode %d %s" % (VMODES[name], name), got, vector_want(name), describe_vector(name))


def _device_scalar(names, lds):
    torch, lib, dev, s = _device()
    for name in names:
        args = scalar_cases(name)
        da = torch.from_numpy(args).to(dev)
        do = torch.zeros(len(args), dtype=torch.int32, device=dev)
        rc = lib.melpe_dsp_scalar_dev(SMODES[name], lds, da.data_ptr(), do.data_ptr(), len(args), s)
        assert rc == 0, lib.melpe_last_error()
        got = do.cpu().numpy()
        print("%s, %s tables: %d cases" % (name, "LDS" if lds else "blob", len(got)))
        first_diff("device, %s tables, scalar mode %d %s" % ("LDS" if lds else "blob", SMODES[name], name),
                   got, scalar_want(name), describe_scalar(name))


@pytest.mark.gpu
def test_device_scalar_math():
    _device_scalar(sorted(SMODES, key=SMODES.get), 0)


@pytest.mark.gpu
def test_device_scalar_math_lds_tables():
    """the table-reading functions from the LDS copy mtab_src assembles, as
    the NPP kernels stage it"""
    _device_scalar([n for n in sorted(SMODES, key=SMODES.get) if SMODES[n] <= LDS_LAST], 1)


FILTERS = ["L_v_inner", "L_v_magsq", "zerflt_Q", "iir_2nd_s", "iir_2nd_d", "iir3_s", "iir3_s_io", "iir3_d",
           "iir3_d_batched", "iir2_d", "envelope", "envelope_e", "lpc_syn"]
FFTS = ["cfft", "fft_npp", "rfft", "rfft_pk", "find_harm"]
LPC = ["lpc_acor", "lpc_schr", "lpc_pred2lsp", "lpc_lsp2pred", "lsp2pred10", "lpc_clmp", "lpc_pred2refl"]
assert sorted(FILTERS + FFTS + LPC) == sorted(VMODES)


@pytest.mark.gpu
def test_device_filters_and_vectors():
    _device_vector(FILTERS)


@pytest.mark.gpu
def test_device_lpc_chain():
    _device_vector(LPC)


@pytest.mark.gpu
def test_device_fft_family():
    _device_vector(FFTS)
    torch, lib, dev, s = _device()
    for name in sorted(WMODES, key=WMODES.get):
        b, a = wave_cases(name)
        for lo in range(0, len(a), 64):	# 64 cases per launch
            db, da = torch.from_numpy(b[lo:lo + 64]).to(dev), torch.from_numpy(a[lo:lo + 64]).to(dev)
            do = torch.zeros((len(da), DE_WV_OUT), dtype=torch.int32, device=dev)
            rc = lib.melpe_dsp_wave_dev(WMODES[name], db.data_ptr(), da.data_ptr(), do.data_ptr(), len(da), s)
            assert rc == 0, lib.melpe_last_error()
            first_diff("device, wave mode %d %s, cases from %d" % (WMODES[name], name, lo),
                       do.cpu().numpy(), wave_want(name)[lo:lo + 64])
