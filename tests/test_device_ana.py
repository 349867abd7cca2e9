"""Function-level parity of the encoder's pitch and voicing analysis
(pairphone_amd/csrc/analysis.h) with the reference's own functions, one
function -- or one sequence of calls of a stateful function -- at a time.

Every mode is run through pairphone_amd/csrc/ana_eval.h -- by the host build
(emu_ana_eval: the CPU tests) and on the device (melpe_ana_eval_dev: the GPU
tests) -- on inputs built to reach the arms of the gfx950 forms (the energy
thresholds that choose the exact correlators, the unscaled-window form, every
lag count modulo 8, the peak list's corner cases), and must be bit-equal to
what oracle/_ref/ref_ana (oracle/ref_ana.c: the reference's functions, a
fresh process per case where a function keeps statics) gives for the same
cases.  The mode ids and the case layout are parsed from
csrc/ana_eval_modes.h.  For the device-only forms the expected value is the
sequence of reference calls the form's comment claims to equal.

The reference runs once per mode; CPU and GPU tests share its result.  The
pitch tracker's four scalars (ratio, L_ratio, updateEn, multiCheck) are
scalar modes of the same harness: four int32 arguments, one int32 result.
"""
import ctypes
import functools
import os
import re
import subprocess
import tempfile
import time

import numpy as np
import pytest

from conftest import REF_DIR
import test_device_dsp as dsp
from test_device_dsp import CSRC, TABLES, MIN16, MAX16, first_diff, emu, ptr, _device

REF_ANA = os.path.join(REF_DIR, "ref_ana")
HDR = open(os.path.join(CSRC, "ana_eval_modes.h")).read()


def _num(name):
    return int(re.search(r"#define %s (\d+)" % name, HDR).group(1))


(AE_IN, AE_WIN, AE_ARGS, AE_CALL, AE_KMAX, AE_INFO, AE_MARK, AE_RET, AE_PAD, AE_PW, AE_PC, AE_FORMS, S_PANA, S_PAVG,
 S_BPVC, S_PAUTO, S_CLS, CLS_BACK, CLS_SPAN) = (_num(k) for k in (
     "AE_IN", "AE_WIN", "AE_ARGS", "AE_CALL", "AE_KMAX", "AE_INFO", "AE_MARK", "AE_RET", "AE_PAD", "AE_PW", "AE_PC",
     "AE_FORMS", "AE_STRIDE_PITCH_ANA", "AE_STRIDE_P_AVG", "AE_STRIDE_BPVC", "AE_STRIDE_PAUTO", "AE_STRIDE_CLASSIFY",
     "AE_CLS_BACK", "AE_CLS_SPAN"))
AE_OUT = AE_RET + AE_WIN
MODES = {m.group(2): int(m.group(1)) for m in re.finditer(
    r"\bX\((\d+), (\w+)\)", HDR[HDR.index("#define AE_MODES("):HDR.index("#define AE_MODE_COUNT")])}
assert len(MODES) == _num("AE_MODE_COUNT") and AE_RET >= AE_KMAX * AE_CALL + 2
STATEFUL = {n for n, m in MODES.items() if m >= _num("AE_FIRST_STATEFUL")}
SMODES = {m.group(2): int(m.group(1)) for m in re.finditer(
    r"\bS\((\d+), (\w+)", HDR[HDR.index("#define AE_SCALAR_MODES("):HDR.index("#define AE_SCALAR_COUNT")])}
assert len(SMODES) == _num("AE_SCALAR_COUNT")

LW_MAX = 2**31 - 1
PITCHMIN, PITCHMAX, PMIN_Q7, PMAX_Q7 = 20, 160, 2560, 20480
MINPITCH, MAXPITCH, NODE = 20, 147, 8
FRAME, SUBFRAME = 180, 90
N = 500		# cases per mode at most 512; the last wave partial
BG = 23130	# what the window holds where a case puts nothing: a stray write shows


# ---------------------------------------------------------------- reference

def ref_run(mode, rows, args):
    """oracle/_ref/ref_ana on one mode's cases (rows None: a scalar mode)"""
    assert os.path.exists(REF_ANA), "oracle/_ref/ref_ana missing: run __graft_entry__.build() where the reference is"
    n = len(args)
    with tempfile.TemporaryDirectory() as tmp:
        fi, fo = os.path.join(tmp, "in"), os.path.join(tmp, "out")
        with open(fi, "wb") as f:
            if rows is not None:
                f.write(np.ascontiguousarray(rows, np.int16).tobytes())
            f.write(np.ascontiguousarray(args, np.int32).tobytes())
        kind = "s" if rows is None else "v"
        r = subprocess.run([REF_ANA, kind, str(mode), str(n), fi, fo], capture_output=True, text=True)
        assert r.returncode == 0, "ref_ana %s %d: exit %d %s" % (kind, mode, r.returncode, r.stderr[-300:])
        out = np.fromfile(fo, np.int32)
        return out if rows is None else out.reshape(n, AE_OUT)


def where(name):
    """what output j of a case of this mode is"""
    def f(j):
        if j == AE_INFO:
            return "the exact flag"
        if j == AE_MARK:
            return "refused by ae_args_ok"
        if j >= AE_RET:
            return "window[%d] after the last call" % (j - AE_RET)
        if name in STATEFUL:
            return "call %d, value %d" % (j // AE_CALL, j % AE_CALL)
        return "return value %d" % j
    return f


# ------------------------------------------------------------------ signals

def clip16(v):
    return np.clip(np.rint(v), MIN16, MAX16).astype(np.int64)


def sig(g, kind, amp, period, n):
    """n samples: noise, sine, pulse (a decaying pulse train), square, step
    (+amp, then -amp from the middle), runs (full-scale runs of random
    length), zero, const; period in samples, not necessarily whole"""
    t = np.arange(n)
    ph = g.random() * period
    if kind == "noise":
        v = (g.random(n) * 2 - 1) * amp
    elif kind == "sine":
        v = amp * np.sin(2 * np.pi * (t + ph) / period) + (g.random(n) * 2 - 1) * amp * 0.03
    elif kind == "puresine":
        v = amp * np.sin(2 * np.pi * t / period)
    elif kind == "pulse":
        v = np.zeros(n + 16)
        pos = np.rint(np.arange(ph, n, period)).astype(int)
        v[pos] = amp
        v = np.convolve(v, (-0.75) ** np.arange(10))[:n] + (g.random(n) * 2 - 1) * amp * 0.02
    elif kind == "square":
        v = np.where(np.sin(2 * np.pi * (t + ph) / period) >= 0, amp, -amp)
    elif kind == "step":
        v = np.where(t < n // 2, amp, -amp)
    elif kind == "runs":
        v = np.zeros(n)
        k, s = 0, 1
        while k < n:
            ln = int(g.integers(max(int(period) // 2, 1), int(period) + 2))
            v[k:k + ln] = s * amp
            s, k = -s, k + ln
    elif kind == "zero":
        v = np.zeros(n)
    elif kind == "const":
        v = np.full(n, amp)
    else:
        raise KeyError(kind)
    return clip16(v)


AMPS = [40, 400, 1500, 6000, 32768]	# the first three keep a 321-sample window's energy within 32 bits


def energy(x):
    """sum of L_mult(x, x), as f_pitch_scale adds it up"""
    x = np.asarray(x, np.int64)
    return int(np.minimum(2 * x * x, LW_MAX).sum())


def scale_model(x):
    """f_pitch_scale's shift and output, only to place a case's `extra` next to
    the threshold (what the cases reach is judged from the reference's output)"""
    x = np.asarray(x, np.int64)
    s, sc = energy(x), 0
    corr = s
    if s > LW_MAX:
        sc = 5
        corr = min(int((2 * (x >> 5) ** 2).sum()), LW_MAX)
    norm = 0 if corr == 0 else 31 - int(corr).bit_length()
    sc -= norm >> 1
    y = x >> sc if sc >= 0 else np.clip(x << -sc, MIN16, MAX16)
    return sc, y


# -------------------------------------------------------------------- cases

def _pack(cases, seed):
    """cases: (row int array up to AE_IN, args list, description); shuffled, so
    that neighbouring lanes take different arms"""
    assert 0 < len(cases) <= 512 and len(cases) % 64 != 0, len(cases)
    order = np.random.default_rng(seed).permutation(len(cases))
    rows = np.zeros((len(cases), AE_IN), np.int16)
    args = np.zeros((len(cases), AE_ARGS), np.int32)
    desc = []
    for k, j in enumerate(order):
        r, a, d = cases[j]
        rows[k, :len(r)] = r
        args[k, :len(a)] = a
        desc.append(d)
    return rows, args, desc


def _window_row(parts):
    """a window of background with the given (offset, samples) parts"""
    b = np.full(AE_WIN, BG, np.int64)
    for off, x in parts:
        assert AE_PAD <= off and off + len(x) <= AE_WIN - AE_PAD
        b[off:off + len(x)] = x
    return b


def _cases_f_pitch_scale(g):
    IN, OUT = AE_PAD, 416
    cases = []

    def add(x, ipar, omode, extra, d):
        a0 = IN + ipar
        a1 = a0 if omode == 0 else OUT + (omode - 1)
        cases.append((_window_row([(a0, x)]), [a0, a1, len(x), extra],
                      "%s, len %d, in %d, out %d, extra %d" % (d, len(x), a0, a1, extra)))

    k = 0
    for ln in list(range(1, 41)) + [AE_PW]:	# the in-place form's head, groups of four dwords, remainder, tail
        for ipar in (0, 1):
            for omode in (0, 1, 2):
                amp = [30, 1000, 12000, 32768][k % 4]
                x = sig(g, "runs" if k % 11 == 5 else "noise", amp, 7, ln)
                add(x, ipar, omode, 0, "noise %d" % amp)
                k += 1

    def sparse(vals, ln):
        x = np.zeros(ln, np.int64)
        x[np.sort(g.choice(ln, len(vals), replace=False))] = vals
        return x

    edge = [([16384] * 4, "sum 2^31"), ([32767, 255, 22, 5], "sum 2^31-2"), ([-32768], "one -32768: sum LW_MAX"),
            ([-32768, 1], "-32768 and 1"), ([-32768, -1], "-32768 and -1"), ([], "all zero")]
    for j in range(15):	# both parities of norm_l(corr): energies 2^(2j+1) and 2^(2j+2)
        edge.append(([1 << j], "one 2^%d" % j))
        edge.append(([1 << j, 1 << j], "two 2^%d" % j))
    assert energy([16384] * 4) == 2**31 and energy([32767, 255, 22, 5]) == 2**31 - 2 and energy([-32768]) == LW_MAX
    for j, (vals, d) in enumerate(edge):
        for v in range(4):
            add(sparse(vals, AE_PW if (j + v) % 2 else 9), v & 1, 0 if v < 2 else 1 + (j & 1), 0, d)
    # the scaled output's energy either side of 2^31 - 1, through `extra` (the
    # persistent tail's term in pitch_ana) and without it
    loud_over = loud_under = 0
    for j in range(400):
        amp = [25, 300, 3000, 12000, 32768][j % 5]
        x = sig(g, ["noise", "sine", "runs"][j % 3], amp, 20 + j % 50, AE_PW if j % 4 else 37)
        if j >= 30 and j % 2:
            # positive samples, the energy just above 2^31 * 4^k: the scaling
            # pass's >> 5 loses enough for a shift one too small
            x = np.abs(x) + 40
            x = clip16(x * np.sqrt(2**31 * 4.0 ** (j % 3) * (1 + 0.002 * (j % 7)) / max(energy(x), 1)))
        e2 = int((2 * scale_model(x)[1] ** 2).sum())
        if j < 30:
            if 1 <= e2 <= LW_MAX - 1:
                add(x, j & 1, 0 if j % 3 else 1, LW_MAX - 1 - e2, "output energy + extra = 2^31-2")
                if j % 2:	# an odd extra: the bound met with equality
                    add(x, j & 1, 0 if j % 3 else 2, LW_MAX - e2, "output energy + extra = 2^31-1")
                add(x, j & 1, 0 if j % 3 else 2, LW_MAX + 1 - e2, "output energy + extra = 2^31")
        elif energy(x) > LW_MAX and e2 > LW_MAX and loud_over < 12:
            add(x, j & 1, (j // 2) % 3, 0, "output energy above 2^31-1, no extra")
            loud_over += 1
        elif energy(x) > LW_MAX and e2 <= LW_MAX and loud_under < 12:
            add(x, j & 1, (j // 2) % 3, 0, "loud, output energy within 2^31-1")
            loud_under += 1
    assert loud_over >= 4 and loud_under >= 4
    return cases


def _pit_window(g, kind, amp, period, par):
    a0 = AE_PAD + 2 + par
    # what lies next to the window is not silence: a read outside it shows
    b = _window_row([(AE_PAD, sig(g, "noise", 20000, 1, AE_PW + 8)), (a0, sig(g, kind, amp, period, AE_PW))])
    return a0, b


KINDS = ["sine", "pulse", "noise", "square", "runs"]


def over_window(g, lo, hi, kind, period, k):
    """a pitch window that leaves the exact path by itself: positive samples
    in [lo, hi) only, silence elsewhere, the energy just above 2^31 4^k, where
    the scaling pass's >> 5 loses enough for a shift one too small, so that
    the scaled window's energy still passes 2^31 - 1.  With [lo, hi) one
    correlation segment, that segment's own energy chain (c00 / cTT, msq /
    m2) clamps where the plain sum does not."""
    seg = np.abs(sig(g, kind, 3000, period, hi - lo)) + 40
    for kk in (k, 0):	# a peaky segment clips at the higher levels
        for m in range(1, 200):
            x = np.zeros(AE_PW, np.int64)
            x[lo:hi] = clip16(seg * np.sqrt(2**31 * 4.0 ** kk * (1 + 0.0002 * m) / energy(seg)))
            if energy(x) > LW_MAX and int((2 * scale_model(x)[1] ** 2).sum()) > LW_MAX:
                return x
    raise AssertionError("no window above the bound")


def _pit_row(x, par):
    a0 = AE_PAD + 2 + par
    return a0, _window_row([(AE_PAD, np.full(AE_PW + 8, BG)), (a0, x)])


def _cases_find_pitch(g):
    cases = []

    def add(kind, amp, period, lower, upper, ln, form, d):
        a0, b = _pit_window(g, kind, amp, period, len(cases) & 1)
        cases.append((b, [a0, form, lower, upper, ln],
                      "%s: %s amp %d period %.1f, lags %d..%d len %d, form %d" % (d, kind, amp, period, lower, upper,
                                                                                 ln, form)))

    k = 0
    # every (lower, upper, len) frac_pch passes down from ip, range 5, lmin 160
    for ip in range(PITCHMIN, PITCHMAX + 1):
        lo = max(ip - 5, PITCHMIN, (ip >> 1) + (ip >> 2))
        hi = min(ip + 5, PITCHMAX)
        for f in (ip % 3, (ip + 1) % 3):
            add(KINDS[k % 5], AMPS[(k // 5) % 5], ip + (k % 7 - 3) * 0.4, lo, hi, max(ip, 160), f, "frac_pch's search")
            k += 1
    # lag counts 1..24: the one-pass form, whole blocks of 8, every remainder;
    # both parities of cb0
    for nl in range(1, 25):
        for ln in (160, 159):
            for f in range(AE_FORMS):
                up = 60 + (7 * nl + ln) % 100
                lo = up - nl + 1
                if lo < PITCHMIN:
                    lo, up = PITCHMIN, PITCHMIN + nl - 1
                add(KINDS[k % 5], AMPS[(k // 5) % 5], (lo + up) / 2 + 0.3, lo, up, ln - (up & 1), f, "%d lags" % nl)
                k += 1
    # the best lag is the first of the last, partial block (lag upper - (nl & ~7))
    for nl in range(13, 24):
        if nl % 8:
            for j, up in enumerate((150, 97)):
                add(["puresine", "pulse"][(nl + j) % 2], [1500, 32768][j], up - (nl & ~7), up - nl + 1, up, 160 - j,
                    0, "%d lags, the best one opens the partial block" % nl)
    # windows whose scaled copy's energy passes 2^31 - 1 (the flag comes out
    # false): spread over the window, and confined to the first lag's first or
    # second segment, whose energy chain then clamps and is updated from there
    j = 0
    for lo, up, ln in ((60, 75, 120), (20, 31, 100), (100, 124, 160), (40, 52, 160), (131, 160, 160), (25, 49, 143)):
        cb0 = AE_PC - ((ln + up) >> 1)
        for where_, a, b in (("whole window", 0, AE_PW), ("first segment", cb0, cb0 + ln),
                             ("second segment", cb0 + up, min(cb0 + up + ln, AE_PW))):
            for f in (0, 1) if where_ != "whole window" else (1,):
                x = over_window(g, a, b, ["noise", "sine", "pulse"][j % 3], (lo + up) / 2.0, j % 3)
                a0, row = _pit_row(x, j & 1)
                cases.append((row, [a0, f, lo, up, ln], "scaled energy above 2^31-1, %s: lags %d..%d len %d, form %d" % (
                    where_, lo, up, ln, f)))
                j += 1
    for f in range(AE_FORMS):
        add("zero", 0, 50, 40, 60, 160, f, "all zero: den clamped to 1")
        add("step", 1200, 50, 100, 110, 160, f, "anticorrelated: every corr <= 0")
        add("step", 32768, 50, 90, 120, 160, f, "anticorrelated, full scale")
        add("const", 900, 50, 30, 70, 160, f, "constant")
        add("const", -32768, 50, 30, 70, 150, f, "all -32768")
        add("runs", 32768, 70, 60, 83, 160, f, "full-scale runs near the lag")
        add("square", 32768, 64, 56, 72, 160, f, "full-scale square wave, period in the search")
        add("square", 1700, 23, 20, 31, 97, f, "short length")
    return cases


def _cases_frac_pch(g):
    cases = []

    def add(kind, amp, period, fpitch, rng, lmin, form, d):
        a0, b = _pit_window(g, kind, amp, period, len(cases) & 1)
        cases.append((b, [a0, form, fpitch, rng, lmin],
                      "%s: %s amp %d period %.2f, fpitch %d range %d lmin %d, form %d" % (
                          d, kind, amp, period, fpitch, rng, lmin, form)))

    k = 0
    for ip in range(PITCHMIN, PITCHMAX + 1):
        for rng in (0, 5):
            # the true period up to a sample either side of the estimate: the
            # ip-1 test both ways, fractions of either sign
            per = ip + (k % 9 - 4) * 0.27
            fp = int(np.clip(ip * 128 + int(g.integers(-64, 64)), PMIN_Q7, PMAX_Q7))
            add(KINDS[k % 4], AMPS[(k // 4) % 5], per, fp, rng, 160, (k + rng) % 3, "sweep")
            k += 1
    for j in range(60):	# len not clamped by lmin
        ip = int(g.integers(45, PITCHMAX))
        add(KINDS[j % 4], AMPS[j % 5], ip + 0.3, ip * 128 + 17, 5 if j % 2 else 0, 40, j % 3, "lmin 40")
    # the flag false by itself, as in find_pitch's cases: the first segment is
    # sig[cb .. cb + len), the second sig[cb + ip - 1 .. + len + 2)
    j = 0
    for ip, lmin in ((30, 160), (64, 160), (101, 160), (140, 160), (159, 160), (90, 40), (52, 40)):
        ln = max(ip, lmin)
        cb = AE_PC - ((ln + ip) >> 1)
        for where_, a, b in (("whole window", 0, AE_PW), ("first segment", cb, cb + ln),
                             ("second segment", cb + ip - 1, min(cb + ip + ln + 1, AE_PW))):
            for rng in (0, 5):
                for f in (0, 1) if where_ != "whole window" else (1,):
                    x = over_window(g, a, b, ["noise", "sine", "pulse"][j % 3], float(ip), j % 3)
                    a0, row = _pit_row(x, j & 1)
                    cases.append((row, [a0, f, ip * 128 + 5 * (j % 7), rng, lmin],
                                  "scaled energy above 2^31-1, %s: lag %d range %d lmin %d, form %d" % (
                                      where_, ip, rng, lmin, f)))
                    j += 1
    for j in range(AE_FORMS * 2):
        f, rng = j % 3, 5 * (j // 3)
        add("zero", 0, 50, 6400, rng, 160, f, "all zero: den == 0, root <= 0")
        add("const", 700, 50, 6400, rng, 160, f, "constant")
        add("step", 1500, 50, 13000, rng, 160, f, "anticorrelated: t <= 0")
        add("step", 32768, 50, 15000, rng, 160, f, "anticorrelated, full scale")
        add("puresine", 1800, 19.2, PMIN_Q7, rng, 160, f, "period below PITCHMIN: clamp at pmin_q7")
        add("puresine", 1800, 19.6, PMIN_Q7 + 60, rng, 160, f, "period below PITCHMIN")
        add("puresine", 1800, 161.5, PMAX_Q7, rng, 160, f, "period above PITCHMAX: ip >= pmax, clamp at pmax_q7")
        add("puresine", 30000, 162.5, PMAX_Q7 - 100, rng, 160, f, "period above PITCHMAX, loud")
        add("square", 1000, 40, 5120, rng, 160, f, "exactly periodic: corr >= root")
        add("puresine", 1500, 64, 8192, rng, 160, f, "exactly periodic sine")
        add("square", 32768, 50, 6400, rng, 160, f, "full-scale square wave")
        add("pulse", 1500, 80, 5120, rng, 160, f, "estimate at half the period")
        add("noise", 1000, 1, 9000, rng, 160, f, "noise")
    return cases


def _cases_gain_ana(g):
    cases = []
    C = 416
    for k in range(N):
        pitch = [PMIN_Q7, PMAX_Q7, 15257, 15258, 2561, 7680, 7679][k % 16] if k % 16 < 7 else int(
            g.integers(PMIN_Q7, PMAX_Q7 + 1))
        minlen, maxlen = [(120, 320), (0, 320), (120, 150), (90, 100), (1, 320), (200, 210)][k % 6]
        amp = [0, 3, 30, 300, 3000, 12000, 32768][(k // 6) % 7]
        kind = "zero" if amp == 0 else ["noise", "sine", "runs"][(k // 42) % 3]
        a0 = C + (k & 1)
        b = _window_row([(AE_PAD, sig(g, "noise", 9000, 1, AE_WIN - 2 * AE_PAD)),
                         (a0 - 190, sig(g, kind, amp, 37, 380))])
        cases.append((b, [a0, pitch, minlen, maxlen],
                      "%s amp %d, pitch %d minlen %d maxlen %d, at %d" % (kind, amp, pitch, minlen, maxlen, a0)))
    return cases


def _track(g, full):
    """a PitTrack as corPeak leaves it: lags ascending, padded with (100, 0)"""
    n = NODE if full else int(g.integers(0, NODE))
    pit = np.sort(g.choice(np.arange(MINPITCH, MAXPITCH + 1), n, replace=False))
    w = g.integers(0, 32768, n)
    if n and g.random() < 0.3:
        w[g.integers(0, n, 3)] = w[0]	# equal weights: the strict '>' picks the first
    return np.concatenate([pit, np.full(NODE - n, 100), w, np.zeros(NODE - n, np.int64), g.integers(-9, 9, NODE)])


def _cases_trackers(g, look):
    cases = []
    for k in range(N):
        num = k % 9 if look else 0
        tr = np.concatenate([_track(g, k % 3 == 0) for _ in range(num + 1)])
        a0 = AE_PAD + (k & 1)
        if look:
            a1 = num
        else:
            # near a listed lag (inside ratio < 0.2), near its edge, or far from all
            p = int(tr[g.integers(0, NODE)]) * 128
            a1 = int(np.clip([p, p + p // 5 - 2, p + p // 5 + 40, p - p // 6, 32000, 1300][k % 6], 1, 32767))
        cases.append((_window_row([(a0, tr)]), [a0, a1], "%d tracks, second argument %d" % (num + 1, a1)))
    return cases


def _cases_pitch_ana(g):
    K = 4
    L = AE_PW + (K - 1) * FRAME
    cases = []
    for k in range(N):
        kind = k % 10
        P = float(g.integers(PITCHMIN, PITCHMAX + 1)) + [0, 0.3, 0.5, 0.8][k % 4]
        noise = float(0.4 + g.random() * 2.0) if k % 4 else 0.0	# spreads pcorr across 9831 and 9012
        amp = AMPS[(k // 70) % 5]
        d = "period %.1f, noise %.2f, amp %d" % (P, noise, amp)
        mult = 1.0
        if kind == 0:
            res = sig(g, "pulse", amp, P, L) + sig(g, "noise", amp * noise * 0.3, 1, L)
            sp = sig(g, "sine", amp, P, L)
            d = "periodic residual, " + d
        elif kind == 1:
            res = sig(g, "noise", amp, 1, L)
            sp = sig(g, "pulse", amp, P, L) + sig(g, "noise", amp * noise * 0.3, 1, L)
            d = "noise residual, periodic speech, " + d
        elif kind == 2:
            res, sp = sig(g, "noise", amp, 1, L), sig(g, "noise", amp, 1, L)
            d = "noise both: the average pitch, " + d
        elif kind in (3, 4):
            m = [2, 3, 4, 5, 6, 7, 8][(k // 10) % 7]
            P = float(g.integers(PITCHMIN, PITCHMAX // m + 1))
            mult = m
            res = sig(g, "pulse", amp, P, L) + sig(g, "noise", amp * 0.05, 1, L)
            sp = sig(g, "noise", amp, 1, L) if kind == 3 else sig(g, "pulse", amp, P, L)
            if kind == 4:
                res = sig(g, "noise", amp, 1, L)
            d = "estimate at %d times the period %.0f, %s, amp %d" % (m, P, "residual" if kind == 3 else "speech", amp)
        elif kind == 5:
            P = float(g.integers(PITCHMIN, 30))	# below 3840 in Q7: double_ver checks a multiple
            res = sig(g, "pulse", amp, P, L) + sig(g, "noise", amp * noise * 0.2, 1, L)
            sp = sig(g, "pulse", amp, P, L)
            d = "short period %.0f (double_ver m > 1), noise %.2f, amp %d" % (P, noise, amp)
        elif kind in (6, 7, 8):
            # a loud speech frame falls back to the speech window and leaves its
            # last samples, unscaled, behind the window of the calls that follow
            # (the tail term of the exactness bound); voiced frames follow,
            # quiet, or with loud speech that renews the tail when it is used
            long_lag = (k // 10) % 2 == 1
            if long_lag:	# the second segment runs into the tail
                P = float(g.integers(154, PITCHMAX + 1))
                if k % 4 != 1:	# a clean residual: the first pass holds, double_chk reads the stale tail
                    noise *= 0.1
            ra = [900, 900, 6000][kind - 6]
            res = sig(g, "pulse", ra, P, L) + sig(g, "noise", ra * noise * 0.3, 1, L)
            # (a long lag's loud speech is a square wave: tail samples of one
            # sign.  With loud ones of alternating sign the correlations
            # saturate at -32768 next to 32767, frac_pch's denominator comes
            # out negative, and the reference's L_sqrt_fxp reads in front of
            # its logarithm table: what it returns there is no property of the
            # codec)
            sp = sig(g, "square" if long_lag else ["sine", "square", "pulse"][kind - 6],
                     [900, 32768, 32768][kind - 6], P, L)
            c = 0 if k % 20 < 10 else 1
            res[c * FRAME:c * FRAME + AE_PW] = sig(g, "noise", 3000, 1, AE_PW)
            sp[c * FRAME:c * FRAME + AE_PW] = sig(g, "square" if long_lag else ["noise", "pulse", "square"][(k // 20) % 3], 32768,
                                                   P, AE_PW)
            d = "loud speech tail left by call %d, then period %.1f, noise %.2f" % (c, P, noise)
        else:
            res, sp = sig(g, "zero", 0, 1, L), sig(g, "zero" if k % 20 < 10 else "noise", 50, 1, L)
            d = "zero residual"
        row = np.zeros(AE_IN, np.int64)
        for c in range(K):
            o = c * S_PANA
            row[o:o + AE_PW] = clip16(sp[c * FRAME:c * FRAME + AE_PW])
            row[o + AE_PW:o + 2 * AE_PW] = clip16(res[c * FRAME:c * FRAME + AE_PW])
            pest = P * mult * 128 + (int(g.integers(-300, 300)) if c % 2 else 0)
            row[o + 2 * AE_PW] = int(np.clip(pest, PMIN_Q7, PMAX_Q7))
            row[o + 2 * AE_PW + 1] = 1000 + 10 * c + k % 50	# the average: a value no search returns
        cases.append((row, [K], d))
    return cases


def _cases_p_avg_update(g):
    cases = []
    for k in range(N):
        row = np.zeros(AE_IN, np.int64)
        th = [13107, 0, 9830][k % 3]
        for c in range(AE_KMAX):
            o = c * S_PAVG
            row[o] = int(g.integers(PMIN_Q7, PMAX_Q7 + 1)) if k % 7 else [MIN16, MAX16, 0][c % 3]
            row[o + 1] = th + [-1, 0, 1, 5000, -5000][int(g.integers(0, 5))]
            row[o + 2] = th
        cases.append((row, [AE_KMAX], "threshold %d" % th))
    return cases


def _band0(x):
    """the reference's three band-0 sections (iir_2nd_s, through ref_dsp's
    iir3_s mode) over each row of x from zero memories, 720 samples a run
    with the memories carried: what bpvc_ana's lowest band makes of these
    frames"""
    n, ln = x.shape
    mem = np.zeros((n, 12), np.int16)
    outs = []
    for lo in range(0, ln, 720):
        part = x[:, lo:lo + 720]
        b = np.zeros((n, dsp.DE_IN), np.int16)
        a = np.zeros((n, dsp.DE_ARGS), np.int32)
        b[:, 0:9], b[:, 9:18], b[:, 18:30] = dsp.table("bpf_den")[:9], dsp.table("bpf_num")[:9], mem
        b[:, 144:144 + part.shape[1]] = part
        a[:, 0], a[:, 2] = 144, part.shape[1]
        out = dsp.ref_run("v", dsp.VMODES["iir3_s"], b, a)
        mem = out[:, dsp.DE_RET + 18:dsp.DE_RET + 30].astype(np.int16)
        outs.append(out[:, dsp.DE_RET + 144:dsp.DE_RET + 144 + part.shape[1]].astype(np.int64))
    return np.concatenate(outs, axis=1)


def _sequential_band0(g, K, count):
    """inputs on which band 0 of bpvc_ana leaves the exact path from the
    second call on.  The window's energy must pass 2^31 - 1 and that of its
    scaled copy too, i.e. f_pitch_scale's shift, found on the samples >> 5,
    must come out one too small: the truncation has to lose energy, which it
    does on positive samples and not on negative ones.  Band 0 passes a
    constant, so an offset tuned to the band's gain does it; what is added
    above 1 kHz (voiced, noisy, at any level up to the offset's) goes to the
    other bands."""
    L = K * FRAME
    v = _band0(np.full((1, 720), 2000, np.int64))[0, -1]
    gain = v / 2000.0
    xs = []
    for j in range(5 * count):
        target = (1833 + j % 20) * 2 ** (j % 4)	# 2 v^2 321 just above 2^31 4^k
        P = float(g.integers(PITCHMIN, PITCHMAX + 1))
        top = sig(g, ["pulse", "noise", "square", "pulse"][j % 4], [60, 400, 1500, 4000][(j // 4) % 4], P, L)
        spec = np.fft.rfft(top.astype(np.float64))
        spec[:L // 8 + 1] = 0	# nothing below 1 kHz
        xs.append(clip16(target / gain + np.fft.irfft(spec, L) + (g.random(L) * 2 - 1) * 2))
    xs = np.array(xs)
    y = np.concatenate([np.zeros((len(xs), AE_PW - FRAME), np.int64), _band0(xs)], axis=1)
    good = []
    for j in range(len(xs)):
        hit = 0
        for c in range(1, K):
            w = y[j, c * FRAME:c * FRAME + AE_PW]
            hit += energy(w) > LW_MAX and int((2 * scale_model(w)[1] ** 2).sum()) > LW_MAX
        if hit == K - 1:
            good.append(xs[j])
    assert len(good) >= count, "%d of %d tuned inputs leave the exact path" % (len(good), len(xs))
    return good[:count]


def _cases_bpvc_ana(g):
    K = 4
    L = K * FRAME
    cases = []
    # more than half of the cases, and twice the calls: band 0 makes two of a
    # call's ten frac_pch calls, and the sequential path is to take an eighth
    KT = 2 * K
    tuned = _sequential_band0(g, KT, 300)
    for k in range(N):
        P = float(g.integers(PITCHMIN, PITCHMAX + 1)) + [0, 0.4][k % 2]
        kind = ["pulse", "noise", "sine", "square", "pulse", "zero", "pulse"][k % 7]
        # per frame: quiet (every band's window energy within 32 bits),
        # moderate, loud (above), in every order
        lv = [(300,) * 4, (30000,) * 4, (2500,) * 4, (40, 40, 32768, 32768), (32768, 32768, 40, 40),
              (9000, 200, 9000, 200), (5, 700, 32768, 60), (1200, 1500, 1800, 2200)][(k // 7) % 8]
        x = np.concatenate([sig(g, kind, lv[c], P, FRAME) for c in range(K)])
        if kind == "pulse" and k % 14 < 7:	# one phase across the frames
            x = clip16(sig(g, "pulse", 1000, P, L) * (np.repeat(lv, FRAME) / 1000.0))
        kk = K
        if k % 5 >= 2:
            x, kind, lv, kk = tuned[(k // 5) * 3 + k % 5 - 2], "offset tuned to band 0's gain", "sequential from call 1", KT
        row = np.zeros(AE_IN, np.int64)
        for c in range(kk):
            o = c * S_BPVC
            row[o:o + FRAME] = x[c * FRAME:c * FRAME + FRAME]
            good = int(np.clip(P * 128, PMIN_Q7, PMAX_Q7))
            bad = int(g.integers(PMIN_Q7, PMAX_Q7 + 1))
            row[o + FRAME:o + FRAME + 2] = (good, bad) if (k + c) % 2 else (bad, good)
        cases.append((row, [kk], "%s period %.1f, frame levels %s" % (kind, P, lv)))
    return cases


HALF_SINES = [(192, 80), (192, 170), (192, 260), (191, 80), (193, 80), (192, 79), (192, 81), (191, 170), (193, 170),
              (192, 169), (192, 171), (190, 80), (194, 80), (192, 259), (192, 261)]


def _cases_pitchAuto(g):
    K = 6
    L = K * SUBFRAME
    cases = []
    for k in range(N):
        kind = k % 12
        amp = [200, 3000, 32768][(k // 12) % 3]
        P = [MAXPITCH, MINPITCH, 30, 21, 146, 49, 73.5][(k // 36) % 7] if kind < 4 else float(
            g.integers(MINPITCH - 2, MAXPITCH + 6))
        if kind == 0:
            x, d = sig(g, "pulse", amp, P, L), "pulse train"
        elif kind == 1:
            x, d = sig(g, "puresine", amp, P, L), "pure sine"
        elif kind == 2:
            x, d = sig(g, "square", amp, P, L), "square wave"
        elif kind == 3:
            x, d = sig(g, "sine", amp, P, L), "sine"
        elif kind == 4:
            x, d = sig(g, "noise", amp, 1, L), "noise"
        elif kind == 5:
            x, d = sig(g, "zero", 0, 1, L), "all zero: rc[0] == 0, no peak"
        elif kind == 6 and k // 12 < len(HALF_SINES):
            # ivfilt's t1 > t2: the second reflection coefficient at -1 and the
            # roundings against it.  Found by a search over widths and starts.
            W, s0 = HALF_SINES[k // 12]
            t = np.arange(L)
            x = clip16(np.where((t >= s0) & (t <= s0 + W), 32000 * np.sin(np.pi * (t - s0) / W), 0))
            d, P, amp = "half sine of %d samples from %d" % (W, s0), 2 * W, 32000
        elif kind == 6 and k % 24 < 12:
            x, d = sig(g, "const", amp, 1, L), "constant"
        elif kind == 6:
            # far below the band edge: the second reflection coefficient at -1,
            # where rounding decides ivfilt's t1 > t2
            P = [200, 333, 500, 800, 1300, 2100][(k // 24) % 6]
            x, d = sig(g, "puresine", amp, P, L), "slow pure sine"
            if (k // 24) % 2:	# one smooth bump in silence
                c0, w = float(g.integers(60, L - 60)), [15, 25, 40, 70, 110][(k // 48) % 5]
                x, d = clip16(amp * np.exp(-(np.arange(L) - c0) ** 2 / (2.0 * w * w))), "smooth bump of width %d" % w
        elif kind == 7:
            x, d = sig(g, "runs", 32768, P, L), "full-scale runs"
        elif kind == 8:
            # low-passed noise: a few broad peaks
            x = clip16(np.convolve((g.random(L + 40) * 2 - 1) * amp, np.ones(int(g.integers(6, 40))) / 6)[:L])
            d = "smoothed noise"
        elif kind == 9:
            x = sig(g, "pulse", amp, P, L)
            x[:int(g.integers(1, 5)) * SUBFRAME] = 0
            d = "onset of a pulse train"
        elif kind == 10:
            x = sig(g, "pulse", amp, P, L) + sig(g, "pulse", amp * 0.6, P * 1.5, L)
            d = "two pulse trains, periods 2:3"
        else:
            x = sig(g, "puresine", amp, P, L)
            x[int(g.integers(0, L))] = 32767	# one spike on a sine
            d = "sine with a spike"
        row = np.zeros(AE_IN, np.int64)
        for c in range(K):
            row[c * S_PAUTO:c * S_PAUTO + SUBFRAME] = clip16(x[c * SUBFRAME:(c + 1) * SUBFRAME])
        cases.append((row, [K], "%s, period %.1f, amp %d" % (d, P, amp)))
    return cases


def _cases_classify(g):
    K = 4
    L = CLS_SPAN + (K - 1) * SUBFRAME
    TH = np.array([9830, 13107, 14746, 16384, 18022, 19661, 21299, 22938, 26214])
    cases = []
    for k in range(N):
        kind = k % 8
        P = float([MINPITCH, 21, 24, 25, MAXPITCH, 146, 143, 142][(k // 8) % 8]) if k % 3 == 0 else float(
            g.integers(MINPITCH, MAXPITCH + 1))
        amp = [15, 150, 1200, 4884 * 1.2, 32768][(k // 8) % 5]
        if kind == 0:
            x, d = sig(g, "pulse", amp, P, L), "voiced pulse train"
        elif kind == 1:
            x, d = sig(g, "noise", amp, 1, L), "noise"
            if k % 4 == 1:	# some samples four times the rest: a sweep of peakiness
                x = clip16(sig(g, "noise", min(amp, 8000), 1, L) * (1 + 3 * (g.random(L) < (k % 37) / 150.0)))
                d = "noise with louder samples"
        elif kind == 2:
            x, d = sig(g, "sine", amp, P, L), "low sine"
        elif kind == 3:
            x = sig(g, "noise", 20, 1, L)
            o = int(g.integers(CLS_BACK, L - 60))
            x[o:] = sig(g, ["pulse", "noise"][k % 2], amp, P, L - o)
            d = "onset"
        elif kind == 4:
            x = sig(g, "noise", 10, 1, L)
            x[g.integers(0, L, 3)] = amp	# peaky
            d = "isolated peaks"
        elif kind == 5:
            x, d = sig(g, "zero", 0, 1, L), "all zero"
        elif kind == 6:
            x = clip16(np.convolve((g.random(L + 20) * 2 - 1) * amp, np.ones(12) / 4)[:L])
            d = "smoothed noise"
        else:
            x, d = sig(g, "square", amp, 2.0 + (k % 5), L), "high-frequency square wave"
        row = np.zeros(AE_IN, np.int64)
        for c in range(K):
            o = c * S_CLS
            span = x[c * SUBFRAME:c * SUBFRAME + CLS_SPAN]
            row[o:o + CLS_SPAN] = clip16(span)
            f = span[CLS_BACK:CLS_BACK + SUBFRAME + 40].astype(np.float64)
            r = np.array([np.dot(f[:len(f) - j], f[j:]) for j in range(17)])
            ac = clip16(32767 * r / r[0]) if r[0] > 0 else np.zeros(17, np.int64)
            if k % 16 >= 12:	# autocorrelations unrelated to the signal: bandEn's range
                ac = np.concatenate([[32767], g.integers(-32768, 32768, 16)])
            row[o + CLS_SPAN:o + CLS_SPAN + 17] = ac
            near = int(TH[g.integers(0, len(TH))]) + int(g.integers(-1, 2))
            ven = int(g.integers(6144, 22000))
            row[o + CLS_SPAN + 17:o + CLS_SPAN + 23] = [
                # previous zeroCrosRate, subEnergy: anywhere, or above this subframe's (no onset seen)
                int(g.integers(0, 32768)) if (k + c) % 2 else 32767, int(g.integers(-20480, 16000)) if (k + c) % 2 else 16000,
                int(np.clip(P + g.integers(-1, 2), MINPITCH, MAXPITCH)) if kind in (0, 2) else int(
                    g.integers(MINPITCH, MAXPITCH + 1)),
                near if c % 2 else int(g.integers(0, 32768)),	# corx
                ven, int(g.integers(ven - 8000, ven + 1000))]	# silenceEn either side of voicedEn - 3072
        cases.append((row, [K], "%s, period %.0f, amp %d" % (d, P, amp)))
    # A second pass for two arms that need the energy thresholds next to the
    # subframe's own energy.  The reference reports subEnergy, zeroCrosRate and
    # peakiness, none of which depends on the thresholds: where a later call's
    # values fit an arm, that call gets no onset (the previous subframe's
    # values above its own), no correlation to speak of, a low-band
    # autocorrelation, and voicedEn / silenceEn placed around its subEnergy.
    rows = np.zeros((len(cases), AE_IN), np.int16)
    for k, (row, _, _) in enumerate(cases):
        rows[k] = row
    ref = ref_run(MODES["classify"], rows, np.full((len(cases), AE_ARGS), K, np.int32))
    for k, (row, _, _) in enumerate(cases):
        for c in range(1, K):
            E, z, pk = (int(v) for v in ref[k, c * AE_CALL + 1:c * AE_CALL + 4])
            o = c * S_CLS + CLS_SPAN
            D = 4000 + 37 * (k % 100)
            if k % 2 == 0 or E < 6144 or E + D > MAX16:
                continue
            if 6554 <= z < 16384 and pk <= 3277:
                # subEnergy between the 0.65 and the 0.6 points of voicedEn .. silenceEn: SILENCE
                ven = E + (5 * D) // 8
                row[o:o + 17] = clip16(32767 * 0.97 ** np.arange(17))
                row[o + 17:o + 23] = [32767, 16000, row[o + 19], 0, ven, ven - D]
            elif 16384 <= z < 22938 and 3072 < pk <= 3277:
                # above the thresholds, not voiced, peakiness just above 3072: TRANSITION
                row[o + 17:o + 23] = [32767, 16000, row[o + 19], 0, E, E - D]
    return cases


BUILDERS = {
    "f_pitch_scale": _cases_f_pitch_scale, "find_pitch": _cases_find_pitch, "frac_pch": _cases_frac_pch,
    "gain_ana": _cases_gain_ana, "trackPitch": lambda g: _cases_trackers(g, False),
    "pitLookahead": lambda g: _cases_trackers(g, True), "pitch_ana": _cases_pitch_ana,
    "p_avg_update": _cases_p_avg_update, "bpvc_ana": _cases_bpvc_ana, "pitchAuto": _cases_pitchAuto,
    "classify": _cases_classify,
}
assert sorted(BUILDERS) == sorted(MODES)


@functools.lru_cache(maxsize=None)
def cases(name):
    """(rows n x AE_IN int16, args n x AE_ARGS int32, descriptions)"""
    seed = 20261021 + 100 * MODES[name]
    return _pack(BUILDERS[name](np.random.default_rng(seed)), seed + 1)


@functools.lru_cache(maxsize=None)
def want(name):
    rows, args, _ = cases(name)
    return ref_run(MODES[name], rows, args)


def check(what, name, got):
    """got against the reference: no case refused, everything but the slot
    only this implementation fills bit-equal"""
    rows, args, desc = cases(name)
    ref = want(name)
    assert (ref[:, AE_INFO] == 0).all() and (ref[:, AE_MARK] == 0).all()
    refused = np.nonzero(got[:, AE_MARK] != 0)[0]
    assert len(refused) == 0, "%s, mode %d %s: ae_args_ok refuses case %d [%s]" % (
        what, MODES[name], name, refused[0], desc[refused[0]])
    g = got.copy()
    g[:, AE_INFO] = 0
    first_diff("%s, mode %d %s" % (what, MODES[name], name), g, ref,
               lambda i: "%s; args %s" % (desc[i], [int(v) for v in args[i]]), where(name))


# ------------------------------------------------------------- scalar cases

@functools.lru_cache(maxsize=None)
def scalar_cases(name):
    g = np.random.default_rng(20261021 + 7 * SMODES[name])
    if name in ("ratio", "multiCheck"):
        # positive Q7 pitches, as the tracker passes them (the reference's
        # divide_s needs 0 <= |x - y| <= max(x, y), max > 0); multiCheck's
        # multiples of the smaller one must pass the larger one before add()
        # saturates: up to PITCHMAX_Q7
        top = 32767 if name == "ratio" else PMAX_Q7
        e = np.array([1, 2, 3, 127, 128, 129, 2559, 2560, 2561, 5119, 5120, 5121, 6400, 10240, 18816, 20479, 20480,
                      32766, 32767], np.int64)
        e = e[e <= top]
        x = np.concatenate([e, g.integers(1, top + 1, 1000)])
        a, b = (v.ravel() for v in np.meshgrid(x, x, indexing="ij"))
        # near-multiples of the smaller one, either side of the half-way test
        k = g.integers(1, 9, len(a))
        near = np.clip(b * k + g.integers(-3, 4, len(a)) + (g.integers(0, 2, len(a)) * (b >> 1)), 1, top)
        a = np.where(np.arange(len(a)) % 2 == 0, a, near)
        c = np.zeros(len(a), np.int64)
    elif name == "L_ratio":
        # x > 0, y >= 0: the divider's asserted precondition holds (|y - x| <=
        # max(x, y), which is not zero)
        M = 1_000_000
        a = np.concatenate([np.array([1, 2, 32767, 6400], np.int64), g.integers(1, 32768, M)])
        y = np.where(g.random(len(a)) < 0.5, g.integers(0, 2**31, len(a)), g.integers(0, 1 << 17, len(a)))
        near = np.clip(a + g.integers(-40, 41, len(a)), 0, 2**31 - 1)
        b = np.where(np.arange(len(a)) % 3 == 0, near, y)
        c = np.zeros(len(a), np.int64)
    elif name == "updateEn":
        # ifact in (0, 32767): both logarithms' arguments are positive; the
        # energies either side of the two thresholds on (curr - prev) / 2
        M = 1_000_000
        a = g.integers(-32768, 32768, M)
        delta = np.array([-2050, -2049, -2048, -2047, 6143, 6144, 6145, 6146, 0, 1, -1], np.int64)
        cur_edge = np.clip(a + delta[g.integers(0, len(delta), M)], -32768, 32767)
        c = np.where(np.arange(M) % 2 == 0, cur_edge, g.integers(-32768, 32768, M))
        b = np.where(np.arange(M) % 4 == 0, 29491, np.where(np.arange(M) % 4 == 1,
                                                            np.array([1, 2, 32765, 32766])[g.integers(0, 4, M)],
                                                            g.integers(1, 32767, M)))
    else:
        raise KeyError(name)
    args = np.stack([a, b, c, np.zeros(len(a), np.int64)], axis=1)
    return np.ascontiguousarray(args.astype(np.int32))


@functools.lru_cache(maxsize=None)
def scalar_want(name):
    return ref_run(SMODES[name], None, scalar_cases(name))


def check_scalar(what, name, got):
    args = scalar_cases(name)
    first_diff("%s, scalar mode %d %s" % (what, SMODES[name], name), got, scalar_want(name),
               lambda i: "%s(%s)" % (name, ", ".join(str(int(v)) for v in args[i])))


# ------------------------------------------------- what the cases must reach

def _calls(name, k):
    """value k of every call of every case, from the reference: cases x calls"""
    K = int(cases(name)[1][:, 0].min())	# the calls every case makes
    return want(name)[:, k:K * AE_CALL:AE_CALL]


def _scaled_energy(name):
    """extra + sum 2 y^2 of the reference's scaled output, per case"""
    rows, args, _ = cases(name)
    ref = want(name)
    e2 = np.zeros(len(args), np.int64)
    for i, a in enumerate(args):
        y = ref[i, AE_RET + a[1]:AE_RET + a[1] + a[2]].astype(np.int64)
        e2[i] = a[3] + (2 * y * y).sum()
    return e2


def test_f_pitch_scale_cases_sit_on_the_thresholds():
    rows, args, _ = cases("f_pitch_scale")
    ref = want("f_pitch_scale")
    ein = np.array([energy(rows[i, a[0]:a[0] + a[2]]) for i, a in enumerate(args)])
    for v in (0, 2**31 - 2, LW_MAX, 2**31, 2**31 + 1):
        assert (ein == v).sum() >= 2, "window energy %d" % v
    e2 = _scaled_energy("f_pitch_scale")
    for extra in (False, True):
        sel = (args[:, 3] > 0) == extra
        assert (e2[sel] <= LW_MAX).sum() >= 4
        assert (e2[sel] > LW_MAX).sum() >= 4, "output energy above 2^31-1, extra %s" % extra
    assert (e2 == LW_MAX - 1).sum() >= 10 and (e2 == LW_MAX + 1).sum() >= 10 and (e2 == LW_MAX).sum() >= 5
    assert len(set(int(v) for v in ref[:, 0])) >= 12, "shifts %s" % sorted(set(ref[:, 0]))
    assert (ref[:, 0] > 0).any() and (ref[:, 0] < 0).any() and (ref[:, 0] == 0).any()
    inplace = args[:, 0] == args[:, 1]
    assert inplace.sum() >= 100 and (~inplace).sum() >= 100
    for sel in (inplace, ~inplace):
        assert set(range(1, 41)) <= set(int(v) for v in args[sel, 2])
        assert {0, 1} <= set(int(v) & 1 for v in args[sel, 0]) and {0, 1} <= set(int(v) & 1 for v in args[sel, 1])


def test_find_pitch_cases_cover_the_lag_blocks():
    rows, args, _ = cases("find_pitch")
    ref = want("find_pitch")
    nl = args[:, 3] - args[:, 2] + 1
    cb0 = -((args[:, 4] + args[:, 3]) >> 1)
    for f in range(AE_FORMS):
        sel = args[:, 1] == f
        assert set(range(1, 25)) <= set(int(v) for v in nl[sel]), "lag counts, form %d" % f
        assert {0, 1} <= set(int(v) & 1 for v in cb0[sel & (nl > 12)])
    assert ((ref[:, 0] == args[:, 2]) & (ref[:, 1] == 0)).sum() >= 6, "no positive correlation: ip stays lower"
    assert (ref[:, 1] >= 16000).sum() >= 20 and ((ref[:, 1] > 0) & (ref[:, 1] < 8000)).sum() >= 20
    # form 2 takes the unscaled window where the energy allows, with lsh 0 and above
    e = np.array([energy(rows[i, a[0]:a[0] + AE_PW]) for i, a in enumerate(args)])
    quiet = (args[:, 1] == 2) & (e <= LW_MAX)
    assert (quiet & (ref[:, 2] == 0)).sum() >= 3 and (quiet & (ref[:, 2] < 0)).sum() >= 20
    assert ((args[:, 1] == 2) & (e > LW_MAX)).sum() >= 20


def _flag_false_and_clamps(name, seg_of):
    """from the reference's scaled windows: form-1 cases whose energy passes
    2^31 - 1, and cases in which one segment's own energy chain clamps"""
    rows, args, _ = cases(name)
    ref = want(name)
    y = np.stack([ref[i, AE_RET + a[0]:AE_RET + a[0] + AE_PW] for i, a in enumerate(args)]).astype(np.int64)
    over = (2 * y * y).sum(axis=1) > LW_MAX
    clamp = np.zeros(len(args), bool)
    for i, a in enumerate(args):
        for lo, hi in seg_of(a):
            clamp[i] |= int((2 * y[i, lo:hi] ** 2).sum()) > LW_MAX
    return args[:, 1], over, clamp


def test_pit_lib_cases_leave_the_exact_path_by_themselves():
    """modes 1 and 2 hold windows whose flag f_pitch_scale itself gives as
    false (not only form 0, which forces it), and windows on which an energy
    chain clamps, so that the sequential and the exact path differ there"""
    def fp_segs(a):
        cb0 = AE_PC - ((a[4] + a[3]) >> 1)
        return [(cb0, cb0 + a[4]), (cb0 + a[3], cb0 + a[3] + a[4])]

    def fr_segs(a):
        ip = min((a[2] + 64) >> 7, PITCHMAX - 1)
        ln = max(ip, a[4])
        cb = AE_PC - ((ln + ip) >> 1)
        return [(cb, cb + ln), (cb + ip - 1, cb + ip + ln + 1)]
    for name, segs in (("find_pitch", fp_segs), ("frac_pch", fr_segs)):
        form, over, clamp = _flag_false_and_clamps(name, segs)
        assert ((form == 1) & over).sum() >= 12, "%s: form 1 with the flag false: %d" % (name, ((form == 1) & over).sum())
        assert ((form == 1) & clamp).sum() >= 6 and ((form == 0) & clamp).sum() >= 6, "%s: a clamping chain" % name


def test_frac_pch_cases_reach_the_clamps():
    rows, args, _ = cases("frac_pch")
    ref = want("frac_pch")
    for rng in (0, 5):
        sel = args[:, 3] == rng
        assert (sel & (ref[:, 0] == PMAX_Q7)).sum() >= 2, "clamp at pmax_q7, range %d" % rng
        assert (sel & (ref[:, 0] == PMIN_Q7)).sum() >= 2, "clamp at pmin_q7, range %d" % rng
        assert (sel & (ref[:, 1] == 0)).sum() >= 2 and (sel & (ref[:, 1] == 16384)).sum() >= 2, "pcorr 0 and 16384"
        for f in range(AE_FORMS):
            assert (sel & (args[:, 1] == f)).sum() >= 60
    ip = (args[:, 2] + 64) >> 7
    r0 = args[:, 3] == 0
    # range 0: the ip-1 outcome shows as a result at least a sample below the estimate's lag
    assert (r0 & (ref[:, 0] < (ip - 1) * 128 + 64)).sum() >= 10 and (r0 & (ref[:, 0] >= ip * 128)).sum() >= 10
    frac = ref[:, 0] - (ref[:, 0] >> 7 << 7)
    assert len(set(int(v) for v in frac)) >= 100, "fractions"
    assert (args[:, 4] < 160).sum() >= 40


def test_gain_ana_cases_clamp_both_ways():
    _, args, _ = cases("gain_ana")
    ref = want("gain_ana")
    assert (ref[:, 0] == 0).sum() >= 10 and (ref[:, 0] > 15000).sum() >= 10
    ln = np.zeros(len(args), np.int64)
    for i, a in enumerate(args):
        fl = a[1] >> 1
        while fl < (a[2] << 6):
            fl += a[1] >> 1
        ln[i] = (fl + 32) >> 6
    assert (ln > args[:, 3]).sum() >= 20 and (ln <= args[:, 3]).sum() >= 100, "halved by maxlen, and not"
    assert {0, 1} <= set(int(v) & 1 for v in ln)


def test_pitch_ana_cases_take_every_outcome():
    rows, _, _ = cases("pitch_ana")
    pitch, pcorr = _calls("pitch_ana", 0), _calls("pitch_ana", 1)
    K = pitch.shape[1]
    pest = np.stack([rows[:, c * S_PANA + 2 * AE_PW] for c in range(K)], 1).astype(np.int64)
    pavg = np.stack([rows[:, c * S_PANA + 2 * AE_PW + 1] for c in range(K)], 1).astype(np.int64)
    avg = pitch == pavg
    assert (avg.sum() >= 100) and ((~avg).sum() >= 400), "the average pitch, and a found one"
    assert (avg == (pcorr < 9012)).all()
    for lo, hi in ((9012, 9831), (9831, 12000), (12000, 16385)):
        assert ((pcorr >= lo) & (pcorr < hi)).sum() >= 20, "pcorr in [%d, %d)" % (lo, hi)
    found = ~avg
    # double_chk leaves the estimate for a sub-multiple, at several m, or keeps it
    ratio = np.where(found, np.rint(pest / np.maximum(pitch, 1)), 0)
    for m in (2, 3, 4):
        assert (ratio == m).sum() >= 5, "break at m = %d" % m
    assert (ratio == 1).sum() >= 300
    assert (found & (pitch > 12800)).sum() >= 50 and (found & (pitch < 3840)).sum() >= 20
    assert (found[:, 1:]).sum() >= 300, "later calls"
    # a loud speech tail left behind, then a clean long-lag frame whose search
    # keeps the residual (a high pcorr) and whose second segment reads the tail
    desc = cases("pitch_ana")[2]
    loud = np.array(["loud speech tail" in d for d in desc])
    assert (loud[:, None] & found & (pitch >= 155 * 128) & (pcorr >= 12000))[:, 1:].sum() >= 20
    # the second pcorr < 9012 test: double_chk brings a found pitch's pcorr down
    # (a speech search alone would have kept it at or above 9012)
    assert (avg & (pcorr > 0)).sum() >= 50


def test_bpvc_ana_cases_take_either_candidate():
    rows, _, _ = cases("bpvc_ana")
    K = _calls("bpvc_ana", 0).shape[1]
    pitch = _calls("bpvc_ana", 5)
    f0 = np.stack([rows[:, c * S_BPVC + FRAME] for c in range(K)], 1).astype(np.int64)
    f1 = np.stack([rows[:, c * S_BPVC + FRAME + 1] for c in range(K)], 1).astype(np.int64)
    far = np.abs(f0 - f1) > 12 * 128
    first, second = far & (np.abs(pitch - f0) < 6 * 128), far & (np.abs(pitch - f1) < 6 * 128)
    assert first.sum() >= 200 and second.sum() >= 200, (first.sum(), second.sum())
    for b in range(5):
        v = _calls("bpvc_ana", b)
        assert (v >= 9830).sum() >= 100 and (v < 9830).sum() >= 100, "band %d voiced and unvoiced" % b


def test_pitchAuto_cases_cover_the_peak_list():
    pit = np.stack([_calls("pitchAuto", k) for k in range(NODE)], 2)
    wgt = np.stack([_calls("pitchAuto", NODE + k) for k in range(NODE)], 2)
    pitch, corx = _calls("pitchAuto", 2 * NODE), _calls("pitchAuto", 2 * NODE + 1)
    pad = ((pit == 100) & (wgt == 0)).sum(axis=2)
    assert set(range(NODE)) <= set(int(v) for v in pad.ravel()), "padded entries per frame: %s" % sorted(set(pad.ravel()))
    nopeak = corx == 0
    assert nopeak.sum() >= 50 and (pitch[nopeak] == MAXPITCH).all(), "frames with no positive peak"
    has147 = (pit == MAXPITCH).any(axis=2)
    w147 = np.where(pit == MAXPITCH, wgt, 0).max(axis=2)
    assert (has147 & (w147 > 0) & (pad == 0)).sum() >= 3, "a peak at MAXPITCH, the list full"
    assert (has147 & (w147 == 0) & (pad > 0) & ~nopeak).sum() >= 10, "lag MAXPITCH in a list that is not full"
    assert ((pit == MINPITCH) & (wgt > 0)).sum() >= 10, "a peak at MINPITCH"
    assert (pitch == MINPITCH).sum() >= 3 and (pitch == MAXPITCH).sum() >= 3
    assert ((wgt == 0) & (pit != 100) & (pit != MAXPITCH)).sum() >= 20, "weights reduced to nothing by a multiple"


def test_classify_cases_take_each_class():
    rows, _, _ = cases("classify")
    cl = _calls("classify", 0)
    K = cl.shape[1]
    for v in (0, 1, 3):
        for c in (0, 1, K - 1):
            assert (cl[:, c] == v).sum() >= 5, "class %d in call %d" % (v, c)
    pitch = _calls("classify", 5)
    for sel in (pitch <= MINPITCH + 4, pitch >= MAXPITCH - 4):	# frac_cor's scan clamped to fewer than ten lags
        assert sel.sum() >= 40 and {0, 1} <= set(int(v) & 1 for v in pitch[sel])
    sen, ven = _calls("classify", 7), _calls("classify", 6)
    given = np.stack([rows[:, c * S_CLS + CLS_SPAN + 22] for c in range(K)], 1)
    assert (sen[:, 1:] != given[:, 1:]).sum() >= 100 and (sen[:, 1:] == given[:, 1:]).sum() >= 100, "silenceEn clamped"
    assert (_calls("classify", 1) == -20480).sum() >= 50 and (_calls("classify", 3) == 2048).sum() >= 50


# ------------------------------------------------------------------ CPU

def run_emu(lib, name):
    rows, args, _ = cases(name)
    out = np.zeros((len(args), AE_OUT), np.int32)
    assert lib.emu_ana_eval(MODES[name], ptr(rows), ptr(args), ptr(out), len(args)) == 0
    return out


def check_exact_flag(what, got):
    """the device-only flag of f_pitch_scale against its definition, computed
    from the reference's scaled output: extra + sum 2 y^2 <= 2^31 - 1"""
    _, args, desc = cases("f_pitch_scale")
    expect = (_scaled_energy("f_pitch_scale") <= LW_MAX).astype(np.int32)
    first_diff("%s, f_pitch_scale's exact flag" % what, got[:, AE_INFO], expect, lambda i: desc[i])


@pytest.mark.parametrize("name", sorted(MODES, key=MODES.get))
def test_hostemu(name):
    got = run_emu(emu(), name)
    check("host build", name, got)
    if name == "f_pitch_scale":
        check_exact_flag("host build", got)


@pytest.mark.parametrize("name", sorted(SMODES, key=SMODES.get))
def test_hostemu_scalar(name):
    args = scalar_cases(name)
    out = np.zeros(len(args), np.int32)
    assert emu().emu_ana_scalar(SMODES[name], ptr(args), ptr(out), ctypes.c_long(len(args))) == 0
    check_scalar("host build", name, out)
    want = scalar_want(name)
    assert len(np.unique(want)) > 1000, "the reference's results vary"


@pytest.fixture(scope="module")
def stats_lib(tmp_path_factory):
    """a host build that counts the find_pitch / frac_pch calls of each path
    (MELPE_EXACT_STATS), compiled into a temporary directory"""
    so = str(tmp_path_factory.mktemp("exact_stats") / "libmelpe_hostemu_stats.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-DMELPE_EXACT_STATS", "-I" + CSRC,
                    os.path.join(CSRC, "hostemu.cpp"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    assert lib.emu_load_tables(TABLES.encode()) == 0
    return lib


@pytest.mark.parametrize("name", ["find_pitch", "frac_pch", "pitch_ana", "bpvc_ana"])
def test_exact_and_sequential_paths_both_run(name, stats_lib):
    """the exact correlators and the saturating chains each take at least an
    eighth of the find_pitch and of the frac_pch calls of every mode that
    reaches them (counted by a host build with MELPE_EXACT_STATS); no case
    is refused and every built case runs.

    bpvc_ana meets the split only because three fifths of its cases are
    built for it.  Its sequential calls need a window whose energy is above
    2^31 - 1 and whose scaled copy's energy is above it too, which takes
    f_pitch_scale's shift (found on the samples >> 5) one too small: the
    truncation of >> 5 has to lose energy.  It loses on positive samples and
    gains as much on negative ones, so a band-passed window (bands 1-4, and
    the envelopes, whose filter starts with a difference) never gets there;
    only band 0, which passes a constant, does, with the input's offset tuned
    to the filter's gain (_sequential_band0).  Band 0 makes two of a call's
    ten frac_pch calls, hence so many such cases, of eight calls each.  On
    these cases the two paths give equal results (the window's energy passes
    the bound by a percent or two, and no chain of half a window's samples
    clamps): they run the sequential path, on the device too, and would not
    notice a wrong choice between the two.  That choice is bound by modes 0,
    1, 2 and pitch_ana's loud tails."""
    lib = stats_lib
    stats = (ctypes.c_long * 6).in_dll(lib, "melpe_exact_stats")
    for k in range(6):
        stats[k] = 0
    got = run_emu(lib, name)
    check("host build with MELPE_EXACT_STATS", name, got)	# every built case ran, none refused
    c = [int(stats[k]) for k in range(4)]
    print("%s: find_pitch sequential %d exact %d, frac_pch sequential %d exact %d" % (name, *c))
    assert c[0] + c[1] > 0 and (name == "find_pitch" or c[2] + c[3] > 0)
    for a, b in ((0, 1), (2, 3)):
        assert 8 * c[a] >= c[a] + c[b] and 8 * c[b] >= c[a] + c[b], "%s: counters %s" % (name, c)


# ------------------------------------------------------------------ GPU

def _device_modes(names):
    torch, lib, dev, s = _device()
    for name in names:
        rows, args, _ = cases(name)
        want(name)
        t0 = time.perf_counter()
        dr, da = torch.from_numpy(rows).to(dev), torch.from_numpy(args).to(dev)
        do = torch.zeros((len(args), AE_OUT), dtype=torch.int32, device=dev)
        rc = lib.melpe_ana_eval_dev(MODES[name], dr.data_ptr(), da.data_ptr(), do.data_ptr(), len(args), s)
        assert rc == 0, lib.melpe_last_error()
        got = do.cpu().numpy()
        print("%s: %d cases, %.3f s on the device" % (name, len(got), time.perf_counter() - t0))
        check("device", name, got)
        if name == "f_pitch_scale":
            check_exact_flag("device", got)


@pytest.mark.gpu
def test_device_pit_lib():
    _device_modes(["f_pitch_scale", "find_pitch", "frac_pch"])


@pytest.mark.gpu
def test_device_pitch_ana_and_average():
    _device_modes(["pitch_ana", "p_avg_update"])


@pytest.mark.gpu
def test_device_bpvc_ana():
    _device_modes(["bpvc_ana"])


@pytest.mark.gpu
def test_device_tracker_and_pitchAuto():
    _device_modes(["trackPitch", "pitLookahead", "pitchAuto"])
    torch, lib, dev, s = _device()
    for name in sorted(SMODES, key=SMODES.get):
        args = scalar_cases(name)
        da = torch.from_numpy(args).to(dev)
        do = torch.zeros(len(args), dtype=torch.int32, device=dev)
        rc = lib.melpe_ana_scalar_dev(SMODES[name], da.data_ptr(), do.data_ptr(), len(args), s)
        assert rc == 0, lib.melpe_last_error()
        check_scalar("device", name, do.cpu().numpy())


@pytest.mark.gpu
def test_device_classify_and_gain_ana():
    _device_modes(["classify", "gain_ana"])
