"""How mixed the waves of the lane analysis are in the voicing pattern lsf_vq
branches on (CPU diagnostics, host build only).

lsf_vq (quant.h lsf_vq_u) branches on the superframe's voicing pattern uvc,
the three uv_flags after sc_ana, and lspVQ_t scans a codebook once per
distinct codebook among a wave's lanes: a wave pays the union of its lanes'
branches.  This tool encodes N channels of the bench's input with the host
build (emu_encode), reads each superframe's parameters (emu_enc_params) and
cuts the channels into waves of 64 under two lane orders:

  engine key   the first lane order (k_state.hip bin_class): the voiced-frame
               count and last pitch of the channel's PREVIOUS superframe;
  pattern key  the second lane order: uvc of the CURRENT superframe.

Per timed superframe it reports the waves that hold more than one pattern
and the codebook rows a wave scans in lsf_vq, in rows of dimension 10 (a
dimension-20 row counts as two, the interpolation search as 600):

  lspVQ on the 512-row unvoiced codebook                512
  lspVQ on the 256/64/32/32 voiced one, 8 candidates    256 + 8 * 128 = 1280
  residual VQ, 256/64 of dimension 20                   2 * (256 + 8 * 64) = 1536
  residual VQ, 256/64/64/64 (uvc == 1)                  2 * (256 + 8 * 192) = 3584

The final uv_flags stand for the ones lsf_vq sees: quant_bp recomputes them
from bpvc[0], which sc_ana keeps, by the test melp_ana made them with.

  python tools/voicing_mix.py [--channels 4096] [--warmup 5] [--steps 20] [--jobs 8]
"""
import argparse
import ctypes
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RUN_SEED = 2026  # bench.py's
WAVE = 64
UV_ROWS, V_ROWS, INTERP, RES2, RES4 = 512, 1280, 600, 1536, 3584
SEP = (7, 6, 5, 3)  # at most one voiced frame: each frame quantised alone


def _chunk(args):
    """channels [c0, c0 + n): per superframe the pattern (uvc), the final
    pitch of frame 2 (Q7) and the voiced-frame count"""
    c0, n, nsf = args
    from pairphone_amd import synth_signal
    from pairphone_amd.params import PITCH, UV_FLAG
    lib = ctypes.CDLL(os.path.join(ROOT, "build", "libmelpe_hostemu.so"))
    lib.emu_create.restype = ctypes.c_void_p
    lib.emu_create.argtypes = [ctypes.c_int]
    lib.emu_encode.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.emu_enc_params.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    lib.emu_destroy.argtypes = [ctypes.c_void_p]
    tables = os.path.join(ROOT, "pairphone_amd", "data", "melpe_tables.bin")
    assert lib.emu_load_tables(tables.encode()) == 0
    x = np.stack([synth_signal(RUN_SEED, c0 + c, nsf * 540) for c in range(n)])
    e = lib.emu_create(n)
    uvc = np.zeros((nsf, n), np.int32)
    pitch = np.zeros((nsf, n), np.int32)
    bits = np.zeros((n, 11), np.uint8)
    row = np.zeros(120, np.int16)
    for k in range(nsf):
        sp = np.ascontiguousarray(x[:, k * 540:(k + 1) * 540])
        lib.emu_encode(e, bits.ctypes.data, sp.ctypes.data)
        for c in range(n):
            lib.emu_enc_params(e, c, row.ctypes.data)
            par = row[:90].reshape(3, 30)
            uv = (par[:, UV_FLAG] != 0).astype(int)
            uvc[k, c] = uv[0] * 4 + uv[1] * 2 + uv[2]
            pitch[k, c] = par[2, PITCH]
    lib.emu_destroy(e)
    return uvc, pitch


def wave_rows(p):
    """row-equivalents lsf_vq scans in a wave whose lanes hold patterns p"""
    p = np.asarray(p)
    sep = np.isin(p, SEP)
    rows = 0
    for bit in (4, 2):  # frames 0 and 1 alone: the sep lanes' call sites
        uv = (p[sep] & bit) != 0
        rows += UV_ROWS * bool(uv.any()) + V_ROWS * bool((~uv).any())
    uv2 = (p & 1) != 0  # frame 2: every lane
    rows += UV_ROWS * bool(uv2.any()) + V_ROWS * bool((~uv2).any())
    if (~sep).any():
        rows += INTERP + (RES4 if (p == 1).any() else RES2)
    return rows


def engine_key(prev_uvc, prev_pitch):
    """k_state.hip bin_class on the previous superframe"""
    nv = 3 - ((prev_uvc >> 2) & 1) - ((prev_uvc >> 1) & 1) - (prev_uvc & 1)
    b = np.clip((prev_pitch >> 7) - 20, 0, 141)
    return nv * 142 + b


def cut(order, pattern):
    w = [pattern[order[i:i + WAVE]] for i in range(0, len(order), WAVE)]
    mixed = sum(1 for q in w if len(set(q.tolist())) > 1)
    return len(w), mixed, float(np.mean([wave_rows(q) for q in w]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--jobs", type=int, default=8)
    a = ap.parse_args()
    nsf = a.warmup + a.steps
    per = (a.channels + a.jobs - 1) // a.jobs
    jobs = [(c0, min(per, a.channels - c0), nsf) for c0 in range(0, a.channels, per)]
    with ProcessPoolExecutor(a.jobs) as ex:
        parts = list(ex.map(_chunk, jobs))
    uvc = np.concatenate([p[0] for p in parts], axis=1)
    pitch = np.concatenate([p[1] for p in parts], axis=1)
    print("voicing mix of the lane analysis' waves: %d channels, run seed %d, superframes %d..%d, "
          "waves of %d" % (a.channels, RUN_SEED, a.warmup, nsf - 1, WAVE))
    print("pattern uvc: frame 0 in bit 2, 1 = unvoiced; rows = codebook rows of dimension 10 "
          "scanned by lsf_vq per wave (mean over the waves)")
    print("%3s | %-47s | %5s %5s %7s | %5s %7s | %5s" % (
        "sf", "channels per pattern uvc 0..7", "waves", "mixed", "rows", "mixed", "rows", "ratio"))
    print("%3s | %-47s | %19s | %13s |" % ("", "", "engine key", "pattern key"))
    tot = np.zeros(8, np.int64)
    ratios = []
    for k in range(a.warmup, nsf):
        hist = np.bincount(uvc[k], minlength=8)
        tot += hist
        o1 = np.argsort(engine_key(uvc[k - 1], pitch[k - 1]), kind="stable")
        o2 = np.argsort(uvc[k], kind="stable")
        n1, m1, r1 = cut(o1, uvc[k])
        _, m2, r2 = cut(o2, uvc[k])
        ratios.append(r1 / r2)
        print("%3d | %-47s | %5d %5d %7.0f | %5d %7.0f | %5.2f" % (
            k, " ".join("%5d" % h for h in hist), n1, m1, r1, m2, r2, r1 / r2))
    share = 100.0 * tot / tot.sum()
    print("pattern shares over the timed superframes, uvc 0..7 (%): " + " ".join("%.1f" % s for s in share))
    print("rows, engine key over pattern key: %.2f .. %.2f" % (min(ratios), max(ratios)))


if __name__ == "__main__":
    main()
