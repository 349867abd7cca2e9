#!/usr/bin/env python3
"""Generates tests/golden/synpar.json from the REFERENCE's synthesis() with its
own build switch SKIP_CHANNEL on (melpe/sc1200.h:53, melpe/melp_syn.c:110-146):
the analysis-to-synthesis loop without a channel, which is what
melpe_synth_params computes.

The harness tests/golden/ref_synpar.c compiles melp_syn.c where it lies with
the switch redefined and links the rest from oracle/_ref/libmelpe_ref.a; it is
built here on demand into oracle/_ref/ref_synpar.  Runs only in the dev
container; the tests import `case_rows` and the constants from here and never
need the harness.

32 channels x 24 superframes of parameter rows ([C, K, 90] int16: three frames
of struct melp_param), integer-only numpy.  Kind of channel c = c % 4:
  0  the encoder's melp_par for csrc/synth.h channel c (the host build's
     emu_enc_params; main() asserts it equals `ref_tool enc`'s dump)
  1  kind 0's rows edited: the pitch scaled by a per-channel factor in
     [1/2, 2] and clamped to the pitch range, the voicing flipped on a third of
     the frames, the gains shifted by up to +-6 dB inside the quantiser's range
  2  random rows drawn field by field inside the admission ranges (decoder.h
     syn_row_admit), the LSFs ascending and spaced
  3  the channel reader's rows (before melp_syn's parameter head) of the
     encoder's bitstream for channel c (the host build's emu_read_rows on the
     host build's bits; main() asserts the bits equal the reference encoder's)
The JSON holds the recipe constants, per channel the SHA-256 of the reference's
PCM and of melp_par as synthesis() left it, and the counts main() asserts.
"""
import ctypes
import functools
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

REFERENCE = "/root/reference"
REF_DIR = os.path.join(ROOT, "oracle", "_ref")
TOOL = os.path.join(REF_DIR, "ref_synpar")
REF_TOOL = os.path.join(REF_DIR, "ref_tool")
EMU = os.path.join(ROOT, "build", "libmelpe_hostemu.so")
TABLES = os.path.join(ROOT, "pairphone_amd", "data", "melpe_tables.bin")

SEED, C, K = 3107, 32, 24
ENC_DUMP = 1332     # bytes per superframe of `ref_tool enc`'s dump

# struct melp_param, word offsets within a frame's 30
PITCH, LSF, GAIN, JITTER, BPVC, UV, FSMAG = 0, slice(1, 11), slice(11, 13), 13, slice(14, 19), 19, slice(20, 30)
PITCH_MIN, PITCH_MAX = 2560, 20480      # Q7: 20 .. 160 samples
GAIN_MIN, GAIN_MAX = 2560, 19712        # Q8: the gain quantiser's 10 .. 77 dB
ADM_GAIN_MAX = 20480                    # admission: 0 .. 80 dB
JITTER_MAX, BPVC_MAX = 8192, 16384


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def emu():
    lib = ctypes.CDLL(EMU)
    lib.emu_create.restype = ctypes.c_void_p
    lib.emu_create.argtypes = [ctypes.c_int]
    lib.emu_destroy.argtypes = [ctypes.c_void_p]
    vp = ctypes.c_void_p
    lib.emu_encode.argtypes = [vp, vp, vp]
    lib.emu_enc_params.argtypes = [vp, ctypes.c_int, vp]
    lib.emu_read_rows.argtypes = [vp, vp, vp, vp]
    lib.emu_row_admit.argtypes = [vp, vp, ctypes.c_long]
    lib.emu_synth_params.argtypes = [vp, vp, vp, vp]
    lib.emu_synth_params2.argtypes = [vp, vp, vp, vp]
    assert lib.emu_load_tables(TABLES.encode()) == 0
    return lib


def signals(channels, nsf=K, seed=SEED):
    from pairphone_amd import synth_signal
    return np.stack([synth_signal(seed, c, nsf * 540) for c in range(channels)])


def encoder_rows(x, nsf):
    """the host build's melpe_a over x [n, nsf * 540]: (melp_par [n, nsf, 90], bits [n, nsf, 11])"""
    lib = emu()
    n = x.shape[0]
    e = lib.emu_create(n)
    par = np.zeros((n, nsf, 90), np.int16)
    bits = np.zeros((n, nsf, 11), np.uint8)
    tap = np.zeros(120, np.int16)
    for k in range(nsf):
        sp = np.ascontiguousarray(x[:, k * 540:(k + 1) * 540])
        b = np.zeros((n, 11), np.uint8)
        lib.emu_encode(e, b.ctypes.data, sp.ctypes.data)
        bits[:, k] = b
        for c in range(n):
            lib.emu_enc_params(e, c, tap.ctypes.data)
            par[c, k] = tap[:90]
    lib.emu_destroy(e)
    return par, bits


def reader_rows(bits):
    """emu_read_rows over bits [n, nsf, 11]: (pre-head rows [n, nsf, 90], erase [n, nsf])"""
    lib = emu()
    n, nsf = bits.shape[:2]
    e = lib.emu_create(n)
    rows = np.zeros((n, nsf, 90), np.int16)
    erase = np.zeros((n, nsf), np.uint8)
    for k in range(nsf):
        b = np.ascontiguousarray(bits[:, k])
        r = np.zeros((n, 90), np.int16)
        er = np.zeros(n, np.uint8)
        assert lib.emu_read_rows(e, r.ctypes.data, er.ctypes.data, b.ctypes.data) == 0
        rows[:, k], erase[:, k] = r, er
    lib.emu_destroy(e)
    return rows, erase


def edit_rows(c, rows, seed=SEED):
    """kind 1: channel c's encoder rows [nsf, 90] with pitch, voicing and gains edited"""
    rng = np.random.Generator(np.random.PCG64(seed + 1000 + c))
    r = rows.reshape(-1, 3, 30).astype(np.int32)
    num = int(rng.integers(64, 257))            # pitch factor num / 128 in [1/2, 2]
    r[..., PITCH] = np.clip(r[..., PITCH] * num // 128, PITCH_MIN, PITCH_MAX)
    flip = rng.integers(0, 3, r.shape[:2]) == 0
    r[..., UV] = np.where(flip, 1 - (r[..., UV] != 0), r[..., UV])
    r[..., GAIN] = np.clip(r[..., GAIN] + rng.integers(-1536, 1537, r.shape[:2] + (2,)), GAIN_MIN, GAIN_MAX)
    return r.astype(np.int16).reshape(rows.shape)


def random_rows(c, nsf, seed=SEED):
    """kind 2: rows drawn inside the admission ranges; one frame in eight at each pitch extreme"""
    rng = np.random.Generator(np.random.PCG64(seed + 2000 + c))
    r = np.zeros((nsf, 3, 30), np.int32)
    p = rng.integers(PITCH_MIN, PITCH_MAX + 1, (nsf, 3))
    ext = rng.integers(0, 8, (nsf, 3))
    r[..., PITCH] = np.where(ext == 0, PITCH_MIN, np.where(ext == 1, PITCH_MAX, p))
    r[..., LSF] = np.cumsum(rng.integers(410, 2950, (nsf, 3, 10)), axis=-1)
    r[..., GAIN] = rng.integers(0, ADM_GAIN_MAX + 1, (nsf, 3, 2))
    r[..., JITTER] = rng.integers(0, JITTER_MAX + 1, (nsf, 3))
    r[..., BPVC] = rng.integers(0, BPVC_MAX + 1, (nsf, 3, 5))
    r[..., UV] = rng.integers(0, 2, (nsf, 3))
    r[..., FSMAG] = rng.integers(0, 32768, (nsf, 3, 10))
    assert r[..., LSF].max() <= 32767
    return r.astype(np.int16).reshape(nsf, 90)


@functools.lru_cache(maxsize=None)
def _case(channels, nsf):
    enc_par, bits = encoder_rows(signals(channels, nsf), nsf)
    rd, erase = reader_rows(bits)
    rows = np.zeros((channels, nsf, 90), np.int16)
    for c in range(channels):
        kind = c % 4
        rows[c] = (enc_par[c], edit_rows(c, enc_par[c]), random_rows(c, nsf), rd[c])[kind]
    for a in (rows, enc_par, bits, erase):
        a.setflags(write=False)
    return rows, enc_par, bits, erase


def case_rows(channels=C, nsf=K):
    """[channels, nsf, 90] int16 (read-only, computed once): the rows of the
    case; its first 32 channels x 24 superframes are the fixture's"""
    return _case(channels, nsf)[0]


def admit(rows):
    """(rows after admission, status per frame row) by the host build's syn_row_admit"""
    lib = emu()
    r = np.ascontiguousarray(rows, np.int16).reshape(-1, 30).copy()
    st = np.zeros(len(r), np.uint8)
    assert lib.emu_row_admit(r.ctypes.data, st.ctypes.data, len(r)) == 0
    return r.reshape(np.shape(rows)), st


def uv_patterns(rows):
    r = np.asarray(rows).reshape(-1, 3, 30)[:, :, UV]
    return set(map(tuple, (r != 0).astype(int).tolist()))


def build_tool():
    os.makedirs(REF_DIR, exist_ok=True)
    subprocess.run(["gcc", "-O2", "-w", "-I" + REFERENCE + "/melpe", os.path.join(HERE, "ref_synpar.c"),
                    os.path.join(REF_DIR, "libmelpe_ref.a"), "-lm", "-o", TOOL], check=True)


def ref_channel(rows):
    """one channel through the harness: (pcm [nsf, 540], melp_par afterwards [nsf, 90])"""
    with tempfile.TemporaryDirectory() as tmp:
        fi, fo = os.path.join(tmp, "in"), os.path.join(tmp, "out")
        np.ascontiguousarray(rows, "<i2").tofile(fi)
        subprocess.run([TOOL, fi, fo], check=True)
        o = np.fromfile(fo, "<i2").reshape(len(rows), 630)
    return o[:, :540].copy(), o[:, 540:].copy()


def main():
    build_tool()
    rows, enc_par, bits, erase = _case(C, K)
    x = signals(C)
    with tempfile.TemporaryDirectory() as tmp:
        for c in range(C):
            p = os.path.join(tmp, "c%d" % c)
            x[c].tofile(p + ".pcm")
            subprocess.run([REF_TOOL, "enc", p + ".pcm", p + ".bits", p + ".dump"], check=True)
            d = np.fromfile(p + ".dump", np.uint8).reshape(K, ENC_DUMP)
            assert np.array_equal(d[:, :180].copy().view(np.int16), enc_par[c]), \
                "channel %d: the host build's melp_par differs from the reference encoder's" % c
            assert np.array_equal(np.fromfile(p + ".bits", np.uint8).reshape(K, 11), bits[c]), \
                "channel %d: the host build's bits differ from the reference encoder's" % c
    assert not erase.any(), "a valid bitstream was flagged erased"
    after, st = admit(rows)
    assert not st.any() and np.array_equal(after, rows), "a fixture row does not pass admission unchanged"
    pats = uv_patterns(rows)
    pitch = rows.reshape(-1, 30)[:, PITCH]
    counts = {"uv_patterns": len(pats), "pitch_min_rows": int((pitch == PITCH_MIN).sum()),
              "pitch_max_rows": int((pitch == PITCH_MAX).sum()), "status_nonzero": int(st.sum())}
    assert counts["uv_patterns"] == 8 and counts["pitch_min_rows"] > 0 and counts["pitch_max_rows"] > 0
    doc = {"what": "synthesis() of melpe/melp_syn.c with SKIP_CHANNEL TRUE via tests/golden/ref_synpar.c",
           "seed": SEED, "channels": C, "superframes": K, "rows_sha256": sha(rows), "counts": counts,
           "pcm_sha256": [], "post_sha256": []}
    for c in range(C):
        pcm, post = ref_channel(rows[c])
        doc["pcm_sha256"].append(sha(pcm))
        doc["post_sha256"].append(sha(post))
    path = os.path.join(HERE, "synpar.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote synpar.json, %d bytes; %s" % (os.path.getsize(path), counts))
    assert os.path.getsize(path) < 16000


if __name__ == "__main__":
    sys.exit(main())
