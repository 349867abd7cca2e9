"""Speech from parameter tensors (melpe_synth_params), CPU side: the host
build of decoder.h synth_superframe / dec2_phase<Hb, true> and of the row
admission (syn_row_admit).

The oracle is the reference's own synthesis() with its build switch
SKIP_CHANNEL on (melpe/sc1200.h:53), run by tests/golden/ref_synpar.c;
tests/golden/synpar.json holds its PCM and melp_par hashes for the 32 x 24
case of tests/golden/make_synpar_golden.py, whose row recipe is imported here.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, GOLDEN
from test_decode import decode_all, emu_decoder, fuzz_bits, gold, sha
from test_encode import golden as enc_golden

sys.path.insert(0, GOLDEN)
import make_synpar_golden as msg  # noqa: E402

TABLES = os.path.join(ROOT, "pairphone_amd", "data", "melpe_tables.bin")


def emu_synth_all(fn, rows):
    """rows [C, K, 90] through the host form `fn` on one engine:
    (pcm [C, K * 540], status [C, K], melp_par afterwards [C, K, 90])"""
    lib = msg.emu()
    lib.emu_dec_params.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    C, K = rows.shape[:2]
    e = lib.emu_create(C)
    pcm = np.zeros((C, K * 540), np.int16)
    status = np.zeros((C, K), np.uint8)
    post = np.zeros((C, K, 90), np.int16)
    tap = np.zeros(90, np.int16)
    for k in range(K):
        r = np.ascontiguousarray(rows[:, k])
        keep = r.copy()
        sp = np.zeros((C, 540), np.int16)
        st = np.full(C, 9, np.uint8)
        assert getattr(lib, fn)(e, sp.ctypes.data, r.ctypes.data, st.ctypes.data) == 0
        assert np.array_equal(r, keep), "the input rows were written"
        pcm[:, k * 540:(k + 1) * 540], status[:, k] = sp, st
        for c in range(C):
            lib.emu_dec_params(e, c, tap.ctypes.data)
            post[c, k] = tap
    lib.emu_destroy(e)
    return pcm, status, post


@pytest.mark.parametrize("fn", ["emu_synth_params", "emu_synth_params2"])
def test_host_synthesis_matches_reference_fixture(fn):
    g = gold("synpar.json")
    rows = msg.case_rows()
    assert (g["seed"], g["channels"], g["superframes"]) == (msg.SEED, msg.C, msg.K)
    assert msg.sha(rows) == g["rows_sha256"], "the row recipe no longer gives the fixture's rows"
    pcm, status, post = emu_synth_all(fn, rows)
    assert not status.any()
    for c in range(msg.C):
        assert sha(pcm[c]) == g["pcm_sha256"][c], "PCM of channel %d (kind %d)" % (c, c % 4)
        assert sha(post[c]) == g["post_sha256"][c], "melp_par after the call, channel %d (kind %d)" % (c, c % 4)


def test_reader_rows_then_synthesis_equal_the_decoder():
    """8 channels of the 1,024-channel golden set over all 149 superframes:
    the channel reader's rows (emu_read_rows, an engine of its own) through
    emu_synth_params give emu_decode's PCM sample for sample, which is the
    reference's (dec_1024.json); no valid bitstream is flagged erased"""
    g, ge = gold("dec_1024.json"), enc_golden()
    ch, nsf = 8, g["superframes"]
    bits = np.stack([np.frombuffer(bytes.fromhex(ge["bits_hex"][c]), np.uint8) for c in range(ch)])
    lib, e, dec = emu_decoder(ch)
    want = decode_all(dec, bits, nsf)
    lib.emu_destroy(e)
    rows, erase = msg.reader_rows(bits.reshape(ch, nsf, 11))
    assert not erase.any(), "erase on channels %s" % sorted(set(np.argwhere(erase)[:, 0].tolist()))
    pcm, status, _ = emu_synth_all("emu_synth_params", rows)
    assert not status.any()
    for c in range(ch):
        np.testing.assert_array_equal(pcm[c], want[c], err_msg="channel %d" % c)
        assert sha(pcm[c]) == g["pcm_sha256"][c], "channel %d" % c


def test_admission_passes_every_valid_row():
    """status 0 and the row unchanged: every fixture row (the encoder's, the
    edited, the in-range random and the reader's) and the reader's rows of the
    dec_fuzz.json bitstreams, where random bits take every parity, FEC and
    erasure branch of low_rate_chn_read"""
    rows = msg.case_rows()
    after, st = msg.admit(rows)
    assert not st.any() and np.array_equal(after, rows)
    g = gold("dec_fuzz.json")
    ch, nsf = 16, g["superframes"]
    bits = fuzz_bits(g["seed"], g["channels"], nsf)[:ch].reshape(ch, nsf, 11)
    rd, erase = msg.reader_rows(bits)
    assert erase.any() and not erase.all(), "the fuzz streams reach erased and unerased superframes"
    after, st = msg.admit(rd)
    bad = np.argwhere(after != rd)
    assert not st.any() and not len(bad), "reader rows changed by admission, first (channel, superframe, word): %s" \
        % bad[:4].tolist()


def test_admission_clamps_and_reports():
    """a row outside the ranges comes back inside them with status 1; the
    fields the parameter head overwrites on an unvoiced frame are left alone"""
    r = np.zeros((4, 30), np.int16)
    r[0, msg.PITCH] = -1
    r[1, msg.UV] = 7
    r[1, msg.PITCH] = -300                  # unvoiced: not looked at
    r[2, msg.GAIN] = [-5, 30000]
    r[2, msg.BPVC] = [-1, 0, 16384, 16385, 32767]
    r[3, msg.LSF] = np.arange(10) * 3000    # in range
    after, st = msg.admit(r)
    assert st.tolist() == [1, 1, 1, 0]
    assert after[0, msg.PITCH] == 0 and after[1, msg.UV] == 1 and after[1, msg.PITCH] == -300
    assert after[2, msg.GAIN].tolist() == [0, msg.ADM_GAIN_MAX]
    assert after[2, msg.BPVC].tolist() == [0, 0, 16384, 16384, 16384]
    assert np.array_equal(after[3], r[3])


def test_synthesis_is_total_on_any_rows(tmp_path):
    """tests/native/synpar_check.cpp under AddressSanitizer and UBSan: 100,000
    superframes of uniformly random int16 rows, 20,000 more with the voiced
    paths open, and the four constant fills, twice (the two runs side by
    side); exit 0 and the same hash"""
    exe = str(tmp_path / "synpar_check")
    subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                    "-I" + os.path.join(ROOT, "pairphone_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "synpar_check.cpp"), "-o", exe], check=True)
    runs = [subprocess.Popen([exe, TABLES], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            for _ in range(2)]
    outs = [p.communicate(timeout=900) for p in runs]
    for p, (out, err) in zip(runs, outs):
        assert p.returncode == 0, out + err
        assert out.startswith("OK 120016 superframes"), out
    assert outs[0][0] == outs[1][0]
