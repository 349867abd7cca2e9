"""The Fourier magnitudes are computed for the last voiced frame only.

quant_fsmag (melpe/qnt12.c:1277-1356) quantises par[last].fs_mag, last the
last voiced frame of the superframe, and overwrites every other voiced
frame's magnitudes in each of its branches, so the product computes the
residual, its window and the FFT for frame last alone (quant.h fsmag_last).
The literal form, analysis_upto (the debug aid behind
melpe_debug_encode_stage and emu_encode_ana_upto), still computes them for
every voiced frame, in the reference's order.  Here the product forms run
beside it on the same input: after every superframe the bits are equal and
the analysis state's live prefix is equal byte for byte.

quant_fsmag branches on the voicing pattern (8) and on fsm_prev_uv (2); the
tests assert, from the records themselves, that the input shows all 16 cases.
Counted on the host build before the shapes were fixed (SEED 2026, 24
superframes): 512 channels give at least 100 channel-superframes in every
case and 64 channels at least 9 (fewest: uvc 1 and uvc 2 with fsm_prev_uv
set).

melpe_debug_encode_stage runs the noise preprocessor itself before the
analysis, so engine B makes that one call per superframe (a separate
encode_npp_dev before it would run the preprocessor twice).
"""
import ctypes

import numpy as np
import pytest

from test_encode import emu, signals

SEED = 2026  # the bench's run seed
NSF = 24
C_GPU = 512
C_CPU = 64


def _layout(lib):
    """byte offsets in an exported encoder record (hostemu.cpp emu_enc_layout)"""
    lib.emu_enc_layout.argtypes = [ctypes.c_void_p, ctypes.c_int]
    v = (ctypes.c_long * 7)()
    assert lib.emu_enc_layout(v, 7) == 7
    names = ("ana", "live", "par", "par_stride", "uv_flag", "fsm_prev_uv", "chbuf")
    return dict(zip(names, [int(k) for k in v]))


def _fields(ana, lay):
    """of analysis states [C, >= live] (uint8): the voicing pattern (uvc 0..7,
    frame 0 the high bit), fsm_prev_uv and the 11 channel bytes"""
    def i16(off):
        return np.ascontiguousarray(ana[:, off:off + 2]).view(np.int16)[:, 0]
    uv = [(i16(lay["par"] + i * lay["par_stride"] + lay["uv_flag"]) != 0).astype(int) for i in range(3)]
    pattern = uv[0] * 4 + uv[1] * 2 + uv[2]
    return pattern, (i16(lay["fsm_prev_uv"]) != 0).astype(int), ana[:, lay["chbuf"]:lay["chbuf"] + 11]


class _Cases:
    """the (fsm_prev_uv before the superframe, voicing pattern) cases seen"""

    def __init__(self):
        self.seen = np.zeros((2, 8), int)

    def add(self, prev_uv, pattern):
        np.add.at(self.seen, (prev_uv, pattern), 1)

    def check(self):
        print("cases seen [fsm_prev_uv][uvc]:", self.seen.tolist())
        assert (self.seen > 0).all(), "cases seen [fsm_prev_uv][uvc]: %s" % self.seen.tolist()


# ---------------------------------------------------------------- CPU

def _host_live(lib, e, ch, n):
    lib.emu_enc_live.restype = ctypes.c_long
    lib.emu_enc_live.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    out = np.zeros((ch, n), np.uint8)
    for c in range(ch):
        assert lib.emu_enc_live(e, c, out[c].ctypes.data) == n
    return out


def test_host_forms_match_the_literal_order_in_every_case():
    """the host build's unsplit analysis and its split form (what the lane
    kernels run) against analysis_upto(6), bits and live prefixes"""
    lib = emu()
    lay = _layout(lib)
    lib.emu_encode_npp.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    for fn in ("emu_encode_ana", "emu_encode_ana_split"):
        getattr(lib, fn).argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.emu_encode_ana_upto.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    ch = C_CPU
    x = signals(SEED, ch, NSF)
    forms = {
        "literal": lambda e, b, sp: lib.emu_encode_ana_upto(e, b, sp, 6),
        "unsplit": lambda e, b, sp: lib.emu_encode_ana(e, b, sp),
        "split": lambda e, b, sp: lib.emu_encode_ana_split(e, b, sp),
    }
    eng = {k: lib.emu_create(ch) for k in forms}
    cases = _Cases()
    prev_uv = _fields(_host_live(lib, eng["literal"], ch, lay["live"]), lay)[1]
    for k in range(NSF):
        got = {}
        for name, f in forms.items():
            sp = np.ascontiguousarray(x[:, k * 540:(k + 1) * 540])
            b = np.zeros((ch, 11), np.uint8)
            lib.emu_encode_npp(eng[name], sp.ctypes.data)
            assert f(eng[name], b.ctypes.data, sp.ctypes.data) == 0
            got[name] = (b, _host_live(lib, eng[name], ch, lay["live"]))
        for name in ("unsplit", "split"):
            np.testing.assert_array_equal(got[name][0], got["literal"][0], err_msg="%s bits, superframe %d" % (name, k))
            np.testing.assert_array_equal(got[name][1], got["literal"][1], err_msg="%s state, superframe %d" % (name, k))
        pattern, uv_after, chbuf = _fields(got["literal"][1], lay)
        np.testing.assert_array_equal(chbuf, got["literal"][0])
        cases.add(prev_uv, pattern)
        prev_uv = uv_after
    for e in eng.values():
        lib.emu_destroy(e)
    cases.check()


# ---------------------------------------------------------------- GPU

@pytest.mark.gpu
def test_product_encode_matches_the_literal_order_in_every_case():
    """engine A: the product encode with the lane kernels forced (k_enc_ana
    -> k_enc_quant -> k_enc_harm -> k_enc_tail); engine B: the literal order
    (k_enc_ana_dbg, analysis_upto(6)); bits and live prefixes after every
    superframe"""
    import torch
    from pairphone_amd import MelpeEngine, load_library
    lay = _layout(emu())
    lib = load_library()
    lib.melpe_debug_encode_stage.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream(dev).cuda_stream
    ch = C_GPU
    x = torch.from_numpy(signals(SEED, ch, NSF).reshape(ch, NSF, 540)).to(dev)
    a, b = MelpeEngine(ch), MelpeEngine(ch)
    a.set_ana_waves(1)
    bits = torch.zeros((ch, 11), dtype=torch.uint8, device=dev)
    lo, hi = lay["ana"], lay["ana"] + lay["live"]
    cases = _Cases()
    prev_uv = _fields(a.export_state(1)[:, lo:hi], lay)[1]
    for k in range(NSF):
        xa, xb = x[:, k].contiguous(), x[:, k].contiguous()
        a.encode_dev(bits.data_ptr(), xa.data_ptr(), None, s)
        torch.cuda.synchronize(dev)
        assert a.last_ana_waves() == 1
        assert lib.melpe_debug_encode_stage(b.h, xb.data_ptr(), 6) == 0, lib.melpe_last_error().decode()
        ra, rb = a.export_state(1)[:, lo:hi], b.export_state(1)[:, lo:hi]
        pattern, uv_after, chbuf = _fields(rb, lay)
        np.testing.assert_array_equal(bits.cpu().numpy(), chbuf, err_msg="bits, superframe %d" % k)
        np.testing.assert_array_equal(ra, rb, err_msg="state, superframe %d" % k)
        assert torch.equal(xa, xb), "NPP output, superframe %d" % k
        cases.add(prev_uv, pattern)
        prev_uv = uv_after
    a.close()
    b.close()
    cases.check()
