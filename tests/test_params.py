"""The codec parameters as tensors: the encoder and decoder taps
(melpe_encode_params / melpe_decode_params) and the parse-only decoder
(melpe_parse), word for word against the reference's own melp_par /
quant_par.

The oracle is oracle/_ref/ref_tool: `enc <pcm> <bits> <dump>` writes per
superframe melp_par[3] (3 x 30 int16), quant_par (30 int16, dump_quant's
order), the 11 bytes + a pad byte and the NPP output (1,332 bytes);
`dec <bits> <pcm> <dump>` writes melp_par[3] after every melpe_s (180 bytes).

Bitstreams come in three kinds: 0 = valid (the reference's encoding of the
csrc/synth.h signal), 1 = the same with 1-7 random bit flips in half of the
superframes, 2 = random bytes with byte 10 masked to its bit 0 (81 bits).

CPU: the host build of parse_superframe (emu_parse) on 12 channels, four of
each kind, and the existing host decoders after the syn_frame_begin split.
GPU: 200 channels (three full waves and a partial one).
"""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, REF_TOOL
from test_encode import emu, signals
from test_decode import decode_all, emu_decoder, fuzz_bits, gold, sha

SEED = 21           # synth seed of the valid streams
NSF = 24            # superframes of the parse / decode cases
ENC_NSF = 12        # superframes of the encoder tap cases
C_GPU = 200
ENC_DUMP = 1332     # bytes per superframe of `ref_tool enc`'s dump
SENTINEL = 0x5A5A

# rows on both sides of every wave boundary, the last row, all three kinds
PARSE_SAMPLE = [0, 1, 2, 31, 32, 33, 62, 63, 64, 65, 100, 101, 102, 126, 127, 128, 129, 160,
                191, 192, 193, 197, 198, 199]
ENC_SAMPLE = [0, 1, 2, 31, 62, 63, 64, 65, 100, 126, 127, 128, 129, 160, 190, 191, 192, 197, 198, 199]


def ref(*args):
    subprocess.run([REF_TOOL] + [str(a) for a in args], check=True)


def make_bits(tmp, kinds, nsf):
    """[C, nsf * 11] bitstreams, channel c of kind kinds[c]; the valid
    streams (kinds 0 and 1) are the reference's encoding of synth channel c"""
    C = len(kinds)
    path = os.path.join(str(tmp), "valid.bits")
    ref("encgen", SEED, 0, C, nsf, path)
    bits = np.fromfile(path, np.uint8).reshape(C, nsf * 11).copy()
    rng = np.random.Generator(np.random.PCG64(4242))
    for c, kind in enumerate(kinds):
        if kind == 1:
            for k in rng.permutation(nsf)[: nsf // 2]:
                for b in rng.integers(0, 81, rng.integers(1, 8)):
                    bits[c, k * 11 + b // 8] ^= 1 << (b % 8)
        elif kind == 2:
            bits[c] = rng.integers(0, 256, nsf * 11, dtype=np.uint8)
            bits[c, 10::11] &= 1
    return bits


def ref_dec_par(tmp, bits, channels, nsf):
    """{c: [nsf, 90]}: melp_par[3] after every melpe_s of the reference"""
    out = {}
    for c in channels:
        p = os.path.join(str(tmp), "d%d" % c)
        bits[c].tofile(p + ".bits")
        ref("dec", p + ".bits", p + ".pcm", p + ".dump")
        out[c] = np.fromfile(p + ".dump", np.int16).reshape(nsf, 90)
    return out


def uv_patterns(rows):
    """the voiced/unvoiced patterns (uv_flag of the three frames, word 19)
    among [..., 90] superframe rows"""
    r = rows.reshape(-1, 3, 30)[:, :, 19]
    return set(map(tuple, (r != 0).astype(int).tolist()))


# ---------------------------------------------------------------- CPU


def test_parse_hostemu_matches_reference_dumps(tmp_path, ref_tool):
    C = 12
    kinds = [0] * 4 + [1] * 4 + [2] * 4
    bits = make_bits(tmp_path, kinds, NSF)
    want = ref_dec_par(tmp_path, bits, range(C), NSF)
    # the inputs reach every voiced/unvoiced pattern of the three frames
    seen = uv_patterns(np.stack([want[c] for c in range(8)]))
    assert len(seen) == 8, "uv_flag patterns among the valid and bit-flipped channels: %s" % sorted(seen)
    lib = emu()
    lib.emu_parse.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    e = lib.emu_create(C)
    for k in range(NSF):
        b = np.ascontiguousarray(bits[:, k * 11:(k + 1) * 11])
        par = np.zeros((C, 90), np.int16)
        assert lib.emu_parse(e, par.ctypes.data, b.ctypes.data) == 0, \
            "parse_superframe wrote past the excitation side of the record"
        for c in range(C):
            np.testing.assert_array_equal(par[c], want[c][k], err_msg="channel %d (kind %d) superframe %d"
                                          % (c, kinds[c], k))
    lib.emu_destroy(e)


@pytest.mark.parametrize("fn", ["emu_decode", "emu_decode2"])
def test_host_decoders_keep_fuzz_hashes_after_head_split(fn):
    """syn_frame_begin now calls the parameter head as a function of its own
    (decoder.h syn_par_head): both host decoders still give the committed
    dec_fuzz.json hashes on the first 8 channels, and a parse-capable build
    exports emu_parse next to them"""
    g = gold("dec_fuzz.json")
    ch, nsf = 8, g["superframes"]
    bits = fuzz_bits(g["seed"], g["channels"], nsf)[:ch]
    lib, e, dec = emu_decoder(ch, fn)
    assert hasattr(lib, "emu_parse")
    pcm = decode_all(dec, bits, nsf)
    lib.emu_destroy(e)
    for c in range(ch):
        assert sha(pcm[c]) == g["pcm_sha256"][c], "channel %d" % c


def test_params_field_slices_and_physical_units():
    import torch
    from pairphone_amd import params
    cover = np.zeros(30, int)
    for s in params.PAR_FIELDS.values():
        cover[s] += 1
    assert (cover == 1).all()
    cover = np.zeros(30, int)
    for s in params.QPAR_FIELDS.values():
        cover[s] += 1
    assert (cover == 1).all()
    row = np.zeros((2, 3, 30), np.int16)
    row[..., params.PITCH] = 6400           # 50 samples
    row[..., params.LSF] = 8192             # a quarter of 4000 Hz
    row[..., params.GAIN] = [2560, -256]    # 10 dB, -1 dB
    row[..., params.JITTER] = 8192
    row[..., params.BPVC] = 16384
    row[0, :, params.UV_FLAG] = 1
    row[..., params.FS_MAG] = 8192
    p = params.to_physical(torch.from_numpy(row))
    assert p["pitch_hz"].shape == (2, 3) and p["lsf_hz"].shape == (2, 3, 10)
    assert torch.all(p["pitch_hz"] == 160.0) and torch.all(p["lsf_hz"] == 1000.0)
    assert p["gain_db"][0, 0].tolist() == [10.0, -1.0]
    assert torch.all(p["jitter"] == 0.25) and torch.all(p["bpvc"] == 1.0) and torch.all(p["fs_mag"] == 1.0)
    assert p["uv_flag"].tolist() == [[True] * 3, [False] * 3]
    with pytest.raises(ValueError):
        params.to_physical(torch.zeros((3, 29), dtype=torch.int16))


# ---------------------------------------------------------------- GPU


@pytest.fixture(scope="module")
def enc_case(tmp_path_factory):
    """200 channels x 12 superframes of signal and, for the sampled channels,
    the reference encoder's dumps: par [12, 90], qpar [12, 30], bits [12, 11]"""
    tmp = str(tmp_path_factory.mktemp("enc_par"))
    x = signals(SEED, C_GPU, ENC_NSF)
    want = {}
    for c in ENC_SAMPLE:
        p = os.path.join(tmp, "e%d" % c)
        x[c].tofile(p + ".pcm")
        ref("enc", p + ".pcm", p + ".bits", p + ".dump")
        d = np.fromfile(p + ".dump", np.uint8).reshape(ENC_NSF, ENC_DUMP)
        want[c] = (d[:, :180].copy().view(np.int16), d[:, 180:240].copy().view(np.int16), d[:, 240:251].copy())
    return x, want


def check_enc_rows(want, k, par, qpar, bits):
    for c in ENC_SAMPLE:
        wp, wq, wb = want[c]
        np.testing.assert_array_equal(bits[c], wb[k], err_msg="bits: channel %d superframe %d" % (c, k))
        np.testing.assert_array_equal(par[c].reshape(90), wp[k], err_msg="par: channel %d superframe %d" % (c, k))
        np.testing.assert_array_equal(qpar[c], wq[k], err_msg="qpar: channel %d superframe %d" % (c, k))


@pytest.mark.gpu
@pytest.mark.parametrize("waves", [1, 4])
def test_encode_params_gpu_match_reference_dumps(enc_case, waves):
    from pairphone_amd import MelpeEngine
    x, want = enc_case
    eng = MelpeEngine(C_GPU)
    eng.set_lane_order(True)
    eng.set_ana_waves(waves)
    for k in range(ENC_NSF):
        bits = eng.encode(np.ascontiguousarray(x[:, k * 540:(k + 1) * 540]))
        assert eng.last_ana_waves() == waves
        par, qpar = eng.encode_params()
        assert par.shape == (C_GPU, 3, 30) and qpar.shape == (C_GPU, 30)
        check_enc_rows(want, k, par, qpar, bits)
    eng.close()


@pytest.mark.gpu
def test_encode_params_gpu_after_pipelined_encode(enc_case):
    """the tap enqueued after every melpe_encode_pipe_dev (the analysis of
    superframe k beside the NPP of k + 1 on a side stream), one sync at the
    end"""
    import torch
    from pairphone_amd import MelpeEngine
    x, want = enc_case
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream(dev).cuda_stream
    d_x = torch.from_numpy(np.ascontiguousarray(
        x.reshape(C_GPU, ENC_NSF, 540).transpose(1, 0, 2))).to(dev)
    d_bits = torch.zeros((ENC_NSF, C_GPU, 11), dtype=torch.uint8, device=dev)
    d_par = torch.zeros((ENC_NSF, C_GPU, 3, 30), dtype=torch.int16, device=dev)
    d_qpar = torch.zeros((ENC_NSF, C_GPU, 30), dtype=torch.int16, device=dev)
    eng = MelpeEngine(C_GPU)
    eng.encode_npp_dev(d_x[0].data_ptr(), None, s)
    for k in range(ENC_NSF):
        eng.encode_pipe_dev(d_bits[k].data_ptr(), d_x[k].data_ptr(),
                            d_x[k + 1].data_ptr() if k + 1 < ENC_NSF else None, stream=s)
        eng.encode_params_dev(d_par[k].data_ptr(), d_qpar[k].data_ptr(), None, s)
    torch.cuda.synchronize(dev)
    eng.close()
    bits, par, qpar = d_bits.cpu().numpy(), d_par.cpu().numpy(), d_qpar.cpu().numpy()
    for k in range(ENC_NSF):
        check_enc_rows(want, k, par[k], qpar[k], bits[k])


@pytest.mark.gpu
def test_encode_params_gpu_mask_keeps_inactive_rows(enc_case):
    import torch
    from pairphone_amd import MelpeEngine
    x, _ = enc_case
    eng = MelpeEngine(C_GPU)
    eng.encode(np.ascontiguousarray(x[:, :540]))
    full_par, full_q = eng.encode_params()
    m = (np.random.default_rng(5).random(C_GPU) < 0.5).astype(np.uint8)
    m[[0, 63, 128, 199]] = 1
    m[[1, 64, 127, 198]] = 0
    # host form: caller's rows
    par = np.full((C_GPU, 3, 30), SENTINEL, np.int16)
    qpar = np.full((C_GPU, 30), SENTINEL, np.int16)
    eng.encode_params(m, par, qpar)
    # device form, and without the indices
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream(dev).cuda_stream
    d_m = torch.from_numpy(m).to(dev)
    d_par = torch.full((C_GPU, 3, 30), SENTINEL, dtype=torch.int16, device=dev)
    d_qpar = torch.full((C_GPU, 30), SENTINEL, dtype=torch.int16, device=dev)
    d_par2 = torch.full((C_GPU, 3, 30), SENTINEL, dtype=torch.int16, device=dev)
    eng.encode_params_dev(d_par.data_ptr(), d_qpar.data_ptr(), d_m.data_ptr(), s)
    eng.encode_params_dev(d_par2.data_ptr(), None, d_m.data_ptr(), s)
    torch.cuda.synchronize(dev)
    eng.close()
    on = m != 0
    for p, q in ((par, qpar), (d_par.cpu().numpy(), d_qpar.cpu().numpy()), (d_par2.cpu().numpy(), None)):
        np.testing.assert_array_equal(p[on], full_par[on])
        assert (p[~on] == SENTINEL).all()
        if q is not None:
            np.testing.assert_array_equal(q[on], full_q[on])
            assert (q[~on] == SENTINEL).all()


@pytest.fixture(scope="module")
def dec_case(tmp_path_factory):
    """200 channels x 24 superframes, channel c of kind c mod 3, and the
    reference decoder's melp_par dumps of the sampled channels"""
    tmp = tmp_path_factory.mktemp("dec_par")
    bits = make_bits(tmp, [c % 3 for c in range(C_GPU)], NSF)
    return bits, ref_dec_par(tmp, bits, PARSE_SAMPLE, NSF)


_runs = {}


def parse_run(bits):
    """[NSF, C, 90] from melpe_parse_dev (one engine, computed once)"""
    if "parse" not in _runs:
        import torch
        from pairphone_amd import MelpeEngine
        dev = torch.device("cuda", 0)
        s = torch.cuda.current_stream(dev).cuda_stream
        d_bits = torch.from_numpy(np.ascontiguousarray(
            bits.reshape(C_GPU, NSF, 11).transpose(1, 0, 2))).to(dev)
        d_par = torch.full((NSF, C_GPU, 90), SENTINEL, dtype=torch.int16, device=dev)
        eng = MelpeEngine(C_GPU)
        for k in range(NSF):
            eng.parse_dev(d_par[k].data_ptr(), d_bits[k].data_ptr(), None, s)
        torch.cuda.synchronize(dev)
        eng.close()
        _runs["parse"] = d_par.cpu().numpy()
    return _runs["parse"]


def decode_tap_run(bits, waves):
    """[NSF, C, 90] from melpe_decode_params_dev after melpe_decode_dev"""
    if ("dec", waves) not in _runs:
        import torch
        from pairphone_amd import MelpeEngine
        dev = torch.device("cuda", 0)
        s = torch.cuda.current_stream(dev).cuda_stream
        d_bits = torch.from_numpy(np.ascontiguousarray(
            bits.reshape(C_GPU, NSF, 11).transpose(1, 0, 2))).to(dev)
        d_par = torch.full((NSF, C_GPU, 90), SENTINEL, dtype=torch.int16, device=dev)
        d_sp = torch.zeros((C_GPU, 540), dtype=torch.int16, device=dev)
        eng = MelpeEngine(C_GPU)
        eng.set_dec_waves(waves)
        for k in range(NSF):
            eng.decode_dev(d_sp.data_ptr(), d_bits[k].data_ptr(), None, s)
            eng.decode_params_dev(d_par[k].data_ptr(), None, s)
        torch.cuda.synchronize(dev)
        eng.close()
        _runs[("dec", waves)] = d_par.cpu().numpy()
    return _runs[("dec", waves)]


def check_sampled(got, want):
    for c in PARSE_SAMPLE:
        for k in range(NSF):
            np.testing.assert_array_equal(got[k, c], want[c][k], err_msg="channel %d (kind %d) superframe %d"
                                          % (c, c % 3, k))


@pytest.mark.gpu
@pytest.mark.parametrize("waves", [1, 2])
def test_parse_gpu_matches_reference_dumps_and_full_decoder(dec_case, waves):
    bits, want = dec_case
    got = parse_run(bits)
    check_sampled(got, want)
    # the project against itself, every lane: the full decoder's melp_par
    full = decode_tap_run(bits, waves)
    bad = sorted(set(np.argwhere(got != full)[:, 1].tolist()))
    assert not bad, "parse and decode disagree on %d channels, first %s" % (len(bad), bad[:8])


@pytest.mark.gpu
@pytest.mark.parametrize("waves", [1, 2])
def test_decode_params_gpu_match_reference_dumps(dec_case, waves):
    bits, want = dec_case
    check_sampled(decode_tap_run(bits, waves), want)


@pytest.mark.gpu
def test_parse_gpu_ragged_mask(dec_case):
    """random per-superframe masks, a cursor per channel: every channel's
    parsed rows are the unmasked run's, rows of inactive channels untouched"""
    from pairphone_amd import MelpeEngine
    bits, _ = dec_case
    full = parse_run(bits)
    rng = np.random.default_rng(11)
    act = rng.random((NSF + 16, C_GPU)) < 0.6
    eng = MelpeEngine(C_GPU)
    pos = np.zeros(C_GPU, int)
    for k in range(act.shape[0]):
        m = (act[k] & (pos < NSF)).astype(np.uint8)
        b = np.zeros((C_GPU, 11), np.uint8)
        for c in np.flatnonzero(m):
            b[c] = bits[c, pos[c] * 11:(pos[c] + 1) * 11]
        par = np.full((C_GPU, 3, 30), SENTINEL, np.int16)
        eng.parse(b, m, par)
        par = par.reshape(C_GPU, 90)
        off = m == 0
        assert (par[off] == SENTINEL).all(), "step %d: a row of an inactive channel was written" % k
        for c in np.flatnonzero(m):
            np.testing.assert_array_equal(par[c], full[pos[c], c], err_msg="channel %d superframe %d" % (c, pos[c]))
            pos[c] += 1
    eng.close()
    assert (pos > NSF // 3).all()


@pytest.mark.gpu
def test_parse_host_form_matches_device_form(dec_case):
    from pairphone_amd import MelpeEngine
    bits, _ = dec_case
    full = parse_run(bits)
    eng = MelpeEngine(C_GPU)
    for k in range(3):
        par = eng.parse(bits[:, k * 11:(k + 1) * 11])
        np.testing.assert_array_equal(par.reshape(C_GPU, 90), full[k])
    eng.close()
