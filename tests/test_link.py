"""The link's packet layer (MakeCtr / ProcessCtr, crp.c:789-982) and its
Golay(24,12) code against the reference.

Oracle = tests/golden/link.json, made by tests/golden/make_link_golden.py from
the reference's own crp.c and fec/fec_golay2412.c (harness
tests/golden/ref_link.c): 72 channels x 64 packets, twelve scenarios by
c % 12 (clean loopback, fast and slow sync, drops and repeats, bit errors,
uncorrectable words, inverted line, far-end reset, the two counter exits, the
late voice fallback, the call-time limit), a long all-voice run of 400
channels x 2,000 packets, plus the Golay code over all 2^24 received words as
256 digests.  Packets, returns and records are compared as
raw bytes, floats bit for bit.

CPU: the host build of link.h / golay.h (hostemu) against the fixture; the
argument errors of the C ABI; Link.setup / Link.fields.
GPU: the kernels through the C ABI against the fixture, in one call, in calls
of K = 1 and of K = 5, under an active mask, at C = K = 1, and in the chain
melpe_tx_dev -> link tx -> link rx -> melpe_decode_dev.
"""
import ctypes
import hashlib
import json
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, GOLDEN

sys.path.insert(0, GOLDEN)
from make_link_golden import (inputs, impair, unpack, voice_inputs, sha, RECORD, C, K, REKEY, STAGE)  # noqa: E402

EMU = os.path.join(ROOT, "build", "libmelpe_hostemu.so")
P = ctypes.c_void_p
_cache = {}


def golden():
    """the fixture, decoded once and shared (callers copy what they change)"""
    if not _cache:
        g = json.load(open(os.path.join(GOLDEN, "link.json")))
        assert (g["channels"], g["packets"]) == (C, K)
        tx0, rx0, pkts, voiced = inputs(g["seed"])
        txp = unpack(g["tx_pkts"], np.uint8, (C, K, 11))
        crafted = {int(c): unpack(p, np.uint8, (K, 11)) for c, p in g["crafted"].items()}
        _cache.update(
            g=g, tx0=tx0, rx0=rx0, pkts=pkts, voiced=voiced, txp=txp,
            txret=unpack(g["tx_ret"], "<i4", (C, K)), tx1=unpack(g["tx_state"], np.uint8, (C, 256)),
            rxin=np.stack([impair(c, txp[c], crafted, g["seed"]) for c in range(C)]),
            rxret=unpack(g["rx_ret"], "<i4", (C, K)), rx1=unpack(g["rx_state"], np.uint8, (C, 256)))
    return _cache


def raw(recs):
    return np.ascontiguousarray(recs).view(np.uint8).reshape(len(recs), 256).copy()


def sha_rows(p):
    return [hashlib.sha256(np.ascontiguousarray(r).tobytes()).hexdigest() for r in p]


def emu():
    return ctypes.CDLL(EMU)


def emu_tx(state, pkts, voiced, active=None):
    state, pkts = state.copy(), pkts.copy()
    n, k = pkts.shape[:2]
    ret = np.full((n, k), 12345, np.int32)
    v = None if voiced is None else P(np.ascontiguousarray(voiced).ctypes.data)
    a = None if active is None else P(active.ctypes.data)
    assert emu().emu_link_tx(P(state.ctypes.data), P(pkts.ctypes.data), v, P(ret.ctypes.data), n, k, a) == 0
    return state, pkts, ret


def emu_rx(state, pkts, active=None):
    state, pkts = state.copy(), pkts.copy()
    n, k = pkts.shape[:2]
    ret = np.full((n, k), 12345, np.int32)
    voice = np.full((n, k), 77, np.uint8)
    a = None if active is None else P(active.ctypes.data)
    assert emu().emu_link_rx(P(state.ctypes.data), P(pkts.ctypes.data), P(ret.ctypes.data),
                             P(voice.ctypes.data), n, k, a) == 0
    return state, pkts, ret, voice


def check_tx(G, state, pkts, ret):
    assert np.array_equal(ret, G["txret"])
    assert np.array_equal(pkts, G["txp"])
    assert np.array_equal(state, G["tx1"])


def check_rx(G, state, pkts, ret, voice):
    assert np.array_equal(ret, G["rxret"])
    assert sha_rows(pkts) == G["g"]["rx_pkts_sha256"]
    assert np.array_equal(state, G["rx1"])
    assert np.array_equal(voice, (G["rxret"] == -3).astype(np.uint8))


# ---------------------------------------------------------------- CPU ----

def test_fixture_covers_every_scenario():
    G = golden()
    assert len(G["g"]["scenarios"]) == 12 and all(n >= 1 for n in G["g"]["scenarios"].values())
    assert (G["txret"] == REKEY).any() and (G["rxret"] == -3).any() and (G["rxret"] == 8).any()


def test_hostemu_tx_matches_reference():
    G = golden()
    check_tx(G, *emu_tx(raw(G["tx0"]), G["pkts"], G["voiced"]))


def test_hostemu_rx_matches_reference():
    G = golden()
    check_rx(G, *emu_rx(raw(G["rx0"]), G["rxin"]))


def test_hostemu_statuses_and_mask():
    G = golden()
    st = G["tx0"].copy()
    st["step"][0], st["step"][1] = 5, 6      # below the work stage / control only
    active = np.ones(C, np.uint8)
    active[2] = 0
    s1, p1, r1 = emu_tx(raw(st), G["pkts"], G["voiced"], active)
    assert (r1[0] == STAGE).all() and np.array_equal(p1[0], G["pkts"][0]) and np.array_equal(s1[0], raw(st)[0])
    assert (r1[1] == -3).all() and p1[1][:, 10].max() == 0      # every packet a control block
    assert (r1[2] == 12345).all() and np.array_equal(p1[2], G["pkts"][2]) and np.array_equal(s1[2], raw(st)[2])
    assert np.array_equal(r1[3:], G["txret"][3:]) and np.array_equal(s1[3:], G["tx1"][3:])
    st = G["rx0"].copy()
    st["step"][0] = 4
    s2, p2, r2, v2 = emu_rx(raw(st), G["rxin"], active)
    assert (r2[0] == STAGE).all() and not v2[0].any() and np.array_equal(p2[0], G["rxin"][0])
    assert np.array_equal(s2[0], raw(st)[0])
    assert (r2[2] == 12345).all() and (v2[2] == 77).all() and np.array_equal(s2[2], raw(st)[2])
    assert np.array_equal(r2[3:], G["rxret"][3:]) and np.array_equal(s2[3:], G["rx1"][3:])


def check_voice_run(v0, state, pkts, ret):
    """A long stretch of voice must not look like a far-end reset.  fcrc
    decays by 0.95 and gains 4 - popcount(crc8 ^ header) per packet; on voice
    that byte is pseudo-random (the stale scratch bytes are the previous
    gamma), so the gain has mean 0 and variance 2 and fcrc is stationary with
    sigma = sqrt(2 / (1 - 0.95^2)) = 4.5.  Bounds: the mean over 400 channels
    within 1.0 (over 4 sigma / sqrt(400)), every channel within 30 (over 6
    sigma), the reset level 60 never reached (13 sigma).  Beyond the bounds,
    everything equals the reference's own run byte for byte."""
    g = golden()["g"]["voice_run"]
    rec = state.reshape(-1).view(RECORD)
    assert (rec["step"] == 8).all() and np.array_equal(rec["cnt_out"], v0["cnt_out"])      # never reset
    assert np.array_equal(rec["cnt_in"], v0["cnt_in"] + g["packets"])
    assert abs(float(rec["fcrc"].mean())) < 1.0 and np.abs(rec["fcrc"]).max() < 30.0
    assert (ret == -3).mean() > 0.999       # voice but for the odd packet that decodes as control
    assert sha(state) == g["state_sha256"] and sha(ret) == g["ret_sha256"] and sha(pkts) == g["pkts_sha256"]


def test_hostemu_long_voice_run_never_resets():
    g = golden()["g"]["voice_run"]
    v0, vp = voice_inputs(g["seed"], g["channels"], g["packets"])
    state, pkts, ret, _ = emu_rx(raw(v0), vp)
    check_voice_run(v0, state, pkts, ret)


def test_hostemu_golay_matches_reference_sweep():
    g = golden()["g"]
    enc = np.zeros(4096, np.uint32)
    dig = np.zeros(256, np.uint64)
    lib = emu()
    assert lib.emu_golay_sweep(P(enc.ctypes.data), P(dig.ctypes.data)) == 0
    assert hashlib.sha256(enc.astype("<u4").tobytes()).hexdigest() == g["golay_enc_sha256"]
    assert ["%016x" % v for v in dig] == g["golay_digest"]
    # the single-symbol entry points, and the code's guarantee on top of parity
    # with the reference: up to three errors anywhere are corrected
    lib.emu_golay_encode.restype = lib.emu_golay_decode.restype = ctypes.c_uint
    for m, e in ((0, 0), (0xABC, 0x800001), (0xFFF, 0x010101), (0x123, 0x7), (0x456, 0xE00000)):
        assert lib.emu_golay_encode(m) == enc[m]
        assert lib.emu_golay_decode(int(enc[m]) ^ e) == m


def test_abi_rejects_bad_arguments(engine_lib):
    lib = engine_lib
    assert lib.melpe_link_state_bytes() == 256 == RECORD.itemsize
    ok = P(4096)
    for tx in (True, False):
        def call(state, pkts, ret, c, k):
            if tx:
                return lib.melpe_link_tx_dev(state, pkts, None, ret, c, k, None, None)
            return lib.melpe_link_rx_dev(state, pkts, ret, None, c, k, None, None)
        for c, k in ((0, 1), (1, 0), (-1, 1), (1, -1)):
            assert call(ok, ok, ok, c, k) < 0
            assert b"positive" in lib.melpe_last_error()
        assert call(P(4098), ok, ok, 1, 1) < 0
        assert b"aligned" in lib.melpe_last_error()
        assert call(None, ok, ok, 1, 1) < 0
        assert b"null state" in lib.melpe_last_error()
        assert call(ok, None, ok, 1, 1) < 0
        assert b"null packet" in lib.melpe_last_error()
    assert lib.melpe_link_tx_host(None, ok, None, ok, 1, 1, None) < 0
    assert lib.melpe_link_rx_host(ok, None, ok, None, 1, 1, None) < 0
    assert lib.melpe_golay_sweep_dev(None, ok, None) < 0


def test_link_setup_fields_round_trip(engine_lib):
    from pairphone_amd import Link, LINK_RECORD
    assert LINK_RECORD == RECORD
    G = golden()
    t = G["tx0"]
    ln = Link(C).setup(t["cnt_out"], t["cnt_in"], t["step"], t["finv"], t["skey"], t["akey"])
    assert ln.state.shape == (C, 256) and ln.state.dtype == np.uint8
    assert np.array_equal(ln.state, raw(t))
    f = ln.fields()
    for name in ("cnt_out", "cnt_in", "step", "finv", "fcrc", "skey", "akey", "fdata"):
        assert np.array_equal(f[name], t[name]), name
    # scalars broadcast
    f = Link(3).setup(7, 0, 5, -1.0, np.zeros((3, 32), np.uint8), np.ones((3, 32), np.uint8)).fields()
    assert f["cnt_out"].tolist() == [7, 7, 7] and f["step"].tolist() == [5, 5, 5] and (f["finv"] == -1).all()


# ---------------------------------------------------------------- GPU ----

def _link(state):
    from pairphone_amd import Link
    ln = Link(len(state))
    ln.state[:] = state
    return ln


@pytest.mark.gpu
def test_gpu_golay_sweep_matches_reference():
    import torch
    from pairphone_amd import load_library
    g = golden()["g"]
    enc = torch.zeros(4096, dtype=torch.int32, device="cuda:0")
    dig = torch.zeros(256, dtype=torch.int64, device="cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    assert load_library().melpe_golay_sweep_dev(enc.data_ptr(), dig.data_ptr(), s) == 0
    assert hashlib.sha256(enc.cpu().numpy().astype("<u4").tobytes()).hexdigest() == g["golay_enc_sha256"]
    assert ["%016x" % v for v in dig.cpu().numpy().view(np.uint64)] == g["golay_digest"]


@pytest.mark.gpu
def test_gpu_tx_rx_match_reference():
    G = golden()
    t = _link(raw(G["tx0"]))
    p, r = t.tx(G["pkts"], G["voiced"])
    check_tx(G, t.state, p, r)
    x = _link(raw(G["rx0"]))
    p, r, v = x.rx(G["rxin"])
    check_rx(G, x.state, p, r, v)


@pytest.mark.gpu
def test_gpu_long_voice_run_never_resets():
    g = golden()["g"]["voice_run"]
    v0, vp = voice_inputs(g["seed"], g["channels"], g["packets"])
    x = _link(raw(v0))
    pkts, ret, _ = x.rx(vp)
    check_voice_run(v0, x.state, pkts, ret)


@pytest.mark.gpu
@pytest.mark.parametrize("step", [1, 5])
def test_gpu_split_calls_carry_the_state(step):
    """the same packets in calls of `step` packets (plus the remainder): the
    counters, fcrc and soft bits carry through the records, and the tiles end
    at other places"""
    G = golden()
    t, x = _link(raw(G["tx0"])), _link(raw(G["rx0"]))
    tp, tr, xp, xr, xv = [], [], [], [], []
    for k in range(0, K, step):
        p, r = t.tx(G["pkts"][:, k:k + step], G["voiced"][:, k:k + step])
        tp.append(p), tr.append(r)
        p, r, v = x.rx(G["rxin"][:, k:k + step])
        xp.append(p), xr.append(r), xv.append(v)
    check_tx(G, t.state, np.concatenate(tp, 1), np.concatenate(tr, 1))
    check_rx(G, x.state, np.concatenate(xp, 1), np.concatenate(xr, 1), np.concatenate(xv, 1))


@pytest.mark.gpu
def test_gpu_active_mask_keeps_masked_channels():
    import torch
    from pairphone_amd import load_library
    lib = load_library()
    G = golden()
    active = np.ones(C, np.uint8)
    active[[0, 1, 5, 6, 7, 31, 63, 64, 71]] = 0
    off = active == 0
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    d_act = torch.from_numpy(active).to(dev)
    # TX
    st0 = raw(G["tx0"])
    d_st, d_p = torch.from_numpy(st0).to(dev), torch.from_numpy(G["pkts"].copy()).to(dev)
    d_v = torch.from_numpy(G["voiced"].copy()).to(dev)
    d_r = torch.full((C, K), 12345, dtype=torch.int32, device=dev)
    assert lib.melpe_link_tx_dev(d_st.data_ptr(), d_p.data_ptr(), d_v.data_ptr(), d_r.data_ptr(), C, K,
                                 d_act.data_ptr(), s) == 0
    st, p, r = d_st.cpu().numpy(), d_p.cpu().numpy(), d_r.cpu().numpy()
    assert np.array_equal(st[off], st0[off]) and np.array_equal(p[off], G["pkts"][off]) and (r[off] == 12345).all()
    assert np.array_equal(st[~off], G["tx1"][~off]) and np.array_equal(p[~off], G["txp"][~off])
    assert np.array_equal(r[~off], G["txret"][~off])
    # RX
    st0 = raw(G["rx0"])
    d_st, d_p = torch.from_numpy(st0).to(dev), torch.from_numpy(G["rxin"].copy()).to(dev)
    d_r = torch.full((C, K), 12345, dtype=torch.int32, device=dev)
    d_vo = torch.full((C, K), 77, dtype=torch.uint8, device=dev)
    assert lib.melpe_link_rx_dev(d_st.data_ptr(), d_p.data_ptr(), d_r.data_ptr(), d_vo.data_ptr(), C, K,
                                 d_act.data_ptr(), s) == 0
    st, p, r, vo = d_st.cpu().numpy(), d_p.cpu().numpy(), d_r.cpu().numpy(), d_vo.cpu().numpy()
    assert np.array_equal(st[off], st0[off]) and np.array_equal(p[off], G["rxin"][off])
    assert (r[off] == 12345).all() and (vo[off] == 77).all()
    assert np.array_equal(st[~off], G["rx1"][~off]) and np.array_equal(r[~off], G["rxret"][~off])
    sha = sha_rows(p)
    assert all(sha[c] == G["g"]["rx_pkts_sha256"][c] for c in range(C) if active[c])
    assert np.array_equal(vo[~off], (G["rxret"][~off] == -3).astype(np.uint8))


@pytest.mark.gpu
def test_gpu_one_channel_one_packet():
    G = golden()
    for c in (0, 3):     # a voiced or silent first packet at step 8; a control packet far from cnt_in
        t = _link(raw(G["tx0"])[c:c + 1])
        p, r = t.tx(G["pkts"][c:c + 1, :1], G["voiced"][c:c + 1, :1])
        es, ep, er = emu_tx(raw(G["tx0"])[c:c + 1], G["pkts"][c:c + 1, :1], G["voiced"][c:c + 1, :1])
        assert np.array_equal(p, ep) and np.array_equal(r, er) and np.array_equal(t.state, es)
        assert np.array_equal(p, G["txp"][c:c + 1, :1]) and np.array_equal(r, G["txret"][c:c + 1, :1])
        x = _link(raw(G["rx0"])[c:c + 1])
        p, r, v = x.rx(G["rxin"][c:c + 1, :1])
        es, ep, er, ev = emu_rx(raw(G["rx0"])[c:c + 1], G["rxin"][c:c + 1, :1])
        assert np.array_equal(p, ep) and np.array_equal(r, er) and np.array_equal(v, ev)
        assert np.array_equal(x.state, es) and np.array_equal(r, G["rxret"][c:c + 1, :1])


@pytest.mark.gpu
def test_gpu_chain_tx_link_rx_decode():
    """melpe_tx_dev -> link tx -> link rx -> melpe_decode_dev on the device:
    128 channels x 6 superframes.  The receiver's `voice` is the sender's
    gate, the bits it hands the decoder are the encoder's where gated, and
    the decoder runs under `voice` with 540 zeros elsewhere (rx.c:356-360)."""
    import torch
    from pairphone_amd import MelpeEngine, Link
    n, nsf = 128, 6
    dev = torch.device("cuda:0")
    rng = np.random.Generator(np.random.PCG64(5))
    skey = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    akey = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    cnt = rng.integers(300, 60000, n).astype(np.uint32)
    far = Link(n).setup(cnt, 0, 8, 1.0, skey, akey)
    # the mirrored record: the receiver's second key halves are the sender's first
    near = Link(n).setup(0, cnt, 8, 1.0, np.roll(skey, 16, 1), np.roll(akey, 16, 1))
    eng, ref = MelpeEngine(n), MelpeEngine(n)
    s = torch.cuda.current_stream().cuda_stream
    eng.synth_seed(11)
    d_far, d_near = torch.from_numpy(far.state).to(dev), torch.from_numpy(near.state).to(dev)
    d_vad = torch.zeros(n * eng.lib.melpe_vad_state_bytes(), dtype=torch.uint8, device=dev)
    assert eng.lib.melpe_vad_reset_dev(d_vad.data_ptr(), n, None, s) == 0
    d_sp = torch.zeros((n, 540), dtype=torch.int16, device=dev)
    d_bits = torch.zeros((n, 11), dtype=torch.uint8, device=dev)
    d_votes = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_gate = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_ret = torch.zeros(n, dtype=torch.int32, device=dev)
    d_voice = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_out = torch.zeros((n, 540), dtype=torch.int16, device=dev)
    d_want = torch.zeros((n, 540), dtype=torch.int16, device=dev)
    gated = 0
    for k in range(nsf):
        eng.synth_dev(d_sp.data_ptr(), 540, s)
        # low noise on every third channel throughout and on a random third of
        # the others, so that the gate closes on some superframes
        quiet = (np.arange(n) % 3 == 0) | (rng.random(n) < 0.3)
        noise = torch.from_numpy(rng.integers(-20, 21, (int(quiet.sum()), 540)).astype(np.int16)).to(dev)
        d_sp[torch.from_numpy(quiet).to(dev)] = noise
        eng.tx_dev(d_vad.data_ptr(), d_bits.data_ptr(), d_sp.data_ptr(), d_votes.data_ptr(),
                   d_gate.data_ptr(), None, s)
        d_pkt = d_bits.clone()
        far.tx_dev(d_far.data_ptr(), d_pkt.data_ptr(), d_gate.data_ptr(), d_ret.data_ptr(), 1, None, s)
        txret = d_ret.cpu().numpy()
        assert np.array_equal(txret, cnt + k + 1)
        near.rx_dev(d_near.data_ptr(), d_pkt.data_ptr(), d_ret.data_ptr(), d_voice.data_ptr(), 1, None, s)
        gate, voice = d_gate.cpu().numpy() != 0, d_voice.cpu().numpy() != 0
        assert np.array_equal(voice, gate)
        assert (d_ret.cpu().numpy()[~gate] == 8).all()      # every control packet fully authenticated
        assert np.array_equal(d_pkt.cpu().numpy()[gate], d_bits.cpu().numpy()[gate])
        d_out.zero_()
        eng.decode_dev(d_out.data_ptr(), d_pkt.data_ptr(), d_voice.data_ptr(), s)
        # a second engine decodes the encoder's own bits under the sender's gate
        d_want.zero_()
        ref.decode_dev(d_want.data_ptr(), d_bits.data_ptr(), d_gate.data_ptr(), s)
        out = d_out.cpu().numpy()
        assert np.array_equal(out, d_want.cpu().numpy())
        assert not out[~gate].any()
        gated += int(gate.sum())
    assert 0 < gated < n * nsf      # the signal exercised both kinds of packet
    assert np.array_equal(d_near.cpu().numpy().view(RECORD)["cnt_in"].ravel(), cnt + nsf)
    eng.close(), ref.close()
