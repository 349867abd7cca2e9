"""The receive loop, line samples to speech in one call (melpe_rx_line_dev:
rx.c:294-361 with the playback buffer empty) against the reference.

Oracle = tests/golden/rxline.json, made by tests/golden/make_rxline_golden.py
from the reference's own Demodulate, ProcessPkt and melpe_s (harness
tests/golden/ref_rxline.c): 72 channels x 24 packet times, twelve scenarios by
c % 12.  The line is regenerated here with the host build of MakeCtr and
Modulate (the generator asserted it equal to the reference's; its SHA-256 is
in the fixture).  Two runs are stored: the main one, 24 launches of 15 calls
with the line arriving in real time (launch l sees avail(l) samples of every
row, so some channels run short and pick up in the next launch), and `full`,
the same 360 calls on the whole row, which does not depend on how the calls
are grouped.  Info rows, counts, bits, voice flags, PCM and every final record
are compared exactly, floats bit for bit.

CPU: the host build of the loop (hostemu emu_rx_line) against the fixture; the
argument errors of the C ABI; RxLine.fields.
GPU: the kernel through the C ABI against the fixture under both decoder
mappings, regrouped launches, one channel, an active mask over sentinel-filled
outputs, the host form, and the chain melpe_tx_dev -> melpe_link_tx_dev ->
melpe_modulate_dev -> melpe_rx_line_dev on the device.
"""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, GOLDEN

sys.path.insert(0, GOLDEN)
import make_rxline_golden as G  # noqa: E402
from make_rxline_golden import C, K, CALLS, STRIDE, INFO, RXREC, RECORD, sha, unpack  # noqa: E402

EMU = os.path.join(ROOT, "build", "libmelpe_hostemu.so")
TABLES = os.path.join(ROOT, "pairphone_amd", "data", "melpe_tables.bin")
P = ctypes.c_void_p
FILL = 0xA5
MAIN = [(CALLS, G.avail(l)) for l in range(K)]
_cache = {}


def golden():
    """the fixture and the regenerated line, made once and shared (callers
    copy what they change)"""
    if not _cache:
        g = json.load(open(os.path.join(GOLDEN, "rxline.json")))
        assert (g["channels"], g["packets"], g["calls"], g["stride"]) == (C, K, CALLS, STRIDE)
        tx0, rx0, pkts, voiced, active = G.inputs(g["seed"])
        _, line = G.clean_line(g["seed"])
        assert sha(line) == g["line_sha256"]
        rows = np.stack([G.impair(c, line[c], g["seed"]) for c in range(C)])
        assert sha(rows) == g["rows_sha256"]
        mb = g["max_blocks"]
        _cache.update(g=g, rx0=rx0, active=active, rows=rows, pos0=np.array([G.pos0(c) for c in range(C)], np.int32),
                      info=unpack(g["info"], INFO, (C, mb)), counts=unpack(g["counts"], np.uint8, (K, C)),
                      made=unpack(g["made"], np.uint8, (K, C)), pos=unpack(g["pos"], "<i4", (C,)),
                      data=unpack(g["data"], np.uint8, (C, 12)), link=unpack(g["link"], RECORD, (C,)),
                      rx=unpack(g["rx"], RXREC, (C,)))
    return _cache


def emu():
    lib = ctypes.CDLL(EMU)
    lib.emu_create.restype = P
    lib.emu_create.argtypes = [ctypes.c_int]
    lib.emu_destroy.argtypes = [P]
    lib.emu_rx_line.argtypes = [P] * 4 + [P, ctypes.c_long] + [P] * 7 + [ctypes.c_int, ctypes.c_int, P]
    assert lib.emu_load_tables(TABLES.encode()) == 0
    return lib


class State:
    """the per-channel arrays of a run, as numpy"""

    def __init__(self, link, pos0):
        lib = ctypes.CDLL(EMU)
        n = len(link)
        self.modem = np.zeros((n, lib.emu_modem_state_bytes()), np.uint8)
        lib.emu_modem_reset(P(self.modem.ctypes.data), n)
        self.link = np.ascontiguousarray(link).view(np.uint8).reshape(n, 256).copy()
        self.rx = np.zeros((n, 16), np.uint8)
        self.pos = np.array(pos0, np.int32)
        self.data = np.zeros((n, 12), np.uint8)


def outputs(slots, n):
    return (np.full((slots, n, 540), FILL, np.uint8).repeat(2, axis=2).view(np.int16), np.full((slots, n, 11), FILL, np.uint8),
            np.full((slots, n), FILL, np.uint8), np.full((slots, n, 8), FILL, np.uint8), np.full(n, FILL, np.uint8))


def emu_stepper(n):
    lib = emu()
    e = lib.emu_create(n)

    def step(st, pcm, calls, slots, active):
        sp, bits, voice, info, count = outputs(slots, n)
        a = None if active is None else P(active.ctypes.data)
        assert lib.emu_rx_line(e, P(st.modem.ctypes.data), P(st.link.ctypes.data), P(st.rx.ctypes.data),
                               P(pcm.ctypes.data), pcm.shape[1], P(st.pos.ctypes.data), P(st.data.ctypes.data),
                               P(sp.ctypes.data), P(bits.ctypes.data), P(voice.ctypes.data), P(info.ctypes.data),
                               P(count.ctypes.data), calls, slots, a) == 0
        return sp, bits, voice, info, count
    return step


def host_stepper(eng):
    def step(st, pcm, calls, slots, active):
        sp, bits, voice, info, count = outputs(slots, eng.channels)
        a = None if active is None else P(active.ctypes.data)
        assert eng.lib.melpe_rx_line_host(eng.h, P(st.modem.ctypes.data), P(st.link.ctypes.data),
                                          P(st.rx.ctypes.data), P(pcm.ctypes.data), pcm.shape[1],
                                          P(st.pos.ctypes.data), P(st.data.ctypes.data), P(sp.ctypes.data),
                                          P(bits.ctypes.data), P(voice.ctypes.data), P(info.ctypes.data),
                                          P(count.ctypes.data), calls, slots, a) == 0, eng.lib.melpe_last_error()
        return sp, bits, voice, info, count
    return step


def dev_stepper(eng):
    """melpe_rx_line_dev on torch buffers; the state lives on the device
    between the launches and comes back into `st` after each"""
    import torch
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    d = {}

    def step(st, pcm, calls, slots, active):
        if "modem" not in d:
            for k in ("modem", "link", "rx", "pos", "data"):
                d[k] = torch.from_numpy(getattr(st, k)).to(dev)
        out = [torch.from_numpy(o).to(dev) for o in outputs(slots, eng.channels)]
        d_pcm = torch.from_numpy(pcm).to(dev)
        d_act = None if active is None else torch.from_numpy(active).to(dev)
        eng.rx_line_dev(d["modem"].data_ptr(), d["link"].data_ptr(), d["rx"].data_ptr(), d_pcm.data_ptr(),
                        pcm.shape[1], d["pos"].data_ptr(), d["data"].data_ptr(), out[0].data_ptr(),
                        out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), out[4].data_ptr(), calls, slots,
                        None if d_act is None else d_act.data_ptr(), s)
        for k in ("modem", "link", "rx", "pos", "data"):
            getattr(st, k)[...] = d[k].cpu().numpy()
        return tuple(o.cpu().numpy() for o in out)
    return step


def run(step, st, rows, plan, active=None, slots=None):
    """the launches of `plan` = [(calls, samples of every row present)];
    returns per channel the blocks in order -- (info rows, bits, voice, pcm) --
    and the counts per launch; checks that nothing past a channel's count, and
    nothing of an inactive channel, was written"""
    n = len(rows)
    blocks = [([], [], [], []) for _ in range(n)]
    counts = np.zeros((len(plan), n), np.uint8)
    for l, (calls, avail) in enumerate(plan):
        ns = calls // 15 + 2 if slots is None else slots
        sp, bits, voice, info, count = step(st, np.ascontiguousarray(rows[:, :avail]), calls, ns, active)
        for c in range(n):
            if active is not None and not active[c]:
                assert count[c] == FILL
                count[c] = 0
            k = int(count[c])
            assert k <= ns
            for a in (sp, bits, voice, info):
                assert (a[k:, c].view(np.uint8) == FILL).all(), "wrote past count"
            for j in range(k):
                for dst, a in zip(blocks[c], (info, bits, voice, sp)):
                    dst.append(a[j, c].copy())
        counts[l] = count
    return blocks, counts


def check_main(g, st, blocks, counts, active):
    """everything the fixture's main run stores"""
    on = active != 0
    assert np.array_equal(counts[:, on], g["counts"][:, on])
    for c in np.flatnonzero(on):
        info, bits, voice, pcm = blocks[c]
        want = g["info"][c, :len(info)]
        assert len(info) == g["counts"][:, c].sum()
        assert np.array_equal(np.array(info, np.uint8).reshape(-1, 8), want.view(np.uint8).reshape(-1, 8)), c
        assert sha(np.array(bits, np.uint8)) == g["g"]["bits_sha256"][c], c
        assert sha(np.array(voice, np.uint8)) == g["g"]["voice_sha256"][c], c
        assert sha(np.array(pcm, "<i2")) == g["g"]["pcm_sha256"][c], c
        assert sha(st.modem[c]) == g["g"]["modem_sha256"][c], c
    assert np.array_equal(st.pos[on], g["pos"][on]) and np.array_equal(st.data[on], g["data"][on])
    assert np.array_equal(st.link.reshape(-1).view(RECORD)[on], g["link"][on])
    assert st.rx.reshape(-1).view(RXREC)[on].tobytes() == g["rx"][on].tobytes()


def full_digests(st, blocks, c):
    info, bits, voice, pcm = blocks[c]
    return (G.blocks_digest(np.array(info, np.uint8).view(INFO).reshape(-1), bits, voice, pcm),
            G.final_digest(int(st.pos[c]), st.data[c], st.modem[c], st.link[c], st.rx[c]))


def check_full(g, st, blocks, active):
    for c in np.flatnonzero(active):
        b, f = full_digests(st, blocks, c)
        assert b == g["g"]["full"]["blocks_sha256"][c] and f == g["g"]["full"]["final_sha256"][c], c


def check_masked(g, st, active):
    off = active == 0
    fresh = State(g["rx0"], g["pos0"])
    for k in ("modem", "link", "rx", "pos", "data"):
        assert np.array_equal(getattr(st, k)[off], getattr(fresh, k)[off]), k


# ---------------------------------------------------------------- CPU ----

def test_fixture_covers_every_scenario():
    g = golden()
    sc = g["g"]["scenarios"]
    assert len(sc) == 12
    forced = [n for name, n in sc.items() if "forced" in name]
    # the forced block with align set: the count the reference gave, 0 included
    assert len(forced) == 1 and all(n >= 1 for name, n in sc.items() if "forced" not in name)
    kinds = g["info"]["kind"]
    assert all((kinds == k).any() for k in range(4))
    assert (g["made"] < CALLS).any() and (g["rx"]["fber"] > 0).any() and (g["rx"]["fau"] > 100).any()


def test_hostemu_matches_reference():
    g = golden()
    st = State(g["rx0"], g["pos0"])
    blocks, counts = run(emu_stepper(C), st, g["rows"], MAIN, g["active"])
    check_main(g, st, blocks, counts, g["active"])
    check_masked(g, st, g["active"])


def test_hostemu_unlocked_blocks_leave_the_link_record():
    """the first three launches: no block lag is locked yet (the fixture says
    so), every block is kind 0, and the link records, cnt_in included, are
    untouched while the block count advances"""
    g = golden()
    assert (g["info"]["kind"][g["active"] != 0, :3] == 0).all()
    st = State(g["rx0"], g["pos0"])
    blocks, counts = run(emu_stepper(C), st, g["rows"], MAIN[:3], g["active"])
    assert np.array_equal(counts, g["counts"][:3])
    on = g["active"] != 0
    for c in np.flatnonzero(on):
        info = np.array(blocks[c][0], np.uint8).view(INFO).ravel()
        assert len(info) >= 2 and (info["kind"] == 0).all() and (info["ret"] == G.NOLOCK).all()
    assert np.array_equal(st.link, State(g["rx0"], g["pos0"]).link)
    rx = st.rx.reshape(-1).view(RXREC)
    assert np.array_equal(rx["blocks"][on], counts[:, on].sum(axis=0)) and not rx["fber"].any() and not rx["fau"].any()


@pytest.mark.parametrize("plan", ["one", "7-8"])
def test_hostemu_regrouped_launches(plan):
    """the whole row present: one launch of 360 calls, or launches of 7 and 8
    calls in turn, give the blocks and records of 24 launches of 15"""
    g = golden()
    p = [(K * CALLS, STRIDE)] if plan == "one" else [(7 + (i & 1), STRIDE) for i in range(K * 2)]
    st = State(g["rx0"], g["pos0"])
    blocks, _ = run(emu_stepper(C), st, g["rows"], p, g["active"])
    check_full(g, st, blocks, g["active"])


def test_abi_rejects_bad_arguments(engine_lib):
    lib = engine_lib
    assert lib.melpe_rx_line_state_bytes() == 16 == RXREC.itemsize
    ok, e = P(4096), P(4096)      # never dereferenced: the arguments are refused first

    def call(modem=ok, link=ok, rx=ok, pcm=ok, stride=STRIDE, pos=ok, data=ok, sp=ok, bits=ok, voice=ok, info=ok,
             count=ok, calls=15, slots=3, eng=e, host=False):
        if host:
            return lib.melpe_rx_line_host(eng, modem, link, rx, pcm, stride, pos, data, sp, bits, voice, info, count,
                                          calls, slots, None)
        return lib.melpe_rx_line_dev(eng, modem, link, rx, pcm, stride, pos, data, sp, bits, voice, info, count,
                                     calls, slots, None, None)
    for host in (False, True):
        for kw in (dict(slots=2), dict(calls=30, slots=3), dict(calls=360, slots=25), dict(slots=256)):
            assert call(host=host, **kw) < 0 and b"slots" in lib.melpe_last_error()
        for kw in (dict(calls=0), dict(calls=-1), dict(stride=1079)):
            assert call(host=host, **kw) < 0 and b"positive" in lib.melpe_last_error()
        for name in ("modem", "link", "rx"):
            assert call(host=host, **{name: None}) < 0 and b"null state" in lib.melpe_last_error()
            assert call(host=host, **{name: P(4098)}) < 0 and b"aligned" in lib.melpe_last_error()
        for name in ("pcm", "pos", "data", "sp", "bits", "voice", "info", "count"):
            assert call(host=host, **{name: None}) < 0 and b"null buffer" in lib.melpe_last_error()
        assert call(host=host, eng=None) < 0 and b"null engine" in lib.melpe_last_error()
    assert call(sp=P(4100)) < 0 and b"8-byte" in lib.melpe_last_error()
    assert call(info=P(4098)) < 0 and call(pos=P(4098)) < 0


def test_rxline_fields_round_trip(engine_lib):
    from pairphone_amd import RxLine, RX_LINE_RECORD, RX_LINE_INFO, rx_line_slots
    assert RX_LINE_RECORD == RXREC and RX_LINE_INFO == INFO
    assert [rx_line_slots(n) for n in (1, 15, 29, 30, 360)] == [2, 3, 3, 4, 26]
    g = golden()
    r = RxLine(C)
    fresh = State(g["rx0"], g["pos0"])
    assert np.array_equal(r.modem, fresh.modem)      # the host reset = the host build's
    assert r.rx.shape == (C, 16) and r.link.shape == (C, 256) and r.data.shape == (C, 12)
    f = r.fields()
    assert not f["fber"].any() and not f["blocks"].any()
    r.set_fields(g["rx"])
    assert r.rx.tobytes() == g["rx"].tobytes() and r.fields().tobytes() == g["rx"].tobytes()
    r.link[:] = fresh.link
    assert np.array_equal(r.link_fields()["cnt_in"], g["rx0"]["cnt_in"])


# ---------------------------------------------------------------- GPU ----

@pytest.mark.gpu
@pytest.mark.parametrize("dec_waves", [1, 2])
def test_gpu_matches_reference(dec_waves):
    from pairphone_amd import MelpeEngine
    g = golden()
    eng = MelpeEngine(C)
    eng.set_dec_waves(dec_waves)
    st = State(g["rx0"], g["pos0"])
    blocks, counts = run(dev_stepper(eng), st, g["rows"], MAIN, g["active"])
    check_main(g, st, blocks, counts, g["active"])
    check_masked(g, st, g["active"])
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("plan", ["15", "one", "7-8"])
def test_gpu_regrouped_launches(plan):
    from pairphone_amd import MelpeEngine
    g = golden()
    p = {"15": [(CALLS, STRIDE)] * K, "one": [(K * CALLS, STRIDE)],
         "7-8": [(7 + (i & 1), STRIDE) for i in range(K * 2)]}[plan]
    eng = MelpeEngine(C)
    st = State(g["rx0"], g["pos0"])
    blocks, _ = run(dev_stepper(eng), st, g["rows"], p, g["active"])
    check_full(g, st, blocks, g["active"])
    eng.close()


@pytest.mark.gpu
def test_gpu_one_channel_one_launch():
    from pairphone_amd import MelpeEngine
    g = golden()
    for c in (0, 6):
        eng = MelpeEngine(1)
        st, se = State(g["rx0"][c:c + 1], [0]), State(g["rx0"][c:c + 1], [0])
        # six packet times in one launch, so that locked blocks are among them
        got, gc = run(dev_stepper(eng), st, g["rows"][c:c + 1], [(90, STRIDE)])
        want, wc = run(emu_stepper(1), se, g["rows"][c:c + 1], [(90, STRIDE)])
        assert np.array_equal(gc, wc) and gc.sum() >= 6
        for a, b in zip(got[0], want[0]):
            assert np.array_equal(np.array(a), np.array(b))
        assert (np.array(got[0][0], np.uint8).view(INFO)["kind"] != 0).any()
        for k in ("modem", "link", "rx", "pos", "data"):
            assert np.array_equal(getattr(st, k), getattr(se, k)), k
        eng.close()


@pytest.mark.gpu
def test_gpu_active_mask_keeps_masked_channels():
    """another mask than the fixture's: masked channels keep their records and
    every output row (sentinel fill, checked in run), the others equal the
    host build under the same mask"""
    from pairphone_amd import MelpeEngine
    g = golden()
    active = np.ones(C, np.uint8)
    active[[0, 1, 5, 6, 7, 31, 63, 64, 71]] = 0
    eng = MelpeEngine(C)
    st, se = State(g["rx0"], g["pos0"]), State(g["rx0"], g["pos0"])
    got, gc = run(dev_stepper(eng), st, g["rows"], MAIN[:8], active)
    want, wc = run(emu_stepper(C), se, g["rows"], MAIN[:8], active)
    assert np.array_equal(gc, wc) and not gc[:, active == 0].any() and gc[:, active != 0].all(axis=1).any()
    for c in range(C):
        for a, b in zip(got[c], want[c]):
            assert np.array_equal(np.array(a), np.array(b)), c
    check_masked(g, st, active)
    for k in ("modem", "link", "rx", "pos", "data"):
        assert np.array_equal(getattr(st, k), getattr(se, k)), k
    eng.close()


@pytest.mark.gpu
def test_gpu_host_form_matches_reference():
    from pairphone_amd import MelpeEngine, RxLine
    g = golden()
    eng = MelpeEngine(C)
    st = State(g["rx0"], g["pos0"])
    blocks, counts = run(host_stepper(eng), st, g["rows"], MAIN, g["active"])
    check_main(g, st, blocks, counts, g["active"])
    check_masked(g, st, g["active"])
    eng.close()
    # the Python form of the same call
    eng = MelpeEngine(C)
    r = RxLine(C)
    r.link[:] = State(g["rx0"], g["pos0"]).link
    r.pos[:] = g["pos0"]
    sp, bits, voice, info, count = eng.rx_line(r, g["rows"][:, :MAIN[0][1]], CALLS, active=g["active"], fill=FILL)
    on = g["active"] != 0
    assert np.array_equal(count[on], g["counts"][0][on]) and (count[~on] == FILL).all()
    c = int(np.flatnonzero(on)[0])
    assert info[0, c].tobytes() == g["info"][c, 0].tobytes() and not sp[0, c].any()
    eng.close()


@pytest.mark.gpu
def test_gpu_chain_tx_link_modulate_rx_line():
    """melpe_tx_dev -> melpe_link_tx_dev -> melpe_modulate_dev ->
    melpe_rx_line_dev on the device, 128 channels x 10 superframes: every
    output equals the host build's loop on the same line, no packet excluded,
    and the PCM equals a second engine's melpe_decode_dev of the same (bits,
    voice) sequence."""
    import torch
    from pairphone_amd import MelpeEngine, Link
    n, nsf = 128, 10
    stride = nsf * 3240 + 1080
    dev = torch.device("cuda:0")
    rng = np.random.Generator(np.random.PCG64(9))
    skey = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    akey = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    cnt = rng.integers(300, 60000, n).astype(np.uint32)
    far = Link(n).setup(cnt, 0, 8, 1.0, skey, akey)
    # the mirrored record; a clean modem loop is an inverted channel (finv < 0)
    near = Link(n).setup(0, cnt, 8, -1.0, np.roll(skey, 16, 1), np.roll(akey, 16, 1))
    eng, rxe, ref = MelpeEngine(n), MelpeEngine(n), MelpeEngine(n)
    s = torch.cuda.current_stream().cuda_stream
    lib = eng.lib
    eng.synth_seed(11)
    d_far = torch.from_numpy(far.state).to(dev)
    d_vad = torch.zeros(n * lib.melpe_vad_state_bytes(), dtype=torch.uint8, device=dev)
    assert lib.melpe_vad_reset_dev(d_vad.data_ptr(), n, None, s) == 0
    d_mod = torch.zeros(n * lib.melpe_modem_state_bytes(), dtype=torch.uint8, device=dev)
    assert lib.melpe_modem_reset_dev(d_mod.data_ptr(), n, None, s) == 0
    d_sp = torch.zeros((n, 540), dtype=torch.int16, device=dev)
    d_bits = torch.zeros((n, 11), dtype=torch.uint8, device=dev)
    d_votes = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_gate = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_ret = torch.zeros(n, dtype=torch.int32, device=dev)
    d_pk = torch.zeros((n, 3240), dtype=torch.int16, device=dev)
    d_line = torch.zeros((n, stride), dtype=torch.int16, device=dev)
    for k in range(nsf):
        eng.synth_dev(d_sp.data_ptr(), 540, s)
        quiet = (np.arange(n) % 3 == 0) | (rng.random(n) < 0.3)
        noise = torch.from_numpy(rng.integers(-20, 21, (int(quiet.sum()), 540)).astype(np.int16)).to(dev)
        d_sp[torch.from_numpy(quiet).to(dev)] = noise
        eng.tx_dev(d_vad.data_ptr(), d_bits.data_ptr(), d_sp.data_ptr(), d_votes.data_ptr(), d_gate.data_ptr(), None, s)
        far.tx_dev(d_far.data_ptr(), d_bits.data_ptr(), d_gate.data_ptr(), d_ret.data_ptr(), 1, None, s)
        assert lib.melpe_modulate_dev(d_mod.data_ptr(), d_bits.data_ptr(), d_pk.data_ptr(), n, 1, None, s) == 0
        d_line[:, k * 3240:(k + 1) * 3240] = d_pk
    line = d_line.cpu().numpy()
    plan = [(CALLS, stride)] * nsf
    st, se = State(near.fields(), np.zeros(n, np.int32)), State(near.fields(), np.zeros(n, np.int32))
    got, gc = run(dev_stepper(rxe), st, line, plan)
    want, wc = run(emu_stepper(n), se, line, plan)
    assert np.array_equal(gc, wc)
    for k in ("modem", "link", "rx", "pos", "data"):
        assert np.array_equal(getattr(st, k), getattr(se, k)), k
    kinds = []
    d_b = torch.zeros((n, 11), dtype=torch.uint8, device=dev)
    d_v = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_want = torch.zeros((n, 540), dtype=torch.int16, device=dev)
    for c in range(n):
        for a, b in zip(got[c], want[c]):
            assert np.array_equal(np.array(a), np.array(b)), c
        kinds.append(np.array(got[c][0], np.uint8).view(INFO)["kind"].ravel())
    # a second engine decodes the same (bits, voice) sequence, block by block
    for j in range(max(len(k) for k in kinds)):
        has = np.array([len(kinds[c]) > j for c in range(n)])
        bits = np.stack([got[c][1][j] if has[c] else np.zeros(11, np.uint8) for c in range(n)])
        voice = np.array([got[c][2][j] if has[c] else 0 for c in range(n)], np.uint8)
        d_b.copy_(torch.from_numpy(bits))
        d_v.copy_(torch.from_numpy(voice))
        d_want.zero_()
        ref.decode_dev(d_want.data_ptr(), d_b.data_ptr(), d_v.data_ptr(), s)
        w = d_want.cpu().numpy()
        for c in np.flatnonzero(has):
            assert np.array_equal(got[c][3][j], w[c]), (c, j)
    allk = np.concatenate(kinds)
    assert (allk == 1).any() and (allk == 2).any() and (allk == 0).any()      # voice and control after lock
    eng.close(), rxe.close(), ref.close()
