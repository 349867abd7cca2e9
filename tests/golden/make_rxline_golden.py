#!/usr/bin/env python3
"""Generates tests/golden/rxline.json from the REFERENCE's receive chain.

Demodulate (modem/modem.c), ProcessPkt (crp.c) and melpe_s, driven through
the harness tests/golden/ref_rxline.c, which compiles crp.c and modem.c where
they lie into oracle/_ref/ref_rxline (built here on demand) and restates only
the control flow of rx.c:294-361 with the playback buffer held empty.  Runs
only in the dev container; the tests import `inputs`, `clean_line`, `impair`,
`avail`, `unpack` and the constants from here and never need the harness.

72 channels (one full wave plus a tail of 8) x 24 packet times.  The line of
channel c is the reference's Modulate of the reference's MakePkt packets
(asserted equal to the host build's, which is how the tests regenerate it;
the fixture keeps its SHA-256), passed through `impair(c, pcm)`, integer-only
numpy.  Scenario of channel c = c % 12 (SCENARIOS below); main() asserts that
each does what its name says and stores the counts.

Two runs are stored.  The main run is 24 launches of 15 calls with the line
arriving in real time: launch l sees the row up to avail(l) samples, one
packet time more per launch, so a receiver that consumes faster than the line
arrives runs short (a call that lacks its 1,080 samples ends the launch) and
picks up in the next.  The `full` run is the same 360 calls with the whole row
present, which is independent of how the calls are grouped into launches.
"""
import base64
import ctypes
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
import make_link_golden as mlg  # noqa: E402

REFERENCE = "/root/reference"
TOOL = os.path.join(ROOT, "oracle", "_ref", "ref_rxline")
REF_MODEM = os.path.join(ROOT, "oracle", "_ref", "ref_modem")
EMU = os.path.join(ROOT, "build", "libmelpe_hostemu.so")

SEED, C, K = 2031, 72, 24
CALLS = 15              # Demodulate calls per launch: one packet time
PKT = 3240              # samples per packet
LOOK = 1080             # samples a call needs (rx.c:246)
STRIDE = 80640          # the whole row: 24 packets, the lookahead, the shift and the repeats
SLACK = 32              # samples the arriving line is ahead of what 15 calls of 216 per launch need
SHIFT10 = 2000          # scenario 10: the channel's cursor starts this far into its row
CUT5 = (30000, 1500)    # scenario 5: samples [at, at + n) cut out of the line
BAD9 = (7, 10)          # scenario 9: the packets whose parity symbols are inverted
STAGE, NOLOCK = -101, -102
RECORD = mlg.RECORD
RXREC = np.dtype([("fber", "<f4"), ("fau", "<f4"), ("blocks", "<u4"), ("rsv", "<u4")])
INFO = np.dtype([("call", "u1"), ("status", "u1"), ("kind", "u1"), ("zero", "u1"), ("ret", "<i4")])
MODEM_BYTES = 1384

SCENARIOS = ["clean loopback at step 8, voice and silence",
             "line starts mid-packet behind 1,000 samples of low noise: blocks before lag lock are kind 0",
             "negated line: it cancels the modem loop's own inversion, finv > 0 where the others have finv < 0",
             "one sample dropped every 400: returns other than 216",
             "one sample repeated every 400: the receiver outruns the arriving line and runs short",
             "1,500 samples cut mid-stream: forced blocks (status 0x8F) with align still set",
             "bursts of integer noise: error nibbles, fber > 0, au < 8, uncorrectable words taken as voice",
             "silence throughout: all control, fau climbs",
             "link record at step 4: kind 3 everywhere, record untouched",
             "three packets with every parity bit inverted under noise (9 symbol errors per block: noise alone "
             "averages 4.5 and cannot reach falign > 40 in 24 packets): align drops, then recovery and resync",
             "cursor 2,000 samples ahead: the row ends mid-launch, -1 stops the channel, the next launch continues",
             "masked out by active"]


def avail(l):
    """samples of every row present at launch l of the main run"""
    return min(STRIDE, ((l + 1) * CALLS - 1) * 216 + LOOK + SLACK)


def inputs(seed=SEED):
    """(tx records, rx records, packets C x K x 11, voiced C x K, active C)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    pkts = rng.integers(0, 256, (C, K, 11), dtype=np.uint8)
    pkts[..., 10] &= 1
    voiced = (rng.random((C, K)) < 0.5).astype(np.uint8)
    tx = np.zeros(C, RECORD)
    rx = np.zeros(C, RECORD)
    for r in (tx, rx):
        r["skey"] = rng.integers(0, 256, (C, 32), dtype=np.uint8)
        r["akey"] = rng.integers(0, 256, (C, 32), dtype=np.uint8)
        # the demodulator hands out the modulator's bits inverted (a clean
        # loopback is an inverted channel, which a real call's key exchange
        # learns): finv < 0 on a plain line, > 0 on a negated one
        r["finv"] = -1.0
        r["step"] = 8
    rx["skey"][:, 16:] = tx["skey"][:, :16]
    rx["akey"][:, 16:] = tx["akey"][:, :16]
    base = rng.integers(300, 20000, C).astype(np.uint32)
    tx["cnt_out"] = base
    rx["cnt_in"] = base
    rx["cnt_out"] = base + 1000
    tx["cnt_in"] = base + 1000
    active = np.ones(C, np.uint8)
    for c in range(C):
        s = c % 12
        if s == 2:
            rx["finv"][c] = 1.0
        elif s in (6, 7):
            voiced[c] = 0
        elif s == 8:
            rx["step"][c] = 4
        elif s == 9:
            voiced[c, 14:] = 0      # control packets after the noise: the counter resynchronises
        elif s == 11:
            active[c] = 0
    return tx, rx, pkts, voiced, active


def emu():
    lib = ctypes.CDLL(EMU)
    return lib


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def clean_line(seed=SEED):
    """(tx packets C x K x 11, line C x K*3240 int16) by the host build of
    MakeCtr and Modulate; main() asserts both equal the reference's"""
    tx0, _, pkts, voiced, _ = inputs(seed)
    lib = emu()
    st = np.ascontiguousarray(tx0).view(np.uint8).reshape(C, 256).copy()
    p = pkts.copy()
    ret = np.zeros((C, K), np.int32)
    assert lib.emu_link_tx(_p(st), _p(p), _p(voiced), _p(ret), C, K, None) == 0
    ms = np.zeros((C, lib.emu_modem_state_bytes()), np.uint8)
    lib.emu_modem_reset(_p(ms), C)
    pcm = np.zeros((C, K * PKT), np.int16)
    assert lib.emu_modulate(_p(ms), _p(p), _p(pcm), C, K) == 0
    return p, pcm


def impair(c, pcm, seed=SEED):
    """the STRIDE samples of channel c's row, from the K * 3240 its sender
    made; what follows the line is silence"""
    s = c % 12
    rng = np.random.Generator(np.random.PCG64(seed + 100 + c))
    x = pcm.astype(np.int32)
    if s == 1:
        x = np.concatenate([rng.integers(-20, 21, 1000), x[1700:]])
    elif s == 2:
        x = -x
    elif s == 3:
        x = np.delete(x, np.arange(399, len(x), 400))
    elif s == 4:
        x = np.insert(x, np.arange(399, len(x), 400), x[399::400])
    elif s == 5:
        x = np.concatenate([x[:CUT5[0]], x[CUT5[0] + CUT5[1]:]])
    elif s == 6:
        # from the seventh packet on, a burst of 150..450 samples of each packet replaced by noise
        # (700 in the thirteenth: more errors than the Golay words correct)
        for k in range(6, K):
            n = 700 if k == 12 else int(rng.integers(150, 451))
            at = k * PKT + int(rng.integers(0, PKT - n))
            x[at:at + n] = rng.integers(-16000, 16001, n)
    elif s == 9:
        # every parity bit of these packets inverted (their last 9 x 36 samples negated) and noise on top
        for k in range(*BAD9):
            x[(k + 1) * PKT - 324:(k + 1) * PKT] *= -1
            x[k * PKT:(k + 1) * PKT] += rng.integers(-3000, 3001, PKT)
    elif s == 10:
        x = np.concatenate([np.zeros(SHIFT10, np.int32), x])
    out = np.zeros(STRIDE, np.int16)
    n = min(len(x), STRIDE)
    out[:n] = np.clip(x[:n], -32768, 32767)
    return out


def pos0(c):
    return SHIFT10 if c % 12 == 10 else 0


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


pack, unpack = mlg.pack, mlg.unpack


def build_tool():
    os.makedirs(os.path.dirname(TOOL), exist_ok=True)
    src = [os.path.join(HERE, "ref_rxline.c")]
    src += ["crypto/%s.c" % n for n in ("sponge", "curve", "havege", "sprng", "b64", "wordlist", "timing")]
    src += ["fec/fec_golay2412.c", os.path.join(ROOT, "oracle", "_ref", "libmelpe_ref.a")]
    subprocess.run(["gcc", "-O2", "-w", "-I" + REFERENCE, "-I" + REFERENCE + "/crypto", "-I" + REFERENCE + "/modem"]
                   + src + ["-lm", "-o", TOOL], check=True, cwd=REFERENCE)


def ref_modulate(pkts):
    out = np.zeros((C, K * PKT), np.int16)
    with tempfile.TemporaryDirectory() as tmp:
        bf, pf = os.path.join(tmp, "b"), os.path.join(tmp, "p")
        for c in range(C):
            open(bf, "wb").write(pkts[c].tobytes())
            subprocess.run([REF_MODEM, "mod", bf, pf], check=True)
            out[c] = np.frombuffer(open(pf, "rb").read(), "<i2")
    return out


def ref_channel(samples, plan, link, rxrec):
    """one channel through the harness: (per-launch counts, blocks (info,
    bits, voice, pcm), pos, data, modem, link, rx)"""
    with tempfile.TemporaryDirectory() as tmp:
        fi, fo = os.path.join(tmp, "in"), os.path.join(tmp, "out")
        blob = np.array([len(samples), len(plan)], "<i4").tobytes() + np.array(plan, "<i4").tobytes()
        blob += link.tobytes() + rxrec.tobytes() + samples.astype("<i2").tobytes()
        open(fi, "wb").write(blob)
        subprocess.run([TOOL, fi, fo], check=True)
        o = open(fo, "rb").read()
    at, counts, blocks = 0, [], []
    for _ in plan:
        n, made = (int(v) for v in np.frombuffer(o[at:at + 8], "<i4"))
        at += 8
        counts.append((n, made))
        for _ in range(n):
            info = np.frombuffer(o[at:at + 8], INFO)[0].copy()
            bits = np.frombuffer(o[at + 8:at + 19], np.uint8).copy()
            voice = o[at + 19]
            pcm = np.frombuffer(o[at + 20:at + 20 + 1080], "<i2").copy()
            at += 1100
            blocks.append((info, bits, voice, pcm))
    pos = int(np.frombuffer(o[at:at + 4], "<i4")[0])
    data = np.frombuffer(o[at + 4:at + 16], np.uint8).copy()
    at += 16
    modem = np.frombuffer(o[at:at + MODEM_BYTES], np.uint8).copy()
    at += MODEM_BYTES
    lk = np.frombuffer(o[at:at + 256], RECORD)[0].copy()
    rx = np.frombuffer(o[at + 256:at + 272], RXREC)[0].copy()
    assert at + 272 == len(o)
    return counts, blocks, pos, data, modem, lk, rx


def blocks_digest(info, bits, voice, pcm):
    """one channel's blocks in order, without the index of the call that
    produced each (which depends on how the calls are grouped)"""
    i = np.ascontiguousarray(info, INFO).view(np.uint8).reshape(-1, 8)[:, 1:]
    h = hashlib.sha256()
    for a in (i, np.asarray(bits, np.uint8), np.asarray(voice, np.uint8), np.asarray(pcm, "<i2")):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def final_digest(pos, data, modem, link, rx):
    h = hashlib.sha256()
    for a in (np.array([pos], "<i4"), data, modem, np.ascontiguousarray(link).view(np.uint8),
              np.ascontiguousarray(rx).view(np.uint8)):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def main():
    mlg.build_tool()
    build_tool()
    tx0, rx0, pkts, voiced, active = inputs()
    _, txp, txret, _, _ = mlg.ref_run(True, tx0, pkts, voiced)
    line = ref_modulate(txp)
    ep, eline = clean_line()
    assert np.array_equal(ep, txp) and np.array_equal(eline, line), "host build and reference disagree on the line"
    rows = np.stack([impair(c, line[c]) for c in range(C)])

    zero = np.zeros(1, RXREC)
    plan = [[(CALLS, avail(l)) for l in range(K)], [(CALLS, STRIDE)] * K]
    runs = []
    for full in (0, 1):
        res = []
        for c in range(C):
            if not active[c]:
                res.append(None)
                continue
            p = [(n, a - pos0(c)) for n, a in plan[full]]
            res.append(ref_channel(rows[c][pos0(c):], p, rx0[c:c + 1], zero))
        runs.append(res)

    stats, weak6 = {}, 0
    for c in range(C):
        s = c % 12
        if runs[0][c] is None:
            assert s == 11
            stats[s] = stats.get(s, 0) + 1
            continue
        cm, blocks, pos, data, modem, lk, rx = runs[0][c]
        counts, made = [n for n, _ in cm], [m for _, m in cm]
        info = np.array([b[0] for b in blocks], INFO)
        kind, ret, st = info["kind"], info["ret"], info["status"]
        assert (kind <= 3).all() and sum(counts) == len(blocks) == rx["blocks"] and max(counts) <= CALLS // 15 + 2
        locked = (st & 0x40) != 0
        assert np.array_equal(kind == 0, ~locked) and (ret[kind == 0] == NOLOCK).all()
        short = sum(1 for m in made if m < CALLS)        # launches the row's end cut short
        forced = int((((st & 0x8F) == 0x8F) & locked).sum())
        ctl = np.flatnonzero(kind == 1)
        n = 1
        if s not in (8,):
            assert len(ctl) and lk["step"] == 8
        if s == 0:
            # the modem locks within five blocks; the first control packet brings the counter in step
            assert (kind[5:] != 0).all() and (kind == 2).any() and (ret[ctl[1:]] == 8).all() and short == 0
            assert lk["cnt_in"] == tx0["cnt_out"][c] + K and counts == [1] * K
            for b in range(ctl[0] + 1, K):      # one block per packet: voice round-trips
                assert (kind[b] == 2) == bool(voiced[c, b])
                if kind[b] == 2:
                    got = blocks[b][1]
                    assert np.array_equal(got[:10], pkts[c, b, :10]) and (got[10] ^ pkts[c, b, 10]) & 1 == 0
        elif s == 1:
            n = int((kind == 0).sum())
            assert n >= 1 and (kind[-8:] != 0).all() and lk["cnt_in"] == tx0["cnt_out"][c] + K
            # the reference again over the launches before the first locked block:
            # blocks before lag lock leave the link record, cnt_in included, untouched
            first = int(np.flatnonzero(kind != 0)[0])
            lead = int(np.searchsorted(np.cumsum(counts), first, side="right"))
            _, b0, _, _, _, lk0, rx0_ = ref_channel(rows[c], plan[0][:lead], rx0[c:c + 1], zero)
            assert 3 <= len(b0) == sum(counts[:lead]) == rx0_["blocks"] and all(b[0]["kind"] == 0 for b in b0)
            assert lk0.tobytes() == rx0[c].tobytes() and lk0["cnt_in"] == rx0["cnt_in"][c]
        elif s == 2:
            assert (kind == 2).any() and (ret[ctl[1:]] == 8).all() and lk["finv"] > 0
            assert lk["cnt_in"] == tx0["cnt_out"][c] + K
            for b in range(ctl[0] + 1, K):
                assert kind[b] != 2 or np.array_equal(blocks[b][1][:10], pkts[c, b, :10])
        elif s == 3:
            assert pos < K * CALLS * 216 - 100 and short == 0 and (ret[ctl[1:]] == 8).all()
        elif s == 4:
            n = short
            assert short >= 1 and (ret[ctl[1:]] == 8).all()
        elif s == 5:
            n = forced      # 0 = the cut did not provoke it with the reference
            assert ((st & 0x0F) > 0).any()
        elif s == 6:
            assert rx["fber"] > 0 and ((st & 0x0F) > 0).sum() >= 10
            assert not voiced[c].any()
            weak6 += int(((ret[ctl[1:]] >= 0) & (ret[ctl[1:]] < 8)).sum())      # au < 8 after the first sync
            n = int((kind == 2).sum())      # control packets taken as voice
        elif s == 7:
            assert (kind[5:] == 1).all() and rx["fau"] > 100 and rx["fber"] == 0
        elif s == 8:
            assert (kind[locked] == 3).all() and (ret[locked] == STAGE).all() and locked.sum() >= K - 6
            assert lk.tobytes() == rx0[c].tobytes() and rx["fau"] == 0
        elif s == 9:
            lost = np.flatnonzero(kind[5:] == 0) + 5
            assert len(lost) >= 3 and (kind[-4:] == 1).all() and (ret[-2:] == 8).all()
            assert lk["cnt_in"] == tx0["cnt_out"][c] + K
            n = len(lost)
        elif s == 10:
            n = K * CALLS - sum(made)      # calls the channel lost to the row's end
            assert 0 < made[0] < CALLS and n >= 1
        stats[s] = stats.get(s, 0) + (n if s in (1, 4, 5, 6, 9, 10) else 1)
    assert sorted(stats) == list(range(12)) and weak6 >= 3 and stats[6] >= 3

    maxb = max(len(r[1]) for r in runs[0] if r)
    info = np.zeros((C, maxb), INFO)
    counts = np.zeros((K, C), np.uint8)
    made = np.zeros((K, C), np.uint8)
    doc = {
        "what": "rx.c:294-361 with the playback buffer empty: Demodulate, ProcessPkt and melpe_s of the "
                "reference via tests/golden/ref_rxline.c",
        "seed": SEED, "channels": C, "packets": K, "calls": CALLS, "stride": STRIDE,
        "scenarios": {SCENARIOS[s]: stats[s] for s in range(12)},
        "line_sha256": sha(line), "rows_sha256": sha(rows),
        "bits_sha256": [], "voice_sha256": [], "pcm_sha256": [], "modem_sha256": [],
        "full": {"blocks_sha256": [], "final_sha256": []},
    }
    pos = np.zeros(C, "<i4")
    data = np.zeros((C, 12), np.uint8)
    link = rx0.copy()
    rxr = np.zeros(C, RXREC)
    for c in range(C):
        r, f = runs[0][c], runs[1][c]
        if r is None:
            for k in ("bits_sha256", "voice_sha256", "pcm_sha256", "modem_sha256"):
                doc[k].append("")
            doc["full"]["blocks_sha256"].append("")
            doc["full"]["final_sha256"].append("")
            continue
        counts[:, c] = [n for n, _ in r[0]]
        made[:, c] = [m for _, m in r[0]]
        info[c, :len(r[1])] = [b[0] for b in r[1]]
        doc["bits_sha256"].append(sha(np.array([b[1] for b in r[1]], np.uint8)))
        doc["voice_sha256"].append(sha(np.array([b[2] for b in r[1]], np.uint8)))
        doc["pcm_sha256"].append(sha(np.array([b[3] for b in r[1]], "<i2")))
        doc["modem_sha256"].append(sha(r[4]))
        pos[c], data[c], link[c], rxr[c] = r[2] + pos0(c), r[3], r[5], r[6]
        doc["full"]["blocks_sha256"].append(blocks_digest([b[0] for b in f[1]], [b[1] for b in f[1]],
                                                          [b[2] for b in f[1]], [b[3] for b in f[1]]))
        doc["full"]["final_sha256"].append(final_digest(f[2] + pos0(c), f[3], f[4], f[5], f[6]))
    doc.update(info=pack(info), counts=pack(counts), made=pack(made), pos=pack(pos), data=pack(data), link=pack(link),
               rx=pack(rxr), max_blocks=maxb)
    path = os.path.join(HERE, "rxline.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote rxline.json, %d bytes" % os.path.getsize(path))
    for s in range(12):
        print("%2d %4d  %s" % (s, stats[s], SCENARIOS[s]))
    assert os.path.getsize(path) < 200000


if __name__ == "__main__":
    sys.exit(main())
