#!/usr/bin/env python3
"""Generates tests/golden/link.json from the REFERENCE's packet layer.

MakeCtr / ProcessCtr (crp.c:789-982) and fec/fec_golay2412.c, driven through
the harness tests/golden/ref_link.c, which compiles crp.c where it lies into
oracle/_ref/ref_link (built here on demand).  Runs only in the dev
container; the tests import `inputs`, `impair` and `unpack` from here and
never need the harness.

72 channels (one full wave plus a tail of 8) x 64 packets.  `inputs(seed)`
regenerates, from numpy's PCG64, both ends' records, the codec-side packets
and VAD flags; `impair(c, tx_pkts, crafted)` is the line between the two
ends.  Scenario of channel c = c % 12 (SCENARIOS below); main() asserts that
each does what its name says and stores the counts.
"""
import base64
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
REFERENCE = "/root/reference"
TOOL = os.path.join(ROOT, "oracle", "_ref", "ref_link")
SEED, C, K = 2027, 72, 64
REKEY, STAGE = -100, -101

RECORD = np.dtype([("cnt_out", "<u4"), ("cnt_in", "<u4"), ("finv", "<f4"), ("fcrc", "<f4"),
                   ("step", "<i4"), ("scratch", "u1", 6), ("rsv0", "u1", 6), ("skey", "u1", 32), ("akey", "u1", 32),
                   ("fdata", "<f4", 32), ("rsv1", "<u4", 8)])
assert RECORD.itemsize == 256

SCENARIOS = ["clean loopback at step 8, voice and silence",
             "RX at step 5 from cnt_in 0: fast Connected",
             "dropped and repeated packets: fast forward, back clamped to -1",
             "RX 2,000 behind, control only: slow sync",
             "1..3 bit errors per Golay word and in the header: au < 8",
             "4 errors in a word: uncorrectable, taken as voice",
             "inverted line: finv < 0 and bit 81 set",
             "header = crc8(payload): fcrc > 60 forces a reset",
             "step 5 never syncs: the cnt_in == 200 exit",
             "cnt_in from 65,500: the counter-limit exit",
             "control blocks with unrelated counters: late voice fallback",
             "TX from cnt_out 65,500: MELPE_LINK_REKEY"]
CRAFTED = (7, 10)   # scenarios whose RX packets are EncodeBlock outputs (stored in the fixture)


def crc8(data):
    """crp.c:204-248: polynomial 0x25, MSB first"""
    crc = 0
    for b in data:
        crc ^= int(b)
        for _ in range(8):
            crc = ((crc << 1) ^ (0x25 if crc & 0x80 else 0)) & 0xFF
    return crc


def inputs(seed=SEED):
    """(tx records, rx records, packets C x K x 11, voiced C x K)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    pkts = rng.integers(0, 256, (C, K, 11), dtype=np.uint8)
    pkts[..., 10] &= 1
    voiced = (rng.random((C, K)) < 0.5).astype(np.uint8)
    tx = np.zeros(C, RECORD)
    rx = np.zeros(C, RECORD)
    for r in (tx, rx):
        r["skey"] = rng.integers(0, 256, (C, 32), dtype=np.uint8)
        r["akey"] = rng.integers(0, 256, (C, 32), dtype=np.uint8)
        r["finv"] = 1.0
        r["step"] = 8
    # the far end decrypts and authenticates with our sending halves
    rx["skey"][:, 16:] = tx["skey"][:, :16]
    rx["akey"][:, 16:] = tx["akey"][:, :16]
    base = rng.integers(300, 20000, C).astype(np.uint32)
    tx["cnt_out"] = base
    rx["cnt_in"] = base
    rx["cnt_out"] = base + 1000
    tx["cnt_in"] = base + 1000
    for c in range(C):
        s = c % 12
        if s == 1:
            tx["cnt_out"][c] = 201 + c // 12
            rx["cnt_in"][c], rx["cnt_out"][c], rx["step"][c] = 0, 7, 5
            voiced[c, :3] = 0
        elif s == 2:
            voiced[c] = rng.random(K) < 0.25
            voiced[c, [7, 17, 60, 61, 62, 63]] = 0      # the packets after each slip are control
        elif s == 3:
            tx["cnt_out"][c] = base[c] + 3000
            rx["cnt_in"][c] = base[c] + 1000
            voiced[c] = 0
        elif s in (4, 5):
            voiced[c] = 0
        elif s == 6:
            rx["finv"][c] = -1.0
        elif s == 8:
            rx["cnt_in"][c], rx["cnt_out"][c], rx["step"][c] = 150, 7, 5
            voiced[c] = 1
        elif s == 9:
            tx["cnt_out"][c] = 65400
            rx["cnt_in"][c] = 65500
            voiced[c] = 1
        elif s == 11:
            tx["cnt_out"][c] = 65500
            rx["cnt_in"][c] = 65500
    return tx, rx, pkts, voiced


def crafted_payloads(seed=SEED):
    """{channel: K x 6 bytes (payload 4, tag, header)} for the CRAFTED scenarios"""
    rng = np.random.Generator(np.random.PCG64(seed + 1))
    out = {}
    for c in range(C):
        s = c % 12
        if s not in CRAFTED:
            continue
        d = rng.integers(0, 256, (K, 6), dtype=np.uint8)
        for k in range(K):
            if s == 7:
                # a key-exchange packet: header = crc8(payload), and a tag that
                # matches neither copy, so it is never taken for control
                while (d[k, 4] & 15) in (d[k, 0] & 15, d[k, 2] & 15):
                    d[k, 4] = (int(d[k, 4]) + 1) & 15
                d[k, 4] &= 15
                d[k, 5] = crc8(d[k, :4])
            else:
                # a well-formed control block whose counter is noise
                d[k, 2:4] = d[k, 0:2]
                d[k, 4] = d[k, 0] & 15
        out[c] = d
    return out


def _flip(p, bits):
    for b in bits:
        p[int(b) // 8] ^= 1 << (int(b) % 8)


def impair(c, tx_pkts, crafted, seed=SEED):
    """the K packets channel c's receiver sees, from the K its sender made
    (tx_pkts K x 11); crafted = the fixture's EncodeBlock outputs {c: K x 11}"""
    s = c % 12
    rng = np.random.Generator(np.random.PCG64(seed + 100 + c))
    out = tx_pkts.copy()
    if s in CRAFTED:
        return crafted[c].copy()
    if s == 2:
        # two dropped after the 5th, an old one again at 18, one more dropped,
        # the last one twice
        m = [k if k < 5 else k + 2 if k < 18 else 17 if k == 18 else min(k + 1, K - 1) for k in range(K)]
        out = tx_pkts[m].copy()
    elif s == 4:
        for k in range(K):
            for w in range(3):
                _flip(out[k], 8 + 24 * w + rng.choice(24, 1 + (k + w) % 3, replace=False))
            _flip(out[k], rng.choice(8, 1 + k % 2, replace=False))
    elif s == 5:
        for k in range(0, K, 3):
            _flip(out[k], 8 + 24 * ((k // 3) % 3) + rng.choice(24, 4, replace=False))
    elif s == 6:
        out[:, :10] ^= 0xFF
        out[:, 10] ^= 1
    return out


VOICE_RUN = (2028, 400, 2000)   # seed, channels, packets


def voice_inputs(seed=VOICE_RUN[0], n=VOICE_RUN[1], k=VOICE_RUN[2]):
    """a long stretch of voice with no silent superframe: (rx records at
    step 8, n x k random packets).  About 43% of them fail their first Golay
    word, so the crc8 behind fcrc runs over the scratch bytes the previous
    packet left."""
    rng = np.random.Generator(np.random.PCG64(seed))
    rx = np.zeros(n, RECORD)
    rx["skey"] = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    rx["akey"] = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    rx["finv"], rx["step"] = 1.0, 8
    rx["cnt_in"] = rng.integers(300, 20000, n)
    rx["cnt_out"] = rx["cnt_in"] + 1000
    pkts = rng.integers(0, 256, (n, k, 11), dtype=np.uint8)
    pkts[..., 10] &= 1
    return rx, pkts


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def pack(a):
    return base64.b64encode(zlib.compress(np.ascontiguousarray(a).tobytes(), 9)).decode()


def unpack(s, dtype, shape):
    return np.frombuffer(zlib.decompress(base64.b64decode(s)), dtype).reshape(shape).copy()


def build_tool():
    os.makedirs(os.path.dirname(TOOL), exist_ok=True)
    src = [os.path.join(HERE, "ref_link.c")]
    src += ["crypto/%s.c" % n for n in ("sponge", "curve", "havege", "sprng", "b64", "wordlist", "timing")]
    src += ["fec/fec_golay2412.c"]
    subprocess.run(["gcc", "-O2", "-w", "-I" + REFERENCE, "-I" + REFERENCE + "/crypto"] + src +
                   ["-lm", "-o", TOOL], check=True, cwd=REFERENCE)


def _tool(mode, blob=None):
    with tempfile.TemporaryDirectory() as tmp:
        fi, fo = os.path.join(tmp, "in"), os.path.join(tmp, "out")
        if blob is None:
            subprocess.run([TOOL, mode, fo], check=True)
        else:
            open(fi, "wb").write(blob)
            subprocess.run([TOOL, mode, fi, fo], check=True)
        return open(fo, "rb").read()


def ref_run(tx, recs, pkts, voiced=None):
    """MakePkt (tx) / ProcessPkt over C x K packets: (records, packets,
    returns, and for rx the cnt_in and fcrc after each packet)"""
    C, K = pkts.shape[:2]
    blob = np.array([C, K], "<i4").tobytes() + recs.tobytes() + pkts.tobytes()
    if tx:
        blob += voiced.tobytes()
    o = _tool("tx" if tx else "rx", blob)
    n = C * K
    r = np.frombuffer(o[:C * 256], RECORD).copy()
    p = np.frombuffer(o[C * 256:C * 256 + n * 11], np.uint8).reshape(C, K, 11).copy()
    ret = np.frombuffer(o[C * 256 + n * 11:C * 256 + n * 15], "<i4").reshape(C, K).copy()
    if tx:
        return r, p, ret, None, None
    trace = np.frombuffer(o[C * 256 + n * 15:C * 256 + n * 19], "<u4").reshape(C, K).copy()
    ftrace = np.frombuffer(o[C * 256 + n * 19:], "<f4").reshape(C, K).copy()
    return r, p, ret, trace, ftrace


def ref_blocks(d):
    o = _tool("block", np.array([len(d)], "<i4").tobytes() + np.ascontiguousarray(d, np.uint8).tobytes())
    return np.frombuffer(o, np.uint8).reshape(len(d), 11).copy()


def main():
    build_tool()
    tx0, rx0, pkts, voiced = inputs()
    tx1, txp, txret, _, _ = ref_run(True, tx0, pkts, voiced)
    crafted = {c: ref_blocks(d) for c, d in crafted_payloads().items()}
    rxin = np.stack([impair(c, txp[c], crafted) for c in range(C)])
    rx1, rxp, rxret, trace, ftrace = ref_run(False, rx0, rxin)

    counts = {}
    for c in range(C):
        s, r, t = c % 12, rxret[c], txret[c]
        ctl = voiced[c] == 0
        if s == 0:
            assert (r[ctl] == 8).all() and (r[~ctl] == -3).all() and ctl.any() and (~ctl).any()
            assert np.array_equal(rxp[c][~ctl], pkts[c][~ctl])      # voice round-trips
        elif s == 1:
            assert rx1["step"][c] == 8 and rx1["cnt_out"][c] == 201 and trace[c, 0] == tx0["cnt_out"][c] + 1
        elif s == 2:
            assert trace[c, 63] == tx1["cnt_out"][c] and (np.diff(trace[c].astype(np.int64)) == 0).any()
        elif s == 3:
            first = int(np.argmax(trace[c] == tx0["cnt_out"][c] + 1 + np.arange(K)))
            assert first == 36, first                                # syncs at the 37th control packet
        elif s == 4:
            assert ((r >= 0) & (r < 8)).all() and trace[c, 63] == tx1["cnt_out"][c]
        elif s == 5:
            assert (r[0::3] == -3).all() and (r[1::3] == 8).all()
        elif s == 6:
            assert (r[ctl] == 8).all() and np.array_equal(rxp[c][~ctl], pkts[c][~ctl]) and (~ctl).any()
        elif s == 7:
            assert (r[:27] == -3).all() and (r[27:] == 0).all()      # resets at the 28th
            assert rx1["step"][c] == 6 and rx1["cnt_out"][c] == 65535
        elif s == 8:
            assert (r == 0).all() and rx1["step"][c] == 6 and rx1["cnt_out"][c] == 65535
            assert trace[c, 49] == 200 and rx1["cnt_in"][c] == 150 + K
            assert (ftrace[c] <= 60).all()                           # not the fcrc exit
        elif s == 9:
            assert rx1["step"][c] == 6 and rx1["cnt_in"][c] == 65500 + K and (r[34:] == 0).all()
            assert (r[:34] == -3).sum() >= 30 and (ftrace[c] <= 60).all()   # in work mode up to the limit
        elif s == 10:
            assert (r == -3).sum() >= K // 2                         # crp.c:980
            assert not np.array_equal(rxp[c], rxin[c])
        elif s == 11:
            assert (t[:34] > 0).all() and (t[34:] == REKEY).all() and tx1["cnt_out"][c] == 65534
            assert np.array_equal(txp[c, 34:], pkts[c, 34:])
        counts[s] = counts.get(s, 0) + 1
    assert sorted(counts) == list(range(12))

    # the long voice run: fcrc hovers around 0 and nothing resets
    v0, vp = voice_inputs()
    v1, vout, vret, _, vf = ref_run(False, v0, vp)
    assert (v1["step"] == 8).all() and np.array_equal(v1["cnt_out"], v0["cnt_out"]) and vf.max() <= 60
    assert abs(float(v1["fcrc"].mean())) < 1.0, v1["fcrc"].mean()

    g = _tool("golay")
    doc = {
        "what": "MakeCtr / ProcessCtr (crp.c:789-982) and fec_golay2412.c via tests/golden/ref_link.c",
        "seed": SEED, "channels": C, "packets": K,
        "scenarios": {SCENARIOS[s]: counts[s] for s in range(12)},
        "tx_pkts": pack(txp), "tx_ret": pack(txret.astype("<i4")), "tx_state": pack(tx1),
        "crafted": {str(c): pack(p) for c, p in crafted.items()},
        "rx_ret": pack(rxret.astype("<i4")), "rx_state": pack(rx1),
        "rx_pkts_sha256": [hashlib.sha256(rxp[c].tobytes()).hexdigest() for c in range(C)],
        "voice_run": {"seed": VOICE_RUN[0], "channels": VOICE_RUN[1], "packets": VOICE_RUN[2],
                      "state_sha256": sha(v1), "ret_sha256": sha(vret.astype("<i4")), "pkts_sha256": sha(vout),
                      "fcrc_mean": float(v1["fcrc"].mean()), "fcrc_max_over_run": float(vf.max())},
        "golay_enc_sha256": hashlib.sha256(g[:4096 * 4]).hexdigest(),
        "golay_digest": ["%016x" % v for v in np.frombuffer(g[4096 * 4:], "<u8")],
    }
    path = os.path.join(HERE, "link.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote link.json, %d bytes" % os.path.getsize(path))
    assert os.path.getsize(path) < 165616


if __name__ == "__main__":
    sys.exit(main())
