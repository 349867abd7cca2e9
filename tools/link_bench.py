#!/usr/bin/env python3
"""Packets per second of the link's packet layer (melpe_link_tx_dev,
melpe_link_rx_dev) beside melpe_voice_crypt_dev, the yardstick: all three do
one Keccak-f per packet.

    python tools/link_bench.py [--channels 262144] [--packets 8] [--reps 20] [--out FILE]

Same shape, same process, HIP events around `reps` back-to-back calls after a
warm-up, the median of five such windows.  Packets are half voice, half
silence; the RX side reads what the TX side made, in sync, so it sees the
common path (one permutation per packet).  A call changes its inputs in
place, which does not change its work: TX advances cnt_out (the counters stay
far below the call-time limit), RX decrypts voice again and keeps its counter
through the control packets.  Prints one JSON line; needs a GPU.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=262144)
    ap.add_argument("--packets", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    from pairphone_amd import Link, load_library
    if not torch.cuda.is_available():
        sys.exit("link_bench: no GPU")
    lib = load_library()
    C, K = a.channels, a.packets
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    rng = np.random.Generator(np.random.PCG64(1))
    skey = rng.integers(0, 256, (C, 32), dtype=np.uint8)
    akey = rng.integers(0, 256, (C, 32), dtype=np.uint8)
    cnt = rng.integers(300, 1000, C).astype(np.uint32)
    tx = Link(C).setup(cnt, 0, 8, 1.0, skey, akey)
    rx = Link(C).setup(0, cnt, 8, 1.0, np.roll(skey, 16, 1), np.roll(akey, 16, 1))
    pk = rng.integers(0, 256, (C, K, 11), dtype=np.uint8)
    pk[..., 10] &= 1
    d_pk = torch.from_numpy(pk).to(dev)
    d_voiced = torch.from_numpy((rng.random((C, K)) < 0.5).astype(np.uint8)).to(dev)
    d_ret = torch.zeros((C, K), dtype=torch.int32, device=dev)
    d_voice = torch.zeros((C, K), dtype=torch.uint8, device=dev)
    d_ctr = torch.from_numpy(cnt.view(np.int32)).to(dev)
    d_key = torch.from_numpy(skey[:, :16].copy()).to(dev)

    def timed(fn, prep=None):
        out = []
        for w in range(6):        # the first window is the warm-up
            if prep:
                prep()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                fn()
            e1.record()
            e1.synchronize()
            if w:
                out.append(e0.elapsed_time(e1) / a.reps)
        return float(np.median(out)), out

    def crypt():
        assert lib.melpe_voice_crypt_dev(d_pk.data_ptr(), d_ctr.data_ptr(), d_key.data_ptr(), None, C, K, 0, s) == 0

    # TX: fresh records each window, so cnt_out stays under 65,534
    d_tx = torch.from_numpy(tx.state).to(dev)
    tx0 = d_tx.clone()

    def link_tx():
        tx.tx_dev(d_tx.data_ptr(), d_pk.data_ptr(), d_voiced.data_ptr(), d_ret.data_ptr(), K, None, s)

    # RX input: one TX call's output; each window restarts from the synced records
    d_tx.copy_(tx0)
    d_line = d_pk.clone()
    tx.tx_dev(d_tx.data_ptr(), d_line.data_ptr(), d_voiced.data_ptr(), d_ret.data_ptr(), K, None, s)
    d_rx = torch.from_numpy(rx.state).to(dev)
    rx0 = d_rx.clone()
    d_in = d_line.clone()

    def link_rx():
        # every call sees the same K packets from the same records
        d_rx.copy_(rx0)
        d_in.copy_(d_line)
        rx.rx_dev(d_rx.data_ptr(), d_in.data_ptr(), d_ret.data_ptr(), d_voice.data_ptr(), K, None, s)

    def rx_copies():
        d_rx.copy_(rx0)
        d_in.copy_(d_line)

    res = {"channels": C, "packets": K, "reps": a.reps}
    ms, all_ms = timed(crypt)
    res["voice_crypt_ms"], res["voice_crypt_pkts_per_s"] = ms, C * K / ms * 1e3
    res["voice_crypt_windows_ms"] = all_ms
    ms, all_ms = timed(link_tx, prep=lambda: d_tx.copy_(tx0))
    res["link_tx_ms"], res["link_tx_pkts_per_s"] = ms, C * K / ms * 1e3
    res["link_tx_windows_ms"] = all_ms
    # the RX call is timed with the two device copies that restore its inputs,
    # and the copies alone are timed and taken off
    both, all_both = timed(link_rx)
    cp, _ = timed(rx_copies)
    ms = both - cp
    res["link_rx_ms"], res["link_rx_pkts_per_s"] = ms, C * K / ms * 1e3
    res["link_rx_with_copies_windows_ms"], res["link_rx_copies_ms"] = all_both, cp
    # the RX run was the common path: in sync, control packets authenticated,
    # voice taken as voice (but for the few random voice packets in 100,000
    # that decode as a well-formed control block)
    r = d_ret.cpu().numpy()
    v = d_voiced.cpu().numpy() != 0
    res["rx_off_common_path"] = int((r[v] != -3).sum() + (r[~v] != 8).sum())
    assert res["rx_off_common_path"] < 1e-3 * C * K, res["rx_off_common_path"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
