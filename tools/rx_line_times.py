#!/usr/bin/env python3
"""melpe_rx_line_dev beside the sequence it replaces, on the same inputs:
melpe_demodulate_dev + melpe_link_rx_dev + melpe_decode_dev.

    python tools/rx_line_times.py [--channels 65536 262144] [--steps 20] [--warmup 5] [--out FILE]

Per channel count: a line of 14 packets per channel is made on the device
(melpe_link_tx_dev on random packets, half voice and half silence, then
melpe_modulate_dev); every channel's cursor starts at its own offset within
the first packet, so the channels' blocks fall on different calls of a launch
and the loop kernel's link branch diverges as it does on real lines.  SYNC
launches of 15 calls bring the receivers in sync; the state after them is
kept, and every timed step restores it (outside the timed span) and makes the
next launch.  The share of channels whose block was locked in the timed launch
is recorded (`locked_share`).  HIP events around each step, the median over
`steps` after `warmup`.

The sequence is timed part by part, without the host round trip and the
compaction it needs between the parts (the link call reads a packet buffer of
the same shape the compaction would give).  The loop kernel itself is
estimated as the call minus its decode launches, which are timed alone on the
fused call's own outputs: slot j's bits under the mask voice[j] where j is
below the channel's count (the zero fill and the mask kernels stay in the
estimate).  The decode launches of the slots past the first are also timed
alone (`decode_extra_slots_ms`): nearly always empty, a sort each.
That difference carries the error of two event-timed spans (it has come out
below k_demodulate's own time); for the kernel's time run this tool under a
kernel trace and read it with tools/rx_line_ktrace.py.
Prints one JSON line per channel count; needs a GPU.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PKT, CALLS, NPKT = 3240, 15, 14
SYNC = 12      # launches before the timed one: the block lag locks after five to eleven, by the cursor offset


def measure(C, steps, warmup):
    import torch
    from pairphone_amd import Link, MelpeEngine, load_library
    lib = load_library()
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    rng = np.random.Generator(np.random.PCG64(3))
    skey = rng.integers(0, 256, (C, 32), dtype=np.uint8)
    akey = rng.integers(0, 256, (C, 32), dtype=np.uint8)
    cnt = rng.integers(300, 1000, C).astype(np.uint32)
    tx = Link(C).setup(cnt, 0, 8, 1.0, skey, akey)
    rx = Link(C).setup(0, cnt, 8, -1.0, np.roll(skey, 16, 1), np.roll(akey, 16, 1))
    pk = rng.integers(0, 256, (C, NPKT, 11), dtype=np.uint8)
    pk[..., 10] &= 1
    d_pk = torch.from_numpy(pk).to(dev)
    d_voiced = torch.from_numpy((rng.random((C, NPKT)) < 0.5).astype(np.uint8)).to(dev)
    d_ret = torch.zeros((C, NPKT), dtype=torch.int32, device=dev)
    d_tx = torch.from_numpy(tx.state).to(dev)
    tx.tx_dev(d_tx.data_ptr(), d_pk.data_ptr(), d_voiced.data_ptr(), d_ret.data_ptr(), NPKT, None, s)
    stride = NPKT * PKT + 1088
    d_line = torch.zeros((C, stride), dtype=torch.int16, device=dev)
    d_mod = torch.zeros(C * lib.melpe_modem_state_bytes(), dtype=torch.uint8, device=dev)
    assert lib.melpe_modem_reset_dev(d_mod.data_ptr(), C, None, s) == 0
    d_tmp = torch.zeros((C, NPKT * PKT), dtype=torch.int16, device=dev)
    assert lib.melpe_modulate_dev(d_mod.data_ptr(), d_pk.data_ptr(), d_tmp.data_ptr(), C, NPKT, None, s) == 0
    d_line[:, :NPKT * PKT] = d_tmp
    del d_tmp

    eng = MelpeEngine(C)
    slots = CALLS // 15 + 2
    st = {"modem": torch.zeros(C * lib.melpe_modem_state_bytes(), dtype=torch.uint8, device=dev),
          "link": torch.from_numpy(rx.state).to(dev),
          "rx": torch.zeros(C * 16, dtype=torch.uint8, device=dev),
          "pos": torch.from_numpy(rng.integers(0, PKT, C).astype(np.int32)).to(dev),
          "data": torch.zeros(C * 12, dtype=torch.uint8, device=dev)}
    assert lib.melpe_modem_reset_dev(st["modem"].data_ptr(), C, None, s) == 0
    d_sp = torch.zeros((slots, C, 540), dtype=torch.int16, device=dev)
    d_bits = torch.zeros((slots, C, 11), dtype=torch.uint8, device=dev)
    d_voice = torch.zeros((slots, C), dtype=torch.uint8, device=dev)
    d_info = torch.zeros((slots, C, 8), dtype=torch.uint8, device=dev)
    d_count = torch.zeros(C, dtype=torch.uint8, device=dev)

    def rx_line():
        eng.rx_line_dev(st["modem"].data_ptr(), st["link"].data_ptr(), st["rx"].data_ptr(), d_line.data_ptr(), stride,
                        st["pos"].data_ptr(), st["data"].data_ptr(), d_sp.data_ptr(), d_bits.data_ptr(),
                        d_voice.data_ptr(), d_info.data_ptr(), d_count.data_ptr(), CALLS, slots, None, s)

    for _ in range(SYNC):
        rx_line()
    torch.cuda.synchronize()
    kept = {k: v.clone() for k, v in st.items()}
    dec0 = eng.export_state(2)      # the decoder records go back too

    def restore():
        for k, v in st.items():
            v.copy_(kept[k])

    def timed(fn, undo=restore):
        out = []
        for i in range(warmup + steps):
            undo()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= warmup:
                out.append(e0.elapsed_time(e1))
        return float(np.median(out)), float(min(out)), float(max(out))

    res = {"channels": C, "calls": CALLS, "steps": steps, "warmup": warmup,
           "rx_line_private_bytes": lib.melpe_rx_line_private_bytes()}
    res["rx_line_ms"], res["rx_line_min_ms"], res["rx_line_max_ms"] = timed(rx_line)
    info = d_info.cpu().numpy().view(np.uint8).reshape(slots, C, 8)
    count = d_count.cpu().numpy()
    kind = info[0, :, 2]
    res["blocks_per_channel_mean"] = float(count.mean())
    res["slot0_kinds"] = [int((kind[count > 0] == k).sum()) for k in range(4)]
    res["event_calls_distinct"] = int(len(np.unique(info[0, count > 0, 0])))
    res["sync_launches"] = SYNC
    res["locked_share"] = float(((kind != 0) & (count > 0)).mean())
    # the fused call's own decode masks and bits, kept for the decode-only baseline
    jj = torch.arange(slots, device=dev, dtype=torch.int32)[:, None]
    f_mask = ((d_voice != 0) & (jj < d_count.to(torch.int32)[None, :])).to(torch.uint8).contiguous()
    f_bits = d_bits.clone()
    res["fused_voice_share"] = [float(f_mask[j].float().mean().item()) for j in range(slots)]

    # the sequence, part by part, on the same state and line
    d_out = torch.zeros((C, CALLS, 12), dtype=torch.uint8, device=dev)
    d_r = torch.zeros((C, CALLS), dtype=torch.int32, device=dev)

    def demod():
        assert lib.melpe_demodulate_dev(st["modem"].data_ptr(), d_line.data_ptr(), stride, st["pos"].data_ptr(),
                                        st["data"].data_ptr(), d_out.data_ptr(), d_r.data_ptr(), C, CALLS, None, s) == 0
    res["demodulate_ms"], res["demodulate_min_ms"], res["demodulate_max_ms"] = timed(demod)

    def demod_bare():      # without the status rows the sequence needs: the calls alone
        assert lib.melpe_demodulate_dev(st["modem"].data_ptr(), d_line.data_ptr(), stride, st["pos"].data_ptr(),
                                        st["data"].data_ptr(), None, None, C, CALLS, None, s) == 0
    res["demodulate_no_rows_ms"], _, _ = timed(demod_bare)
    # the packets the compaction would hand the link: the blocks the loop handed out, before ProcessPkt
    restore()
    demod()
    o = d_out.cpu().numpy()
    ready = (o[:, :, 11] & 0x80) != 0
    first = ready.argmax(axis=1)
    d_p = torch.from_numpy(np.ascontiguousarray(o[np.arange(C), first, :11])).to(dev)
    p0 = d_p.clone()
    d_lret = torch.zeros(C, dtype=torch.int32, device=dev)
    d_lv = torch.zeros(C, dtype=torch.uint8, device=dev)

    def link_undo():
        restore()
        d_p.copy_(p0)

    def link():
        assert lib.melpe_link_rx_dev(st["link"].data_ptr(), d_p.data_ptr(), d_lret.data_ptr(), d_lv.data_ptr(), C, 1,
                                     None, s) == 0
    res["link_rx_ms"], _, _ = timed(link, link_undo)
    res["sequence_voice_share"] = float(d_lv.cpu().numpy().mean())
    d_dsp = torch.zeros((C, 540), dtype=torch.int16, device=dev)

    def dec_undo():
        eng.import_state(2, dec0)

    def decode():
        eng.decode_dev(d_dsp.data_ptr(), d_p.data_ptr(), d_lv.data_ptr(), s)
    res["decode_ms"], res["decode_min_ms"], res["decode_max_ms"] = timed(decode, dec_undo)

    def decode_slots(first=0):
        for j in range(first, slots):
            eng.decode_dev(d_dsp.data_ptr(), f_bits[j].data_ptr(), f_mask[j].data_ptr(), s)
    res["decode_slots_ms"], res["decode_slots_min_ms"], res["decode_slots_max_ms"] = timed(decode_slots, dec_undo)
    res["decode_extra_slots_ms"], _, _ = timed(lambda: decode_slots(1), dec_undo)
    res["sequence_ms"] = res["demodulate_ms"] + res["link_rx_ms"] + res["decode_ms"]
    res["rx_line_kernel_est_ms"] = res["rx_line_ms"] - res["decode_slots_ms"]
    res["kernel_over_demodulate"] = res["rx_line_kernel_est_ms"] / res["demodulate_ms"]
    res["kernel_over_demodulate_no_rows"] = res["rx_line_kernel_est_ms"] / res["demodulate_no_rows_ms"]
    res["rx_line_over_sequence"] = res["rx_line_ms"] / res["sequence_ms"]
    eng.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, nargs="+", default=[65536, 262144])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("rx_line_times: no GPU")
    rows = []
    for C in a.channels:
        rows.append(measure(C, a.steps, a.warmup))
        print(json.dumps(rows[-1]), flush=True)
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
