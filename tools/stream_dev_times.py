"""Times of the device stream-format calls (melpe_stream_pack_dev,
melpe_rx_stream_dev) at 65,536 channels with about half the channels silent
per superframe, HIP events around each call, 20 steps after 5 warm-ups:

  pack      melpe_stream_pack_dev
  rx        melpe_rx_stream_dev on the packed frames
  decode    melpe_decode_dev alone with the same bits and mask (what the
            parse and zero-fill kernels add = rx - decode)
  host_rx   the same superframes through the host path, wall clock: one
            melpe_stream_unpack call over the step's frames (they form one
            stream of C frames), H2D of bits and mask, melpe_decode_dev with
            the mask, D2H of the PCM, zero fill of the silent rows on the host
  dev_rx    wall clock of the device path from the same starting point (the
            framed bytes on the host): H2D of bytes and offsets,
            melpe_rx_stream_dev, D2H of the PCM

The bits are the engine's own encoding of the synthetic signal, the votes
random.  Writes one JSON line; --out appends it to a file.

  python tools/stream_dev_times.py [--channels 65536] [--out profiles/x.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pairphone_amd import (MelpeEngine, load_library, stream_pack_dev,  # noqa: E402
                           stream_pack_work_bytes)


def stats(ms):
    a = np.sort(np.asarray(ms))
    return {"median_ms": round(float(np.median(a)), 4), "min_ms": round(float(a[0]), 4),
            "max_ms": round(float(a[-1]), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    C, W, K = a.channels, a.warmup, a.steps
    N = W + K
    lib = load_library()
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream(dev).cuda_stream
    rng = np.random.default_rng(5)

    # the bits of N superframes of every channel
    eng = MelpeEngine(C)
    eng.synth_seed(17)
    pcm = torch.zeros((C, 540), dtype=torch.int16, device=dev)
    bits = torch.zeros((N, C, 11), dtype=torch.uint8, device=dev)
    for k in range(N):
        eng.synth_dev(pcm.data_ptr(), 540, s)
        eng.encode_dev(bits[k].data_ptr(), pcm.data_ptr(), None, s)
    votes = torch.from_numpy((rng.integers(1, 7, (N, C)) * rng.integers(0, 2, (N, C))).astype(np.uint8)).to(dev)
    mask = (votes > 0).to(torch.uint8)
    torch.cuda.synchronize(dev)

    def timed(fn):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(N)]
        for k in range(N):
            ev[k][0].record()
            fn(k)
            ev[k][1].record()
        torch.cuda.synchronize(dev)
        return stats([b.elapsed_time(e) for b, e in ev[W:]])

    # pack
    last = torch.zeros(C, dtype=torch.uint8, device=dev)
    work = torch.zeros(stream_pack_work_bytes(C), dtype=torch.uint8, device=dev)
    out = torch.zeros((N, C * 11), dtype=torch.uint8, device=dev)
    offs = torch.zeros((N, C + 1), dtype=torch.int32, device=dev)
    res = {"channels": C, "steps": K, "warmup": W, "silent_fraction": round(float((mask == 0).float().mean()), 4)}
    res["pack"] = timed(lambda k: stream_pack_dev(bits[k].data_ptr(), votes[k].data_ptr(), last.data_ptr(),
                                                  out[k].data_ptr(), offs[k].data_ptr(), work.data_ptr(),
                                                  C, None, s))

    # rx on the device, then the decode alone from the same decoder state
    sp = torch.zeros((C, 540), dtype=torch.int16, device=dev)
    rbits = torch.zeros((C, 11), dtype=torch.uint8, device=dev)
    voiced = torch.zeros(C, dtype=torch.uint8, device=dev)
    lens = torch.zeros(C, dtype=torch.uint8, device=dev)
    eng.reset(which=2)
    res["rx"] = timed(lambda k: eng.rx_stream_dev(out[k].data_ptr(), offs[k].data_ptr(), offs[k].data_ptr() + 4,
                                                  None, sp.data_ptr(), rbits.data_ptr(), voiced.data_ptr(),
                                                  lens.data_ptr(), None, s))
    want = sp.cpu().numpy().copy()
    eng.reset(which=2)
    res["decode"] = timed(lambda k: eng.decode_dev(sp.data_ptr(), bits[k].data_ptr(), mask[k].data_ptr(), s))
    a_ms, b_ms = res["rx"]["median_ms"], res["decode"]["median_ms"]
    res["parse_and_zero_ms"] = round(a_ms - b_ms, 4)
    res["parse_and_zero_percent_of_decode"] = round(100 * (a_ms - b_ms) / b_ms, 2)

    # the two receive paths from framed bytes on the host, wall clock
    h_out = [out[k].cpu().numpy() for k in range(N)]
    h_offs = [offs[k].cpu().numpy() for k in range(N)]
    h_bits = np.zeros((C, 11), np.uint8)
    h_voiced = np.zeros(C, np.uint8)
    h_pcm = torch.zeros((C, 540), dtype=torch.int16).pin_memory()

    def host_rx(k):
        total = int(h_offs[k][C])
        n = lib.melpe_stream_unpack(h_out[k].ctypes.data, total, h_bits.ctypes.data, h_voiced.ctypes.data, C)
        assert n == C
        rbits.copy_(torch.from_numpy(h_bits))
        voiced.copy_(torch.from_numpy(h_voiced))
        eng.decode_dev(sp.data_ptr(), rbits.data_ptr(), voiced.data_ptr(), s)
        h_pcm.copy_(sp)
        torch.cuda.synchronize(dev)
        h_pcm.numpy()[h_voiced == 0] = 0

    d_stream = torch.zeros(C * 11, dtype=torch.uint8, device=dev)
    d_offs = torch.zeros(C + 1, dtype=torch.int32, device=dev)

    def dev_rx(k):
        total = int(h_offs[k][C])
        d_stream[:total].copy_(torch.from_numpy(h_out[k][:total]))
        d_offs.copy_(torch.from_numpy(h_offs[k]))
        eng.rx_stream_dev(d_stream.data_ptr(), d_offs.data_ptr(), d_offs.data_ptr() + 4, None, sp.data_ptr(),
                          rbits.data_ptr(), voiced.data_ptr(), lens.data_ptr(), None, s)
        h_pcm.copy_(sp)
        torch.cuda.synchronize(dev)

    for name, fn in (("host_rx", host_rx), ("dev_rx", dev_rx)):
        eng.reset(which=2)
        ms = []
        for k in range(N):
            t0 = time.perf_counter()
            fn(k)
            ms.append(1e3 * (time.perf_counter() - t0))
        res[name + "_wall"] = stats(ms[W:])
        # both paths must give the PCM of the timed rx above (last step)
        assert np.array_equal(h_pcm.numpy()[h_voiced > 0], want[h_voiced > 0]), name
        assert not h_pcm.numpy()[h_voiced == 0].any(), name
    eng.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
