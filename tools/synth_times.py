"""Times of the synthesis from parameter rows against the full decoder, HIP
events around each call, on equivalent content:

  synth       melpe_synth_params_dev on the channel reader's rows of the bits
  decode      melpe_decode_dev on the bits (the yardstick, on a second engine)

The bits are the engine's own encoding of the synthetic signal for --distinct
channels, tiled up to the channel count; their reader rows (before melp_syn's
parameter head) come from the host build's emu_read_rows, which is why the
distinct channels are few.  synth and decode alternate superframe by
superframe in one loop, --steps timed superframes after --warmup, once with
the lane order on (the synthesis cuts it by the rows being synthesised, the
decode by the previous superframe's) and once with it off.  Every superframe's
PCM of the two engines is compared.  Writes one JSON line per channel count
and lane order; --out appends them to a file.

  python tools/synth_times.py [--channels 32768,262144] [--out profiles/synth_params_times.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from pairphone_amd import MelpeEngine  # noqa: E402
from make_synpar_golden import reader_rows  # noqa: E402


def stats(ms):
    a = np.sort(np.asarray(ms))
    return {"median_ms": round(float(np.median(a)), 4), "min_ms": round(float(a[0]), 4),
            "max_ms": round(float(a[-1]), 4)}


def content(D, N, dev, s):
    """(bits [N, D, 11] uint8, rows [N, D, 90] int16) of D distinct channels"""
    eng = MelpeEngine(D)
    eng.synth_seed(17)
    pcm = torch.zeros((D, 540), dtype=torch.int16, device=dev)
    bits = torch.zeros((N, D, 11), dtype=torch.uint8, device=dev)
    for k in range(N):
        eng.synth_dev(pcm.data_ptr(), 540, s)
        eng.encode_dev(bits[k].data_ptr(), pcm.data_ptr(), None, s)
    torch.cuda.synchronize(dev)
    eng.close()
    b = bits.cpu().numpy()
    rows, erase = reader_rows(np.ascontiguousarray(b.transpose(1, 0, 2)))
    assert not erase.any()
    return b, np.ascontiguousarray(rows.transpose(1, 0, 2))


def run(C, W, K, order, bits, rows, dev, s):
    N = W + K
    reps = C // bits.shape[1]
    d_bits = torch.from_numpy(np.tile(bits, (1, reps, 1))).to(dev)
    d_rows = torch.from_numpy(np.tile(rows, (1, reps, 1))).to(dev)

    def pair():
        return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(ev, fn):
        ev[0].record()
        fn()
        ev[1].record()

    def ms(evs):
        return stats([b.elapsed_time(e) for b, e in evs[W:]])

    se, de = MelpeEngine(C), MelpeEngine(C)
    for e in (se, de):
        e.set_lane_order(order)
    sp_s = torch.zeros((C, 540), dtype=torch.int16, device=dev)
    sp_d = torch.zeros((C, 540), dtype=torch.int16, device=dev)
    diff = torch.zeros(1, dtype=torch.int64, device=dev)
    ev_s, ev_d = ([pair() for _ in range(N)] for _ in range(2))
    for k in range(N):
        timed(ev_s[k], lambda: se.synth_params_dev(sp_s.data_ptr(), d_rows[k].data_ptr(), None, None, s))
        timed(ev_d[k], lambda: de.decode_dev(sp_d.data_ptr(), d_bits[k].data_ptr(), None, s))
        diff += (sp_s != sp_d).sum()
    torch.cuda.synchronize(dev)
    se.close()
    de.close()
    synth, decode = ms(ev_s), ms(ev_d)
    return {"channels": C, "distinct": bits.shape[1], "steps": K, "warmup": W, "lane_order": int(order),
            "synth": synth, "decode": decode,
            "synth_over_decode": round(synth["median_ms"] / decode["median_ms"], 4),
            "pcm_samples_differing": int(diff.item())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", default="32768,262144")
    ap.add_argument("--distinct", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream(dev).cuda_stream
    bits, rows = content(a.distinct, a.warmup + a.steps, dev, s)
    for C in (int(c) for c in a.channels.split(",")):
        assert C % a.distinct == 0
        for order in (True, False):
            line = json.dumps(run(C, a.warmup, a.steps, order, bits, rows, dev, s))
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
