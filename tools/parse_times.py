"""Times of the parameter calls against the full decoder, HIP events around
each call, on the same valid bitstreams (the engine's own encoding of the
synthetic signal):

  parse       melpe_parse_dev
  decode      melpe_decode_dev (the comparator, on a second engine)
  dec_tap     melpe_decode_params_dev after each decode
  enc_tap     melpe_encode_params_dev (par and qpar) on the encoding engine

parse and decode alternate superframe by superframe in one loop, --steps
timed superframes after --warmup.  The last superframe's parsed rows are
compared with the decoder tap's.  Writes one JSON line per channel count;
--out appends them to a file.

  python tools/parse_times.py [--channels 32768,262144] [--out profiles/parse_times.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pairphone_amd import MelpeEngine  # noqa: E402


def stats(ms):
    a = np.sort(np.asarray(ms))
    return {"median_ms": round(float(np.median(a)), 4), "min_ms": round(float(a[0]), 4),
            "max_ms": round(float(a[-1]), 4)}


def run(C, W, K):
    N = W + K
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream(dev).cuda_stream

    def pair():
        return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(ev, fn):
        ev[0].record()
        fn()
        ev[1].record()

    def ms(evs):
        return stats([b.elapsed_time(e) for b, e in evs[W:]])

    # the bits of N superframes of every channel, and the encoder tap
    eng = MelpeEngine(C)
    eng.synth_seed(17)
    pcm = torch.zeros((C, 540), dtype=torch.int16, device=dev)
    bits = torch.zeros((N, C, 11), dtype=torch.uint8, device=dev)
    e_par = torch.zeros((C, 3, 30), dtype=torch.int16, device=dev)
    e_qpar = torch.zeros((C, 30), dtype=torch.int16, device=dev)
    ev_et = [pair() for _ in range(N)]
    for k in range(N):
        eng.synth_dev(pcm.data_ptr(), 540, s)
        eng.encode_dev(bits[k].data_ptr(), pcm.data_ptr(), None, s)
        timed(ev_et[k], lambda: eng.encode_params_dev(e_par.data_ptr(), e_qpar.data_ptr(), None, s))
    torch.cuda.synchronize(dev)
    enc_tap = ms(ev_et)
    eng.close()

    pe, de = MelpeEngine(C), MelpeEngine(C)
    p_par = torch.zeros((C, 3, 30), dtype=torch.int16, device=dev)
    d_par = torch.zeros((C, 3, 30), dtype=torch.int16, device=dev)
    sp = torch.zeros((C, 540), dtype=torch.int16, device=dev)
    ev_p, ev_d, ev_t = ([pair() for _ in range(N)] for _ in range(3))
    for k in range(N):
        timed(ev_p[k], lambda: pe.parse_dev(p_par.data_ptr(), bits[k].data_ptr(), None, s))
        timed(ev_d[k], lambda: de.decode_dev(sp.data_ptr(), bits[k].data_ptr(), None, s))
        timed(ev_t[k], lambda: de.decode_params_dev(d_par.data_ptr(), None, s))
    torch.cuda.synchronize(dev)
    same = bool(torch.equal(p_par, d_par))
    pe.close()
    de.close()
    parse, decode = ms(ev_p), ms(ev_d)
    return {"channels": C, "steps": K, "warmup": W, "parse": parse, "decode": decode,
            "decode_over_parse": round(decode["median_ms"] / parse["median_ms"], 2),
            "dec_tap": ms(ev_t), "enc_tap": enc_tap, "parse_equals_decoder_tap": same}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", default="32768,262144")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    for C in (int(c) for c in a.channels.split(",")):
        line = json.dumps(run(C, a.warmup, a.steps))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
