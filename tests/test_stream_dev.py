"""The VAD-framed stream format on the device: melpe_stream_pack_dev (frames
compacted across channels by a three-launch exclusive scan) against the host
melpe_stream_pack, and melpe_rx_stream_dev / MelpeEngine.decode_streams (the
batched melpe_dec.c:33-49) against the reference's unchanged melpe_dec
(oracle/_ref/melpe_dec) on ragged streams.

The reference side is built once per module (ref_vad, ref_tool encgate, the
host stream_pack, melpe_dec) and shared by the GPU tests, which only read it.
"""
import ctypes
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch  # before libmelpe_amd.so is loaded: the process then has one HIP runtime, torch's

from conftest import ROOT, GOLDEN, REF_DIR

sys.path.insert(0, GOLDEN)
from make_vad_golden import ref_vad  # noqa: E402

MELPE_DEC = os.path.join(REF_DIR, "melpe_dec")
C, NSF = 66, 16          # one full wave plus two lanes
FILL = 0xA5
NEW = ("melpe_stream_pack_dev", "melpe_stream_pack_work_bytes", "melpe_rx_stream_dev")


# ---------------------------------------------------------------- CPU ----

def test_exports_work_size_and_bad_arguments(engine_lib):
    lib = engine_lib
    hdr = open(os.path.join(ROOT, "include", "melpe_batch.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    raw = ctypes.CDLL(os.path.join(ROOT, "pairphone_amd", "libmelpe_amd.so"))
    for name in NEW:
        assert hasattr(raw, name), "missing export " + name
        assert re.search(r"\b%s\s*\(" % name, hdr), name + " not declared in melpe_batch.h"

    sizes = [lib.melpe_stream_pack_work_bytes(c) for c in (1, 64, 256, 257, 321, 65536, 65857, 1 << 20)]
    assert all(s > 0 for s in sizes)
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))
    # one block total per 256 channels at least, or the scan overruns d_work
    assert lib.melpe_stream_pack_work_bytes(65857) >= 4 * ((65857 + 255) // 256)

    # never dereferenced: every call below must return before any HIP call
    buf = np.zeros(64, np.uint8)
    p = buf.ctypes.data
    good = [p, p, p, p, p, p]
    for i in range(6):
        args = list(good)
        args[i] = None
        lib.melpe_last_error()
        rc = lib.melpe_stream_pack_dev(*args, 4, None, None)
        assert rc < 0, i
        assert b"melpe_stream_pack_dev" in lib.melpe_last_error()
    assert lib.melpe_stream_pack_dev(*good, 0, None, None) < 0
    # rx: e, stream, pos, end, (pos_next optional), sp, bits, voiced, lens
    good = [p, p, p, p, None, p, p, p, p]
    for i in (0, 1, 2, 3, 5, 6, 7, 8):
        args = list(good)
        args[i] = None
        rc = lib.melpe_rx_stream_dev(*args, None, None)
        assert rc < 0, i
        assert b"melpe_rx_stream_dev" in lib.melpe_last_error()
    from pairphone_amd import stream_pack_dev, MelpeEngine
    assert callable(stream_pack_dev)
    assert callable(MelpeEngine.rx_stream_dev) and callable(MelpeEngine.decode_streams)


# ------------------------------------------------------ reference side ----

def _signals():
    from pairphone_amd import synth_signal
    rng = np.random.default_rng(21)
    x = np.stack([synth_signal(4, c, NSF * 540) for c in range(C)]).reshape(C, NSF, 540)
    for c in range(C):
        for k in rng.choice(NSF, size=4 + c % 9, replace=False):
            x[c, k] = rng.integers(-15, 16, 540)
    return x


@pytest.fixture(scope="module")
def ragged(tmp_path_factory, ref_tool):
    """66 reference-gated channels cut to NSF - c % 5 frames: votes, bits,
    the framed streams and melpe_dec's PCM of each"""
    from pairphone_amd import stream_pack
    tmp = tmp_path_factory.mktemp("ragged")
    x = _signals()
    votes = ref_vad(x.reshape(C, -1), NSF)
    nfr = np.array([NSF - c % 5 for c in range(C)])

    def one(c):
        pcm, gate, out, fi, fo = (str(tmp / ("%s%d" % (n, c))) for n in "pgbso")
        x[c].tofile(pcm)
        (votes[c] > 0).astype(np.uint8).tofile(gate)
        subprocess.run([ref_tool, "encgate", pcm, gate, out], check=True)
        bits = np.fromfile(out, np.uint8).reshape(NSF, 11)
        stream = stream_pack(bits[:nfr[c]], votes[c, :nfr[c]])
        open(fi, "wb").write(stream)
        subprocess.run([MELPE_DEC, fi, fo], check=True, capture_output=True)
        return bits, stream, np.fromfile(fo, np.int16)
    with ThreadPoolExecutor(8) as ex:
        res = list(ex.map(one, range(C)))
    bits = np.stack([r[0] for r in res])
    streams = [r[1] for r in res]
    want = [r[2] for r in res]
    have = np.arange(NSF)[None, :] < nfr[:, None]        # channel c has frame k
    voiced = have & (votes > 0)
    silent = have & (votes == 0)
    # the inputs must exercise every case, or the tests below pass vacuously
    assert voiced.any() and silent.any()
    assert any(voiced[:, k].any() and silent[:, k].any() and (~have[:, k]).any() for k in range(NSF))
    for c in range(C):
        assert len(streams[c]) == 11 * voiced[c].sum() + silent[c].sum()
        assert len(want[c]) == 540 * nfr[c]
    for a in (votes, bits, have, voiced, silent, nfr):
        a.setflags(write=False)
    return dict(votes=votes, bits=bits, streams=streams, want=want, nfr=nfr, have=have,
                voiced=voiced, silent=silent)


# ---------------------------------------------------------------- GPU ----

def _pack_inputs(Cn, rng):
    """three superframes of bits, votes and masks with long all-silent and
    all-voiced runs (whole blocks of equal length) and a fully inactive
    block"""
    bits = rng.integers(0, 256, (3, Cn, 11), dtype=np.uint8)
    bits[:, :, 10] &= 1
    votes = (rng.integers(0, 7, (3, Cn)) * rng.integers(0, 2, (3, Cn))).astype(np.uint8)
    votes[0, 0:300] = 0
    votes[1, Cn - 300:Cn] = 3
    if Cn > 4000:
        for k in range(3):
            votes[k, 1000 + 700 * k:1400 + 700 * k] = 0
            votes[k, 30000 + 700 * k:30400 + 700 * k] = 1 + k
    # superframe 0 unmasked; 1 masked outside its runs only, so the runs stay
    # runs of equal lengths; 2 masked at random
    act = (rng.random((3, Cn)) < 0.8).astype(np.uint8)
    act[1, :40000] = 1
    act[:, 256:512] = 0                      # block 1 is masked out entirely
    return bits, votes, [None, act[1], act[2]]


@pytest.mark.gpu
@pytest.mark.parametrize("Cn", [321, 65857])
def test_gpu_pack_matches_host_pack(Cn):
    from pairphone_amd import load_library, stream_pack_dev, stream_pack_work_bytes
    lib = load_library()
    rng = np.random.default_rng(100 + Cn)
    bits, votes, acts = _pack_inputs(Cn, rng)
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream(dev).cuda_stream
    d_last = torch.zeros(Cn, dtype=torch.uint8, device=dev)
    d_work = torch.zeros(stream_pack_work_bytes(Cn), dtype=torch.uint8, device=dev)
    h_last = np.zeros(Cn, np.uint8)
    for k in range(3):
        h_out = np.zeros((Cn, 11), np.uint8)
        h_lens = np.zeros(Cn, np.uint8)
        act = acts[k]
        assert lib.melpe_stream_pack(bits[k].ctypes.data, votes[k].ctypes.data, h_last.ctypes.data,
                                     h_out.ctypes.data, h_lens.ctypes.data, Cn,
                                     None if act is None else act.ctypes.data) == 0
        want_offs = np.concatenate([[0], np.cumsum(h_lens.astype(np.int64))])
        want_out = np.concatenate([h_out[c, :h_lens[c]] for c in range(Cn)])
        total = int(want_offs[-1])
        assert len(want_out) == total
        assert {1, 11} <= set(np.unique(h_lens)) <= {0, 1, 11}
        assert act is None or (h_lens[256:512] == 0).all()

        d_bits = torch.from_numpy(bits[k]).to(dev)
        d_votes = torch.from_numpy(votes[k]).to(dev)
        d_act = None if act is None else torch.from_numpy(act).to(dev)
        d_out = torch.full((Cn * 11,), FILL, dtype=torch.uint8, device=dev)
        d_offs = torch.full((Cn + 1,), -1, dtype=torch.int32, device=dev)
        stream_pack_dev(d_bits.data_ptr(), d_votes.data_ptr(), d_last.data_ptr(), d_out.data_ptr(),
                        d_offs.data_ptr(), d_work.data_ptr(), Cn,
                        None if d_act is None else d_act.data_ptr(), s)
        torch.cuda.synchronize(dev)
        got_offs = d_offs.cpu().numpy().view(np.uint32).astype(np.int64)
        got_out = d_out.cpu().numpy()
        assert np.array_equal(got_offs, want_offs), k
        assert np.array_equal(got_out[:total], want_out), k
        assert (got_out[total:] == FILL).all(), k
        assert np.array_equal(d_last.cpu().numpy(), h_last), k


@pytest.mark.gpu
@pytest.mark.parametrize("waves", [1, 2])
def test_gpu_decode_streams_matches_reference_melpe_dec(ragged, waves):
    from pairphone_amd import MelpeEngine
    eng = MelpeEngine(C)
    eng.set_dec_waves(waves)
    got = eng.decode_streams(ragged["streams"])
    cursors = eng.last_cursors
    eng.close()
    assert len(got) == C
    for c in range(C):
        assert got[c].dtype == np.int16
        assert np.array_equal(got[c], ragged["want"][c]), c
    assert np.array_equal(cursors, [len(s) for s in ragged["streams"]])


@pytest.mark.gpu
def test_gpu_pack_feeds_rx_on_the_device(ragged):
    from pairphone_amd import MelpeEngine, stream_pack_dev, stream_pack_work_bytes
    have, voiced, silent = ragged["have"], ragged["voiced"], ragged["silent"]
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream(dev).cuda_stream
    d_bits_in = torch.from_numpy(np.ascontiguousarray(ragged["bits"].transpose(1, 0, 2))).to(dev)
    d_votes = torch.from_numpy(np.ascontiguousarray(ragged["votes"].T)).to(dev)
    d_act = torch.from_numpy(np.ascontiguousarray(have.T.astype(np.uint8))).to(dev)
    d_last = torch.zeros(C, dtype=torch.uint8, device=dev)
    d_work = torch.zeros(stream_pack_work_bytes(C), dtype=torch.uint8, device=dev)
    d_out = torch.zeros((NSF, C * 11), dtype=torch.uint8, device=dev)
    d_offs = torch.zeros((NSF, C + 1), dtype=torch.int32, device=dev)
    d_sp = torch.full((NSF, C, 540), 0x5A5A, dtype=torch.int16, device=dev)
    d_bits = torch.full((NSF, C, 11), FILL, dtype=torch.uint8, device=dev)
    d_voiced = torch.full((NSF, C), FILL, dtype=torch.uint8, device=dev)
    d_lens = torch.full((NSF, C), FILL, dtype=torch.uint8, device=dev)
    eng = MelpeEngine(C)
    for k in range(NSF):
        stream_pack_dev(d_bits_in[k].data_ptr(), d_votes[k].data_ptr(), d_last.data_ptr(),
                        d_out[k].data_ptr(), d_offs[k].data_ptr(), d_work.data_ptr(), C,
                        d_act[k].data_ptr(), s)
        eng.rx_stream_dev(d_out[k].data_ptr(), d_offs[k].data_ptr(), d_offs[k].data_ptr() + 4, None,
                          d_sp[k].data_ptr(), d_bits[k].data_ptr(), d_voiced[k].data_ptr(),
                          d_lens[k].data_ptr(), None, s)
    torch.cuda.synchronize(dev)
    eng.close()
    sp = d_sp.cpu().numpy().transpose(1, 0, 2)           # C x NSF x 540
    bits = d_bits.cpu().numpy().transpose(1, 0, 2)
    got_voiced = d_voiced.cpu().numpy().T
    got_lens = d_lens.cpu().numpy().T
    assert np.array_equal(got_voiced, voiced.astype(np.uint8))
    assert np.array_equal(got_lens, np.where(voiced, 11, np.where(silent, 1, 0)))
    for c in range(C):
        n = ragged["nfr"][c]
        assert np.array_equal(sp[c, :n].reshape(-1), ragged["want"][c]), c
        assert (sp[c, n:] == 0x5A5A).all(), c
        assert np.array_equal(bits[c][voiced[c]], ragged["bits"][c][voiced[c]]), c
        assert not bits[c][silent[c]].any(), c
        assert (bits[c, n:] == FILL).all(), c


@pytest.mark.gpu
def test_gpu_rx_truncated_and_ended_channels():
    from pairphone_amd import MelpeEngine
    rng = np.random.default_rng(7)
    frames = rng.integers(0, 256, (3, 11), dtype=np.uint8)
    frames[:, 10] &= 1
    wire = frames.copy()                                   # bytes 0 and 10 swapped
    wire[:, 0], wire[:, 10] = frames[:, 10], frames[:, 0]
    fresh = MelpeEngine(3)
    want = fresh.decode(frames)                            # every channel's first melpe_s
    fresh.close()

    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream(dev).cuda_stream
    # channel 0: a voiced first byte and only 5 more; 1: nothing left; 2: a whole frame
    blob = np.concatenate([wire[0, :6], wire[2]])
    pos = np.array([0, 6, 6], np.int32)
    end = np.array([6, 6, 17], np.int32)
    d_stream = torch.from_numpy(blob).to(dev)
    d_pos, d_end = torch.from_numpy(pos).to(dev), torch.from_numpy(end).to(dev)
    d_next = torch.full((3,), -1, dtype=torch.int32, device=dev)
    d_sp = torch.full((3, 540), 0x5A5A, dtype=torch.int16, device=dev)
    d_bits = torch.full((3, 11), FILL, dtype=torch.uint8, device=dev)
    d_voiced = torch.full((3,), FILL, dtype=torch.uint8, device=dev)
    d_lens = torch.full((3,), FILL, dtype=torch.uint8, device=dev)
    eng = MelpeEngine(3)
    rc = eng.lib.melpe_rx_stream_dev(eng.h, d_stream.data_ptr(), d_pos.data_ptr(), d_end.data_ptr(),
                                     d_next.data_ptr(), d_sp.data_ptr(), d_bits.data_ptr(),
                                     d_voiced.data_ptr(), d_lens.data_ptr(), None, s)
    assert rc == 0
    torch.cuda.synchronize(dev)
    sp = d_sp.cpu().numpy()
    assert list(d_lens.cpu().numpy()) == [0xFF, 0, 11]
    assert list(d_voiced.cpu().numpy()) == [0, 0, 1]
    assert list(d_next.cpu().numpy()) == [0, 6, 17]
    assert (sp[0] == 0x5A5A).all() and (sp[1] == 0x5A5A).all()
    assert np.array_equal(sp[2], want[2])
    got_bits = d_bits.cpu().numpy()
    assert (got_bits[:2] == FILL).all() and np.array_equal(got_bits[2], frames[2])

    # channel 0 now gets its whole frame: its decoder state was not advanced
    d_stream2 = torch.from_numpy(wire[0].copy()).to(dev)
    d_pos2 = torch.from_numpy(np.array([0, 11, 11], np.int32)).to(dev)
    d_end2 = torch.from_numpy(np.array([11, 11, 11], np.int32)).to(dev)
    d_sp.fill_(0x5A5A)
    eng.rx_stream_dev(d_stream2.data_ptr(), d_pos2.data_ptr(), d_end2.data_ptr(), d_pos2.data_ptr(),
                      d_sp.data_ptr(), d_bits.data_ptr(), d_voiced.data_ptr(), d_lens.data_ptr(),
                      None, s)
    torch.cuda.synchronize(dev)
    eng.close()
    sp = d_sp.cpu().numpy()
    assert list(d_lens.cpu().numpy()) == [11, 0, 0]
    assert list(d_pos2.cpu().numpy()) == [11, 11, 11]
    assert np.array_equal(sp[0], want[0])
    assert (sp[1:] == 0x5A5A).all()
