"""Speech from parameter tensors on the GPU (melpe_synth_params_dev /
_host, k_dec.hip): against the reference's SKIP_CHANNEL synthesis
(tests/golden/synpar.json), the reference decoder's goldens (dec_1024.json)
and the host build of the same device code, every channel and sample.

The row recipe and the host forms come from tests/golden/
make_synpar_golden.py and tests/test_synth_params.py.
"""
import ctypes

import numpy as np
import pytest

from test_decode import gold, sha
from test_encode import golden as enc_golden, signals
from test_synth_params import emu_synth_all, msg

C_GPU = 200         # three full waves and a tail of 8
K = msg.K
SENTINEL = 0x5A5A
FUZZ_C, FUZZ_K = 128, 8
CHECK_SEED, CHECK_TOTAL = 0x53594E50, 100000     # tests/native/synpar_check.cpp

_cache = {}


def case200():
    """(rows [200, K, 90], the host build's pcm [200, K * 540], status, melp_par afterwards)"""
    if "case" not in _cache:
        rows = msg.case_rows(C_GPU, K)
        _cache["case"] = (rows,) + emu_synth_all("emu_synth_params", rows)
    return _cache["case"]


def gpu_synth(rows, waves=0, order=None, tap=False):
    """rows [C, K, 90] through melpe_synth_params_dev, one sync at the end:
    (pcm [C, K * 540], status [C, K], melp_par afterwards [C, K, 90] if tap)"""
    import torch
    from pairphone_amd import MelpeEngine
    C, nsf = rows.shape[:2]
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream(dev).cuda_stream
    d_par = torch.from_numpy(np.ascontiguousarray(rows.transpose(1, 0, 2))).to(dev)
    keep = d_par.clone()
    d_sp = torch.zeros((nsf, C, 540), dtype=torch.int16, device=dev)
    d_st = torch.full((nsf, C), 9, dtype=torch.uint8, device=dev)
    d_post = torch.zeros((nsf, C, 90), dtype=torch.int16, device=dev)
    eng = MelpeEngine(C)
    if waves:
        eng.set_dec_waves(waves)
    if order is not None:
        eng.set_lane_order(order)
    for k in range(nsf):
        eng.synth_params_dev(d_sp[k].data_ptr(), d_par[k].data_ptr(), d_st[k].data_ptr(), None, s)
        if tap:
            eng.decode_params_dev(d_post[k].data_ptr(), None, s)
    torch.cuda.synchronize(dev)
    eng.close()
    assert torch.equal(d_par, keep), "the input tensor was written"
    pcm = d_sp.cpu().numpy().transpose(1, 0, 2).reshape(C, nsf * 540)
    return pcm, d_st.cpu().numpy().T, d_post.cpu().numpy().transpose(1, 0, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("order", [True, False])
@pytest.mark.parametrize("waves", [1, 2])
def test_synth_gpu_matches_fixture_and_host_build(waves, order):
    g = gold("synpar.json")
    rows, want_pcm, want_st, want_post = case200()
    pcm, st, post = gpu_synth(rows, waves, order, tap=True)
    for c in range(msg.C):
        assert sha(pcm[c]) == g["pcm_sha256"][c], "fixture PCM, channel %d (kind %d)" % (c, c % 4)
        assert sha(post[c]) == g["post_sha256"][c], "fixture melp_par, channel %d (kind %d)" % (c, c % 4)
    bad = sorted(set(np.argwhere(pcm != want_pcm)[:, 0].tolist()))
    assert not bad, "PCM differs from the host build on %d channels, first %s" % (len(bad), bad[:8])
    assert not st.any() and np.array_equal(st, want_st)
    bad = sorted(set(np.argwhere(post != want_post)[:, 0].tolist()))
    assert not bad, "melp_par after the call differs on %d channels, first %s" % (len(bad), bad[:8])


def golden_rows():
    """the 1,024-channel golden set encoded on the GPU (bits checked against
    enc_1024.json), then the channel reader's rows of those bits by the host
    build: [1024, 149, 90]"""
    if "gold" not in _cache:
        from pairphone_amd import MelpeEngine
        ge = enc_golden()
        C, nsf = ge["channels"], ge["superframes"]
        x = signals(ge["seed"], C, nsf)
        eng = MelpeEngine(C)
        bits = np.zeros((C, nsf, 11), np.uint8)
        for k in range(nsf):
            bits[:, k] = eng.encode(np.ascontiguousarray(x[:, k * 540:(k + 1) * 540]))
        eng.close()
        for c in range(C):
            assert sha(bits[c]) == ge["bits_sha256"][c], "bitstream of channel %d" % c
        rows, erase = msg.reader_rows(bits)
        assert not erase.any()
        _cache["gold"] = rows
    return _cache["gold"]


@pytest.mark.gpu
@pytest.mark.parametrize("waves", [1, 2])
def test_synth_gpu_goldens_through_reader_rows(waves):
    """reader rows -> synth_params gives the reference's own decode of the
    golden bitstreams, all 1,024 channels"""
    gd = gold("dec_1024.json")
    pcm, st, _ = gpu_synth(golden_rows(), waves)
    assert not st.any()
    bad = [c for c in range(pcm.shape[0]) if sha(pcm[c]) != gd["pcm_sha256"][c]]
    assert not bad, "%d channels differ from dec_1024.json, first %s" % (len(bad), bad[:8])


@pytest.mark.gpu
def test_synth_gpu_ragged_mask():
    """random per-superframe masks, a cursor per channel: every channel's PCM
    is the unmasked run's; PCM and status of inactive channels untouched"""
    from pairphone_amd import MelpeEngine
    rows, want_pcm, _, _ = case200()
    rng = np.random.default_rng(13)
    act = rng.random((K + 16, C_GPU)) < 0.6
    eng = MelpeEngine(C_GPU)
    pos = np.zeros(C_GPU, int)
    for k in range(act.shape[0]):
        m = (act[k] & (pos < K)).astype(np.uint8)
        par = np.zeros((C_GPU, 3, 30), np.int16)
        for c in np.flatnonzero(m):
            par[c] = rows[c, pos[c]].reshape(3, 30)
        sp = np.full((C_GPU, 540), SENTINEL, np.int16)
        st = np.full(C_GPU, 0x5A, np.uint8)
        eng.synth_params(par, m, sp, st)
        off = m == 0
        assert (sp[off] == SENTINEL).all() and (st[off] == 0x5A).all(), \
            "step %d: PCM or status of an inactive channel was written" % k
        assert not st[~off].any()
        for c in np.flatnonzero(m):
            np.testing.assert_array_equal(sp[c], want_pcm[c, pos[c] * 540:(pos[c] + 1) * 540],
                                          err_msg="channel %d superframe %d" % (c, pos[c]))
            pos[c] += 1
    eng.close()
    assert (pos > K // 3).all()


@pytest.mark.gpu
def test_synth_host_form_status_and_const_input():
    from pairphone_amd import MelpeEngine
    rows, want_pcm, _, _ = case200()
    eng = MelpeEngine(C_GPU)
    for k in range(3):
        par = np.ascontiguousarray(rows[:, k]).reshape(C_GPU, 3, 30)
        keep = par.copy()
        st = np.full(C_GPU, 9, np.uint8)
        sp = eng.synth_params(par, status=st)
        assert par.tobytes() == keep.tobytes(), "the input rows were written"
        assert not st.any()
        np.testing.assert_array_equal(sp, want_pcm[:, k * 540:(k + 1) * 540])
    assert eng.synth_params(np.ascontiguousarray(rows[:, 3]).reshape(C_GPU, 3, 30)).shape == (C_GPU, 540)
    eng.close()


def splitmix64(x):
    x = (x + np.uint64(0x9E3779B97F4A7C15))
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def check_rows(first, count):
    """superframes [first, first + count) of synpar_check.cpp's stream: [count, 90] int16"""
    with np.errstate(over="ignore"):
        i = np.uint64(CHECK_SEED) + np.uint64(90) * np.uint64(first) + np.arange(count * 90, dtype=np.uint64)
        w = (splitmix64(i) >> np.uint64(48)).astype(np.uint16).view(np.int16).reshape(count, 3, 30).copy()
    if first >= CHECK_TOTAL:
        w[..., msg.UV] &= 1
    return w.reshape(count, 90)


@pytest.mark.gpu
def test_synth_gpu_out_of_range_rows_equal_host_build():
    """Full-range random rows: PCM and status equal the host build's, in both
    mappings.  The rows are superframes of the very stream that
    tests/native/synpar_check.cpp (tests/test_synth_params.py
    test_synthesis_is_total_on_any_rows) synthesises under AddressSanitizer and
    UBSan -- the first 512 of its uniformly random part and the first 512 of
    its part with the voiced paths open -- and that test passed on the host
    before this one was first run on a GPU.  It checks equality; it is not a
    probe."""
    n = FUZZ_C * FUZZ_K // 2
    rows = np.concatenate([check_rows(0, n), check_rows(CHECK_TOTAL, n)]).reshape(FUZZ_K, FUZZ_C, 90)
    rows = np.ascontiguousarray(rows.transpose(1, 0, 2))
    assert (rows.reshape(-1, 30)[:, msg.UV] == 0).sum() > 100
    want_pcm, want_st, _ = emu_synth_all("emu_synth_params", rows)
    assert want_st.all(), "every channel's rows need clamping somewhere"
    for waves in (1, 2):
        pcm, st, _ = gpu_synth(rows, waves)
        bad = sorted(set(np.argwhere(pcm != want_pcm)[:, 0].tolist()))
        assert not bad, "waves %d: PCM differs from the host build on channels %s" % (waves, bad[:8])
        assert np.array_equal(st, want_st), "waves %d: status" % waves


@pytest.mark.gpu
def test_synth_scratch_is_reserved_at_create():
    """the synthesis kernels' private bytes are inside what the engine
    reserved at create, and the first call does not move the device's scratch
    limit"""
    import torch
    from pairphone_amd import MelpeEngine, load_library
    lib = load_library()
    hip = lib       # the HIP runtime the engine is linked against, through the engine's own handle
    hip.hipDeviceGetLimit.argtypes = [ctypes.POINTER(ctypes.c_size_t), ctypes.c_int]
    SCRATCH_CURRENT = 0x1002        # hipExtLimitScratchCurrent

    def limit():
        v = ctypes.c_size_t(0)
        assert hip.hipDeviceGetLimit(ctypes.byref(v), SCRATCH_CURRENT) == 0
        return v.value

    C = 4096
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream(dev).cuda_stream
    d_par = torch.from_numpy(np.ascontiguousarray(np.tile(msg.case_rows()[0, 0], (C, 1)))).to(dev)
    d_sp = torch.zeros((C, 540), dtype=torch.int16, device=dev)
    for waves in (1, 2):
        eng = MelpeEngine(C)
        eng.set_dec_waves(waves)
        before = limit()
        need = lib.melpe_synth_params_private_bytes(waves)
        assert 0 < need and need * 64 * waves * (C // 64) <= before
        eng.synth_params_dev(d_sp.data_ptr(), d_par.data_ptr(), None, None, s)
        torch.cuda.synchronize(dev)
        assert limit() == before
        eng.close()


ALT_STEPS = 4       # synth, decode, synth, decode


def alternation_case():
    """One engine serving both sources: 4 superframes on C_GPU channels,
    steps 0 and 2 the synthesis from the fixture's rows (tiled), steps 1 and 3
    the decode of the golden bitstreams (tiled), every step under a ragged mask
    of its own.  Expected values from the host build doing the same, a
    one-channel engine per channel (its forms take no mask):
    (rows [2, C, 90], bits [2, C, 11], masks [4, C], pcm [4, C, 540] and
    status [2, C] with the sentinels where a channel is inactive, melp_par
    afterwards [C, 90])"""
    if "alt" not in _cache:
        vp = ctypes.c_void_p
        lib = msg.emu()
        lib.emu_decode.argtypes = [vp, vp, vp]
        lib.emu_dec_params.argtypes = [vp, ctypes.c_int, vp]
        src = msg.case_rows()
        ge = enc_golden()
        rows = np.ascontiguousarray(np.stack([src[c % msg.C, :2] for c in range(C_GPU)]).transpose(1, 0, 2))
        gb = np.stack([np.frombuffer(bytes.fromhex(h), np.uint8)[:22] for h in ge["bits_hex"]])
        bits = np.stack([gb[c % len(gb)] for c in range(C_GPU)]).reshape(C_GPU, 2, 11)
        bits = np.ascontiguousarray(bits.transpose(1, 0, 2))
        masks = (np.random.default_rng(29).random((ALT_STEPS, C_GPU)) < 0.6).astype(np.uint8)
        assert all((masks[a] != masks[b]).any() for a in range(ALT_STEPS) for b in range(a))
        assert all(0 < masks[k, 192:].sum() < 8 for k in range(ALT_STEPS)), "the tail wave is ragged in every step"
        pcm = np.full((ALT_STEPS, C_GPU, 540), SENTINEL, np.int16)
        status = np.full((2, C_GPU), 0x5A, np.uint8)
        post = np.zeros((C_GPU, 90), np.int16)
        for c in range(C_GPU):
            e = lib.emu_create(1)
            for k in range(ALT_STEPS):
                if not masks[k, c]:
                    continue
                sp = np.zeros(540, np.int16)
                if k % 2 == 0:
                    r, st = rows[k // 2, c].copy(), np.full(1, 9, np.uint8)
                    assert lib.emu_synth_params(e, sp.ctypes.data, r.ctypes.data, st.ctypes.data) == 0
                    status[k // 2, c] = st[0]
                else:
                    b = bits[k // 2, c].copy()
                    assert lib.emu_decode(e, sp.ctypes.data, b.ctypes.data) == 0
                pcm[k, c] = sp
            lib.emu_dec_params(e, 0, post[c].ctypes.data)
            lib.emu_destroy(e)
        _cache["alt"] = (rows, bits, masks, pcm, status, post)
    return _cache["alt"]


@pytest.mark.gpu
@pytest.mark.parametrize("order", [True, False])
@pytest.mark.parametrize("waves", [1, 2])
def test_synth_and_decode_alternate_on_one_engine(waves, order):
    """synth_params_dev and decode_dev superframe by superframe on a single
    engine of 200 channels (three full waves and 8 lanes: the lane grid's last
    wave is partial, the two-wave grid's last workgroup holds a full group and
    an 8-lane one), each call under its own ragged mask: the one BinBuf, the
    one hand-over buffer and the one launch path serve both sources.  PCM,
    status bytes and the final melp_par equal the host build's; nothing of an
    inactive channel is written."""
    import torch
    from pairphone_amd import MelpeEngine
    rows, bits, masks, want_pcm, want_st, want_post = alternation_case()
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream(dev).cuda_stream
    d_rows, d_bits, d_masks = (torch.from_numpy(a).to(dev) for a in (rows, bits, masks))
    d_sp = torch.full((ALT_STEPS, C_GPU, 540), SENTINEL, dtype=torch.int16, device=dev)
    d_st = torch.full((2, C_GPU), 0x5A, dtype=torch.uint8, device=dev)
    d_post = torch.zeros((C_GPU, 90), dtype=torch.int16, device=dev)
    eng = MelpeEngine(C_GPU)
    eng.set_dec_waves(waves)
    eng.set_lane_order(order)
    for k in range(ALT_STEPS):
        if k % 2 == 0:
            eng.synth_params_dev(d_sp[k].data_ptr(), d_rows[k // 2].data_ptr(), d_st[k // 2].data_ptr(),
                                 d_masks[k].data_ptr(), s)
        else:
            eng.decode_dev(d_sp[k].data_ptr(), d_bits[k // 2].data_ptr(), d_masks[k].data_ptr(), s)
    eng.decode_params_dev(d_post.data_ptr(), None, s)
    torch.cuda.synchronize(dev)
    eng.close()
    pcm, st, post = d_sp.cpu().numpy(), d_st.cpu().numpy(), d_post.cpu().numpy()
    for k in range(ALT_STEPS):
        off = masks[k] == 0
        assert (pcm[k, off] == SENTINEL).all(), "step %d: PCM of an inactive channel was written" % k
        if k % 2 == 0:
            assert (st[k // 2, off] == 0x5A).all(), "step %d: status of an inactive channel was written" % k
        bad = sorted(set(np.argwhere(pcm[k] != want_pcm[k])[:, 0].tolist()))
        assert not bad, "step %d: PCM differs from the host build on %d channels, first %s" % (k, len(bad), bad[:8])
    assert np.array_equal(st, want_st), "status"
    bad = sorted(set(np.argwhere(post != want_post)[:, 0].tolist()))
    assert not bad, "melp_par after the calls differs on %d channels, first %s" % (len(bad), bad[:8])
