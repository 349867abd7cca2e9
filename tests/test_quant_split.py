"""The lane analysis split at sc_ana (k_enc_ana -> k_enc_quant -> k_enc_harm
-> k_enc_tail) and the second lane order, by the superframe's current voicing
pattern, that the last three kernels run on (engine.hip ana_launch).

CPU: the host build's three-part split (emu_encode_ana_split, each part on a
pattern-filled frame holding only what the kernel is handed) against the
serial host build, bits and parameters, over channels that show all eight
voicing patterns.

GPU: 150 channels -- two full waves and a ragged third, so the second order
moves channels between waves -- x 12 superframes with the lane kernels forced,
against the reference codec, under no mask, ragged masks, 1 and 65 live
channels and no live channel; the lane order on against off (bits and
records); the pipelined form; and both sides of the live-count threshold
between the four-wave kernel and the lane kernels.

A masked-out channel's state does not move and it consumes no input, so
channel c is fed the next block of its own signal each time it is live, and
its j-th live superframe must give the reference's j-th superframe.
"""
import ctypes
import subprocess

import numpy as np
import pytest

from test_encode import emu, signals

SEED = 2026  # the bench's run seed
C, NSF = 150, 12


# ---------------------------------------------------------------- CPU

def _emu_run(fn, x, nsf):
    """bits [C, nsf, 11] and the parameter taps [C, nsf, 120] (melp_par rows
    and quant_par, emu_enc_params) of the host build's encoder `fn`"""
    lib = emu()
    lib.emu_encode_npp.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.emu_enc_params.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    f = getattr(lib, fn)
    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    ch = x.shape[0]
    e = lib.emu_create(ch)
    bits = np.zeros((ch, nsf, 11), np.uint8)
    taps = np.zeros((ch, nsf, 120), np.int16)
    row = np.zeros(120, np.int16)
    for k in range(nsf):
        sp = np.ascontiguousarray(x[:, k * 540:(k + 1) * 540])
        b = np.zeros((ch, 11), np.uint8)
        if fn != "emu_encode":
            lib.emu_encode_npp(e, sp.ctypes.data)
        assert f(e, b.ctypes.data, sp.ctypes.data) == 0
        bits[:, k] = b
        for c in range(ch):
            assert lib.emu_enc_params(e, c, row.ctypes.data) == 30
            taps[c, k] = row
    lib.emu_destroy(e)
    return bits, taps


def test_three_part_split_hostemu_matches_serial_on_every_voicing_pattern():
    from pairphone_amd.params import UV_FLAG
    ch, nsf = 128, 25
    x = signals(SEED, ch, nsf)
    want_b, want_p = _emu_run("emu_encode", x.copy(), nsf)
    got_b, got_p = _emu_run("emu_encode_ana_split", x.copy(), nsf)
    np.testing.assert_array_equal(got_b, want_b)
    np.testing.assert_array_equal(got_p, want_p)
    uv = (want_p[:, :, :90].reshape(ch, nsf, 3, 30)[..., UV_FLAG] != 0).astype(int)
    pattern = uv[..., 0] * 4 + uv[..., 1] * 2 + uv[..., 2]
    seen = np.bincount(pattern.ravel(), minlength=8)
    assert (seen > 0).all(), "voicing patterns seen (uvc 0..7): %s" % seen.tolist()


# ---------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def stream():
    """the 150 channels' signals, [C, NSF, 540]"""
    # a module fixture runs ahead of conftest's per-test _torch_hip_first, and
    # the signal generator loads the engine library: torch's HIP context first
    import torch
    if torch.cuda.is_available():
        torch.cuda.init()
    return signals(SEED, C, NSF).reshape(C, NSF, 540)


@pytest.fixture(scope="module")
def ref_bits(tmp_path_factory, ref_tool):
    """the reference codec on the same channels, [C, NSF, 11]"""
    p = str(tmp_path_factory.mktemp("quant_split") / "ref.bits")
    subprocess.run([ref_tool, "jobs", "16", "encgen", str(SEED), "0", str(C), str(NSF), p], check=True)
    return np.fromfile(p, dtype=np.uint8).reshape(C, NSF, 11)


def _masks(kind):
    """[NSF, C] activity masks (None: no mask)"""
    rng = np.random.default_rng(31)
    if kind == "none":
        return None
    m = np.zeros((NSF, C), np.uint8)
    if kind == "ragged":  # another live set every superframe
        for k in range(NSF):
            m[k] = rng.random(C) < (0.3 + 0.05 * k)
    elif kind == "one":
        m[:, 77] = 1
    elif kind == "65":
        m[:, rng.choice(C, 65, replace=False)] = 1
    return m


def _feed(stream, masks):
    """the PCM of each superframe, [NSF, C, 540]: a live channel's next
    unread block; and the block index each (superframe, channel) ran"""
    live = np.ones((NSF, C), np.uint8) if masks is None else masks
    idx = np.cumsum(live, axis=0) - live  # live superframes before this one
    pcm = np.zeros((NSF, C, 540), np.int16)
    for k in range(NSF):
        pcm[k] = stream[np.arange(C), idx[k]]
    return pcm, idx, live.astype(bool)


def _encode(stream, masks, order=None, waves=1, live_max=None, pipe=False, records=False, choice=None):
    """bits [NSF, C, 11] (0xAB where nothing was written) of the engine under
    `masks`; with records, the exported encoder records too"""
    import torch
    from pairphone_amd import MelpeEngine
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream(dev).cuda_stream
    pcm, _, _ = _feed(stream, masks)
    x = torch.from_numpy(pcm).to(dev)
    m = None if masks is None else torch.from_numpy(masks).to(dev)
    bits = torch.full((NSF, C, 11), 0xAB, dtype=torch.uint8, device=dev)
    eng = MelpeEngine(C)
    eng.set_ana_waves(waves)
    if order is not None:
        eng.set_lane_order(order)
    if live_max is not None:
        eng.set_mw_live_max(live_max)

    def act(k):
        return None if m is None or k >= NSF else m[k].data_ptr()
    if pipe:
        eng.encode_npp_dev(x[0].data_ptr(), act(0), s)
    for k in range(NSF):
        if pipe:
            eng.encode_pipe_dev(bits[k].data_ptr(), x[k].data_ptr(),
                                x[k + 1].data_ptr() if k + 1 < NSF else None, act(k), act(k + 1), s)
        else:
            eng.encode_dev(bits[k].data_ptr(), x[k].data_ptr(), act(k), s)
        if choice is not None:
            choice.append(eng.last_ana_waves())
    torch.cuda.synchronize(dev)
    rec = eng.export_state(1) if records else None
    eng.close()
    b = bits.cpu().numpy()
    return (b, rec) if records else b


def _check_against_reference(bits, stream, masks, ref_bits):
    _, idx, live = _feed(stream, masks)
    for k in range(NSF):
        want = ref_bits[np.arange(C), idx[k]]
        np.testing.assert_array_equal(bits[k][live[k]], want[live[k]], err_msg="bits, superframe %d" % k)
        assert (bits[k][~live[k]] == 0xAB).all(), "a masked channel's bits were written (superframe %d)" % k


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["none", "ragged", "one", "65"])
def test_lane_kernels_150_channels_match_reference(kind, stream, ref_bits):
    masks = _masks(kind)
    if kind == "one":
        assert masks.sum(axis=1).tolist() == [1] * NSF
    if kind == "65":
        assert masks.sum(axis=1).tolist() == [65] * NSF
    choice = []
    bits = _encode(stream, masks, choice=choice)
    assert choice == [1] * NSF
    _check_against_reference(bits, stream, masks, ref_bits)


@pytest.mark.gpu
def test_no_live_channel_moves_no_state(stream, ref_bits):
    """superframe 0 under an all-zero mask, then the stream from its start:
    the masked call wrote nothing and every channel starts from reset"""
    import torch
    from pairphone_amd import MelpeEngine
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream(dev).cuda_stream
    eng = MelpeEngine(C)
    eng.set_ana_waves(1)
    before = eng.export_state(1)
    x = torch.from_numpy(np.ascontiguousarray(stream[:, 0])).to(dev)
    zero = torch.zeros(C, dtype=torch.uint8, device=dev)
    bits = torch.full((2, C, 11), 0xAB, dtype=torch.uint8, device=dev)
    eng.encode_dev(bits[0].data_ptr(), x.data_ptr(), zero.data_ptr(), s)
    torch.cuda.synchronize(dev)
    np.testing.assert_array_equal(eng.export_state(1), before)
    np.testing.assert_array_equal(x.cpu().numpy(), stream[:, 0])
    eng.encode_dev(bits[1].data_ptr(), x.data_ptr(), None, s)
    torch.cuda.synchronize(dev)
    eng.close()
    b = bits.cpu().numpy()
    assert (b[0] == 0xAB).all()
    np.testing.assert_array_equal(b[1], ref_bits[:, 0])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["none", "ragged"])
def test_lane_order_on_and_off_agree(kind, stream):
    masks = _masks(kind)
    b_off, r_off = _encode(stream, masks, order=False, records=True)
    b_on, r_on = _encode(stream, masks, order=True, records=True)
    np.testing.assert_array_equal(b_on, b_off)
    np.testing.assert_array_equal(r_on, r_off)


@pytest.mark.gpu
def test_pipelined_form_matches_encode_dev(stream):
    want = _encode(stream, None)
    got = _encode(stream, None, pipe=True)
    np.testing.assert_array_equal(got, want)


@pytest.mark.gpu
def test_live_count_threshold_both_sides(stream, ref_bits):
    """a live-count threshold of 100 on the 150-channel engine: superframes
    with 100 live channels run the four-wave kernel, those with 101 the lane
    kernels (both enqueued, the device's live count decides)"""
    rng = np.random.default_rng(32)
    masks = np.zeros((NSF, C), np.uint8)
    n = [100 if k % 2 == 0 else 101 for k in range(NSF)]
    for k in range(NSF):
        masks[k, rng.choice(C, n[k], replace=False)] = 1
    choice = []
    bits = _encode(stream, masks, waves=0, live_max=100, choice=choice)
    assert choice == [4 if v <= 100 else 1 for v in n], choice
    _check_against_reference(bits, stream, masks, ref_bits)
