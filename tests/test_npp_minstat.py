"""NPP minimum statistics (npp.h npp_min_search_val, npp_wave.h NppMinRegs):
the minimum search on values against the reference run live.

The input is synth_signal under a noise floor that steps up and down, each
channel at its own frames (stepped_input), to take the rare arm of the
minimum search (localflag set, the sub-minimum between the ring's minimum and
`slope` times it, the ring refilled whole).  Counted with a scratch build of
the host emulation that counts inside npp_min_search_val (bin-frames, 144
frames x 129 bins per channel):
  - the rare arm, 8 channels: 27, 93, 60, 111, 89, 151, 143, 173 times (all 8
    channels, 847 in all); 64 channels: every channel, 10,868 in all;
  - the plain synth_signal takes it too (8 channels: 45, 30, 74, 242, 35, 55,
    39, 52; 64 channels: every channel, 6,018 in all), so the steps are not
    what makes the arm reachable; they take it more often;
  - the first compare (new value below act_min), 8 channels, [no, yes] by
    minspec_counter: 0 [11119, 5393], 2 [5110, 11402], 3 [7857, 8655],
    4 [8759, 7753], 5 [9388, 7124], 6 [9781, 6731], 7 [10422, 6090],
    8 [10546, 5966]; the fewest in any one channel is 550.  Phase 1 has no
    compare: it takes the new value unconditionally.

CPU: the host emulation (emu_npp), 8 channels x 144 frames = two ring periods
of 8 windows x 9 frames.  GPU: 64 channels x 144 frames through
MelpeEngine.npp in calls of 1, 2, 4 and 7 frames, cycling, so the 9-frame
window falls on every position inside a call and the register copies' write-
back and reload are crossed at every phase; then the same input through
encode_npp_dev (three frames per call) on a second engine, whose NPP output
and exported records must equal the first engine's.
"""
import numpy as np
import pytest

from conftest import run_ref
from test_npp import emu

SEED = 41
FRAMES = 144
HOP = 180
CPU_CHANNELS = 8
GPU_CHANNELS = 64
LEVELS = (90, 180, 360, 180, 90, 256, 724, 256)  # noise amplitude, cycled


def stepped_input(channels, frames):
    """synth_signal at a quarter of its level plus uniform noise whose
    amplitude steps through LEVELS every 7 + 3 (c % 16) frames, starting
    c % 8 levels in: integer arithmetic on a fixed generator"""
    from pairphone_amd import synth_signal
    n = frames * HOP + 76
    out = np.zeros((channels, n), np.int16)
    for c in range(channels):
        rng = np.random.RandomState(SEED * 1000 + c)
        u = rng.randint(-32768, 32768, n).astype(np.int64)
        period = (7 + 3 * (c % 16)) * HOP
        lev = np.array(LEVELS, np.int64)[((np.arange(n) // period) + c % 8) % len(LEVELS)]
        x = (synth_signal(SEED, c, n).astype(np.int64) >> 2) + ((u * lev) >> 15)
        out[c] = np.clip(x, -32768, 32767)
    return out


_cache = {}


def live(channels, tmp_path_factory):
    """(input, reference output) of the first `channels` channels; the
    reference keeps its state in process globals, so one process per channel,
    each run once per session"""
    if "x" not in _cache:
        _cache["x"] = stepped_input(GPU_CHANNELS, FRAMES)
        _cache["x"].flags.writeable = False  # shared among the tests: they work on copies
    x = _cache["x"]
    ref = _cache.setdefault("ref", {})
    tmp = None
    for c in range(channels):
        if c not in ref:
            tmp = tmp or tmp_path_factory.mktemp("minstat")
            p = str(tmp / ("c%d.pcm" % c))
            x[c].tofile(p)
            run_ref("npp", p, p + ".out")
            ref[c] = np.fromfile(p + ".out", dtype=np.int16)
            assert ref[c].size == FRAMES * HOP
    return x[:channels], np.stack([ref[c] for c in range(channels)])


def test_minstat_hostemu_matches_reference_live(tmp_path_factory, ref_tool):
    x, ref = live(CPU_CHANNELS, tmp_path_factory)
    y = x.copy()  # the shared input stays as it is
    lib = emu()
    e = lib.emu_create(CPU_CHANNELS)
    lib.emu_npp(e, y.ctypes.data, FRAMES, y.shape[1], 1)
    lib.emu_destroy(e)
    for c in range(CPU_CHANNELS):
        np.testing.assert_array_equal(y[c, :FRAMES * HOP], ref[c], err_msg="channel %d" % c)


def chunked(tmp_path_factory):
    """engine A: the input through MelpeEngine.npp in calls of 1, 2, 4, 7
    frames; returns (input, reference, A's output, A's encoder records).
    Run once, by the first GPU test that asks (inside the test, so after
    conftest has brought up torch's HIP context)."""
    from pairphone_amd import MelpeEngine
    if "chunked" in _cache:
        return _cache["chunked"]
    x, ref = live(GPU_CHANNELS, tmp_path_factory)
    eng = MelpeEngine(GPU_CHANNELS)
    out = np.zeros((GPU_CHANNELS, FRAMES * HOP), np.int16)
    f, k = 0, 0
    while f < FRAMES:
        n = min((1, 2, 4, 7)[k % 4], FRAMES - f)
        a = x[:, f * HOP:(f + n) * HOP + 76].copy()
        eng.npp(a, n)
        out[:, f * HOP:(f + n) * HOP] = a[:, :n * HOP]
        f, k = f + n, k + 1
    rec = eng.export_state(1)
    eng.close()
    _cache["chunked"] = (x, ref, out, rec)
    return _cache["chunked"]


@pytest.mark.gpu
def test_minstat_gpu_chunked_matches_reference_live(tmp_path_factory, ref_tool):
    x, ref, out, rec = chunked(tmp_path_factory)
    for c in range(GPU_CHANNELS):
        np.testing.assert_array_equal(out[c], ref[c], err_msg="channel %d" % c)


@pytest.mark.gpu
def test_minstat_gpu_encode_npp_same_output_and_records(tmp_path_factory, ref_tool):
    import torch
    from pairphone_amd import MelpeEngine
    x, ref, out, rec = chunked(tmp_path_factory)
    nsf = FRAMES // 3
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream(dev).cuda_stream
    d = torch.from_numpy(np.ascontiguousarray(
        x[:, :nsf * 540].reshape(GPU_CHANNELS, nsf, 540).transpose(1, 0, 2))).to(dev)
    eng = MelpeEngine(GPU_CHANNELS)
    for k in range(nsf):
        eng.encode_npp_dev(d[k].data_ptr(), None, s)
    torch.cuda.synchronize(dev)
    rec2 = eng.export_state(1)
    eng.close()
    y = d.cpu().numpy().transpose(1, 0, 2).reshape(GPU_CHANNELS, nsf * 540)
    for c in range(GPU_CHANNELS):
        np.testing.assert_array_equal(y[c], out[c], err_msg="channel %d" % c)
    np.testing.assert_array_equal(rec2, rec)
