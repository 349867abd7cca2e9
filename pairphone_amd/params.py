"""The codec parameter rows of the engine (include/melpe_batch.h): field
slices by name, and the conversion of a parameter tensor to physical units.

A parameter row is PAR_WORDS = 30 int16 per frame in melp_param order
(melpe/sc1200.h:233); MelpeEngine.encode_params / decode_params / parse give
[C, 3, 30].  The quantiser indices are QPAR_WORDS = 30 int16 per superframe
in quant_param's field order, [C, 30].

    par = eng.parse(bits)
    voiced = par[..., UV_FLAG] == 0
    f0 = to_physical(torch.from_numpy(par))["pitch_hz"]
"""

PAR_WORDS = 30
QPAR_WORDS = 30
FRAMES = 3
SAMPLE_RATE = 8000.0

# one frame's row (last axis of a [..., 30] parameter array)
PITCH = 0               # Q7, samples
LSF = slice(1, 11)      # Q15, 1.0 = half the sample rate
GAIN = slice(11, 13)    # Q8, dB
JITTER = 13             # Q15
BPVC = slice(14, 19)    # Q14
UV_FLAG = 19            # 1 = unvoiced
FS_MAG = slice(20, 30)  # Q13

PAR_FIELDS = {"pitch": PITCH, "lsf": LSF, "gain": GAIN, "jitter": JITTER, "bpvc": BPVC,
              "uv_flag": UV_FLAG, "fs_mag": FS_MAG}

# one superframe's quantiser indices (last axis of a [..., 30] index array)
Q_PITCH = 0
Q_LSF = slice(1, 13)        # [3 frames][4 stages]
Q_GAIN = slice(13, 15)
Q_JITTER = slice(15, 18)
Q_BPVC = slice(18, 21)
Q_FS = 21
Q_UV_FLAG = slice(22, 25)
Q_MSVQ = slice(25, 29)
Q_FSVQ = 29

QPAR_FIELDS = {"pitch_index": Q_PITCH, "lsf_index": Q_LSF, "gain_index": Q_GAIN,
               "jit_index": Q_JITTER, "bpvc_index": Q_BPVC, "fs_index": Q_FS,
               "uv_flag": Q_UV_FLAG, "msvq_index": Q_MSVQ, "fsvq_index": Q_FSVQ}


def to_physical(par):
    """A parameter tensor ([..., 30] int16, any device) in physical units, as
    a dict of float32 tensors (uv_flag: bool) with the same leading axes:

      pitch_hz  fundamental frequency, 8000 / the pitch period (Q7 samples);
                an unvoiced frame carries the codec's default period of 50
                samples, so mask with ~uv_flag for a pitch track
      lsf_hz    the ten line spectral frequencies (Q15 of 4000 Hz)
      gain_db   the two subframe gains (Q8 dB)
      jitter    pitch jitter as a fraction of the period (Q15)
      bpvc      the five band-pass voicing strengths, 0..1 (Q14)
      uv_flag   True = unvoiced
      fs_mag    the ten Fourier magnitudes, 1.0 = flat (Q13)

    A convenience for feature pipelines, not a codec path."""
    import torch
    if par.shape[-1] != PAR_WORDS or par.dtype != torch.int16:
        raise ValueError("to_physical takes an int16 tensor of [..., %d] parameter rows" % PAR_WORDS)
    f = par.to(torch.float32)
    return {
        "pitch_hz": SAMPLE_RATE * 128.0 / f[..., PITCH].clamp(min=1.0),
        "lsf_hz": f[..., LSF] * (SAMPLE_RATE / 2.0 / 32768.0),
        "gain_db": f[..., GAIN] / 256.0,
        "jitter": f[..., JITTER] / 32768.0,
        "bpvc": f[..., BPVC] / 16384.0,
        "uv_flag": par[..., UV_FLAG] != 0,
        "fs_mag": f[..., FS_MAG] / 8192.0,
    }
