"""pairphone_amd -- MI355X-native batched MELPe-1200 engine.

The product is libmelpe_amd.so (HIP kernels for gfx950 behind the C ABI in
include/melpe.h and include/melpe_batch.h).  This package is the Python host
mirror of that ABI (pairphone_amd.codec); it has no compute of its own and
raises if the HIP library is missing.
"""
from .codec import (MelpeEngine, Melpe, load_library, LIB_PATH,  # noqa: F401
                    SF_SAMPLES, SF_BYTES, FRAME_SAMPLES, synth_signal)
from .codec import VoiceEnc, VoiceDec, Vad, stream_pack, stream_unpack  # noqa: F401
from .codec import stream_pack_dev, stream_pack_work_bytes  # noqa: F401
from .codec import Link, LINK_RECORD, LINK_REKEY, LINK_STAGE  # noqa: F401
from .codec import RxLine, RX_LINE_RECORD, RX_LINE_INFO, RX_NOLOCK, rx_line_slots  # noqa: F401
from .codec import PAR_WORDS, QPAR_WORDS  # noqa: F401
from . import params  # noqa: F401
