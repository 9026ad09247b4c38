"""Drop-in for the reference's `audio_processing.py` (data.py:27 does `from audio_processing import
TacotronSTFT`): same names and contracts, HIP kernels underneath -- the mel front end, STFT.transform /
inverse / forward, `griffin_lim` on the device and the host `window_sumsquare` (audio_processing.py:7-75,
237-270).  TacotronSTFT.mel_to_audio (an addition) vocodes model output with Griffin-Lim."""
from flowtron_amd.audio import (STFT, TacotronSTFT, dynamic_range_compression,  # noqa: F401
                                dynamic_range_decompression, griffin_lim, window_sumsquare)

for _cls in (STFT, TacotronSTFT):
    _cls.__module__ = "audio_processing"
