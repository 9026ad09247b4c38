"""Drop-in for the reference's `audio_processing.py` (data.py:27 does `from audio_processing import
TacotronSTFT`): same names and contracts, HIP kernels underneath -- the mel front end, STFT.transform /
inverse / forward, `griffin_lim` on the device and the host `window_sumsquare` (audio_processing.py:7-75,
237-270).  TacotronSTFT.mel_to_audio (an addition) vocodes model output with Griffin-Lim; `griffin_lim_ragged`,
STFT.transform_ragged / inverse_ragged and TacotronSTFT.mel_to_magnitude_ragged / mel_to_audio_ragged (additions) take a
batch of utterances of different lengths; `resample` / `resample_ragged` / `resample_length` (additions) convert the sample rate
on the device."""
from flowtron_amd.audio import (STFT, TacotronSTFT, dynamic_range_compression,  # noqa: F401
                                dynamic_range_decompression, griffin_lim, griffin_lim_ragged, resample, resample_length,
                                resample_ragged, window_sumsquare)

for _cls in (STFT, TacotronSTFT):
    _cls.__module__ = "audio_processing"
