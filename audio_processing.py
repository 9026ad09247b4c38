"""Drop-in for the reference's `audio_processing.py` (data.py:27 does `from audio_processing import
TacotronSTFT`): same names and contracts, HIP kernels underneath -- the mel front end, STFT.transform /
inverse / forward, `griffin_lim` on the device and the host `window_sumsquare` (audio_processing.py:7-75,
237-270).  TacotronSTFT.mel_to_audio (an addition) vocodes model output with Griffin-Lim; `griffin_lim_ragged`,
STFT.transform_ragged / inverse_ragged and TacotronSTFT.mel_to_magnitude_ragged / mel_to_audio_ragged (additions) take a
batch of utterances of different lengths; `resample` / `resample_ragged` / `resample_length` (additions) convert the sample rate
on the device; `spsi_phase` (an addition) is the single-pass phase start of Griffin-Lim; `active_bounds` / `frame_power` / `trim` /
`loudness` / `normalize` / `prepare` (additions, flowtron_amd.level) cut silence and bring a batch to one BS.1770 loudness on the
device.  `griffin_lim` keeps the reference's signature here (tests hold it to it); its `momentum`, `n_frames`, `angles`
and `phase_init` keywords (fast Griffin-Lim, also for a ragged batch, and the SPSI start) are on flowtron_amd.audio.griffin_lim and behind TacotronSTFT.mel_to_audio."""
from flowtron_amd import audio as _audio
from flowtron_amd.audio import (STFT, TacotronSTFT, dynamic_range_compression,  # noqa: F401
                                dynamic_range_decompression, griffin_lim_ragged, resample, resample_length,
                                resample_ragged, spsi_phase, window_sumsquare)
from flowtron_amd.level import active_bounds, frame_power, loudness, normalize, prepare, trim  # noqa: F401


def griffin_lim(magnitudes, stft_fn, n_iters=30):
    """audio_processing.py:59-75 on the device: flowtron_amd.audio.griffin_lim at its defaults."""
    return _audio.griffin_lim(magnitudes, stft_fn, n_iters)


for _cls in (STFT, TacotronSTFT):
    _cls.__module__ = "audio_processing"
