"""Host side of ragged vocoding (STFT.transform_ragged / inverse_ragged, griffin_lim_ragged, TacotronSTFT.mel_to_magnitude_ragged /
mel_to_audio_ragged), no GPU needed: the exported names, the four C entries (declared, bound with the declared arity, exported,
refusing bad arguments before the device), the refusal of CPU tensors, the length checks and the unchanged state_dict."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

EINVAL = -1        # FT_EINVAL (include/flowtron_hip.h)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["ft_stft_r8_ragged_phase", "ft_istft_r8_ragged", "ft_stft_pow2_ragged_phase", "ft_istft_pow2_ragged"]


def test_the_five_names_import_from_audio_processing():
    from audio_processing import STFT, TacotronSTFT, griffin_lim_ragged
    assert list(inspect.signature(griffin_lim_ragged).parameters) == ["magnitudes", "n_frames", "stft_fn", "n_iters", "angles"]
    assert inspect.signature(griffin_lim_ragged).parameters["n_iters"].default == 30
    assert list(inspect.signature(STFT.transform_ragged).parameters) == ["self", "input_data", "n_samples"]
    assert list(inspect.signature(STFT.inverse_ragged).parameters) == ["self", "magnitude", "phase", "n_frames"]
    assert list(inspect.signature(TacotronSTFT.mel_to_magnitude_ragged).parameters) == ["self", "mel", "lengths"]
    assert list(inspect.signature(TacotronSTFT.mel_to_audio_ragged).parameters) == ["self", "mel", "lengths", "n_iters", "angles"]


@pytest.mark.parametrize("name", ENTRIES)
def test_entries_declared_bound_and_exported(name):
    from flowtron_amd import _lib as L
    from flowtron_amd import build
    hdr = open(os.path.join(ROOT, "include", "flowtron_hip.h")).read()
    m = re.search(r"\bint %s\(([^)]*)\);" % name, hdr)
    assert m, "%s is not declared in include/flowtron_hip.h" % name
    params = [p.strip() for p in m.group(1).split(",")]
    argtypes, restype = L.SIGNATURES[name]
    assert restype is L._i and len(argtypes) == len(params), (params, argtypes)
    for p, t in zip(params, argtypes):
        assert t is (L._p if "*" in p else L._i), (name, p, t)
    assert hasattr(C.CDLL(build.build(verbose=False)), name)


def test_entries_refuse_before_touching_the_device():
    from flowtron_amd import _lib as L
    from flowtron_amd import build
    build.build(verbose=False)
    lib = L.lib()
    f = 1 << 20                                                              # never dereferenced: every call below is refused
    assert lib.ft_istft_r8_ragged(f, f, None, f, f, 2, 8, 256, None) == EINVAL          # no frame counts
    assert lib.ft_istft_r8_ragged(f, f, f, f, f, 2, 1, 256, None) == EINVAL             # T < 2, as ft_istft_r8
    assert lib.ft_istft_r8_ragged(f, f, f, f, f, 2, 8, 257, None) == EINVAL             # hop > 256
    assert lib.ft_istft_pow2_ragged(f, f, None, f, f, 2, 8, 512, 128, 512, None) == EINVAL
    assert lib.ft_istft_pow2_ragged(f, f, f, f, f, 2, 8, 800, 200, 800, None) == EINVAL  # not a power of two
    assert lib.ft_istft_pow2_ragged(f, f, f, f, f, 2, 8, 512, 513, 512, None) == EINVAL  # hop > win_length
    assert lib.ft_stft_r8_ragged_phase(f, None, f, None, f, 2, 4096, 256, None) == EINVAL   # no sample counts
    assert lib.ft_stft_r8_ragged_phase(f, f, f, f, None, 2, 4096, 256, None) == EINVAL      # the phase is not optional
    assert lib.ft_stft_r8_ragged_phase(f, f, f, None, f, 2, 512, 256, None) == EINVAL       # N <= n_fft / 2
    assert lib.ft_stft_pow2_ragged_phase(f, f, f, None, None, 2, 4096, 512, 128, 512, None) == EINVAL
    assert lib.ft_stft_pow2_ragged_phase(f, f, f, None, f, 2, 4096, 800, 200, 800, None) == EINVAL
    assert lib.ft_stft_pow2_ragged_phase(f, f, f, None, f, 2, 256, 512, 128, 512, None) == EINVAL


def test_cpu_tensors_are_refused_by_every_new_function():
    import audio_processing
    st = audio_processing.STFT(1024, 256, 1024)
    tst = audio_processing.TacotronSTFT(1024, 256, 1024, 80, 22050, 0.0, 8000.0)
    M, P = torch.ones(2, 513, 8), torch.zeros(2, 513, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        st.transform_ragged(torch.zeros(2, 4096), [4096, 2000])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        st.inverse_ragged(M, P, [8, 5])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        audio_processing.griffin_lim_ragged(M, [8, 5], st, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tst.mel_to_magnitude_ragged(torch.zeros(2, 80, 8), [8, 5])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tst.mel_to_audio_ragged(torch.zeros(2, 80, 8), [8, 5], 2)


def test_state_dict_keys_unchanged():
    import audio_processing
    assert list(audio_processing.TacotronSTFT().state_dict()) == ["mel_basis", "stft_fn.fft_window"]
    assert list(audio_processing.STFT(1024, 256, 1024).state_dict()) == ["fft_window"]


def lengths(v, B=3, lo=1, hi=8, name="n_frames"):
    from flowtron_amd.audio import _host_lengths
    return _host_lengths(v, B, lo, hi, name, "%d ..= %d" % (lo, hi))


def test_lengths_accept_lists_tuples_and_cpu_integer_tensors():
    assert lengths([1, 8, 4]) == [1, 8, 4]
    assert lengths((3, 2), B=2) == [3, 2]
    assert lengths([np.int64(7), np.int32(2)], B=2) == [7, 2]
    for dt in (torch.int64, torch.int32, torch.int16, torch.uint8):
        got = lengths(torch.tensor([5, 1, 8], dtype=dt))
        assert got == [5, 1, 8] and all(type(x) is int for x in got), dt


@pytest.mark.parametrize("v, msg", [
    ([1, 2], r"holds 2 lengths for a batch of 3"),
    (torch.tensor([4, 4, 4, 4]), r"holds 4 lengths for a batch of 3"),
    ([1, 0, 3], r"\[1\] = 0 is outside 1 \.\.= 8"),
    ([1, 2, 9], r"\[2\] = 9 is outside 1 \.\.= 8"),
    ([-1, 2, 3], r"\[0\] = -1 is outside"),
    (torch.tensor([1, 9, 3]), r"\[1\] = 9 is outside"),
    ([1, 2.0, 3], r"\[1\] = 2\.0 is not an integer"),
    ([True, 2, 3], r"\[0\] = True is not an integer"),
    (torch.tensor([1.0, 2.0, 3.0]), "must be host integers"),
    (torch.tensor([True, True, False]), "must be host integers"),
    (torch.tensor([[1, 2, 3]]), "must be host integers"),
    (5, "must be host integers"),
])
def test_lengths_refused_with_the_argument_and_the_utterance(v, msg):
    with pytest.raises(ValueError, match=msg):
        lengths(v)
    with pytest.raises(ValueError, match="n_samples"):
        lengths(v, name="n_samples")
