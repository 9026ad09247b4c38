"""CPU checks of the synthesis side of the drop-in audio module (audio_processing.py:7-75, 237-270 of the reference):
exports and signatures against the reference's, the host window_sumsquare against the reference's output, the no-CPU-fallback
rule of the device entry points and an unchanged TacotronSTFT state_dict.  Fixture: tests/golden/griffin_lim.pt
(tests/golden/make_golden_gl.py)."""
import inspect
import os

import numpy as np
import pytest
import torch

import audio_processing

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "griffin_lim.pt")


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN, weights_only=False)


def test_exports_match_reference_signatures(golden):
    from audio_processing import STFT, TacotronSTFT, griffin_lim, window_sumsquare  # noqa: F401
    sig = golden["signatures"]
    assert str(inspect.signature(griffin_lim)) == sig["griffin_lim"]
    assert str(inspect.signature(window_sumsquare)) == sig["window_sumsquare"]
    assert str(inspect.signature(STFT.inverse)) == sig["STFT.inverse"]
    assert str(inspect.signature(STFT.forward)) == sig["STFT.forward"]
    assert callable(TacotronSTFT.mel_to_audio) and callable(TacotronSTFT.mel_to_magnitude)


def test_window_sumsquare_matches_reference(golden):
    for case in golden["wss"]:
        got = audio_processing.window_sumsquare("hann", dtype=np.float32, **case["args"])
        ref = case["out"].numpy()
        assert got.dtype == np.float32 and got.shape == ref.shape
        # the reference squares scipy's float64 hann window, this restates it as 0.5 - 0.5 cos: the float32 sums agree to
        # one rounding
        np.testing.assert_allclose(got, ref, rtol=2 * np.finfo(np.float32).eps, atol=1e-30)
        assert np.array_equal(got == 0, ref == 0)


def test_window_sumsquare_rejects_other_windows():
    with pytest.raises(NotImplementedError):
        audio_processing.window_sumsquare("hamming", 4, 256, 1024, 1024)
    with pytest.raises(NotImplementedError):
        audio_processing.window_sumsquare("hann", 4, 256, 1024, 1024, norm=2)
    # win_length None means n_fft, as in librosa
    a = audio_processing.window_sumsquare("hann", 5, 256, None, 1024)
    b = audio_processing.window_sumsquare("hann", 5, 256, 1024, 1024)
    assert np.array_equal(a, b)


def test_cpu_tensors_raise_no_fallback():
    st = audio_processing.STFT(1024, 256, 1024)
    mag, ph = torch.ones(1, 513, 8), torch.zeros(1, 513, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        st.inverse(mag, ph)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        st(torch.zeros(1, 2048))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        audio_processing.griffin_lim(mag, st, 2)
    tst = audio_processing.TacotronSTFT()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tst.mel_to_magnitude(torch.zeros(1, 80, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tst.mel_to_audio(torch.zeros(1, 80, 8))


def test_state_dict_keys_unchanged():
    tst = audio_processing.TacotronSTFT()
    assert sorted(tst.state_dict().keys()) == ["mel_basis", "stft_fn.fft_window"]
    assert tst.mel_pinv.shape == (513, 80)
