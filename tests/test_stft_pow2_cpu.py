"""CPU checks of the power-of-two STFT path (csrc/stft_pow2.hip): the routing predicates over the whole scope, the CSR
filterbank at the large sizes, window_sumsquare against the reference's (tests/golden/stft_pow2.pt), the no-CPU-fallback rule,
and the argument checks of the C entries, which return FT_EINVAL before any device call."""
import os

import numpy as np
import pytest
import torch

import audio_processing
from flowtron_amd import _lib as L
from flowtron_amd.audio import POW2_NFFT, filterbank_csr, slaney_mel_filterbank

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stft_pow2.pt")


def route(n_fft, hop, win):
    st = audio_processing.STFT(n_fft, hop, win)
    if st.fast_path():
        return "r8"
    if st.pow2_path():
        return "pow2"
    return None


@pytest.mark.parametrize("n_fft", [128, 256, 512, 800, 1024, 1200, 2048, 4096, 8192])
def test_routing_over_the_scope(n_fft):
    for win in sorted({n_fft, n_fft - 1, n_fft // 2 + 1, n_fft * 3 // 4}):
        for hop in sorted({1, 2, 64, 128, 200, 256, 257, 300, 512, win - 1, win, win + 1} - {0}):
            if hop > n_fft * 2:
                continue
            got = route(n_fft, hop, win)
            if n_fft == 1024 and hop <= 256:
                want = "r8"                                   # unchanged: fast_path() means what it meant
            elif n_fft in (256, 512, 1024, 2048, 4096) and 1 <= hop <= win <= n_fft:
                want = "pow2"
            else:
                want = None
            assert got == want, (n_fft, hop, win, got)


def test_ragged_path_and_scope_table():
    assert POW2_NFFT == (256, 512, 1024, 2048, 4096)
    for n_fft, hop, win, n_mel, ok in ((512, 128, 512, 80, True), (2048, 300, 1200, 80, True), (2048, 512, 2048, 128, True),
                                       (2048, 512, 2048, 129, False), (1024, 256, 1024, 80, True), (800, 200, 800, 80, False),
                                       (4096, 4096, 4096, 80, True), (4096, 1024, 1000, 80, False)):
        t = audio_processing.TacotronSTFT(n_fft, hop, win, n_mel, 44100, 0.0, None)
        assert t.ragged_path() == ok, (n_fft, hop, win, n_mel)


@pytest.mark.parametrize("n_fft,sr,fmax,n_mel", [(2048, 44100, 8000.0, 80), (4096, 48000, 8000.0, 80), (2048, 44100, None, 80),
                                                 (4096, 44100, None, 80), (4096, 48000, None, 128)])
def test_csr_filterbank_rebuilds_the_dense_basis(n_fft, sr, fmax, n_mel):
    basis = slaney_mel_filterbank(sr, n_fft, n_mel, 0.0, fmax)
    bin0, ptr, w = filterbank_csr(basis)
    dense = np.zeros_like(basis)
    for b in range(n_mel):
        n = ptr[b + 1] - ptr[b]
        dense[b, bin0[b]:bin0[b] + n] = w[ptr[b]:ptr[b + 1]]
    assert np.array_equal(dense, basis)
    assert ptr[0] == 0 and np.all(np.diff(ptr) >= 0) and ptr[-1] == w.size
    if fmax is None and n_fft == 4096:
        assert w.size > 2048                                  # the kernel reads these weights from global memory


def test_window_sumsquare_matches_reference():
    g = torch.load(GOLDEN, weights_only=False)
    for name in g["settings"]:
        case = g[name]["wss"]
        got = audio_processing.window_sumsquare("hann", dtype=np.float32, **case["args"])
        ref = case["out"].numpy()
        assert got.dtype == np.float32 and got.shape == ref.shape
        np.testing.assert_allclose(got, ref, rtol=2 * np.finfo(np.float32).eps, atol=1e-30)
        assert np.array_equal(got == 0, ref == 0)


def test_cpu_tensors_raise_no_fallback():
    st = audio_processing.STFT(2048, 512, 2048)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        st.transform(torch.zeros(1, 4096))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        st.inverse(torch.ones(1, 1025, 8), torch.zeros(1, 1025, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        audio_processing.griffin_lim(torch.ones(1, 1025, 8), st, 2)
    tst = audio_processing.TacotronSTFT(2048, 512, 2048, 80, 44100, 0.0, 8000.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tst.mel_spectrogram(torch.zeros(1, 4096))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tst.mel_spectrogram_ragged(torch.zeros(1, 4096), torch.tensor([4096], dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tst.mel_to_audio(torch.zeros(1, 80, 8))


# Dummy host addresses: every call below fails its argument check and returns before any pointer is used or any device call
# is made.
P = 4096
FT_EINVAL = -1                                                # include/flowtron_hip.h


def _stft(**over):
    a = dict(y=P, window=P, bin0=P, ptr=P, w=P, mel=P, mag=None, phase=None, B=1, N=4096, n_fft=2048, hop=512, win=2048, n_mel=80)
    a.update(over)
    return L.lib().ft_stft_pow2(a["y"], a["window"], a["bin0"], a["ptr"], a["w"], a["mel"], a["mag"], a["phase"], a["B"], a["N"],
                                a["n_fft"], a["hop"], a["win"], a["n_mel"], None)


def _ragged(**over):
    a = dict(y=P, ns=P, window=P, bin0=P, ptr=P, w=P, mel=P, B=2, N=4096, n_fft=2048, hop=512, win=2048, n_mel=80, T_out=9)
    a.update(over)
    return L.lib().ft_stft_pow2_ragged(a["y"], a["ns"], a["window"], a["bin0"], a["ptr"], a["w"], a["mel"], a["B"], a["N"],
                                       a["n_fft"], a["hop"], a["win"], a["n_mel"], a["T_out"], None)


def _istft(**over):
    a = dict(mag=P, phase=P, window=P, y=P, B=1, T=9, n_fft=2048, hop=512, win=2048)
    a.update(over)
    return L.lib().ft_istft_pow2(a["mag"], a["phase"], a["window"], a["y"], a["B"], a["T"], a["n_fft"], a["hop"], a["win"], None)


@pytest.mark.parametrize("fn,bad", [
    (_stft, dict(y=None)), (_stft, dict(window=None)), (_stft, dict(mel=None)), (_stft, dict(mag=P)),
    (_stft, dict(bin0=None)), (_stft, dict(n_fft=768)), (_stft, dict(n_fft=128)), (_stft, dict(n_fft=8192)),
    (_stft, dict(hop=600, win=512)), (_stft, dict(hop=0)), (_stft, dict(win=4096)), (_stft, dict(N=1024)),
    (_stft, dict(n_mel=129)), (_stft, dict(B=0)),
    (_ragged, dict(ns=None)), (_ragged, dict(mel=None)), (_ragged, dict(n_fft=768)), (_ragged, dict(hop=1025, win=1024)),
    (_ragged, dict(N=1024)), (_ragged, dict(T_out=0)), (_ragged, dict(n_mel=0)),
    (_istft, dict(mag=None)), (_istft, dict(y=None)), (_istft, dict(n_fft=768)), (_istft, dict(hop=300, win=200)),
    (_istft, dict(T=1)), (_istft, dict(win=4096)),
])
def test_c_entries_reject_out_of_scope_arguments(fn, bad):
    name = {_stft: b"ft_stft_pow2:", _ragged: b"ft_stft_pow2_ragged:", _istft: b"ft_istft_pow2:"}[fn]
    assert fn(**bad) == FT_EINVAL, bad
    err = L.lib().ft_last_error()
    assert err.startswith(name) and b"invalid argument" in err, err
