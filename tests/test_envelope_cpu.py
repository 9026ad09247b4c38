"""The spectral-envelope RULE (include/flowtron_hip.h, replayed by tests/envelope_ref.py in float64) held to yardsticks that are
not the kernel, and the host side of flowtron_amd.envelope (tables, refusals).  No GPU."""
import numpy as np
import pytest
import torch

import envelope_ref as R
from flowtron_amd import envelope, metrics

SR, HOP = 22050, 256
N_FFT = 1024
H = N_FFT // 2
N = 8192
F0_REF = 120.0
F0_OTHERS = (90.0, 180.0, 240.0, 330.0)
MID = slice(6, -6)         # frames whose window lies inside the signal and behind the filter's onset


@pytest.fixture(scope="module")
def analysed():
    """f0 -> (env [T, H + 1], mc [T, 25], log-mel cepstra [T, 13]) of the test signal at that F0, the constructed F0 given"""
    A = envelope.freqt_matrix(H, 24, 0.455)
    out = {}
    for f0 in (F0_REF,) + F0_OTHERS:
        x = R.vowel(f0, SR, N)
        env, _, mc = R.analyse(x, N, np.full(N // HOP + 1, f0, np.float32), SR, HOP, A)
        out[f0] = (env, mc, R.logmel_cepstra(x, SR, HOP))
    return out


def test_fft_size_follows_the_formula():
    assert [envelope.fft_size(sr) for sr in (8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000)] == [512, 512, 1024, 1024, 1024, 2048, 2048, 2048]
    assert R.fft_size(SR) == N_FFT
    with pytest.raises(NotImplementedError, match="4096"):
        envelope.fft_size(96000)
    with pytest.raises(NotImplementedError, match="256"):
        envelope.fft_size(4000)
    assert envelope.fft_size(8000, f0_floor=20.0) == 2048
    with pytest.raises(NotImplementedError, match="4096"):
        envelope.fft_size(8000, f0_floor=10.0)


def test_the_widest_window_fits_the_transform():
    for sr in (8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000):
        g = R.frame_integers(71.0, sr, envelope.fft_size(sr))
        assert 2 * g["half"] + 1 <= envelope.fft_size(sr) and g["n_w"] >= 1 and g["n_w"] <= g["bnd"]
        g = R.frame_integers(1000.0, sr, envelope.fft_size(sr))
        assert g["ul"] < envelope.fft_size(sr) // 2 and g["ul"] - 1 < 256


def test_f0_independence(analysed):
    """The envelope cepstra barely move with F0 where the log-mel cepstra move a lot.  Measured (dB, against F0 = 120 Hz):
        F0                         90      180     240     330
        log-mel 13                 10.32   18.07   36.86   40.21
        envelope, order 24         0.75    1.22    1.66    3.43        worst ratio 1 / 11.7
        envelope - filter, rms     0.89    1.47    1.91    2.96        (120 Hz: 0.99)
    The two thresholds (a quarter; 3.5 dB) are conditions with slack, not measurements."""
    fr = np.arange(H + 1) * SR / N_FFT
    sel = fr < 3500.0
    target = R.filter_response_db(fr, SR)
    _, mc0, lm0 = analysed[F0_REF]
    for f0 in F0_OTHERS:
        env, mc, lm = analysed[f0]
        d_env = R.cepstral_distance_db(mc[MID][:, 1:], mc0[MID][:, 1:])
        d_lm = R.cepstral_distance_db(lm[MID], lm0[MID])
        print("F0 %g: envelope %.2f dB, log-mel %.2f dB" % (f0, d_env, d_lm))
        assert d_env < 0.25 * d_lm, (f0, d_env, d_lm)
    for f0 in (F0_REF,) + F0_OTHERS:
        d = (10.0 * np.log10(analysed[f0][0][MID]) - target)[:, sel]
        d = d - d.mean(axis=1, keepdims=True)
        rms = float(np.sqrt((d ** 2).mean()))
        print("F0 %g: envelope against the filter %.2f dB rms" % (f0, rms))
        assert rms < 3.5, (f0, rms)


def test_steady_signal_wobbles_less(analysed):
    """frame-to-frame distance on one steady signal, dB.  Measured: envelope 0.98 .. 2.27, log-mel 2.81 .. 7.42; at every F0
    the envelope's is below the log-mel's (120: 1.30 / 3.29, 90: 0.98 / 2.81, 180: 1.60 / 3.13, 240: 1.89 / 7.42, 330: 2.27 / 3.94)"""
    for f0, (_, mc, lm) in analysed.items():
        w_env = R.cepstral_distance_db(mc[MID][1:, 1:], mc[MID][:-1, 1:])
        w_lm = R.cepstral_distance_db(lm[MID][1:], lm[MID][:-1])
        print("F0 %g: wobble envelope %.2f dB, log-mel %.2f dB" % (f0, w_env, w_lm))
        assert w_env < w_lm, (f0, w_env, w_lm)


def test_freqt_matrix():
    rng = np.random.RandomState(3)
    for Hh, order in ((256, 24), (64, 1), (40, 32)):
        A0 = envelope.freqt_matrix(Hh, order, 0.0)
        assert np.array_equal(A0[:, : order + 1], np.eye(order + 1)) and not A0[:, order + 1:].any()
        for alpha in (0.31, 0.455, -0.42):
            A = envelope.freqt_matrix(Hh, order, alpha)
            c = rng.standard_normal(Hh + 1) * np.exp(-0.05 * np.arange(Hh + 1))
            assert np.abs(A @ c - R.freqt_direct(c, order, alpha)).max() <= 1e-12
    # warping by alpha and back by -alpha returns a band-limited cepstrum (the intermediate order long enough to hold it)
    c = np.zeros(257)
    c[:20] = rng.standard_normal(20) * np.exp(-0.2 * np.arange(20))
    for alpha in (0.31, 0.455):
        w = R.freqt_direct(c, 400, alpha)
        back = R.freqt_direct(w, 19, -alpha)
        assert np.abs(back - c[:20]).max() <= 1e-9


def test_direct_sum_equals_cumulative_sum_form():
    rng = np.random.RandomState(5)
    for sr, f0 in ((8000, 71.0), (8000, 1000.0), (22050, 123.4), (22050, 999.0), (48000, 71.0), (32000, 500.0)):
        n_fft = R.fft_size(sr)
        g = R.frame_integers(f0, sr, n_fft)
        P = np.exp(rng.standard_normal(n_fft // 2 + 1))
        a, b = R.smooth_direct(P, g), R.smooth_cumsum(P, g)
        # 1e-12 of the spectrum's scale: the cumulative form's own error is an ulp of its prefix sum (up to ~2000 here, 4e-13),
        # whatever the bin holds -- which is why the kernel does not use it
        assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max(), (sr, f0)


def test_silence():
    A = envelope.freqt_matrix(H, 24, 0.455)
    x = np.zeros(2048, np.float32)
    env, _, mc = R.analyse(x, 2048, np.array([0, 120, 71, 1000, np.nan, 300, 200, 150, 100], np.float32), SR, HOP, A)
    assert np.abs(env / 1e-20 - 1.0).max() <= 1e-12
    assert np.isfinite(mc).all()


def test_integers_come_from_fp32():
    """values of f0 at which 1.5 sr / f0 + 0.5 sits within an fp32 ulp of an integer: float64 and fp32 disagree about floor()"""
    differ = 0
    for half in range(40, 460, 7):
        f = np.float32(1.5 * SR / (half - 0.5))
        for ff in (np.nextafter(f, np.float32(0)), f, np.nextafter(f, np.float32(2000))):
            g = R.frame_integers(ff, SR, N_FFT)
            differ += g["half"] != int(np.floor(1.5 * SR / float(ff) + 0.5))
            assert abs(g["half"] - half) <= 1
    assert differ > 0


def test_refusals_without_a_launch():
    a = torch.zeros(2, 4096)
    f0 = torch.zeros(2, 17)
    for kw, err in ((dict(sampling_rate=96000), NotImplementedError), (dict(sampling_rate=22050.0), ValueError),
                    (dict(hop_length=0), ValueError), (dict(f0_floor=0.0), ValueError), (dict(f0_floor=1200.0), ValueError),
                    (dict(q1=float("nan")), ValueError)):
        with pytest.raises(err):
            envelope.spectral_envelope(a, [4096, 100], f0, **kw)
    with pytest.raises(ValueError, match="17 frames"):
        envelope.spectral_envelope(a, [4096, 100], f0[:, :16])
    with pytest.raises(ValueError):
        envelope.spectral_envelope(a, [4097, 100], f0)
    with pytest.raises(ValueError):
        envelope.spectral_envelope(a, [4096, 0], f0)
    with pytest.raises(ValueError):
        envelope.spectral_envelope(a.double(), [4096, 100], f0)
    with pytest.raises(ValueError):
        envelope.spectral_envelope(a, [4096, 100], f0.double())
    for kw in (dict(order=0), dict(order=33), dict(order=24.0), dict(alpha=1.0), dict(sampling_rate=24000)):
        with pytest.raises(ValueError):
            envelope.mel_cepstra(a, [4096, 100], f0, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        envelope.spectral_envelope(a, [4096, 100], f0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        envelope.mel_cepstra(a, [4096, 100], f0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.envelope_cepstral_distortion(a, [4096, 100], f0, a, [4096, 100], f0)
    with pytest.raises(ValueError, match="equal lengths"):
        metrics.envelope_cepstral_distortion(a, [4096, 100], f0, a, [4096, 1000], f0, align=False)
    big = torch.zeros(1, 1024 * 256)
    with pytest.raises(NotImplementedError, match="MAX_FRAMES"):
        metrics.envelope_cepstral_distortion(big, None, torch.zeros(1, 1025), big, None, torch.zeros(1, 1025))
    assert envelope.alpha_for(22050) == 0.455 and envelope.alpha_for(48000) == 0.554


def test_library_exports_the_entry():
    from flowtron_amd import _lib
    assert "ft_spectral_envelope" in _lib.SIGNATURES
    lib = _lib.lib()
    assert lib.ft_abi_version() == 15                                  # a function was added; no signature or struct changed
    # refusals of the entry point itself come before any device call
    rc = lib.ft_spectral_envelope(8, 1, 1, 8, 8, 1, 1, 8, None, 8, None, 1, 4096, 17, 256, 4096, 0, 22050.0, 33075.0, 71.0, -0.15, None)
    assert rc != 0 and b"4096" in lib.ft_last_error()
    rc = lib.ft_spectral_envelope(8, 1, 1, 8, 8, 1, 1, 8, None, 8, None, 1, 4096, 16, 256, 1024, 0, 22050.0, 33075.0, 71.0, -0.15, None)
    assert rc != 0 and b"T_f0" in lib.ft_last_error()
