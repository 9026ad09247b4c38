"""The synthesis side of the audio front end on the MI355X: STFT.inverse (ft_istft_r8), STFT.forward, griffin_lim (ft_stft_r8 +
ft_istft_r8 in a loop) and TacotronSTFT.mel_to_magnitude / mel_to_audio (ft_gemm + Griffin-Lim), against the float64 restatement
of the reference's formulas (audio_processing.py:7-75, 237-270) in tests/stft_ref64.py, and against the REAL reference's
outputs in tests/golden/griffin_lim.pt (tests/golden/make_golden_gl.py).  The fixture stores no inputs: they are rebuilt
here from the same seeds (`random_spectrum`, `magnitudes32`), and the magnitudes are checked against its fingerprint.

The restatement: y[n] = sum_t w[n + 512 - t hop] irfft(M e^{i phase})_t[n + 512 - t hop] / wss[n + 512] where
wss > tiny(float32), wss[u] = sum_t w^2[u - t hop]; numpy's irfft ignores Im of bins 0 and 512 like the reference's
pseudo-inverse basis."""
import os

import numpy as np
import pytest
import torch

import audio_processing
from flowtron_amd import _lib as L
from stft_ref64 import griffin_lim64, inverse_bound, istft64, rel_l2, start_angles, stft64

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "griffin_lim.pt")
EPS32 = float(np.finfo(np.float32).eps)


def random_spectrum(seed, B, T):
    rs = np.random.RandomState(seed)
    M = rs.uniform(0.0, 2.0, (B, 513, T)).astype(np.float32)
    P = rs.uniform(-np.pi, np.pi, (B, 513, T)).astype(np.float32)
    return M, P


def magnitudes32(y, hop=256, win_length=1024):
    """Griffin-Lim input of the fixture's cases: |STFT(y)| in float64, rounded once to float32."""
    return np.abs(stft64(np.asarray(y, np.float64), 1024, hop, win_length)).astype(np.float32)


def spectral_convergence(y, M, hop=256, win_length=1024):
    return float(np.linalg.norm(np.abs(stft64(y, 1024, hop, win_length)) - M) / np.linalg.norm(M))


def check_inverse(M, P, hop, win_length, what):
    st = audio_processing.STFT(1024, hop, win_length).cuda()
    y = st.inverse(torch.from_numpy(M).cuda(), torch.from_numpy(P).cuda())
    B, _, T = M.shape
    assert y.shape == (B, 1, hop * (T - 1)), (what, y.shape)
    y = y[:, 0].cpu().double().numpy()
    y64 = istft64(M, P, 1024, hop, win_length)[0]
    bound = inverse_bound(M, 1024, hop, win_length) + 8 * EPS32 * np.abs(y64)
    ratio = np.abs(y - y64) / bound
    print("%s: max |gpu - f64| / bound = %.3g, rel L2 %.2e" % (what, ratio.max(), rel_l2(y, y64)))
    assert ratio.max() <= 1.0, (what, ratio.max(), np.unravel_index(ratio.argmax(), ratio.shape))
    return y


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN, weights_only=False)


# ---- STFT.inverse ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,hop,win_length,phase_range", [
    (1, 4, 256, 1024, np.pi),           # the fewest frames griffin_lim accepts at hop 256
    (3, 37, 256, 800, np.pi),           # T not a multiple of 16
    (32, 862, 256, 1024, np.pi),        # 10 s batch
    (3, 50, 200, 800, np.pi),
    (1, 862, 200, 1024, np.pi),
    (2, 29, 128, 1024, np.pi),
    (1, 4, 128, 800, 60.0),             # phases far outside [-pi, pi]: sincosf's range reduction
])
def test_inverse_matches_float64(B, T, hop, win_length, phase_range):
    rs = np.random.RandomState(B * 1000 + T + hop)
    M = rs.uniform(0.0, 2.0, (B, 513, T)).astype(np.float32)
    P = rs.uniform(-phase_range, phase_range, (B, 513, T)).astype(np.float32)
    M[:, :, T // 2] *= 40.0                                              # one loud frame among quiet ones
    check_inverse(M, P, hop, win_length, "B%d T%d hop%d win%d" % (B, T, hop, win_length))


@pytest.mark.parametrize("name", ["inverse_h256", "inverse_h200"])
def test_inverse_vs_reference_golden(golden, name):
    g = golden[name]
    M, P = random_spectrum(g["seed"], g["B"], g["T"])
    y = check_inverse(M, P, g["hop"], g["win_length"], name)
    print("%s: gpu vs reference rel L2 %.2e (reference vs f64 %.2e)" % (name, rel_l2(y, g["y"].numpy()), g["dev64"]))
    assert rel_l2(y, g["y"].numpy()) < 10 * g["dev64"]


@pytest.mark.parametrize("hop,win_length", [(256, 1024), (200, 800), (128, 1024)])
def test_forward_round_trip(hop, win_length):
    """inverse(transform(y)) reproduces y (overlap-add of a hann-windowed STFT is exact where wss > 0)."""
    from oracle import synth
    y = torch.stack([synth.make_audio(22050, seed=s) for s in (4, 5)]).cuda()
    st = audio_processing.STFT(1024, hop, win_length).cuda()
    r = st(y)
    n = hop * (22050 // hop)
    assert r.shape == (2, 1, n)
    assert torch.equal(r, st.inverse(st.magnitude, st.phase))
    err = (r[:, 0, 1024:n - 1024] - y[:, 1024:n - 1024]).abs().max().item()
    # fp32 forward FFT + magnitude / atan2 + inverse FFT: each a few eps log2(1024) of the signal's scale
    bound = 64 * EPS32 * 10 * y.abs().max().item()
    print("round trip hop %d win %d: max err %.2e (bound %.2e)" % (hop, win_length, err, bound))
    assert err < bound
    full = (r[:, 0] - y[:, :n]).abs().max().item()
    assert full < bound, full                                           # the ends too: the reflect padding is inverted exactly


# ---- griffin_lim -------------------------------------------------------------------------------------------------------------
def _gl_magnitudes(g):
    """The fixture case's input, rebuilt from its synth audio and checked against the generator's fingerprint."""
    from oracle import synth
    seeds = g["audio_seeds"] if "audio_seeds" in g else [g["audio_seed"]]
    M = magnitudes32(torch.stack([synth.make_audio(g["n_samples"], seed=s) for s in seeds]).numpy())
    fp = g["mag"]
    assert np.array_equal(M.reshape(-1)[::997], fp["sample"].numpy())
    assert abs(float(M.astype(np.float64).sum()) - fp["sum64"]) <= 1e-9 * abs(fp["sum64"])
    return M


def _gl_case(golden, name, n):
    g = golden[name]
    M = _gl_magnitudes(g)
    stft = audio_processing.STFT(1024, 256, 1024).cuda()
    np.random.seed(0)
    y = audio_processing.griffin_lim(torch.from_numpy(M).cuda(), stft, n).cpu()
    y64 = griffin_lim64(M, start_angles(M.shape), n, 1024, 256, 1024)
    ref = g["y"][n] if name == "gl_41" else g["y"]                      # every stride-th sample of the reference's output
    dev = g["dev64"][n] if name == "gl_41" else g["dev64"]
    return M, y.numpy(), y64, ref.numpy(), dev, g["stride"]


@pytest.mark.parametrize("name,n", [("gl_41", 0), ("gl_41", 1), ("gl_41", 8), ("gl_41", 32), ("gl_862", 30)])
def test_griffin_lim_vs_float64(golden, name, n):
    M, y, y64, ref, dev, stride = _gl_case(golden, name, n)
    assert y.shape == (M.shape[0], 256 * (M.shape[2] - 1)) and ref.shape == y[:, ::stride].shape
    d64, dref = rel_l2(y, y64), rel_l2(y[:, ::stride], ref)
    sc, sc64 = spectral_convergence(y, M), spectral_convergence(y64, M)
    print("%s n_iters %d: gpu vs f64 %.2e (bound 10 x %.2e), gpu vs reference %.2e (every %d-th sample), spectral convergence "
          "%.4f (f64 %.4f)" % (name, n, d64, dev, dref, stride, sc, sc64))
    assert d64 <= 10 * dev
    assert abs(sc / sc64 - 1) <= 0.01


def test_griffin_lim_deterministic(golden):
    M = torch.from_numpy(_gl_magnitudes(golden["gl_862"])).cuda()
    stft = audio_processing.STFT(1024, 256, 1024).cuda()
    outs = []
    for _ in range(2):
        np.random.seed(0)
        outs.append(audio_processing.griffin_lim(M, stft, 10))
    assert torch.equal(outs[0], outs[1])
    np.random.seed(1)
    assert not torch.equal(outs[0], audio_processing.griffin_lim(M, stft, 10))


# ---- mel -> waveform ---------------------------------------------------------------------------------------------------------
def _tacotron_stft():
    return audio_processing.TacotronSTFT(1024, 256, 1024, 80, 22050, 0.0, 8000.0).cuda()


def test_mel_to_magnitude_matches_float64():
    tst = _tacotron_stft()
    rs = np.random.RandomState(3)
    mel = torch.from_numpy(rs.uniform(-8, 2, (3, 80, 45)).astype(np.float32))
    mag = tst.mel_to_magnitude(mel.cuda()).cpu().double().numpy()
    pinv = np.linalg.pinv(tst.mel_basis.cpu().double().numpy())
    ref = np.maximum(np.einsum("km,bmt->bkt", pinv, np.exp(mel.double().numpy())), 0)
    # fp32 GEMM over K = 80 from fp32 pinv and exp: a few eps of sum_m |pinv[k, m]| exp(mel[m, t])
    scale = np.einsum("km,bmt->bkt", np.abs(pinv), np.exp(mel.double().numpy()))
    assert mag.shape == (3, 513, 45)
    assert (np.abs(mag - ref) <= 64 * EPS32 * scale + 1e-30).all(), (np.abs(mag - ref) / scale).max()
    one = tst.mel_to_magnitude(mel[1].cuda())
    assert one.shape == (513, 45) and torch.equal(one, tst.mel_to_magnitude(mel.cuda())[1])


def test_mel_round_trip():
    """synth audio -> mel_spectrogram -> mel_to_audio -> mel_spectrogram: 60 iterations end closer to the mel than 0 do, and
    within a few percent of what the same pipeline in float64 reaches."""
    from oracle import synth
    tst = _tacotron_stft()
    y = synth.make_audio(256 * 120, seed=3)[None].cuda()
    mel = tst.mel_spectrogram(y)
    fb = tst.mel_basis.cpu().double().numpy()
    pinv = np.linalg.pinv(fb)
    mel_np = mel.cpu().double().numpy()

    def logmel_err(audio):
        return float(np.abs(tst.mel_spectrogram(audio).cpu().double().numpy() - mel_np).mean())

    def logmel_err64(audio):
        m64 = np.log(np.maximum(np.einsum("mk,bkt->bmt", fb, np.abs(stft64(audio, 1024, 256, 1024))), 1e-5))
        return float(np.abs(m64 - mel_np).mean())

    errs, errs64 = {}, {}
    for n in (0, 60):
        np.random.seed(0)
        audio = tst.mel_to_audio(mel, n_iters=n)
        assert audio.shape == (1, 256 * (mel.shape[2] - 1))
        errs[n] = logmel_err(audio)
        M64 = np.maximum(np.einsum("km,bmt->bkt", pinv, np.exp(mel_np)), 0)
        errs64[n] = logmel_err64(griffin_lim64(M64, start_angles(M64.shape), n, 1024, 256, 1024))
    print("log-mel mean |error|: n_iters 0 %.4f, 60 %.4f (float64 pipeline %.4f, %.4f)" % (errs[0], errs[60], errs64[0], errs64[60]))
    assert errs[60] < errs[0]
    assert abs(errs[60] / errs64[60] - 1) < 0.05


def test_flowtron_infer_to_audio():
    import flowtron
    from oracle import synth
    os.environ["FLOWTRON_MFMA"] = "f32"
    cfg = dict(synth.SMALL_MODEL_CONFIG)
    m = flowtron.Flowtron(**cfg)
    m.load_state_dict(synth.make_state_dict(cfg, seed=21))
    m = m.cuda().eval()
    b = synth.make_batch(cfg, [30], [9], seed=21, with_prior=False)
    rs = np.random.RandomState(21)
    residual = torch.from_numpy(rs.standard_normal((1, cfg["n_mel_channels"], 30)).astype(np.float32)).cuda() * 0.5
    with torch.no_grad():
        mel, _ = m.infer(residual, b["speaker_ids"][:1].cuda(), b["text"][:1, :9].cuda(), gate_threshold=1.0)
    tst = _tacotron_stft()
    T = mel.shape[2]
    outs = []
    for _ in range(2):
        np.random.seed(0)
        outs.append(tst.mel_to_audio(mel, n_iters=8))
    assert outs[0].shape == (1, 256 * (T - 1))
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1])


# ---- input validation ------------------------------------------------------------------------------------------------------------
def test_input_validation():
    st = audio_processing.STFT(1024, 256, 1024).cuda()
    M = torch.ones(1, 513, 8, device="cuda")
    with pytest.raises(ValueError):
        st.inverse(M, torch.zeros(1, 513, 7, device="cuda"))
    with pytest.raises(ValueError):
        st.inverse(M[:, :512], torch.zeros(1, 512, 8, device="cuda"))
    with pytest.raises(ValueError):
        audio_processing.griffin_lim(M[:, :, :3], st, 2)                  # hop (T - 1) = 512 <= filter_length / 2
    audio_processing.griffin_lim(M[:, :, :4], st, 1)                      # 768 samples: accepted
    assert st.inverse(M[:, :, :1], M[:, :, :1]).shape == (1, 1, 0)       # the reference trims a single frame to nothing
    with pytest.raises(NotImplementedError):
        audio_processing.STFT(800, 200, 800).cuda().inverse(M[:, :401], M[:, :401])
    with pytest.raises(NotImplementedError):
        audio_processing.griffin_lim(M[:, :401], audio_processing.STFT(800, 200, 800).cuda(), 2)
    with pytest.raises(ValueError):
        _tacotron_stft().mel_to_magnitude(torch.zeros(1, 79, 8, device="cuda"))
    y = torch.empty(1, 256 * 7, device="cuda")
    for bad in [dict(B=0), dict(hop=257), dict(T=1)]:
        a = dict(B=1, T=8, hop=256)
        a.update(bad)
        rc = L.lib().ft_istft_r8(L.ptr(M), L.ptr(M), L.ptr(st.fft_window), L.ptr(y), a["B"], a["T"], a["hop"], L.stream())
        assert rc == -1 and b"ft_istft_r8" in L.lib().ft_last_error(), bad
