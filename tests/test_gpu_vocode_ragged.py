"""Vocoding a batch of utterances of different lengths on the MI355X: STFT.inverse_ragged / transform_ragged (ft_istft_*_ragged,
ft_stft_*_ragged_phase), griffin_lim_ragged and TacotronSTFT.mel_to_magnitude_ragged / mel_to_audio_ragged.  Every utterance of a
ragged call must come out bit for bit as the tested dense path computes it alone, with exact zeros behind its end, and the frames
and samples behind an utterance's length (filled with NaN here) must never be read.  Both kernel families: n_fft 1024 with
hop <= 256 (csrc/stft_r8.hip) and the power-of-two sizes (csrc/stft_pow2.hip).

Lengths sit where a per-utterance count can go wrong.  An inverse workgroup owns 16 hop samples (1024 family: 16 frames) or 4 096
samples (power-of-two family: 32 frames at hop 128, 13.65 at hop 300, one workgroup for everything at hop 1):
  1024 / 256 and 1024 / 200   n_frames 40, 17, 33, 4: an end inside a span, exactly one span, exactly two, the shortest legal
  512 / 128                   48, 33, 20, 4: inside the second span, exactly one span, inside the first, the shortest legal
  2048 / 300                  48, 15, 14, 5: 300 (n - 1) is never a multiple of 4 096, so 15 ends 104 samples into the second span
                              and 14 ends 196 samples before it; 48 ends in the fourth; 5 is the shortest legal
  256 / 1                     200, 130, 177, 161: 130 frames is the shortest legal utterance at hop 1
(the shortest legal utterance: hop (n - 1) > n_fft / 2, griffin_lim's reflect rule).  Measured figures are printed (pytest -s)."""
import os

import numpy as np
import pytest
import torch

import audio_processing
from call_count import count_calls
from stft_ref64 import TINY32, istft64

pytestmark = pytest.mark.gpu

INV_BOUND = 1e-6                      # relative L2 against float64: the bound of test_gpu_stft_pow2.py for the dense inverse

# (n_fft, hop, win_length) -> (T, n_frames)
SETTINGS = {
    (1024, 256, 1024): (42, [40, 17, 33, 4]),
    (1024, 200, 800): (42, [40, 17, 33, 4]),
    (512, 128, 512): (48, [48, 33, 20, 4]),
    (2048, 300, 1200): (48, [48, 15, 14, 5]),
    (256, 1, 201): (203, [200, 130, 177, 161]),
}
KEYS = list(SETTINGS)
IDS = ["n%d_h%d_w%d" % k for k in KEYS]
DENSE = ["ft_stft_r8", "ft_istft_r8", "ft_stft_r8_ragged", "ft_stft_pow2", "ft_istft_pow2", "ft_stft_pow2_ragged", "ft_stft_mel"]
RAGGED = ["ft_stft_r8_ragged_phase", "ft_istft_r8_ragged", "ft_stft_pow2_ragged_phase", "ft_istft_pow2_ragged"]


def stft_of(key):
    return audio_processing.STFT(*key).cuda()


def spectrum(key, B, T, seed, lens=None):
    """(M, P) float32 [B, n_fft/2+1, T] on the host; NaN in the frames t >= lens[b] when lens is given."""
    rs = np.random.RandomState(seed)
    nb = key[0] // 2 + 1
    M = rs.uniform(0.0, 2.0, (B, nb, T)).astype(np.float32)
    P = rs.uniform(-np.pi, np.pi, (B, nb, T)).astype(np.float32)
    if lens is not None:
        for b, n in enumerate(lens):
            M[b, :, n:] = np.nan
            P[b, :, n:] = np.nan
    return torch.from_numpy(M), torch.from_numpy(P)


# ---- 1. the inverse equals each utterance alone ---------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_inverse_equals_each_utterance_alone(key):
    n_fft, hop, win = key
    st = stft_of(key)
    T, lens = SETTINGS[key]
    for case, nf in enumerate([lens, [1, 2, lens[1] - 1, T]]):              # one frame: no samples; two frames: hop samples
        M, P = spectrum(key, 4, T, seed=n_fft + hop + case, lens=nf)
        Md, Pd = M.cuda(), P.cuda()
        y = st.inverse_ragged(Md, Pd, nf)
        assert y.shape == (4, 1, hop * (T - 1)) and y.dtype == torch.float32
        assert not torch.isnan(y).any(), "a frame behind an utterance's end was read"
        for b, n in enumerate(nf):
            own = hop * (n - 1)
            one = st.inverse(Md[b:b + 1, :, :n], Pd[b:b + 1, :, :n])
            assert one.shape == (1, 1, own)
            assert torch.equal(y[b, 0, :own], one[0, 0]), (nf, b)
            assert torch.all(y[b, 0, own:] == 0), (nf, b)
        assert torch.equal(y, st.inverse_ragged(Md, Pd, torch.tensor(nf)))   # a second launch, lengths as a CPU tensor


# ---- 2. the inverse against float64 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [(1024, 256, 1024), (2048, 300, 1200)], ids=["n1024_h256_w1024", "n2048_h300_w1200"])
def test_inverse_matches_float64(key):
    n_fft, hop, win = key
    st = stft_of(key)
    T, lens = SETTINGS[key]
    M, P = spectrum(key, 4, T, seed=7 * n_fft + hop, lens=lens)
    y = st.inverse_ragged(M.cuda(), P.cuda(), lens)[:, 0].cpu().double().numpy()
    for b in (int(np.argmin(lens)), int(np.argmax(lens))):
        n = lens[b]
        y64, wss = istft64(M[b:b + 1, :, :n].numpy(), P[b:b + 1, :, :n].numpy(), n_fft, hop, win)
        got = y[b, :hop * (n - 1)]
        e = float(np.linalg.norm(got - y64[0]) / np.linalg.norm(y64[0]))
        zero = wss <= TINY32
        print("inverse_ragged %d / %d / %d, utterance %d (%d frames): rel L2 vs f64 %.2e, %d samples with wss <= FLT_MIN"
              % (n_fft, hop, win, b, n, e, zero.sum()))
        assert e <= INV_BOUND
        assert np.all(got[zero] == 0)


# ---- 3. the transform equals each utterance alone -------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_transform_equals_each_utterance_alone(key):
    from oracle import synth
    n_fft, hop, win = key
    st = stft_of(key)
    T = SETTINGS[key][0]
    N, half = hop * (T - 1), n_fft // 2
    g = 16 * hop * (half // (16 * hop) + 1)            # the first multiple of 16 frames' worth of samples above n_fft / 2
    lens = [N, half + 1, g - 1, g]                      # all of it, the shortest legal, 16 k frames exactly, 16 k + 1 frames
    assert all(half < n <= N for n in lens)
    y = torch.full((4, N), float("nan"))
    for b, n in enumerate(lens):
        y[b, :n] = synth.make_audio(n, seed=n_fft + hop + b)
    yd = y.cuda()
    mag, phase = st.transform_ragged(yd, lens)
    assert mag.shape == (4, half + 1, N // hop + 1) and phase.shape == mag.shape
    assert not torch.isnan(mag).any() and not torch.isnan(phase).any(), "the reflection reached the padding"
    for b, n in enumerate(lens):
        t = n // hop + 1
        m1, p1 = st.transform(yd[b:b + 1, :n])
        assert m1.shape == (1, half + 1, t)
        assert torch.equal(mag[b, :, :t], m1[0]) and torch.equal(phase[b, :, :t], p1[0]), b
        assert torch.all(mag[b, :, t:] == 0) and torch.all(phase[b, :, t:] == 0), b
    mag2, phase2 = st.transform_ragged(yd, tuple(lens))
    assert torch.equal(mag, mag2) and torch.equal(phase, phase2)


# ---- 4. Griffin-Lim tied to the tested dense path ---------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_griffin_lim_full_lengths_equal_dense(key):
    st = stft_of(key)
    T = SETTINGS[key][0]
    M = spectrum(key, 3, T, seed=11 + key[1])[0].cuda()
    for n in (0, 1, 8):
        np.random.seed(0)
        got = audio_processing.griffin_lim_ragged(M, [T] * 3, st, n)
        np.random.seed(0)
        ref = audio_processing.griffin_lim(M, st, n)
        assert got.shape == ref.shape == (3, key[1] * (T - 1))
        assert torch.equal(got, ref), n


# ---- 5. Griffin-Lim, ragged -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_griffin_lim_ragged_equals_each_utterance_alone(key):
    hop = key[1]
    st = stft_of(key)
    T, lens = SETTINGS[key]
    M, A = spectrum(key, 4, T, seed=23 + hop, lens=lens)                     # NaN behind every utterance, in both
    Md = M.cuda()
    for n in (0, 3):
        y = audio_processing.griffin_lim_ragged(Md, lens, st, n, angles=A)   # starting phase from the host
        assert y.shape == (4, hop * (T - 1))
        assert not torch.isnan(y).any()
        for b, nf in enumerate(lens):
            own = hop * (nf - 1)
            one = audio_processing.griffin_lim_ragged(Md[b:b + 1, :, :nf], [nf], st, n, angles=A[b:b + 1, :, :nf].cuda())
            assert one.shape == (1, own)
            assert torch.equal(y[b, :own], one[0]), (n, b)
            assert torch.all(y[b, own:] == 0), (n, b)


# ---- 6. launch count --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [(1024, 256, 1024), (512, 128, 512)], ids=["n1024_h256_w1024", "n512_h128_w512"])
def test_griffin_lim_ragged_launch_count(key, monkeypatch):
    st = stft_of(key)
    T, lens = SETTINGS[key]
    M, A = spectrum(key, 4, T, seed=5)
    Md, Ad = M.cuda(), A.cuda()
    calls = count_calls(monkeypatch, DENSE + RAGGED)
    audio_processing.griffin_lim_ragged(Md, lens, st, 3, angles=Ad)
    fam = "r8" if st.fast_path() else "pow2"
    want = {n: 0 for n in DENSE + RAGGED}
    want["ft_istft_%s_ragged" % fam] = 4
    want["ft_stft_%s_ragged_phase" % fam] = 3
    assert calls == want, calls


# ---- 7. mel level -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr,key", [(22050, (1024, 256, 1024)), (16000, (512, 128, 512))], ids=["n1024_h256", "n512_h128"])
def test_mel_level_equals_each_utterance_alone(sr, key):
    tst = audio_processing.TacotronSTFT(key[0], key[1], key[2], 80, sr, 0.0, 8000.0).cuda()
    T, lens = SETTINGS[key]
    hop = key[1]
    rs = np.random.RandomState(31)
    mel = torch.from_numpy(rs.uniform(-9.0, 0.5, (4, 80, T)).astype(np.float32)).cuda()
    mag = tst.mel_to_magnitude_ragged(mel, lens)
    assert mag.shape == (4, key[0] // 2 + 1, T)
    for b, n in enumerate(lens):
        assert torch.equal(mag[b, :, :n], tst.mel_to_magnitude(mel[b:b + 1, :, :n])[0]), b
        assert torch.all(mag[b, :, n:] == 0), b
    A = spectrum(key, 4, T, seed=37)[1].cuda()
    y = tst.mel_to_audio_ragged(mel, lens, 2, angles=A)
    assert y.shape == (4, hop * (T - 1)) and torch.isfinite(y).all()
    for b, n in enumerate(lens):
        own = hop * (n - 1)
        one = tst.mel_to_audio_ragged(mel[b:b + 1, :, :n], [n], 2, angles=A[b:b + 1, :, :n])
        assert torch.equal(y[b, :own], one[0]), b
        assert torch.all(y[b, own:] == 0), b


# ---- 8. end to end: text batch -> mel batch -> waveform batch -----------------------------------------------------------------------
def test_flowtron_infer_ragged_to_audio():
    import flowtron
    from oracle import synth
    os.environ["FLOWTRON_MFMA"] = "f32"
    cfg = dict(synth.SMALL_MODEL_CONFIG)
    m = flowtron.Flowtron(**cfg)
    m.load_state_dict(synth.make_state_dict(cfg, seed=21))
    m = m.cuda().eval()
    out_lens, in_lens = [30, 22], [9, 6]
    b = synth.make_batch(cfg, out_lens, in_lens, seed=21, with_prior=False)
    rs = np.random.RandomState(21)
    residual = torch.from_numpy(rs.standard_normal((2, cfg["n_mel_channels"], 30)).astype(np.float32)).cuda() * 0.5
    with torch.no_grad():                                                    # gate_threshold 1.0: the gate never fires, every
        mel, _, lens = m.infer(residual, b["speaker_ids"][:2].cuda(), b["text"][:2, :9].cuda(), gate_threshold=1.0,
                               in_lens=in_lens, out_lens=out_lens, return_lengths=True)   # utterance keeps its frame budget
    assert lens.tolist() == out_lens and mel.shape == (2, 80, 30)
    tst = audio_processing.TacotronSTFT(1024, 256, 1024, 80, 22050, 0.0, 8000.0).cuda()
    A = spectrum((1024, 256, 1024), 2, 30, seed=41)[1].cuda()
    y = tst.mel_to_audio_ragged(mel, lens, 4, angles=A)
    assert y.shape == (2, 256 * 29) and torch.isfinite(y).all()
    for u, n in enumerate(out_lens):
        own = 256 * (n - 1)
        one = tst.mel_to_audio_ragged(mel[u:u + 1, :, :n], [n], 4, angles=A[u:u + 1, :, :n])
        assert torch.equal(y[u, :own], one[0]), u
        assert torch.all(y[u, own:] == 0), u
        assert y[u, :own].abs().max() > 0
    # the seeded default start: two runs agree
    np.random.seed(0)
    a = tst.mel_to_audio_ragged(mel, lens, 2)
    np.random.seed(0)
    assert torch.equal(a, tst.mel_to_audio_ragged(mel, lens, 2))
    # an utterance the gate (here: its budget) cut too short for the reflect padding is named
    with torch.no_grad():
        mel3, _, lens3 = m.infer(residual, b["speaker_ids"][:2].cuda(), b["text"][:2, :9].cuda(), gate_threshold=1.0,
                                 in_lens=in_lens, out_lens=[30, 3], return_lengths=True)
    with pytest.raises(ValueError, match=r"lengths\[1\] = 3 frames"):
        tst.mel_to_audio_ragged(mel3, lens3, 4)


# ---- 9. validation ----------------------------------------------------------------------------------------------------------------
def test_validation():
    st = audio_processing.STFT(1024, 256, 1024).cuda()
    tst = audio_processing.TacotronSTFT(1024, 256, 1024, 80, 22050, 0.0, 8000.0).cuda()
    M, P = torch.ones(2, 513, 8, device="cuda"), torch.zeros(2, 513, 8, device="cuda")
    y = torch.zeros(2, 4096, device="cuda")
    mel = torch.zeros(2, 80, 8, device="cuda")
    calls = [
        ("n_frames", lambda v: st.inverse_ragged(M, P, v)),
        ("n_frames", lambda v: audio_processing.griffin_lim_ragged(M, v, st, 1)),
        ("lengths", lambda v: tst.mel_to_magnitude_ragged(mel, v)),
        ("lengths", lambda v: tst.mel_to_audio_ragged(mel, v, 1)),
    ]
    for name, f in calls:
        with pytest.raises(ValueError, match=r"%s holds 3 lengths for a batch of 2" % name):
            f([8, 8, 8])
        with pytest.raises(ValueError, match=r"%s\[1\] = 5\.0 is not an integer" % name):
            f([8, 5.0])
        with pytest.raises(ValueError, match=r"%s must be host integers" % name):
            f(torch.tensor([8.0, 5.0]))
        with pytest.raises(ValueError, match=r"%s must be host integers" % name):
            f(torch.tensor([8, 5]).cuda())
        with pytest.raises(ValueError, match=r"%s\[0\] = 9 is outside 1 \.\.= T = 8" % name):
            f([9, 8])
        with pytest.raises(ValueError, match=r"%s\[1\] = 0 is outside 1 \.\.= T = 8" % name):
            f([8, 0])
    for name, f in (calls[1], calls[3]):                                     # griffin_lim's reflect rule, per utterance
        with pytest.raises(ValueError, match=r"%s\[1\] = 3 frames" % name):
            f([8, 3])
    with pytest.raises(ValueError, match=r"n_samples holds 1 lengths for a batch of 2"):
        st.transform_ragged(y, [4096])
    with pytest.raises(ValueError, match=r"n_samples\[0\] = 4000\.5 is not an integer"):
        st.transform_ragged(y, [4000.5, 4096])
    with pytest.raises(ValueError, match=r"n_samples\[1\] = 512 is outside filter_length / 2 = 512 < n <= N = 4096"):
        st.transform_ragged(y, [4096, 512])
    with pytest.raises(ValueError, match=r"n_samples\[0\] = 4097 is outside"):
        st.transform_ragged(y, [4097, 4096])
    with pytest.raises(ValueError, match="angles"):
        audio_processing.griffin_lim_ragged(M, [8, 8], st, 1, angles=torch.zeros(2, 513, 7))
    with pytest.raises(ValueError):
        st.inverse_ragged(M, torch.zeros(2, 513, 7, device="cuda"), [8, 8])
    # sizes outside fast_path() / pow2_path(): the dense functions' NotImplementedError
    odd = audio_processing.STFT(800, 200, 800).cuda()
    Mo = torch.ones(1, 401, 8, device="cuda")
    with pytest.raises(NotImplementedError, match="256/512/1024/2048/4096"):
        odd.transform_ragged(torch.zeros(1, 4000, device="cuda"), [4000])
    with pytest.raises(NotImplementedError, match="256/512/1024/2048/4096"):
        odd.inverse_ragged(Mo, torch.zeros_like(Mo), [8])
    with pytest.raises(NotImplementedError, match="256/512/1024/2048/4096"):
        audio_processing.griffin_lim_ragged(Mo, [8], odd, 1)
    todd = audio_processing.TacotronSTFT(800, 200, 800, 80, 22050, 0.0, 8000.0).cuda()
    with pytest.raises(NotImplementedError, match="256/512/1024/2048/4096"):
        todd.mel_to_audio_ragged(torch.zeros(1, 80, 8, device="cuda"), [8], 1)
    assert todd.mel_to_magnitude_ragged(torch.zeros(1, 80, 8, device="cuda"), [8]).shape == (1, 401, 8)   # a GEMM: any size
