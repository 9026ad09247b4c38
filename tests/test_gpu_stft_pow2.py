"""The audio front end at every power-of-two analysis size on the MI355X: STFT.transform / inverse (ft_stft_pow2 / ft_istft_pow2),
the mel spectrogram, its ragged one-launch form (ft_stft_pow2_ragged), DeferredMel, griffin_lim and mel_to_audio at n_fft =
256 .. 4096 and hops the 1024 kernels do not take, against the float64 restatement of the reference's formulas
(audio_processing.py:7-75, 96-270) in tests/stft_ref64.py, and against the REAL reference's outputs in tests/golden/stft_pow2.pt
(tests/golden/make_golden_stft_pow2.py).  The 1024 / hop <= 256 setting keeps its own kernels (checked by counting calls).

Measured deviations from the float64 restatement are printed by every test (pytest -s)."""
import os

import numpy as np
import pytest
import torch

import audio_processing
from call_count import count_calls
from flowtron_amd import _lib as L
from stft_ref64 import TINY32, griffin_lim64, istft64, istft_bound, istft_ratio, mel64, rel_l2, start_angles, stft64

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stft_pow2.pt")


def front(tst):
    """mel64's (n_fft, hop, win, fb) of a TacotronSTFT."""
    st = tst.stft_fn
    return st.filter_length, st.hop_length, st.win_length, tst.mel_basis.cpu().double().numpy()


def audio(B, N, seed):
    from oracle import synth
    return torch.stack([synth.make_audio(N, seed=seed + i) for i in range(B)])


# (n_fft, hop, win_length, B, N): every power-of-two size, 1024 at hops above 256, win_length < n_fft with an odd gap,
# hop = 1 on a short signal, hop = win_length (and = n_fft: wss is zero between frames)
GRID = [
    (256, 64, 256, 3, 5000),
    (256, 1, 201, 1, 300),
    (512, 128, 512, 1, 16000),
    (512, 160, 401, 3, 7001),
    (1024, 257, 1024, 1, 9000),
    (1024, 300, 999, 3, 12000),
    (1024, 512, 512, 1, 11025),
    (2048, 512, 2048, 3, 44100),
    (2048, 300, 1200, 1, 24000),
    (4096, 1024, 4096, 1, 30000),
    (4096, 333, 3001, 1, 20000),
    (4096, 4096, 4096, 3, 20000),
]
IDS = ["n%d_h%d_w%d_B%d" % g[:4] for g in GRID]

# Bounds against the float64 restatement, from the estimate ~eps log2 N of an fp32 FFT.  Measured on an MI355X over GRID:
# |X| relative L2 8.2e-8 .. 1.0e-7, phase max 2.2e-5 .. 7.0e-5 (where |X| > 1e-3 max|X|), inverse relative L2 1.2e-7 .. 2.0e-7;
# the real reference's own deviations (dev64 in stft_pow2.pt) are 2.2e-7 .. 7.0e-7 (transform) and 3.1e-7 .. 3.5e-7 (inverse).
MAG_BOUND, PHASE_BOUND, INV_BOUND = 1e-6, 1e-4, 1e-6


@pytest.mark.parametrize("n_fft,hop,win,B,N", GRID, ids=IDS)
def test_transform_matches_float64(n_fft, hop, win, B, N):
    st = audio_processing.STFT(n_fft, hop, win).cuda()
    assert st.pow2_path() and not st.fast_path()
    y = audio(B, N, seed=n_fft + hop)
    mag, phase = st.transform(y.cuda())
    T = N // hop + 1
    assert mag.shape == (B, n_fft // 2 + 1, T) and phase.shape == mag.shape
    X = stft64(y.numpy(), n_fft, hop, win)
    m, p = mag.cpu().double().numpy(), phase.cpu().double().numpy()
    e_mag = rel_l2(m, np.abs(X))
    strong = np.abs(X) > 1e-3 * np.abs(X).max()
    dphi = np.remainder(p - np.angle(X) + np.pi, 2 * np.pi) - np.pi
    e_ph = float(np.abs(dphi[strong]).max())
    print("transform n_fft %d hop %d win %d: |X| rel L2 %.2e, phase max %.2e" % (n_fft, hop, win, e_mag, e_ph))
    assert e_mag <= MAG_BOUND
    assert e_ph <= PHASE_BOUND
    # determinism: a second launch is bitwise equal
    mag2, phase2 = st.transform(y.cuda())
    assert torch.equal(mag, mag2) and torch.equal(phase, phase2)


@pytest.mark.parametrize("n_fft,hop,win,B,N", GRID, ids=IDS)
def test_inverse_matches_float64(n_fft, hop, win, B, N):
    st = audio_processing.STFT(n_fft, hop, win).cuda()
    T = max(2, min(N // hop + 1, 40))
    rs = np.random.RandomState(n_fft + 7 * hop + T)
    M = rs.uniform(0.0, 2.0, (B, n_fft // 2 + 1, T)).astype(np.float32)
    P = rs.uniform(-np.pi, np.pi, (B, n_fft // 2 + 1, T)).astype(np.float32)
    y = st.inverse(torch.from_numpy(M).cuda(), torch.from_numpy(P).cuda())
    assert y.shape == (B, 1, hop * (T - 1))
    y64, wss = istft64(M, P, n_fft, hop, win)
    got = y[:, 0].cpu().double().numpy()
    e = rel_l2(got, y64)
    zero = wss <= TINY32
    print("inverse n_fft %d hop %d win %d T %d: rel L2 %.2e, %d samples with wss <= FLT_MIN" % (n_fft, hop, win, T, e, zero.sum()))
    assert e <= INV_BOUND
    assert np.all(got[:, zero] == 0)
    # every sample by itself (stft_ref64.istft_bound), against the float64 inverse on the very float32 window the kernel read
    w32 = st.fft_window.cpu().numpy()
    ratio = istft_ratio(got, istft64(M, P, n_fft, hop, win, w32)[0], istft_bound(M, P, n_fft, hop, win, None, w32))
    print("inverse n_fft %d hop %d win %d T %d: max |gpu - f64| / bound = %.3g" % (n_fft, hop, win, T, ratio.max()))
    assert ratio.max() <= 1.0, (ratio.max(), np.unravel_index(ratio.argmax(), ratio.shape))
    y2 = st.inverse(torch.from_numpy(M).cuda(), torch.from_numpy(P).cuda())
    assert torch.equal(y, y2)


def test_inverse_of_transform_round_trip():
    """forward(y) = inverse(transform(y)) gives y back at 2048 / 512 (overlap-add of a hann-windowed STFT is exact)."""
    st = audio_processing.STFT(2048, 512, 2048).cuda()
    y = audio(2, 44100, seed=3).cuda()
    r = st(y)
    n = 512 * (44100 // 512)
    assert r.shape == (2, 1, n)
    err = (r[:, 0] - y[:, :n]).abs().max().item()
    print("round trip 2048 / 512: max err %.2e" % err)
    assert err < 1e-5


# ---- mel: ragged batch, old path, launch counts ------------------------------------------------------------------------------
RAGGED = [  # (sr, n_fft, hop, win, n_mel, fmax)
    (16000, 512, 128, 512, 80, 8000.0),
    (22050, 1024, 300, 1024, 80, 8000.0),
    (24000, 2048, 300, 1200, 80, 8000.0),
    (44100, 2048, 512, 2048, 80, 8000.0),
    (44100, 4096, 512, 4096, 128, None),       # fmax = sr / 2: ~4 000 filterbank weights, read from global memory
    (16000, 256, 1, 256, 40, None),
]


@pytest.mark.parametrize("sr,n_fft,hop,win,n_mel,fmax", RAGGED)
def test_ragged_mel_equals_each_utterance(sr, n_fft, hop, win, n_mel, fmax):
    tst = audio_processing.TacotronSTFT(n_fft, hop, win, n_mel, sr, 0.0, fmax).cuda()
    assert tst.ragged_path()
    if fmax is None and n_fft == 4096:
        assert tst.fb_w.numel() > 2048                                    # the global-memory filterbank branch
    short = n_fft // 2 + 1
    lens = [short, 3 * n_fft + 17, 5 * n_fft + hop // 2] if hop > 1 else [short, 700, 450]
    N = max(lens)
    y = torch.zeros(len(lens), N)
    for i, n in enumerate(lens):
        y[i, :n] = audio(1, n, seed=40 + i)[0]
    frames = [n // hop + 1 for n in lens]
    T_out = max(frames) + 3
    mel = tst.mel_spectrogram_ragged(y.cuda(), torch.tensor(lens, dtype=torch.int32).cuda(), T_out)
    assert mel.shape == (len(lens), n_mel, T_out)
    for i, (n, t) in enumerate(zip(lens, frames)):
        one = tst.mel_spectrogram(y[i:i + 1, :n].cuda())
        assert one.shape == (1, n_mel, t)
        assert torch.equal(mel[i, :, :t], one[0]), i
        assert torch.all(mel[i, :, t:] == 0), i
        e = np.abs(one[0].cpu().double().numpy() - mel64(y[i:i + 1, :n].numpy(), *front(tst))[0]).max()
        print("mel sr %d n_fft %d hop %d n_mel %d, utterance %d (%d samples): max |log-mel - f64| %.2e" % (sr, n_fft, hop, n_mel, i, n, e))
        assert e < 2e-4


@pytest.mark.parametrize("sr,n_fft,hop,win", [(16000, 512, 128, 512), (24000, 2048, 300, 1200), (44100, 2048, 512, 2048),
                                              (22050, 1024, 512, 1024), (44100, 4096, 1024, 4096)])
def test_mel_agrees_with_general_kernel(sr, n_fft, hop, win):
    """The mel of these settings moved from ft_stft_mel (complex radix-2 FFT, dense filterbank) to ft_stft_pow2: the two
    agree within the 2e-4 test_gpu_model allows between ft_stft_mel and ft_stft_r8 at 1024."""
    tst = audio_processing.TacotronSTFT(n_fft, hop, win, 80, sr, 0.0, 8000.0).cuda()
    y = audio(2, 3 * sr // 2, seed=n_fft).cuda()
    mel = tst.mel_spectrogram(y)
    dense = torch.empty_like(mel)
    st = tst.stft_fn
    L.check(L.lib().ft_stft_mel(L.ptr(y), L.ptr(st.fft_window), L.ptr(tst.mel_basis), L.ptr(dense), 2, y.shape[1], n_fft, hop, 80,
                                L.stream()), "ft_stft_mel")
    d = (mel - dense).abs().max().item()
    print("mel n_fft %d hop %d: max |pow2 - ft_stft_mel| %.2e" % (n_fft, hop, d))
    assert d < 2e-4


def test_deferred_mel_one_launch_at_44k(monkeypatch):
    from flowtron_amd.data import DeferredMel
    args = dict(filter_length=2048, hop_length=512, win_length=2048, n_mel_channels=80, sampling_rate=44100, mel_fmin=0.0,
                mel_fmax=8000.0)
    lens = [44100 * s // 4 for s in (8, 3, 5, 7, 2, 6, 4, 1)]
    lens[-1] = 1025                                                          # just over n_fft / 2
    y = torch.zeros(8, max(lens))
    for i, n in enumerate(lens):
        y[i, :n] = audio(1, n, seed=60 + i)[0]
    slot = DeferredMel(y, torch.tensor(lens), args)
    calls = count_calls(monkeypatch, ["ft_stft_pow2_ragged", "ft_stft_pow2", "ft_stft_mel", "ft_stft_r8_ragged"])
    mel = slot.cuda()
    assert calls == {"ft_stft_pow2_ragged": 1, "ft_stft_pow2": 0, "ft_stft_mel": 0, "ft_stft_r8_ragged": 0}, calls
    tst = audio_processing.TacotronSTFT(2048, 512, 2048, 80, 44100, 0.0, 8000.0).cuda()
    T = max(n // 512 + 1 for n in lens)
    assert mel.shape == (8, 80, T)
    for i, n in enumerate(lens):
        t = n // 512 + 1
        assert torch.equal(mel[i, :, :t], tst.mel_spectrogram(y[i:i + 1, :n].cuda())[0])
        assert torch.all(mel[i, :, t:] == 0)


def test_collate_batch_at_44k():
    """A batch through DataCollate / DeferredMel at 44.1 kHz / 2048 / 512: the mel slot is computed on the device and every
    utterance matches the float64 restatement."""
    from flowtron_amd.data import AudioItem, DataCollate, DeferredMel
    args = dict(filter_length=2048, hop_length=512, win_length=2048, n_mel_channels=80, sampling_rate=44100, mel_fmin=0.0,
                mel_fmax=8000.0)
    lens = [30000, 52000, 41000]
    items = []
    for i, n in enumerate(lens):
        a = audio(1, n, seed=80 + i)[0]
        items.append((AudioItem(a, n // 512 + 1, args), torch.tensor([0]), torch.randint(1, 50, (5 + i,))))
    batch = DataCollate(1, False)(items)
    assert isinstance(batch[0], DeferredMel)
    mel = batch[0].cuda()
    tst = audio_processing.TacotronSTFT(**args).cuda()
    order = batch[4].tolist()                                                # output lengths in the collated order
    for i in range(3):
        n = int(batch[0].n_samples[i])
        t = n // 512 + 1
        assert t == order[i]
        ref = mel64(batch[0].audio[i:i + 1, :n].numpy(), *front(tst))[0]
        e = np.abs(mel[i, :, :t].cpu().double().numpy() - ref).max()
        print("collated utterance %d: max |log-mel - f64| %.2e" % (i, e))
        assert e < 2e-4
        assert torch.all(mel[i, :, t:] == 0)


def test_mel_of_10s_clip_at_44k():
    tst = audio_processing.TacotronSTFT(2048, 512, 2048, 80, 44100, 0.0, 8000.0).cuda()
    y = audio(1, 441000, seed=5)
    mel = tst.mel_spectrogram(y.cuda())
    assert mel.shape == (1, 80, 441000 // 512 + 1)
    ref = mel64(y.numpy(), *front(tst))
    e = np.abs(mel.cpu().double().numpy() - ref).max()
    print("10 s clip at 44.1 kHz: max |log-mel - f64| %.2e, rel L2 %.2e" % (e, rel_l2(mel.cpu().numpy(), ref)))
    assert e < 2e-4


# ---- synthesis ----------------------------------------------------------------------------------------------------------------
def test_mel_to_audio_at_2048():
    tst = audio_processing.TacotronSTFT(2048, 512, 2048, 80, 44100, 0.0, 8000.0).cuda()
    mel = tst.mel_spectrogram(audio(2, 44100, seed=9).cuda())
    T = mel.shape[2]
    np.random.seed(3)
    a = tst.mel_to_audio(mel, n_iters=4)
    np.random.seed(3)
    b = tst.mel_to_audio(mel, n_iters=4)
    assert a.shape == (2, 512 * (T - 1)) and torch.isfinite(a).all()
    assert torch.equal(a, b)
    # zero iterations: pinv(mel_basis) magnitudes + the seeded starting phase, against float64
    np.random.seed(3)
    y0 = tst.mel_to_audio(mel, n_iters=0).cpu().double().numpy()
    Mag = np.maximum(tst.mel_pinv.cpu().double().numpy() @ np.exp(mel.cpu().double().numpy()), 0)
    ref = istft64(Mag, start_angles(Mag.shape, seed=3), 2048, 512, 2048)[0]
    e = rel_l2(y0, ref)
    print("mel_to_audio 2048 / 512, 0 iterations: rel L2 vs f64 %.2e" % e)
    assert e < 1e-6                                                          # measured 1.6e-7


def test_griffin_lim_deterministic_and_matches_float64():
    st = audio_processing.STFT(2048, 300, 1200).cuda()
    y = audio(1, 24000, seed=12)
    M = np.abs(stft64(y.numpy(), 2048, 300, 1200)).astype(np.float32)
    Md = torch.from_numpy(M).cuda()
    outs = []
    for _ in range(2):
        np.random.seed(0)
        outs.append(audio_processing.griffin_lim(Md, st, 8))
    assert torch.equal(outs[0], outs[1])
    d = rel_l2(outs[0].cpu().numpy(), griffin_lim64(M, start_angles(M.shape), 8, 2048, 300, 1200))
    print("griffin_lim 2048 / 300 / 1200, 8 iterations: rel L2 vs f64 %.2e" % d)
    assert d < 1e-4                                                          # measured 9.1e-6


# ---- reference goldens ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN, weights_only=False)


@pytest.mark.parametrize("name", ["sr16k", "sr24k", "sr44k"])
def test_reference_goldens(golden, name):
    sr, n_fft, hop, win = golden["settings"][name]
    g = golden[name]
    tst = audio_processing.TacotronSTFT(n_fft, hop, win, 80, sr, 0.0, 8000.0).cuda()
    st = tst.stft_fn
    # mel_spectrogram
    y = audio(1, g["mel"]["n_samples"], seed=g["mel"]["audio_seed"])
    mel = tst.mel_spectrogram(y.cuda())[0].cpu()
    e = rel_l2(mel, g["mel"]["mel"])
    print("%s mel: gpu vs reference %.2e (reference vs f64 %.2e)" % (name, e, g["mel"]["dev64"]))
    assert e <= 10 * g["mel"]["dev64"]
    # STFT.transform magnitude columns
    mag, _ = st.transform(y.cuda())
    e = rel_l2(mag[0, :, ::golden["mag_stride"]].cpu(), g["transform"]["mag"])
    print("%s transform: gpu vs reference %.2e (reference vs f64 %.2e)" % (name, e, g["transform"]["dev64"]))
    assert e <= 10 * g["transform"]["dev64"]
    # STFT.inverse on the seeded spectrum
    gi = g["inverse"]
    rs = np.random.RandomState(gi["seed"])
    M = rs.uniform(0.0, 2.0, (gi["B"], n_fft // 2 + 1, gi["T"])).astype(np.float32)
    P = rs.uniform(-np.pi, np.pi, (gi["B"], n_fft // 2 + 1, gi["T"])).astype(np.float32)
    yi = st.inverse(torch.from_numpy(M).cuda(), torch.from_numpy(P).cuda())[:, 0, ::golden["y_stride"]].cpu()
    e = rel_l2(yi, gi["y"])
    print("%s inverse: gpu vs reference %.2e (reference vs f64 %.2e)" % (name, e, gi["dev64"]))
    assert e <= 10 * gi["dev64"]
    # griffin_lim at 0 / 1 / 8 iterations, against float64 (the rule of test_gpu_griffin_lim.py)
    gg = g["gl"]
    Mg = np.abs(stft64(audio(1, gg["n_samples"], seed=gg["audio_seed"]).numpy(), n_fft, hop, win)).astype(np.float32)
    assert np.array_equal(Mg.reshape(-1)[::997], gg["mag"]["sample"].numpy())
    for it in gg["n_iters"]:
        np.random.seed(0)
        out = audio_processing.griffin_lim(torch.from_numpy(Mg).cuda(), st, it).cpu().numpy()
        d64 = rel_l2(out, griffin_lim64(Mg, start_angles(Mg.shape), it, n_fft, hop, win))
        print("%s griffin_lim %d: gpu vs f64 %.2e, vs reference %.2e (reference vs f64 %.2e)"
              % (name, it, d64, rel_l2(out[:, ::golden["y_stride"]], gg["y"][it]), gg["dev64"][it]))
        assert d64 <= 10 * gg["dev64"][it]


# ---- unchanged paths ---------------------------------------------------------------------------------------------------------
def test_1024_keeps_its_kernels(monkeypatch):
    names = ["ft_stft_r8", "ft_istft_r8", "ft_stft_r8_ragged", "ft_stft_pow2", "ft_istft_pow2", "ft_stft_pow2_ragged", "ft_stft_mel"]
    calls = count_calls(monkeypatch, names)
    tst = audio_processing.TacotronSTFT(1024, 256, 1024, 80, 22050, 0.0, 8000.0).cuda()
    y = audio(1, 22050, seed=1).cuda()
    mag, ph = tst.stft_fn.transform(y)
    tst.mel_spectrogram(y)
    tst.stft_fn.inverse(mag, ph)
    tst.mel_spectrogram_ragged(y, torch.tensor([22050], dtype=torch.int32).cuda())
    assert calls == {"ft_stft_r8": 2, "ft_istft_r8": 1, "ft_stft_r8_ragged": 1, "ft_stft_pow2": 0, "ft_istft_pow2": 0,
                     "ft_stft_pow2_ragged": 0, "ft_stft_mel": 0}, calls


def test_non_power_of_two_still_raises():
    st = audio_processing.STFT(800, 200, 800).cuda()
    assert not st.pow2_path()
    with pytest.raises(NotImplementedError, match="256/512/1024/2048/4096"):
        st.transform(torch.zeros(1, 4000, device="cuda"))
    with pytest.raises(NotImplementedError):
        st.inverse(torch.ones(1, 401, 8, device="cuda"), torch.zeros(1, 401, 8, device="cuda"))
