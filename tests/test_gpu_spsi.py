"""The single-pass phase start (ft_spsi_phase, csrc/vocode.hip) on the MI355X: the kernel bit for bit against the float32 replay
of the header's rule (tests/spsi_ref.py), the ragged contract, and phase_init="spsi" through griffin_lim and
TacotronSTFT.mel_to_audio down to the launch count."""
import numpy as np
import pytest
import torch

import audio_processing
import spsi_ref as S
import vocode_ref as R
from call_count import count_calls
from flowtron_amd import audio
from stft_ref64 import istft64, stft64

pytestmark = pytest.mark.gpu

TILE = 16                      # frames of the kernel's tile at n_fft <= 2048 (8 at 4096): one wave per frame
T_LONG = 2 * TILE + 5          # two whole tiles and a part of a third
SETTINGS = [(256, 64), (1024, 256), (1024, 200), (2048, 512), (4096, 1024)]      # the last one on the tile of 8
ALL_LAUNCHES = ["ft_gemm", "ft_mel_nnls", "ft_gl_momentum", "ft_spsi_phase", "ft_stft_r8", "ft_istft_r8", "ft_stft_r8_ragged",
                "ft_stft_pow2", "ft_istft_pow2", "ft_stft_pow2_ragged", "ft_stft_mel", "ft_stft_r8_ragged_phase", "ft_istft_r8_ragged",
                "ft_stft_pow2_ragged_phase", "ft_istft_pow2_ragged"]
_STFT, _TST = {}, {}


def stft_of(n_fft, hop):
    if (n_fft, hop) not in _STFT:
        _STFT[(n_fft, hop)] = audio_processing.STFT(n_fft, hop, n_fft).cuda()
    return _STFT[(n_fft, hop)]


def tacotron_stft():
    if "1024" not in _TST:
        _TST["1024"] = audio_processing.TacotronSTFT(1024, 256, 1024, 80, 22050, 0.0, 8000.0).cuda()
    return _TST["1024"]


def same_bits(got, want):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float32 and want.dtype == np.float32
    same = got.view(np.uint32) == want.view(np.uint32)
    assert same.all(), (int((~same).sum()), np.argwhere(~same)[:4].tolist(), float(np.nanmax(np.abs(got - want))))


def stft_magnitudes(n_fft, hop, seeds, T):
    from oracle import synth
    y = torch.stack([synth.make_audio(hop * (T - 1), seed=s) for s in seeds]).double().numpy()
    return np.abs(stft64(y, n_fft, hop, n_fft)).astype(np.float32)


def adversarial(K, T, seed):
    """[K, T]: uniform noise (a peak every few bins) with plateaus, silent frames (two of them across the first tile's end),
    full-width ramps both ways, one NaN cell and one inf cell."""
    rs = np.random.RandomState(seed)
    M = rs.rand(K, T).astype(np.float32)
    M[:, 3] = 0
    M[:, 5] = np.round(rs.rand(K) * 3)
    M[:, 6] = np.repeat(rs.rand(K // 6 + 1), 6)[:K]
    M[:, 8] = np.arange(K)
    M[:, 9] = np.arange(K)[::-1]
    M[K // 3, 12] = np.nan
    M[:, TILE - 1:TILE + 1] = 0
    M[K // 2, 20] = np.inf
    M[:, 23] = 1.0
    return M


@pytest.mark.parametrize("n_fft,hop", SETTINGS)
def test_spsi_phase_equals_the_float32_replay(n_fft, hop):
    st = stft_of(n_fft, hop)
    K = n_fft // 2 + 1
    # |STFT| of the synthetic audio, a ragged batch: T frames, 9 and none
    M = stft_magnitudes(n_fft, hop, (3, 4, 5), T_LONG)
    lens = [T_LONG, 9, 0]
    want = S.spsi32(M, n_fft, hop, n_frames=lens)
    got = audio.spsi_phase(torch.from_numpy(M).cuda(), st, n_frames=lens)
    same_bits(got, want)
    assert (want[0] != 0).any() and np.abs(want).max() <= np.pi * (1 + 2.0 ** -23)
    same_bits(audio_processing.spsi_phase(torch.from_numpy(M).cuda(), st), S.spsi32(M, n_fft, hop))      # no lengths: every frame
    # adversarial magnitudes
    A = adversarial(K, T_LONG, n_fft + hop)
    with np.errstate(invalid="ignore"):
        want = S.spsi32(A, n_fft, hop)
    assert np.isfinite(want).all()
    same_bits(audio.spsi_phase(torch.from_numpy(A).cuda(), st), want)              # [K, T] goes too
    # T = 1 and T = 3
    for T in (1, 3):
        same_bits(audio.spsi_phase(torch.from_numpy(A[None, :, 10:10 + T].copy()).cuda(), st), S.spsi32(A[None, :, 10:10 + T], n_fft, hop))


def test_spsi_phase_on_nnls_inverted_magnitudes():
    """Magnitudes of the NNLS mel inversion: smooth slopes many bins long, zeros above fmax and where the solver cut off."""
    from oracle import synth
    tst = tacotron_stft()
    y = torch.stack([synth.make_audio(256 * (T_LONG - 1), seed=s) for s in (3, 4)]).cuda()
    mag = tst.mel_to_magnitude(tst.mel_spectrogram(y), method="nnls")
    M = mag.cpu().numpy()
    assert (M[:, :, 400:] == 0).all() and (M[:, :, :372].max(axis=1) > 0).all()
    same_bits(audio.spsi_phase(mag, tst.stft_fn), S.spsi32(M, 1024, 256))


def test_spsi_phase_ragged_contract():
    """What lies behind the lengths is never read (NaN there changes nothing), the output is 0 there, and every utterance equals
    bit for bit the same utterance run alone."""
    n_fft, hop = 1024, 256
    st = stft_of(n_fft, hop)
    lens = [T_LONG, TILE + 1, TILE, 3, 0]
    M = np.stack([adversarial(513, T_LONG, s) for s in range(5)])
    Mn = M.copy()
    for b, n in enumerate(lens):
        Mn[b, :, n:] = np.nan
    Md = torch.from_numpy(Mn).cuda()
    got = audio.spsi_phase(Md, st, n_frames=torch.tensor(lens))
    assert torch.isfinite(got).all()
    for b, n in enumerate(lens):
        assert torch.all(got[b, :, n:] == 0), b
        if n:
            assert torch.equal(got[b, :, :n], audio.spsi_phase(Md[b, :, :n], st)), b
            assert torch.equal(got[b, :, :n], audio.spsi_phase(Md[b:b + 1, :, :n].contiguous(), st, n_frames=[n])[0]), b
    with np.errstate(invalid="ignore"):
        same_bits(got, S.spsi32(M, n_fft, hop, n_frames=lens))


# ---- phase_init="spsi" ---------------------------------------------------------------------------------------------------------
LENS = [40, 29, 17]


@pytest.fixture(scope="module")
def utterances():
    """(tst, log-mel [3, 80, 40] of three synthetic utterances, the frames each holds)"""
    from oracle import synth
    tst = tacotron_stft()
    y = torch.stack([synth.make_audio(256 * 39, seed=s) for s in (3, 4, 5)]).cuda()
    return tst, tst.mel_spectrogram(y), LENS


def test_single_pass_vocode(utterances):
    """mel_to_audio at zero iterations from SPSI, NNLS inversion, a ragged batch of 3: the mean |log-mel error| of the round
    trip is below half of the random start's (the same call without phase_init), and its spectral convergence against the
    inverted magnitudes is within 2 % of the float64 replay's (spsi64 + istft64) for the same magnitudes."""
    tst, mel, lens = utterances
    y = tst.mel_to_audio(mel, n_iters=0, phase_init="spsi", inversion="nnls", lengths=lens)
    np.random.seed(0)
    y_rand = tst.mel_to_audio(mel, n_iters=0, inversion="nnls", lengths=lens)
    assert y.shape == (3, 256 * 39) and torch.isfinite(y).all()
    mag = tst.mel_to_magnitude(mel, method="nnls", lengths=lens).cpu().numpy()

    def logmel_err(audio_):
        tot, cells = 0.0, 0
        for b, n in enumerate(lens):
            back = tst.mel_spectrogram(audio_[b:b + 1, :256 * (n - 1)])
            tot += float((back - mel[b:b + 1, :, :n]).abs().double().sum())
            cells += back.numel()
        return tot / cells
    e_spsi, e_rand = logmel_err(y), logmel_err(y_rand)
    print("zero iterations, NNLS: mean |log-mel error| SPSI %.4f, random %.4f (ratio %.3f)" % (e_spsi, e_rand, e_spsi / e_rand))
    assert e_spsi < 0.5 * e_rand
    for b, n in enumerate(lens):
        own = 256 * (n - 1)
        assert torch.all(y[b, own:] == 0), b
        M = mag[b:b + 1, :, :n]
        sc = R.spectral_convergence(y[b:b + 1, :own].cpu().double().numpy(), M, 1024, 256, 1024)
        sc64 = R.spectral_convergence(istft64(M, S.spsi64(M, 1024, 256), 1024, 256, 1024)[0], M, 1024, 256, 1024)
        print("utterance %d: spectral convergence %.5f (float64 replay %.5f), deviation %.3e" % (b, sc, sc64, abs(sc / sc64 - 1)))
        assert abs(sc / sc64 - 1) <= 0.02, b


@pytest.mark.parametrize("n_iters,momentum", [(0, 0.0), (2, 0.0), (2, 0.99)])
def test_each_ragged_utterance_is_the_call_on_it_alone(utterances, n_iters, momentum):
    tst, mel, lens = utterances
    kw = dict(n_iters=n_iters, momentum=momentum, inversion="nnls", phase_init="spsi")
    y = tst.mel_to_audio(mel, lengths=lens, **kw)
    for b, n in enumerate(lens):
        own = 256 * (n - 1)
        one = tst.mel_to_audio(mel[b:b + 1, :, :n], lengths=[n], **kw)
        assert torch.equal(y[b, :own], one[0]) and torch.all(y[b, own:] == 0) and y[b, :own].abs().max() > 0, b
    # the dense call is the ragged loop with every length T, on the pseudo-inverse as well
    dense = tst.mel_to_audio(mel, n_iters, momentum, phase_init="spsi")
    assert torch.equal(dense, tst.mel_to_audio(mel, n_iters, momentum, lengths=[40, 40, 40], phase_init="spsi"))
    assert torch.equal(dense[1], tst.mel_to_audio(mel[1], n_iters, momentum, phase_init="spsi"))
    mag = tst.mel_to_magnitude(mel)
    assert torch.equal(dense, audio.griffin_lim(mag, tst.stft_fn, n_iters, momentum, phase_init="spsi"))
    start = audio.spsi_phase(mag, tst.stft_fn)
    assert torch.equal(dense, audio.griffin_lim(mag, tst.stft_fn, n_iters, momentum, n_frames=[40, 40, 40], angles=start))


def test_phase_init_random_is_the_call_without_it(utterances):
    tst, mel, lens = utterances
    mag = tst.mel_to_magnitude(mel)

    def twice(fn):
        np.random.seed(5)
        a = fn({})
        np.random.seed(5)
        assert torch.equal(a, fn(dict(phase_init="random")))
        return a
    twice(lambda kw: tst.mel_to_audio(mel, 2, **kw))
    twice(lambda kw: tst.mel_to_audio(mel, 2, momentum=0.99, inversion="nnls", lengths=lens, **kw))
    twice(lambda kw: audio.griffin_lim(mag, tst.stft_fn, 2, **kw))
    a = twice(lambda kw: audio.griffin_lim(mag, tst.stft_fn, 2, n_frames=lens, **kw))
    np.random.seed(5)
    assert torch.equal(a, audio_processing.griffin_lim_ragged(mag, lens, tst.stft_fn, 2))
    assert not torch.equal(a, audio.griffin_lim(mag, tst.stft_fn, 2, n_frames=lens, phase_init="spsi"))


def test_single_pass_vocode_launches(utterances, monkeypatch):
    """inversion (pseudo-inverse GEMM + NNLS), ft_spsi_phase, one inverse STFT: exactly one launch more than the same call
    with the starting angles given."""
    tst, mel, lens = utterances
    A = torch.zeros(3, 513, 40, device="cuda")
    calls = count_calls(monkeypatch, ALL_LAUNCHES)
    tst.mel_to_audio(mel, n_iters=0, inversion="nnls", lengths=lens, angles=A)
    given = dict(calls)
    assert given["ft_spsi_phase"] == 0 and given["ft_istft_r8_ragged"] == 1 and sum(given.values()) == 3, given
    for k in calls:
        calls[k] = 0
    tst.mel_to_audio(mel, n_iters=0, inversion="nnls", lengths=lens, phase_init="spsi")
    assert calls["ft_spsi_phase"] == 1 and sum(calls.values()) == sum(given.values()) + 1, calls
    assert all(calls[k] == given[k] for k in given if k != "ft_spsi_phase"), (calls, given)
    for k in calls:
        calls[k] = 0
    tst.mel_to_audio(mel, n_iters=5, momentum=0.99, inversion="nnls", lengths=lens, phase_init="spsi")
    assert calls["ft_spsi_phase"] == 1 and sum(calls.values()) == 2 + 1 + 1 + 3 * 5, calls
