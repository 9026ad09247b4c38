"""NNLS mel inversion (ft_mel_nnls) and fast Griffin-Lim (ft_gl_momentum) on the MI355X, csrc/vocode.hip: the solver bit
for bit against the float32 replay of the header's rule, the momentum step and the loops around it against float64
(tests/vocode_ref.py, tests/stft_ref64.py), launch counts, the per-utterance promise of the ragged forms, and the path from the
model to audio."""
import os

import numpy as np
import pytest
import torch

import audio_processing
import vocode_ref as R
from call_count import count_calls
from flowtron_amd import _lib as L
from flowtron_amd import audio
from stft_ref64 import griffin_lim64, start_angles, stft64

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
ALL_LAUNCHES = ["ft_gemm", "ft_mel_nnls", "ft_gl_momentum", "ft_stft_r8", "ft_istft_r8", "ft_stft_r8_ragged", "ft_stft_pow2",
                "ft_istft_pow2", "ft_stft_pow2_ragged", "ft_stft_mel", "ft_stft_r8_ragged_phase", "ft_istft_r8_ragged",
                "ft_stft_pow2_ragged_phase", "ft_istft_pow2_ragged"]

# name -> (sampling rate, n_fft, hop, bands, fmax, B, T, lengths or None)
NNLS_CASES = {
    "1024": (22050, 1024, 256, 80, 8000.0, 3, 37, (37, 16, 1)),     # 513 = 8 x 64 + 1 bins, 142 uncovered, a tile not full
    "256": (16000, 256, 64, 40, None, 1, 48, None),                 # whole tiles of 16 frames, no lengths
    "4096": (44100, 4096, 1024, 128, None, 2, 5, (5, 3)),           # the largest LDS footprint
}
_TST, _NNLS = {}, {}


def tacotron_stft(name):
    if name not in _TST:
        sr, n_fft, hop, n_mel, fmax = NNLS_CASES[name][:5]
        _TST[name] = audio_processing.TacotronSTFT(n_fft, hop, n_fft, n_mel, sr, 0.0, fmax).cuda()
    return _TST[name]


def nnls_case(name):
    """(log-mel, s, m0 on the device; the float32 iterates 0 .. 100 of every frame on the host [n_iters + 1][B, nb, T]), once."""
    if name not in _NNLS:
        n_mel, B, T = NNLS_CASES[name][3], NNLS_CASES[name][5], NNLS_CASES[name][6]
        tst = tacotron_stft(name)
        rs = np.random.RandomState(11)
        mel = rs.uniform(-8, 2, (B, n_mel, T)).astype(np.float32)
        if name == "1024":
            mel[0, :, 5] = -11.5                                  # the floor of the log compression everywhere
            mel[0, :, 7] = -np.inf                                # an all-zero frame
        mel = torch.from_numpy(mel).cuda()
        s = torch.exp(mel).contiguous()
        m0 = tst.mel_to_magnitude(mel)
        W = tst.mel_basis.cpu().numpy()
        sh, mh = s.cpu().numpy(), m0.cpu().numpy()
        hist = R.nnls32(W, np.concatenate(list(sh), axis=1), np.concatenate(list(mh), axis=1), 100, history=True)
        hist = [np.stack(np.split(h, B, axis=1)) for h in hist]
        _NNLS[name] = (mel, s, m0, hist)
    return _NNLS[name]


def run_nnls(tst, s, m0, lens, n_iters, out=None):
    """ft_mel_nnls itself, with the module's own tables."""
    B, n_mel, T = s.shape
    band, weight = tst._bin_table(s.device)
    nf = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=s.device)
    out = torch.full_like(m0, 7.0) if out is None else out
    L.check(L.lib().ft_mel_nnls(L.ptr(s), L.ptr(m0), L.ptr(out), L.ptr(nf), L.ptr(tst.fb_bin0), L.ptr(tst.fb_ptr), L.ptr(tst.fb_w),
                                L.ptr(band), L.ptr(weight), B, n_mel, tst.stft_fn.filter_length, T, tst.fb_w.numel(), n_iters,
                                L.stream()), "ft_mel_nnls")
    return out


def expected(hist_n, lens):
    want = hist_n.copy()
    if lens is not None:
        for b, n in enumerate(lens):
            want[b, :, n:] = 0
    return want


# ---- ft_mel_nnls ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n_iters", [("1024", 0), ("1024", 1), ("1024", 100), ("256", 100), ("4096", 100)])
def test_mel_nnls_equals_the_float32_replay(name, n_iters):
    lens = NNLS_CASES[name][7]
    tst = tacotron_stft(name)
    _, s, m0, hist = nnls_case(name)
    got = run_nnls(tst, s, m0, lens, n_iters).cpu().numpy()
    want = expected(hist[n_iters], lens)
    assert got.shape == want.shape and got.dtype == np.float32
    same = got.view(np.uint32) == want.view(np.uint32)
    assert same.all(), (int((~same).sum()), np.argwhere(~same)[:4], float(np.abs(got - want).max()))
    if name == "1024":
        assert (got[0, :, 7] == 0).all()                           # the all-zero frame
        covered = tst.mel_basis.cpu().numpy().sum(axis=0) > 0
        assert (got[:, ~covered] == 0).all() and (~covered).sum() == 142
        assert (got[0, covered, 5] > 0).all()                      # exp(-11.5) everywhere is not silence
        if n_iters == 100:
            assert not np.array_equal(got, expected(hist[99], lens))


@pytest.mark.parametrize("name", ["1024", "4096"])
def test_mel_nnls_never_reads_behind_a_length(name):
    lens = NNLS_CASES[name][7]
    tst = tacotron_stft(name)
    _, s, m0, hist = nnls_case(name)
    s2, m2 = s.clone(), m0.clone()
    for b, n in enumerate(lens):
        s2[b, :, n:] = float("nan")
        m2[b, :, n:] = float("nan")
    want = expected(hist[3], lens)
    got = run_nnls(tst, s2, m2, lens, 3)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    run_nnls(tst, s2, m2, lens, 3, out=m2)                          # in place on the estimate, as mel_to_magnitude calls it
    assert np.array_equal(m2.cpu().numpy().view(np.uint32), want.view(np.uint32))


def test_method_nnls_against_method_pinv(monkeypatch):
    tst = tacotron_stft("1024")
    rs = np.random.RandomState(12)
    mel = torch.from_numpy(rs.uniform(-8, 2, (3, 80, 37)).astype(np.float32)).cuda()
    calls = count_calls(monkeypatch, ALL_LAUNCHES)
    base = tst.mel_to_magnitude(mel)
    n_base = dict(calls)
    assert sum(n_base.values()) == 1 and n_base["ft_gemm"] == 1
    assert torch.equal(base, tst.mel_to_magnitude(mel, method="pinv"))
    assert torch.equal(base, tst.mel_to_magnitude(mel, "pinv", 100))
    for k in calls:
        calls[k] = 0
    mag = tst.mel_to_magnitude(mel, method="nnls")
    assert sum(calls.values()) == 2 and calls["ft_gemm"] == 1 and calls["ft_mel_nnls"] == 1, calls
    W = tst.mel_basis.cpu().numpy()
    s = np.exp(mel.cpu().double().numpy())
    worst = 0.0
    for b in range(3):
        before, after = R.residual(W, base[b].cpu().numpy(), s[b]), R.residual(W, mag[b].cpu().numpy(), s[b])
        assert (after < before).all(), (b, np.nonzero(after >= before)[0])
        worst = max(worst, float((after / before).max()))
    print("uniform log-mels: worst frame keeps %.3f of the pinv + ReLU residual" % worst)
    # the keyword reaches the kernel: fewer iterations give other bits, 0 gives the start
    assert not torch.equal(mag, tst.mel_to_magnitude(mel, method="nnls", n_iters=99))
    assert torch.equal(tst.mel_to_magnitude(mel, method="nnls", n_iters=0), run_nnls(tst, torch.exp(mel), base, None, 0))
    assert torch.equal(tst.mel_to_magnitude(mel[1], method="nnls"), mag[1])
    # ragged: one launch behind the GEMM, no masked fill; every utterance as inverted alone
    lens = [37, 16, 1]
    for k in calls:
        calls[k] = 0
    rag = tst.mel_to_magnitude(mel, method="nnls", lengths=lens)
    assert sum(calls.values()) == 2 and calls["ft_mel_nnls"] == 1, calls
    for b, n in enumerate(lens):
        assert torch.equal(rag[b, :, :n], tst.mel_to_magnitude(mel[b:b + 1, :, :n], method="nnls")[0]), b
        assert torch.equal(rag[b, :, :n], mag[b, :, :n]) and torch.all(rag[b, :, n:] == 0), b
    assert torch.equal(tst.mel_to_magnitude_ragged(mel, lens), tst.mel_to_magnitude(mel, method="pinv", lengths=lens))


# ---- ft_gl_momentum ---------------------------------------------------------------------------------------------------------------
ALPHA32 = float(np.float32(0.99))


def _momentum_inputs():
    rs = np.random.RandomState(13)
    shape = (2, 513, 19)
    M = rs.uniform(0.0, 2.0, shape).astype(np.float32)
    P = rs.uniform(-np.pi, np.pi, shape).astype(np.float32)
    pre, pim = rs.standard_normal(shape).astype(np.float32), rs.standard_normal(shape).astype(np.float32)
    return M, P, pre, pim


def _run_momentum(M, P, pre, pim, lens, first):
    d = [torch.from_numpy(a.copy()).cuda() for a in (M, P, pre, pim)]
    nf = None if lens is None else torch.tensor(lens, dtype=torch.int32, device="cuda")
    L.check(L.lib().ft_gl_momentum(L.ptr(d[0]), L.ptr(d[1]), L.ptr(d[2]), L.ptr(d[3]), L.ptr(nf), M.shape[0], M.shape[1], M.shape[2],
                                   0.99, first, L.stream()), "ft_gl_momentum")
    return [a.cpu().numpy() for a in d[1:]]


def test_gl_momentum_against_float64():
    """The bound.  cos and sin carry at most 4 ulp (the bound sincosf is built to) and the product with M half an ulp more:
    each component of c is off by at most 4.5 eps |c|.  t = c + alpha (c - c_prev) takes that (1 + alpha) times and adds the
    roundings of the difference and of the product (half an eps of alpha (|c| + |c_prev|) each) and of the sum (half an eps of
    |t| <= (1 + alpha) |c| + alpha |c_prev|): per component at most 6 eps ((1 + alpha) |c| + alpha |c_prev|), for the vector
    sqrt(2) times that: c = 9.  Divided by |t| it is the angle's error to first order (cells with |t| below 1e-3 of the numerator
    are left out: there the error is no small angle).  atan2f adds at most 6 ulp of an angle up to pi, an ulp of which is at
    most 2 eps: 12 eps."""
    M, P, pre, pim = _momentum_inputs()
    lens = (19, 7)
    Mn = M.copy()
    for b, n in enumerate(lens):
        Mn[b, :, n:] = np.nan                                       # what lies behind an utterance is not read
    ph, ore, oim = _run_momentum(Mn, P, pre, pim, lens, 0)
    live = np.zeros(M.shape, bool)
    for b, n in enumerate(lens):
        live[b, :, :n] = True
    for got, was in ((ph, P), (ore, pre), (oim, pim)):
        assert np.array_equal(got[~live].view(np.uint32), was[~live].view(np.uint32))
    c = M.astype(np.float64) * np.exp(1j * P.astype(np.float64))
    prev = pre.astype(np.float64) + 1j * pim.astype(np.float64)
    t = c + ALPHA32 * (c - prev)
    num = (1 + ALPHA32) * np.abs(c) + ALPHA32 * np.abs(prev)
    keep = live & (np.abs(t) >= 1e-3 * num)
    assert (live & ~keep).sum() <= 0.01 * live.sum()
    err = np.abs(np.exp(1j * ph.astype(np.float64)) - t / np.abs(t))
    bound = 9 * EPS32 * num / np.abs(t) + 12 * EPS32
    print("momentum step: worst error / bound %.3f, %d of %d cells left out" % ((err / bound)[keep].max(), (live & ~keep).sum(), live.sum()))
    assert (err <= bound)[keep].all()
    assert np.isfinite(ph[live]).all() and (np.abs(ph[live]) <= np.float32(np.pi)).all()
    assert (np.abs(ore - c.real) <= 5 * EPS32 * M)[live].all() and (np.abs(oim - c.imag) <= 5 * EPS32 * M)[live].all()
    # first = 1: the phase passes through, c_prev is stored
    ph1, ore1, oim1 = _run_momentum(Mn, P, pre, pim, lens, 1)
    assert np.array_equal(ph1.view(np.uint32), P.view(np.uint32))
    assert np.array_equal(ore1.view(np.uint32), ore.view(np.uint32)) and np.array_equal(oim1.view(np.uint32), oim.view(np.uint32))
    # no lengths: every cell
    ph2, ore2, _ = _run_momentum(M, P, pre, pim, None, 0)
    assert np.array_equal(ph2[live].view(np.uint32), ph[live].view(np.uint32)) and np.isfinite(ph2).all()
    assert not np.array_equal(ore2[~live], pre[~live])


# ---- griffin_lim with momentum ----------------------------------------------------------------------------------------------------
GL_DEV = 0.01          # |sc(device) / sc(float64) - 1|: the plain path's bound (test_griffin_lim_vs_float64)


def _magnitudes(seeds, n_fft=1024, hop=256, T=41):
    from oracle import synth
    y = torch.stack([synth.make_audio(hop * (T - 1), seed=s) for s in seeds]).double().numpy()
    return np.abs(stft64(y, n_fft, hop, n_fft)).astype(np.float32)


@pytest.fixture(scope="module")
def gl41():
    """(M [2, 513, 41], the float64 replays' spectral convergence {(momentum, n_iters): sc})"""
    M = _magnitudes((3, 4))
    a = start_angles(M.shape, 0)
    sc = {}
    for n in (8, 30):
        sc[(0.99, n)] = R.spectral_convergence(R.fast_griffin_lim64(M, a, n, 1024, 256, 1024, ALPHA32), M, 1024, 256, 1024)
    sc[(0.0, 30)] = R.spectral_convergence(griffin_lim64(M, a, 30, 1024, 256, 1024), M, 1024, 256, 1024)
    return M, sc


def _gl(M, st, n, seed=0, **kw):
    np.random.seed(seed)
    return audio.griffin_lim(torch.from_numpy(M).cuda(), st, n, **kw)


def test_griffin_lim_momentum_against_float64(gl41):
    """Spectral convergence of the device's fast Griffin-Lim against the float64 replay, from the same starting angles.
    Measured on the MI355X: |sc / sc64 - 1| = 1.2e-7 at 8 iterations and 3.7e-7 at 30 (3.4e-9 at 512 / 128, 8 iterations):
    momentum does not lift the deviation above the plain path's bound of 1 %, which therefore stays."""
    M, sc64 = gl41
    st = audio_processing.STFT(1024, 256, 1024).cuda()
    sc = {}
    for n in (8, 30):
        y = _gl(M, st, n, momentum=0.99).cpu().double().numpy()
        sc[n] = R.spectral_convergence(y, M, 1024, 256, 1024)
        print("fast Griffin-Lim n_iters %d: spectral convergence %.5f (float64 %.5f), deviation %.3e"
              % (n, sc[n], sc64[(0.99, n)], abs(sc[n] / sc64[(0.99, n)] - 1)))
    plain = R.spectral_convergence(_gl(M, st, 30).cpu().double().numpy(), M, 1024, 256, 1024)
    print("plain n_iters 30: %.5f (float64 %.5f); fast / plain %.3f" % (plain, sc64[(0.0, 30)], sc[30] / plain))
    for n in (8, 30):
        assert abs(sc[n] / sc64[(0.99, n)] - 1) <= GL_DEV, n
    assert sc[30] <= 0.8 * plain


def test_griffin_lim_momentum_bits_and_launches(gl41, monkeypatch):
    M = gl41[0]
    st = audio_processing.STFT(1024, 256, 1024).cuda()
    assert torch.equal(_gl(M, st, 1, momentum=0.99), _gl(M, st, 1))
    assert torch.equal(_gl(M, st, 0, momentum=0.99), _gl(M, st, 0))
    a = _gl(M, st, 6, momentum=0.99)
    assert torch.equal(a, _gl(M, st, 6, momentum=0.99))
    assert not torch.equal(a, _gl(M, st, 6)) and not torch.equal(a, _gl(M, st, 6, momentum=0.5))
    calls = count_calls(monkeypatch, ALL_LAUNCHES)
    plain = _gl(M, st, 6)
    assert calls["ft_istft_r8"] == 7 and calls["ft_stft_r8"] == 6 and sum(calls.values()) == 13, calls
    for k in calls:
        calls[k] = 0
    assert torch.equal(plain, _gl(M, st, 6, momentum=0.0))
    assert sum(calls.values()) == 13 and calls["ft_gl_momentum"] == 0, calls
    np.random.seed(0)                                               # the drop-in name keeps the reference's signature
    assert torch.equal(plain, audio_processing.griffin_lim(torch.from_numpy(M).cuda(), st, 6))
    for k in calls:
        calls[k] = 0
    _gl(M, st, 6, momentum=0.99)
    assert calls["ft_istft_r8"] == 7 and calls["ft_stft_r8"] == 6 and calls["ft_gl_momentum"] == 6 and sum(calls.values()) == 19, calls


@pytest.mark.parametrize("key", [(1024, 256), (512, 128)])
def test_griffin_lim_ragged_momentum(key, monkeypatch):
    n_fft, hop = key
    lens = [41, 23, 9]
    M = _magnitudes((3, 4, 5), n_fft, hop, 41)
    Mn = M.copy()
    for b, n in enumerate(lens):
        Mn[b, :, n:] = np.nan
    st = audio_processing.STFT(n_fft, hop, n_fft).cuda()
    A = torch.from_numpy(start_angles(M.shape, 2)).cuda()
    Md = torch.from_numpy(Mn).cuda()
    fam = "r8" if st.fast_path() else "pow2"
    n_iters = 5
    calls = count_calls(monkeypatch, ALL_LAUNCHES)
    y = audio.griffin_lim(Md, st, n_iters, momentum=0.99, n_frames=lens, angles=A)
    assert calls["ft_istft_%s_ragged" % fam] == n_iters + 1 and calls["ft_stft_%s_ragged_phase" % fam] == n_iters \
        and calls["ft_gl_momentum"] == n_iters and sum(calls.values()) == 1 + 3 * n_iters, calls
    assert y.shape == (3, hop * 40) and torch.isfinite(y).all()
    for b, n in enumerate(lens):
        own = hop * (n - 1)
        one = audio.griffin_lim(Md[b:b + 1, :, :n], st, n_iters, momentum=0.99, n_frames=[n], angles=A[b:b + 1, :, :n])
        assert torch.equal(y[b, :own], one[0]), b
        assert torch.all(y[b, own:] == 0), b
    # the full-length utterance is the dense loop from the same angles
    np.random.seed(2)
    dense = audio.griffin_lim(torch.from_numpy(M[:1]).cuda(), st, n_iters, momentum=0.99)
    np.random.seed(2)
    first = audio.griffin_lim(torch.from_numpy(M[:1]).cuda(), st, n_iters, momentum=0.99, n_frames=[41])
    assert torch.equal(dense, first)
    for k in calls:
        calls[k] = 0
    plain = audio_processing.griffin_lim_ragged(Md, lens, st, n_iters, angles=A)
    assert sum(calls.values()) == 1 + 2 * n_iters and calls["ft_gl_momentum"] == 0, calls
    assert torch.equal(plain, audio.griffin_lim(Md, st, n_iters, momentum=0.0, n_frames=lens, angles=A))
    assert torch.equal(audio.griffin_lim(Md, st, 1, momentum=0.99, n_frames=lens, angles=A),
                       audio_processing.griffin_lim_ragged(Md, lens, st, 1, angles=A))
    assert not torch.equal(plain, y)


def test_griffin_lim_momentum_pow2_against_float64():
    """n_fft 512, hop 128 on the power-of-two kernels, 8 iterations: the same bound as at 1024."""
    M = _magnitudes((3, 4), 512, 128, 41)
    st = audio_processing.STFT(512, 128, 512).cuda()
    assert st.pow2_path()
    y = _gl(M, st, 8, momentum=0.99).cpu().double().numpy()
    y64 = R.fast_griffin_lim64(M, start_angles(M.shape, 0), 8, 512, 128, 512, ALPHA32)
    sc, sc64 = R.spectral_convergence(y, M, 512, 128, 512), R.spectral_convergence(y64, M, 512, 128, 512)
    print("fast Griffin-Lim 512 / 128, n_iters 8: spectral convergence %.5f (float64 %.5f), deviation %.3e" % (sc, sc64, abs(sc / sc64 - 1)))
    assert abs(sc / sc64 - 1) <= GL_DEV


# ---- mel -> waveform ------------------------------------------------------------------------------------------------------------
RT_DEV = 0.05          # |err(device) / err(float64 pipeline) - 1|: the existing round trip's bound (test_mel_round_trip)


def test_round_trip_with_nnls_and_momentum():
    """synth audio -> mel_spectrogram -> mel_to_audio -> mel_spectrogram at 1024 / 256, 80 bands, T 120, 30 iterations: NNLS +
    momentum ends closer to the mel than the defaults, and agrees with the float64 pipeline (nnls64 + fast_griffin_lim64).
    Measured on the MI355X: 0.2322 with the defaults, 0.1014 with NNLS + momentum, float64 pipeline 0.1015: a deviation of
    1.9e-5, so the existing round trip's bound of 5 % stays."""
    from oracle import synth
    tst = tacotron_stft("1024")
    y = synth.make_audio(256 * 120, seed=3)[None].cuda()
    mel = tst.mel_spectrogram(y)
    W = tst.mel_basis.cpu().numpy()
    mel_np = mel.cpu().double().numpy()

    def logmel_err(audio):
        return float(np.abs(tst.mel_spectrogram(audio).cpu().double().numpy() - mel_np).mean())

    np.random.seed(0)
    plain = logmel_err(tst.mel_to_audio(mel, n_iters=30))
    np.random.seed(0)
    audio = tst.mel_to_audio(mel, n_iters=30, momentum=0.99, inversion="nnls")
    assert audio.shape == (1, 256 * 120) and torch.isfinite(audio).all()
    fast = logmel_err(audio)
    s = np.exp(mel_np[0]).astype(np.float32)
    M64 = R.nnls64(W, s, R.pinv_relu(W, s).astype(np.float32), 100)[None]
    y64 = R.fast_griffin_lim64(M64, start_angles(M64.shape, 0), 30, 1024, 256, 1024, ALPHA32)
    m64 = np.log(np.maximum(np.einsum("mk,bkt->bmt", W.astype(np.float64), np.abs(stft64(y64, 1024, 256, 1024))), 1e-5))
    fast64 = float(np.abs(m64 - mel_np).mean())
    print("log-mel mean |error|: defaults %.4f, NNLS + momentum %.4f (float64 pipeline %.4f, deviation %.3e)"
          % (plain, fast, fast64, abs(fast / fast64 - 1)))
    assert fast < plain
    assert abs(fast / fast64 - 1) <= RT_DEV


def test_flowtron_infer_to_audio_with_nnls_and_momentum():
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
    with torch.no_grad():
        mel, _, lens = m.infer(residual, b["speaker_ids"][:2].cuda(), b["text"][:2, :9].cuda(), gate_threshold=1.0,
                               in_lens=in_lens, out_lens=out_lens, return_lengths=True)
    assert lens.tolist() == out_lens and mel.shape == (2, 80, 30)
    tst = tacotron_stft("1024")
    A = torch.from_numpy(start_angles((2, 513, 30), 41)).cuda()
    y = tst.mel_to_audio(mel, 4, momentum=0.99, inversion="nnls", lengths=lens, angles=A)
    assert y.shape == (2, 256 * 29) and torch.isfinite(y).all()
    for u, n in enumerate(out_lens):
        own = 256 * (n - 1)
        one = tst.mel_to_audio(mel[u:u + 1, :, :n], 4, momentum=0.99, inversion="nnls", lengths=[n], angles=A[u:u + 1, :, :n])
        assert torch.equal(y[u, :own], one[0]), u
        assert torch.all(y[u, own:] == 0), u
        assert y[u, :own].abs().max() > 0
    assert not torch.equal(y, tst.mel_to_audio_ragged(mel, lens, 4, angles=A))
