"""NNLS mel inversion and fast Griffin-Lim without a GPU: what the host restatements of tests/vocode_ref.py (the yardsticks of
tests/test_gpu_vocode_quality.py) are themselves worth, and the refusals of flowtron_amd.audio and of the C entries of
csrc/vocode.hip before anything reaches the device."""
import numpy as np
import pytest
import torch

import vocode_ref as R
from flowtron_amd import audio
from stft_ref64 import griffin_lim64, start_angles, stft64

EPS32 = float(np.finfo(np.float32).eps)
U = 2.0 ** -24                                    # unit roundoff of float32
T = 24
BANKS = {                                         # name -> (sampling rate, n_fft, hop, bands, fmax)
    "1024": (22050, 1024, 256, 80, 8000.0),
    "256": (16000, 256, 64, 40, None),
    "2048": (24000, 2048, 512, 100, None),
}
KINDS = ("representable", "perturbed", "uniform")
N_ITERS = 100
_CASES = {}


def case(bank, kind):
    """(W, s, pinv + ReLU estimate as the device forms it: float32, and the float32 iterates), computed once."""
    key = (bank, kind)
    if key not in _CASES:
        from oracle import synth
        sr, n_fft, hop, n_mel, fmax = BANKS[bank]
        W = audio.slaney_mel_filterbank(sr, n_fft, n_mel, 0.0, fmax)
        y = synth.make_audio(hop * (T - 1), seed=3)[None].double().numpy()
        s = W.astype(np.float64) @ np.abs(stft64(y, n_fft, hop, n_fft))[0]
        rs = np.random.RandomState(7)
        if kind == "perturbed":
            s = s * np.exp(0.3 * rs.standard_normal(s.shape))
        elif kind == "uniform":
            s = np.exp(rs.uniform(-8, 2, s.shape))
        s = s.astype(np.float32)
        m0 = R.pinv_relu(W, s).astype(np.float32)
        _CASES[key] = (W, s, m0, R.nnls32(W, s, m0, N_ITERS, history=True))
    return _CASES[key]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("bank", list(BANKS))
def test_every_frame_ends_below_pinv_relu(bank, kind):
    """Every frame in which the ReLU clipped something ends strictly lower.  Where the pseudo-inverse has no negative bin
    (the reflect-padded first frame of the 129-bin filterbank, and its last one at this length) pinv + ReLU already
    reproduces the mel to float32 rounding (relative residual 1e-8) and nothing can end lower: there the two must tie to
    the precision of the format, 8 eps32 ||s|| (the mel and every m[k] are float32 numbers, half an eps each; measured
    here 7e-8 ||s||).  Such frames are 2 of 24 at most."""
    W, s, m0, hist = case(bank, kind)
    norm = np.linalg.norm(s.astype(np.float64), axis=0)
    before, after = R.residual(W, m0, s), R.residual(W, hist[-1], s)
    clipped = ((np.linalg.pinv(W.astype(np.float64)) @ s.astype(np.float64)) < 0).any(axis=0)
    print("%s %s: relative residual %.4f .. %.4f -> %.4f .. %.4f; %d frames unclipped, there %.1e -> %.1e" % (
        (bank, kind) + tuple(f(v / norm) for v in (before, after) for f in (np.min, np.max))
        + ((~clipped).sum(), (before / norm)[~clipped].max(initial=0), (after / norm)[~clipped].max(initial=0))))
    assert hist[-1].dtype == np.float32 and (hist[-1] >= 0).all()
    assert (after < before)[clipped].all()
    assert (~clipped).sum() <= 2
    assert (after <= 8 * EPS32 * norm)[~clipped].all()


@pytest.mark.parametrize("bank", list(BANKS))
def test_gain_on_representable_mels(bank):
    W, s, m0, hist = case(bank, "representable")
    norm = np.linalg.norm(s, axis=0)
    before, after = (R.residual(W, m0, s) / norm).max(), (R.residual(W, hist[-1], s) / norm).max()
    print("%s: worst frame %.4f -> %.4f (ratio %.3f)" % (bank, before, after, after / before))
    assert after < 0.2 * before


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("bank", list(BANKS))
def test_objective_never_rises(bank, kind):
    W, s, m0, hist = case(bank, kind)
    obj = np.stack([R.residual(W, m, s) ** 2 for m in hist])
    slack = 64 * EPS32 * np.linalg.norm(s.astype(np.float64), axis=0) ** 2
    assert (obj[1:] <= obj[:-1] + slack[None, :]).all(), float((obj[1:] - obj[:-1] - slack[None, :]).max())


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("bank", list(BANKS))
def test_float32_against_float64(bank, kind):
    """The bound.  One update of m[k] in float32 carries the roundings of a band sum of at most L bins (L products, L adds),
    of d (two products, one add), of q (the same, once) and of the product and the quotient of the update: a relative error
    of at most (2 L + 8) u, u = 2^-24.  In the logarithms the update is x <- x + log q - log d(e^x) with the Jacobian I - P,
    P = D_d^-1 W'W D_m: P is row-stochastic (d is linear in m) and similar to the symmetric positive semi-definite
    E^1/2 W'W E^1/2, E = D_m D_d^-1, so its eigenvalues lie in [0, 1], and so do those of I - P: to first order an
    iteration does not amplify the difference between the two precisions, it only adds its own roundings.  After n
    iterations that leaves n (2 L + 8) u per frame in the relative 2-norm, taken with a factor 4 for the change of norm
    between iterations: ||m32 - m64|| <= 4 n (2 L + 8) u ||m64||."""
    W, s, m0, hist = case(bank, kind)
    m64 = R.nnls64(W, s, m0, N_ITERS)
    assert m64.dtype == np.float64
    L = int(np.diff(R.tables(W)[1]).max())
    bound = 4 * N_ITERS * (2 * L + 8) * U
    rel = np.linalg.norm(hist[-1] - m64, axis=0) / np.linalg.norm(m64, axis=0)
    print("%s %s: ||m32 - m64|| / ||m64|| <= %.2e (bound %.2e, longest band %d bins)" % (bank, kind, rel.max(), bound, L))
    assert rel.max() <= bound


def test_zero_iterations_return_the_start_and_a_silent_frame_stays_silent():
    W, s, m0, _ = case("1024", "representable")
    s, m0 = s.copy(), m0.copy()
    s[:, 3], m0[:, 3] = 0, 0
    start = R.nnls32(W, s, m0, 0)
    covered = W.sum(axis=0) > 0
    assert (start[~covered] == 0).all() and covered.sum() == 513 - 142
    assert (start[:, 3] == 0).all() and (R.nnls32(W, s, m0, 5)[:, 3] == 0).all()
    live = np.delete(np.arange(T), 3)
    assert (start[np.ix_(covered, live)] > 0).all()
    assert (start[covered] >= m0[covered]).all()


def _gl_inputs(seed):
    from oracle import synth
    y = synth.make_audio(256 * 40, seed=seed)[None].double().numpy()
    return np.abs(stft64(y, 1024, 256, 1024)).astype(np.float32)


@pytest.mark.parametrize("seed", [3, 4])
def test_fast_beats_plain(seed):
    M = _gl_inputs(seed)
    a = start_angles(M.shape, 0)
    plain = R.spectral_convergence(griffin_lim64(M, a, 30, 1024, 256, 1024), M, 1024, 256, 1024)
    fast = R.spectral_convergence(R.fast_griffin_lim64(M, a, 30, 1024, 256, 1024, 0.99), M, 1024, 256, 1024)
    print("seed %d: spectral convergence plain %.4f, fast %.4f (ratio %.3f)" % (seed, plain, fast, fast / plain))
    assert fast <= 0.8 * plain


def test_first_iteration_is_the_plain_one():
    M = _gl_inputs(3)
    a = start_angles(M.shape, 0)
    for n in (0, 1):
        assert np.array_equal(R.fast_griffin_lim64(M, a, n, 1024, 256, 1024, 0.99), griffin_lim64(M, a, n, 1024, 256, 1024))
    assert not np.array_equal(R.fast_griffin_lim64(M, a, 2, 1024, 256, 1024, 0.99), griffin_lim64(M, a, 2, 1024, 256, 1024))


def test_refusals_are_raised_without_a_device():
    tst = audio.TacotronSTFT(1024, 256, 1024, 80, 22050, 0.0, 8000.0)
    mel = torch.zeros(2, 80, 8)
    mag = torch.ones(1, 513, 8)
    for bad in ("NNLS", "lstsq", None, 1):
        with pytest.raises(ValueError, match="method"):
            tst.mel_to_magnitude(mel, method=bad)
        with pytest.raises(ValueError, match="method"):
            tst.mel_to_magnitude(mel, method=bad, lengths=[8, 4])
        with pytest.raises(ValueError, match="method"):
            tst.mel_to_audio(mel, inversion=bad)
        with pytest.raises(ValueError, match="method"):
            tst.mel_to_audio(mel, inversion=bad, lengths=[8, 4])
    for bad in (-1, 2.5, True, None):
        with pytest.raises(ValueError, match="iterations"):
            tst.mel_to_magnitude(mel, method="nnls", n_iters=bad)
    for bad in (1.0, -0.1, 1.5, float("nan"), None, "0.99", True):
        with pytest.raises(ValueError, match="momentum"):
            audio.griffin_lim(mag, tst.stft_fn, 2, momentum=bad)
        with pytest.raises(ValueError, match="momentum"):
            audio.griffin_lim(mag, tst.stft_fn, 2, momentum=bad, n_frames=[8])
        with pytest.raises(ValueError, match="momentum"):
            tst.mel_to_audio(mel, momentum=bad)
        with pytest.raises(ValueError, match="momentum"):
            tst.mel_to_audio(mel, momentum=bad, lengths=[8, 4])
    for kw in (dict(method="nnls"), dict(method="pinv"), dict()):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            tst.mel_to_magnitude(mel, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        audio.griffin_lim(mag, tst.stft_fn, 2, momentum=0.99)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        audio.griffin_lim(mag, tst.stft_fn, 2, momentum=0.99, n_frames=[8])
    with pytest.raises(ValueError, match="angles"):                       # starting angles belong to the ragged loop
        audio.griffin_lim(mag, tst.stft_fn, 2, angles=torch.zeros(1, 513, 8))
    with pytest.raises(ValueError, match="angles"):
        tst.mel_to_audio(mel, angles=torch.zeros(2, 513, 8))


def test_per_bin_table():
    W = audio.slaney_mel_filterbank(22050, 1024, 80, 0.0, 8000.0)
    bin0, ptr, w = audio.filterbank_csr(W)
    band, weight = audio.filterbank_bin_table(bin0, ptr, w, 513)
    rb0, rptr, rw, rband, rweight = R.tables(W)
    assert np.array_equal(band, rband) and np.array_equal(weight, rweight) and band.dtype == np.int32 and weight.dtype == np.float32
    assert int((band[:, 0] < 0).sum()) == 142 and band[0, 0] == -1
    dense = np.zeros_like(W)
    for k in range(513):
        for c in range(2):
            if band[k, c] >= 0:
                dense[band[k, c], k] = weight[k, c]
    assert np.array_equal(dense, W)
    both = band[:, 1] >= 0
    assert (band[both, 0] < band[both, 1]).all()
    three = np.zeros((3, 9), np.float32)
    three[0, 1:5], three[1, 2:6], three[2, 4:8] = 1, 1, 1                # bin 4 lies in all three
    with pytest.raises(NotImplementedError, match="bin 4 .* more than two bands"):
        audio.filterbank_bin_table(*audio.filterbank_csr(three), 9)
    two = three.copy()
    two[0, 4] = 0
    assert audio.filterbank_bin_table(*audio.filterbank_csr(two), 9)[0][4].tolist() == [1, 2]


def test_c_abi_refuses_bad_arguments_before_the_device():
    """FT_EINVAL / FT_EUNSUPPORTED from the entry points themselves, with host memory standing in for the buffers: nothing may
    be launched"""
    import ctypes as C
    from flowtron_amd import _lib as L
    lib = L.lib()
    f = (C.c_float * 64)()
    i = (C.c_int32 * 64)()
    pf, pi = C.addressof(f), C.addressof(i)
    ok = dict(s=pf, m0=pf, m=pf, nf=pi, bin0=pi, ptr=pi, w=pf, band=pi, bw=pf, B=1, n_mel=2, n_fft=256, T=1, nnz=4, n_iters=1)

    def nnls(**kw):
        a = dict(ok, **kw)
        return lib.ft_mel_nnls(a["s"], a["m0"], a["m"], a["nf"], a["bin0"], a["ptr"], a["w"], a["band"], a["bw"], a["B"], a["n_mel"],
                               a["n_fft"], a["T"], a["nnz"], a["n_iters"], None)
    for kw in (dict(s=None), dict(m0=None), dict(m=None), dict(bin0=None), dict(ptr=None), dict(w=None), dict(band=None), dict(bw=None),
               dict(B=0), dict(B=65536), dict(n_mel=0), dict(T=0), dict(nnz=0), dict(n_iters=-1)):
        assert nnls(**kw) == -1, kw
        assert b"ft_mel_nnls" in lib.ft_last_error()
    for kw in (dict(n_mel=129), dict(n_fft=1000), dict(n_fft=800), dict(n_fft=128), dict(n_fft=8192), dict(n_fft=0), dict(nnz=1 << 20)):
        assert nnls(**kw) == -3, kw
        assert b"ft_mel_nnls" in lib.ft_last_error()

    okm = dict(mag=pf, ph=pf, re=pf, im=pf, nf=pi, B=1, nb=3, T=4, alpha=0.99, first=0)

    def step(**kw):
        a = dict(okm, **kw)
        return lib.ft_gl_momentum(a["mag"], a["ph"], a["re"], a["im"], a["nf"], a["B"], a["nb"], a["T"], a["alpha"], a["first"], None)
    for kw in (dict(mag=None), dict(ph=None), dict(re=None), dict(im=None), dict(B=0), dict(nb=0), dict(T=0), dict(B=65536),
               dict(nb=1 << 16, T=1 << 15), dict(alpha=1.0), dict(alpha=-0.5), dict(alpha=float("nan"))):
        assert step(**kw) == -1, kw
        assert b"ft_gl_momentum" in lib.ft_last_error()
