"""The single-pass phase start (SPSI, ft_spsi_phase) without a GPU: what the rule of include/flowtron_hip.h is worth as a start
of Griffin-Lim (the float64 replay of tests/spsi_ref.py under the yardsticks of tests/stft_ref64.py and tests/vocode_ref.py), the
rule's corners on the float32 replay, and the refusals of flowtron_amd.audio and of the C entry before anything reaches the
device."""
import numpy as np
import pytest
import torch

import spsi_ref as S
import vocode_ref as R
from flowtron_amd import audio
from stft_ref64 import griffin_lim64, istft64, start_angles, stft64

N_FFT, HOP, SR = 1024, 256, 22050
K = N_FFT // 2 + 1


def voice(seed, n=HOP * 40):
    """A harmonic signal with vibrato, tremolo and a little noise: what a voiced stretch of speech looks like to an STFT."""
    rs = np.random.RandomState(seed)
    t = np.arange(n) / SR
    f0 = (130.0 + 25.0 * seed) * (1.0 + 0.02 * np.sin(2 * np.pi * 5.5 * t))
    ph = 2 * np.pi * np.cumsum(f0) / SR
    y = sum(np.sin(h * ph + rs.uniform(0, 2 * np.pi)) / h for h in range(1, 25))
    y = y * (1.0 + 0.3 * np.sin(2 * np.pi * 3.0 * t)) + 0.01 * rs.standard_normal(n)
    return 0.3 * y / np.abs(y).max()


_SIGNALS = {}


def magnitudes(name):
    """[1, 513, 41] float32 |STFT| of the named signal, once."""
    if name not in _SIGNALS:
        from oracle import synth
        kind, seed = name.split("-")
        y = synth.make_audio(HOP * 40, seed=int(seed)).double().numpy() if kind == "synth" else voice(int(seed))
        _SIGNALS[name] = np.abs(stft64(y[None], N_FFT, HOP, N_FFT)).astype(np.float32)
    return _SIGNALS[name]


def sc(y, M):
    return R.spectral_convergence(y, M, N_FFT, HOP, N_FFT)


# (b)'s ratio r as measured with the rule of the header on the CPU (printed by the test), asserted with a quarter above it.
R_MEASURED = {"synth-3": 0.503, "synth-4": 0.471, "voice-1": 0.302}


@pytest.mark.parametrize("name", list(R_MEASURED))
def test_spsi_start_beats_the_random_start(name):
    """(a) zero iterations from SPSI end below 30 plain iterations from the random start; (b) 10 plain iterations from SPSI end
    at most r x the random start's 30, r = 1.25 x the measured ratio (the computation is deterministic: the margin is for BLAS
    and FFT differences between machines)."""
    M = magnitudes(name)
    spsi = S.spsi64(M, N_FFT, HOP)
    rand = start_angles(M.shape, 0)
    assert spsi.dtype == np.float64 and spsi.shape == M.shape
    spsi0 = sc(istft64(M, spsi, N_FFT, HOP, N_FFT)[0], M)
    spsi10 = sc(griffin_lim64(M, spsi, 10, N_FFT, HOP, N_FFT), M)
    rand0 = sc(istft64(M, rand, N_FFT, HOP, N_FFT)[0], M)
    rand30 = sc(griffin_lim64(M, rand, 30, N_FFT, HOP, N_FFT), M)
    spsi_fast = sc(R.fast_griffin_lim64(M, spsi, 30, N_FFT, HOP, N_FFT, 0.99), M)
    rand_fast = sc(R.fast_griffin_lim64(M, rand, 30, N_FFT, HOP, N_FFT, 0.99), M)
    print("%s: spectral convergence SPSI 0 iters %.4f, 10 plain %.4f, 30 fast %.4f; random 0 iters %.4f, 30 plain %.4f, 30 fast %.4f; "
          "r = %.4f" % (name, spsi0, spsi10, spsi_fast, rand0, rand30, rand_fast, spsi10 / rand30))
    assert spsi0 < rand30
    assert spsi10 <= 1.25 * R_MEASURED[name] * rand30


@pytest.mark.parametrize("name", ["synth-3", "voice-1"])
def test_spsi_start_through_the_mel(name):
    """80 bands, fmax 8000, NNLS inversion (100 iterations): the round trip's mean |log-mel error| at zero iterations from SPSI
    is below half of the random start's."""
    W = audio.slaney_mel_filterbank(SR, N_FFT, 80, 0.0, 8000.0)
    s = (W.astype(np.float64) @ magnitudes(name)[0].astype(np.float64)).astype(np.float32)
    M = R.nnls64(W, s, R.pinv_relu(W, s).astype(np.float32), 100)[None]
    want = np.log(np.maximum(s.astype(np.float64), 1e-5))

    def err(angles):
        y = istft64(M, angles, N_FFT, HOP, N_FFT)[0]
        got = np.log(np.maximum(W.astype(np.float64) @ np.abs(stft64(y, N_FFT, HOP, N_FFT))[0], 1e-5))
        return float(np.abs(got - want).mean())
    e_spsi, e_rand = err(S.spsi64(M, N_FFT, HOP)), err(start_angles(M.shape, 0))
    print("%s: mean |log-mel error| at zero iterations: SPSI %.4f, random %.4f (ratio %.3f)" % (name, e_spsi, e_rand, e_spsi / e_rand))
    assert e_spsi < 0.5 * e_rand


# ---- the rule's corners, on the float32 replay -------------------------------------------------------------------------------
def walk_owner(m, j):
    """The owner of bin j by the header's words, one step at a time (spsi_ref.owners scans instead)."""
    Kk = len(m)

    def peak(q):
        return 1 <= q <= Kk - 2 and m[q] > m[q - 1] and m[q] > m[q + 1]
    if peak(j):
        return j
    if j < Kk - 1 and m[j] < m[j + 1]:
        q = j + 1
        while q < Kk - 1 and m[q] < m[q + 1]:
            q += 1
        return q if peak(q) else -1
    if j > 0 and m[j] < m[j - 1]:
        q = j - 1
        while q > 0 and m[q] < m[q - 1]:
            q -= 1
        return q if peak(q) else -1
    return -1


def frame(values):
    """One frame [K, 1] float32 with the given leading bins, the others 0."""
    m = np.zeros((K, 1), np.float32)
    m[:len(values), 0] = values
    return m


def test_owner_scan_is_the_walk():
    rs = np.random.RandomState(5)
    cases = [rs.rand(K), np.round(rs.rand(K) * 3), np.arange(K), np.arange(K)[::-1], np.zeros(K),
             np.abs(np.sin(np.arange(K) / 37.0)), np.repeat(rs.rand(K // 5 + 1), 5)[:K]]
    holes = np.abs(np.sin(np.arange(K) / 11.0))
    holes[[0, 100, 101, 300, K - 1]] = [np.nan, np.nan, np.inf, np.inf, np.nan]
    cases.append(holes)
    with np.errstate(invalid="ignore"):
        for m in cases:
            m = m.astype(np.float32)
            peak, owner = S.owners(m)
            assert owner.tolist() == [walk_owner(m, j) for j in range(K)]
            assert np.array_equal(np.nonzero(peak)[0], np.nonzero(owner == np.arange(K))[0])


def test_first_frame_and_lobe_alternation():
    """T = 1 is frame 0 from zeros: a symmetric peak at bin 8 (p = 0, hop * 8 mod n_fft = 0) stays at 0 turns and its lobe
    alternates by half a turn; one bin further the integer split gives 0.25 turns."""
    t = S.spsi32(frame([0, 0, 0, 0, 0, 1, 3, 5, 9, 5, 3, 1]), N_FFT, HOP, turns=True)[:, 0]
    assert t.dtype == np.float32
    assert t[5:12].tolist() == [0.5, 0.0, 0.5, 0.0, 0.5, 0.0, 0.5]          # bin 8 and its slopes (rint(0.5) = 0: +0.5 stays)
    assert (t[:5] == 0).all() and (t[12:] == 0).all()
    t = S.spsi32(frame([0, 0, 0, 0, 0, 0, 1, 3, 5, 9, 5, 3, 1]), N_FFT, HOP, turns=True)[:, 0]
    assert t[9] == 0.25 and t[8] == -0.25 and t[10] == -0.25 and t[7] == 0.25      # 0.75 wraps to -0.25
    a = S.spsi32(frame([0, 0, 0, 0, 0, 0, 1, 3, 5, 9, 5, 3, 1]), N_FFT, HOP)[:, 0]
    assert a[9] == np.float32(6.2831855) * np.float32(0.25)
    # an asymmetric peak: p by the formula, in float32
    m = frame([0, 1, 4, 2])
    p = (np.float32(0.5) * (np.float32(1) - np.float32(2))) / ((np.float32(1) - np.float32(4)) + (np.float32(2) - np.float32(4)))
    inc = np.float32(512) / np.float32(1024) + (np.float32(256) / np.float32(1024)) * p
    assert S.spsi32(m, N_FFT, HOP, turns=True)[2, 0] == inc - np.rint(inc) and p == np.float32(0.1)


def test_silent_frame_plateau_ramp_and_trough():
    lobe = [0, 1, 4, 2, 0, 0, 3, 7, 3]
    M = np.concatenate([frame(lobe), frame([]), frame(lobe)], axis=1)
    t = S.spsi32(M, N_FFT, HOP, turns=True)
    assert np.array_equal(t[:, 1], t[:, 0]) and t[2, 0] != 0                   # an all-zero frame carries the previous phase
    assert t[2, 2] != t[2, 0]                                                 # ... and the walk goes on behind it
    v = t[2, 0] + (np.float32(0.5) + np.float32(0.25) * np.float32(0.1))      # bin 2: hop * 2 mod n_fft = 512, p = 0.1
    assert t[2, 2] == v - np.rint(v)
    # a plateau keeps its phase: bins 2 and 3 tie, so neither is a peak and nothing on their slopes has an owner
    M = np.concatenate([frame(lobe), frame([0, 1, 4, 4, 1, 0, 3, 7, 3])], axis=1)
    t = S.spsi32(M, N_FFT, HOP, turns=True)
    assert np.array_equal(t[:5, 1], t[:5, 0]) and t[7, 1] != t[7, 0]
    # a ramp ascending to K - 1 has no owner (K - 1 is no peak), nor has one descending from bin 0
    ramp = np.arange(K, dtype=np.float32)[:, None]
    for r in (ramp, ramp[::-1]):
        assert (S.owners(r[:, 0])[1] == -1).all()
        assert np.array_equal(S.spsi32(np.concatenate([frame(lobe), r], axis=1), N_FFT, HOP, turns=True)[:, 1], t[:, 0])
    # a trough goes to the peak on its right; the bin of a trough whose right walk ends on a plateau has none
    assert S.owners(np.array([0, 5, 1, 6, 0], np.float32))[1].tolist() == [1, 1, 3, 3, 3]
    assert S.owners(np.array([0, 5, 1, 6, 6, 0], np.float32))[1].tolist() == [1, 1, -1, -1, -1, -1]


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_a_nan_or_inf_cell_stays_local(bad):
    rs = np.random.RandomState(6)
    M = rs.rand(K, 6).astype(np.float32)
    clean = S.spsi32(M, N_FFT, HOP, turns=True)
    M2 = M.copy()
    M2[200, 2] = bad
    with np.errstate(invalid="ignore"):
        got = S.spsi32(M2, N_FFT, HOP, turns=True)
        peak, owner = S.owners(M2[:, 2])
    assert np.isfinite(got).all()
    assert np.array_equal(got[:, :2], clean[:, :2])
    if np.isnan(bad):
        assert not peak[199:202].any() and owner[200] == -1                   # every comparison with it is false
    else:
        assert peak[200] and not peak[199] and not peak[201]
        assert got[200, 2] == got[200, 1]                                     # den = -inf: p = 0, and hop * 200 mod n_fft = 0
    # owners change only where a walk meets the cell: between the stops on either side of it
    _, owner0 = S.owners(M[:, 2])
    changed = np.nonzero(owner != owner0)[0]
    assert len(changed) and changed.min() >= 200 - 12 and changed.max() <= 200 + 12      # uniform noise: no slope is that long
    assert (np.abs(got) <= 0.5).all()


def test_angles_stay_inside_pi():
    rs = np.random.RandomState(7)
    M = np.concatenate([rs.rand(K, 40), magnitudes("synth-3")[0]], axis=1).astype(np.float32)
    a = S.spsi32(M, N_FFT, HOP)
    assert a.dtype == np.float32 and np.abs(a).max() <= np.pi * (1 + 2.0 ** -23) and np.abs(a).max() > 3.0
    t = S.spsi32(M, N_FFT, HOP, turns=True)
    assert np.array_equal(a, np.float32(6.2831855) * t)
    # ragged: zeros at and behind every length, the rest as alone
    B = np.stack([M[:, :9], M[:, 9:18], M[:, 18:27]])
    r = S.spsi32(B, N_FFT, HOP, n_frames=[9, 4, 0])
    assert (r[1, :, 4:] == 0).all() and (r[2] == 0).all() and np.array_equal(r[1, :, :4], S.spsi32(B[1, :, :4], N_FFT, HOP))


def test_pure_tone_advance():
    """The peak bin's advance per frame against hop f / sr mod 1.  The parabola through three samples of a Hann main lobe
    under-estimates a small offset d by about a quarter of it, 0.25 d of a bin or (hop / n_fft) 0.25 d = d / 16 turns: within
    1e-3 turns of the truth only at |d| < 0.016 bins.  The tone sits at d = 0.012 bins, where a rule without interpolation misses
    by 0.25 d = 3e-3 turns and one with a wrong integer split by a quarter turn or more (hop k mod n_fft steps by 256 / 1024).
    At other offsets the replay is held to the parabola itself, evaluated here in float64 from the magnitudes."""
    n = HOP * 40
    for d, k in ((0.012, 46), (0.012, 45), (-0.012, 47)):
        f = (k + d) * SR / N_FFT
        y = 0.5 * np.sin(2 * np.pi * f * np.arange(n) / SR)[None]
        M = np.abs(stft64(y, N_FFT, HOP, N_FFT))[0].astype(np.float32)
        t = S.spsi32(M, N_FFT, HOP, turns=True).astype(np.float64)
        assert int(M[:, 20].argmax()) == k
        adv = np.diff(t[k, 8:32])
        err = (adv - (HOP * f / SR) % 1 + 0.5) % 1 - 0.5
        print("tone at bin %d%+.3f: advance %.5f turns a frame, wanted %.5f, worst error %.2e" % (k, d, adv[0] % 1, (HOP * f / SR) % 1, np.abs(err).max()))
        assert np.abs(err).max() <= 1e-3
    for d in (0.1, 0.25, 0.4, -0.3):
        k = 57
        f = (k + d) * SR / N_FFT
        y = 0.5 * np.sin(2 * np.pi * f * np.arange(n) / SR)[None]
        M = np.abs(stft64(y, N_FFT, HOP, N_FFT))[0].astype(np.float32)
        t = S.spsi32(M, N_FFT, HOP, turns=True).astype(np.float64)
        a, b, c = (M[k + i, 9:32].astype(np.float64) for i in (-1, 0, 1))
        p = 0.5 * (a - c) / (a - 2 * b + c)
        assert (np.sign(p) == np.sign(d)).all() and (np.abs(p) < abs(d)).all() and (np.abs(p) > 0.5 * abs(d)).all()
        want = ((HOP * k) % N_FFT) / N_FFT + HOP / N_FFT * p
        err = (np.diff(t[k, 8:32]) - want + 0.5) % 1 - 0.5
        assert np.abs(err).max() <= 1e-5                             # float32 roundings of p and of the accumulator


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_are_raised_without_a_device():
    import audio_processing
    assert audio_processing.spsi_phase is audio.spsi_phase
    tst = audio.TacotronSTFT(1024, 256, 1024, 80, 22050, 0.0, 8000.0)
    st = tst.stft_fn
    mag = torch.ones(2, 513, 8)
    mel = torch.zeros(2, 80, 8)
    for bad in (mag.double(), mag.half(), mag.long()):
        with pytest.raises(ValueError, match="float32"):
            audio.spsi_phase(bad, st)
    for bad in (torch.ones(513), torch.ones(1, 2, 513, 8), torch.ones(2, 512, 8), torch.ones(8, 513), torch.ones(2, 513, 0), None):
        with pytest.raises(ValueError, match="shape"):
            audio.spsi_phase(bad, st)
    for bad in ([8], [8, 9], [8, -1], [8, 2.0], [True, 8], torch.tensor([8.0, 8.0]), 8):
        with pytest.raises(ValueError, match="n_frames"):
            audio.spsi_phase(mag, st, n_frames=bad)
    for kw in (dict(), dict(n_frames=[8, 0]), dict(n_frames=torch.tensor([0, 8]))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            audio.spsi_phase(mag, st, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        audio.spsi_phase(mag[0], st)
    with pytest.raises(NotImplementedError, match="filter_length"):
        audio.spsi_phase(torch.ones(1, 401, 8), audio.STFT(800, 200, 800))
    for bad in ("SPSI", "pghi", "", None, 0, True):
        with pytest.raises(ValueError, match="phase_init .*random.*spsi"):
            audio.griffin_lim(mag, st, 2, phase_init=bad)
        with pytest.raises(ValueError, match="phase_init .*random.*spsi"):
            audio.griffin_lim(mag, st, 2, n_frames=[8, 8], phase_init=bad)
        with pytest.raises(ValueError, match="phase_init .*random.*spsi"):
            tst.mel_to_audio(mel, phase_init=bad)
        with pytest.raises(ValueError, match="phase_init .*random.*spsi"):
            tst.mel_to_audio(mel, lengths=[8, 4], phase_init=bad)
    A = torch.zeros(2, 513, 8)
    with pytest.raises(ValueError, match="angles"):
        audio.griffin_lim(mag, st, 2, n_frames=[8, 8], angles=A, phase_init="spsi")
    with pytest.raises(ValueError, match="angles"):
        audio.griffin_lim(mag, st, 2, angles=A, phase_init="spsi")
    with pytest.raises(ValueError, match="angles"):
        tst.mel_to_audio(mel, lengths=[8, 4], angles=A, phase_init="spsi")
    for kw in (dict(), dict(n_frames=[8, 8]), dict(momentum=0.99)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            audio.griffin_lim(mag, st, 0, phase_init="spsi", **kw)
    for kw in (dict(), dict(lengths=[8, 4]), dict(inversion="nnls")):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            tst.mel_to_audio(mel, 0, phase_init="spsi", **kw)


def test_c_abi_refuses_bad_arguments_before_the_device():
    """FT_EINVAL / FT_EUNSUPPORTED from the entry point itself, with host memory standing in for the buffers: nothing may be
    launched."""
    import ctypes as C
    from flowtron_amd import _lib as L
    lib = L.lib()
    assert lib.ft_abi_version() == 15
    f = (C.c_float * 64)()
    i = (C.c_int32 * 64)()
    pf, pi = C.addressof(f), C.addressof(i)
    ok = dict(mag=pf, ph=pf, nf=pi, B=1, n_fft=256, hop=64, T=1)

    def spsi(**kw):
        a = dict(ok, **kw)
        return lib.ft_spsi_phase(a["mag"], a["ph"], a["nf"], a["B"], a["n_fft"], a["hop"], a["T"], None)
    for kw in (dict(mag=None), dict(ph=None), dict(B=0), dict(B=-1), dict(T=0), dict(hop=0), dict(hop=257), dict(hop=-4),
               dict(B=65536), dict(n_fft=4096, hop=1024, T=1 << 21), dict(n_fft=1024, hop=256, T=0x7fffffff)):
        assert spsi(**kw) == -1, kw
        assert b"ft_spsi_phase" in lib.ft_last_error()
    for kw in (dict(n_fft=1000, hop=100), dict(n_fft=800, hop=200), dict(n_fft=128, hop=32), dict(n_fft=8192, hop=64),
               dict(n_fft=768, hop=64)):
        assert spsi(**kw) == -3, kw
        assert b"ft_spsi_phase" in lib.ft_last_error()
