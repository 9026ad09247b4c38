"""The STFT and mel front end that produces every training mel (stft_r8_k, csrc/stft_r8.hip: n_fft 1024, hop <= 256), the CSR
filterbank text of the power-of-two kernels (csrc/stft_pow2.hip) and the fallback stft_mel_k (csrc/stft.hip) against the float64
restatement in tests/stft_ref64.py, element by element and frame by frame.

Bounds (none tuned on the code under test): per-frame magnitude relative L2 <= MAG_BOUND = 1e-6 and phase <= PHASE_BOUND = 1e-4
where |X| > 1e-3 max|X| are the project's numbers for an fp32 FFT (test_gpu_stft_pow2.py); a log-mel element must lie in the
interval stft_ref64.logmel_judge derives from them (ratio <= 1).  test_stft_ref64_cpu.py shows on these same inputs
(tests/stft_front_end_cases.py) that an honest fp32 computation sits at ratio <= 0.14, that every wrong reference sits >= 370
bounds away, and that the phase mask keeps >= 81 % of every frame.

Which case enters which branch of stft_r8_k:
  * filterbank read from global memory (nnz = 2 127 > BWMAX)       C WIDE_n1024_*  (and the pow2 copy: C WIDE_n512_*)
  * empty band, bn == 0 -> logf(1e-5f)                             C, band 125 of WIDE and NARROW
  * bins 0 and 512 in a mel sum (512: lane 0's r = 8 trip)         C, bands 126 and 127
  * band counts 1 | 64 | 65 | 128 (a lane owns bands l, l + 64)    B m1, m64, m65, m128 (and C: 128)
  * widths 1, 7, 8, 9, 16, 17 around the eight-at-a-time loop      C NARROW_* (clamped tail j = n - 1), WIDE: 17 = 2 x 8 + 1
  * odd hops (a frame's float2 reads only 4-byte aligned)           A h1, h255; B h255; C h255
  * 15 | 16 | 16 | 17 frames (workgroup edge), 4 | 5 (wave edge)     A N3839 .. N4096, N768, N1024; shortest signal A N513
  * ragged tail, NaN behind every length, mag = NULL                D
  * n_samples <= n_fft / 2 (single fold, zeros beyond)              D short utterance
stft_mel_k: E (> 128 bands, n_fft 64 / 128 / 4096, hop > win_length, 9 and 10 frames of its 8 per workgroup, N = n_fft/2 + 1).

Worst values measured on an MI355X, 2026-10-21 (pytest -s prints every one; profiles/stft_front_end_f64_pytest_gpu.log):

  section                                        worst measured                          bound
  A  |X| per-frame relative L2                   1.21e-7                                 1e-6
  A  phase, masked bins                          4.87e-5                                 1e-4
  B  log-mel ratio (r8, Slaney)                  0.085 (silence: 0.27; 0.58 at floor)    1.0
  C  log-mel ratio (hand-made CSR)               0.20 (0.58 at the floor)                1.0
  D  ragged: |X| / phase / ratio                 1.19e-7 / 6.21e-5 / 0.070               as A, B
  E  log-mel ratio (ft_stft_mel)                 0.34                                    1.0
  F  smallest wrong-reference ratio              376 (symmetric hann, WIDE)              >= 4

An element at the floor measures the device's logf(1e-5f) alone: -11.512927, 1.64 ulp from log(1e-5f), ratio 0.58 of logf's
allowance (see the log_floor32 fixture).  No case failed against the kernels as they were; nothing in csrc/ changed.
"""
import numpy as np
import pytest
import torch

import audio_processing
import stft_front_end_cases as cases
from call_count import count_calls
from flowtron_amd import _lib as L
from stft_ref64 import (FLOOR, HANDMADE_EMPTY, MAG_BOUND, MUTATIONS, PHASE_BOUND, csr_dense64, frame_phase_err, frame_rel_l2,
                        handmade_csr, logmel_judge, stft64, stft64_single_fold)

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
STFT_ENTRIES = ["ft_stft_mel", "ft_stft_r8", "ft_stft_r8_ragged", "ft_stft_r8_ragged_phase", "ft_stft_pow2",
                "ft_stft_pow2_ragged", "ft_stft_pow2_ragged_phase"]
SENTINEL = 12345.0


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def judge_spectrum(what, mag, phase, X64):
    """Every frame of every batch row alone: magnitude relative L2 and masked phase.  Returns the two worst values."""
    e_mag = frame_rel_l2(mag.cpu().numpy(), np.abs(X64))
    e_ph = frame_phase_err(phase.cpu().numpy(), X64)
    print("%s: per-frame |X| rel L2 max %.2e (at frame %s), phase max %.2e (at frame %s)"
          % (what, e_mag.max(), np.unravel_index(e_mag.argmax(), e_mag.shape), e_ph.max(),
             np.unravel_index(e_ph.argmax(), e_ph.shape)))
    assert e_mag.max() <= MAG_BOUND, (what, e_mag.max())
    assert e_ph.max() <= PHASE_BOUND, (what, e_ph.max())
    return float(e_mag.max()), float(e_ph.max())


def judge_mel(what, mel, absX64, fb):
    r = logmel_judge(mel.cpu().numpy(), absX64, fb)
    assert np.isfinite(r).all(), what
    live = np.einsum("mk,bkt->bmt", fb, absX64) > FLOOR                   # elements at the floor measure logf(1e-5f) alone
    print("%s: log-mel ratio max %.3f (at %s), above the floor %.3f, %d elements at the floor"
          % (what, r.max(), np.unravel_index(r.argmax(), r.shape), r[live].max(), int((~live).sum())))
    assert r.max() <= 1.0, (what, r.max())
    return float(r.max())


@pytest.fixture(scope="module")
def log_floor32():
    """The one float32 the device's logf gives for 1e-5f, taken from the mel of an all-zero signal (every band sum is exactly
    0, so every element is logf(fmaxf(0, 1e-5f))): all elements must carry the same bits, and that value must lie within the
    allowance logmel_judge grants logf, 4 x 2^-24 |log|, of log(1e-5f).  The device's logf is not correctly rounded (measured
    -11.512927, 1.6 ulp below log(1e-5f) = -11.5129255), so "exactly the floor" is stated as: these bits, everywhere."""
    tst = audio_processing.TacotronSTFT(1024, 256, 1024, 80, 22050, 0.0, 8000.0).cuda()
    v = np.unique(tst.mel_spectrogram(torch.zeros(1, 4000, device="cuda")).cpu().numpy())
    true = np.log(np.float64(np.float32(1e-5)))
    print("logf(1e-5f) on the device: %r (float64: %.9f, %.2f ulp)" % (v, true, abs(float(v[0]) - true) / 2.0 ** -20))
    assert v.size == 1 and abs(float(v[0]) - true) <= 4 * U32 * abs(true)
    return v[0]


# ---- A: r8 transform ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop,win,B,N", cases.A_GRID, ids=cases.A_IDS)
def test_a_transform_every_frame(monkeypatch, hop, win, B, N):
    st = audio_processing.STFT(1024, hop, win).cuda()
    assert st.fast_path()
    y = cases.audio_a(hop, win, B, N)
    calls = count_calls(monkeypatch, STFT_ENTRIES)
    mag, phase = st.transform(dev(y))
    assert calls == dict({n: 0 for n in STFT_ENTRIES}, ft_stft_r8=1), calls
    assert mag.shape == (B, 513, N // hop + 1) and phase.shape == mag.shape
    judge_spectrum("A hop %d win %d B %d N %d (%d frames)" % (hop, win, B, N, N // hop + 1), mag, phase, stft64(y, 1024, hop, win))
    mag2, phase2 = st.transform(dev(y))
    assert torch.equal(mag, mag2) and torch.equal(phase, phase2)


# ---- B: r8 log-mel, Slaney ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def absx_b():
    """hop -> (y, |X| float64) of the B audio: one float64 spectrum per hop, shared by the six filterbanks and by F."""
    return {hop: (cases.audio_b(hop), np.abs(stft64(cases.audio_b(hop), 1024, hop, win))) for hop, win in cases.B_HOPS}


def mel_b(sr, n_mel, fmin, fmax, hop, win, y):
    tst = audio_processing.TacotronSTFT(1024, hop, win, n_mel, sr, fmin, fmax).cuda()
    assert tst.stft_fn.fast_path() and tst.ragged_path()
    return tst, tst.mel_spectrogram(dev(y))


@pytest.mark.parametrize("sr,n_mel,fmin,fmax,hop,win", cases.B_CASES, ids=cases.B_IDS)
def test_b_log_mel(monkeypatch, absx_b, sr, n_mel, fmin, fmax, hop, win):
    y, absX = absx_b[hop]
    calls = count_calls(monkeypatch, STFT_ENTRIES)
    tst, mel = mel_b(sr, n_mel, fmin, fmax, hop, win, y)
    assert calls == dict({n: 0 for n in STFT_ENTRIES}, ft_stft_r8=1), calls
    assert mel.shape == (y.shape[0], n_mel, y.shape[1] // hop + 1)
    fb = tst.mel_basis.cpu().double().numpy()
    assert np.array_equal(fb, cases.slaney(sr, n_mel, fmin, fmax).astype(np.float64))
    judge_mel("B sr %d n_mel %d hop %d win %d" % (sr, n_mel, hop, win), mel, absX, fb)
    assert torch.equal(mel, tst.mel_spectrogram(dev(y)))


def test_b_silence_hits_the_floor_exactly(log_floor32):
    y = cases.silence()
    tst, mel = mel_b(*cases.B_BANKS[0], 256, 1024, y)
    judge_mel("B silence", mel, np.abs(stft64(y, 1024, 256, 1024)), tst.mel_basis.cpu().double().numpy())
    quiet = cases.silent_frames(1024, 256)
    got = mel.cpu().numpy()[:, :, quiet]
    print("B silence: %d frames of zeros, values there %s (logf(1e-5f) = %r)" % (quiet.sum(), np.unique(got), log_floor32))
    assert quiet.sum() >= 8 and np.all(got == log_floor32)
    assert np.any(mel.cpu().numpy()[:, :, :4] > log_floor32)                         # the quiet third is not all floor


# ---- C: hand-made CSR filterbanks through the entry points ------------------------------------------------------------------------
def mel_c(kind, n_fft, hop, y):
    """ft_stft_r8 (1024) or ft_stft_pow2 (512) called directly on a hand-made CSR; the mel buffer has one row of sentinels in
    front and one behind, checked here."""
    bin0, ptr, w = handmade_csr(kind, n_fft // 2 + 1)
    B, N = y.shape
    T = N // hop + 1
    st = audio_processing.STFT(n_fft, hop, n_fft).cuda()
    buf = torch.full((B * 128 + 2, T), SENTINEL, device="cuda")
    mel = buf[1:-1]
    yd, b0, pt, wd = dev(y), dev(bin0), dev(ptr), dev(w)
    head = (L.ptr(yd), L.ptr(st.fft_window), L.ptr(b0), L.ptr(pt), L.ptr(wd), mel.data_ptr(), None, None, B, N)
    if n_fft == 1024:
        L.check(L.lib().ft_stft_r8(*head, hop, 128, L.stream()), "ft_stft_r8")
    else:
        L.check(L.lib().ft_stft_pow2(*head, n_fft, hop, n_fft, 128, L.stream()), "ft_stft_pow2")
    torch.cuda.synchronize()
    assert torch.all(buf[0] == SENTINEL) and torch.all(buf[-1] == SENTINEL)
    return mel.reshape(B, 128, T).clone(), csr_dense64(bin0, ptr, w, n_fft // 2 + 1)


@pytest.mark.parametrize("kind,n_fft,hop", cases.C_CASES, ids=cases.C_IDS)
def test_c_handmade_filterbank(log_floor32, kind, n_fft, hop):
    y = cases.audio_c(n_fft, hop)
    T = y.shape[1] // hop + 1
    assert T % 16 != 0
    mel, fb = mel_c(kind, n_fft, hop, y)
    judge_mel("C %s n_fft %d hop %d (%d weights)" % (kind, n_fft, hop, int((fb != 0).sum())), mel, np.abs(stft64(y, n_fft, hop, n_fft)), fb)
    assert np.all(mel.cpu().numpy()[:, HANDMADE_EMPTY, :] == log_floor32)
    mel2, _ = mel_c(kind, n_fft, hop, y)
    assert torch.equal(mel, mel2)


# ---- D: ragged r8 entries -----------------------------------------------------------------------------------------------------------
def ragged_batch(lens, N):
    """[len(lens), N] with NaN behind every length."""
    y = np.full((len(lens), N), np.nan, np.float32)
    for i, n in enumerate(lens):
        y[i, :n] = cases.audio_d(i, n)
    return y


def check_ragged(y, lens, ref_fn):
    """mel_spectrogram_ragged and ft_stft_r8_ragged_phase on the NaN-padded batch; ref_fn(y_b) -> float64 spectrum of one
    utterance alone.  Returns the worst (|X|, phase, ratio)."""
    hop = 256
    B, N = y.shape
    tst = audio_processing.TacotronSTFT(1024, hop, 1024, *[cases.B_BANKS[0][i] for i in (1, 0, 2, 3)]).cuda()
    fb = tst.mel_basis.cpu().double().numpy()
    frames = [n // hop + 1 for n in lens]
    T_out = max(frames) + 3
    yd, ns = dev(y), dev(np.asarray(lens, np.int32))
    mel = tst.mel_spectrogram_ragged(yd, ns, T_out)
    mag, phase = tst.stft_fn._transform_ragged(yd, ns, want_magnitude=True)
    none, phase_only = tst.stft_fn._transform_ragged(yd, ns, want_magnitude=False)
    assert mel.shape == (B, 80, T_out) and mag.shape == phase.shape == (B, 513, N // hop + 1)
    assert none is None and torch.equal(phase.view(torch.int32), phase_only.view(torch.int32))      # mag = NULL: the same phase bits
    worst = np.zeros(3)
    for b, (n, t) in enumerate(zip(lens, frames)):
        X = ref_fn(y[b:b + 1, :n])
        assert X.shape == (1, 513, t)
        for z in (mel[b, :, :t], mag[b, :, :t], phase[b, :, :t]):
            assert torch.isfinite(z).all(), b
        e = judge_spectrum("D utterance %d (%d samples, %d frames)" % (b, n, t), mag[b:b + 1, :, :t], phase[b:b + 1, :, :t], X)
        r = judge_mel("D utterance %d (%d samples, %d frames)" % (b, n, t), mel[b:b + 1, :, :t], np.abs(X), fb)
        worst = np.maximum(worst, [e[0], e[1], r])
        assert torch.all(mel[b, :, t:] == 0) and torch.all(mag[b, :, t:] == 0) and torch.all(phase[b, :, t:] == 0), b
    return tst, mel, mag, phase, worst


def test_d_ragged_every_utterance_alone():
    lens = cases.D_LENS
    y = ragged_batch(lens, max(lens))
    _, _, _, _, worst = check_ragged(y, lens, lambda yb: stft64(yb, 1024, 256, 1024))
    print("D ragged: worst |X| %.2e, phase %.2e, ratio %.3f" % tuple(worst))


def test_d_short_utterance_single_fold():
    """An utterance of 300 <= n_fft / 2 samples between two ordinary ones: the dense call refuses it, the ragged launch computes
    the single-fold spectrum (stft64_single_fold), and its neighbours are bit for bit what they are without it."""
    lens = [cases.D_LENS[3], cases.D_SHORT, cases.D_LENS[0]]
    y = ragged_batch(lens, max(lens))
    tst, mel, mag, phase, worst = check_ragged(y, lens, lambda yb: stft64_single_fold(yb, 1024, 256, 1024))
    print("D short utterance: worst |X| %.2e, phase %.2e, ratio %.3f" % tuple(worst))
    with pytest.raises(RuntimeError, match="ft_stft_mel"):
        tst.mel_spectrogram(dev(y[1:2, :cases.D_SHORT]))
    for b in (0, 2):
        n = lens[b]
        t = n // 256 + 1
        assert torch.equal(mel[b, :, :t], tst.mel_spectrogram(dev(y[b:b + 1, :n]))[0])
        m1, p1 = tst.stft_fn.transform(dev(y[b:b + 1, :n]))
        assert torch.equal(mag[b, :, :t], m1[0]) and torch.equal(phase[b, :, :t], p1[0])


# ---- E: ft_stft_mel in the settings it alone serves -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases.E_CASES, ids=cases.E_IDS)
def test_e_general_kernel(monkeypatch, case):
    sr, n_fft, hop, win, n_mel, B, N = case
    tst = audio_processing.TacotronSTFT(n_fft, hop, win, n_mel, sr, 0.0, None).cuda()
    y = cases.audio_e(case)
    calls = count_calls(monkeypatch, STFT_ENTRIES)
    mel = tst.mel_spectrogram(dev(y))
    assert calls == dict({n: 0 for n in STFT_ENTRIES}, ft_stft_mel=1), calls
    assert mel.shape == (B, n_mel, N // hop + 1)
    judge_mel("E n_fft %d hop %d win %d n_mel %d N %d (%d frames)" % (n_fft, hop, win, n_mel, N, N // hop + 1), mel,
              np.abs(stft64(y, n_fft, hop, win)), tst.mel_basis.cpu().double().numpy())
    assert torch.equal(mel, tst.mel_spectrogram(dev(y)))


@pytest.mark.parametrize("n_fft,hop,win,n_mel,sr,N,match", [
    (800, 200, 800, 80, 22050, 4000, "invalid argument"),                 # not a power of two
    (1024, 256, 1024, 80, 22050, 512, "invalid argument"),                # exactly n_fft / 2 samples
    (4096, 4096, 4096, 160, 44100, 5000, "LDS"),                          # 4 (7 x 4096 + 4 x 4096 + 2052 + 8 x 160) B = 193 KB > 160 KB
], ids=["n800", "N512", "lds"])
def test_e_refused_settings(monkeypatch, n_fft, hop, win, n_mel, sr, N, match):
    tst = audio_processing.TacotronSTFT(n_fft, hop, win, n_mel, sr, 0.0, None).cuda()
    calls = count_calls(monkeypatch, STFT_ENTRIES)
    with pytest.raises(RuntimeError, match=match):
        tst.mel_spectrogram(torch.zeros(1, N, device="cuda"))
    assert calls == dict({n: 0 for n in STFT_ENTRIES}, ft_stft_mel=1), calls   # the entry was asked, and returned its error
    torch.cuda.synchronize()


# ---- F: the wrong references, seen from the device's own output ------------------------------------------------------------------
def test_f_device_output_is_far_from_every_wrong_reference(absx_b):
    smallest = np.inf
    named = dict(cases.MUTATION_INPUTS)
    # one r8 case of B
    sr, n_mel, fmin, fmax = cases.B_BANKS[0]
    y, absX = absx_b[256]
    tst, mel = mel_b(sr, n_mel, fmin, fmax, 256, 1024, y)
    runs = [(cases.F_B, y, (1024, 256, 1024), tst.mel_basis.cpu().double().numpy(), absX, mel.cpu().numpy())]
    # one of C: WIDE at 1024 / 255
    y = cases.audio_c(1024, 255)
    mel, fb = mel_c("WIDE", 1024, 255, y)
    runs.append((cases.F_C, y, (1024, 255, 1024), fb, np.abs(stft64(y, 1024, 255, 1024)), mel.cpu().numpy()))
    for name, y, st, fb, absX, got in runs:
        assert logmel_judge(got, absX, fb).max() <= 1.0
        for mut in named[name]:
            r = float(logmel_judge(MUTATIONS[mut](y, st, fb), absX, fb, center=got).max())
            print("F %-28s %-15s: %.0f bounds from the device's output" % (name, mut, r))
            assert r >= 4.0, (name, mut, r)
            smallest = min(smallest, r)
    print("F smallest wrong-reference ratio %.0f" % smallest)
