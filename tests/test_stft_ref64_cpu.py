"""The float64 STFT oracle of the GPU tests (tests/stft_ref64.py) against the REAL reference's recorded outputs in
tests/golden/stft_pow2.pt (tests/golden/make_golden_stft_pow2.py), no GPU needed: STFT.transform magnitudes, STFT.inverse and
window_sumsquare at the fixture's three settings (sr16k 512 / 128, sr24k 2048 / 300 / 1200, sr44k 2048 / 512), inside the bounds
the device code is held to (test_gpu_stft_pow2.py: relative L2 1e-6), and griffin_lim64 tied to istft64.  The reference runs in
float32, so what is measured is its own rounding: 2.1e-7 .. 7.6e-7 (transform), 3.0e-7 .. 3.3e-7 (inverse).

The second half holds the mel front end's bound (stft_ref64.logmel_judge) to its purpose on the very inputs of
test_gpu_stft_front_end_f64.py (tests/stft_front_end_cases.py): an honest fp32 computation (torch.stft in float32, a float32
filterbank sum, log) lies inside it, every wrong reference lies at least four bounds outside, the phase mask keeps most of every
frame, and the hand-made filterbanks have the properties their names promise."""
import math
import os

import numpy as np
import pytest
import torch

import stft_front_end_cases as cases
from stft_ref64 import (FLOOR, HANDMADE_BIN0, HANDMADE_EMPTY, HANDMADE_LAST, HANDMADE_WIDTHS, MUTATIONS, TINY32, csr_dense64,
                        frame_rel_l2, griffin_lim64, handmade_csr, istft64, logmel_judge, mel64, phase_mask, rel_l2, start_angles,
                        stft64, stft64_single_fold, wss64)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stft_pow2.pt")
MAG_BOUND, INV_BOUND = 1e-6, 1e-6                  # the bounds of test_gpu_stft_pow2.py (stft_ref64.MAG_BOUND is the same number)
EPS32 = float(np.finfo(np.float32).eps)
NAMES = ["sr16k", "sr24k", "sr44k"]


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN, weights_only=False)


def spectrum(g, n_fft):
    """The fixture's inverse input, as make_golden_stft_pow2.random_spectrum draws it."""
    rs = np.random.RandomState(g["seed"])
    M = rs.uniform(0.0, 2.0, (g["B"], n_fft // 2 + 1, g["T"])).astype(np.float32)
    P = rs.uniform(-np.pi, np.pi, (g["B"], n_fft // 2 + 1, g["T"])).astype(np.float32)
    return M, P


@pytest.mark.parametrize("name", NAMES)
def test_transform_matches_reference(golden, name):
    from oracle import synth
    _, n_fft, hop, win = golden["settings"][name]
    g = golden[name]["transform"]
    y = synth.make_audio(g["n_samples"], seed=g["audio_seed"])[None].numpy()
    mag = np.abs(stft64(y, n_fft, hop, win))
    assert mag.shape == (1, n_fft // 2 + 1, g["n_samples"] // hop + 1)
    e = rel_l2(mag[0][:, ::golden["mag_stride"]], g["mag"].numpy())
    print("%s transform: f64 oracle vs reference rel L2 %.2e" % (name, e))
    assert e <= MAG_BOUND


@pytest.mark.parametrize("name", NAMES)
def test_inverse_matches_reference(golden, name):
    _, n_fft, hop, win = golden["settings"][name]
    g = golden[name]["inverse"]
    assert (g["B"], g["T"]) == (1, 12)
    M, P = spectrum(g, n_fft)
    y, wss = istft64(M, P, n_fft, hop, win)
    assert y.shape == (1, hop * 11) and wss.shape == (hop * 11,)
    e = rel_l2(y[:, ::golden["y_stride"]], g["y"].numpy())
    print("%s inverse: f64 oracle vs reference rel L2 %.2e" % (name, e))
    assert e <= INV_BOUND


@pytest.mark.parametrize("name", NAMES)
def test_griffin_lim_zero_iterations_is_the_inverse(golden, name):
    _, n_fft, hop, win = golden["settings"][name]
    M, _ = spectrum(golden[name]["inverse"], n_fft)
    A = start_angles(M.shape, seed=5)
    assert A.dtype == np.float32 and np.array_equal(A, start_angles(M.shape, seed=5))
    assert np.array_equal(griffin_lim64(M, A, 0, n_fft, hop, win), istft64(M, A, n_fft, hop, win)[0])


@pytest.mark.parametrize("name", NAMES)
def test_wss_matches_reference(golden, name):
    """The reference adds the window's squares (float64) into a float32 envelope: every sample takes at most ceil(n_fft / hop)
    additions of non-negative terms, each rounding the running sum once (<= eps32 / 2 of it), so the float32 envelope is within
    ceil(n_fft / hop) eps32 / 2 of the exact one, relatively; exact zeros stay zero."""
    _, n_fft, hop, win = golden["settings"][name]
    case = golden[name]["wss"]
    a = case["args"]
    assert (a["n_fft"], a["hop_length"], a["win_length"]) == (n_fft, hop, win)
    ref = case["out"].numpy().astype(np.float64)
    got = wss64(a["n_frames"], n_fft, hop, win)
    assert got.shape == ref.shape == (n_fft + hop * 11,)
    rtol = math.ceil(n_fft / hop) * EPS32 / 2
    live = got > TINY32
    worst = float((np.abs(got[live] - ref[live]) / got[live]).max())
    print("%s wss: max relative deviation %.2e (bound %.2e), %d zeros" % (name, worst, rtol, int((~live).sum())))
    assert worst <= rtol
    assert np.array_equal(got == 0, ref == 0)
    # the trimmed envelope istft64 returns is the same one
    M = np.ones((1, n_fft // 2 + 1, a["n_frames"]), np.float32)
    assert np.array_equal(istft64(M, np.zeros_like(M), n_fft, hop, win)[1], got[n_fft // 2:got.size - n_fft // 2])


# ---- the mel front end's bound on the inputs of test_gpu_stft_front_end_f64.py ------------------------------------------------
def test_bounds_are_the_projects():
    import stft_ref64
    assert (stft_ref64.MAG_BOUND, stft_ref64.PHASE_BOUND) == (1e-6, 1e-4) and MAG_BOUND == stft_ref64.MAG_BOUND


@pytest.fixture(scope="module")
def mel_inputs():
    """name -> (y, settings, fb, |X| float64): computed once, read by every test below."""
    return {name: (y, st, fb, np.abs(stft64(y, *st))) for name, y, st, fb in cases.mel_inputs()}


def fp32_stand_in(y, settings, fb):
    """(magnitudes, log-mel) of a plain fp32 computation: torch.stft in float32, a float32 filterbank sum, log."""
    n_fft, hop, win = settings
    X = torch.stft(torch.from_numpy(np.asarray(y, np.float32)), n_fft, hop_length=hop, win_length=win,
                   window=torch.hann_window(win, periodic=True), center=True, pad_mode="reflect", return_complex=True)
    mag = X.abs()
    mel = torch.log(torch.clamp(torch.einsum("mk,bkt->bmt", torch.from_numpy(np.asarray(fb, np.float32)), mag), min=1e-5))
    return mag.numpy(), mel.numpy()


def test_fp32_stand_in_is_inside_the_bound(mel_inputs):
    worst_r, worst_m = 0.0, 0.0
    for name, (y, st, fb, absX) in mel_inputs.items():
        mag, mel = fp32_stand_in(y, st, fb)
        assert mel.shape == (y.shape[0], fb.shape[0], y.shape[1] // st[1] + 1), name
        r = float(logmel_judge(mel, absX, fb).max())
        e = float(frame_rel_l2(mag, absX).max())
        print("%-34s fp32 stand-in: ratio %.3f, per-frame |X| rel L2 %.2e" % (name, r, e))
        assert r <= 1.0, (name, r)
        assert e <= MAG_BOUND, (name, e)
        worst_r, worst_m = max(worst_r, r), max(worst_m, e)
    print("fp32 stand-in over %d inputs: worst ratio %.3f, worst per-frame |X| rel L2 %.2e" % (len(mel_inputs), worst_r, worst_m))


def test_float64_reference_judges_itself_zero(mel_inputs):
    y, st, fb, absX = mel_inputs[cases.F_B]
    assert float(np.abs(logmel_judge(mel64(y, *st, fb), absX, fb)).max()) == 0.0


def test_every_mutation_leaves_the_bound(mel_inputs):
    smallest = np.inf
    for name, muts in cases.MUTATION_INPUTS:
        y, st, fb, absX = mel_inputs[name]
        for mut in muts:
            r = float(logmel_judge(MUTATIONS[mut](y, st, fb), absX, fb).max())
            print("%-34s %-15s worst ratio %.0f" % (name, mut, r))
            assert r >= 4.0, (name, mut, r)
            smallest = min(smallest, r)
    assert {m for _, ms in cases.MUTATION_INPUTS for m in ms} == set(MUTATIONS)
    print("smallest mutation ratio %.0f" % smallest)


def test_floor_mutation_needs_silence(mel_inputs):
    """Why the floor has an input of its own: on ordinary audio no Slaney band sum is below 1e-5, the two floors agree."""
    y, st, fb, absX = mel_inputs[cases.F_B]
    assert np.einsum("mk,bkt->bmt", fb, absX).min() > FLOOR
    y, st, fb, absX = mel_inputs["B_silence"]
    quiet = cases.silent_frames(st[0], st[1])
    assert quiet.sum() >= 8 and not quiet[:4].any()
    assert np.all(absX[:, :, quiet] == 0) and np.all(mel64(y, *st, fb)[:, :, quiet] == np.log(FLOOR))


def test_phase_mask_keeps_most_of_every_frame():
    lo = 1.0
    for g, name in zip(cases.A_GRID, cases.A_IDS):
        hop, win, B, N = g
        keep = phase_mask(np.abs(stft64(cases.audio_a(*g), 1024, hop, win))).mean(axis=1)       # [B, T]
        print("%-24s phase mask keeps %.1f %% .. %.1f %% of a frame's bins" % (name, 100 * keep.min(), 100 * keep.max()))
        assert keep.min() >= 0.8, (name, keep.min())
        lo = min(lo, float(keep.min()))
    for i, n in enumerate(cases.D_LENS):
        keep = phase_mask(np.abs(stft64(cases.audio_d(i, n)[None], 1024, 256, 1024))).mean(axis=1)
        assert keep.min() >= 0.8, (i, keep.min())
        lo = min(lo, float(keep.min()))
    for i, n in ((0, cases.D_LENS[3]), (2, cases.D_LENS[0])):                 # the short utterance's two neighbours
        keep = phase_mask(np.abs(stft64(cases.audio_d(i, n)[None], 1024, 256, 1024))).mean(axis=1)
        assert keep.min() >= 0.8, (i, n, keep.min())
        lo = min(lo, float(keep.min()))
    keep = phase_mask(np.abs(stft64_single_fold(cases.audio_d(1, cases.D_SHORT)[None], 1024, 256, 1024))).mean(axis=1)
    print("short utterance (single fold): phase mask keeps %.1f %% .. %.1f %%" % (100 * keep.min(), 100 * keep.max()))
    assert keep.min() >= 0.8
    lo = min(lo, float(keep.min()))
    print("phase mask: the emptiest frame keeps %.1f %%" % (100 * lo))


@pytest.mark.parametrize("n_bins", [513, 257])
def test_handmade_filterbanks(n_bins):
    for kind in ("WIDE", "NARROW"):
        bin0, ptr, w = handmade_csr(kind, n_bins)
        n = np.diff(ptr)
        assert bin0.dtype == np.int32 and ptr.dtype == np.int32 and w.dtype == np.float32
        assert len(bin0) == 128 and len(ptr) == 129 and ptr[0] == 0 and ptr[-1] == len(w)
        assert np.all(w > 0)
        assert np.all(bin0 >= 0) and np.all(bin0 + n <= n_bins)                   # no band reaches past the last bin
        assert n[HANDMADE_EMPTY] == 0
        assert (bin0[HANDMADE_BIN0], n[HANDMADE_BIN0]) == (0, 1)
        assert (bin0[HANDMADE_LAST], n[HANDMADE_LAST]) == (n_bins - 1, 1)
        cyc = HANDMADE_WIDTHS[kind]
        assert list(n[:125]) == [cyc[m % len(cyc)] for m in range(125)]
        if kind == "WIDE":
            assert len(w) == 2127 > 2048                                           # the global-memory branch
            assert np.all(n[:125] == 17) and bin0[124] + 17 == n_bins              # the last wide band ends on the last bin
            if n_bins == 513:
                assert list(bin0[:125]) == [4 * m for m in range(125)]
        else:
            assert len(w) == 1203 <= 2048                                          # staged in LDS
            assert set(n[:125]) == {1, 7, 8, 9, 16, 17}
        fb = csr_dense64(bin0, ptr, w, n_bins)
        assert fb.shape == (128, n_bins) and fb.dtype == np.float64
        assert np.array_equal((fb != 0).sum(axis=1), n) and not fb[HANDMADE_EMPTY].any()
        assert fb[HANDMADE_BIN0, 0] == w[ptr[HANDMADE_BIN0]] and fb[HANDMADE_LAST, n_bins - 1] == w[ptr[HANDMADE_LAST]]
        from flowtron_amd.audio import filterbank_csr
        b2, p2, w2 = filterbank_csr(fb.astype(np.float32))                        # the project's own CSR of that matrix
        assert np.array_equal(p2, ptr) and np.array_equal(w2, w) and np.array_equal(b2[n > 0], bin0[n > 0])


def test_slaney_never_reaches_what_the_handmade_banks_do():
    """The reason for the hand-made filterbanks: over the B filterbanks no Slaney bank at 1024 weights bin 0 or bin 512, has an
    empty band, or more than 2048 weights."""
    from flowtron_amd.audio import filterbank_csr
    for bank in cases.B_BANKS:
        fb = cases.slaney(*bank)
        assert not fb[:, 0].any() and not fb[:, 512].any()
        _, ptr, w = filterbank_csr(fb)
        assert np.diff(ptr).min() >= 1 and len(w) <= 2048


@pytest.mark.parametrize("n_fft,hop,win,N", [(1024, 256, 1024, 513), (1024, 255, 800, 2000), (512, 1, 512, 300), (1024, 200, 800, 3089)])
def test_single_fold_equals_reflect_padding_above_half(n_fft, hop, win, N):
    y = cases.audio(2, N, seed=7)
    assert np.array_equal(stft64_single_fold(y, n_fft, hop, win), stft64(y, n_fft, hop, win))


def test_single_fold_of_a_short_signal():
    """300 samples at 1024 / 256, the kernel's rule written out sample by sample: n < 0 -> -n, then n >= 300 -> 598 - n, zero
    where that is still outside.  Frame 0 is wholly folded signal; frame 1 reaches past 598 and ends in zeros."""
    y = cases.audio(1, cases.D_SHORT, seed=8)
    X = stft64_single_fold(y, 1024, 256, 1024)
    assert X.shape == (1, 513, 2)
    w = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(1024) / 1024)
    zeros = []
    for t in range(2):
        fr = np.zeros(1024)
        for j in range(1024):
            m = t * 256 + j - 512
            m = -m if m < 0 else m
            m = 2 * 299 - m if m >= 300 else m
            fr[j] = y[0, m] if 0 <= m < 300 else 0.0
        zeros.append(int((fr == 0).sum()))
        assert np.allclose(X[0, :, t], np.fft.rfft(fr * w), rtol=0, atol=1e-12)
    assert zeros[0] == 0 and zeros[1] >= 767 - 598
