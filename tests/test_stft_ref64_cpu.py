"""The float64 STFT oracle of the GPU tests (tests/stft_ref64.py) against the REAL reference's recorded outputs in
tests/golden/stft_pow2.pt (tests/golden/make_golden_stft_pow2.py), no GPU needed: STFT.transform magnitudes, STFT.inverse and
window_sumsquare at the fixture's three settings (sr16k 512 / 128, sr24k 2048 / 300 / 1200, sr44k 2048 / 512), inside the bounds
the device code is held to (test_gpu_stft_pow2.py: relative L2 1e-6), and griffin_lim64 tied to istft64.  The reference runs in
float32, so what is measured is its own rounding: 2.1e-7 .. 7.6e-7 (transform), 3.0e-7 .. 3.3e-7 (inverse)."""
import math
import os

import numpy as np
import pytest
import torch

from stft_ref64 import TINY32, griffin_lim64, istft64, rel_l2, start_angles, stft64, wss64

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stft_pow2.pt")
MAG_BOUND, INV_BOUND = 1e-6, 1e-6                  # the bounds of test_gpu_stft_pow2.py
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
