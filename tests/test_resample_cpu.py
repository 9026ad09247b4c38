"""Sample-rate conversion, host side (no GPU): the library's tap table against the float64 restatement of the definition
(tests/resample_ref64.py), the length arithmetic, argument validation, the `Data(resample=True)` switch through
DataCollate, and the definition itself against ideal resampled tones."""
import inspect
import math

import numpy as np
import pytest
import torch

import audio_processing
import resample_case as C
import resample_ref64 as R
from flowtron_amd import _lib as L
from flowtron_amd import audio as A
from flowtron_amd.data import Data, DataCollate, DeferredMel

PAIRS = [(24000, 22050), (16000, 22050), (44100, 22050), (48000, 8000), (8000, 48000)]
TONE_PAIRS = PAIRS + [(44100, 32000)]
SHAPE = {(24000, 22050): (147, 14), (16000, 22050): (441, 13), (44100, 22050): (1, 25), (48000, 8000): (1, 73),
         (8000, 48000): (6, 13)}                       # (phases, K): new / gcd and the issue's tap counts


# ---- 1. the tap table ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("orig,new", PAIRS)
def test_tap_table_equals_float64_definition(orig, new):
    taps, start, og, ng, K = A.resample_taps(orig, new)
    rt, rstart, rog, rng, rK = R.phase_table(orig, new)
    assert (og, ng, K) == (rog, rng, rK)
    assert (ng, K) == SHAPE[(orig, new)]
    assert taps.dtype == np.float32 and taps.shape == (ng, K) and start.dtype == np.int32
    assert np.array_equal(start, rstart)
    assert (taps == rt.astype(np.float32)).all()


def test_every_common_rate_pair_has_a_table():
    for orig in A.RESAMPLE_RATES:
        for new in A.RESAMPLE_RATES:
            if orig != new:
                taps, start, og, ng, K = A.resample_taps(orig, new)
                assert ng <= L.RESAMPLE_MAX_PHASES and ng * K <= L.RESAMPLE_MAX_TAPS, (orig, new, ng, K)
                assert taps.nbytes <= 72 * 1024                        # the largest: 11 025 -> 32 000 Hz, 1280 phases x 14 taps


# ---- 2. lengths ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("orig,new", PAIRS)
def test_output_length_is_ceil(orig, new):
    lib = L.lib()
    for n in (1, 2, 159, 160, 161, 22050, 10 ** 7):
        want = -((-n * new) // orig)
        assert A.resample_length(n, orig, new) == want
        assert audio_processing.resample_length(n, orig, new) == want
        assert lib.ft_resample_out_len(n, orig, new) == want
        assert R.out_len(n, orig, new) == want
    assert lib.ft_resample_out_len(-1, orig, new) == -1 and lib.ft_resample_out_len(5, 0, new) == -1


# ---- 3. signatures and refusals ------------------------------------------------------------------------------------------------
def test_signatures():
    assert list(inspect.signature(audio_processing.resample).parameters) == ["audio", "orig_sr", "new_sr"]
    assert list(inspect.signature(audio_processing.resample_ragged).parameters) == ["audio", "n_samples", "orig_sr", "new_sr"]
    assert list(inspect.signature(audio_processing.resample_length).parameters) == ["n", "orig_sr", "new_sr"]
    p = inspect.signature(Data.__init__).parameters
    assert list(p)[-1] == "resample" and p["resample"].default is False
    assert "source_rates" in inspect.signature(DeferredMel.__init__).parameters


def test_refusals():
    x = torch.zeros(2, 100)
    for bad in (0, -8000, 22050.0, "22050", True, None):
        with pytest.raises(ValueError):
            A.resample(x, bad, 22050)
        with pytest.raises(ValueError):
            A.resample_ragged(x, [100, 50], 24000, bad)
        with pytest.raises(ValueError):
            A.resample_length(10, bad, 22050)
    for lens in ([100, 0], [101, 5], [100], [100, 2.5], torch.tensor([100.0, 5.0])):
        with pytest.raises(ValueError):
            A.resample_ragged(x, lens, 24000, 22050)
    with pytest.raises(ValueError):
        A.resample(torch.zeros(2, 3, 4), 24000, 22050)
    with pytest.raises(NotImplementedError, match="8000/11025/16000/22050/24000/32000/44100/48000"):
        A.resample(x, 22050, 22051)
    with pytest.raises(NotImplementedError):
        A.resample_ragged(x, [100, 50], 22051, 22050)
    for f in (lambda: A.resample(x, 24000, 22050), lambda: A.resample(x, 22050, 22050),
              lambda: A.resample_ragged(x, [100, 50], 24000, 22050)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            f()


# ---- 4. the data path on the host ----------------------------------------------------------------------------------------------
def test_data_resample_switch(tmp_path):
    rows, counts = C.write_wavs(tmp_path, [24000, 22050, 24000, 16000])
    plain = Data(rows, text_frontend=C.grapheme_frontend, **C.DATA_KW)
    with pytest.raises(ValueError, match="SR doesn't match target"):
        plain[0]
    assert plain[1][0].n_frames == counts[1] // C.HOP + 1 and plain[1][0].source_rate is None
    ds = Data(rows, text_frontend=C.grapheme_frontend, resample=True, **C.DATA_KW)
    items = [ds[i] for i in range(4)]
    rates = [24000, 22050, 24000, 16000]
    frames = []
    for it, n, sr in zip(items, counts, rates):
        a = it[0]
        assert a.audio.numel() == n                                    # the audio travels at the file's rate
        assert a.source_rate == (None if sr == C.TARGET_SR else sr)
        want = -((-n * C.TARGET_SR) // sr) // C.HOP + 1
        assert a.n_frames == want
        frames.append(want)
    assert frames[0] != counts[0] // C.HOP + 1                         # the frame count is the resampled audio's, not the file's
    mel, spk, text, in_lens, out_lens, gate, prior = DataCollate(n_frames_per_step=1, use_attn_prior=True)(items)
    order = sorted(range(4), key=lambda i: -len(items[i][2]))
    assert in_lens.tolist() == [len(items[i][2]) for i in order]
    assert out_lens.tolist() == [frames[i] for i in order]
    T = max(frames)
    assert gate.shape == (4, T)
    for r, i in enumerate(order):
        assert gate[r].tolist() == [0.0] * (frames[i] - 1) + [1.0] * (T - frames[i] + 1)
    assert isinstance(mel, DeferredMel) and mel.max_t == T
    assert mel.source_rates == [rates[i] for i in order] and mel.n_samples.tolist() == [counts[i] for i in order]
    assert prior.out_lens.tolist() == out_lens.tolist() and prior.max_t == T
    same = DataCollate()([ds[1]])[0]                                   # a batch at the target rate only: the slot is as it always was
    assert same.source_rates is None
    with pytest.raises(NotImplementedError):                            # a pair the kernel does not take is refused in the worker
        Data(rows, text_frontend=C.grapheme_frontend, resample=True, **dict(C.DATA_KW, sampling_rate=22051))[0]


# ---- 5. the definition itself --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("orig,new", TONE_PAIRS)
def test_definition_resamples_tones(orig, new):
    n = -((-700 * orig) // new)
    for f in (200.0, 0.3 * min(orig, new)):
        x = np.sin(2 * np.pi * f * np.arange(n) / orig)
        y, _ = R.resample64(x, orig, new)
        ideal = np.sin(2 * np.pi * f * np.arange(len(y)) / new)
        assert len(y) >= 600
        err = np.abs(y - ideal)[200:-200].max()
        print("tone %g Hz, %d -> %d: interior error %.3e" % (f, orig, new, err))
        assert err <= 1e-2, (f, err)


def test_definition_suppresses_what_would_alias():
    # 0.45 * 44100 = 19 845 Hz is above the new Nyquist (11 025 Hz) and would alias to 2 205 Hz.  Bound: 0.3 (the issue's);
    # measured with this helper: interior amplitude 4.3e-4, the cos^2 window's stopband at 1.8x the cutoff.
    orig, new = 44100, 22050
    n = 1400
    x = np.sin(2 * np.pi * 0.45 * orig * np.arange(n) / orig)
    y, _ = R.resample64(x, orig, new)
    amp = np.abs(y)[200:-200].max()
    print("stopband amplitude %.3e" % amp)
    assert amp < 0.3


def test_helper_polyphase_view_matches_its_own_loop():
    # phase_table (what tests 1 and 8 compare against) says the same as the per-sample loop it is derived from
    orig, new = 16000, 22050
    x = np.random.RandomState(0).standard_normal(300)
    y, _ = R.resample64(x, orig, new)
    taps, start, og, ng, K = R.phase_table(orig, new)
    xp = np.concatenate([np.zeros(2 * K + og), x, np.zeros(2 * K + og)])
    for m in (0, 1, 7, 200, len(y) - 1):
        q, p = divmod(m, ng)
        k0 = q * og + int(start[p]) + 2 * K + og
        assert math.isclose(float(taps[p] @ xp[k0:k0 + K]), y[m], rel_tol=0, abs_tol=1e-14)
