"""Probabilistic YIN on the device (-m gpu): pitch.f0_candidates and pitch.f0_track against the float32 replay
(tests/pyin_ref.py) bit for bit -- candidate mass, refined frequencies, voiced mass and the path's F0 -- on a ragged batch from a
contiguous tensor and from a strided view, every utterance alone and in the batch, the default configuration, the edge frames
and other bin and lag layouts; pitch.f0 unchanged on the same audio; launch counts; the accuracy conditions on the device's
output."""
import numpy as np
import pytest
import torch

import pitch_ref as R
import pyin_ref as P
from call_count import count_calls
from flowtron_amd import pitch

pytestmark = pytest.mark.gpu

_REPLAYS = {}


def replay(x, cfg):
    """the float32 replay of an utterance, once"""
    key = (x.tobytes(), tuple(sorted((k, str(v)) for k, v in cfg.items())))
    if key not in _REPLAYS:
        _REPLAYS[key] = P.track(x, cfg, np.float32)
    return _REPLAYS[key]


def args(cfg):
    return dict(sampling_rate=cfg["sr"], hop_length=cfg["hop"], win_length=cfg["W"], fmin=cfg["fmin"], fmax=cfg["fmax"],
                bins_per_semitone=cfg["bps"], beta=cfg["beta"], absolute_min_prob=cfg["amp"])


def on_device(audio, n_samples, cfg):
    """-> numpy dict(prob, freq, f0, voiced) of pitch.f0_candidates and pitch.f0_track"""
    prob, freq = pitch.f0_candidates(audio, n_samples, **args(cfg))
    f0, voiced = pitch.f0_track(audio, n_samples, max_octaves_per_second=cfg["max_octaves"], switch_prob=cfg["switch"], **args(cfg))
    for t in (prob, freq, f0, voiced):
        assert t.is_cuda and t.dtype == torch.float32
    T = audio.shape[-1] // cfg["hop"] + 1
    assert tuple(prob.shape) == tuple(freq.shape) == tuple(audio.shape[:-1]) + (T, P.n_bins(cfg))
    assert tuple(f0.shape) == tuple(voiced.shape) == tuple(audio.shape[:-1]) + (T,)
    return dict(prob=prob.cpu().numpy(), freq=freq.cpu().numpy(), f0=f0.cpu().numpy(), voiced=voiced.cpu().numpy())


def same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and a.view(np.int32).tobytes() == b.view(np.int32).tobytes()


def assert_equals_replay(got, b, x, cfg):
    """utterance b of a device result (None: an unbatched one) against the replay of its samples x; zeros behind its frames"""
    want = replay(x, cfg)
    Tb = len(want["f0"])
    for key in ("prob", "freq", "voiced", "f0"):
        g = got[key] if b is None else got[key][b]
        if not same_bits(g[:Tb], want[key]):
            bad = np.nonzero(np.asarray(g[:Tb]).reshape(Tb, -1).view(np.int32) != want[key].reshape(Tb, -1).view(np.int32))
            raise AssertionError("%s of utterance %s differs from the replay at frames %s" % (key, b, sorted(set(bad[0].tolist()))[:10]))
        assert np.all(g[Tb:] == 0), key


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


RAGGED = ((8000, "voice"), (5000, "tone"), (1234, "grid"))


def ragged_batch(cfg):
    xs = [R.signal(kind, n, cfg, 11 + b) for b, (n, kind) in enumerate(RAGGED)]
    return xs, [n for n, _ in RAGGED]


def test_ragged_batch_equals_the_replay_contiguous_strided_and_alone():
    """279 bins, a band of 43; 101, 63 and 16 frames.  NaN stands behind every utterance and between the samples of the strided
    view: it is never read.  pitch.f0 on the same audio still equals its own replay."""
    cfg = P.config("small")
    assert (P.n_bins(cfg), P.band(cfg)) == (279, 43)
    xs, ns = ragged_batch(cfg)
    flat = np.full((3, 8000), np.nan, np.float32)
    for b, x in enumerate(xs):
        flat[b, :len(x)] = x
    contiguous = dev(flat)
    big = torch.full((5, 2 * 8100 + 3), float("nan"))
    big[1:4, 1:2 * 8000 + 1:2] = torch.from_numpy(flat)
    strided = big.cuda()[1:4, 1:2 * 8000 + 1:2]
    assert contiguous.is_contiguous() and not strided.is_contiguous() and tuple(strided.shape) == (3, 8000)
    results = [on_device(a, ns, cfg) for a in (contiguous, strided)]
    for got in results:
        assert tuple(got["f0"].shape) == (3, 101)
        for b, x in enumerate(xs):
            assert_equals_replay(got, b, x, cfg)
        assert not any(np.isnan(v).any() for v in got.values())
    for b, x in enumerate(xs):                                      # alone: [N] and [1, N], its own length as N
        alone = on_device(dev(x), None, cfg)
        assert_equals_replay(alone, None, x, cfg)
        Tb = len(alone["f0"])
        for key in alone:
            assert same_bits(alone[key], results[0][key][b, :Tb]), (key, b)
    want = replay(xs[0], cfg)
    assert (want["f0"] > 0).sum() > 40 and (want["f0"] == 0).sum() > 10 and (want["prob"] > 0).sum() > 80    # the case has what it is meant to have
    f0, ap = pitch.f0(strided, ns, cfg["sr"], cfg["hop"], cfg["W"], cfg["fmin"], cfg["fmax"], cfg["threshold"])
    f0, ap = f0.cpu().numpy(), ap.cpu().numpy()
    for b, x in enumerate(xs):
        yf, ya = R.yin(x, cfg, np.float32)
        assert same_bits(f0[b, :len(yf)], yf) and same_bits(ap[b, :len(ya)], ya), b


def test_default_configuration_equals_the_replay():
    """329 bins, a band of 50, 173 frames"""
    cfg = P.config("default")
    assert (P.n_bins(cfg), P.band(cfg)) == (329, 50)
    x = R.signal("voice", 44100, cfg, 4)
    got = on_device(dev(x), None, cfg)
    assert got["f0"].shape == (173,)
    assert_equals_replay(got, None, x, cfg)
    assert (got["f0"] > 0).sum() > 60 and (got["f0"] == 0).sum() > 20
    f0, ap = pitch.f0(dev(x))
    yf, ya = R.yin(x, cfg, np.float32)
    assert same_bits(f0.cpu().numpy(), yf) and same_bits(ap.cpu().numpy(), ya)


def test_edge_utterances_one_sample_silence_nan_and_garbage_behind_the_length():
    cfg = P.config("small")
    N = 2000
    tone = R.signal("tone", N, cfg, 3)
    with_nan = tone.copy()
    with_nan[1000] = np.nan
    short = R.signal("voice", 700, cfg, 8)
    xs = [tone[:1], np.zeros(N, np.float32), with_nan, short]
    flat = np.full((4, N), np.nan, np.float32)                      # garbage behind every length
    for b, x in enumerate(xs):
        flat[b, :len(x)] = x
    got = on_device(dev(flat), [len(x) for x in xs], cfg)
    for b, x in enumerate(xs):
        assert_equals_replay(got, b, x, cfg)
    assert not any(np.isnan(v).any() for v in got.values())
    assert np.all(got["prob"][1] == 0) and np.all(got["f0"][1] == 0) and np.all(got["voiced"][1] == 0)      # digital silence
    start = np.arange(N // cfg["hop"] + 1) * cfg["hop"] - cfg["W"] // 2
    sees = (start <= 1000) & (1000 < start + cfg["W"] + cfg["tau_max"] + 1)
    assert sees.sum() >= 4 and np.all(got["prob"][2][sees] == 0) and np.all(got["f0"][2][sees] == 0)
    assert (got["f0"][2][~sees] > 0).sum() > 10
    one = on_device(dev(tone[:1]), None, cfg)                       # T = 1
    assert one["f0"].shape == (1,) and one["f0"][0] == 0
    assert_equals_replay(one, None, tone[:1], cfg)


@pytest.mark.parametrize("kw", [dict(bps=5), dict(fmin=100.0), dict(fmax=300.0, bps=12), dict(amp=0.5, switch=0.2, max_octaves=10.0),
                                dict(beta=(2.0, 8.0), max_octaves=52.0)])
def test_other_bins_lags_and_settings_equal_the_replay(kw):
    """bins_per_semitone 5 (140 bins, a band of 22); 61 lags, one to a lane; 275 bins of a twelfth of a semitone; a heavy global
    minimum with a narrow band of 12; a flatter prior with the widest band that fits, 62"""
    cfg = P.config("small", **kw)
    cfg["tau_min"], cfg["tau_max"] = pitch.lag_range(cfg["sr"], cfg["fmin"], cfg["fmax"])
    x = R.signal("voice", 3000, cfg, 6)
    assert_equals_replay(on_device(dev(x), None, cfg), None, x, cfg)
    y = R.signal("tone", 1500, cfg, 2)
    assert_equals_replay(on_device(dev(y), None, cfg), None, y, cfg)


def test_repeated_calls_give_identical_bytes_and_two_launches_per_track(monkeypatch):
    cfg = P.config("small")
    x = dev(np.stack([R.signal("voice", 2000, cfg, s) for s in range(4)]))
    ns = [2000, 1999, 80, 1]
    names = ["ft_f0_candidates_ragged", "ft_f0_viterbi_ragged", "ft_f0_yin_ragged"]
    calls = count_calls(monkeypatch, names)
    first = pitch.f0_track(x, ns, max_octaves_per_second=cfg["max_octaves"], switch_prob=cfg["switch"], **args(cfg))
    assert calls == {"ft_f0_candidates_ragged": 1, "ft_f0_viterbi_ragged": 1, "ft_f0_yin_ragged": 0}
    cand = pitch.f0_candidates(x, ns, **args(cfg))
    assert calls == {"ft_f0_candidates_ragged": 2, "ft_f0_viterbi_ragged": 1, "ft_f0_yin_ragged": 0}
    second = pitch.f0_track(x, ns, max_octaves_per_second=cfg["max_octaves"], switch_prob=cfg["switch"], **args(cfg))
    for a, b in zip(first, second):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    assert float(cand[0].sum(-1).max()) <= 1.0 + 1e-6
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pitch.f0_track(x.cpu(), ns)


@pytest.mark.parametrize("sigma", [0.05, 0.10])
def test_accuracy_conditions_hold_on_the_device(sigma):
    """The noisy glide of tests/pyin_ref.py, seeds 1 and 2 in one batch; the conditions are tests/pyin_ref.check_conditions, the same as
    on the float64 replay (tests/test_pyin_cpu.py has its figures); the noise gives frames with several candidates, so the bits
    are compared here too.  The tracker's F0 goes into f0_statistics as it is."""
    cfg = P.config("small")
    made = [P.noisy_glide(sigma, seed) for seed in (1, 2)]
    audio = dev(np.stack([m[0] for m in made]))
    f0, voiced_prob = pitch.f0_track(audio, None, max_octaves_per_second=cfg["max_octaves"], switch_prob=cfg["switch"], **args(cfg))
    cand = [t.cpu().numpy() for t in pitch.f0_candidates(audio, None, **args(cfg))]
    plain, _ = pitch.f0(audio, None, cfg["sr"], cfg["hop"], cfg["W"], cfg["fmin"], cfg["fmax"], cfg["threshold"])
    for b, (x, truth, voiced) in enumerate(made):
        got = P.score(f0[b].cpu().numpy(), truth, voiced)
        yin = P.score(plain[b].cpu().numpy(), truth, voiced)
        print("sigma %.2f seed %d: tracker %s; plain YIN %s" % (sigma, b + 1, got, yin))
        P.check_conditions(sigma, got, yin)
        assert_equals_replay(dict(f0=f0.cpu().numpy(), voiced=voiced_prob.cpu().numpy(), **dict(zip(("prob", "freq"), cand))), b, x, cfg)
    n, mean, std = pitch.f0_statistics(f0)
    assert torch.all(n > 40) and not torch.isnan(std).any()
