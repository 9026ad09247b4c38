"""Pitch and pace of audio on the device (-m gpu): prosody.marks and prosody.modify against the fp32 replay (tests/prosody_ref.py)
bit for bit -- marks, counts, sources, half-widths, n_out and the output -- on a ragged batch whose padding is NaN in the audio
and in F0, every utterance alone and in the batch, a strided view and device lengths, an utterance with more frames than the
marks kernel keeps in LDS, grains dense enough for a second staging round of the synthesis; the identity bound; the chain
f0_track -> modify -> f0_track against the glide's true contour; entry calls and no synchronisation; n_out into the mel front
end and level.prepare.  8 kHz, a hop of 80; the F0 comes from pitch.f0_track on the device."""
import numpy as np
import pytest
import torch

import pitch_ref
import prosody_ref as R
import pyin_ref as P
from call_count import count_calls
from flowtron_amd import level, pitch, prosody
from flowtron_amd.audio import TacotronSTFT

pytestmark = pytest.mark.gpu

SR, HOP = 8000.0, 80
LENGTHS = (8000, 5000, 1601, 79, 1)
KW = dict(sampling_rate=SR, hop_length=HOP)
UP7 = 2.0 ** (7.0 / 12.0)
# name -> (pitch_ratio, pace); "monotone" and "mixed" take tensors made from the batch
SETTINGS = {"unity": (1.0, 1.0), "up7": (UP7, 1.0), "monotone": (None, 1.0), "clamp_low": (0.3, 1.0), "clamp_high": (5.0, 1.0),
            "slow": (1.0, 0.8), "fast": (1.0, 1.25), "mixed": (None, (0.8, 1.25, 1.0, 4.0, 0.25))}
MIXED_RATIOS = (1.5, 0.7, 2.0, 1.0, 0.625)

_CASE = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a).tobytes()


def track_on_device(audio, n_samples):
    cfg = P.config("small")
    return pitch.f0_track(audio, n_samples, sampling_rate=cfg["sr"], hop_length=cfg["hop"], win_length=cfg["W"], fmin=cfg["fmin"],
                          fmax=cfg["fmax"], bins_per_semitone=cfg["bps"], beta=cfg["beta"], absolute_min_prob=cfg["amp"],
                          max_octaves_per_second=cfg["max_octaves"], switch_prob=cfg["switch"])[0]


def case():
    """the utterances, their NaN-padded batch on the device and its F0 with NaN behind every utterance's frames, made once"""
    if not _CASE:
        glide = R.pulse_glide(1)[0]
        xs = [glide, pitch_ref.voice(5000, P.config("small"), 5), (0.05 * np.random.RandomState(7).randn(1601)).astype(np.float32),
              glide[:79].copy(), glide[:1].copy()]
        assert tuple(len(x) for x in xs) == LENGTHS
        X = np.full((len(xs), 8000), np.nan, np.float32)
        for b, x in enumerate(xs):
            X[b, :len(x)] = x
        Xd = dev(X)
        f0 = track_on_device(Xd, list(LENGTHS))
        frames = torch.tensor([n // HOP + 1 for n in LENGTHS], device="cuda")
        behind = torch.arange(f0.shape[1], device="cuda")[None, :] >= frames[:, None]
        f0 = torch.where(behind, torch.full_like(f0, float("nan")), f0)
        monotone = prosody.pitch_ratio(f0, lens=frames, range_scale=0.0)
        monotone = torch.where(behind, torch.full_like(f0, float("nan")), monotone)
        _CASE.update(xs=xs, X=Xd, f0=f0, f0_host=f0.cpu().numpy(), monotone=monotone, monotone_host=monotone.cpu().numpy(), replays={})
    return _CASE


def arguments(name):
    """-> (pitch_ratio for the device, per-utterance ratios for the replay, per-utterance paces)"""
    c = case()
    ratio, pace = SETTINGS[name]
    B = len(LENGTHS)
    if name == "monotone":
        return c["monotone"], [c["monotone_host"][b, :n // HOP + 1] for b, n in enumerate(LENGTHS)], [pace] * B, pace
    if name == "mixed":
        return torch.tensor(MIXED_RATIOS, dtype=torch.float32).cuda(), list(MIXED_RATIOS), list(pace), list(pace)
    return ratio, [ratio] * B, [pace] * B, pace


def replayed(name):
    c = case()
    if name not in c["replays"]:
        _, ratios, paces, _ = arguments(name)
        c["replays"][name] = [R.modify(x, c["f0_host"][b, :len(x) // HOP + 1], SR, HOP, ratios[b], paces[b])
                              for b, x in enumerate(c["xs"])]
    return c["replays"][name]


def assert_marks_equal(got, b, want, who):
    """utterance b of a Marks tuple (None: unbatched) against the replay's dict"""
    pick = (lambda t: t) if b is None else (lambda t: t[b])
    K, J = int(pick(got.n_analysis)), int(pick(got.n_synthesis))
    assert (K, J, int(pick(got.n_out))) == (len(want["analysis"]), len(want["synthesis"]), want["n_out"]), (who, b)
    assert bits(pick(got.analysis)[:K]) == want["analysis"].tobytes(), (who, b, "analysis")
    for key in ("synthesis", "source", "half"):
        assert bits(pick(getattr(got, key))[:J]) == want[key].tobytes(), (who, b, key)


def test_the_batch_holds_what_it_is_meant_to_hold():
    c = case()
    f0 = c["f0_host"]
    assert torch.isnan(c["X"][1, 5000:]).all() and np.isnan(f0[1, 63:]).all() and not np.isnan(f0[0]).any()
    assert (f0[0] > 0).sum() >= 75 and (f0[1, :63] > 0).sum() >= 40 and not (f0[2, :21] > 0).any()          # the noise burst: unvoiced
    for b, x in enumerate(c["xs"]):                                                                          # the tracker is bit-equal to its replay
        assert f0[b, :len(x) // HOP + 1].tobytes() == P.track(x, P.config("small"), np.float32)["f0"].tobytes(), b
    m = c["monotone_host"]
    assert 0.8 < np.nanmin(m[0]) < 0.97 and 1.03 < np.nanmax(m[0]) < 1.25 and np.all(m[2, :21] == 1)


@pytest.mark.parametrize("name", list(SETTINGS))
def test_marks_and_output_equal_the_replay_alone_and_in_the_batch(name):
    c = case()
    ratio, ratios, paces, pace = arguments(name)
    want = replayed(name)
    got = prosody.marks(c["X"], list(LENGTHS), c["f0"], pitch_ratio=ratio, pace=pace, **KW)
    out, n_out = prosody.modify(c["X"], list(LENGTHS), c["f0"], pitch_ratio=ratio, pace=pace, **KW)
    N_out = prosody.out_samples(8000, min(paces))
    assert all(t.dtype == torch.int32 and t.is_cuda for t in got) and n_out.dtype == torch.int32 and n_out.is_cuda
    assert tuple(out.shape) == (5, N_out) and out.dtype == torch.float32
    assert tuple(got.analysis.shape) == (5, 500) and tuple(got.synthesis.shape) == (5, -(-N_out // 8))
    assert bits(n_out) == bits(got.n_out)
    o = out.cpu().numpy()
    for b, (x, (w_out, w_marks)) in enumerate(zip(c["xs"], want)):
        assert_marks_equal(got, b, w_marks, name)
        n = w_marks["n_out"]
        assert o[b, :n].tobytes() == w_out.tobytes(), (name, b, "differs first at %s" % np.nonzero(o[b, :n].view(np.int32) != w_out.view(np.int32))[0][:5])
        assert not o[b, n:].any(), (name, b)
        r1 = ratio[b] if name == "mixed" else (ratio[b, :len(x) // HOP + 1] if name == "monotone" else ratio)
        f1 = c["f0"][b, :len(x) // HOP + 1].contiguous()
        alone = prosody.modify(dev(x), None, f1, pitch_ratio=r1, pace=paces[b], **KW)
        assert alone[1].dim() == 0 and int(alone[1]) == n and bits(alone[0]) == w_out.tobytes(), (name, b, "alone")
        assert_marks_equal(prosody.marks(dev(x), None, f1, pitch_ratio=r1, pace=paces[b], **KW), None, w_marks, name + " alone")


def test_the_clamps_are_the_settings_at_the_limits():
    c = case()
    for outside, limit in ((0.3, prosody.MIN_RATIO), (5.0, prosody.MAX_RATIO)):
        a = prosody.modify(c["X"], list(LENGTHS), c["f0"], pitch_ratio=outside, **KW)
        b = prosody.modify(c["X"], list(LENGTHS), c["f0"], pitch_ratio=limit, **KW)
        assert bits(a[0]) == bits(b[0]) and bits(a[1]) == bits(b[1])


def test_strided_audio_and_device_lengths_give_the_same_bits():
    c = case()
    want_out, want_n = prosody.modify(c["X"], list(LENGTHS), c["f0"], pitch_ratio=UP7, pace=1.25, **KW)
    wide = torch.full((5, 8000, 3), float("nan"), device="cuda")
    wide[:, :, 1] = c["X"]
    view = wide[:, :, 1]
    assert not view.is_contiguous()
    f0_wide = torch.full((5, 101, 2), float("nan"), device="cuda")
    f0_wide[:, :, 0] = c["f0"]
    n_dev = torch.tensor(LENGTHS, dtype=torch.int32).cuda()
    for audio, n, f0 in ((view, list(LENGTHS), c["f0"]), (c["X"], n_dev, c["f0"]), (view, n_dev, f0_wide[:, :, 0])):
        out, n_out = prosody.modify(audio, n, f0, pitch_ratio=UP7, pace=1.25, **KW)
        assert bits(out) == bits(want_out) and bits(n_out) == bits(want_n)
    loose = torch.tensor([9000, 5000, 1601, 79, 0], dtype=torch.int32).cuda()         # clamped to 1 ..= N in the kernels
    out, n_out = prosody.modify(c["X"], loose, c["f0"], pitch_ratio=UP7, pace=1.25, **KW)
    assert bits(out) == bits(want_out) and bits(n_out) == bits(want_n)


def test_identity_bound_holds_on_the_device():
    c = case()
    out, n_out = prosody.modify(c["X"], list(LENGTHS), c["f0"], **KW)
    m = prosody.marks(c["X"], list(LENGTHS), c["f0"], **KW)
    assert n_out.tolist() == list(LENGTHS)
    o = out.cpu().numpy()
    for b, x in enumerate(c["xs"]):
        K = int(m.n_analysis[b])
        assert K == int(m.n_synthesis[b]) and bits(m.analysis[b, :K]) == bits(m.synthesis[b, :K])
        assert m.source[b, :K].tolist() == list(range(K))
        worst = float(np.abs(o[b, :len(x)].astype(np.float64) - x).max())
        print("utterance %d: %d marks, max |out - x| = %.2e" % (b, K, worst))
        assert worst <= 1e-6
    big = c["xs"][0] / np.abs(c["xs"][0]).max()                               # the bound is stated for |x| <= 1
    got = prosody.modify(dev(big), None, c["f0"][0].contiguous(), **KW)[0].cpu().numpy()
    assert float(np.abs(got.astype(np.float64) - big).max()) <= 1e-6


def test_more_frames_than_the_marks_kernel_keeps_in_lds():
    """a hop of 16: 4376 frames, 280 of them behind the 4096 the wave stages; 249 tiles of the synthesis"""
    n, hop = 70000, 16
    rng = np.random.RandomState(11)
    x = (0.2 * rng.randn(n)).astype(np.float32)
    t = np.arange(n // hop + 1)
    f0 = (150.0 * 2.0 ** (0.4 * np.sin(2 * np.pi * t / 700.0))).astype(np.float32)
    f0[(t % 300) > 250] = 0.0
    ratio = (2.0 ** (0.5 * np.cos(2 * np.pi * t / 300.0))).astype(np.float32)
    assert len(t) > 4096 and (f0[4096:] > 0).any() and (f0[4096:] == 0).any()
    w_out, w_marks = R.modify(x, f0, SR, hop, ratio, 1.1)
    got = prosody.marks(dev(x), None, dev(f0), SR, hop, dev(ratio), 1.1)
    assert_marks_equal(got, None, w_marks, "long")
    out, n_out = prosody.modify(dev(x), None, dev(f0), SR, hop, dev(ratio), 1.1)
    assert int(n_out) == w_marks["n_out"] == len(w_out) and bits(out) == w_out.tobytes()


def test_grains_dense_enough_for_a_second_staging_round():
    """500 Hz at ratio 2: a grain every 8 samples, 288 within reach of a tile of 256 samples, more than one round of 256"""
    n = 4000
    x = (0.3 * np.sin(2 * np.pi * 500.0 * np.arange(n) / SR)).astype(np.float32)
    f0 = np.full(n // HOP + 1, 500.0, np.float32)
    w_out, w_marks = R.modify(x, f0, SR, HOP, 2.0, 1.0)
    assert len(w_marks["synthesis"]) == 500 and np.all(w_marks["half"] == 16)
    wide = R.modify(x, np.full(n // HOP + 1, 8.0, np.float32), SR, HOP, 2.0, 1.0)    # half-widths of 1000: every tile reaches far
    assert np.all(wide[1]["half"] == 1000)
    for f, (want_out, want_marks) in ((f0, (w_out, w_marks)), (np.full(n // HOP + 1, 8.0, np.float32), wide)):
        assert_marks_equal(prosody.marks(dev(x), None, dev(f), pitch_ratio=2.0, **KW), None, want_marks, "dense")
        assert bits(prosody.modify(dev(x), None, dev(f), pitch_ratio=2.0, **KW)[0]) == want_out.tobytes()


@pytest.mark.parametrize("semitones", [7, -7])
@pytest.mark.parametrize("seed", [1, 2])
def test_device_chain_meets_the_f0_conditions(seed, semitones):
    x, truth, voiced = R.pulse_glide(seed)
    r = 2.0 ** (semitones / 12.0)
    audio = dev(x)
    f0 = track_on_device(audio, None)
    out, n_out = prosody.modify(audio, None, f0, pitch_ratio=r, **KW)
    got = P.score(track_on_device(out, n_out.reshape(1).tolist()).cpu().numpy(), truth * r, voiced)
    print("%+d semitones, seed %d, on the device: %s" % (semitones, seed, got))
    assert got["gross"] == 0 and got["missed"] <= 3 and got["rms"] <= 15.0, got


def test_modify_makes_two_entry_calls_and_never_synchronises(monkeypatch):
    c = case()
    n_dev = torch.tensor(LENGTHS, dtype=torch.int32).cuda()
    want = prosody.modify(c["X"], n_dev, c["f0"], pitch_ratio=c["monotone"], pace=1.25, **KW)        # warm: the window table is on the device
    entries = ("ft_psola_marks", "ft_psola_synth")
    calls = count_calls(monkeypatch, entries)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out, n_out = prosody.modify(c["X"], n_dev, c["f0"], pitch_ratio=c["monotone"], pace=1.25, **KW)
        also = prosody.modify(c["X"], n_dev, c["f0"], pitch_ratio=UP7, pace=1.25, **KW)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert calls == {n: 2 for n in entries}
    assert bits(out) == bits(want[0]) and bits(n_out) == bits(want[1]) and also[0].shape == out.shape
    prosody.marks(c["X"], n_dev, c["f0"], **KW)
    assert calls == {"ft_psola_marks": 3, "ft_psola_synth": 2}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        prosody.modify(c["X"].cpu(), list(LENGTHS), c["f0"].cpu(), **KW)


def test_n_out_feeds_the_mel_front_end_and_prepare_unchanged():
    c = case()
    out, n_out = prosody.modify(c["X"], list(LENGTHS), c["f0"], pitch_ratio=UP7, pace=0.8, **KW)
    stft = TacotronSTFT(filter_length=256, hop_length=64, win_length=256, n_mel_channels=40, sampling_rate=8000, mel_fmin=0.0,
                        mel_fmax=4000.0).cuda()
    mel = stft.mel_spectrogram_ragged(out[:3], n_out[:3])                    # (the two fragments are shorter than the STFT's reflection)
    lens = n_out.tolist()
    assert lens == [prosody.out_samples(n, 0.8) for n in LENGTHS]
    for b in (0, 1, 2):
        n = lens[b]
        alone = stft.mel_spectrogram(out[b:b + 1, :n].contiguous())
        assert bits(mel[b, :, :n // 64 + 1]) == bits(alone[0]), b
    prepared, n_prep, info = level.prepare(out, n_out, 8000, top_db=60.0, frame_length=256, hop_length=64)
    again, n_again, _ = level.prepare(out, lens, 8000, top_db=60.0, frame_length=256, hop_length=64)
    assert bits(prepared) == bits(again) and bits(n_prep) == bits(n_again) and n_prep.dtype == torch.int32
    f0_after = track_on_device(out, n_out.tolist())
    assert tuple(f0_after.shape) == (5, out.shape[1] // HOP + 1)
