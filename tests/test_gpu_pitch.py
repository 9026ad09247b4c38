"""F0 tracking and F0 error along a path on the device (-m gpu): the YIN kernel against its float32 replay
(tests/pitch_ref.py) bit for bit -- F0 and aperiodicity of voiced, unvoiced, silent and edge frames --, raggedness inside a
poisoned view, the lag limits, the path statistics against the float64 statement, repeatability and launch counts, and the
chain from a small model's mels to an F0 error along the warping path."""
import os

import numpy as np
import pytest
import torch

import pitch_ref as R
from call_count import count_calls
from flowtron_amd import metrics, ops, pitch

pytestmark = pytest.mark.gpu

_REPLAYS = {}


def replay(kind, name, n, seed=7, **lags):
    """(x, f0, aperiodicity) of a shared signal at a configuration, replayed once in float32"""
    key = (kind, name, n, seed, tuple(sorted(lags.items())))
    if key not in _REPLAYS:
        cfg = R.with_lags(R.CONFIGS[name], **lags)
        x = R.signal(kind, n, R.CONFIGS[name], seed)
        _REPLAYS[key] = (x,) + R.yin(x, cfg, np.float32)
    return _REPLAYS[key]


def track(x, n_samples, cfg):
    """ops.f0_yin_ragged on a device tensor with the lags of cfg as they are -> numpy (f0, aperiodicity)"""
    n32 = torch.tensor(n_samples, dtype=torch.int32, device=x.device)
    f0, ap = ops.f0_yin_ragged(x, n32, cfg["sr"], cfg["hop"], cfg["W"], cfg["tau_min"], cfg["tau_max"], cfg["threshold"])
    assert f0.dtype == torch.float32 and ap.dtype == torch.float32 and f0.is_cuda and ap.is_cuda
    assert tuple(f0.shape) == tuple(ap.shape) == (x.shape[0], x.shape[1] // cfg["hop"] + 1)
    return f0.cpu().numpy(), ap.cpu().numpy()


def same_bits(a, b):
    return np.asarray(a, np.float32).view(np.int32).tolist() == np.asarray(b, np.float32).view(np.int32).tolist()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("kind", ["tone", "voice", "grid"])
@pytest.mark.parametrize("name,n", [("small", 1), ("small", 79), ("small", 80), ("small", 81), ("small", 2000),
                                    ("default", 1), ("default", 255), ("default", 256), ("default", 4000)])
def test_tracker_equals_the_float32_replay_bit_for_bit(name, n, kind):
    cfg = R.CONFIGS[name]
    x, want_f0, want_ap = replay(kind, name, n)
    f0, ap = pitch.f0(dev(x), None, cfg["sr"], cfg["hop"], cfg["W"], cfg["fmin"], cfg["fmax"], cfg["threshold"])
    assert tuple(f0.shape) == (n // cfg["hop"] + 1,)
    f0, ap = f0.cpu().numpy(), ap.cpu().numpy()
    assert same_bits(f0, want_f0), (f0, want_f0)
    assert same_bits(ap, want_ap), (ap, want_ap)
    if n >= 2000 and kind != "grid":
        assert (want_f0 > 0).any() and (kind == "tone" or (want_f0 == 0).any())        # the case has what it is meant to have


def test_ragged_batch_inside_a_padded_view_equals_each_utterance_alone():
    """three utterances in a non-contiguous view of a larger buffer, NaN behind every length and all around: each equals itself
    tracked alone, bit for bit; frames behind an utterance's are 0; nothing is NaN"""
    cfg = R.SMALL
    lens = [4000, 1300, 1]
    big = torch.full((5, 2 * 4100 + 3), float("nan"))
    view = big[1:4, 1:2 * 4000 + 1:2]
    xs = []
    for b, (n, kind) in enumerate(zip(lens, ("voice", "tone", "tone"))):
        x = R.signal(kind, n, cfg, 20 + b)
        view[b, :n] = torch.from_numpy(x)
        xs.append(x)
    d = big.cuda()
    v = d[1:4, 1:2 * 4000 + 1:2]
    assert not v.is_contiguous() and tuple(v.shape) == (3, 4000)
    f0, ap = pitch.f0(v, torch.tensor(lens).cuda(), cfg["sr"], cfg["hop"], cfg["W"], cfg["fmin"], cfg["fmax"], cfg["threshold"])
    f0, ap = f0.cpu().numpy(), ap.cpu().numpy()
    assert f0.shape == (3, 51)
    assert not np.isnan(f0).any() and not np.isnan(ap).any()
    for b, n in enumerate(lens):
        Tb = n // cfg["hop"] + 1
        alone = track(dev(xs[b])[None], [n], cfg)
        assert same_bits(f0[b, :Tb], alone[0][0]) and same_bits(ap[b, :Tb], alone[1][0]), b
        want = R.yin(xs[b], cfg, np.float32)
        assert same_bits(f0[b, :Tb], want[0]) and same_bits(ap[b, :Tb], want[1]), b
        assert np.all(f0[b, Tb:] == 0) and np.all(ap[b, Tb:] == 0)
    assert (f0[0] > 0).sum() > 10


def test_non_finite_samples_silence_the_frames_that_see_them_and_no_others():
    cfg = R.SMALL
    x = R.signal("tone", 2000, cfg, 3).copy()
    clean = track(dev(x)[None], [2000], cfg)
    for bad in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[1000] = bad
        f0, ap = track(dev(y)[None], [2000], cfg)
        t = np.arange(len(f0[0]))
        start = t * cfg["hop"] - cfg["W"] // 2
        sees = (start <= 1000) & (1000 < start + cfg["W"] + cfg["tau_max"] + 1)
        assert sees.sum() >= 4 and np.all(f0[0][sees] == 0)
        assert same_bits(f0[0][~sees], clean[0][0][~sees]) and same_bits(ap[0][~sees], clean[1][0][~sees])


@pytest.mark.parametrize("lags", [dict(tau_min=21, tau_max=99), dict(tau_min=37, tau_max=37), dict(tau_min=2, tau_max=3),
                                  dict(tau_min=20, tau_max=101), dict(tau_min=20, tau_max=102)])
def test_lag_ranges_off_the_four_lags_of_a_thread(lags):
    cfg = R.with_lags(R.SMALL, **lags)
    for kind in ("tone", "voice"):
        x, want_f0, want_ap = replay(kind, "small", 1500, **lags)
        f0, ap = track(dev(x)[None], [1500], cfg)
        assert same_bits(f0[0], want_f0) and same_bits(ap[0], want_ap), kind


def test_the_widest_window_and_the_longest_lag():
    """W = 2048 and tau_max = 1022, the limits; and a window that is no multiple of four"""
    base = dict(R.DEFAULT, hop=512, W=2048, tau_min=55, tau_max=1022)
    x = R.signal("voice", 6000, R.DEFAULT, 9)
    for cfg in (base, dict(R.SMALL, W=250), dict(R.SMALL, W=2, hop=3)):
        n = 6000 if cfg is base else 700
        want = R.yin(x[:n], cfg, np.float32)
        f0, ap = track(dev(x[:n])[None], [n], cfg)
        assert same_bits(f0[0], want[0]) and same_bits(ap[0], want[1]), cfg
    with pytest.raises(NotImplementedError, match="1022"):
        pitch.f0(dev(x), sampling_rate=22050, fmin=21.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pitch.f0(torch.from_numpy(x))


def contours(Ta, Tb, seed):
    rng = np.random.RandomState(seed)
    fa = np.where(rng.rand(Ta) < 0.7, rng.uniform(80, 300, Ta), 0).astype(np.float32)
    fb = np.where(rng.rand(Tb) < 0.7, rng.uniform(80, 300, Tb), 0).astype(np.float32)
    return fa, fb


def stairs(Ta, Tb):
    """a full-length path: up the first column, then along the last row -- Ta + Tb - 1 cells"""
    return np.array([[i, 0] for i in range(Ta)] + [[Ta - 1, j] for j in range(1, Tb)], np.int32)


def test_path_statistics_equal_the_float64_statement():
    Ta, Tb = 40, 33
    P = Ta + Tb - 1
    diag = np.array([[min(c, Ta - 1), min(c * Tb // Ta, Tb - 1)] for c in range(Ta)], np.int32)
    paths = [stairs(Ta, Tb), np.array([[5, 7]], np.int32), diag, np.array([[0, 0], [1, 1]], np.int32)]
    B = len(paths)
    fa, fb = np.zeros((B, Ta), np.float32), np.zeros((B, Tb), np.float32)
    path = np.full((B, P, 2), -1, np.int32)
    for b, p in enumerate(paths):
        fa[b], fb[b] = contours(Ta, Tb, 40 + b)
        path[b, :len(p)] = p
    fa[1, 5], fb[1, 7] = 100.0, 200.0                                       # the one-cell path: an octave
    fa[3, :2], fb[3, :2] = (0.0, 120.0), (0.0, 0.0)                          # no cell with both voiced
    plen = np.array([len(p) for p in paths], np.int32)
    rmse, vuv, n = metrics.f0_distortion(dev(fa), dev(fb), dev(path), dev(plen))
    assert rmse.dtype == torch.float32 and vuv.dtype == torch.float32 and n.dtype == torch.int32
    rmse, vuv, n = rmse.cpu().numpy(), vuv.cpu().numpy(), n.cpu().numpy()
    for b, p in enumerate(paths):
        want_rmse, want_vuv, want_n = R.distortion(fa[b], fb[b], p)
        assert n[b] == want_n, b
        assert same_bits(vuv[b], want_vuv), (b, vuv[b], want_vuv)
        if want_n == 0:
            assert np.isnan(rmse[b])
        else:                                                               # formed in float64: only the final rounding can differ
            assert rmse[b] == want_rmse or rmse[b] in (np.nextafter(want_rmse, np.float32(0)), np.nextafter(want_rmse, np.float32(1e9))), b
    assert n[1] == 1 and rmse[1] == np.float32(1200.0) and n[3] == 0 and vuv[3] == np.float32(0.5)
    eq = dev(np.stack([np.arange(Tb, dtype=np.int32)] * 2, 1)[None])          # equal contours along the diagonal: 0 cents
    same = metrics.f0_distortion(dev(fa[:1]), dev(fa[:1, :Tb]), eq, dev(np.array([Tb], np.int32)))
    assert float(same[0][0]) == 0 and float(same[1][0]) == 0 and int(same[2][0]) == int((fa[0, :Tb] > 0).sum()) > 0
    # strided contours, read in place
    wide = torch.full((B, 2 * Ta + 1), float("nan")).cuda()
    wide[:, 1::2] = dev(fa)
    again = metrics.f0_distortion(wide[:, 1::2], dev(fb), dev(path), dev(plen))
    assert same_bits(again[0].cpu().numpy()[:3], rmse[:3]) and np.array_equal(again[2].cpu().numpy(), n)


def test_repeated_calls_give_identical_bytes_and_one_launch_per_call(monkeypatch):
    cfg = R.SMALL
    x = dev(np.stack([R.signal("voice", 2000, cfg, s) for s in range(5)]))
    names = ["ft_f0_yin_ragged", "ft_f0_path_stats"]
    calls = count_calls(monkeypatch, names)
    args = (cfg["sr"], cfg["hop"], cfg["W"], cfg["fmin"], cfg["fmax"], cfg["threshold"])
    first = pitch.f0(x, [2000, 1999, 800, 80, 1], *args)
    assert calls == {"ft_f0_yin_ragged": 1, "ft_f0_path_stats": 0}
    second = pitch.f0(x, [2000, 1999, 800, 80, 1], *args)
    assert calls["ft_f0_yin_ragged"] == 2
    for a, b in zip(first, second):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    T = first[0].shape[1]
    path = dev(np.tile(stairs(T, T)[None], (5, 1, 1)))
    plen = torch.full((5,), 2 * T - 1, dtype=torch.int32).cuda()
    one = metrics.f0_distortion(first[0], first[0].flip(0), path, plen)
    assert calls == {"ft_f0_yin_ragged": 2, "ft_f0_path_stats": 1}
    two = metrics.f0_distortion(first[0], first[0].flip(0), path, plen)
    assert calls["ft_f0_path_stats"] == 2
    for a, b in zip(one, two):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


@pytest.fixture(scope="module")
def case():
    """the small model and ragged batch of three of tests/test_gpu_metrics.py's `case`, fp32 operand mode"""
    import flowtron
    from oracle import synth
    old = os.environ.get("FLOWTRON_MFMA")
    os.environ["FLOWTRON_MFMA"] = "f32"
    cfg = dict(synth.SMALL_MODEL_CONFIG)
    m = flowtron.Flowtron(**cfg)
    m.load_state_dict(synth.make_state_dict(cfg, seed=31))
    m = m.cuda().eval()
    b = synth.make_batch(cfg, [30, 21, 17], [9, 7, 5], seed=31, with_prior=False)
    b = {k: b[k].cuda() for k in ("mel", "speaker_ids", "text", "in_lens", "out_lens")}
    yield dict(m=m, b=b, il=b["in_lens"].tolist(), ol=b["out_lens"].tolist())
    if old is None:
        os.environ.pop("FLOWTRON_MFMA", None)
    else:
        os.environ["FLOWTRON_MFMA"] = old


def test_from_a_models_mels_to_an_f0_error_along_the_warping_path(case):
    """infer_aligned reconstruction -> mel_to_audio_ragged -> pitch.f0 on both waveforms -> f0_distortion along the frame-by-frame
    path.  An untrained model's pitch means nothing: the chain runs, the shapes fit and the counts are consistent."""
    from flowtron_amd.audio import TacotronSTFT
    m, b, il, ol = case["m"], case["b"], case["il"], case["ol"]
    mel = b["mel"]
    z, attn, _ = m.alignments(mel, b["speaker_ids"], b["text"], b["in_lens"], b["out_lens"])
    back, lengths = m.infer_aligned(z, b["speaker_ids"], b["text"], attn, in_lens=il, n_frames=ol)
    stft = TacotronSTFT(n_mel_channels=mel.shape[1]).cuda()
    hop = stft.stft_fn.hop_length
    audio_a = stft.mel_to_audio_ragged(mel, ol, n_iters=2)
    audio_b = stft.mel_to_audio_ragged(back, lengths.tolist(), n_iters=2)
    n_a, n_b = [hop * (n - 1) for n in ol], [hop * (n - 1) for n in lengths.tolist()]
    f0_a, _ = pitch.f0(audio_a, n_a, hop_length=hop)
    f0_b, _ = pitch.f0(audio_b, n_b, hop_length=hop)
    assert f0_a.shape[1] == mel.shape[2] and f0_b.shape[1] == back.shape[2]   # hop (T - 1) samples: one F0 frame per mel frame
    mcd, path, path_len = metrics.mel_cepstral_distortion(mel, ol, back, ol, align=False, return_path=True)
    rmse, vuv, n_both = metrics.f0_distortion(f0_a, f0_b, path, path_len)
    print("rmse %s cents, voicing error %s, both voiced %s of %s cells" % (rmse.tolist(), vuv.tolist(), n_both.tolist(), path_len.tolist()))
    n_mis = torch.round(vuv.double() * path_len.double()).long()
    assert torch.all(n_both >= 0) and torch.all(n_both.long() + n_mis <= path_len.long())
    assert torch.all(torch.isnan(rmse) == (n_both == 0)) and torch.all((vuv >= 0) & (vuv <= 1))
    n, mean, std = pitch.f0_statistics(f0_a, ol)
    assert torch.all(n <= torch.tensor(ol, device=n.device)) and torch.all(torch.isnan(mean) == (n == 0))
