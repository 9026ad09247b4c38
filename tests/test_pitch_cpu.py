"""F0 tracking and F0 error along a path without a GPU: the numpy restatement (tests/pitch_ref.py) on signals of known pitch,
its float32 against its float64 form, the edge frames, the float64 statement of the path statistics on hand-made contours,
f0_statistics, and the refusals of flowtron_amd.pitch / metrics.f0_distortion and of the C entries of csrc/pitch.hip before
anything reaches the device."""
import math

import numpy as np
import pytest
import torch

import pitch_ref as R
from flowtron_amd import metrics, pitch

U = 2.0 ** -24                                    # unit roundoff of float32
SEEDS = (1, 2, 3, 4)


def n_for(cfg):
    return 30 * cfg["hop"] + 7                    # 31 frames: 18 interior ones


@pytest.mark.parametrize("name", ["default", "small"])
def test_known_pitch_of_a_tone_is_found_in_every_interior_frame(name):
    cfg = R.CONFIGS[name]
    worst = 0.0
    for seed in SEEDS:
        x, f = R.tone(n_for(cfg), cfg, seed)
        f0, ap, lag, _, _ = R.yin(x, cfg, np.float64, details=True)
        T = len(f0)
        assert T == n_for(cfg) // cfg["hop"] + 1
        inner = slice(4, T - 8)                   # frames 4 .. T - 9
        assert np.all(lag[inner] > 0), (seed, lag)
        worst = max(worst, float(np.abs(f0[inner] / f - 1).max()))
        assert np.all(ap[inner] < cfg["threshold"])
    print("%s: worst relative F0 error %.2e" % (name, worst))
    assert worst <= 1e-3


@pytest.mark.parametrize("name", ["default", "small"])
def test_exact_grid_gives_the_same_bits_in_both_precisions_and_the_period_as_lag(name):
    cfg = R.CONFIGS[name]
    for seed in SEEDS:
        x, period = R.grid(n_for(cfg), cfg, seed)
        f32, a32, l32, d32, s32 = R.yin(x, cfg, np.float32, details=True)
        f64, a64, l64, d64, s64 = R.yin(x, cfg, np.float64, details=True)
        assert d32.dtype == np.float32 and d64.dtype == np.float64
        assert np.array_equal(d32.astype(np.float64), d64) and np.array_equal(s32.astype(np.float64), s64)
        assert np.array_equal(l32, l64)
        T = len(l32)
        assert np.all(l32[4:T - 8] == period), (period, l32)
        assert np.all(a32[4:T - 8] == 0)         # d(period) is an exact zero
        assert np.all(np.abs(f32[4:T - 8] * period / cfg["sr"] - 1) <= 0.5 / (period - 0.5))   # the parabola: half a lag at most


@pytest.mark.parametrize("name", ["default", "small"])
def test_float32_difference_function_stays_within_its_rounding_bound(name):
    """every term carries two roundings from the rounded difference, once squared, and one from the product; the sum adds at
    most W - 1 more"""
    cfg = R.CONFIGS[name]
    for kind in ("tone", "voice"):
        x = R.signal(kind, n_for(cfg), cfg, 5)
        d32, _ = R.difference(x, cfg, np.float32)
        d64, _ = R.difference(x, cfg, np.float64)
        assert np.all(np.abs(d32.astype(np.float64) - d64) <= 1.01 * (cfg["W"] + 2) * U * d64)


def test_float32_and_float64_replays_agree_on_tones_and_voices():
    """what keeps the device test honest: the float32 rule the kernel must reproduce bit for bit is itself the float64 tracker
    up to a handful of frames"""
    frames = differ = 0
    worst = 0.0
    for name, cfg in R.CONFIGS.items():
        for kind in ("tone", "voice"):
            for seed in SEEDS:
                x = R.signal(kind, n_for(cfg) if name == "default" else 60 * cfg["hop"] + 3, cfg, seed)
                f32, _, l32, _, _ = R.yin(x, cfg, np.float32, details=True)
                f64, _, l64, _, _ = R.yin(x, cfg, np.float64, details=True)
                frames += len(l32)
                differ += int((l32 != l64).sum())
                both = (l32 == l64) & (l32 > 0)
                if both.any():
                    worst = max(worst, float(np.abs(f32[both].astype(np.float64) / f64[both] - 1).max()))
    print("%d of %d frames differ in lag or voicing, worst F0 difference %.2e" % (differ, frames, worst))
    assert differ <= 0.01 * frames
    assert worst <= 1e-5


@pytest.mark.parametrize("name", ["default", "small"])
def test_edge_frames(name):
    cfg = R.CONFIGS[name]
    hop = cfg["hop"]
    for dtype in (np.float32, np.float64):
        f0, ap = R.yin(np.zeros(3 * hop, np.float32), cfg, dtype)
        assert len(f0) == 4 and np.all(f0 == 0) and np.all(ap == 1)
        f0, ap = R.yin(np.array([0.25], np.float32), cfg, dtype)
        assert len(f0) == 1 and len(ap) == 1
        for n in (hop - 1, hop, hop + 1):
            f0, _ = R.yin(R.signal("tone", n, cfg, 1), cfg, dtype)
            assert len(f0) == n // hop + 1
    assert pitch.lag_range(cfg["sr"], cfg["fmin"], cfg["fmax"]) == (cfg["tau_min"], cfg["tau_max"])


def test_path_statistics_on_hand_made_contours():
    fa = np.array([100.0, 0.0, 200.0, 220.0, 0.0], np.float32)
    diag = np.stack([np.arange(5)] * 2, 1)
    assert R.path_stats(fa, fa, diag) == (3, 0, 0.0)
    rmse, vuv, n = R.distortion(fa, 2 * fa, diag)
    assert n == 3 and vuv == 0 and abs(float(rmse) - 1200.0) < 1e-3
    fb = np.array([0.0, 50.0, 100.0], np.float32)
    path = np.array([[0, 0], [1, 0], [1, 1], [2, 2], [3, 2], [4, 2]])
    n_both, n_mis, total = R.path_stats(fa, fb, path)
    assert (n_both, n_mis) == (2, 3)              # (2,2) and (3,2) both; (0,0), (1,1), (4,2) one; (1,0) neither
    want = (1200 * math.log2(2.0)) ** 2 + (1200 * math.log2(2.2)) ** 2
    assert abs(total - want) < 1e-6 * want
    rmse, vuv, n = R.distortion(fa, fb, path)
    assert n == 2 and vuv == np.float32(0.5) and abs(float(rmse) - math.sqrt(want / 2)) < 1e-3
    rmse, vuv, n = R.distortion(fa, fb, np.array([[0, 0], [1, 0]]))
    assert n == 0 and np.isnan(rmse) and vuv == np.float32(0.5)


def test_f0_statistics_against_the_float64_statement():
    f0 = torch.tensor([[100.0, 0.0, 200.0, 400.0, 0.0], [0.0, 0.0, 0.0, 0.0, 0.0], [110.0, 110.0, 110.0, 0.0, 880.0]])
    n, mean, std = pitch.f0_statistics(f0)
    assert n.tolist() == [3, 0, 4] and mean.dtype == torch.float64 and std.dtype == torch.float64
    for b in range(3):
        wn, wm, ws = R.statistics(f0[b].numpy())
        assert int(n[b]) == wn
        if wn == 0:
            assert math.isnan(float(mean[b])) and math.isnan(float(std[b]))
        else:
            assert abs(float(mean[b]) - wm) < 1e-12 * abs(wm) and abs(float(std[b]) - ws) < 1e-9
    assert abs(float(mean[0]) - 12 * math.log2(200.0)) < 1e-9             # 100, 200, 400 Hz: an octave either side
    n, mean, std = pitch.f0_statistics(f0, [5, 5, 3])
    assert n.tolist() == [3, 0, 3] and float(std[2]) == 0.0 and abs(float(mean[2]) - 12 * math.log2(110.0)) < 1e-9
    n1, m1, s1 = pitch.f0_statistics(f0[0])
    assert n1.tolist() == [3] and float(m1[0]) == float(pitch.f0_statistics(f0)[1][0])
    with pytest.raises(ValueError, match="f0"):
        pitch.f0_statistics(f0[None])
    with pytest.raises(ValueError, match="lens"):
        pitch.f0_statistics(f0, [5, 5, 6])


def test_refusals_are_raised_without_a_device():
    x = torch.zeros(2, 4000)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pitch.f0(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pitch.f0(x[0], [4000])
    for bad in (x.double(), x[None], torch.zeros(2, 0), [0.0] * 10):
        with pytest.raises(ValueError, match="audio"):
            pitch.f0(bad)
    for kw, what in ((dict(sampling_rate=0), "sampling_rate"), (dict(sampling_rate=float("nan")), "sampling_rate"),
                     (dict(hop_length=0), "hop_length"), (dict(hop_length=2.0), "hop_length"), (dict(hop_length=True), "hop_length"),
                     (dict(win_length=0), "win_length"), (dict(win_length=None), "win_length"),
                     (dict(fmin=0.0), "fmin"), (dict(fmax=-1.0), "fmax"), (dict(fmin=500.0), "fmin must not exceed fmax"),
                     (dict(threshold=0.0), "threshold"), (dict(threshold=1.5), "threshold"), (dict(threshold=None), "threshold"),
                     (dict(fmax=12000.0), "half the sampling rate"),
                     (dict(n_samples=[4000]), "n_samples"), (dict(n_samples=[4000, 4001]), "n_samples"),
                     (dict(n_samples=[4000, 0]), "n_samples"), (dict(n_samples=torch.tensor([4000.0, 1.0])), "n_samples")):
        with pytest.raises(ValueError, match=what):
            pitch.f0(x, **kw)
    assert metrics.MAX_LAG == 1022 and pitch.MAX_WINDOW == 2048
    for kw in (dict(win_length=2050), dict(win_length=1023), dict(fmin=21.5), dict(sampling_rate=48000, fmin=40.0)):
        with pytest.raises(NotImplementedError, match="2048.*1022"):
            pitch.f0(x, **kw)
    with pytest.raises(NotImplementedError, match="65535"):
        pitch.f0(torch.zeros(65536, 1))

    fa, fb = torch.zeros(2, 6), torch.zeros(2, 4)
    path, plen = torch.zeros(2, 9, 2, dtype=torch.int32), torch.ones(2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.f0_distortion(fa, fb, path, plen)
    for args, what in (((fa[0], fb, path, plen), "f0_a"), ((fa, fb.double(), path, plen), "f0_b"), ((fa, fb[:1], path, plen), "one pair"),
                       ((fa, torch.zeros(2, 0), path, plen), "f0_b"), ((fa, fb, path.long(), plen), "path"),
                       ((fa, fb, path[:, :, :1], plen), "path"), ((fa, fb, path[:1], plen), "path"), ((fa, fb, path[0], plen), "path"),
                       ((fa, fb, path, plen.long()), "path_len"), ((fa, fb, path, plen[:1]), "path_len"), ((fa, fb, path, [1, 1]), "path_len"),
                       ((fa, fb, torch.zeros(2, 10, 2, dtype=torch.int32), plen), "at most 9")):
        with pytest.raises(ValueError, match=what):
            metrics.f0_distortion(*args)


def test_c_abi_refuses_bad_arguments_before_the_device():
    """FT_EINVAL / FT_EUNSUPPORTED from the entry points themselves, with host memory standing in for the buffers: nothing may
    be launched"""
    import ctypes as C
    from flowtron_amd import _lib as L
    lib = L.lib()
    audio = (C.c_float * 64)()
    n = (C.c_int32 * 2)()
    f0 = (C.c_float * 10)()
    ap = (C.c_float * 10)()
    ok = dict(audio=C.addressof(audio), s=(32, 1), n=C.addressof(n), f0=C.addressof(f0), ap=C.addressof(ap), B=2, N=32, sr=8000.0, hop=8,
              W=16, lo=2, hi=10, thr=0.15)

    def yin(**kw):
        a = dict(ok, **kw)
        return lib.ft_f0_yin_ragged(a["audio"], *a["s"], a["n"], a["f0"], a["ap"], a["B"], a["N"], a["sr"], a["hop"], a["W"], a["lo"],
                                    a["hi"], a["thr"], None)
    for kw in (dict(audio=None), dict(n=None), dict(f0=None), dict(ap=None), dict(B=0), dict(N=0), dict(hop=0), dict(W=0), dict(B=-1),
               dict(W=-2), dict(s=(-32, 1)), dict(s=(32, -1)), dict(lo=1), dict(lo=0), dict(lo=11), dict(hi=1), dict(thr=0.0),
               dict(thr=-0.5), dict(thr=1.25), dict(thr=float("nan")), dict(sr=0.0), dict(B=65536)):
        assert yin(**kw) == -1, kw
        assert b"ft_f0_yin_ragged" in lib.ft_last_error()
    for kw in (dict(W=2050), dict(W=15), dict(W=2049), dict(hi=1023)):      # FT_EUNSUPPORTED: beyond the limits
        assert yin(**kw) == -3, kw
        assert b"ft_f0_yin_ragged" in lib.ft_last_error() and b"2048" in lib.ft_last_error() and b"1022" in lib.ft_last_error()

    fa = (C.c_float * 12)()
    fb = (C.c_float * 8)()
    path = (C.c_int32 * 36)()
    plen = (C.c_int32 * 2)()
    nb = (C.c_int32 * 2)()
    nm = (C.c_int32 * 2)()
    sq = (C.c_double * 2)()
    oks = dict(fa=C.addressof(fa), sa=(6, 1), fb=C.addressof(fb), sb=(4, 1), path=C.addressof(path), plen=C.addressof(plen),
               nb=C.addressof(nb), nm=C.addressof(nm), sq=C.addressof(sq), B=2, Ta=6, Tb=4, P=9)

    def stats(**kw):
        a = dict(oks, **kw)
        return lib.ft_f0_path_stats(a["fa"], *a["sa"], a["fb"], *a["sb"], a["path"], a["plen"], a["nb"], a["nm"], a["sq"], a["B"],
                                    a["Ta"], a["Tb"], a["P"], None)
    for kw in (dict(fa=None), dict(fb=None), dict(path=None), dict(plen=None), dict(nb=None), dict(nm=None), dict(sq=None), dict(B=0),
               dict(Ta=0), dict(Tb=0), dict(P=0), dict(B=-2), dict(sa=(-6, 1)), dict(sa=(6, -1)), dict(sb=(-4, 1)), dict(sb=(4, -1)),
               dict(P=10), dict(Ta=5)):
        assert stats(**kw) == -1, kw
        assert b"ft_f0_path_stats" in lib.ft_last_error()
