"""Probabilistic YIN without a GPU: the numpy restatement (tests/pyin_ref.py) against itself -- an exact periodic signal, the mass
of a frame, float32 against float64 --, the accuracy conditions on its float64 form, the host-side tables of flowtron_amd.pitch
against the replay's own, and the refusals of pitch.f0_candidates / pitch.f0_track and of the C entries before anything
reaches the device."""
import numpy as np
import pytest
import torch

import pitch_ref as R
import pyin_ref as P
from flowtron_amd import metrics, pitch

SEEDS = (1, 2)


@pytest.mark.parametrize("name", ["default", "small"])
def test_exact_grid_puts_all_mass_on_the_periods_bin_and_the_track_returns_the_period(name):
    cfg = P.config(name)
    n = 30 * cfg["hop"] + 7
    for seed in (1, 2, 3):
        x, period = R.grid(n, cfg, seed)
        for dtype in (np.float32, np.float64):
            r = P.track(x, cfg, dtype)
            T = len(r["f0"])
            inner = slice(4, T - 8)
            edges = P.tables(cfg, dtype)["edges"]
            k = int(np.nonzero(edges[:-1] >= period)[0][-1])
            # d'(period) = 0 is below every threshold and the global minimum.  A shallow trough at a shorter lag (d' near 1) is
            # by the rule the first one below the thresholds above its own d', whose Beta(2, 18) weight is an ulp of 1 at most
            assert np.all(r["prob"][inner, k] >= 1 - 1e-6), (seed, r["prob"][inner, k])
            assert np.all(np.delete(r["prob"][inner], k, axis=1).sum(1) <= 1e-6)
            assert np.all(r["states"][inner] == 2 * k + 1)
            assert np.array_equal(r["f0"][inner], r["freq"][inner, k])
            assert np.all(np.abs(r["f0"][inner] * period / cfg["sr"] - 1) <= 0.5 / (period - 0.5))       # the parabola: half a lag at most
            assert np.all(r["voiced"] <= 1.0 + 1e-6) and np.all(r["prob"].sum(1) <= 1.0 + 1e-6)


@pytest.mark.parametrize("kind", ["voice", "tone"])
def test_mass_is_at_most_one_and_both_precisions_choose_the_same_path(kind):
    cfg = P.config("small")
    x = R.signal(kind, 4000, cfg, 5)
    a, b = P.track(x, cfg, np.float32), P.track(x, cfg, np.float64)
    for r in (a, b):
        assert np.all(r["prob"] >= 0) and np.all(r["voiced"] <= 1.0 + 1e-6)
        assert np.all((r["freq"] > 0) == (r["prob"] > 0))
        assert np.all(r["f0"][r["states"] % 2 == 0] == 0) and np.all(r["f0"][r["states"] % 2 == 1] > 0)
    assert np.array_equal(a["states"], b["states"])
    assert np.allclose(a["f0"], b["f0"], rtol=1e-4)
    if kind == "voice":                                             # voiced, then noise, then exact zeros
        on = a["f0"] > 0
        assert on[3:25].all() and not on[-4:].any()
        assert np.all(a["prob"][-3:] == 0) and np.all(a["voiced"][-3:] == 0)      # digital silence: no mass


def test_a_frame_with_a_non_finite_sample_has_no_mass_and_the_path_goes_on():
    cfg = P.config("small")
    x = R.signal("tone", 2000, cfg, 3).copy()
    clean = P.track(x, cfg, np.float32)
    x[1000] = np.nan
    r = P.track(x, cfg, np.float32)
    start = np.arange(len(r["f0"])) * cfg["hop"] - cfg["W"] // 2
    sees = (start <= 1000) & (1000 < start + cfg["W"] + cfg["tau_max"] + 1)
    assert sees.sum() >= 4 and np.all(r["prob"][sees] == 0) and np.all(r["f0"][sees] == 0)
    assert np.array_equal(r["prob"][~sees], clean["prob"][~sees])
    assert not np.isnan(r["f0"]).any() and (r["f0"][~sees] > 0).sum() > 10


@pytest.mark.parametrize("sigma", [0.05, 0.10])
@pytest.mark.parametrize("seed", SEEDS)
def test_accuracy_conditions_hold_on_the_float64_replay(sigma, seed):
    """The noisy glide (tests/pyin_ref.noisy_glide), 81 truly voiced frames of 101.  This replay gave, seeds 1 and 2:
    sigma 0.05: missed 0 / 0, false-voiced 2 / 3, none 100 cents off, RMS 9.7 / 8.6 cents (plain YIN misses 11 / 12);
    sigma 0.10: missed 2 / 15, false-voiced 3 / 2, none 100 cents off, RMS 22.4 / 23.3 cents (plain YIN voices nothing)."""
    cfg = P.config("small")
    x, truth, voiced = P.noisy_glide(sigma, seed)
    assert voiced.sum() == 81 and len(voiced) == 101
    got = P.score(P.track(x, cfg, np.float64)["f0"], truth, voiced)
    yin = P.score(R.yin(x, cfg, np.float64)[0], truth, voiced)
    print("sigma %.2f seed %d: tracker %s; plain YIN %s" % (sigma, seed, got, yin))
    P.check_conditions(sigma, got, yin)


def test_host_tables_equal_the_replays_own():
    """flowtron_amd.pitch forms the Beta table from a continued fraction, the replay from quadrature: the same float32"""
    for name, beta, bps in (("small", (2.0, 18.0), 10), ("default", (2.0, 18.0), 10), ("small", (2.0, 34.0 / 3.0), 5), ("default", (3.0, 8.0), 12)):
        cfg = P.config(name, beta=beta, bps=bps)
        want = P.tables(cfg, np.float32)
        cum, edges, centres = pitch.candidate_tables(cfg["sr"], cfg["fmin"], cfg["fmax"], bps, beta)
        for a, b in ((cum, want["cum"]), (edges, want["edges"]), (centres, want["centres"])):
            assert a.dtype == np.float32 and a.tobytes() == b.tobytes()
        assert len(centres) == P.n_bins(cfg) == pitch.n_pitch_bins(cfg["fmin"], cfg["fmax"], bps)
        bd = pitch.transition_band(cfg["max_octaves"], bps, cfg["hop"], cfg["sr"])
        assert bd == P.band(cfg) and pitch.transition_table(bd).tobytes() == want["tri"].tobytes()
        assert cum[0] == 0 and cum[100] == 1 and np.all(np.diff(cum) >= 0) and np.all(np.diff(edges) < 0)
        assert abs(float(pitch.transition_table(bd).astype(np.float64).sum()) - 1) < 1e-6
    assert (P.n_bins(P.config("default")), P.band(P.config("default"))) == (329, 50)
    assert (P.n_bins(P.config("small")), P.band(P.config("small"))) == (279, 43)
    assert abs(pitch.beta_cdf(0.5, 1.0, 1.0) - 0.5) < 1e-15 and abs(pitch.beta_cdf(0.25, 2.0, 1.0) - 0.0625) < 1e-15


def test_refusals_are_raised_without_a_device():
    x = torch.zeros(2, 4000)
    for fn in (pitch.f0_candidates, pitch.f0_track):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(x)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(x[0], [4000])
        for bad in (x.double(), x[None], torch.zeros(2, 0), [0.0] * 10):
            with pytest.raises(ValueError, match="audio"):
                fn(bad)
        for kw, what in ((dict(sampling_rate=0), "sampling_rate"), (dict(hop_length=0), "hop_length"), (dict(hop_length=2.0), "hop_length"),
                         (dict(win_length=None), "win_length"), (dict(fmin=0.0), "fmin"), (dict(fmin=500.0), "fmin must not exceed fmax"),
                         (dict(fmax=12000.0), "half the sampling rate"), (dict(n_samples=[4000]), "n_samples"),
                         (dict(n_samples=[4000, 0]), "n_samples"), (dict(bins_per_semitone=0), "bins_per_semitone"),
                         (dict(bins_per_semitone=2.5), "bins_per_semitone"), (dict(beta=2.0), "beta"), (dict(beta=(2.0, 0.0)), "beta"),
                         (dict(beta=(1.0, 2.0, 3.0)), "beta"), (dict(beta=(2.0, float("nan"))), "beta"),
                         (dict(absolute_min_prob=-0.1), "absolute_min_prob"), (dict(absolute_min_prob=1.5), "absolute_min_prob"),
                         (dict(absolute_min_prob=None), "absolute_min_prob")):
            with pytest.raises(ValueError, match=what):
                fn(x, **kw)
        for kw in (dict(win_length=2050), dict(win_length=1023), dict(fmin=21.5), dict(sampling_rate=48000, fmin=40.0)):
            with pytest.raises(NotImplementedError, match="2048.*1022"):
                fn(x, **kw)
        with pytest.raises(NotImplementedError, match="512"):
            fn(x, bins_per_semitone=16)                             # 526 bins over 60 .. 400 Hz
        with pytest.raises(NotImplementedError, match="65535"):
            fn(torch.zeros(65536, 1))
    for kw, what in ((dict(switch_prob=0.0), "switch_prob"), (dict(switch_prob=1.0), "switch_prob"), (dict(switch_prob=None), "switch_prob"),
                     (dict(max_octaves_per_second=0.0), "max_octaves_per_second"), (dict(max_octaves_per_second="fast"), "max_octaves_per_second")):
        with pytest.raises(ValueError, match=what):
            pitch.f0_track(x, **kw)
    assert pitch.MAX_BINS == 512 and pitch.MAX_BAND == 63 and metrics.MAX_LAG == 1022
    with pytest.raises(NotImplementedError, match="63"):
        pitch.f0_track(x, max_octaves_per_second=46.0)              # a band of 64 bins
    with pytest.raises(NotImplementedError, match="63"):
        pitch.f0_track(x, hop_length=512)                           # 100 bins
    # 329 and 279 bins, bands of 43, 50 and 63 fit: refused only for the missing device
    for kw in (dict(), dict(fmin=80.0), dict(sampling_rate=8000, hop_length=80, win_length=256, fmin=80.0), dict(max_octaves_per_second=45.0)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            pitch.f0_track(x, **kw)


def test_library_has_the_new_entries_and_refuses_bad_arguments_before_the_device():
    """FT_EINVAL / FT_EUNSUPPORTED from the entry points themselves, with host memory standing in for the buffers: nothing may
    be launched"""
    import ctypes as C
    from flowtron_amd import _lib as L
    lib = L.lib()
    assert lib.ft_abi_version() == 15
    for name in ("ft_f0_candidates_ragged", "ft_f0_viterbi_ragged", "ft_f0_viterbi_workspace_bytes"):
        assert hasattr(lib, name) and name in L.SIGNATURES
    assert lib.ft_f0_viterbi_workspace_bytes(3, 101, 279) == 3 * 101 * 2 * 279
    assert lib.ft_f0_viterbi_workspace_bytes(0, 101, 279) == 0 and lib.ft_f0_viterbi_workspace_bytes(3, 101, -1) == 0

    buf = (C.c_float * 4096)()
    n = (C.c_int32 * 2)()
    a = C.addressof(buf)
    ok = dict(audio=a, s=(32, 1), n=C.addressof(n), cum=a, edges=a, prob=a, freq=a, voiced=a, B=2, N=32, sr=8000.0, hop=8, W=16, lo=2, hi=10,
              nb=20, amp=0.01)

    def cand(**kw):
        v = dict(ok, **kw)
        return lib.ft_f0_candidates_ragged(v["audio"], *v["s"], v["n"], v["cum"], v["edges"], v["prob"], v["freq"], v["voiced"], v["B"],
                                           v["N"], v["sr"], v["hop"], v["W"], v["lo"], v["hi"], v["nb"], v["amp"], None)
    for kw in (dict(audio=None), dict(n=None), dict(cum=None), dict(edges=None), dict(prob=None), dict(freq=None), dict(voiced=None),
               dict(B=0), dict(N=0), dict(hop=0), dict(W=0), dict(nb=0), dict(s=(-32, 1)), dict(s=(32, -1)), dict(lo=1), dict(lo=11),
               dict(amp=-0.5), dict(amp=1.5), dict(amp=float("nan")), dict(sr=0.0), dict(B=65536)):
        assert cand(**kw) == -1, kw
        assert b"ft_f0_candidates_ragged" in lib.ft_last_error()
    for kw in (dict(W=2050), dict(W=15), dict(hi=1023), dict(nb=513)):
        assert cand(**kw) == -3, kw
        err = lib.ft_last_error()
        assert b"ft_f0_candidates_ragged" in err and b"2048" in err and b"1022" in err and b"512" in err

    okv = dict(prob=a, freq=a, voiced=a, n=C.addressof(n), tri=a, centres=a, f0=a, work=a, bytes=2 * 5 * 40, B=2, N=32, hop=8, nb=20, band=3, sw=0.01)

    def vit(**kw):
        v = dict(okv, **kw)
        return lib.ft_f0_viterbi_ragged(v["prob"], v["freq"], v["voiced"], v["n"], v["tri"], v["centres"], v["f0"], v["work"], v["bytes"],
                                        v["B"], v["N"], v["hop"], v["nb"], v["band"], v["sw"], None)
    for kw in (dict(prob=None), dict(freq=None), dict(voiced=None), dict(n=None), dict(tri=None), dict(centres=None), dict(f0=None),
               dict(work=None), dict(bytes=2 * 5 * 40 - 1), dict(B=0), dict(N=0), dict(hop=0), dict(nb=0), dict(band=-1), dict(sw=0.0),
               dict(sw=1.0), dict(sw=1e-7), dict(sw=float("nan")), dict(B=65536)):
        assert vit(**kw) == -1, kw
        assert b"ft_f0_viterbi_ragged" in lib.ft_last_error()
    for kw in (dict(nb=513, bytes=1 << 20), dict(band=64)):
        assert vit(**kw) == -3, kw
        err = lib.ft_last_error()
        assert b"ft_f0_viterbi_ragged" in err and b"512" in err and b"63" in err
