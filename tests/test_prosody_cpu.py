"""Pitch and pace of audio without a GPU: the NumPy replay of the overlap-add rule (tests/prosody_ref.py) against the rule's
consequences, the accuracy conditions on the pulse-like glide (F0 through tests/pyin_ref.py, fp32, the `small`
configuration, before and after), prosody.pitch_ratio on the host, and the refusals of the Python layer and of the C entries
of csrc/prosody.hip before anything reaches the device.

What the fp32 replay gives (seed 1 / seed 2; the float64 replay's F0 figures differ from these by less than 1e-5 cents):
    input: tracking error 3.81 / 3.84 cents rms, envelope deviation 0.30 / 0.29 dB, log-F0 spread 1.18 semitones
    +4 semitones: gross 0, missed 0 / 1, 5.41 / 5.18 cents, envelope 1.00 / 0.90 dB (resampling 2.52 / 2.50)
    -4 semitones: gross 0, missed 0, 6.41 / 6.26 cents, envelope 1.04 / 1.00 dB (resampling 4.02 / 3.99)
    +7 semitones: gross 0, missed 0, 6.39 / 5.75 cents, envelope 1.03 / 0.93 dB (resampling 3.27 / 3.31)
    -7 semitones: gross 0, missed 0, 7.95 / 6.88 cents, envelope 1.40 / 1.30 dB (resampling 7.53 / 7.62)
    range_scale 0: spread 0.140 / 0.056 semitones, mean moved by 0.03 / 0.03;  range_scale 2: 2.340 / 2.355
    pace 0.8: 9999 samples, gross 0, 5.89 / 6.57 cents over the inner voiced frames;  pace 1.25: 6400 samples, 7.16 / 7.38
    identity (ratio 1, pace 1): max |out - x| = 3.0e-8 at amplitude 0.3"""
import ctypes as C

import numpy as np
import pytest
import torch

import pitch_ref
import prosody_ref as R
import pyin_ref as P
from flowtron_amd import prosody

SR, HOP = 8000.0, 80
_TRACKS = {}


def tracked(seed):
    """the glide, its truth and its fp32 track, once"""
    if seed not in _TRACKS:
        x, truth, voiced = R.pulse_glide(seed)
        _TRACKS[seed] = (x, truth, voiced, P.track(x, P.config("small"), np.float32)["f0"])
    return _TRACKS[seed]


def track(y):
    return P.track(np.asarray(y, np.float32), P.config("small"), np.float32)["f0"]


def flat(n, hz=100.0):
    """a 100 Hz tone and its exact contour: a period of 80 samples"""
    x = (0.3 * np.sin(2 * np.pi * hz * np.arange(n) / SR)).astype(np.float32)
    return x, np.full(n // HOP + 1, hz, np.float32)


# ---- the rule's consequences ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_identity_at_ratio_1_and_pace_1(dtype):
    x, truth, voiced, f0 = tracked(1)
    out, m = R.modify(x, f0, SR, HOP, dtype=dtype)
    assert m["n_out"] == 8000 and out.dtype == dtype and len(out) == 8000
    assert np.array_equal(m["analysis"], m["synthesis"]) and np.array_equal(m["source"], np.arange(len(m["analysis"])))
    worst = float(np.abs(out.astype(np.float64) - x).max())
    print("identity, %s: %d marks, max |out - x| = %.2e" % (np.dtype(dtype).name, len(m["analysis"]), worst))
    assert worst <= 1e-6
    big = (x / np.abs(x).max()).astype(np.float32)                           # the bound is stated for |x| <= 1
    assert float(np.abs(R.modify(big, f0, SR, HOP, dtype=dtype)[0].astype(np.float64) - big).max()) <= 1e-6


def test_mark_counts_on_a_constant_pitch():
    x, f0 = flat(8000)
    m = R.marks(f0, 8000, SR, HOP)
    assert np.array_equal(m["analysis"], np.arange(100) * 80 * 256) and np.all(m["half"] == 80)
    up = R.marks(f0, 8000, SR, HOP, ratio=2.0)
    assert np.array_equal(up["synthesis"], np.arange(200) * 40 * 256) and np.array_equal(up["source"], np.minimum((np.arange(200) + 1) // 2, 99))
    down = R.marks(f0, 8000, SR, HOP, ratio=0.625)
    assert np.array_equal(down["synthesis"], np.arange(63) * 128 * 256) and np.all(down["half"] == 80)
    fast = R.marks(f0, 8000, SR, HOP, pace=1.25)
    assert fast["n_out"] == 6400 and len(fast["synthesis"]) == 80 and np.array_equal(fast["source"], (np.arange(80) * 5 + 2) // 4)
    assert all(v.dtype == np.int32 for k, v in m.items() if k != "n_out")


def test_output_lengths_for_pace():
    x, f0 = flat(8000)
    assert R.marks(f0, 8000, SR, HOP, pace=0.8)["n_out"] == 9999 == prosody.out_samples(8000, 0.8)
    assert R.marks(f0, 8000, SR, HOP, pace=1.25)["n_out"] == 6400 == prosody.out_samples(8000, 1.25)
    assert prosody.pace_q(1.0) == 65536 and prosody.out_samples(1, 4.0) == 1 and prosody.out_samples(8000, 0.25) == 32000
    assert prosody.default_unvoiced_period(22050) == 110 and prosody.default_unvoiced_period(8000) == 40


def test_an_all_unvoiced_utterance_is_reproduced_at_ratio_2():
    x = (0.1 * np.random.RandomState(3).randn(5000)).astype(np.float32)
    f0 = np.zeros(5000 // HOP + 1, np.float32)
    out, m = R.modify(x, f0, SR, HOP, ratio=2.0)
    assert np.array_equal(m["analysis"], np.arange(125) * 40 * 256) and np.array_equal(m["analysis"], m["synthesis"])
    assert float(np.abs(out - x).max()) <= 1e-6
    other, m2 = R.modify(x, f0, SR, HOP, ratio=2.0, unvoiced_period=16)
    assert len(m2["analysis"]) == 313 and float(np.abs(other - x).max()) <= 1e-6


def test_one_sample_gives_one_mark_and_one_grain():
    x = np.array([0.25], np.float32)
    for f in (0.0, 200.0):
        out, m = R.modify(x, np.array([f], np.float32), SR, HOP, ratio=1.5, pace=1.25)
        assert [len(m[k]) for k in ("analysis", "synthesis", "source", "half")] == [1, 1, 1, 1] and m["n_out"] == 1
        assert out.tobytes() == x.tobytes()
    short = R.marks(np.zeros(1, np.float32), 79, SR, HOP)                    # shorter than two periods
    assert len(short["analysis"]) == 2 and len(short["synthesis"]) == 2


def test_extra_frames_are_ignored_and_nan_counts_as_unvoiced():
    x, truth, voiced, f0 = tracked(1)
    want = R.marks(f0, 8000, SR, HOP, ratio=1.3)
    more = np.concatenate([f0, np.array([np.nan, 1e9, -5.0, 333.0], np.float32)])
    got = R.marks(more, 8000, SR, HOP, ratio=1.3)
    assert all(np.array_equal(want[k], got[k]) for k in want)
    holes = f0.copy()
    holes[10:14] = (np.nan, np.inf, -1.0, 0.0)
    zeros = f0.copy()
    zeros[10:14] = 0.0
    a, b = R.marks(holes, 8000, SR, HOP, ratio=1.3), R.marks(zeros, 8000, SR, HOP, ratio=1.3)
    assert all(np.array_equal(a[k], b[k]) for k in a) and not np.array_equal(a["analysis"], want["analysis"])


def test_ratios_outside_the_range_clamp_and_periods_too():
    x, f0 = flat(4000)
    same = lambda a, b: all(np.array_equal(a[k], b[k]) for k in a)
    assert same(R.marks(f0, 4000, SR, HOP, ratio=5.0), R.marks(f0, 4000, SR, HOP, ratio=2.0))
    assert same(R.marks(f0, 4000, SR, HOP, ratio=0.1), R.marks(f0, 4000, SR, HOP, ratio=0.625))
    assert same(R.marks(f0, 4000, SR, HOP, ratio=float("nan")), R.marks(f0, 4000, SR, HOP, ratio=0.625))
    assert not same(R.marks(f0, 4000, SR, HOP, ratio=1.9), R.marks(f0, 4000, SR, HOP, ratio=2.0))
    high = R.marks(np.full(51, 4000.0, np.float32), 4000, SR, HOP)           # a period of 2 samples: held at 16
    assert np.all(np.diff(high["analysis"]) == 16 * 256)
    low = R.marks(np.full(51, 1.0, np.float32), 4000, SR, HOP)               # 8000 samples: held at 1024
    assert np.all(np.diff(low["analysis"]) == 1024 * 256) and np.all(low["half"] == 1024)


def test_reciprocal_quotient_equals_the_integer_quotient():
    """csrc/prosody.hip forms (|d| 1024) / half as int(float(|d| 1024) * (1.f / half)) and one correction: every |d| < half <= 1024"""
    for h in range(1, 1025):
        num = np.arange(h, dtype=np.int64) * 1024
        rcp = np.float32(1.0) / np.float32(h)
        q = (num.astype(np.float32) * rcp).astype(np.float32).astype(np.int64)
        q = q + ((q + 1) * h <= num)
        assert np.array_equal(q, num // h), h


# ---- the accuracy conditions ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("semitones,seed", [(4, 1), (-4, 1), (7, 1), (-7, 1), (7, 2), (-7, 2)])
def test_shifted_glide_keeps_its_contour_and_its_envelope(semitones, seed):
    x, truth, voiced, f0 = tracked(seed)
    r = 2.0 ** (semitones / 12.0)
    out, _ = R.modify(x, f0, SR, HOP, ratio=r)
    got = P.score(track(out), truth * r, voiced)
    dev = R.envelope_deviation(out, truth * r, voiced)
    y, fy, vy = R.resample_shift(x, r)
    base = R.envelope_deviation(y, fy, vy)
    print("%+d semitones, seed %d: %s, envelope %.2f dB (resampling %.2f dB)" % (semitones, seed, got, dev, base))
    assert got["gross"] == 0, got
    assert got["missed"] <= 3, got
    assert got["rms"] <= 15.0, got
    assert dev <= 2.2
    if abs(semitones) == 7:
        assert dev < 0.6 * base, (dev, base)


@pytest.mark.parametrize("seed", [1, 2])
def test_range_scale_flattens_and_widens_the_intonation(seed):
    x, truth, voiced, f0 = tracked(seed)
    _, mean_in, std_in = pitch_ref.statistics(f0)
    for scale in (0.0, 2.0):
        ratio = prosody.pitch_ratio(torch.from_numpy(f0), range_scale=scale).numpy()
        assert ratio.dtype == np.float32 and np.all(ratio[f0 == 0] == 1)
        assert np.allclose(ratio, R.pitch_ratio(f0, 0.0, scale), rtol=3e-7, atol=0)
        out, _ = R.modify(x, f0, SR, HOP, ratio=ratio)
        _, mean, std = pitch_ref.statistics(track(out))
        print("seed %d, range_scale %g: spread %.3f semitones (input %.3f), mean moved by %.3f" % (seed, scale, std, std_in, mean - mean_in))
        if scale == 0.0:
            assert std < 0.3 and abs(mean - mean_in) <= 0.2
        else:
            assert 2.0 <= std <= 2.7


@pytest.mark.parametrize("pace,n_out", [(0.8, 9999), (1.25, 6400)])
@pytest.mark.parametrize("seed", [1, 2])
def test_pace_keeps_the_pitch(seed, pace, n_out):
    x, truth, voiced, f0 = tracked(seed)
    out, m = R.modify(x, f0, SR, HOP, pace=pace)
    assert len(out) == n_out == m["n_out"]
    f_true, v_true = R.mapped_truth(n_out, pace)
    got = P.score(track(out), f_true, R.inner(v_true))
    print("pace %g, seed %d: %d samples, %s" % (pace, seed, n_out, got))
    assert got["gross"] == 0 and got["found"] >= 40, got
    assert got["rms"] <= 15.0, got


def test_pitch_ratio_on_the_host():
    f0 = torch.tensor([[100.0, 0.0, 200.0, 400.0], [0.0, 0.0, 0.0, 0.0]])
    r = prosody.pitch_ratio(f0, shift_semitones=12.0)
    assert torch.allclose(r, torch.tensor([[2.0, 1.0, 2.0, 2.0], [1.0] * 4])) and r.dtype == torch.float32
    flat_ = prosody.pitch_ratio(f0, range_scale=0.0)
    assert torch.allclose(flat_[0] * f0[0], torch.tensor([200.0, 0.0, 200.0, 200.0])) and torch.equal(flat_[1], torch.ones(4))
    assert torch.equal(prosody.pitch_ratio(f0, lens=[2, 4], shift_semitones=3.0)[0, 2:], torch.ones(2))   # frames behind the length
    assert tuple(prosody.pitch_ratio(f0[0], range_scale=2.0).shape) == (4,)
    for kw in (dict(shift_semitones=float("nan")), dict(range_scale=None), dict(lens=[4])):
        with pytest.raises(ValueError):
            prosody.pitch_ratio(f0, **kw)
    with pytest.raises(ValueError, match="f0"):
        prosody.pitch_ratio([100.0, 0.0])


# ---- refusals --------------------------------------------------------------------------------------------------------------------

def test_refusals_are_raised_without_a_device():
    x, f0 = torch.zeros(2, 8000), torch.zeros(2, 101)
    for f in (prosody.modify, prosody.marks):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            f(x, None, f0, 8000, 80)
        for bad in (x.double(), x[None], torch.zeros(2, 0), [0.0] * 10):
            with pytest.raises(ValueError, match="audio"):
                f(bad, None, f0, 8000, 80)
        for bad in (f0.double(), f0[0], f0[:1], torch.zeros(2, 101, 1), [0.0] * 101):
            with pytest.raises(ValueError, match="f0"):
                f(x, None, bad, 8000, 80)
        with pytest.raises(ValueError, match="f0"):
            f(x[0], None, f0, 8000, 80)                                      # [N] takes [T]
        with pytest.raises(ValueError, match="101 frames"):
            f(x, None, f0[:, :100], 8000, 80)
        for ns in ([8000], [8000, 8001], [8000, 0], torch.tensor([8000.0, 1.0])):
            with pytest.raises(ValueError, match="n_samples"):
                f(x, ns, f0, 8000, 80)
        for kw, what in ((dict(pace=0.2), "pace"), (dict(pace=4.5), "pace"), (dict(pace=float("nan")), "pace"), (dict(pace=[1.0]), "pace"),
                         (dict(pace=[1.0, 5.0]), "pace"), (dict(pace=None), "pace"), (dict(hop_length=0), "hop_length"),
                         (dict(hop_length=80.0), "hop_length"), (dict(sampling_rate=0), "sampling_rate"),
                         (dict(sampling_rate=None), "sampling_rate"), (dict(pitch_ratio=float("inf")), "pitch_ratio"),
                         (dict(pitch_ratio=None), "pitch_ratio"), (dict(pitch_ratio=torch.ones(3)), "pitch_ratio"),
                         (dict(pitch_ratio=torch.ones(2, 100)), "pitch_ratio"), (dict(pitch_ratio=torch.ones(2, 101).double()), "pitch_ratio"),
                         (dict(unvoiced_period=40.0), "unvoiced_period")):
            with pytest.raises(ValueError, match=what):
                f(x, None, f0, **dict(dict(sampling_rate=8000, hop_length=80), **kw))
        for period in (15, 1025):
            with pytest.raises(NotImplementedError, match="unvoiced_period"):
                f(x, None, f0, 8000, 80, unvoiced_period=period)
        with pytest.raises(NotImplementedError, match="unvoiced_period"):
            f(x, None, f0, 2000, 80)                                         # the default, 5 ms, is 10 samples there
        with pytest.raises(NotImplementedError, match="65535"):
            f(torch.zeros(65536, 1), None, torch.zeros(65536, 1), 8000, 80)
        big = torch.zeros(1, (1 << 22) + 1)
        with pytest.raises(NotImplementedError, match="MAX_SAMPLES"):
            f(big, None, torch.zeros(1, big.shape[1] // 4096 + 1), 8000, 4096)
        with pytest.raises(NotImplementedError, match="N_out = 4194308"):
            f(big[:, :(1 << 20) + 1], None, torch.zeros(1, 257), 8000, 4096, pace=0.25)


def test_c_abi_refuses_bad_arguments_before_the_device():
    """FT_EINVAL / FT_EUNSUPPORTED from the entry points themselves, with host memory standing in for the buffers: nothing may
    be launched"""
    from flowtron_amd import _lib as L
    lib = L.lib()
    B, N, T, hop = 2, 1024, 13, 80
    KA, KS = 64, 128
    f32 = [(C.c_float * (B * N))() for _ in range(5)]
    i32 = [(C.c_int32 * (B * KS))() for _ in range(13)]
    adr = C.addressof
    okm = dict(f0=adr(f32[0]), fs=(T, 1), ratio=adr(f32[1]), rs=(0, 0), n=adr(i32[0]), pq=adr(i32[1]), a=adr(i32[2]), na=adr(i32[3]),
               s=adr(i32[4]), src=adr(i32[5]), half=adr(i32[6]), ns=adr(i32[7]), no=adr(i32[8]), B=B, N=N, N_out=N, T=T, hop=hop, KA=KA,
               KS=KS, sr256=2048000.0, unv=40)

    def marks(**kw):
        a = dict(okm, **kw)
        return lib.ft_psola_marks(a["f0"], *a["fs"], a["ratio"], *a["rs"], a["n"], a["pq"], a["a"], a["na"], a["s"], a["src"], a["half"],
                                  a["ns"], a["no"], a["B"], a["N"], a["N_out"], a["T"], a["hop"], a["KA"], a["KS"], a["sr256"], a["unv"],
                                  None)
    for kw in (dict(f0=None), dict(ratio=None), dict(n=None), dict(pq=None), dict(a=None), dict(na=None), dict(s=None), dict(src=None),
               dict(half=None), dict(ns=None), dict(no=None), dict(B=0), dict(B=65536), dict(N=0), dict(N_out=0), dict(T=0), dict(T=12),
               dict(hop=0), dict(fs=(-T, 1)), dict(fs=(T, -1)), dict(rs=(-1, 0)), dict(rs=(0, -1)), dict(KA=63), dict(KS=127),
               dict(sr256=0.0), dict(sr256=float("nan")), dict(sr256=float("inf"))):
        assert marks(**kw) == -1, kw
        assert b"ft_psola_marks" in lib.ft_last_error()
    for kw, what in ((dict(unv=15), b"16 .. 1024"), (dict(unv=1025), b"16 .. 1024"), (dict(N=(1 << 22) + 1), b"4194304"),
                     (dict(N_out=(1 << 22) + 1), b"4194304")):
        assert marks(**kw) == -3, kw
        assert b"ft_psola_marks" in lib.ft_last_error() and what in lib.ft_last_error()

    oks = dict(audio=adr(f32[2]), s=(N, 1), n=adr(i32[0]), a=adr(i32[2]), sm=adr(i32[4]), src=adr(i32[5]), half=adr(i32[6]), ns=adr(i32[7]),
               no=adr(i32[8]), hann=adr(f32[3]), out=adr(f32[4]), B=B, N=N, N_out=N, KA=KA, KS=KS)

    def synth(**kw):
        a = dict(oks, **kw)
        return lib.ft_psola_synth(a["audio"], *a["s"], a["n"], a["a"], a["sm"], a["src"], a["half"], a["ns"], a["no"], a["hann"], a["out"],
                                  a["B"], a["N"], a["N_out"], a["KA"], a["KS"], None)
    for kw in (dict(audio=None), dict(n=None), dict(a=None), dict(sm=None), dict(src=None), dict(half=None), dict(ns=None), dict(no=None),
               dict(hann=None), dict(out=None), dict(B=0), dict(B=65536), dict(N=0), dict(N_out=0), dict(KA=0), dict(KS=0),
               dict(s=(-N, 1)), dict(s=(N, -1))):
        assert synth(**kw) == -1, kw
        assert b"ft_psola_synth" in lib.ft_last_error()
    for kw in (dict(N=(1 << 22) + 1), dict(N_out=(1 << 22) + 1)):
        assert synth(**kw) == -3, kw
        assert b"ft_psola_synth" in lib.ft_last_error() and b"4194304" in lib.ft_last_error()
