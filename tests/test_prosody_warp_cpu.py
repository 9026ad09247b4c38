"""A pace that varies within the utterance, without a GPU: the NumPy replay of the time-map rules (tests/prosody_warp_ref.py)
against the constant-pace rule it must equal bit for bit (tests/prosody_ref.py at paces 1, 2 and 0.5: a yardstick that is not
its own replay), against the rule's consequences, and on a signal with known truth -- one "sentence" said twice, the second
time with another rhythm and another melody, the first made to follow the second through log-power DTW (tests/dtw_ref.py),
the time map, transfer_ratio on the output's axis and the warp; F0 through tests/pyin_ref.py (`small`, fp32).  Then
prosody.time_map_from_durations and prosody.transfer_ratio on the host against their restatements, and the refusals of the
Python layer and of the two C entries before anything reaches the device.

What the fp32 replay gives on the transfer signal (smooth = 0 / 4 / 8):
    the reference's own tracking error 2.69 cents rms over its inner voiced frames
    transferred: gross 0, missed 0, 7.15 / 7.70 / 7.23 cents against the reference's TRUE contour
    uniformly paced, untransferred: 275.9 cents, every frame gross
    map against the constructed truth: 1.25 / 0.96 / 0.95 frames rms
    log-power contour against the reference's: 0.38 / 0.31 / 0.34 rms; uniformly paced: 1.88
    the glide of prosody_ref along a known smooth map, ratio 1: gross 0, 6.34 cents, envelope deviation 1.16 dB"""
import ctypes as C

import numpy as np
import pytest
import torch

import dtw_ref as D
import prosody_ref as R
import prosody_warp_ref as W
import pyin_ref as P
from flowtron_amd import prosody

SR, HOP, Q = 8000.0, 80, 256
_CACHE = {}


def tracked():
    """the glide of prosody_ref (seed 1) and its fp32 track, once"""
    if "glide" not in _CACHE:
        x, truth, voiced = R.pulse_glide(1)
        _CACHE["glide"] = (x, P.track(x, P.config("small"), np.float32)["f0"])
    return _CACHE["glide"]


def track(y):
    return P.track(np.asarray(y, np.float32), P.config("small"), np.float32)["f0"]


def same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


def identity_map(entries, hop=HOP):
    return W.constant_map(1, hop, entries)


# ---- constant maps are the existing rule ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("pace,grains", [(1, 189), (2, 95), (0.5, 377)])
def test_constant_map_equals_the_constant_pace_rule_bit_for_bit(pace, grains):
    x, f0 = tracked()
    n_out = max(1, (8000 << 16) // prosody.pace_q(pace))
    want_out, want = R.modify(x, f0, SR, HOP, 1.19, pace)
    got_out, got = W.warp(x, f0, SR, HOP, W.constant_map(pace, HOP, n_out // HOP + 2), n_out, 1.19, 0)
    print("pace %g: %d grains, %d samples" % (pace, len(got["synthesis"]), got["n_out"]))
    assert len(want["synthesis"]) == grains and same(want, got) and got["n_out"] == n_out == want["n_out"]
    assert got_out.tobytes() == want_out.tobytes()
    per_frame = np.full(len(f0), 1.19, np.float32)                           # a per-frame ratio on the input's axis is the same thing
    assert same(want, W.marks_warp(f0, 8000, SR, HOP, W.constant_map(pace, HOP, n_out // HOP + 2), n_out, per_frame, 0))


def test_output_hop_need_not_be_the_input_hop():
    x, f0 = tracked()
    want = R.marks(f0, 8000, SR, HOP, 1.19, 1.0)
    for hop_out in (64, 1, 8000, 9000):
        got = W.marks_warp(f0, 8000, SR, HOP, identity_map(8000 // hop_out + 2, hop_out), 8000, 1.19, 0, hop_out=hop_out)
        assert same(want, got), hop_out
    on_output = W.marks_warp(f0, 8000, SR, HOP, identity_map(127, 64), 8000, 1.0, 1, hop_out=64)      # ratio 1: the axis does not matter
    assert same(R.marks(f0, 8000, SR, HOP), on_output)


# ---- the rule's consequences -----------------------------------------------------------------------------------------------------

def frozen_map():
    """identity, held still for 20 output frames from frame 20: 8000 samples become 9600; 122 entries"""
    u = np.arange(122)
    return np.where(u < 20, u, np.where(u < 40, 20, u - 20)).astype(np.int64) * HOP * Q


def test_a_frozen_map_repeats_source_grains_and_still_ends():
    x, f0 = tracked()
    m = W.marks_warp(f0, 8000, SR, HOP, frozen_map(), 9600, 1.0, 0)
    s, src = m["synthesis"] >> 8, m["source"]
    held = (s >= 21 * HOP) & (s < 40 * HOP)
    print("frozen for 20 frames: %d grains for %d samples, %d of them while the map stands still, all from source grain %s"
          % (len(s), m["n_out"], held.sum(), np.unique(src[held])))
    assert m["n_out"] == 9600 and held.sum() >= 15 and len(np.unique(src[held])) == 1
    assert np.all(np.diff(src) >= 0) and np.all(np.diff(m["synthesis"]) >= 8 * Q) and (s[-1] < 9600)
    assert src[-1] >= len(m["analysis"]) - 2                                 # and the walk reaches the input's end afterwards
    still = W.marks_warp(f0, 8000, SR, HOP, np.zeros(122, np.int64), 9600, 1.0, 0)       # a map that never moves: one grain, over and over
    assert np.all(still["source"] == 0) and (still["synthesis"][-1] >> 8) < 9600 and len(still["synthesis"]) > 100


def test_a_decreasing_stretch_acts_as_its_running_maximum():
    x, f0 = tracked()
    u = np.arange(102)
    dip = (u * HOP * Q).astype(np.int64)
    dip[31:36] = dip[30] - np.array([5, 9, 6, 3, 0]) * HOP * Q               # back by up to 9 frames, then up to where it was
    held = np.maximum.accumulate(dip)
    assert not np.array_equal(dip, held)
    a, b = W.marks_warp(f0, 8000, SR, HOP, dip, 8000, 1.19, 0), W.marks_warp(f0, 8000, SR, HOP, held, 8000, 1.19, 0)
    assert same(a, b) and np.all(np.diff(a["source"]) >= 0)
    wild = np.random.RandomState(5).randint(-2 ** 31, 2 ** 31 - 1, size=102, dtype=np.int64)          # whatever the map holds
    m = W.marks_warp(f0, 8000, SR, HOP, wild, 8000, 1.19, 0)
    assert np.all(np.diff(m["source"]) >= 0) and m["source"].max() < len(m["analysis"]) and (m["synthesis"][-1] >> 8) < 8000


def test_a_slope_of_six_skips_grains():
    x, f0 = tracked()
    u = np.arange(27)
    fast = np.minimum(u * 6, 100).astype(np.int64) * HOP * Q
    m = W.marks_warp(f0, 8000, SR, HOP, fast, 2000, 1.0, 0)
    moving = (m["synthesis"] >> 8) < 16 * HOP
    jumps = np.diff(m["source"][moving])
    print("slope 6: %d grains, source steps %s" % (len(m["source"]), np.unique(jumps)))
    assert m["n_out"] == 2000 and jumps.min() >= 3 and jumps.max() <= 9
    assert m["source"][-1] == len(m["analysis"]) - 1                         # behind the input's end the last grain repeats


def test_one_sample_and_less_than_two_periods():
    one = np.array([0.25], np.float32)
    for f in (0.0, 200.0):
        out, m = W.warp(one, np.array([f], np.float32), SR, HOP, [0, 7 * Q], 1, 1.5, 0)
        assert [len(m[k]) for k in ("analysis", "synthesis", "source", "half")] == [1, 1, 1, 1] and m["n_out"] == 1
        assert out.tobytes() == one.tobytes()
    long_ = W.marks_warp(np.array([0.0], np.float32), 1, SR, HOP, np.zeros(4, np.int64), 200, 1.0, 0)  # one sample played for 200
    assert len(long_["analysis"]) == 1 and np.all(long_["source"] == 0) and len(long_["synthesis"]) == 5
    short = W.marks_warp(np.zeros(1, np.float32), 79, SR, HOP, identity_map(2), 79, 1.0, 0)
    assert same(short, R.marks(np.zeros(1, np.float32), 79, SR, HOP))


def test_n_out_is_clamped():
    x, f0 = tracked()
    tm = identity_map(102)
    assert W.marks_warp(f0, 8000, SR, HOP, tm, 0, 1.0, 0, N_out=8000)["n_out"] == 1
    assert W.marks_warp(f0, 8000, SR, HOP, tm, -5, 1.0, 0, N_out=8000)["n_out"] == 1
    big = W.marks_warp(f0, 8000, SR, HOP, tm, 2 ** 31 - 1, 1.0, 0, N_out=8000)
    assert big["n_out"] == 8000 and same(big, W.marks_warp(f0, 8000, SR, HOP, tm, 8000, 1.0, 0))


def test_nan_and_wild_ratios_count_as_clamped_on_either_axis():
    x, f0 = tracked()
    tm = identity_map(102)
    for axis, T in ((0, len(f0)), (1, 101)):
        r = np.full(T, 1.3, np.float32)
        bad, lim = r.copy(), r.copy()
        bad[10:14], lim[10:14] = (np.nan, -np.inf, np.inf, 0.1), (0.625, 0.625, 2.0, 0.625)
        a, b = W.marks_warp(f0, 8000, SR, HOP, tm, 8000, bad, axis), W.marks_warp(f0, 8000, SR, HOP, tm, 8000, lim, axis)
        assert same(a, b) and not same(a, W.marks_warp(f0, 8000, SR, HOP, tm, 8000, r, axis))


def test_the_output_axis_reads_the_ratio_where_the_mark_lies():
    """a map at pace 0.5 and a ratio that steps from 1 to 1.5 at output frame 100, which plays input frame 50"""
    x, f0 = tracked()
    r_out = np.where(np.arange(201) < 100, 1.0, 1.5).astype(np.float32)
    r_in = np.where(np.arange(101) < 50, 1.0, 1.5).astype(np.float32)
    tm = W.constant_map(0.5, HOP, 202)
    a, b = W.marks_warp(f0, 8000, SR, HOP, tm, 16000, r_out, 1), W.marks_warp(f0, 8000, SR, HOP, tm, 16000, r_in, 0)
    s = a["synthesis"].astype(np.int64)
    before = int(((s >> 8) < 7900).sum())                                    # the two axes' frame edges lie at 7920 and 7960
    assert np.array_equal(a["synthesis"][:before], b["synthesis"][:before]) and np.array_equal(a["source"][:before], b["source"][:before])
    per = R._periods(f0, 1.0, SR, 40, np.float32)[0]
    frame = np.minimum(100, (((s >> 1) >> 8) + HOP // 2) // HOP)[:-1]         # frame(ta), ta = s / 2
    rel, voiced, at = np.diff(s) / per[frame], f0[frame] > 0, s[:-1] >> 8
    assert (voiced & (at < 7900)).sum() > 50 and (voiced & (at >= 8000)).sum() > 50
    assert np.allclose(rel[voiced & (at < 7900)], 1.0, atol=1e-3) and np.allclose(rel[voiced & (at >= 8000)], 1 / 1.5, atol=1e-3)
    assert np.all(np.diff(s)[~voiced] == 40 * Q)                              # unvoiced frames are never shifted


def test_reciprocal_quotient_of_the_interpolation_equals_the_integer_quotient():
    """csrc/prosody.hip forms ((tmap[u + 1] - tmap[u]) fr) / (hop_out Q) as int64(double(|d fr|) * (1.0 / den)) and one correction
    by the remainder: any difference of two int32, any fr < den, the largest and some awkward hops"""
    rng = np.random.RandomState(9)
    for hop_out in (1, 2, 3, 64, 80, 255, 256, 257, 4095, 1 << 22):
        den = hop_out * Q
        inv = np.float64(1.0) / np.float64(den)
        k = rng.randint(0, 2 ** 32 // den + 1, size=20000).astype(np.int64)
        d = np.concatenate([rng.randint(-2 ** 32 + 1, 2 ** 32, size=100000), k * den - 1, k * den, k * den + 1,
                            [2 ** 32 - 1, -(2 ** 32 - 1), 1, -1, 0]]).astype(np.int64)
        d = np.clip(d, -(2 ** 32 - 1), 2 ** 32 - 1)
        fr = rng.randint(0, den, size=len(d)).astype(np.int64)
        fr[100000:] = den - 1
        mag = np.abs(d * fr)
        q = (mag.astype(np.float64) * inv).astype(np.int64)
        r = mag - q * den
        q = q + np.where(r >= den, 1, np.where(r < 0, -1, 0))
        assert np.array_equal(q, mag // den), hop_out


# ---- a path to a map ---------------------------------------------------------------------------------------------------------------

def test_time_map_of_a_path():
    stairs = np.array([(0, 0), (1, 0), (2, 0), (3, 1), (3, 2), (3, 3), (4, 4)], np.int32)
    tm = W.time_map_from_path(stairs, 7, HOP, 7, 0)
    assert tm.dtype == np.int32 and tm.tolist() == [128 * HOP * v for v in (2, 6, 6, 6, 8, 8, 8)]     # the middle of 0 .. 2, then 3, 3, 3, 4
    smooth = W.time_map_from_path(stairs, 7, HOP, 7, 1)
    assert smooth.tolist() == [(128 * HOP * v) // 3 for v in (10, 14, 18, 20, 22, 24, 24)]
    assert W.time_map_from_path(stairs, 3, HOP, 3, 4).tolist() == [128 * HOP * 2] * 3                 # path_len: three cells, one frame
    assert np.array_equal(W.time_map_from_path(stairs, 0, HOP, 2, 0), W.time_map_from_path(stairs, 1, HOP, 2, 0))
    assert np.array_equal(W.time_map_from_path(stairs, 99, HOP, 9, 2), W.time_map_from_path(stairs, 7, HOP, 9, 2))
    for Ta, Tb in ((1, 1), (1, 7), (7, 1), (63, 65), (65, 63)):
        x, y = D.pair("normal", Ta, Tb, 3)
        path = D.replay(x, y)[1]
        for w in (0, 4, 32):
            tm = W.time_map_from_path(path, len(path), HOP, Tb + 1, w).astype(np.int64)
            assert np.all(np.diff(tm) >= 0) and tm[0] >= 0 and tm[-1] <= (Ta - 1) * HOP * Q, (Ta, Tb, w)
    wild = np.random.RandomState(2).randint(-2 ** 31, 2 ** 31 - 1, size=(40, 2)).astype(np.int32)     # any cells: in range, no more
    tm = W.time_map_from_path(wild, 40, HOP, 50, 3).astype(np.int64)
    assert tm.min() >= 0 and tm.max() <= Q * ((1 << 22) - 1)


# ---- durations to a map ------------------------------------------------------------------------------------------------------------

def test_time_map_from_durations_hits_every_token_boundary():
    src = torch.tensor([[3, 5, 0, 4, 2], [2, 2, 2, 9, 9]])
    tgt = torch.tensor([[6, 5, 3, 0, 1], [1, 4, 2, 9, 9]])
    tmap, frames = prosody.time_map_from_durations(src, tgt, [5, 3], HOP)
    assert tmap.dtype == torch.int32 and frames.dtype == torch.int32 and frames.tolist() == [15, 7] and tuple(tmap.shape) == (2, 17)
    qh = Q * HOP
    for b, L in enumerate((5, 3)):
        want, total = W.time_map_from_durations(src[b, :L].tolist(), tgt[b, :L].tolist(), HOP, 17)
        assert total == int(frames[b]) and np.array_equal(tmap[b].numpy(), want), b
    t0 = tmap[0].tolist()
    assert [t0[e] for e in (0, 6, 11, 14, 15, 16)] == [qh * s for s in (0, 3, 8, 12, 14, 14)]          # E_l -> S_l; token 3 (no target frames) is skipped
    assert t0[3] == qh * 3 // 2 and t0[12] == t0[11] == qh * 8                                        # a token with no source frames holds still
    assert tmap[1].tolist()[7:] == [qh * 6] * 10                              # tokens behind in_lens count for nothing
    wide, _ = prosody.time_map_from_durations(src, tgt, [5, 3], HOP, n_frames=30)
    assert tuple(wide.shape) == (2, 32) and torch.equal(wide[:, :17], tmap) and wide[0, 17:].tolist() == [qh * 14] * 15
    same_, n = prosody.time_map_from_durations(src, src, None, HOP)          # unchanged durations: the identity
    assert same_[0, :15].tolist() == [qh * u for u in range(15)] and n.tolist() == [14, 24]
    for bad in (dict(src_durations=src.float()), dict(tgt_durations=tgt[:, :4]), dict(in_lens=[5]), dict(hop_length=0), dict(src_durations=[1, 2])):
        with pytest.raises(ValueError):
            prosody.time_map_from_durations(**dict(dict(src_durations=src, tgt_durations=tgt, in_lens=[5, 3], hop_length=HOP), **bad))


def test_durations_drive_the_walk_to_the_token_boundaries():
    """emphasis: the second quarter of the glide at half speed; what plays at an output boundary is the input boundary"""
    x, f0 = tracked()
    src = torch.tensor([[25, 25, 50]])
    tmap, frames = prosody.time_map_from_durations(src, torch.tensor([[25, 50, 50]]), None, HOP)
    m = W.marks_warp(f0, 8000, SR, HOP, tmap[0].numpy(), int(frames[0]) * HOP, 1.0, 0)
    a, s = m["analysis"][m["source"]] >> 8, m["synthesis"] >> 8
    assert m["n_out"] == 10000
    for out_at, in_at in ((25 * HOP, 25 * HOP), (50 * HOP, 37 * HOP + 40), (75 * HOP, 50 * HOP), (110 * HOP, 85 * HOP)):
        j = int(np.argmin(np.abs(s - out_at)))
        assert abs((a[j] - in_at) - (s[j] - out_at) * (0.5 if 25 * HOP <= out_at < 75 * HOP else 1.0)) <= 60, (out_at, a[j], s[j])


# ---- the ratio of a transfer --------------------------------------------------------------------------------------------------------

def test_transfer_ratio_is_one_wherever_either_side_is_unvoiced():
    f_src = torch.tensor([[100.0, 0.0, 200.0, 400.0, float("nan")], [0.0, 0.0, 0.0, 0.0, 0.0]])
    f_ref = torch.tensor([[150.0, 150.0, 0.0, 300.0, 300.0, float("inf"), 300.0], [150.0] * 7])
    tmap = torch.tensor([[0, 1, 2, 2, 3, 4, 4, 4]] * 2, dtype=torch.int32) * (HOP * Q)
    r = prosody.transfer_ratio(f_src, f_ref, tmap, HOP)
    assert r.dtype == torch.float32 and tuple(r.shape) == (2, 7)
    assert r[0].tolist() == [1.5, 1.0, 1.0, 1.5, 0.75, 1.0, 1.0] and torch.equal(r[1], torch.ones(7))
    for b in (0, 1):
        assert r[b].numpy().tobytes() == W.transfer_ratio(f_src[b].numpy(), f_ref[b].numpy(), tmap[b].numpy(), HOP).tobytes()
    own = prosody.transfer_ratio(f_src, f_ref, tmap, HOP, register="source")
    assert torch.equal(own == 1, r == 1)                                    # the register moves the voiced frames only
    c = 2.0 ** (np.log2([100.0, 200.0, 400.0]).mean() - np.log2([150.0, 150.0, 300.0, 300.0, 300.0]).mean())   # voiced mean onto voiced mean
    assert np.allclose((own[0] / r[0])[[0, 3, 4]].numpy(), c, rtol=1e-6, atol=0)
    assert np.allclose(own[0].numpy(), W.transfer_ratio(f_src[0].numpy(), f_ref[0].numpy(), tmap[0].numpy(), HOP, "source"), rtol=3e-7, atol=0)
    cut = prosody.transfer_ratio(f_src, f_ref, tmap, HOP, src_lens=[3, 5], ref_lens=[4, 7])
    assert cut[0].tolist() == [1.5, 1.0, 1.0, 1.5, 1.0, 1.0, 1.0]
    half = prosody.transfer_ratio(f_src[0], f_ref[0], tmap[0] + 40 * Q, HOP)          # half a frame on: the next source frame
    assert tuple(half.shape) == (7,) and half.tolist()[:2] == [1.0, 0.75]
    for kw in (dict(register="mine"), dict(hop_length=0), dict(time_map=tmap[:, :6]), dict(time_map=tmap.long()), dict(f0_ref=f_ref[0]),
               dict(f0_src=[1.0]), dict(src_lens=[3]), dict(f0_ref=f_ref[:1])):
        with pytest.raises(ValueError):
            prosody.transfer_ratio(**dict(dict(f0_src=f_src, f0_ref=f_ref, time_map=tmap, hop_length=HOP), **kw))


# ---- transfer on a signal with known truth -----------------------------------------------------------------------------------------

def transfer_case():
    """the two signals' tracks, the DTW path of their log-power contours and the uniformly paced baseline, once"""
    if "transfer" not in _CACHE:
        S = W.transfer_signal()
        f_src, f_ref = track(S["src"]), track(S["ref"])
        path = D.replay(W.log_power(S["src"]), W.log_power(S["ref"]))[1]
        uniform = R.modify(S["src"], f_src, SR, HOP, 1.0, W.N_SRC / W.N_REF)[0]
        _CACHE["transfer"] = dict(S, f_src=f_src, f_ref=f_ref, path=path, uniform=uniform, lp_ref=W.log_power(S["ref"]))
    return _CACHE["transfer"]


def rms(v):
    return float(np.sqrt(np.mean(np.asarray(v, np.float64) ** 2)))


def test_the_transfer_signal_is_what_the_figures_are_about():
    c = transfer_case()
    assert len(c["src"]) == 8000 and len(c["ref"]) == 9600 and len(c["uniform"]) == 9600 and len(c["truth"]) == 121
    own = P.score(c["f_ref"], c["truth"], R.inner(c["voiced"]))
    base = P.score(track(c["uniform"]), c["truth"], R.inner(c["voiced"]))
    base_lp = rms(W.log_power(c["uniform"]) - c["lp_ref"])
    print("the reference's own tracking error: %s" % own)
    print("uniformly paced, untransferred: %s; log-power contour %.3f rms" % (base, base_lp))
    assert own["gross"] == 0 and own["missed"] == 0 and own["rms"] <= 5.0 and own["found"] >= 60
    assert base["gross"] >= 0.9 * base["found"] and base["rms"] > 200.0      # the parent's capability: the right length, the wrong melody
    assert np.all(np.diff(c["true_map"]) > 0)


@pytest.mark.parametrize("smooth", [0, 4, 8])
def test_transfer_follows_the_reference_in_melody_and_rhythm(smooth):
    c = transfer_case()
    tm = W.time_map_from_path(c["path"], len(c["path"]), HOP, 122, smooth)
    ratio = W.transfer_ratio(c["f_src"], c["f_ref"], tm, HOP)
    out, m = W.warp(c["src"], c["f_src"], SR, HOP, tm, W.N_REF, ratio, 1)
    got = P.score(track(out), c["truth"], R.inner(c["voiced"]))
    map_err = rms((tm[:121] / 256.0 - c["true_map"]) / HOP)
    lp, base_lp = rms(W.log_power(out) - c["lp_ref"]), rms(W.log_power(c["uniform"]) - c["lp_ref"])
    print("smooth %d: %d grains, %s; map %.2f frames rms; log-power contour %.3f rms against the reference's (uniform pace: %.3f)"
          % (smooth, len(m["synthesis"]), got, map_err, lp, base_lp))
    assert len(out) == W.N_REF == m["n_out"]
    assert got["gross"] == 0, got
    assert got["rms"] <= 15.0, got                                           # what test_prosody_cpu.py asserts for a constant shift
    assert lp < 0.5 * base_lp, (lp, base_lp)
    _CACHE[("transfer", smooth)] = dict(tmap=tm, ratio=ratio, out=out, marks=m, score=got)


def test_known_smooth_map_keeps_the_envelope():
    """the glide of prosody_ref along a smooth map of its own (slope 0.75 .. 1.25), ratio 1: the harmonics stay on the envelope"""
    x, f0 = tracked()
    u = np.arange(102)
    pos = 8000.0 * (u / 100.0 + 0.04 * np.sin(2 * np.pi * u / 100.0))
    tm = np.rint(np.minimum(pos, 8000.0) * Q).astype(np.int64)
    out, m = W.warp(x, f0, SR, HOP, tm, 8000, 1.0, 0)
    at = np.minimum(pos[:101], 7999.0)
    contour, voiced = R.glide_f0(at / 8000.0), ~((at >= R.GAP[0]) & (at < R.GAP[1]))
    got = P.score(track(out), contour, R.inner(voiced))
    dev = R.envelope_deviation(out, contour, voiced)
    print("known smooth map: %s, envelope deviation %.2f dB" % (got, dev))
    assert got["gross"] == 0 and got["rms"] <= 15.0, got
    assert dev <= 2.2                                                        # test_prosody_cpu.py's bound for the same measure


# ---- refusals --------------------------------------------------------------------------------------------------------------------

def test_refusals_are_raised_without_a_device():
    x, f0 = torch.zeros(2, 8000), torch.zeros(2, 101)
    tm = torch.zeros(2, 102, dtype=torch.int32)
    for f in (prosody.warp, prosody.warp_marks):
        ok = dict(audio=x, n_samples=None, f0=f0, time_map=tm, n_out=[8000, 4000], sampling_rate=8000, hop_length=80)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            f(**ok)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            f(**dict(ok, pitch_ratio=torch.ones(2, 130), ratio_axis="output", out_hop_length=64, time_map=torch.zeros(2, 127, dtype=torch.int32)))
        for bad in (x.double(), x[None], torch.zeros(2, 0), [0.0] * 10):
            with pytest.raises(ValueError, match="audio"):
                f(**dict(ok, audio=bad))
        for bad in (f0.double(), f0[0], f0[:1], [0.0] * 101):
            with pytest.raises(ValueError, match="f0"):
                f(**dict(ok, f0=bad))
        with pytest.raises(ValueError, match="101 frames"):
            f(**dict(ok, f0=f0[:, :100]))
        for ns in ([8000], [8000, 8001], [8000, 0]):
            with pytest.raises(ValueError, match="n_samples"):
                f(**dict(ok, n_samples=ns))
        for bad in (tm.long(), tm[0], tm[:1], tm.float(), None, [0] * 102):
            with pytest.raises(ValueError, match="time_map"):
                f(**dict(ok, time_map=bad))
        with pytest.raises(ValueError, match="102 entries"):
            f(**dict(ok, time_map=tm[:, :101]))
        with pytest.raises(ValueError, match="127 entries"):
            f(**dict(ok, time_map=tm, out_hop_length=64))
        for bad in ([8000], [8000, 0], [8000, 4000.0], [8000, True], None, 8000, torch.tensor([8000.0, 1.0])):
            with pytest.raises(ValueError, match="n_out"):
                f(**dict(ok, n_out=bad))
        with pytest.raises(ValueError, match="max_out"):
            f(**dict(ok, max_out=7999))
        for kw, what in ((dict(max_out=0), "max_out"), (dict(max_out=8000.0), "max_out"), (dict(out_hop_length=0), "out_hop_length"),
                         (dict(out_hop_length=80.0), "out_hop_length"), (dict(hop_length=0), "hop_length"), (dict(sampling_rate=0), "sampling_rate"),
                         (dict(ratio_axis="frames"), "ratio_axis"), (dict(ratio_axis=1), "ratio_axis"), (dict(pitch_ratio=float("inf")), "pitch_ratio"),
                         (dict(pitch_ratio=None), "pitch_ratio"), (dict(pitch_ratio=torch.ones(3)), "pitch_ratio"),
                         (dict(pitch_ratio=torch.ones(2, 100)), "pitch_ratio"), (dict(pitch_ratio=torch.ones(2, 102)), "pitch_ratio"),
                         (dict(pitch_ratio=torch.ones(2, 100), ratio_axis="output"), "pitch_ratio"),
                         (dict(pitch_ratio=torch.ones(2, 101).double()), "pitch_ratio"), (dict(unvoiced_period=40.0), "unvoiced_period")):
            with pytest.raises(ValueError, match=what):
                f(**dict(ok, **kw))
        for period in (15, 1025):
            with pytest.raises(NotImplementedError, match="unvoiced_period"):
                f(**dict(ok, unvoiced_period=period))
        with pytest.raises(NotImplementedError, match="65535"):
            f(torch.zeros(65536, 1), None, torch.zeros(65536, 1), torch.zeros(65536, 2, dtype=torch.int32), [1] * 65536, 8000, 80)
        with pytest.raises(NotImplementedError, match="N_out = 4194305"):
            f(**dict(ok, n_out=[8000, (1 << 22) + 1]))
        big = torch.zeros(1, (1 << 22) + 1)
        with pytest.raises(NotImplementedError, match="MAX_SAMPLES"):
            f(big, None, torch.zeros(1, big.shape[1] // 4096 + 1), torch.zeros(1, 4, dtype=torch.int32), [100], 8000, 4096)
    path, plen = torch.zeros(2, 9, 2, dtype=torch.int32), torch.ones(2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        prosody.time_map_from_path(path, plen, 80, 5)
    for kw, what in ((dict(path=path.long()), "path"), (dict(path=path[0]), "path"), (dict(path=path[:, :, :1]), "path"), (dict(path=None), "path"),
                     (dict(path_len=plen.long()), "path_len"), (dict(path_len=plen[:1]), "path_len"), (dict(path_len=[1, 1]), "path_len"),
                     (dict(hop_length=0), "hop_length"), (dict(hop_length=(1 << 22) + 1), "hop_length"), (dict(n_frames=0), "n_frames"),
                     (dict(n_frames=5.0), "n_frames"), (dict(smooth=-1), "smooth"), (dict(smooth=33), "smooth"), (dict(smooth=1.0), "smooth")):
        with pytest.raises(ValueError, match=what):
            prosody.time_map_from_path(**dict(dict(path=path, path_len=plen, hop_length=80, n_frames=5), **kw))
    with pytest.raises(NotImplementedError, match="4096 cells"):
        prosody.time_map_from_path(torch.zeros(1, 4097, 2, dtype=torch.int32), plen[:1], 80, 5)


def test_c_abi_refuses_bad_arguments_before_the_device():
    """FT_EINVAL / FT_EUNSUPPORTED from the two entry points themselves, with host memory standing in for the buffers: nothing may
    be launched"""
    from flowtron_amd import _lib as L
    lib = L.lib()
    B, N, T, hop = 2, 1024, 13, 80
    KA, KS, TM = 64, 128, 14
    f32 = [(C.c_float * (B * N))() for _ in range(2)]
    i32 = [(C.c_int32 * (B * KS))() for _ in range(11)]
    adr = C.addressof
    ok = dict(f0=adr(f32[0]), fs=(T, 1), ratio=adr(f32[1]), rs=(0, 0), n=adr(i32[0]), noi=adr(i32[1]), tm=adr(i32[2]), a=adr(i32[3]),
              na=adr(i32[4]), s=adr(i32[5]), src=adr(i32[6]), half=adr(i32[7]), ns=adr(i32[8]), no=adr(i32[9]), B=B, N=N, N_out=N, T=T, RT=T,
              TM=TM, hop=hop, hop_out=hop, axis=0, KA=KA, KS=KS, sr256=2048000.0, unv=40)

    def warp(**kw):
        a = dict(ok, **kw)
        return lib.ft_psola_marks_warp(a["f0"], *a["fs"], a["ratio"], *a["rs"], a["n"], a["noi"], a["tm"], a["a"], a["na"], a["s"], a["src"],
                                       a["half"], a["ns"], a["no"], a["B"], a["N"], a["N_out"], a["T"], a["RT"], a["TM"], a["hop"], a["hop_out"],
                                       a["axis"], a["KA"], a["KS"], a["sr256"], a["unv"], None)
    for kw in (dict(f0=None), dict(ratio=None), dict(n=None), dict(noi=None), dict(tm=None), dict(a=None), dict(na=None), dict(s=None),
               dict(src=None), dict(half=None), dict(ns=None), dict(no=None), dict(B=0), dict(B=65536), dict(N=0), dict(N_out=0), dict(T=0),
               dict(T=12), dict(hop=0), dict(fs=(-T, 1)), dict(fs=(T, -1)), dict(rs=(-1, 0)), dict(rs=(0, -1)), dict(KA=63), dict(KS=127),
               dict(sr256=0.0), dict(sr256=float("nan")), dict(sr256=float("inf")),
               dict(TM=13), dict(TM=0), dict(hop_out=0), dict(hop_out=-80), dict(hop_out=(1 << 22) + 1), dict(hop_out=64), dict(RT=12), dict(RT=0),
               dict(axis=2), dict(axis=-1), dict(axis=1, hop_out=64, TM=18, RT=16)):
        assert warp(**kw) == -1, kw
        assert b"ft_psola_marks_warp" in lib.ft_last_error()
    for kw, what in ((dict(unv=15), b"16 .. 1024"), (dict(unv=1025), b"16 .. 1024"), (dict(N=(1 << 22) + 1), b"4194304"),
                     (dict(N_out=(1 << 22) + 1), b"4194304")):
        assert warp(**kw) == -3, kw
        assert b"ft_psola_marks_warp" in lib.ft_last_error() and what in lib.ft_last_error()

    okt = dict(path=adr(i32[0]), plen=adr(i32[1]), tm=adr(i32[2]), B=B, P=20, TM=TM, hop=hop, w=4)

    def tmap(**kw):
        a = dict(okt, **kw)
        return lib.ft_psola_time_map(a["path"], a["plen"], a["tm"], a["B"], a["P"], a["TM"], a["hop"], a["w"], None)
    for kw in (dict(path=None), dict(plen=None), dict(tm=None), dict(B=0), dict(B=65536), dict(P=0), dict(TM=0), dict(hop=0),
               dict(hop=(1 << 22) + 1), dict(w=-1), dict(w=33)):
        assert tmap(**kw) == -1, kw
        assert b"ft_psola_time_map" in lib.ft_last_error()
    assert tmap(P=4097) == -3 and b"ft_psola_time_map" in lib.ft_last_error() and b"4096" in lib.ft_last_error()
