"""A pace that varies within the utterance, on the device (-m gpu): prosody.warp_marks and prosody.warp against the fp32 replay
(tests/prosody_warp_ref.py) bit for bit -- marks, counts, sources, half-widths, n_out and the output -- on a ragged batch whose
padding is NaN in the audio, in F0 and in the ratio and garbage in the map, every utterance alone and in the batch, strided
views, lengths and n_out on the device; four kinds of map (smooth, frozen, jumping, non-monotone), both ratio axes, an output
hop that is not the input's; an utterance with more frames, map entries and ratio entries than the marks kernel keeps in LDS;
grains dense enough for the synthesis' second staging round.  Then device against device: constant maps at paces 1, 2 and 0.5
against prosody.marks / prosody.modify.  prosody.time_map_from_path against its replay on the paths of metrics.dtw.  The chain
f0_track -> dtw -> time_map_from_path -> transfer_ratio -> warp -> f0_track on the transfer signal against the host's figures
(tests/test_prosody_warp_cpu.py).  Entry calls and no synchronisation.  8 kHz, a hop of 80."""
import numpy as np
import pytest
import torch

import dtw_ref as D
import pitch_ref
import prosody_ref as R
import prosody_warp_ref as W
import pyin_ref as P
from call_count import count_calls
from flowtron_amd import metrics, pitch, prosody

pytestmark = pytest.mark.gpu

SR, HOP, Q = 8000.0, 80, 256
LENGTHS = (8000, 5000, 1601, 79, 1)
KW = dict(sampling_rate=SR, hop_length=HOP)
# name -> (map, ratio axis, out_hop_length, ratio: "frames" = a [B, RT] tensor on that axis, "each" = a [B] tensor, or a number)
SETTINGS = {"smooth_in": ("smooth", "input", 80, "frames"), "smooth_out": ("smooth", "output", 80, "frames"),
            "smooth_out_hop64": ("smooth", "output", 64, "frames"), "smooth_in_hop64": ("smooth", "input", 64, 1.19),
            "frozen_in": ("frozen", "input", 80, "each"), "frozen_out": ("frozen", "output", 80, "frames"),
            "jump_in": ("jump", "input", 80, 1.0), "jump_out": ("jump", "output", 80, "frames"),
            "wild_in": ("wild", "input", 80, "frames"), "wild_out": ("wild", "output", 80, "each")}
EACH = (1.5, 0.7, 2.0, 1.0, 0.625)
GARBAGE = -(2 ** 31)                                                        # what lies behind the entries of a map that count

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


def one_map(kind, n, hop_out, b):
    """-> (the entries the utterance alone would hand over [n_out // hop_out + 2] int64, n_out) for an utterance of n samples"""
    frames = n // HOP
    if kind == "smooth":                                                     # 1.2 times as long, the pace swinging by a half
        n_out = max(1, n * 6 // 5)
        v = np.arange(n_out // hop_out + 2) * hop_out / float(n_out)
        return np.rint(n * (v + 0.08 * np.sin(2 * np.pi * v)) * Q).astype(np.int64), n_out
    if kind == "frozen":                                                     # held still for 20 frames a quarter in
        n_out = n + 20 * HOP
        u = np.arange(n_out // hop_out + 2) * hop_out // HOP
        at = frames // 4
        return np.where(u < at, u, np.where(u < at + 20, at, u - 20)).astype(np.int64) * HOP * Q, n_out
    if kind == "jump":                                                       # five frames at a slope of 6, the end reached early
        n_out = n
        u = np.arange(n_out // hop_out + 2) * hop_out // HOP
        at = frames // 4
        return np.where(u < at, u, np.where(u < at + 5, at + 6 * (u - at), u + 25)).astype(np.int64) * HOP * Q, n_out
    assert kind == "wild"                                                    # the identity and up to 12 frames to either side, and outliers
    n_out = n
    rng = np.random.RandomState(40 + b)
    u = np.arange(n_out // hop_out + 2)
    m = (u * hop_out + rng.randint(-12 * HOP, 12 * HOP + 1, size=len(u))).astype(np.int64) * Q
    m[::17] = np.resize([-2 ** 31, 2 ** 31 - 1, -1, 0], len(m[::17]))
    return m, n_out


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
        _CASE.update(xs=xs, X=Xd, f0=f0, f0_host=f0.cpu().numpy(), settings={})
    return _CASE


def setting(name):
    """-> dict(tmap [B, TM] on the device, n_out list, N_out, ratio for the device, ratios for the replay, rows: the maps' entries
    that count, want: the replay's (out, marks) per utterance), made once per name"""
    c = case()
    if name not in c["settings"]:
        kind, axis, hop_out, ratio = SETTINGS[name]
        rows, n_outs = zip(*[one_map(kind, n, hop_out, b) for b, n in enumerate(LENGTHS)])
        N_out = max(n_outs)
        TM = N_out // hop_out + 2
        tm = np.full((len(LENGTHS), TM), GARBAGE, np.int64)
        for b, row in enumerate(rows):
            tm[b, :len(row)] = np.clip(row, -2 ** 31, 2 ** 31 - 1)
        rows = [tm[b, :len(row)] for b, row in enumerate(rows)]
        if ratio == "frames":                                                # 0.5 .. 2.2 per frame of the axis, NaN behind, some NaN within
            widths = [n // HOP + 1 for n in LENGTHS] if axis == "input" else [n // hop_out + 1 for n in n_outs]
            RT = 101 if axis == "input" else N_out // hop_out + 1
            rng = np.random.RandomState(len(name))
            r = np.full((len(LENGTHS), RT), np.nan, np.float32)
            for b, wd in enumerate(widths):
                r[b, :wd] = 2.0 ** rng.uniform(-1.0, 1.14, size=wd)
                r[b, 3:wd:29] = np.nan
            r_dev, r_host = dev(r), [r[b, :wd] for b, wd in enumerate(widths)]
        elif ratio == "each":
            r_dev, r_host = torch.tensor(EACH, dtype=torch.float32).cuda(), list(EACH)
        else:
            r_dev, r_host = ratio, [ratio] * len(LENGTHS)
        want = [W.warp(x, c["f0_host"][b, :len(x) // HOP + 1], SR, HOP, rows[b], n_outs[b], r_host[b], prosody._AXES[axis], hop_out)
                for b, x in enumerate(c["xs"])]
        c["settings"][name] = dict(tmap=dev(tm.astype(np.int32)), n_out=list(n_outs), N_out=N_out, ratio=r_dev, rows=rows, want=want,
                                   kw=dict(KW, out_hop_length=hop_out, ratio_axis=axis), axis=axis, hop_out=hop_out)
    return c["settings"][name]


def assert_marks_equal(got, b, want, who):
    """utterance b of a Marks tuple (None: unbatched) against the replay's dict"""
    pick = (lambda t: t) if b is None else (lambda t: t[b])
    K, J = int(pick(got.n_analysis)), int(pick(got.n_synthesis))
    assert (K, J, int(pick(got.n_out))) == (len(want["analysis"]), len(want["synthesis"]), want["n_out"]), (who, b)
    assert bits(pick(got.analysis)[:K]) == want["analysis"].tobytes(), (who, b, "analysis")
    for key in ("synthesis", "source", "half"):
        assert bits(pick(getattr(got, key))[:J]) == want[key].tobytes(), (who, b, key)


def test_the_maps_hold_what_they_are_meant_to_hold():
    s = setting("frozen_in")
    assert s["n_out"] == [n + 1600 for n in LENGTHS] and np.all(np.diff(s["rows"][0])[25:45] == 0)
    assert np.diff(setting("jump_in")["rows"][0]).max() == 6 * HOP * Q
    wild = setting("wild_in")["rows"][0]
    assert (np.diff(wild) < 0).sum() > 30 and wild.min() == -2 ** 31 and wild.max() == 2 ** 31 - 1
    smooth = setting("smooth_out_hop64")
    assert smooth["N_out"] == 9600 and tuple(smooth["tmap"].shape) == (5, 152) and int(smooth["tmap"][1, -1]) == GARBAGE
    assert tuple(smooth["ratio"].shape) == (5, 151) and torch.isnan(smooth["ratio"][1, 6000 // 64 + 1:]).all()
    grains = [len(w[1]["synthesis"]) for w in setting("frozen_in")["want"]]
    assert grains[0] > 150 and grains[3] >= 25 and grains[4] >= 25           # 79 samples and 1 sample, played for 1600 more


@pytest.mark.parametrize("name", list(SETTINGS))
def test_marks_and_output_equal_the_replay_alone_and_in_the_batch(name):
    c, s = case(), setting(name)
    got = prosody.warp_marks(c["X"], list(LENGTHS), c["f0"], s["tmap"], s["n_out"], pitch_ratio=s["ratio"], **s["kw"])
    out, n_out = prosody.warp(c["X"], list(LENGTHS), c["f0"], s["tmap"], s["n_out"], pitch_ratio=s["ratio"], **s["kw"])
    N_out = s["N_out"]
    assert all(t.dtype == torch.int32 and t.is_cuda for t in got) and n_out.dtype == torch.int32 and n_out.is_cuda
    assert tuple(out.shape) == (5, N_out) and out.dtype == torch.float32
    assert tuple(got.analysis.shape) == (5, 500) and tuple(got.synthesis.shape) == (5, -(-N_out // 8))
    assert bits(n_out) == bits(got.n_out) and n_out.tolist() == s["n_out"]
    o = out.cpu().numpy()
    for b, (x, (w_out, w_marks)) in enumerate(zip(c["xs"], s["want"])):
        assert_marks_equal(got, b, w_marks, name)
        n = w_marks["n_out"]
        assert o[b, :n].tobytes() == w_out.tobytes(), (name, b, "differs first at %s" % np.nonzero(o[b, :n].view(np.int32) != w_out.view(np.int32))[0][:5])
        assert not o[b, n:].any(), (name, b)
        f1 = c["f0"][b, :len(x) // HOP + 1].contiguous()
        r1 = s["ratio"]
        if torch.is_tensor(r1):
            r1 = r1[b] if r1.dim() == 1 else r1[b, :(len(x) // HOP + 1 if s["axis"] == "input" else n // s["hop_out"] + 1)].contiguous()
        t1 = dev(s["rows"][b].astype(np.int32))                              # its own entries and no more
        alone = prosody.warp(dev(x), None, f1, t1, n, pitch_ratio=r1, **s["kw"])
        assert alone[1].dim() == 0 and int(alone[1]) == n and bits(alone[0]) == w_out.tobytes(), (name, b, "alone")
        assert_marks_equal(prosody.warp_marks(dev(x), None, f1, t1, [n], pitch_ratio=r1, **s["kw"]), None, w_marks, name + " alone")


def test_strided_views_and_device_lengths_give_the_same_bits():
    c, s = case(), setting("smooth_out_hop64")
    want_out, want_n = prosody.warp(c["X"], list(LENGTHS), c["f0"], s["tmap"], s["n_out"], pitch_ratio=s["ratio"], **s["kw"])
    wide = torch.full((5, 8000, 3), float("nan"), device="cuda")
    wide[:, :, 1] = c["X"]
    f0_wide = torch.full((5, 101, 2), float("nan"), device="cuda")
    f0_wide[:, :, 0] = c["f0"]
    r_wide = torch.full((5, 160, 2), float("nan"), device="cuda")
    r_wide[:, :151, 1] = s["ratio"]
    t_wide = torch.full((5, 170, 2), 7, dtype=torch.int32, device="cuda")
    t_wide[:, :152, 0] = s["tmap"]
    n_dev, no_dev = torch.tensor(LENGTHS, dtype=torch.int32).cuda(), torch.tensor(s["n_out"], dtype=torch.int32).cuda()
    assert not wide[:, :, 1].is_contiguous() and not t_wide[:, :, 0].is_contiguous()
    for audio, n, f0, tm, no, ratio, more in ((wide[:, :, 1], list(LENGTHS), c["f0"], s["tmap"], s["n_out"], s["ratio"], {}),
                                              (c["X"], n_dev, f0_wide[:, :, 0], s["tmap"], no_dev, s["ratio"], dict(max_out=9600)),
                                              (c["X"], n_dev, c["f0"], t_wide[:, :, 0], no_dev, r_wide[:, :, 1], dict(max_out=9600))):
        out, n_out = prosody.warp(audio, n, f0, tm, no, pitch_ratio=ratio, **dict(s["kw"], **more))
        assert bits(out) == bits(want_out) and bits(n_out) == bits(want_n)
    loose_n = torch.tensor([9000, 5000, 1601, 79, 0], dtype=torch.int32).cuda()          # both clamped in the kernels: 1 ..= N, 1 ..= N_out
    loose_out = torch.tensor([2 ** 31 - 1, 6000, 1921, 94, 0], dtype=torch.int32).cuda()
    out, n_out = prosody.warp(c["X"], loose_n, c["f0"], s["tmap"], loose_out, pitch_ratio=s["ratio"], max_out=9600, **s["kw"])
    assert bits(out) == bits(want_out) and bits(n_out) == bits(want_n)
    wider, n_wider = prosody.warp(c["X"], n_dev, c["f0"], t_wide[:, :, 0], no_dev, pitch_ratio=r_wide[:, :, 1], max_out=10000, **s["kw"])
    assert tuple(wider.shape) == (5, 10000) and bits(wider[:, :9600]) == bits(want_out) and not wider[:, 9600:].any() and bits(n_wider) == bits(want_n)


@pytest.mark.parametrize("pace", [1, 2, 0.5])
def test_constant_maps_equal_marks_and_modify_device_against_device(pace):
    c = case()
    ratio = torch.tensor(EACH, dtype=torch.float32).cuda()
    want_marks = prosody.marks(c["X"], list(LENGTHS), c["f0"], pitch_ratio=ratio, pace=float(pace), **KW)
    want_out, want_n = prosody.modify(c["X"], list(LENGTHS), c["f0"], pitch_ratio=ratio, pace=float(pace), **KW)
    N_out = prosody.out_samples(8000, pace)
    n_out = [prosody.out_samples(n, pace) for n in LENGTHS]
    tm = dev(np.tile(W.constant_map(pace, HOP, N_out // HOP + 2).astype(np.int32), (5, 1)))
    got_marks = prosody.warp_marks(c["X"], list(LENGTHS), c["f0"], tm, n_out, pitch_ratio=ratio, **KW)
    got_out, got_n = prosody.warp(c["X"], list(LENGTHS), c["f0"], tm, n_out, pitch_ratio=ratio, **KW)
    assert bits(got_out) == bits(want_out) and bits(got_n) == bits(want_n) and want_n.tolist() == n_out
    K, J = want_marks.n_analysis.tolist(), want_marks.n_synthesis.tolist()
    assert got_marks.n_analysis.tolist() == K and got_marks.n_synthesis.tolist() == J and bits(got_marks.n_out) == bits(want_marks.n_out)
    for b in range(5):
        assert bits(got_marks.analysis[b, :K[b]]) == bits(want_marks.analysis[b, :K[b]]), b
        for key in ("synthesis", "source", "half"):
            assert bits(getattr(got_marks, key)[b, :J[b]]) == bits(getattr(want_marks, key)[b, :J[b]]), (b, key)
    print("pace %g: %s grains, device against device" % (pace, J))


def test_more_frames_than_the_marks_kernel_keeps_in_lds():
    """a hop of 16 on both sides: 4376 input frames, 5252 map entries and 5251 output frames of the ratio, each more than the
    4096 the wave stages"""
    n, hop = 70000, 16
    rng = np.random.RandomState(11)
    x = (0.2 * rng.randn(n)).astype(np.float32)
    t = np.arange(n // hop + 1)
    f0 = (150.0 * 2.0 ** (0.4 * np.sin(2 * np.pi * t / 700.0))).astype(np.float32)
    f0[(t % 300) > 250] = 0.0
    n_out = 84000
    u = np.arange(n_out // hop + 2)
    v = u * hop / float(n_out)
    tm = np.rint(n * (v + 0.05 * np.sin(2 * np.pi * 3 * v)) * Q).astype(np.int64)
    assert len(t) > 4096 and (f0[4096:] > 0).any() and (f0[4096:] == 0).any() and len(tm) == 5252 and tm.max() < 2 ** 31
    for axis, ratio in (("output", (2.0 ** (0.5 * np.cos(2 * np.pi * np.arange(n_out // hop + 1) / 300.0))).astype(np.float32)),
                        ("input", (2.0 ** (0.5 * np.cos(2 * np.pi * t / 300.0))).astype(np.float32))):
        w_out, w_marks = W.warp(x, f0, SR, hop, tm, n_out, ratio, prosody._AXES[axis])
        kw = dict(sampling_rate=SR, hop_length=hop, pitch_ratio=dev(ratio), ratio_axis=axis)
        assert_marks_equal(prosody.warp_marks(dev(x), None, dev(f0), dev(tm.astype(np.int32)), n_out, **kw), None, w_marks, "long " + axis)
        out, got_n = prosody.warp(dev(x), None, dev(f0), dev(tm.astype(np.int32)), n_out, **kw)
        assert int(got_n) == n_out == len(w_out) and bits(out) == w_out.tobytes(), axis
        late = (w_marks["synthesis"] >> 8) > 4200 * hop
        assert late.sum() > 150 and len(np.unique(np.diff(w_marks["synthesis"][late]))) > 20             # the walk does go there, and the ratio counts


@pytest.mark.parametrize("hz,grains", [(400.0, 400), (500.0, 500)])
def test_grains_dense_enough_for_a_second_staging_round(hz, grains):
    """ratio 2 on a 400 Hz contour, on the output's axis, along a map at half speed: a grain every 10 samples (231 within reach
    of a tile of 256); at 500 Hz every 8 samples: 288, more than one round of 256"""
    n, n_out = 2000, 4000
    x = (0.3 * np.sin(2 * np.pi * hz * np.arange(n) / SR)).astype(np.float32)
    f0 = np.full(n // HOP + 1, hz, np.float32)
    tm = W.constant_map(0.5, HOP, n_out // HOP + 2)
    ratio = np.full(n_out // HOP + 1, 2.0, np.float32)
    w_out, w_marks = W.warp(x, f0, SR, HOP, tm, n_out, ratio, 1)
    assert len(w_marks["synthesis"]) == grains and np.all(w_marks["half"] == int(SR / hz))
    args = (dev(x), None, dev(f0), dev(tm.astype(np.int32)), n_out)
    assert_marks_equal(prosody.warp_marks(*args, pitch_ratio=dev(ratio), ratio_axis="output", **KW), None, w_marks, "dense")
    assert bits(prosody.warp(*args, pitch_ratio=dev(ratio), ratio_axis="output", **KW)[0]) == w_out.tobytes()


# ---- a path to a map ---------------------------------------------------------------------------------------------------------------

SHAPES = ((1, 1), (1, 7), (7, 1), (63, 65), (65, 63), (257, 255))


def test_time_map_from_path_equals_the_replay_batched_and_alone():
    pairs = [D.pair("normal", Ta, Tb, 3) for Ta, Tb in SHAPES]
    xb, yb = np.full((6, 257, 3), np.nan, np.float32), np.full((6, 257, 3), np.nan, np.float32)
    for b, (x, y) in enumerate(pairs):
        xb[b, :len(x)], yb[b, :len(y)] = x, y
    _, path, plen = metrics.dtw(dev(xb), dev(yb), [s[0] for s in SHAPES], [s[1] for s in SHAPES])
    cells, lens = path.cpu().numpy(), plen.tolist()
    assert tuple(path.shape) == (6, 513, 2) and lens[0] == 1 and lens[1] == 7 and lens[2] == 7
    for b, (x, y) in enumerate(pairs):
        assert np.array_equal(cells[b, :lens[b]], D.replay(x, y)[1]), b      # the device's path is the replay's
    for w in (0, 4, 32):
        tm = prosody.time_map_from_path(path, plen, HOP, 258, smooth=w)
        assert tm.dtype == torch.int32 and tuple(tm.shape) == (6, 259) and tm.is_cuda
        for b, (Ta, Tb) in enumerate(SHAPES):
            assert bits(tm[b]) == W.time_map_from_path(cells[b], lens[b], HOP, 259, w).tobytes(), (w, b)
            _, p1, l1 = metrics.dtw(dev(pairs[b][0])[None], dev(pairs[b][1])[None])
            alone = prosody.time_map_from_path(p1, l1, HOP, Tb, smooth=w)
            assert tuple(alone.shape) == (1, Tb + 1) and bits(alone[0]) == bits(tm[b, :Tb + 1]), (w, b, "alone")
            assert bool((tm[b, 1:] >= tm[b, :-1]).all())
    part = [0, 5, 7, 3, 100, lens[5] - 10]                                   # the first cells of a path are a path; 0 counts as 1
    tm = prosody.time_map_from_path(path, torch.tensor(part, dtype=torch.int32).cuda(), 256, 40, smooth=2)
    for b, n in enumerate(part):
        assert bits(tm[b]) == W.time_map_from_path(cells[b], max(n, 1), 256, 41, 2).tobytes(), b
    diagonal = dev(np.stack([np.arange(20), np.arange(20)], 1).astype(np.int32))[None]                # a length above P counts as P
    a, b = (prosody.time_map_from_path(diagonal, torch.tensor([n], dtype=torch.int32).cuda(), HOP, 25) for n in (9999, 20))
    assert bits(a) == bits(b) and bits(a[0]) == W.time_map_from_path(diagonal[0].cpu().numpy(), 20, HOP, 26, 4).tobytes()


# ---- the chain -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("smooth", [4])
def test_device_chain_transfers_melody_and_rhythm(smooth):
    S = W.transfer_signal()
    src, ref = dev(S["src"]), dev(S["ref"])
    f_src, f_ref = track_on_device(src, None), track_on_device(ref, None)
    lp_src, lp_ref = W.log_power(S["src"]), W.log_power(S["ref"])
    _, path, plen = metrics.dtw(dev(lp_src)[None], dev(lp_ref)[None])
    tmap = prosody.time_map_from_path(path, plen, HOP, 121, smooth=smooth)
    ratio = prosody.transfer_ratio(f_src[None], f_ref[None], tmap, HOP, register="reference")
    out, n_out = prosody.warp(src[None], None, f_src[None], tmap, [W.N_REF], pitch_ratio=ratio, ratio_axis="output", **KW)
    f_out = track_on_device(out, [W.N_REF])[0].cpu().numpy()
    got = P.score(f_out, S["truth"], R.inner(S["voiced"]))
    # the same chain on the host, replay by replay
    h_src, h_ref = (P.track(S[k], P.config("small"), np.float32)["f0"] for k in ("src", "ref"))
    h_path = D.replay(lp_src, lp_ref)[1]
    h_tmap = W.time_map_from_path(h_path, len(h_path), HOP, 122, smooth)
    h_ratio = W.transfer_ratio(h_src, h_ref, h_tmap, HOP)
    h_out, h_marks = W.warp(S["src"], h_src, SR, HOP, h_tmap, W.N_REF, h_ratio, 1)
    want = P.score(P.track(h_out, P.config("small"), np.float32)["f0"], S["truth"], R.inner(S["voiced"]))
    lp = float(np.sqrt(np.mean((W.log_power(out[0].cpu().numpy()).astype(np.float64) - lp_ref) ** 2)))
    uniform = prosody.modify(src, None, f_src, pace=W.N_SRC / W.N_REF, **KW)[0].cpu().numpy()
    base = float(np.sqrt(np.mean((W.log_power(uniform).astype(np.float64) - lp_ref) ** 2)))
    print("on the device, smooth %d: %s; log-power contour %.3f rms (uniform pace %.3f); the host gives %s" % (smooth, got, lp, base, want))
    assert bits(tmap[0]) == h_tmap.tobytes() and bits(ratio[0]) == h_ratio.tobytes()
    assert int(n_out) == W.N_REF and bits(out[0]) == h_out.tobytes()
    assert got == want                                                       # the host test's figures, exactly
    assert got["gross"] == 0 and got["rms"] <= 15.0 and lp < 0.5 * base, (got, lp, base)


def test_register_source_keeps_the_speakers_mean():
    S = W.transfer_signal()
    f_src, f_ref = track_on_device(dev(S["src"]), None), track_on_device(dev(S["ref"]), None)
    tmap = dev(np.rint(np.append(S["true_map"], S["true_map"][-1]) * Q).astype(np.int32))
    r = prosody.transfer_ratio(f_src, f_ref, tmap, HOP, register="source")
    want = W.transfer_ratio(f_src.cpu().numpy(), f_ref.cpu().numpy(), tmap.cpu().numpy(), HOP, "source")
    assert tuple(r.shape) == (121,) and np.allclose(r.cpu().numpy(), want, rtol=3e-7, atol=0)
    plain = prosody.transfer_ratio(f_src, f_ref, tmap, HOP)
    on = (plain != 1).cpu().numpy()
    assert on.sum() > 60 and np.ptp(np.log2(r.cpu().numpy()[on] / plain.cpu().numpy()[on])) < 1e-6       # one factor on every voiced frame


def test_durations_give_a_map_on_the_device_that_warp_takes():
    c = case()
    src = torch.tensor([[25, 25, 50, 0], [20, 20, 22, 0], [5, 5, 5, 5], [0, 0, 0, 0], [0, 0, 0, 0]]).cuda()
    tgt = torch.tensor([[25, 50, 50, 0], [20, 10, 22, 9], [5, 0, 5, 5], [1, 0, 0, 0], [0, 0, 0, 1]]).cuda()
    tmap, frames = prosody.time_map_from_durations(src, tgt, None, HOP, n_frames=125)
    assert tmap.is_cuda and tmap.dtype == torch.int32 and tuple(tmap.shape) == (5, 127) and frames.tolist() == [125, 61, 15, 1, 1]
    for b in range(5):
        assert bits(tmap[b]) == W.time_map_from_durations(src[b].tolist(), tgt[b].tolist(), HOP, 127)[0].tobytes(), b
    n_out = (frames * HOP).clamp(max=10000)
    out, got_n = prosody.warp(c["X"], list(LENGTHS), c["f0"], tmap, n_out, max_out=10000, **KW)
    assert got_n.tolist() == [10000, 4880, 1200, 80, 80]
    for b, x in enumerate(c["xs"]):
        w_out, _ = W.warp(x, c["f0_host"][b, :len(x) // HOP + 1], SR, HOP, tmap[b].cpu().numpy(), int(got_n[b]))
        assert bits(out[b, :len(w_out)]) == w_out.tobytes(), b


# ---- calls ------------------------------------------------------------------------------------------------------------------------

def test_warp_makes_two_entry_calls_and_never_synchronises(monkeypatch):
    c, s = case(), setting("smooth_out")
    n_dev, no_dev = torch.tensor(LENGTHS, dtype=torch.int32).cuda(), torch.tensor(s["n_out"], dtype=torch.int32).cuda()
    kw = dict(s["kw"], pitch_ratio=s["ratio"], max_out=s["N_out"])
    want = prosody.warp(c["X"], n_dev, c["f0"], s["tmap"], no_dev, **kw)      # warm: the window table is on the device
    path = torch.zeros(5, 9, 2, dtype=torch.int32).cuda()
    plen = torch.ones(5, dtype=torch.int32).cuda()
    durations = torch.ones(5, 4, dtype=torch.int64).cuda()
    entries = ("ft_psola_marks_warp", "ft_psola_synth", "ft_psola_time_map", "ft_psola_marks")
    calls = count_calls(monkeypatch, entries)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out, n_out = prosody.warp(c["X"], n_dev, c["f0"], s["tmap"], no_dev, **kw)
        prosody.warp_marks(c["X"], n_dev, c["f0"], s["tmap"], no_dev, **kw)
        tm = prosody.time_map_from_path(path, plen, HOP, 120)
        prosody.transfer_ratio(c["f0"], c["f0"], tm, HOP, register="source")
        prosody.time_map_from_durations(durations, durations * 2, n_dev.clamp(max=4), HOP, n_frames=8)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert calls == {"ft_psola_marks_warp": 2, "ft_psola_synth": 1, "ft_psola_time_map": 1, "ft_psola_marks": 0}
    assert bits(out) == bits(want[0]) and bits(n_out) == bits(want[1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        prosody.warp(c["X"].cpu(), list(LENGTHS), c["f0"].cpu(), s["tmap"].cpu(), s["n_out"], **dict(kw, pitch_ratio=1.0))
    with pytest.raises(ValueError, match="max_out"):
        prosody.warp(c["X"], n_dev, c["f0"], s["tmap"], no_dev, **dict(kw, max_out=None))
