"""Mel-cepstral distortion along a dynamic-time-warping path on the device (-m gpu): the warp kernel against its float32 replay
(tests/dtw_ref.py) bit for bit -- cost, path and path length --, the cepstra kernel against the float32 restatement bit for
bit, raggedness inside a poisoned view, inputs on which every compare fails, the frame-by-frame form, the dB formula, and the
round trip of a small model: a reconstruction along its own alignments is nearer the recording than a fresh sample."""
import math
import os

import numpy as np
import pytest
import torch

import dtw_ref as R
from call_count import count_calls
from flowtron_amd import metrics

pytestmark = pytest.mark.gpu

_REPLAYS = {}


def replay(kind, Ta, Tb, K):
    """(x, y, cost, path) of the shared inputs at a shape, computed once"""
    key = (kind, Ta, Tb, K)
    if key not in _REPLAYS:
        x, y = R.pair(kind, Ta, Tb, K)
        _REPLAYS[key] = (x, y) + R.replay(x, y, np.float32)
    return _REPLAYS[key]


def warp(x, y, x_lens, y_lens, **kw):
    """-> numpy (cost, path, path_len) of metrics.dtw on device features"""
    cost, path, path_len = metrics.dtw(x, y, x_lens, y_lens, **kw)
    assert cost.dtype == torch.float32 and path.dtype == torch.int32 and path_len.dtype == torch.int32
    assert cost.is_cuda and path.is_cuda and path_len.is_cuda
    assert tuple(path.shape) == (x.shape[0], x.shape[1] + y.shape[1] - 1, 2)
    return cost.cpu().numpy(), path.cpu().numpy(), path_len.cpu().numpy()


def same_float(a, b):
    return np.float32(a).tobytes() == np.float32(b).tobytes() or (np.isnan(a) and np.isnan(b))


def assert_equals(got, want_cost, want_path, b=0):
    """pair b of `got` against a replay: the same bits, -1 behind the path"""
    cost, path, path_len = got
    n = len(want_path)
    assert path_len[b] == n, (b, path_len[b], n)
    assert np.array_equal(path[b, :n], want_path), b
    assert np.all(path[b, n:] == -1)
    assert same_float(cost[b], want_cost), (b, cost[b], want_cost)


def assert_valid(path, n, A, N):
    p = path[:n]
    assert tuple(p[0]) == (0, 0) and tuple(p[-1]) == (A - 1, N - 1)
    assert {tuple(s) for s in np.diff(p, axis=0).tolist()} <= {(1, 1), (1, 0), (0, 1)}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("kind,K", [("normal", 13), ("grid", 1)])
@pytest.mark.parametrize("Ta,Tb", R.SHAPES)
def test_warp_equals_the_float32_replay_bit_for_bit(Ta, Tb, kind, K):
    x, y, cost, path = replay(kind, Ta, Tb, K)
    got = warp(dev(x)[None], dev(y)[None], [Ta], [Tb])
    assert_equals(got, cost, path)
    assert_valid(got[1][0], got[2][0], Ta, Tb)


def test_warp_at_32_features_and_at_widths_between_the_compiled_ones():
    for K, Ta, Tb in ((32, 257, 255), (5, 70, 63), (20, 63, 70), (2, 9, 130)):
        x, y, cost, path = replay("normal", Ta, Tb, K)
        assert_equals(warp(dev(x)[None], dev(y)[None], [Ta], [Tb]), cost, path)


@pytest.mark.parametrize("K", [13, 32])
def test_single_frame_pairs_give_the_distance_itself(K):
    """256 pairs of one frame each: cost[b] is d[0][0], no sum behind which a rounding of the distance could hide"""
    x, y = R.features("normal", 256, K, 11), R.features("normal", 256, K, 12)
    want = np.array([R.distances(x[b:b + 1], y[b:b + 1])[0, 0] for b in range(256)], np.float32)
    cost, path, path_len = warp(dev(x)[:, None], dev(y)[:, None], [1] * 256, [1] * 256)
    assert cost.tobytes() == want.tobytes()
    assert np.all(path == 0) and np.all(path_len == 1)
    fused = np.array([R.distances(x[b:b + 1], y[b:b + 1], fma=True)[0, 0] for b in range(256)], np.float32)
    assert fused.tobytes() != want.tobytes()                                # the inputs would show a fused multiply-add


@pytest.mark.parametrize("M,K,T", [(80, 13, 70), (128, 32, 333), (80, 1, 64)])
def test_cepstra_equal_the_float32_restatement_bit_for_bit(M, K, T):
    """T off the wave and off the workgroup, a [B, M, T] view with a stride in every dimension, per-utterance frame counts"""
    B = 3
    lens = [T, 1, T - 5]
    big = torch.full((B + 1, M + 3, 2 * T + 4), float("nan"))
    view = big[1:, 2:M + 2, 1:2 * T + 1:2]
    mels = []
    for b in range(B):
        mel = R.log_mel(M, lens[b], 10 * M + b)
        view[b, :, :lens[b]] = torch.from_numpy(mel)
        mels.append(mel)
    d = big.cuda()
    v = d[1:, 2:M + 2, 1:2 * T + 1:2]
    assert not v.is_contiguous() and v.stride(2) == 2
    cep = metrics.mel_cepstra(v, lens, n_coeffs=K)
    assert tuple(cep.shape) == (B, T, K) and cep.dtype == torch.float32 and cep.is_contiguous()
    got = cep.cpu().numpy()
    for b in range(B):
        assert got[b, :lens[b]].tobytes() == R.cepstra(mels[b], K).tobytes(), b
        assert np.all(got[b, lens[b]:] == 0)
    d[torch.isnan(d)] = 1e30                                                # nothing behind a length or around the view is read
    assert metrics.mel_cepstra(v, torch.tensor(lens).cuda(), n_coeffs=K).cpu().numpy().tobytes() == got.tobytes()
    full = metrics.mel_cepstra(dev(mels[0])[None], n_coeffs=K)              # contiguous, no lengths
    assert full.cpu().numpy()[0].tobytes() == R.cepstra(mels[0], K).tobytes()


def test_ragged_batch_inside_a_padded_view_never_reads_behind_the_lengths():
    """six pairs of one call, their features inside non-contiguous views; everything behind the lengths and around the views is
    NaN, then 1e30: nothing of it may be read"""
    lens = [(75, 70), (40, 40), (9, 1), (1, 66), (64, 65), (12, 5)]         # (A, N)
    K = 13
    bigx, bigy = torch.full((2, 8, 80, 16), float("nan")), torch.full((8, 150, 14), float("nan"))
    vx, vy = bigx[1, 1:7, 2:77, 1:14], bigy[1:7, 3:143:2, :13]             # [6, 75, 13], [6, 70, 13]
    pairs = []
    for b, (A, N) in enumerate(lens):
        x, y = R.pair("normal", A, N, K)
        if b % 2:
            x, y = np.round(x * 2) / 2, np.round(y * 2) / 2               # coarse values: some ties
        vx[b, :A], vy[b, :N] = torch.from_numpy(x), torch.from_numpy(y)
        pairs.append((x, y))
    dx, dy = bigx.cuda(), bigy.cuda()
    x, y = dx[1, 1:7, 2:77, 1:14], dy[1:7, 3:143:2, :13]
    assert not x.is_contiguous() and not y.is_contiguous()
    al, nl = [a for a, _ in lens], [n for _, n in lens]
    got = warp(x, y, torch.tensor(al), torch.tensor(nl).cuda())             # lengths on the host and on the device
    for b, (px, py) in enumerate(pairs):
        cost, path = R.replay(px, py, np.float32)
        assert_equals(got, cost, path, b)
    for big in (dx, dy):
        big[torch.isnan(big)] = 1e30
    again = warp(x, y, al, nl)
    for a, b_ in zip(got, again):
        assert a.tobytes() == b_.tobytes()


def test_equal_features_infinite_distances_and_nan_features_keep_the_path_valid():
    A, N, K = 90, 70, 13
    flat = np.ones((A, K), np.float32), np.ones((N, K), np.float32)        # every path costs 0: the tie rule alone decides
    far = np.full((A, K), 1e30, np.float32), np.full((N, K), -1e30, np.float32)       # every distance +inf
    nan = R.features("normal", A, K, 1), R.features("normal", N, K, 2)
    nan[0][::3], nan[1][1::2] = np.nan, np.nan
    allnan = np.full((A, K), np.nan, np.float32), np.full((N, K), np.nan, np.float32)
    for x, y in (flat, far, nan, allnan):
        got = warp(dev(x)[None], dev(y)[None], [A], [N])
        assert_valid(got[1][0], got[2][0], A, N)
        cost, path = R.replay(x, y, np.float32)
        assert_equals(got, cost, path)
    got = warp(dev(flat[0])[None], dev(flat[1])[None], [A], [N])
    assert got[0][0] == 0 and got[2][0] == A                                # up the first column, then the diagonal
    got = warp(dev(far[0])[None], dev(far[1])[None], [A], [N])
    assert got[0][0] == np.inf


def test_diagonal_equals_the_replay_and_refuses_unequal_lengths():
    lens = [257, 64, 1, 300]
    K = 13
    x, y = torch.full((4, 300, K), float("nan")), torch.full((4, 310, K), float("nan"))
    pairs = []
    for b, n in enumerate(lens):
        px, py = R.pair("normal", n, n, K)
        x[b, :n], y[b, :n] = torch.from_numpy(px), torch.from_numpy(py)
        pairs.append((px, py))
    got = warp(x.cuda(), y.cuda(), lens, lens, diagonal=True)
    for b, (px, py) in enumerate(pairs):
        cost, path = R.replay(px, py, np.float32, diagonal=True)
        assert_equals(got, cost, path, b)
    with pytest.raises(ValueError, match="equal lengths"):
        metrics.dtw(x.cuda(), y.cuda(), lens, [257, 64, 2, 300], diagonal=True)


def test_distortion_is_the_formula_on_the_replays_cost_and_path_length():
    """mcd = (10 / ln 10) sqrt(2) cost / path_len in float64, rounded to float32 once; both forms, ragged, with the path"""
    M, K = 80, 13
    lens = [(100, 131), (64, 64), (33, 20)]
    a, b = torch.zeros(3, M, 100), torch.zeros(3, M, 131)
    want, want_diag, paths = [], [], []
    for i, (A, N) in enumerate(lens):
        ma, mb = R.log_mel(M, A, 20 + i), R.log_mel(M, N, 30 + i)
        a[i, :, :A], b[i, :, :N] = torch.from_numpy(ma), torch.from_numpy(mb)
        cost, path = R.replay(R.cepstra(ma, K), R.cepstra(mb, K), np.float32)
        want.append(np.float32(metrics.MCD_SCALE * np.float64(cost) / np.float64(len(path))))
        paths.append(path)
        n = min(A, N)
        cost, path = R.replay(R.cepstra(ma[:, :n], K), R.cepstra(mb[:, :n], K), np.float32, diagonal=True)
        want_diag.append(np.float32(metrics.MCD_SCALE * np.float64(cost) / np.float64(n)))
    assert metrics.MCD_SCALE == 10.0 / math.log(10.0) * math.sqrt(2.0)
    al, bl = [x for x, _ in lens], [x for _, x in lens]
    mcd, path, path_len = metrics.mel_cepstral_distortion(a.cuda(), al, b.cuda(), bl, return_path=True)
    assert mcd.dtype == torch.float32 and mcd.is_cuda and tuple(mcd.shape) == (3,)
    assert mcd.cpu().numpy().tobytes() == np.array(want, np.float32).tobytes()
    for i, p in enumerate(paths):
        assert int(path_len[i]) == len(p) and np.array_equal(path[i, :len(p)].cpu().numpy(), p)
    assert torch.equal(metrics.mel_cepstral_distortion(a.cuda(), al, b.cuda(), bl), mcd)
    short = [min(x) for x in lens]
    diag = metrics.mel_cepstral_distortion(a.cuda(), short, b.cuda(), short, align=False)
    assert diag.cpu().numpy().tobytes() == np.array(want_diag, np.float32).tobytes()
    assert 1.0 < float(mcd.min()) and float(mcd.max()) < 100.0              # dB, not nepers or a sum


def test_repeated_calls_give_identical_bytes_and_one_launch_per_call(monkeypatch):
    x, y, cost, path = replay("normal", 257, 255, 13)
    for B in (1, 5, 70):
        xs, ys = dev(x)[None].expand(B, -1, -1), dev(y)[None].expand(B, -1, -1)       # stride 0 over the batch
        calls = count_calls(monkeypatch, ["ft_dtw_ragged", "ft_mel_cepstra"])
        first = warp(xs, ys, [257] * B, [255] * B)
        assert calls == {"ft_dtw_ragged": 1, "ft_mel_cepstra": 0}
        second = warp(xs, ys, [257] * B, [255] * B)
        assert calls["ft_dtw_ragged"] == 2
        for a, b in zip(first, second):
            assert a.tobytes() == b.tobytes()
        for b in range(B):
            assert_equals(first, cost, path, b)
        monkeypatch.undo()
    mel = dev(R.log_mel(80, 90, 3))[None].expand(4, -1, -1)
    calls = count_calls(monkeypatch, ["ft_dtw_ragged", "ft_mel_cepstra"])
    one = metrics.mel_cepstral_distortion(mel, [90, 80, 70, 1], mel[:, :, :77], [77, 77, 5, 1])
    assert calls == {"ft_dtw_ragged": 1, "ft_mel_cepstra": 2}
    two = metrics.mel_cepstral_distortion(mel, [90, 80, 70, 1], mel[:, :, :77], [77, 77, 5, 1])
    assert torch.equal(one, two) and float(one[3]) == 0.0


def test_more_than_max_frames_is_refused_on_the_device_too(monkeypatch):
    calls = count_calls(monkeypatch, ["ft_dtw_ragged", "ft_mel_cepstra"])
    n = metrics.MAX_FRAMES + 1
    with pytest.raises(NotImplementedError, match=str(metrics.MAX_FRAMES)):
        metrics.dtw(torch.zeros(1, n, 2).cuda(), torch.zeros(1, 4, 2).cuda(), [n], [4])
    with pytest.raises(NotImplementedError, match=str(metrics.MAX_FRAMES)):
        metrics.mel_cepstral_distortion(torch.zeros(1, 80, 4).cuda(), [4], torch.zeros(1, 80, n).cuda(), [n])
    assert calls == {"ft_dtw_ragged": 0, "ft_mel_cepstra": 0}              # refused before any launch
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.dtw(torch.zeros(1, 4, 2), torch.zeros(1, 4, 2).cuda(), [4], [4])


@pytest.fixture(scope="module")
def case():
    """synth.SMALL_MODEL_CONFIG with the coupling weights oracle.synth makes for the goldens, fp32 operand mode, a ragged batch
    of three (the size tests/test_gpu_align.py decodes)"""
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


def test_a_reconstruction_is_nearer_the_recording_than_a_fresh_sample(case):
    """mel -> alignments -> infer_aligned along the soft maps gives the mel back; a fresh residual along the same maps gives
    another utterance.  An ordering, not a number."""
    m, b, il, ol = case["m"], case["b"], case["il"], case["ol"]
    mel = b["mel"]
    z, attn, _ = m.alignments(mel, b["speaker_ids"], b["text"], b["in_lens"], b["out_lens"])
    back, lengths = m.infer_aligned(z, b["speaker_ids"], b["text"], attn, in_lens=il, n_frames=ol)
    assert lengths.tolist() == ol
    g = torch.Generator().manual_seed(5)
    fresh, _ = m.infer_aligned((0.5 * torch.randn(z.shape, generator=g)).cuda(), b["speaker_ids"], b["text"], attn, in_lens=il,
                               n_frames=ol)
    zero = metrics.mel_cepstral_distortion(mel, ol, mel, ol, align=False)
    assert torch.equal(zero, torch.zeros(3, device=mel.device))
    assert torch.equal(metrics.mel_cepstral_distortion(mel, ol, mel, ol), zero)       # the warp of a mel onto itself: the diagonal
    near = metrics.mel_cepstral_distortion(mel, ol, back, ol, align=False)
    far = metrics.mel_cepstral_distortion(mel, ol, fresh, ol, align=True)
    print("round trip %s dB, fresh sample %s dB" % (near.tolist(), far.tolist()))
    assert torch.isfinite(near).all() and torch.isfinite(far).all()
    assert (near < far).all()
