"""Mel-cepstral distortion and dynamic time warping without a GPU: the numpy restatement (tests/dtw_ref.py) against brute force
over every warping path, its float32 against its float64 form, the DCT table, the properties a warp must have, the refusals
of flowtron_amd.metrics and of the C entries of csrc/dtw.hip before anything reaches the device, and the sharpness of the
inputs the GPU tests use."""
import time

import numpy as np
import pytest
import torch

import dtw_ref as R
from flowtron_amd import metrics

U = 2.0 ** -24                                    # unit roundoff of float32


def assert_valid(path, A, N):
    assert tuple(path[0]) == (0, 0) and tuple(path[-1]) == (A - 1, N - 1)
    steps = {tuple(s) for s in np.diff(path, axis=0).tolist()}
    assert steps <= {(1, 1), (1, 0), (0, 1)}, steps


def test_replay_equals_brute_force_and_takes_the_lowest_move_from_the_end_backwards():
    """every Ta, Tb <= 5, K = 1, multiples of 1/8, four seeds each: all sums are exact in both precisions, so the replay's cost IS
    the least cost over all paths, and its path is the one the tie rule singles out"""
    tied = 0
    for A in range(1, 6):
        for N in range(1, 6):
            for seed in range(4):
                x, y = R.features("grid", A, 1, 100 * A + 10 * N + seed), R.features("grid", N, 1, 7000 + 100 * A + 10 * N + seed)
                best, best_path, n_best = R.brute_force(x, y)
                tied += n_best > 1
                for dtype in (np.float32, np.float64):
                    cost, path = R.replay(x, y, dtype)
                    assert_valid(path, A, N)
                    assert float(cost) == best and float(R.path_cost(x, y, path)) == best, (A, N, seed)
                    assert np.array_equal(path, best_path), (A, N, seed, path.tolist(), best_path.tolist())
    print("%d of 100 cases have more than one cheapest path" % tied)
    assert tied >= 25                             # the tie rule was exercised, not merely stated


def test_float32_and_float64_replays_agree_on_log_mel_like_data():
    """862 x 700 frames, K 13 cepstra of N(-5, 2^2) frames.  The float32 cost of ANY path is within (P + (K + 5) / 2) u of its
    float64 cost, relative, P <= A + N - 1 cells: a distance's K subtractions, products and sums and its root add up to
    (K + 5) / 2 roundings at first order, every add along the path one more.  Two minima over the same set of paths whose
    members differ by at most that much differ by at most that much, whichever paths attain them."""
    A, N, K = 862, 700, 13
    x, y = R.cepstra(R.log_mel(80, A, 1), K), R.cepstra(R.log_mel(80, N, 2), K)
    t0 = time.perf_counter()
    c32, p32 = R.replay(x, y, np.float32)
    took = time.perf_counter() - t0
    c64, p64 = R.replay(x, y, np.float64)
    assert c32.dtype == np.float32 and c64.dtype == np.float64
    assert_valid(p32, A, N)
    assert_valid(p64, A, N)
    rel = abs(float(c32) - float(c64)) / float(c64)
    print("862 x 700: cost %.6f, relative difference %.3e, paths of %d and %d cells, float32 replay %.2f s" % (c64, rel, len(p32), len(p64), took))
    assert rel <= 1.01 * (A + N - 1 + (K + 5) / 2) * U
    # on the exact grid the two agree on the path as well
    x, y = R.features("grid", 300, 1, 5), R.features("grid", 257, 1, 6)
    c32, p32 = R.replay(x, y, np.float32)
    c64, p64 = R.replay(x, y, np.float64)
    assert float(c32) == float(c64) and np.array_equal(p32, p64)


@pytest.mark.parametrize("M,K", [(80, 13), (128, 32), (80, 1), (33, 32)])
def test_dct_rows_are_orthonormal_and_the_float32_cepstra_stay_near_float64(M, K):
    D = R.dct_table(M, K)
    assert D.dtype == np.float32 and D.shape == (K, M)
    assert np.abs(D.astype(np.float64) @ D.astype(np.float64).T - np.eye(K)).max() < 1e-6
    c0 = np.full(M, np.sqrt(1.0 / M))             # the row left out: the others are orthogonal to it
    assert np.abs(D.astype(np.float64) @ c0).max() < 1e-6
    assert torch.equal(metrics.dct_table(M, K), torch.from_numpy(D))
    mel = R.log_mel(M, 50, M + K)
    c32, c64 = R.cepstra(mel, K, np.float32), R.cepstra(mel, K, np.float64)
    assert c32.dtype == np.float32 and c32.shape == (50, K)
    terms = np.abs(mel.astype(np.float64).T[:, None, :] * D.astype(np.float64)[None, :, :]).sum(2)        # [T, K]
    assert np.all(np.abs(c32.astype(np.float64) - c64) <= M * U * terms)


def test_a_sequence_against_itself_and_against_its_stretched_copy():
    x = R.features("normal", 37, 13, 3)
    for dtype in (np.float32, np.float64):
        cost, path = R.replay(x, x, dtype)
        assert cost == 0 and np.array_equal(path, np.stack([np.arange(37)] * 2, 1))
        for r in (2, 3):
            cost, path = R.replay(x, np.repeat(x, r, axis=0), dtype)
            assert cost == 0 and len(path) == r * 37
            assert np.array_equal(path[:, 0], np.arange(r * 37) // r) and np.array_equal(path[:, 1], np.arange(r * 37))
            cost, path = R.replay(np.repeat(x, r, axis=0), x, dtype)
            assert cost == 0 and np.array_equal(path[:, 1], np.arange(r * 37) // r)


def test_diagonal_is_the_running_float32_sum():
    x, y = R.features("normal", 91, 13, 4), R.features("normal", 91, 13, 5)
    cost, path = R.replay(x, y, np.float32, diagonal=True)
    d = R.distances(x, y, np.float32)
    run = np.float32(0)
    for i in range(91):
        run = np.float32(d[i, i] + run)
    assert cost.dtype == np.float32 and cost.tobytes() == run.tobytes()
    assert np.array_equal(path, np.stack([np.arange(91)] * 2, 1))
    assert float(cost) >= float(R.replay(x, y, np.float64)[0]) * (1 - 200 * U)      # the warp can only be cheaper


@pytest.mark.parametrize("wrong", ["ties", "strict", "fma", "descending", "c0"])
def test_wrong_references_differ_from_the_replay_on_the_test_inputs(wrong):
    """the shapes and inputs of tests/test_gpu_metrics.py tell the rule from its neighbours: each wrong reference gives another
    cost (bit for bit) or another path than the replay on at least one of them.  A single rounding inside one distance often
    vanishes in the sum along a short path; the long shapes catch it."""
    if wrong == "c0":
        mel = R.log_mel(80, 40, 9)
        a, b = R.cepstra(mel, 13), R.cepstra(mel, 13, c0=True)
        assert np.array_equal(a[:, :12], b[:, 1:]) and not np.array_equal(a, b)
        return
    kind, K = ("grid", 1) if wrong in ("ties", "strict") else ("normal", 13)
    kw = dict(ties="high") if wrong == "ties" else {wrong: True} if wrong != "strict" else dict(strict=False)
    shown = []
    for A, N in R.SHAPES:
        x, y = R.pair(kind, A, N, K)
        right, other = R.replay(x, y), R.replay(x, y, **kw)
        if kind == "grid":
            assert right[0] == other[0]           # exact sums: the same least cost, whichever path
        if right[0].tobytes() != other[0].tobytes() or not np.array_equal(right[1], other[1]):
            shown.append((A, N))
    print("%s: differs at %s" % (wrong, shown))
    assert shown


def test_refusals_are_raised_without_a_device():
    mel = torch.zeros(2, 80, 30)
    x, y = torch.zeros(2, 30, 13), torch.zeros(2, 20, 13)
    for call in (lambda: metrics.mel_cepstra(mel), lambda: metrics.mel_cepstra(mel, [30, 7]),
                 lambda: metrics.dtw(x, y, [30, 4], [20, 20]),
                 lambda: metrics.mel_cepstral_distortion(mel, [30, 30], mel[:, :, :20], [20, 9])):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="float32"):
        metrics.mel_cepstra(mel.double())
    with pytest.raises(ValueError, match="float32"):
        metrics.dtw(x.half(), y.half(), [30, 4], [20, 20])
    with pytest.raises(ValueError, match="float32"):
        metrics.mel_cepstral_distortion(mel, None, mel.double(), None)
    with pytest.raises(ValueError, match="B, M, T"):
        metrics.mel_cepstra(mel[0])
    with pytest.raises(ValueError, match="B, M, T"):
        metrics.mel_cepstral_distortion(mel, None, mel[0], None)
    with pytest.raises(ValueError, match="B, T, K"):
        metrics.dtw(x[0], y, [30], [20, 20])
    with pytest.raises(ValueError, match="one pair per utterance"):
        metrics.dtw(x, y[:1], [30, 4], [20])
    with pytest.raises(ValueError, match="one pair per utterance"):
        metrics.mel_cepstral_distortion(mel, None, mel[:1], None)
    with pytest.raises(ValueError, match="features per frame"):
        metrics.dtw(x, y[:, :, :12], [30, 4], [20, 20])
    with pytest.raises(ValueError, match="mel channels"):
        metrics.mel_cepstral_distortion(mel, None, mel[:, :40], None)
    for bad in (0, 33, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="n_coeffs"):
            metrics.mel_cepstra(mel, n_coeffs=bad)
        with pytest.raises(ValueError, match="n_coeffs"):
            metrics.mel_cepstral_distortion(mel, None, mel, None, n_coeffs=bad)
    with pytest.raises(ValueError, match="n_coeffs"):
        metrics.mel_cepstra(mel[:, :13], n_coeffs=13)                      # K must stay below M
    with pytest.raises(ValueError, match="lens"):
        metrics.mel_cepstra(mel, [30, 31])
    with pytest.raises(ValueError, match="x_lens"):
        metrics.dtw(x, y, [30, 0], [20, 20])
    with pytest.raises(ValueError, match="y_lens"):
        metrics.dtw(x, y, [30, 4], torch.tensor([20.0, 20.0]))
    with pytest.raises(ValueError, match="b_lens"):
        metrics.mel_cepstral_distortion(mel, [30, 30], mel, [30])
    with pytest.raises(ValueError, match="equal lengths"):
        metrics.dtw(x, y, [20, 4], [20, 5], diagonal=True)
    with pytest.raises(ValueError, match="equal lengths"):
        metrics.mel_cepstral_distortion(mel, [30, 12], mel, [30, 13], align=False)
    assert metrics.MAX_FRAMES == 1024
    big = torch.zeros(1, 80, metrics.MAX_FRAMES + 1)
    with pytest.raises(NotImplementedError, match="1024"):
        metrics.mel_cepstral_distortion(big, None, mel[:1], None)
    with pytest.raises(NotImplementedError, match="1024"):
        metrics.mel_cepstral_distortion(mel[:1], None, big, None)
    with pytest.raises(NotImplementedError, match="1024"):
        metrics.dtw(torch.zeros(1, 1025, 2), torch.zeros(1, 5, 2), [1025], [5])
    with pytest.raises(NotImplementedError, match="1024"):
        metrics.mel_cepstral_distortion(big, [7], big, [7], align=False)


def test_c_abi_refuses_bad_arguments_before_the_device():
    """FT_EINVAL / FT_EUNSUPPORTED from the entry points themselves, with host memory standing in for the buffers: nothing may
    be launched"""
    import ctypes as C
    from flowtron_amd import _lib as L
    lib = L.lib()
    assert lib.ft_dtw_workspace_bytes(1, 1, 1, 1) == 16
    assert lib.ft_dtw_workspace_bytes(2, 6, 4, 13) == 2 * 9 * 1 * 16
    assert lib.ft_dtw_workspace_bytes(3, 10, 65, 1) == 3 * 74 * 2 * 16
    assert lib.ft_dtw_workspace_bytes(64, 862, 862, 13) == 64 * 1723 * 14 * 16
    assert lib.ft_dtw_workspace_bytes(1, 1024, 1024, 32) == 2047 * 16 * 16
    for bad in ((0, 6, 4, 2), (2, 0, 4, 2), (2, 6, 0, 2), (2, 6, 4, 0), (-1, 6, 4, 2)):
        assert lib.ft_dtw_workspace_bytes(*bad) == 0

    x = (C.c_float * 24)()
    y = (C.c_float * 16)()
    lens = (C.c_int32 * 2)()
    cost = (C.c_float * 2)()
    plen = (C.c_int32 * 2)()
    path = (C.c_int32 * 36)()
    work = (C.c_uint64 * 38)()
    base = C.addressof(work) + (-C.addressof(work)) % 16
    a_ = dict(x=C.addressof(x), y=C.addressof(y), xl=C.addressof(lens), yl=C.addressof(lens), cost=C.addressof(cost),
              plen=C.addressof(plen), path=C.addressof(path), work=base)
    ok = dict(a_, sx=(12, 2, 1), sy=(8, 2, 1), wb=288, B=2, Ta=6, Tb=4, K=2, diag=0)

    def dtw(**kw):
        a = dict(ok, **kw)
        return lib.ft_dtw_ragged(a["x"], *a["sx"], a["y"], *a["sy"], a["xl"], a["yl"], a["cost"], a["plen"], a["path"], a["work"],
                                 a["wb"], a["B"], a["Ta"], a["Tb"], a["K"], a["diag"], None)
    for kw in (dict(x=None), dict(y=None), dict(xl=None), dict(yl=None), dict(cost=None), dict(plen=None), dict(path=None),
               dict(work=None), dict(B=0), dict(Ta=0), dict(Tb=0), dict(K=0), dict(B=-3), dict(sx=(-1, 2, 1)), dict(sx=(12, -2, 1)),
               dict(sy=(8, 2, -1)), dict(wb=287), dict(wb=0), dict(Ta=7), dict(work=base + 8)):
        assert dtw(**kw) == -1, kw
        assert b"ft_dtw_ragged" in lib.ft_last_error()
    for kw in (dict(Ta=1025), dict(Tb=1025), dict(K=33)):                  # FT_EUNSUPPORTED: beyond the limits
        assert dtw(wb=1 << 30, **kw) == -3, kw
        assert b"ft_dtw_ragged" in lib.ft_last_error() and (b"1024" in lib.ft_last_error() or b"32" in lib.ft_last_error())

    mel = (C.c_float * 64)()
    dct = (C.c_float * 16)()
    cep = (C.c_float * 16)()
    okc = dict(mel=C.addressof(mel), s=(32, 4, 1), lens=C.addressof(lens), dct=C.addressof(dct), cep=C.addressof(cep), B=2, M=8, T=4, K=2)

    def cepstra(**kw):
        a = dict(okc, **kw)
        return lib.ft_mel_cepstra(a["mel"], *a["s"], a["lens"], a["dct"], a["cep"], a["B"], a["M"], a["T"], a["K"], None)
    for kw in (dict(mel=None), dict(dct=None), dict(cep=None), dict(B=0), dict(M=0), dict(T=0), dict(K=0), dict(s=(32, -4, 1)),
               dict(B=65536)):
        assert cepstra(**kw) == -1, kw
        assert b"ft_mel_cepstra" in lib.ft_last_error()
    for kw in (dict(K=8), dict(K=9), dict(K=33, M=64), dict(M=129)):       # K >= M, K > 32, M > 128
        assert cepstra(**kw) == -3, kw
        assert b"ft_mel_cepstra" in lib.ft_last_error()
