"""Alignment search and pace control without a GPU: the numpy restatement of the search (tests/align_ref.py) against brute
force over every monotone path, the host arithmetic of scale_durations, and the argument errors the three C entries of
csrc/align.hip raise before anything reaches the device."""
import math

import numpy as np
import pytest
import torch

import align_ref as R
from flowtron_amd import align

SHAPES = [(T, L) for T in range(1, 11) for L in range(1, min(T, 5) + 1)]
KINDS = ("normal", "grid", "grid_inf")


def scores(kind, T, L, seed):
    rs = np.random.RandomState(seed)
    if kind == "normal":
        return rs.standard_normal((T, L)).astype(np.float32)
    s = (-rs.randint(0, 17, size=(T, L)) / 8.0).astype(np.float32)          # multiples of 1/8 in [-2, 0]: ties everywhere
    if kind == "grid_inf":
        s[rs.random_sample((T, L)) < 0.3] = -np.inf
    return s


def assert_valid(path, dur, T, L):
    assert path.shape == (T,) and path[0] == 0 and path[-1] == L - 1
    assert set(np.diff(path).tolist()) <= {0, 1}
    assert dur.shape == (L,) and dur.min() >= 1 and dur.sum() == T
    assert np.array_equal(dur, np.bincount(path, minlength=L))


@pytest.mark.parametrize("kind", KINDS)
def test_replay_equals_brute_force_and_takes_the_earliest_advancing_best_path(kind):
    """For every T <= 10, L <= min(T, 5), five seeds each: the replay's score is the brute-force maximum, and its path is the
    lexicographically greatest of the paths that reach it.  Where NO path has a finite score (the -inf kind: 30 % of the
    entries, so s[0][0] alone rules out 30 % of the cases) every path is 'best', the maximum is -inf, and the rule promises
    structural validity only -- a finite prefix still steers it; those cases are checked for the score and validity.  Both
    classes must occur in the -inf kind (52 of its 200 cases have a finite best path)."""
    finite = total = 0
    for T, L in SHAPES:
        for seed in range(5):
            s = scores(kind, T, L, 1000 * T + 10 * L + seed)
            best, best_path = R.brute_force(s)
            for dtype in (np.float32, np.float64):
                path, dur, score = R.replay(s, dtype)
                assert_valid(path, dur, T, L)
                own = R.path_score(s, path)                                             # what the returned path itself scores
                if kind == "normal" and dtype == np.float32:
                    # T - 1 fp32 adds, each within 2^-24 of a partial sum that is at most sum |s|: near-ties may resolve otherwise
                    bound = T * 2.0 ** -24 * float(np.abs(s).sum())
                    assert abs(float(score) - own) <= bound and best - own <= 2 * bound, (T, L, seed)
                else:
                    assert float(score) == best and own == best, (T, L, seed)       # grid sums are exact in fp32 too
                    if np.isfinite(best):
                        assert np.array_equal(path, best_path), (T, L, seed, path, best_path)
            total += 1
            finite += bool(np.isfinite(best))
    assert total == 5 * len(SHAPES)
    print(kind, "cases with a finite best path:", finite, "of", total)
    assert finite == total if kind != "grid_inf" else 0 < finite < total, (finite, total)


@pytest.mark.parametrize("kind", ("grid", "grid_inf"))
def test_float32_and_float64_replays_agree_exactly_on_grid_scores(kind):
    """sums of fewer than 2^14 multiples of 1/8 in [-2, 0] are exact in fp32: an identity, not a tolerance"""
    for T, L in SHAPES + [(40, 17), (64, 64), (130, 65)]:
        s = scores(kind, T, L, 7 * T + L)
        p32, d32, q32 = R.replay(s, np.float32)
        p64, d64, q64 = R.replay(s, np.float64)
        assert np.array_equal(p32, p64) and np.array_equal(d32, d64)
        assert q32.dtype == np.float32 and q64.dtype == np.float64 and float(q32) == float(q64)


def test_path_is_structurally_valid_when_every_score_is_minus_infinity():
    for T, L in SHAPES + [(70, 65)]:
        s = np.full((T, L), -np.inf, np.float32)
        path, dur, score = R.replay(s)
        assert_valid(path, dur, T, L)
        assert score == -np.inf
        assert np.array_equal(path, np.minimum(np.arange(T), L - 1))     # all paths tie: the earliest advancing one


def _ends(d):
    return np.cumsum(np.asarray(d, np.int64))


def test_scale_durations_is_the_identity_at_pace_one():
    rs = np.random.RandomState(3)
    d = torch.from_numpy(rs.randint(1, 9, size=(4, 12)).astype(np.int32))
    il = [12, 7, 1, 9]
    out, totals = align.scale_durations(d, il, 1.0)
    assert out.dtype == torch.int32 and totals.dtype == torch.int64 and tuple(totals.shape) == (4,)
    for b in range(4):
        assert torch.equal(out[b, :il[b]], d[b, :il[b]]) and int(out[b, il[b]:].abs().sum()) == 0
        assert int(totals[b]) == int(d[b, :il[b]].sum())
    out3, _ = align.scale_durations(d, il, 1.0, min_frames=3)             # not the identity where a token is shorter than 3
    assert int(out3[0, :12].min()) >= 3


@pytest.mark.parametrize("min_frames", [0, 1, 2])
def test_scale_durations_totals_and_monotone_ends(min_frames):
    """total = max(floor(T / pace + 0.5), what min_frames forces): the forced part in closed form is
    max_j (round(e_j / pace) + (L_b - 1 - j) min_frames) over j = -1 .. L_b - 1 with e_{-1} = 0."""
    rs = np.random.RandomState(5)
    d = rs.randint(0, 12, size=(5, 20)).astype(np.int64)
    il = [20, 13, 5, 1, 17]
    for pace in (0.5, 0.8, 1.0, 1.25, 2.0, 3.7, 40.0):
        out, totals = align.scale_durations(torch.from_numpy(d), il, pace, min_frames=min_frames)
        for b in range(5):
            e = _ends(d[b, :il[b]])
            r = [0] + [int(math.floor(x / pace + 0.5)) for x in e]
            want = max(r[j + 1] + (il[b] - 1 - j) * min_frames for j in range(-1, il[b]))
            assert want >= int(math.floor(int(e[-1]) / pace + 0.5))
            assert int(totals[b]) == want, (pace, b)
            o = out[b].numpy().astype(np.int64)
            assert o[:il[b]].min() >= min_frames and o[il[b]:].sum() == 0
            assert np.all(np.diff(np.concatenate([[0], _ends(o[:il[b]])])) >= min_frames)      # ends are monotone
            assert _ends(o[:il[b]])[-1] == want
            # every end lies at its rounded place unless min_frames pushed it later
            assert np.all(_ends(o[:il[b]]) >= np.array(r[1:]))


def test_scale_durations_takes_one_pace_per_utterance_and_refuses_bad_arguments():
    d = torch.tensor([[4, 4, 4, 4], [4, 4, 4, 4], [4, 4, 0, 0]], dtype=torch.int32)
    il = [4, 4, 2]
    out, totals = align.scale_durations(d, il, [0.5, 2.0, 1.0])
    assert totals.tolist() == [32, 8, 8]
    assert out.tolist() == [[8, 8, 8, 8], [2, 2, 2, 2], [4, 4, 0, 0]]
    same, _ = align.scale_durations(d, il, torch.tensor([0.5, 2.0, 1.0]))
    assert torch.equal(same, out)
    for bad in (0.0, -1.0, float("nan"), float("inf"), [1.0, 1.0], "fast", True):
        with pytest.raises(ValueError, match="pace"):
            align.scale_durations(d, il, bad)
    with pytest.raises(ValueError, match="min_frames"):
        align.scale_durations(d, il, 1.0, min_frames=-1)
    with pytest.raises(ValueError, match="in_lens"):
        align.scale_durations(d, [4, 4, 5], 1.0)
    with pytest.raises(ValueError, match="integers"):
        align.scale_durations(d.float(), il, 1.0)


def test_device_entries_refuse_host_tensors_and_impossible_lengths():
    lp = torch.zeros(2, 6, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        align.monotonic_alignment(lp, [4, 2], [6, 5])
    with pytest.raises(ValueError, match="in_lens 4 > out_lens 3"):
        align.monotonic_alignment(lp, [4, 2], [3, 5])
    with pytest.raises(ValueError, match="out_lens"):
        align.monotonic_alignment(lp, [4, 2], [7, 5])
    with pytest.raises(ValueError, match="float32"):
        align.monotonic_alignment(lp.double(), [4, 2], [6, 5])
    with pytest.raises(ValueError, match="B, T, L"):
        align.monotonic_alignment(lp[0], [4], [6])
    with pytest.raises(NotImplementedError, match="1024"):
        align.monotonic_alignment(torch.zeros(1, 1030, 1025), [1025], [1030])
    d = torch.ones(2, 4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        align.durations_to_alignment(d, [4, 2])
    with pytest.raises(ValueError, match="n_frames"):
        align.durations_to_alignment(d, [4, 2], n_frames=0)
    with pytest.raises(ValueError, match="integers"):
        align.durations_to_alignment(d.float(), [4, 2])


def test_c_abi_refuses_bad_arguments_before_the_device():
    """FT_EINVAL / FT_EUNSUPPORTED from the entry points themselves, with host memory standing in for the buffers: nothing may
    be launched"""
    import ctypes as C
    from flowtron_amd import _lib as L
    lib = L.lib()
    assert lib.ft_mas_workspace_bytes(2, 6, 4) == 2 * 6 * 1 * 8
    assert lib.ft_mas_workspace_bytes(3, 10, 65) == 3 * 10 * 2 * 8
    assert lib.ft_mas_workspace_bytes(64, 862, 190) == 64 * 862 * 3 * 8
    assert lib.ft_mas_workspace_bytes(1, 1030, 1024) == 1030 * 16 * 8
    for bad in ((0, 6, 4), (2, 0, 4), (2, 6, 0), (-1, 6, 4)):
        assert lib.ft_mas_workspace_bytes(*bad) == 0

    lp = (C.c_float * 48)()
    lens = (C.c_int32 * 2)()
    path = (C.c_int32 * 12)()
    dur = (C.c_int32 * 8)()
    score = (C.c_float * 2)()
    work = (C.c_uint64 * 12)()
    a_ = {k: C.addressof(v) for k, v in dict(lp=lp, il=lens, ol=lens, path=path, dur=dur, score=score, work=work).items()}
    ok = dict(a_, sb=24, st=4, sl=1, wb=96, B=2, T=6, L=4)

    def mas(**kw):
        a = dict(ok, **kw)
        return lib.ft_mas_ragged(a["lp"], a["sb"], a["st"], a["sl"], a["il"], a["ol"], a["path"], a["dur"], a["score"], a["work"],
                                 a["wb"], a["B"], a["T"], a["L"], None)
    for kw in (dict(lp=None), dict(il=None), dict(ol=None), dict(path=None), dict(dur=None), dict(work=None), dict(B=0), dict(T=0),
               dict(L=0), dict(B=-3), dict(sb=-1), dict(st=-1), dict(sl=-1), dict(wb=95), dict(wb=0), dict(T=7),
               dict(work=a_["work"] + 4)):
        assert mas(**kw) == -1, kw
        assert b"ft_mas_ragged" in lib.ft_last_error()
    assert mas(L=1025, wb=1 << 20) == -3                                   # FT_EUNSUPPORTED: beyond the text limit
    assert b"ft_mas_ragged" in lib.ft_last_error() and b"1024" in lib.ft_last_error()

    rows = (C.c_float * 48)()
    okr = dict(dur=a_["dur"], il=a_["il"], rows=C.addressof(rows), B=2, N=6, L=4, rev=0)

    def expand(**kw):
        a = dict(okr, **kw)
        return lib.ft_durations_to_rows(a["dur"], a["il"], a["rows"], a["B"], a["N"], a["L"], a["rev"], None)
    for kw in (dict(dur=None), dict(il=None), dict(rows=None), dict(B=0), dict(N=0), dict(L=0), dict(N=-2)):
        assert expand(**kw) == -1, kw
        assert b"ft_durations_to_rows" in lib.ft_last_error()
