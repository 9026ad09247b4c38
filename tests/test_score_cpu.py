"""CPU checks of utterance scoring (csrc/score.hip, flowtron_amd/score.py): the NumPy replays (tests/score_ref.py) against
brute-force definitions and hand-written maps whose counters are known by inspection, the argument checks of the C entries,
which return FT_EINVAL before any device call, the host-side length checks, and the refusals of Flowtron.log_likelihood."""
import ctypes

import numpy as np
import pytest
import torch

import score_ref as R
from flowtron_amd import _lib as L
from flowtron_amd import score


def one_hot(peaks, L_):
    a = np.zeros((len(peaks), L_), np.float32)
    a[np.arange(len(peaks)), peaks] = 1.0
    return a


# (name, map [T, L], the six counters by inspection)
HAND = [
    ("clean staircase", one_hot([0, 0, 1, 2, 2, 2, 3], 4),
     dict(n_attended=4, n_backward=0, n_skipped=0, longest_run=3, first_peak=0, last_peak=3)),
    ("repeated block", one_hot([0, 1, 2, 1, 2, 3], 4),
     dict(n_attended=4, n_backward=1, n_skipped=0, longest_run=1, first_peak=0, last_peak=3)),
    ("jumps over two tokens", one_hot([0, 1, 4, 4, 5], 6),
     dict(n_attended=4, n_backward=0, n_skipped=2, longest_run=2, first_peak=0, last_peak=5)),
    ("stops short", one_hot([0, 1, 1, 2, 2, 2, 2], 5),
     dict(n_attended=3, n_backward=0, n_skipped=0, longest_run=4, first_peak=0, last_peak=2)),
    ("an all-zero row", np.array([[0, 1, 0], [0, 0, 0], [0, 0, 1]], np.float32),
     dict(n_attended=3, n_backward=1, n_skipped=1, longest_run=1, first_peak=1, last_peak=2)),
    ("exact ties", np.array([[.5, .5, 0], [.25, .5, .5], [0, .5, .5], [.25, .25, .5]], np.float32),
     dict(n_attended=3, n_backward=0, n_skipped=0, longest_run=2, first_peak=0, last_peak=2)),
]


@pytest.mark.parametrize("name,a,want", HAND, ids=[h[0] for h in HAND])
def test_replay_gives_the_counters_known_by_inspection(name, a, want):
    T, L_ = a.shape
    peaks, counters, focus = R.attn_diagnostics(a[None, None], [L_], [T])
    assert dict(zip(R.COUNTERS, counters[0, 0].tolist())) == want
    assert [R.peak_brute(r)[0] for r in a] == peaks[0, 0].tolist()
    assert focus[0, 0] == np.sum([np.float64(R.peak_brute(r)[1]) for r in a])    # (these sums are exact in any order)
    # a longer tensor around it changes nothing: the lengths cut it
    big = np.full((1, 1, T + 2, L_ + 3), np.nan, np.float32)
    big[0, 0, :T, :L_] = a
    p2, c2, f2 = R.attn_diagnostics(big, [L_], [T])
    assert np.array_equal(p2[0, 0, :T], peaks[0, 0]) and np.all(p2[0, 0, T:] == -1)
    assert np.array_equal(c2, counters) and f2[0, 0] == focus[0, 0]


def test_peak_rule_against_the_sequential_definition():
    rs = np.random.RandomState(0)
    rows = [rs.randint(0, 4, size=rs.randint(1, 9)).astype(np.float32) / 4 for _ in range(200)]
    rows += [np.array(r, np.float32) for r in ([np.nan], [np.nan, np.nan], [np.nan, 1, 1], [1, np.nan, 2], [-np.inf, -np.inf],
                                               [-np.inf, np.nan, -3], [0, -0.0], [-0.0, 0], [np.inf, np.inf], [np.nan, -np.inf])]
    for r in rows:
        got, want = R.peak_of(r), R.peak_brute(r)
        assert got[0] == want[0] and np.array([got[1]]).tobytes() == np.array([want[1]]).tobytes(), r
    assert R.peak_of(np.array([np.nan, 1, 1], np.float32))[0] == 1               # NaN never wins
    assert R.peak_of(np.zeros(5, np.float32))[0] == 0                            # an all-zero row peaks at 0


@pytest.mark.parametrize("M,T,n_ls", [(1, 1, 1), (3, 5, 2), (65, 4, 3), (128, 3, 1), (80, 300, 2)])
def test_likelihood_replay_against_the_definition(M, T, n_ls):
    rs = np.random.RandomState(M + T)
    B = 3
    z = rs.standard_normal((T, B, M)).astype(np.float32)
    wide = [rs.standard_normal((T, B, 2 * M)).astype(np.float32) * 0.3 for _ in range(n_ls)]
    ls = [w[:, :, M:] for w in wide]                                             # strided views, as the coupling outputs
    rev = [f % 2 == 1 for f in range(n_ls)]
    lens = [T, 1, max(T // 2, 1)]
    for sigma in (1.0, 0.7):
        fl, tot = R.frame_loglik(z, ls, rev, lens, sigma)
        bl, bt = R.frame_loglik_brute(z, ls, rev, lens, sigma)
        scale = np.abs(bl).max()
        assert np.abs(fl - bl).max() <= 64 * np.finfo(np.float64).eps * scale * (n_ls + 1)
        assert np.abs(tot - bt).max() <= 64 * np.finfo(np.float64).eps * scale * T
        for b in range(B):
            assert np.all(fl[b, lens[b]:] == 0.0)
            one = R.frame_loglik(z[:, b:b + 1], [x[:, b:b + 1] for x in ls], rev, lens[b:b + 1], sigma)
            assert one[0].tobytes() == fl[b:b + 1].tobytes() and one[1].tobytes() == tot[b:b + 1].tobytes()
    if n_ls >= 2 and T >= 3:                                                     # the flag moves frames, not the total's terms
        other = R.frame_loglik(z, ls, [not r for r in rev], lens, 1.0)
        assert not np.array_equal(other[0], R.frame_loglik(z, ls, rev, lens, 1.0)[0])


def test_abi_version_stays_15():
    assert L.lib().ft_abi_version() == 15


# Dummy host addresses: every call below fails its argument check and returns before any pointer is used or any device call
# is made (tests/test_stft_pow2_cpu.py).
P = 4096
FT_EINVAL = -1                                                # include/flowtron_hip.h


def _loglik(**over):
    a = dict(z=P, n_ptrs=1, log_s=True, rev=True, n_ls=1, ld=80, lens=P, sigma=1.0, frame_ll=P, total=P, T=4, B=2, M=80, null_entry=False)
    a.update(over)
    k = max(a["n_ptrs"], 1)
    ptrs = (ctypes.c_void_p * k)(*[None if a["null_entry"] else P] * k)
    rev = (ctypes.c_int32 * k)(*[0] * k)
    return L.lib().ft_frame_loglik(a["z"], ptrs if a["log_s"] else None, rev if a["rev"] else None, a["n_ls"], a["ld"], a["lens"],
                                   a["sigma"], a["frame_ll"], a["total"], a["T"], a["B"], a["M"], None)


def _diag(**over):
    a = dict(attn=P, sf=0, sb=1000, st=10, sl=1, il=P, ol=P, peaks=P, counters=P, focus=P, work=P, work_bytes=1 << 20, F=2, B=3, T=7, L=10)
    a.update(over)
    return L.lib().ft_attn_diagnostics(a["attn"], a["sf"], a["sb"], a["st"], a["sl"], a["il"], a["ol"], a["peaks"], a["counters"],
                                       a["focus"], a["work"], a["work_bytes"], a["F"], a["B"], a["T"], a["L"], None)


@pytest.mark.parametrize("fn,bad", [
    (_loglik, dict(z=None)), (_loglik, dict(log_s=False)), (_loglik, dict(rev=False)), (_loglik, dict(lens=None)),
    (_loglik, dict(frame_ll=None)), (_loglik, dict(total=None)), (_loglik, dict(null_entry=True)),
    (_loglik, dict(n_ls=0)), (_loglik, dict(n_ls=9, n_ptrs=9)), (_loglik, dict(M=0)), (_loglik, dict(M=129, ld=129)),
    (_loglik, dict(ld=79)), (_loglik, dict(B=0)), (_loglik, dict(B=65536)), (_loglik, dict(T=0)),
    (_loglik, dict(sigma=0.0)), (_loglik, dict(sigma=-1.0)), (_loglik, dict(sigma=float("nan"))), (_loglik, dict(sigma=float("inf"))),
    (_loglik, dict(sigma=1e-200)),
    (_diag, dict(attn=None)), (_diag, dict(il=None)), (_diag, dict(ol=None)), (_diag, dict(peaks=None)), (_diag, dict(counters=None)),
    (_diag, dict(focus=None)), (_diag, dict(work=None)), (_diag, dict(F=0)), (_diag, dict(B=0)), (_diag, dict(T=0)), (_diag, dict(L=0)),
    (_diag, dict(F=65536)), (_diag, dict(st=-1)), (_diag, dict(work=P + 2)), (_diag, dict(work_bytes=2 * 3 * 4 - 1)),
])
def test_c_entries_reject_bad_arguments(fn, bad):
    name = {_loglik: b"ft_frame_loglik:", _diag: b"ft_attn_diagnostics:"}[fn]
    assert fn(**bad) == FT_EINVAL, bad
    err = L.lib().ft_last_error()
    assert err.startswith(name) and b"invalid argument" in err, err


def test_workspace_bytes_is_host_arithmetic():
    f = L.lib().ft_attn_diagnostics_workspace_bytes
    assert f(2, 3, 10) == 2 * 3 * 4 and f(1, 1, 32) == 4 and f(1, 1, 33) == 8 and f(0, 3, 10) == 0 and f(2, 3, 0) == 0


def test_host_side_checks_raise_value_error():
    a = torch.zeros(2, 3, 7, 10)
    for il, ol in (([10, 10], [7, 7, 7]), ([10, 10, 11], [7, 7, 7]), ([10, 10, 10], [7, 0, 7]), ([10, 10, 10], [7, 8, 7]),
                   ([10, 10, 1.5], [7, 7, 7]), (torch.tensor([10., 10., 10.]), [7, 7, 7]), (None, [7, 7, 7]),
                   ([10, 10, 10], torch.tensor([[7, 7, 7]]))):
        with pytest.raises(ValueError):
            score.attention_diagnostics(a, il, ol)
    with pytest.raises(ValueError, match="float32"):
        score.attention_diagnostics(a.double(), [10] * 3, [7] * 3)
    with pytest.raises(ValueError, match=r"\[F, B, T, L\]"):
        score.attention_diagnostics(a[0, 0], [10], [7])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        score.attention_diagnostics(a, [10] * 3, [7] * 3)
    z, ls = torch.zeros(5, 2, 8), [torch.zeros(5, 2, 8)]
    for kw in (dict(out_lens=[5]), dict(out_lens=[5, 6]), dict(out_lens=[5, 0]), dict(out_lens=None), dict(out_lens=[5, 5], sigma=0.0),
               dict(out_lens=[5, 5], sigma=float("nan")), dict(out_lens=[5, 5], reversed=[True, False])):
        with pytest.raises(ValueError):
            score.frame_log_likelihood(z, ls, **kw)
    with pytest.raises(ValueError):
        score.frame_log_likelihood(z, [], [5, 5])
    with pytest.raises(ValueError):
        score.frame_log_likelihood(z, ls * 9, [5, 5])
    with pytest.raises(ValueError):
        score.frame_log_likelihood(z, [torch.zeros(5, 2, 7)], [5, 5])
    with pytest.raises(ValueError):
        score.frame_log_likelihood(torch.zeros(5, 2, 129), [torch.zeros(5, 2, 129)], [5, 5])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        score.frame_log_likelihood(z, ls, [5, 5])
    rows = [[torch.zeros(2, 1, 4)] * 3] * 2
    for lengths in ([3], [3, 4], [0, 3], None):
        with pytest.raises(ValueError):
            score.infer_attention_maps(rows, lengths)
    with pytest.raises(ValueError):
        score.infer_attention_maps([], [3, 3])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        score.infer_attention_maps(rows, [3, 2])


def test_log_likelihood_refuses_training_mode_and_mixture_models():
    import flowtron
    from oracle import synth
    cfg = dict(synth.SMALL_MODEL_CONFIG)
    b = synth.make_batch(cfg, [9, 7], [5, 4], seed=3, with_prior=False)
    args = (b["mel"], b["speaker_ids"], b["text"], b["in_lens"], b["out_lens"])
    m = flowtron.Flowtron(**cfg)
    m.train()
    with pytest.raises(ValueError, match="eval"):
        m.log_likelihood(*args)
    gm = flowtron.Flowtron(**dict(cfg, n_components=4)).eval()
    with pytest.raises(NotImplementedError, match="n_components"):
        gm.log_likelihood(*args)
    with pytest.raises(ValueError, match="sigma"):
        m.eval().log_likelihood(*args, sigma=0.0)
