"""Restatement of the monotonic alignment search (include/flowtron_hip.h, token durations; csrc/align.hip) in plain numpy,
written from the rule, and a brute force over every monotone path:

    Q[0][0] = s[0][0]
    Q[t][l] = s[t][l] + (adv[t][l] ? Q[t-1][l-1] : Q[t-1][l])          l <= min(t, L-1)
    adv[t][l] = l > 0 and (l == t or Q[t-1][l-1] > Q[t-1][l])          (strict: a tie stays)
    backtrack from (T-1, L-1):  path[t] = l;  l -= adv[t][l]

replay(s, dtype) runs it in float32 (the kernel's arithmetic: one add and one compare per cell, so the kernel must give the
same bits) or in float64.  brute_force(s) sums every one of the C(T-1, L-1) monotone paths in float64."""
import itertools
import warnings

import numpy as np


def replay(s, dtype=np.float32):
    """s [T, L] with L <= T -> (path [T] int32, durations [L] int32, score as `dtype`)."""
    s = np.asarray(s, dtype)
    T, L = s.shape
    assert 1 <= L <= T
    adv = np.zeros((T, L), bool)
    q = np.full(L, -np.inf, dtype)
    q[0] = s[0, 0]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for t in range(1, T):
            n = min(t, L - 1) + 1                               # cells 0 .. n-1 of this row
            left = np.concatenate([np.full(1, -np.inf, dtype), q[:n - 1]])
            a = left > q[:n]
            a[0] = False
            if n - 1 == t:
                a[t] = True
            adv[t, :n] = a
            q = q.copy()
            q[:n] = s[t, :n] + np.where(a, left, q[:n])
    path = np.zeros(T, np.int32)
    l = L - 1
    for t in range(T - 1, -1, -1):
        path[t] = l
        l -= int(adv[t, l])
    return path, np.bincount(path, minlength=L).astype(np.int32), q[L - 1]


def paths(T, L):
    """every monotone path [T] from token 0 to token L-1 in steps of 0 or 1, in ascending lexicographic order"""
    for steps in itertools.combinations(range(1, T), L - 1):     # the frames at which the path advances
        p = np.zeros(T, np.int64)
        for t in steps:
            p[t:] += 1
        yield p


def path_score(s, p):
    """the float64 sum of s along path p, added frame by frame as the recurrence adds it"""
    s = np.asarray(s, np.float64)
    v = s[0, p[0]]
    for t in range(1, s.shape[0]):
        v = s[t, p[t]] + v
    return float(v)


def brute_force(s):
    """-> (best score in float64, the lexicographically greatest path among those that reach it)"""
    s = np.asarray(s, np.float64)
    T, L = s.shape
    best, best_path = None, None
    for p in paths(T, L):
        v = path_score(s, p)
        if best is None or v > best or (v == best and tuple(p) > tuple(best_path)):
            best, best_path = v, p
    return best, best_path.astype(np.int32)


def one_hot_rows(durations, in_len, n_frames, reverse=False):
    """the expansion of ft_durations_to_rows for one utterance: [n_frames, L] float32"""
    d = np.maximum(np.asarray(durations, np.int64), 0)
    L = d.shape[0]
    d = d[:in_len]
    total = int(d.sum())
    rows = np.zeros((n_frames, L), np.float32)
    tok = np.repeat(np.arange(in_len), d)                        # the token of every frame
    if reverse:
        tok = tok[::-1]
    n = min(total, n_frames)
    rows[np.arange(n), tok[:n]] = 1.0
    return rows
