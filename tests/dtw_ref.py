"""Restatement of the cepstra and of dynamic time warping (include/flowtron_hip.h, mel-cepstral distortion; csrc/dtw.hip) in
plain numpy, written from the rule, and a brute force over every warping path:

    cep[t][k-1] = sum_m mel[m][t] * D[k-1][m]      D[k-1][m] = fp32(sqrt(2/M) cos(pi k (m + 0.5) / M)), m ascending
    d[i][j] = sqrt(sum_k (x[i][k] - y[j][k])^2)     k ascending; sub, mul, add and sqrt rounded one at a time
    C[0][0] = d[0][0];   i == 0: move 2, from (i, j-1);   j == 0: move 1, from (i-1, j)
    else best = C[i-1][j-1], move 0;  if C[i-1][j] < best: best, move 1;  if C[i][j-1] < best: best, move 2     (strict)
    C[i][j] = d[i][j] + best;   backtrack from (A-1, N-1) to (0, 0)

replay(x, y, dtype) runs it in float32 (the kernel's arithmetic, so the kernel must give the same bits) or in float64, one
anti-diagonal per numpy step.  brute_force(x, y) sums every warping path in float64.  The keyword switches of replay and
cepstra (ties, strict, fma, descending, c0) build deliberately WRONG references: the tests use them to show that their
inputs tell the rule from its neighbours."""
import warnings

import numpy as np

MOVES = ((1, 1), (1, 0), (0, 1))                 # move 0, 1, 2: what (i, j) loses on the way back
# (Ta, Tb) of the device tests: the edges, the wave boundary, the 256-thread boundary and the limit
SHAPES = [(1, 1), (1, 7), (7, 1), (5, 5), (63, 65), (64, 64), (65, 63), (64, 200), (257, 255), (300, 1024), (1024, 1), (1024, 1024)]


def dct_table(M, K, c0=False):
    """rows 1 .. K (c0: 0 .. K-1) of the orthonormal DCT-II over M points, float64 rounded to float32 once"""
    k = (np.arange(K, dtype=np.float64) + (0 if c0 else 1))[:, None]
    m = np.arange(M, dtype=np.float64)[None, :]
    D = np.sqrt(2.0 / M) * np.cos(np.pi * k * (m + 0.5) / M)
    if c0:
        D[0] = np.sqrt(1.0 / M)
    return D.astype(np.float32)


def cepstra(mel, K, dtype=np.float32, c0=False):
    """mel [M, T] -> [T, K] as `dtype`: the float32 table, the sum over ascending m, every product and sum rounded to dtype"""
    mel = np.asarray(mel, dtype)
    M, T = mel.shape
    D = dct_table(M, K, c0).astype(dtype)
    acc = np.zeros((T, K), dtype)
    for m in range(M):
        acc = acc + mel[m][:, None] * D[:, m][None, :]
    return acc


def distances(x, y, dtype=np.float32, fma=False, descending=False):
    """x [A, K], y [N, K] -> d [A, N] as `dtype`"""
    x, y = np.asarray(x, dtype), np.asarray(y, dtype)
    K = x.shape[1]
    acc = np.zeros((x.shape[0], y.shape[0]), dtype)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for k in (range(K - 1, -1, -1) if descending else range(K)):
            df = x[:, k][:, None] - y[:, k][None, :]
            if fma:                              # the product is exact in float64; one rounding of the sum (float32 only)
                acc = (df.astype(np.float64) * df.astype(np.float64) + acc.astype(np.float64)).astype(dtype)
            else:
                acc = acc + df * df
        return np.sqrt(acc)


def replay(x, y, dtype=np.float32, diagonal=False, ties="low", strict=True, fma=False, descending=False):
    """x [A, K], y [N, K] -> (cost as `dtype`, path [P, 2] int32 in ascending order).  diagonal: the cells (i, i), A == N."""
    d = distances(x, y, dtype, fma, descending)
    A, N = d.shape
    if diagonal:
        assert A == N
        c = d[0, 0]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            for i in range(1, A):
                c = d[i, i] + c
        return c, np.stack([np.arange(A), np.arange(A)], 1).astype(np.int32)
    C = np.zeros((A, N), dtype)
    mv = np.zeros((A, N), np.int8)
    C[0, 0] = d[0, 0]
    mv[0, 0] = 2
    order = (0, 1, 2) if ties == "low" else (2, 1, 0)
    less = (lambda a, b: a < b) if strict else (lambda a, b: a <= b)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for s in range(1, A + N - 1):
            i = np.arange(max(0, s - N + 1), min(A - 1, s) + 1)
            j = s - i
            im, jm = np.maximum(i - 1, 0), np.maximum(j - 1, 0)
            cand = (C[im, jm], C[im, j], C[i, jm])             # diagonal, up, left
            best = cand[order[0]].copy()
            move = np.full(i.shape, order[0], np.int8)
            for o in order[1:]:
                t = less(cand[o], best)
                best = np.where(t, cand[o], best)
                move[t] = o
            top, edge = i == 0, j == 0
            best[top], move[top] = cand[2][top], 2
            best[edge], move[edge] = cand[1][edge], 1
            C[i, j] = d[i, j] + best
            mv[i, j] = move
    cells = []
    i, j = A - 1, N - 1
    while True:
        cells.append((i, j))
        if i == 0 and j == 0:
            break
        di, dj = MOVES[mv[i, j]]
        i, j = i - di, j - dj
    return C[A - 1, N - 1], np.array(cells[::-1], np.int32)


def path_cost(x, y, path, dtype=np.float64):
    """the sum of d along `path`, added cell by cell as the recurrence adds it"""
    d = distances(x, y, dtype)
    v = d[path[0][0], path[0][1]]
    for i, j in path[1:]:
        v = d[i, j] + v
    return v


def warping_paths(A, N):
    """every path from (0, 0) to (A-1, N-1) in steps (1, 1), (1, 0), (0, 1), as the list of its moves from the END backwards"""
    def back(i, j):
        if i == 0 and j == 0:
            yield ()
            return
        for m, (di, dj) in enumerate(MOVES):
            if i - di >= 0 and j - dj >= 0:
                for rest in back(i - di, j - dj):
                    yield (m,) + rest
    return back(A - 1, N - 1)


def cells_of(moves, A, N):
    cells, i, j = [(A - 1, N - 1)], A - 1, N - 1
    for m in moves:
        i, j = i - MOVES[m][0], j - MOVES[m][1]
        cells.append((i, j))
    return np.array(cells[::-1], np.int32)


def brute_force(x, y):
    """-> (the least cost in float64, among the paths that reach it the one whose moves, read from the end backwards, are
    lexicographically least: the lowest-numbered move at the last cell where minimal paths part, the number of paths that
    reach it)"""
    A, N = np.shape(x)[0], np.shape(y)[0]
    d = distances(x, y, np.float64)
    best, n_best = None, 0
    for moves in warping_paths(A, N):
        cells = cells_of(moves, A, N)
        v = d[0, 0]
        for i, j in cells[1:]:
            v = d[i, j] + v
        n_best = 1 if best is None or v < best[0] else n_best + (v == best[0])
        if best is None or (v, moves) < (best[0], best[1]):
            best = (v, moves, cells)
    return float(best[0]), best[2], n_best


def features(kind, T, K, seed):
    """the inputs the tests share: "normal" draws, or multiples of 1/8 in [0, 1/2] ("grid": with K = 1 every distance and every
    sum of distances is exact in float32, and ties are everywhere)"""
    rs = np.random.RandomState(seed)
    if kind == "normal":
        return rs.standard_normal((T, K)).astype(np.float32)
    return (rs.randint(0, 5, size=(T, K)) / 8.0).astype(np.float32)


def pair(kind, Ta, Tb, K):
    """the pair of sequences the tests use at a shape"""
    return features(kind, Ta, K, 100 * Ta + Tb), features(kind, Tb, K, 100 * Tb + Ta + 1)


def log_mel(M, T, seed):
    """log-mel-like frames [M, T]: N(-5, 2^2), smoothed a little along time so that neighbouring frames resemble each other"""
    rs = np.random.RandomState(seed)
    m = -5.0 + 2.0 * rs.standard_normal((M, T + 2))
    return ((m[:, :-2] + m[:, 1:-1] + m[:, 2:]) / 3.0).astype(np.float32)
