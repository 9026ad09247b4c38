"""(-m gpu) The encoder's persistent BiLSTM backward with K split over the four waves of a workgroup (csrc/bilstm_persist.hip).

The float64 step-by-step replay of test_gpu_recurrence_replay.py is the reference (imported, with its own bound: ratio <= 1.0 and
its mutation checks), at the shapes where the new structure can go wrong: no hand-off at all (T 1), XCD groups without rows, a
single row, a partial last group, the full batch; groups that end at step 1 beside groups that run to T, and sequences long enough
for the parity buffers (hand-off granules, LDS partials, leave flags) to wrap 18 times.  Saved gates and cells always come from a
real ft_bilstm_persist_fwd call.  Beyond the replay: a row's dgx does not depend on its batch, a workspace that still holds the
hand-off of earlier launches changes nothing, two calls agree bit for bit, and padded frames are exactly zero."""
import types

import pytest
import torch

from test_gpu_recurrence_replay import _keep_capsys, check_bwd, clean, env, make  # noqa: F401  (env, _keep_capsys: fixtures)

pytestmark = pytest.mark.gpu
HB = 256                         # the kernel's hidden size
SHAPES = [(1, 32), (2, 5), (5, 1), (9, 30), (37, 32)]
PATTERNS = ["all_T", "all_1", "short_group", "decreasing", "T_in_every_group"]


def lengths(pattern, T, B):
    if pattern == "all_T":
        return [T] * B
    if pattern == "all_1":
        return [1] * B
    if pattern == "short_group":                         # group 0 (rows 0..3) ends after one step, every other group runs to T
        return [1 if b < 4 else T for b in range(B)]
    if pattern == "decreasing":
        return [max(1, T - b) for b in range(B)]
    return [T if b % 4 == 0 else 1 + (7 * b) % T for b in range(B)]


@pytest.fixture(scope="module")
def bi(env):
    L, ops = env
    if not ops.bilstm_persist_ok(32, HB, 1, torch.device("cuda", 0)):
        pytest.skip("bidirectional persistent kernel not usable here")
    return L, ops


def workspace(L, B, garbage=True):
    n = L.lib().ft_bilstm_persist_workspace_bytes(B, HB)
    if garbage:                                          # a fresh workspace promises nothing about its contents
        return torch.randint(0, 256, (n,), device="cuda", dtype=torch.uint8)
    return torch.empty(n, device="cuda", dtype=torch.uint8)


def forward(L, ops, gx, w, lens, fmt, work=None):
    """ft_bilstm_persist_fwd on (gx, w) of both directions: y, saved gates and cells"""
    T, B = gx[0].shape[:2]
    y = torch.full((T, B, 2 * HB), 7.0, device="cuda")
    g = [torch.full((T, B, 4 * HB), 7.0, device="cuda") for _ in range(2)]
    c = [torch.full((T, B, HB), 7.0, device="cuda") for _ in range(2)]
    st = ops._persist_watch(gx[0].device)
    work = workspace(L, B) if work is None else work
    L.check(L.op16("ft_bilstm_persist_fwd", fmt)(L.ptr(gx[0]), L.ptr(gx[1]), L.ptr(w[0]), L.ptr(w[1]), L.ptr(lens), L.ptr(y), 2 * HB, L.ptr(g[0]),
                                                  L.ptr(g[1]), L.ptr(c[0]), L.ptr(c[1]), L.ptr(work), L.ptr(st.status), T, B, HB, L.stream()),
            "ft_bilstm_persist_fwd")
    ops._persist_arm(st, bilstm=True)
    return y, g, c


def backward(L, ops, S, fmt, work=None, fill=7.0):
    """ft_bilstm_persist_bwd on a saved forward: dgx of both directions (pre-filled: the call has to write every row)"""
    T, B = S.dy.shape[:2]
    d = [torch.full((T, B, 4 * HB), fill, device="cuda") for _ in range(2)]
    st = ops._persist_watch(S.dy.device)
    work = workspace(L, B) if work is None else work
    L.check(L.op16("ft_bilstm_persist_bwd", fmt)(L.ptr(S.dy), 2 * HB, L.ptr(S.w[0]), L.ptr(S.w[1]), L.ptr(S.lens), L.ptr(S.g[0]), L.ptr(S.g[1]),
                                                  L.ptr(S.c[0]), L.ptr(S.c[1]), L.ptr(d[0]), L.ptr(d[1]), L.ptr(work), L.ptr(st.status), T, B, HB,
                                                  L.stream()), "ft_bilstm_persist_bwd")
    ops._persist_arm(st, bilstm=True)
    return d


def inputs(T, B, lens, seed):
    gf, wf, lens_t = make(T, B, seed, lens, Hd=HB)
    gr, wr, _ = make(T, B, seed + 2, lens, Hd=HB)
    dy = torch.randn(T, B, 2 * HB, generator=torch.Generator().manual_seed(seed + 1)).cuda() * 0.1
    return [gf, gr], [wf, wr], lens_t, dy


_SAVED = {}


def saved(L, ops, T, B, lens, fmt, seed, work=None):
    """inputs and the saved tensors of a real forward call, made once per case and shared (never written to afterwards)"""
    key = (T, B, tuple(lens), fmt, seed)
    if key not in _SAVED or work is not None:
        gx, w, lens_t, dy = inputs(T, B, lens, seed)
        y, g, c = forward(L, ops, gx, w, lens_t, fmt, work)
        S = types.SimpleNamespace(gx=gx, w=w, lens=lens_t, dy=dy, y=y, g=g, c=c)
        if work is not None:
            return S
        torch.cuda.synchronize()
        clean(ops)
        _SAVED[key] = S
    return _SAVED[key]


def replay_both(name, S, d, fmt, sharp=True):
    check_bwd(name + " dir 0", S.dy[..., :HB].contiguous(), S.w[0], S.lens, S.g[0], S.c[0], d[0], fmt, sharp=sharp)
    check_bwd(name + " dir 1", S.dy[..., HB:].contiguous(), S.w[1], S.lens, S.g[1], S.c[1], d[1], fmt, reverse=True, sharp=sharp)


@pytest.mark.parametrize("fmt", [1, 2])
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("T,B", SHAPES)
def test_split_backward_replays_step_by_step(bi, T, B, pattern, fmt):
    """dgx of both directions against the float64 replay, within the replay's own bound, with its mutation checks on"""
    L, ops = bi
    lens = lengths(pattern, T, B)
    S = saved(L, ops, T, B, lens, fmt, 100 + 3 * T + B)
    d = backward(L, ops, S, fmt)
    torch.cuda.synchronize()
    clean(ops)
    replay_both("split bwd T %d B %d %s fmt %d" % (T, B, pattern, fmt), S, d, fmt)


@pytest.mark.parametrize("fmt", [1, 2])
def test_split_backward_replays_at_the_encoder_shape(bi, fmt):
    """T 157, B 32 with the benchmark's text lengths"""
    import bench
    L, ops = bi
    T, B = 157, 32
    lens = [int(v) for v in bench.synth_batch(B, 1234 + 7)["in_lens"]]
    assert max(lens) <= T
    S = saved(L, ops, T, B, lens, fmt, 1234)
    d = backward(L, ops, S, fmt)
    torch.cuda.synchronize()
    clean(ops)
    replay_both("split bwd encoder shape fmt %d" % fmt, S, d, fmt, sharp=False)


@pytest.mark.parametrize("fmt", [1, 2])
def test_a_rows_dgx_does_not_depend_on_its_batch(bi, fmt):
    """one utterance (same gx, dy, length) at positions 0, 13 and 31 of a batch of 32 and alone: its dgx rows are the same bits"""
    L, ops = bi
    T, n = 37, 29
    ugx, w, _, udy = inputs(T, 1, [n], 7)
    got = []
    for B, pos in ((32, 0), (32, 13), (32, 31), (1, 0)):
        lens = [T if b % 5 == 0 else 1 + (11 * b + pos) % T for b in range(B)]
        lens[pos] = n
        gx, _, lens_t, dy = inputs(T, B, lens, 50 + pos)
        for k in range(2):
            gx[k][:, pos] = ugx[k][:, 0]
        dy[:, pos] = udy[:, 0]
        y, g, c = forward(L, ops, gx, w, lens_t, fmt)
        S = types.SimpleNamespace(w=w, lens=lens_t, dy=dy, g=g, c=c)
        d = backward(L, ops, S, fmt)
        torch.cuda.synchronize()
        clean(ops)
        got.append([g[0][:n, pos].clone(), g[1][:n, pos].clone(), d[0][:, pos].clone(), d[1][:, pos].clone()])
    for other in got[1:]:
        for k in range(2):
            assert torch.equal(got[0][k], other[k]), "the forward's saved gates of the row differ: the comparison below would mean nothing"
        assert torch.equal(got[0][2], other[2]) and torch.equal(got[0][3], other[3])


@pytest.mark.parametrize("fmt", [1, 2])
def test_stale_hand_off_of_earlier_launches_changes_nothing(bi, fmt):
    """ONE workspace and status word, three forward / backward launches back to back (T 37, T 5, T 37 with other lengths): each dgx
    equals the same call on a fresh workspace"""
    L, ops = bi
    B = 32
    cases = [(37, lengths("T_in_every_group", 37, B), 300), (5, lengths("decreasing", 5, B), 301), (37, lengths("decreasing", 37, B), 302)]
    work = workspace(L, B)
    shared = []
    for T, lens, seed in cases:
        S = saved(L, ops, T, B, lens, fmt, seed, work=work)
        shared.append((S, backward(L, ops, S, fmt, work=work)))
    torch.cuda.synchronize()
    clean(ops)
    for (T, lens, seed), (S, d) in zip(cases, shared):
        F = saved(L, ops, T, B, lens, fmt, seed)
        for k in range(2):
            assert torch.equal(S.g[k], F.g[k]) and torch.equal(S.c[k], F.c[k])
        f = backward(L, ops, F, fmt)
        torch.cuda.synchronize()
        clean(ops)
        assert torch.equal(d[0], f[0]) and torch.equal(d[1], f[1]), "T %d" % T


@pytest.mark.parametrize("fmt", [1, 2])
def test_two_identical_calls_agree_bit_for_bit(bi, fmt):
    L, ops = bi
    T, B = 37, 32
    S = saved(L, ops, T, B, lengths("T_in_every_group", T, B), fmt, 100 + 3 * T + B)
    a, b = backward(L, ops, S, fmt), backward(L, ops, S, fmt)
    torch.cuda.synchronize()
    clean(ops)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("fmt", [1, 2])
def test_padded_frames_are_zero_and_valid_frames_written(bi, fmt):
    """dgx pre-filled with 7.0: every row with t >= len is exactly 0 afterwards, and no valid row still holds 7.0"""
    L, ops = bi
    T, B = 9, 30
    S = saved(L, ops, T, B, lengths("decreasing", T, B), fmt, 100 + 3 * T + B)
    d = backward(L, ops, S, fmt, fill=7.0)
    torch.cuda.synchronize()
    clean(ops)
    valid = torch.arange(T, device="cuda")[:, None] < S.lens[None, :]
    assert bool((~valid).any()) and bool(valid.any())
    for k in range(2):
        assert float(d[k][~valid].abs().max()) == 0.0
        assert not bool((d[k][valid] == 7.0).any())
