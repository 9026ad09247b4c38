"""(-m gpu) ft_lstm_roles_prepare_table: the W_hh fragment images of several recurrences in ONE launch, and ops.roles_wimg's plan that
uses it inside a model's forward (weight_images_begin / _end).

The table's images are compared BYTE for byte with the per-weight entry points (ft_lstm_roles_prepare_fwd: make_wfrag_fwd_ug;
ft_lstm_roles_prepare_bwd: make_wfrag_rs, the kernel ft_lstm_persist_bwd also runs for its own image).  Both are pure re-orderings of
f2op16(W_hh), so equality is the only right tolerance.  H is fixed at 1024: a weight is 16 MB and a case takes milliseconds."""
import pytest
import torch

pytestmark = pytest.mark.gpu
H = 1024


@pytest.fixture(scope="module")
def env():
    from flowtron_amd import _lib as L
    from flowtron_amd import ops
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return L, ops


def weights(n, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter((torch.randn(4 * H, H, generator=g) * (0.03 + 0.01 * i)).cuda()) for i in range(n)]


def single(L, w, fmt, backward):
    img = torch.full((L.lib().ft_lstm_roles_wimg_bytes(H),), 0x5A, device="cuda", dtype=torch.uint8)
    fn = L.op16("ft_lstm_roles_prepare_bwd" if backward else "ft_lstm_roles_prepare_fwd", fmt)
    L.check(fn(L.ptr(w), L.ptr(img), H, L.stream()), "prepare")
    return img


def table(L, ws, fmt, want_fwd, want_bwd):
    nb = L.lib().ft_lstm_roles_wimg_bytes(H)
    f = [torch.full((nb,), 0xA5, device="cuda", dtype=torch.uint8) if on else None for on in want_fwd]
    b = [torch.full((nb,), 0xA5, device="cuda", dtype=torch.uint8) if on else None for on in want_bwd]
    descs = (L.WfragDesc * len(ws))(*[L.WfragDesc(w.data_ptr(), L.ptr(fi), L.ptr(bi)) for w, fi, bi in zip(ws, f, b)])
    rc = L.op16("ft_lstm_roles_prepare_table", fmt)(descs, len(ws), H, L.stream())
    return rc, f, b


@pytest.mark.parametrize("n,fmt,both", [(1, 1, True), (3, 1, False), (3, 1, True), (6, 1, True), (3, 2, True)])
def test_table_images_are_the_per_weight_images(env, n, fmt, both):
    """1, 3 and 6 weights; forward images only, and forward + backward (with n = 6: every other weight without its backward image, and
    one with the backward image alone); bf16 and the fp16 twin"""
    L, ops = env
    ws = weights(n, 7 * n + fmt)
    want_f = [not (n == 6 and i == 5) for i in range(n)]
    want_b = [both and not (n == 6 and i % 2 == 1 and i != 5) for i in range(n)]
    rc, f, b = table(L, ws, fmt, want_f, want_b)
    assert rc == 0, L.lib().ft_last_error()
    for i, w in enumerate(ws):
        if f[i] is not None:
            assert torch.equal(f[i], single(L, w.data, fmt, False)), ("forward image", i)
        if b[i] is not None:
            assert torch.equal(b[i], single(L, w.data, fmt, True)), ("backward image", i)


def test_table_refusals(env):
    L, ops = env
    ws = weights(1, 3)
    assert table(L, ws, 1, [False], [False])[0] == -1                 # a weight without a destination
    descs = (L.WfragDesc * 17)()
    assert L.lib().ft_lstm_roles_prepare_table(descs, 17, H, L.stream()) == -1
    assert L.lib().ft_lstm_roles_prepare_table(descs, 0, H, L.stream()) == -1
    nb = L.lib().ft_lstm_roles_wimg_bytes(H)
    img = torch.empty(nb + 256, device="cuda", dtype=torch.uint8)
    one = (L.WfragDesc * 1)(L.WfragDesc(ws[0].data_ptr(), img.data_ptr() + 16, None))
    assert L.lib().ft_lstm_roles_prepare_table(one, 1, H, L.stream()) == -1      # image not 256-byte aligned
    assert L.lib().ft_lstm_roles_prepare_table(one, 1, 512, L.stream()) == -1


class Model:
    pass


def test_roles_wimg_plan_builds_every_forward_from_current_values(env, monkeypatch):
    """ops.roles_wimg inside a model's forward: the first forward has no plan (per-weight launches); the second builds the three forward
    images in one table launch; after a backward has asked for two backward images, the third forward builds those too (only with
    gradients enabled) and the backward takes them.  An in-place update between two forwards -- and one between a forward and its
    backward -- is seen: the images are those of the CURRENT values."""
    L, ops = env
    monkeypatch.setattr(ops, "_WIMG_ON", True)
    calls = []
    real = L.lib().ft_lstm_roles_prepare_table
    monkeypatch.setattr(L.lib(), "ft_lstm_roles_prepare_table", lambda d, n, h, s: calls.append(n) or real(d, n, h, s))
    ws = weights(3, 11)
    m = Model()

    def forward():
        ops.weight_images_begin(m)
        try:
            return [ops.roles_wimg(w, 1, False) for w in ws]
        finally:
            ops.weight_images_end(m)

    def check(imgs, backward):
        for w, img in zip(ws, imgs):
            assert torch.equal(img, single(L, w.data, 1, backward))

    check(forward(), False)
    assert calls == []
    check(forward(), False)                                            # forward images alone: nobody has asked for a backward image
    assert calls == [3]
    check([ops.roles_wimg(w, 1, True) for w in ws[:2]], True)          # the pass's backward: per-weight launches, and marks in the plan
    assert calls == [3]
    with torch.no_grad():
        ws[0].mul_(1.5)                                                # the optimizer step
    check(forward(), False)
    assert calls == [3, 3]
    check([ops.roles_wimg(w, 1, True) for w in ws[:2]], True)          # ... made by the table this time
    assert len(ops._WIMG["wf_cache"]) == 0, "the backward took its two images; the third weight has none"
    with torch.no_grad():
        forward()
    assert len(ops._WIMG["wf_cache"]) == 0, "no backward images without gradients"
    forward()
    with torch.no_grad():
        ws[1].add_(0.25)                                               # changed between the forward and its backward: the cached image is stale
    check([ops.roles_wimg(w, 1, True) for w in ws[:2]], True)
    ops.weight_images_begin(m)
    ops.weight_images_end(m)
    assert len(ops._WIMG["wf_cache"]) == 0
