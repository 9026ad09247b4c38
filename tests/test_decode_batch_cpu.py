"""Host side of the batched persistent decode (ft_decode_flow_batch, csrc/decode_batch.hip), no GPU needed: the batch bound, the
granule size query and every refusal, which must come before anything reaches the device."""
import ctypes as C

import pytest

EINVAL, EUNSUPPORTED = -1, -3      # FT_EINVAL, FT_EUNSUPPORTED (include/flowtron_hip.h)


@pytest.fixture(scope="module")
def lib():
    from flowtron_amd import _lib as L
    from flowtron_amd import build
    build.build(verbose=False)
    return L.lib()


def _args(lm, nb=2, **kw):
    """a full-geometry argument block with fake (16-byte aligned, never dereferenced) addresses"""
    fake = 1 << 20
    a = lm.DecodeArgs()
    for name, typ in lm.DecodeArgs._fields_:
        if typ is lm._p and name not in ("cond_w1", "cond_b1", "cond_w2", "cond_b2", "w_key", "enc", "prior", "forced", "wimg",
                                        "extra_layers", "work"):
            setattr(a, name, fake)
            fake += 1 << 12
    a.N, a.L, a.H, a.A, a.M, a.E = 10, 23, 1024, 640, 80, 1
    a.temperature, a.gate_threshold, a.n_layers = 1.0, 0.5, 2
    a.wimg, a.wimg_bytes = 1 << 30, 1 << 28                    # the 16-bit weight-image mode
    for k, v in kw.items():
        setattr(a, k, v)
    return lm.DecodeBatchArgs(a, nb, fake, 0)


def test_batch_bound_and_granule_sizes(lib):
    nbmax = lib.ft_decode_batch_max()
    assert nbmax >= 4
    one = lib.ft_decode_persist_gran_bytes()            # the single-utterance buffer: 9 copies of the layout + census
    for nb in range(1, nbmax + 1):
        assert lib.ft_decode_batch_gran_bytes(nb) == (one - 64) * nb + 64
    assert lib.ft_decode_batch_gran_bytes(0) == 0


def test_batch_entry_refuses_before_touching_the_device(lib):
    from flowtron_amd import _lib as L
    run = lambda b: lib.ft_decode_flow_batch(C.byref(b), None)
    nbmax = lib.ft_decode_batch_max()
    assert lib.ft_decode_flow_batch(None, None) == EINVAL
    for nb in (-1, 0, 1, nbmax + 1):
        assert run(_args(L, nb)) == EINVAL, nb
    b = _args(L)
    b.n_lim = None
    assert run(b) == EINVAL
    for name in ("att_w_ih", "K", "V", "residual", "mel_out", "attn_out", "n_done_dev", "persist_gran", "persist_status", "l1_w_ih"):
        b = _args(L)
        setattr(b.a, name, None)
        assert run(b) == EINVAL, name
    for name in ("K", "residual", "l0_w_ih", "persist_gran"):
        b = _args(L)
        setattr(b.a, name, getattr(b.a, name) + 4)      # 4-byte aligned only
        assert run(b) == EINVAL, name
    b = _args(L, gate_w=None)                            # gate weight without bias
    assert run(b) == EINVAL
    b = _args(L, wimg_bytes=16)                          # image buffer too small
    assert run(b) == EINVAL
    b = _args(L, wimg=(1 << 30) + 16)                    # image buffer not 256-byte aligned
    assert run(b) == EINVAL
    for kw in (dict(H=512), dict(A=128), dict(M=64), dict(L=1025), dict(n_layers=3), dict(n_layers=1),
               dict(prior=1 << 29), dict(forced=1 << 29), dict(cond_w1=1 << 29)):
        assert run(_args(L, **kw)) == EUNSUPPORTED, kw
