"""Host side of ragged batch decode (Flowtron.infer with in_lens / out_lens), no GPU needed: the normalisation and checking of the
length arguments, and the ft_decode_flow_batch_keys entry (declared, exported, refusing bad arguments before the device)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

EINVAL = -1        # FT_EINVAL (include/flowtron_hip.h)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def lengths_arg(*a):
    from flowtron_amd.model import lengths_arg as f
    return f(*a)


def test_lengths_accept_lists_tuples_and_integer_tensors():
    assert lengths_arg(None, "in_lens", 3, 10) is None
    assert lengths_arg([1, 10, 4], "in_lens", 3, 10) == [1, 10, 4]
    assert lengths_arg((3, 2), "out_lens", 2, 5) == [3, 2]
    assert lengths_arg([np.int64(7), np.int32(2)], "in_lens", 2, 7) == [7, 2]
    for dt in (torch.int64, torch.int32, torch.int16, torch.uint8):
        got = lengths_arg(torch.tensor([5, 1, 9], dtype=dt), "in_lens", 3, 9)
        assert got == [5, 1, 9] and all(type(x) is int for x in got), dt


@pytest.mark.parametrize("v, msg", [
    ([1, 2], "has 2 entries for a batch of 3"),
    (torch.tensor([4, 4, 4, 4]), "has 4 entries for a batch of 3"),
    ([0, 2, 3], r"must lie in 1 \.\.= 8"),
    ([1, 9, 3], r"must lie in 1 \.\.= 8"),
    ([-1, 2, 3], r"must lie in 1 \.\.= 8"),
    (torch.tensor([1, 0, 3]), r"must lie in 1 \.\.= 8"),
    (torch.tensor([1.0, 2.0, 3.0]), "must hold integers"),
    ([1.0, 2, 3], "must hold integers"),
    ([True, 2, 3], "must hold integers"),
    (torch.tensor([True, True, False]), "must hold integers"),
    (torch.tensor([[1, 2, 3]]), "one-dimensional"),
    (5, "list, tuple or tensor"),
    ("123", "list, tuple or tensor"),
])
def test_lengths_refused_with_a_message(v, msg):
    with pytest.raises(ValueError, match=msg):
        lengths_arg(v, "in_lens", 3, 8)
    with pytest.raises(ValueError, match="out_lens"):
        lengths_arg(v, "out_lens", 3, 8)


def test_infer_signature_keeps_the_old_arguments_first():
    import inspect
    import flowtron
    names = list(inspect.signature(flowtron.Flowtron.infer).parameters)
    assert names == ["self", "residual", "speaker_ids", "text", "temperature", "gate_threshold", "attns", "attn_prior",
                     "in_lens", "out_lens", "return_lengths"]


def test_keys_entry_declared_and_exported():
    from flowtron_amd import _lib as L
    from flowtron_amd import build
    hdr = open(os.path.join(ROOT, "include", "flowtron_hip.h")).read()
    assert re.search(r"int ft_decode_flow_batch_keys\(const ft_decode_batch_args\* a, const int32_t\* n_keys, void\* stream\);", hdr)
    assert L.SIGNATURES["ft_decode_flow_batch_keys"] == ([C.POINTER(L.DecodeBatchArgs), L._p, L._p], L._i)
    lib = C.CDLL(build.build(verbose=False))
    assert hasattr(lib, "ft_decode_flow_batch_keys")


def test_keys_entry_refuses_before_touching_the_device():
    from flowtron_amd import _lib as L
    from flowtron_amd import build
    build.build(verbose=False)
    lib = L.lib()
    assert lib.ft_decode_flow_batch_keys(None, None, None) == EINVAL
    fake = 1 << 20
    a = L.DecodeArgs()
    for name, typ in L.DecodeArgs._fields_:
        if typ is L._p and name not in ("cond_w1", "cond_b1", "cond_w2", "cond_b2", "w_key", "enc", "prior", "forced", "wimg",
                                        "extra_layers", "work"):
            setattr(a, name, fake)
            fake += 1 << 12
    a.N, a.L, a.H, a.A, a.M, a.E = 10, 23, 1024, 640, 80, 1
    a.temperature, a.gate_threshold, a.n_layers = 1.0, 0.5, 2
    ok = L.DecodeBatchArgs(a, 2, fake, 0)
    assert lib.ft_decode_flow_batch_keys(C.byref(ok), fake + 2, None) == EINVAL      # key counts not 4-byte aligned
    bad = L.DecodeBatchArgs(a, 1, fake, 0)
    assert lib.ft_decode_flow_batch_keys(C.byref(bad), fake, None) == EINVAL         # a group of one
    bad = L.DecodeBatchArgs(a, 2, None, 0)
    assert lib.ft_decode_flow_batch_keys(C.byref(bad), fake, None) == EINVAL         # no frame limits
