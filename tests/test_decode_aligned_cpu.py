"""Host side of the decode along given alignments in the persistent launches (Flowtron.infer_aligned(persistent=True),
ft_decode_flow_batch_forced, csrc/decode_forced.hip), no GPU needed: the row preparation against the rows the utterance loop
builds, the float64 reference as a fixed point of "decode along your own attention", and the entry's declaration and its
refusals before anything reaches the device."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

import decode_ref64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -3


def loop_rows(alignment, F_, b, nf, il):
    """infer_aligned's utterance loop, as it builds the rows of utterance b for every flow"""
    rows = []
    for f in range(F_):
        a = (alignment[f, b] if alignment.dim() == 4 else alignment[b])[:nf[b], :il[b]].float()
        rows.append(torch.flip(a, (0,)) if f % 2 == 1 else a)
    return rows


@pytest.mark.parametrize("rank", [3, 4])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_aligned_rows_are_the_rows_of_the_utterance_loop(rank, dtype):
    from flowtron_amd.model import aligned_rows
    g = torch.Generator().manual_seed(rank)
    F_, B, N, Lt = 3, 5, 19, 11
    nf, il = [19, 1, 7, 12, 2], [11, 3, 1, 8, 11]
    alignment = torch.rand((F_, B, N, Lt) if rank == 4 else (B, N, Lt), generator=g, dtype=dtype)
    for n_text in (max(il), Lt):
        for f in range(F_):
            got = aligned_rows(alignment, f, nf, n_text)
            assert got.dtype == torch.float32 and got.is_contiguous() and tuple(got.shape) == (B, max(nf), n_text)
            for b in range(B):
                assert torch.equal(got[b, :nf[b], :il[b]], loop_rows(alignment, F_, b, nf, il)[f]), (f, b)
    short = [5, 1, 5, 4, 2]                                      # every utterance shorter than N: the result is cut to the longest
    assert tuple(aligned_rows(alignment, 1, short, Lt).shape) == (B, 5, Lt)
    for b in range(B):
        assert torch.equal(aligned_rows(alignment, 1, short, Lt)[b, :short[b], :il[b]], loop_rows(alignment, F_, b, short, il)[1])


def test_signatures_keep_the_default_path():
    import flowtron
    from flowtron_amd.model import AR_Step
    p = inspect.signature(flowtron.Flowtron.infer_aligned).parameters
    assert list(p)[-1] == "persistent" and p["persistent"].default is False
    p = inspect.signature(AR_Step.infer_batch).parameters
    assert list(p) == ["self", "x", "text", "lens", "in_lens", "forced"] and p["forced"].default is None


def small_case(N, Lk):
    from oracle import flowtron_oracle as O
    cfg, sd = R.model_sd(small=True, seed=31)
    w = {k: v for k, v in R.flow_weights(sd, O.flow_prefix(cfg["n_flows"] - 1)).items() if not k.startswith("gate_layer.")}
    residual, enc = R.case_inputs(cfg, sd, N, Lk, seed=7)
    return (w, residual, enc @ w["attention_layer.key.linear_layer.weight"].t(),
            enc @ w["attention_layer.value.linear_layer.weight"].t())


@pytest.mark.parametrize("rounding", [None, torch.bfloat16])
def test_reference_decoding_along_its_own_attention_reproduces_its_mel(rounding):
    """the construction of the GPU test "own attention reproduces the decode", on the float64 reference itself: exact up to the
    float64 roundings of 17 frames (the rows pass through unchanged, so every later operation sees the same operands)"""
    w, residual, K, V = small_case(17, 9)
    free = R.decode(w, residual, K, V, rounding=rounding)
    again = R.decode(w, residual, K, V, rounding=rounding, forced=free["attn"])
    assert again["n_done"] == free["n_done"] == 17
    assert torch.equal(again["attn"], free["attn"])
    assert (again["mel"] - free["mel"]).abs().max().item() <= 1e-12
    other = R.decode(w, residual, K, V, rounding=rounding, forced=torch.roll(free["attn"], 1, 1))
    assert (other["mel"] - free["mel"]).abs().max().item() > 1e-6   # and the rows do matter


def test_forced_entry_declared_and_exported():
    from flowtron_amd import _lib as L
    from flowtron_amd import build
    hdr = open(os.path.join(ROOT, "include", "flowtron_hip.h")).read()
    assert re.search(r"int ft_decode_flow_batch_forced\(const ft_decode_batch_args\* a, const int32_t\* n_keys, void\* stream\);", hdr)
    assert L.SIGNATURES["ft_decode_flow_batch_forced"] == ([C.POINTER(L.DecodeBatchArgs), L._p, L._p], L._i)
    lib = C.CDLL(build.build(verbose=False))
    assert hasattr(lib, "ft_decode_flow_batch_forced")
    assert lib.ft_abi_version() == 15                            # a function more, no layout changed


def forced_args(lib_mod, **over):
    """a ft_decode_args with every pointer the forced entry reads set to a fake aligned address (nothing is dereferenced on the host)"""
    fake = 1 << 20
    a = lib_mod.DecodeArgs()
    for name, typ in lib_mod.DecodeArgs._fields_:
        if typ is lib_mod._p and name not in ("cond_w1", "cond_b1", "cond_w2", "cond_b2", "w_key", "enc", "prior", "wimg",
                                              "extra_layers", "work", "w_query", "K"):
            setattr(a, name, fake)
            fake += 1 << 12
    a.N, a.L, a.H, a.A, a.M, a.E = 10, 23, 1024, 640, 80, 1
    a.temperature, a.gate_threshold, a.n_layers = 1.0, 0.5, 2
    for k, v in over.items():
        setattr(a, k, v)
    return a, fake


def test_forced_entry_refuses_before_touching_the_device():
    from flowtron_amd import _lib as L
    from flowtron_amd import build
    build.build(verbose=False)
    lib = L.lib()
    run = lambda a, nb, lim, keys=None: lib.ft_decode_flow_batch_forced(C.byref(L.DecodeBatchArgs(a, nb, lim, 0)), keys, None)
    assert lib.ft_decode_flow_batch_forced(None, None, None) == EINVAL
    a, fake = forced_args(L)
    nbmax = lib.ft_decode_batch_max()
    assert run(a, 0, fake) == EUNSUPPORTED and b"ft_decode_flow_batch_forced" in lib.ft_last_error()
    assert run(a, nbmax + 1, fake) == EUNSUPPORTED
    assert run(forced_args(L, forced=None)[0], 2, fake) == EUNSUPPORTED           # no rows to decode along
    assert run(forced_args(L, prior=fake)[0], 2, fake) == EUNSUPPORTED            # attention priors stay on the staged chain
    assert run(forced_args(L, cond_w1=fake)[0], 2, fake) == EUNSUPPORTED          # cumulative attention
    assert run(forced_args(L, n_layers=3)[0], 2, fake) == EUNSUPPORTED
    assert run(forced_args(L, L=1025)[0], 2, fake) == EUNSUPPORTED
    assert run(a, 1, None) == EINVAL                                              # a group of one is taken; no frame limits is not
    assert run(a, 2, fake, fake + 2) == EINVAL                                    # key counts not 4-byte aligned
    assert run(forced_args(L, forced=fake + 4)[0], 2, fake) == EINVAL             # rows not 16-byte aligned
    assert run(forced_args(L, V=None)[0], 2, fake) == EINVAL                      # V is read
    # the free-running entries keep refusing given rows
    b = L.DecodeBatchArgs(forced_args(L, w_query=fake, K=fake)[0], 2, fake, 0)
    assert lib.ft_decode_flow_batch(C.byref(b), None) == EUNSUPPORTED
    assert lib.ft_decode_flow_batch_keys(C.byref(b), None, None) == EUNSUPPORTED
