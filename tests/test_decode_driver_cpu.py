"""Host side of the decode driver (flowtron_amd/decode.py), no GPU needed: the argument builder against a table typed from
include/flowtron_hip.h (ft_decode_args), the cache of the buffers per shape, the retry helper, the padding helpers, and the
scratch attributes across a checkpoint pickle."""
import ctypes as C
import pickle

import pytest
import torch

# ft_decode_args field -> the AR_Step parameter it points to (include/flowtron_hip.h: attention_lstm; attention; lstm l0, l1;
# dense, conv; gate)
WEIGHTS = {
    "att_w_ih": "attention_lstm.weight_ih_l0", "att_w_hh": "attention_lstm.weight_hh_l0",
    "att_b_ih": "attention_lstm.bias_ih_l0", "att_b_hh": "attention_lstm.bias_hh_l0",
    "w_query": "attention_layer.query.linear_layer.weight", "v": "attention_layer.v.linear_layer.weight",
    "l0_w_ih": "lstm.weight_ih_l0", "l0_w_hh": "lstm.weight_hh_l0", "l0_b_ih": "lstm.bias_ih_l0", "l0_b_hh": "lstm.bias_hh_l0",
    "l1_w_ih": "lstm.weight_ih_l1", "l1_w_hh": "lstm.weight_hh_l1", "l1_b_ih": "lstm.bias_ih_l1", "l1_b_hh": "lstm.bias_hh_l1",
    "d0_w": "dense_layer.layers.0.linear_layer.weight", "d0_b": "dense_layer.layers.0.linear_layer.bias",
    "d1_w": "dense_layer.layers.1.linear_layer.weight", "d1_b": "dense_layer.layers.1.linear_layer.bias",
    "conv_w": "conv.weight", "conv_b": "conv.bias",
}
GATE = {"gate_w": "gate_layer.linear_layer.weight", "gate_b": "gate_layer.linear_layer.bias"}
SCRATCH = ("_decode_bufs", "_decode_batch_bufs", "_decode_wimg", "_decode_gran", "_decode_batch_gran")
M, H, A = 8, 16, 8


@pytest.fixture(scope="module")
def lib():
    from flowtron_amd import _lib as L
    from flowtron_amd import build
    build.build(verbose=False)
    return L.lib()


def make_step(n_layers, gate, cumm=False):
    from flowtron_amd.model import AR_Step
    torch.manual_seed(0)
    return AR_Step(M, 4, 12, M + 4, H, A, n_layers, gate, cumm)


def check_args(args, step, expect):
    """every field of the struct: a weight of the table, a value of `expect`, or null / zero"""
    from flowtron_amd import _lib as L
    want = {name: step.get_parameter(path).data_ptr() for name, path in WEIGHTS.items()
            if not name.startswith("l1_") or step.n_lstm_layers >= 2}
    if hasattr(step, "gate_layer"):
        want.update({name: step.get_parameter(path).data_ptr() for name, path in GATE.items()})
    want.update(H=H, A=A, M=M, n_layers=step.n_lstm_layers)
    want.update(expect)
    for name, _ in L.DecodeArgs._fields_:
        got = getattr(args, name)
        if name in ("temperature", "gate_threshold"):
            assert got == pytest.approx(want[name], rel=1e-7), name
        else:
            assert (got or 0) == want.get(name, 0), name


def test_args_with_gate_two_layers_every_field(lib):
    from flowtron_amd import decode
    step = make_step(2, True, cumm=True)
    step.attention_layer.temperature = 0.7
    step.gate_threshold = 0.3
    t = {n: torch.zeros(4) for n in ("K", "V", "residual", "mel_out", "attn_out", "prior", "forced", "persist_gran", "enc")}
    n_done, status = torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    work, wimg = torch.zeros(48, dtype=torch.uint8), torch.zeros(80, dtype=torch.uint8)
    c1, c2 = step.attn_cond_layer.location_conv_hidden.conv, step.attn_cond_layer.location_conv_out.conv
    w_key = step.attention_layer.key.linear_layer.weight
    args = decode.decode_args(step, K=t["K"], V=t["V"], residual=t["residual"], mel_out=t["mel_out"], attn_out=t["attn_out"],
                              n_done_dev=n_done, work=work, N=5, L=7, E=16, use_graph=1, cond_w1=c1.weight, cond_b1=c1.bias,
                              cond_w2=c2.weight, cond_b2=c2.bias, w_key=w_key, enc=t["enc"], prior=t["prior"], forced=t["forced"],
                              wimg=wimg, persist_gran=t["persist_gran"], persist_status=status)
    expect = {n: v.data_ptr() for n, v in t.items()}
    expect.update(n_done_dev=n_done.data_ptr(), persist_status=status.data_ptr(), work=work.data_ptr(), work_bytes=48,
                  wimg=wimg.data_ptr(), wimg_bytes=80, N=5, L=7, E=16, use_graph=1, cond_w1=c1.weight.data_ptr(),
                  cond_b1=c1.bias.data_ptr(), cond_w2=c2.weight.data_ptr(), cond_b2=c2.bias.data_ptr(), w_key=w_key.data_ptr(),
                  temperature=0.7, gate_threshold=0.3)
    check_args(args, step, expect)
    assert len({getattr(args, n) for n in list(WEIGHTS) + list(GATE)}) == len(WEIGHTS) + len(GATE)      # no two fields share a tensor


def test_args_without_gate_three_layers_rest_null(lib):
    from flowtron_amd import decode
    step = make_step(3, False)
    V, res = torch.zeros(4), torch.zeros(4)
    ptrs = [step.get_parameter("lstm.%s_l2" % nm).data_ptr() for nm in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    extra = (C.c_void_p * 4)(*ptrs)
    args = decode.decode_args(step, K=None, V=V, residual=res, N=3, L=2, E=1, extra_layers=C.cast(extra, C.c_void_p))
    check_args(args, step, dict(V=V.data_ptr(), residual=res.data_ptr(), N=3, L=2, E=1, extra_layers=C.addressof(extra),
                                temperature=1.0, gate_threshold=2.0))
    assert args.gate_w is None and args.gate_b is None and args.K is None and args.work is None and args.work_bytes == 0
    one = make_step(1, False)                                        # depth 1: the layer-1 slots stay null
    check_args(decode.decode_args(one), one, dict(temperature=1.0, gate_threshold=2.0))
    assert decode.decode_args(one).l1_w_ih is None and decode.decode_args(one).n_layers == 1


def test_args_refuse_an_unknown_field(lib):
    from flowtron_amd import decode
    with pytest.raises(TypeError):
        decode.decode_args(make_step(2, True), residuals=torch.zeros(1))


def test_shape_lru_evicts_the_least_recently_used():
    from flowtron_amd import decode
    lru = decode.ShapeLRU()
    made = []

    def make():
        made.append(dict(K=torch.zeros(1), V=torch.zeros(1)))
        return made[-1]
    first = [lru.get_or_create(("shape", k), make) for k in range(8)]
    assert len(made) == 8 and list(lru) == [("shape", k) for k in range(8)]
    hit = lru.get_or_create(("shape", 0), make)                      # a hit: the identical tensors, and the key moves to the end
    assert len(made) == 8 and hit is first[0] and hit["K"] is first[0]["K"] and hit["V"] is first[0]["V"]
    assert list(lru)[-1] == ("shape", 0) and list(lru)[0] == ("shape", 1)
    lru.get_or_create(("shape", 8), make)                            # the ninth shape evicts the least recently used: 1, not 0
    assert len(lru) == 8 and ("shape", 1) not in lru and ("shape", 0) in lru and ("shape", 8) in lru
    assert lru[("shape", 2)] is first[2]                             # plain indexing, as the GPU tests read the scratch


def test_the_two_kinds_of_shape_keep_their_own_eight():
    from flowtron_amd import decode
    step, cpu = make_step(2, True), torch.device("cpu")
    first, (K, V, res, mel, attn, n_done) = decode.shape_bufs(step, "_decode_bufs", (), 1, 3, A, M, cpu)
    assert first is step._decode_bufs[(1, 3, "cpu")] and [first[k] for k in ("K", "V", "res", "mel", "attn", "n_done")] == [K, V, res, mel, attn, n_done]
    assert K.shape == V.shape == (3, A) and res.shape == mel.shape == (1, M) and attn.shape == (1, 3)
    assert n_done.shape == (1,) and n_done.dtype == torch.int32 and all(t.dtype == torch.float32 for t in (K, V, res, mel, attn))
    for N in range(2, 9):
        decode.shape_bufs(step, "_decode_bufs", (), N, 3, A, M, cpu)
    for N in range(1, 9):
        bufs, (K, V, res, mel, attn, n_done) = decode.shape_bufs(step, "_decode_batch_bufs", (2,), N, 3, A, M, cpu)
        assert bufs is step._decode_batch_bufs[(2, N, 3, "cpu")]
        assert K.shape == V.shape == (2, 3, A) and res.shape == mel.shape == (2, N, M) and attn.shape == (2, N, 3) and n_done.shape == (2,)
    assert len(step._decode_bufs) == 8 and len(step._decode_batch_bufs) == 8
    again, tensors = decode.shape_bufs(step, "_decode_bufs", (), 1, 3, A, M, cpu)        # still there: the batched shapes evicted none
    assert again is first and tensors[0] is first["K"]


def test_retry_helper_reads_the_status_only_after_a_persistent_launch(monkeypatch):
    from flowtron_amd import decode, ops
    checks, answer = [], [True]
    monkeypatch.setattr(ops, "check_persist_status", lambda raise_on_failure=True: checks.append(raise_on_failure) or answer[0])
    calls = []
    launch, staged = (lambda: calls.append("launch") or "first"), (lambda: calls.append("staged") or "second")
    assert decode.launch_or_staged(launch, False, staged) == "first" and checks == [] and calls == ["launch"]
    assert decode.launch_or_staged(launch, True, staged) == "first" and checks == [False] and calls == ["launch"] * 2
    answer[0] = False
    assert decode.launch_or_staged(launch, True, staged) == "second" and checks == [False] * 2 and calls == ["launch"] * 3 + ["staged"]


def test_padding_helpers():
    from flowtron_amd import decode
    mels = [torch.full((1, 3, 2), 1.0), torch.full((1, 3, 4), 2.0, dtype=torch.float64)]
    mel, n = decode.pad_mels(mels)
    assert n == [2, 4] and mel.shape == (2, 3, 4) and mel.dtype == torch.float32
    assert torch.equal(mel[0], torch.tensor([[1.0, 1.0, 0.0, 0.0]] * 3)) and torch.equal(mel[1], torch.full((3, 4), 2.0))
    rows = [[torch.full((1, 1, 2), 1.0)] * 2, [], [torch.full((1, 1, 3), 3.0)] * 4]
    out = decode.pad_attn_rows(rows, 4, 5, mel)
    assert len(out) == 4 and all(r.shape == (3, 1, 5) for r in out)
    att = torch.stack(out)
    want = torch.zeros(4, 3, 1, 5)
    want[:2, 0, :, :2] = 1.0
    want[:, 2, :, :3] = 3.0
    assert torch.equal(att, want)


def test_scratch_is_dropped_by_pickle_and_made_again_on_first_use(lib):
    from flowtron_amd import decode
    step, cpu = make_step(2, True), torch.device("cpu")
    keys = list(step.state_dict())

    def use(s):
        """what a first infer and a first infer_batch create"""
        return (decode.shape_bufs(s, "_decode_bufs", (), 5, 3, A, M, cpu)[0], decode.shape_bufs(s, "_decode_batch_bufs", (2,), 5, 3, A, M, cpu)[0],
                decode.scratch(s.__dict__, "_decode_wimg", lib.ft_decode_wimg_bytes(H, A, M), cpu),
                decode.scratch(s.__dict__, "_decode_gran", lib.ft_decode_persist_gran_bytes(), cpu),
                decode.scratch(s.__dict__, "_decode_batch_gran", lib.ft_decode_batch_gran_bytes(4), cpu))
    made = use(step)
    assert all(hasattr(step, a) for a in SCRATCH) and made[2] is step._decode_wimg and made[3] is step._decode_gran
    assert made[2].numel() == lib.ft_decode_wimg_bytes(H, A, M) and made[2].dtype == torch.uint8
    assert all(x is y for x, y in zip(use(step), made))              # a second use: the identical buffers
    assert decode.scratch(step.__dict__, "_decode_wimg", made[2].numel() + 1, cpu) is not made[2]      # too small: a new one
    assert list(step.state_dict()) == keys                          # no scratch became a buffer, parameter or submodule
    copy = pickle.loads(pickle.dumps(step))
    assert not any(hasattr(copy, a) for a in SCRATCH) and not any(k.startswith("_decode_") for k in copy.__dict__)
    assert list(copy.state_dict()) == keys
    assert all(hasattr(step, a) for a in SCRATCH)                   # (the pickled module keeps its own)
    made2 = use(copy)
    assert all(hasattr(copy, a) for a in SCRATCH) and not any(x is y for x, y in zip(made2, use(step)))
    assert made2[0] is copy._decode_bufs[(5, 3, "cpu")] and made2[1] is copy._decode_batch_bufs[(2, 5, 3, "cpu")]
