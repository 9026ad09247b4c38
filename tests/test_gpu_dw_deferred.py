"""-m gpu: the weight-gradient GEMMs of a backward pass deferred into grouped launches (ops.weight_grad_gemm, ops.flush_weight_grads,
ops._DW_GROUP) against the same pass with every GEMM launched at once.

What is compared.  The grouped launch multiplies the very operand images the immediate launch multiplies, so each weight gradient
is held against the float64 product of THOSE images (decoded from the queue: tests/gemm_ref64.py's reference and bound, with the
slices of the plan that ran), and the immediate result against the same reference under the bound of either extreme the single
call's own planner can choose (one slice, or 64 combined by atomics).  Input gradients do not pass through the changed code:
bit-identical.  Gradients that reach a parameter through fp32 atomics elsewhere (bias column sums, the gate layer's GEMV^T, the staging
GEMMs, scatter-adds) differ between two runs of the SAME code: the op-level tests leave them out, the model-level test holds them to
four times that run-to-run difference plus 2^-20 of the gradient's norm (sixteen units of fp32 at the size of the result: a
reordered fp32 sum).  The queue tests run on integer data whose every partial sum is exact in fp32 (below 2^24), so deferred and
immediate must be EQUAL."""
import pytest
import torch

import gemm_ref64 as R

pytestmark = pytest.mark.gpu
H = 1024


@pytest.fixture(scope="module")
def env():
    from flowtron_amd import _lib as L
    from flowtron_amd import ops
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return L, ops


class Recorder:
    """wraps ops._dw_run: keeps every queue item that was launched (its argument struct and the references the queue held)"""

    def __init__(self, ops, monkeypatch):
        self.ops, self.batches = ops, []
        real = ops._dw_run
        monkeypatch.setattr(ops, "_dw_run", lambda batch: (self.batches.append(list(batch)), real(batch))[1])

    @property
    def problems(self):
        return sum(len(b) for b in self.batches)

    def references(self):
        """{C address: (C alias, float64 reference, bound of the grouped plan, bound of the single call's extremes)} of every problem"""
        ops, out = self.ops, {}
        for batch in self.batches:
            plans = ops.gemm_img_group_plan([it[0] for it in batch])
            for (a, fmt, _st, _dev, keep), pl in zip(batch, plans):
                A, B, Cm, rowmap, _bias = keep
                k_len = a.K if a.compact != 2 else max(0, int(rowmap.rows.item()) - a.k_shift)

                def matrix(buf, ptr, ld, cols):
                    flat = buf.view(ops.op16_dtype(fmt))
                    e = (ptr - buf.data_ptr()) // 2
                    return flat[e:].as_strided((k_len, cols), (ld, 1)).double().t().contiguous()

                a64, b64 = matrix(A, a.A, a.lda, a.M), matrix(B, a.B, a.ldb, a.N)
                assert a.alpha == 1.0 and a.bias is None             # (C starts at zero: beta decides nothing about the value)
                beta = float(a.beta)
                ref, bound = R.reference(a64, b64, beta=beta, fmt=fmt, slices=pl.splits, split=bool(pl.atomics))
                b1 = R.reference(a64, b64, beta=beta, fmt=fmt, slices=1, split=False)[1]
                b64s = R.reference(a64, b64, beta=beta, fmt=fmt, slices=64, split=True)[1]
                assert Cm.data_ptr() not in out, "two problems of one pass write one C: not expected in these graphs"
                out[Cm.data_ptr()] = (Cm, ref, bound, torch.maximum(b1, b64s))
        return out


def compare(on, off, refs, names_bitwise, tag, skip=()):
    """on / off: {name: gradient}; refs: Recorder.references() of the `on` pass; names_bitwise: gradients that must be equal;
    skip: gradients summed by atomics outside the changed code"""
    held = 0
    for n, g in on.items():
        if n in skip:
            continue
        if n in names_bitwise:
            assert torch.equal(g, off[n]), "%s: %s differs between deferred and immediate" % (tag, n)
            continue
        hit = refs.get(on.ptr[n])
        assert hit is not None, "%s: the gradient of %s did not come out of a grouped launch" % (tag, n)
        _, ref, bound, bound_single = hit
        r_on, r_off = R.ratio(g.reshape(ref.shape), ref, bound), R.ratio(off[n].reshape(ref.shape), ref, bound_single)
        print("%s %s: deferred %.3f x its bound, immediate %.3f x its bound" % (tag, n, r_on, r_off))
        assert r_on <= 1.0 and r_off <= 1.0, (tag, n, r_on, r_off)
        held += 1
    return held


class Grads(dict):
    """{name: a copy of the gradient}; .ptr[name] = the address of the gradient itself (what a grouped problem wrote to)"""


def run_pass(ops, on, monkeypatch, body):
    monkeypatch.setattr(ops, "_DW_GROUP", on)
    out = body()
    torch.cuda.synchronize()
    assert not ops._DWQ["items"], "the queue is not empty after backward()"
    g = Grads((n, t.clone()) for n, t in out.items())
    g.ptr = {n: t.data_ptr() for n, t in out.items()}
    for n, t in g.items():
        assert bool(torch.isfinite(t).all()), "%s: %d non-finite elements (deferred: %s)" % (n, int((~torch.isfinite(t)).sum()), on)
    return g


@pytest.mark.parametrize("inputs", [1, 2])
def test_linear_weight_gradient_deferred_against_immediate(env, monkeypatch, inputs):
    """LinearFn over a row map: one input, and two inputs as one concatenated image"""
    L, ops = env
    T, B, N, mode = 48, 32, 1024, L.FT_BF16
    torch.manual_seed(5)
    Ks = [H, 640][:inputs]
    W = (torch.randn(N, sum(Ks), device="cuda") / 30).requires_grad_(True)
    bias = torch.zeros(N, device="cuda", requires_grad=True)
    lens = torch.randint(10, T + 1, (B,), dtype=torch.int32)
    lens[3] = T
    lens = lens.cuda()
    xs0 = [torch.randn(T, B, K, device="cuda") * 0.3 for K in Ks]
    dy = torch.randn(T, B, N, device="cuda") * 0.1

    def body():
        xs = [x.clone().requires_grad_(True) for x in xs0]
        W.grad = bias.grad = None
        rm = ops.row_map(lens, T, B)
        y = ops.linear(xs, W, bias, mode=mode, rowmap=rm, fill="y+dx")
        (y * dy).sum().backward()
        torch.cuda.synchronize()
        g = {"W": W.grad, "bias": bias.grad}
        g.update({"x%d" % i: x.grad for i, x in enumerate(xs)})
        return g

    rec = Recorder(ops, monkeypatch)
    on = run_pass(ops, True, monkeypatch, body)
    refs = rec.references()
    assert rec.problems == 1
    off = run_pass(ops, False, monkeypatch, body)
    assert rec.problems == 1, "_DW_GROUP = False still deferred"
    assert compare(on, off, refs, {"x%d" % i for i in range(inputs)}, "linear/%d" % inputs, skip={"bias"}) == 1


@pytest.mark.parametrize("pair", [False, True])
def test_recurrence_weight_gradients_deferred_against_immediate(env, monkeypatch, pair):
    """the decoder LSTM (nn.LSTM(1664, 1024, 2) with the gate layer riding on layer 0's projection) as two ops.lstm_layer calls
    (LinearGateFn / LinearFn + LSTMSeqFn) and as ops.decoder_pair (DecoderPairFn), at the shape of tests/test_gpu_roles.py"""
    L, ops = env
    import torch.nn as nn
    if not ops.persist_usable(torch.device("cuda", 0)):
        pytest.skip("persistent kernels not usable on this device")
    T, B, A, mode = 48, 32, 640, L.FT_BF16
    torch.manual_seed(3)
    p = nn.LSTM(H + A, H, 2).cuda()
    gw, gb = (torch.randn(1, H + A, device="cuda") * 0.02).requires_grad_(True), torch.zeros(1, device="cuda", requires_grad=True)
    lens = torch.randint(10, T + 1, (B,), dtype=torch.int32)
    lens[3] = T
    lens = lens.cuda()
    x0, c0 = torch.randn(T, B, H, device="cuda") * 0.3, torch.randn(T, B, A, device="cuda") * 0.3
    dh, dg = torch.randn(T, B, H, device="cuda") * 0.1, torch.randn(T, B, 1, device="cuda") * 0.1
    valid = (torch.arange(T, device="cuda")[:, None] < lens[None, :])[..., None].float()

    def body():
        x, cx = x0.clone().requires_grad_(True), c0.clone().requires_grad_(True)
        for q in list(p.parameters()) + [gw, gb]:
            q.grad = None
        rm = ops.row_map(lens, T, B)
        if pair:
            h, gates = ops.decoder_pair(x, lens, p, mode, [cx], rm, "dx", (gw, gb), 3)
        else:
            h0, gates = ops.lstm_layer(x, lens, p.weight_ih_l0, p.weight_hh_l0, p.bias_ih_l0, p.bias_hh_l0, mode=mode, xs_extra=[cx], rowmap=rm,
                                       fill="dx", gate=(gw, gb))
            h = ops.lstm_layer(h0, lens, p.weight_ih_l1, p.weight_hh_l1, p.bias_ih_l1, p.bias_hh_l1, mode=mode, rowmap=rm)
        ((h * dh).sum() + (gates * dg * valid).sum()).backward()
        torch.cuda.synchronize()
        assert ops.check_persist_status(), "a persistent launch timed out"
        g = {n: q.grad for n, q in p.named_parameters()}
        g.update(gw=gw.grad, gb=gb.grad, x=x.grad * valid, cx=cx.grad * valid)
        return g

    rec = Recorder(ops, monkeypatch)
    on = run_pass(ops, True, monkeypatch, body)
    refs = rec.references()
    assert rec.problems == 4 and len(rec.batches) == 1, "four weight gradients in one call: %s" % [len(b) for b in rec.batches]
    off = run_pass(ops, False, monkeypatch, body)
    weights = {"weight_ih_l0", "weight_hh_l0", "weight_ih_l1", "weight_hh_l1"}
    assert compare(on, off, refs, {"x", "cx"}, "pair" if pair else "layers", skip=set(on) - weights - {"x", "cx"}) == 4


def small_model(monkeypatch):
    import flowtron
    from oracle import synth
    monkeypatch.setenv("FLOWTRON_MFMA", "bf16")
    cfg = dict(synth.SMALL_MODEL_CONFIG)
    m = flowtron.Flowtron(**cfg)
    m.load_state_dict(synth.make_state_dict(cfg, seed=9))
    m = m.cuda().eval()
    crit = flowtron.FlowtronLoss(1.0, False, True, True, 0.01, -8)

    def step(out_lens, in_lens, seed):
        bc = synth.make_batch(cfg, out_lens, in_lens, seed=seed, with_prior=True)
        b = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in bc.items()}
        for q in m.parameters():
            q.grad = None
        out = m(b["mel"], b["speaker_ids"], b["text"], b["in_lens"], b["out_lens"], b["attn_prior"])
        nll, gl, ctc = crit(out, b["gate_target"], b["in_lens"], b["out_lens"])
        (nll + gl + 0.01 * ctc).backward()
        torch.cuda.synchronize()
        return {n: q.grad for n, q in m.named_parameters() if q.grad is not None}

    return m, step


def test_small_model_all_parameter_gradients_and_two_shapes_in_a_row(env, monkeypatch):
    """oracle.synth.SMALL_MODEL_CONFIG, two steps of different (T, L) in a row: every parameter gradient, deferred against immediate"""
    L, ops = env
    m, step = small_model(monkeypatch)
    # (whole-length utterances: the compact row maps of ragged batches are the op-level tests' part, at the kernels' own H)
    shapes = [([29, 29, 29], [11, 8, 4], 9), ([40, 40, 40, 40], [6, 13, 9, 3], 4)]
    rec = Recorder(ops, monkeypatch)
    for out_lens, in_lens, seed in shapes:
        rec.batches.clear()
        on = run_pass(ops, True, monkeypatch, lambda: step(out_lens, in_lens, seed))
        refs = rec.references()
        assert rec.problems >= 1, "the small model defers no weight gradient: this test holds nothing"
        launched = rec.problems
        off1 = run_pass(ops, False, monkeypatch, lambda: step(out_lens, in_lens, seed))
        off2 = run_pass(ops, False, monkeypatch, lambda: step(out_lens, in_lens, seed))
        assert rec.problems == launched
        assert set(on) == set(off1)
        grouped = {n for n in on if on.ptr[n] in refs}
        for n in set(on) - grouped:
            noise = float((off1[n] - off2[n]).norm())
            d = float((on[n] - off1[n]).norm())
            assert d <= 4.0 * noise + 2.0 ** -20 * float(off1[n].norm()), (n, d, noise)
        assert compare(on, off1, refs, set(), "small model T=%d" % max(out_lens), skip=set(on) - grouped) == len(grouped)


def two_layers(ops, L, seed=0):
    T, B, mode = 40, 32, L.FT_BF16
    torch.manual_seed(seed)
    # integers: |y1| <= 512 (its 16-bit image rounds to integers), |y2| <= 2^19, |dy2| <= 2, |dW2| <= 1280 * 2 * 512, |dy1| <= 1536,
    # |dW1| <= 1280 * 1536 -- every sum stays below 2^24 in any order
    tri = lambda *shape: torch.randint(-1, 2, shape, device="cuda").float()
    W1, W2 = tri(1024, 512).requires_grad_(True), tri(768, 1024).requires_grad_(True)
    lens = torch.full((B,), T, dtype=torch.int32).cuda()
    x, dyc = tri(T, B, 512), torch.randint(-2, 3, (T, B, 768), device="cuda").float()

    def forward():
        W1.grad = W2.grad = None
        rm = ops.row_map(lens, T, B)
        y1 = ops.linear([x], W1, None, mode=mode, rowmap=rm, fill="y+dx")
        y2 = ops.linear([y1], W2, None, mode=mode, rowmap=rm, fill="y+dx")
        return y1, (y2 * dyc).sum()

    return W1, W2, forward


def immediate(ops, monkeypatch, W1, W2, forward):
    monkeypatch.setattr(ops, "_DW_GROUP", False)
    forward()[1].backward()
    torch.cuda.synchronize()
    monkeypatch.setattr(ops, "_DW_GROUP", True)
    return W1.grad.clone(), W2.grad.clone()


def close(a, b):
    """integer data, exact sums: equal, and not trivially so"""
    return bool(torch.equal(a, b)) and float(b.abs().max()) > 0.0


def test_a_pass_that_raises_leaves_nothing_stale(env, monkeypatch):
    L, ops = env
    W1, W2, forward = two_layers(ops, L)
    g1, g2 = immediate(ops, monkeypatch, W1, W2, forward)
    rec = Recorder(ops, monkeypatch)

    def boom(_g):
        raise RuntimeError("hook")

    y1, loss = forward()
    y1.register_hook(boom)
    with pytest.raises(RuntimeError, match="hook"):
        loss.backward()
    torch.cuda.synchronize()
    assert rec.problems == 0 and len(ops._DWQ["items"]) == 1, "W2's gradient was queued, the pass died before the flush"
    forward()[1].backward()
    torch.cuda.synchronize()
    assert rec.problems == 2 and not ops._DWQ["items"], "the dead pass's problem was launched: %d problems" % rec.problems
    assert close(W1.grad, g1) and close(W2.grad, g2)


def test_autograd_grad_on_a_sub_graph_flushes(env, monkeypatch):
    L, ops = env
    W1, W2, forward = two_layers(ops, L)
    g1, g2 = immediate(ops, monkeypatch, W1, W2, forward)
    rec = Recorder(ops, monkeypatch)
    (d2,) = torch.autograd.grad(forward()[1], [W2])
    torch.cuda.synchronize()
    assert rec.problems == 1 and not ops._DWQ["items"]
    assert close(d2, g2) and W1.grad is None and W2.grad is None


def test_flush_in_the_middle_of_a_pass(env, monkeypatch):
    """ops.flush_weight_grads() from a parameter hook: the gradients of the parameters already seen are complete at that point"""
    L, ops = env
    W1, W2, forward = two_layers(ops, L)
    g1, g2 = immediate(ops, monkeypatch, W1, W2, forward)
    rec = Recorder(ops, monkeypatch)
    seen = {}

    def hook(_p):
        seen["before"] = W2.grad.clone()                 # W2's node ran, its GEMM waits
        ops.flush_weight_grads()
        seen["after"] = W2.grad.clone()

    h = W1.register_post_accumulate_grad_hook(hook)
    forward()[1].backward()
    torch.cuda.synchronize()
    h.remove()
    assert float(seen["before"].abs().max()) == 0.0, "nothing was deferred: this test holds nothing"
    assert torch.equal(seen["after"], W2.grad) and close(W2.grad, g2) and close(W1.grad, g1)
    assert [len(b) for b in rec.batches] == [2], "W1's own gradient is queued before its hook runs: both leave in the hook's flush"


@pytest.mark.parametrize("second", ["image path", "staging path"])
def test_a_weight_used_twice_in_one_pass(env, monkeypatch, second):
    """the engine adds the two gradients of a weight as soon as the second arrives: the queued first one must have been written by then
    -- also when the second never meets the queue (16 rows are too few for the image path: the fp32-staging GEMM).  Integer data."""
    L, ops = env
    mode = L.FT_BF16
    torch.manual_seed(1)
    tri = lambda *shape: torch.randint(-1, 2, shape, device="cuda").float()
    W = tri(1024, 512).requires_grad_(True)
    x1, x2 = tri(40, 32, 512), tri(40 if second == "image path" else 1, 32 if second == "image path" else 16, 512)
    d1, d2 = tri(40, 32, 1024), tri(*x2.shape[:2], 1024)

    def run(on):
        monkeypatch.setattr(ops, "_DW_GROUP", on)
        W.grad = None
        ((ops.linear([x1], W, None, mode=mode) * d1).sum() + (ops.linear([x2], W, None, mode=mode) * d2).sum()).backward()
        torch.cuda.synchronize()
        assert not ops._DWQ["items"]
        return W.grad.clone()

    rec = Recorder(ops, monkeypatch)
    on = run(True)
    # one of the two gradients waits and the other flushes and runs at once -- or, where the staging GEMM's node comes first, none waits
    assert rec.problems == 1 if second == "image path" else rec.problems <= 1, rec.problems
    want = d1.reshape(-1, 1024).t().double() @ x1.reshape(-1, 512).double() + d2.reshape(-1, 1024).t().double() @ x2.reshape(-1, 512).double()
    assert torch.equal(on.double(), want) and torch.equal(run(False), on)
