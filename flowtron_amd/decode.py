"""Host driver of the decode entries (ft_decode_flow, ft_decode_flow_batch, _batch_keys, _batch_forced; csrc/decode*.hip): what
AR_Step.infer and AR_Step.infer_batch (flowtron_amd.model, where their contracts are written down) call.  The scratch lives on
the AR_Step as plain attributes, created on first use (a module unpickled from a checkpoint has none: its __getstate__ drops every
`_decode_*`).  Every entry is looked up as L.lib().ft_... at call time and the utterance loops go through step.infer, so a test
that wraps either on the instance sees every call."""
import collections
import ctypes as C
import os

import torch

from . import _lib as L
from . import ops

_FIELDS = frozenset(n for n, _ in L.DecodeArgs._fields_)


class ShapeLRU(collections.OrderedDict):
    """The buffers of the eight most recently used decode shapes: the decode hipGraph bakes every pointer, so stable addresses =
    one capture, replayed for every later utterance of the shape; the bound keeps a server with varied lengths from growing."""
    def get_or_create(self, key, make):
        if key in self:
            self.move_to_end(key)
        else:
            while len(self) >= 8:
                self.popitem(last=False)
            self[key] = make()
        return self[key]


def shape_bufs(step, attr, lead, N, Lk, A, M, dev):
    """step.<attr>[(*lead, N, Lk, str(dev))] and its six buffers: K, V [*lead, Lk, A], res, mel [*lead, N, M], attn [*lead, N, Lk]
    and n_done.  lead = () for one utterance (`_decode_bufs`), (nb,) for a batched launch (`_decode_batch_bufs`): a ShapeLRU per
    attribute, so each kind keeps its own eight shapes."""
    f32 = dict(device=dev, dtype=torch.float32)
    bufs = step.__dict__.setdefault(attr, ShapeLRU()).get_or_create((*lead, N, Lk, str(dev)), lambda: dict(
        K=torch.empty(*lead, Lk, A, **f32), V=torch.empty(*lead, Lk, A, **f32), res=torch.empty(*lead, N, M, **f32),
        mel=torch.empty(*lead, N, M, **f32), attn=torch.empty(*lead, N, Lk, **f32),
        n_done=torch.zeros(*(lead or (1,)), device=dev, dtype=torch.int32)))
    return bufs, [bufs[k] for k in ("K", "V", "res", "mel", "attn", "n_done")]


def scratch(d, key, nbytes, dev):
    """d[key]: a byte buffer of at least nbytes on dev, allocated when missing, too small or elsewhere.  d = step.__dict__ for the
    weight image (`_decode_wimg`: one per flow, whatever the shape or the entry) and the granules, a shape's entry for `work`."""
    buf = d.get(key)
    if buf is None or buf.numel() < nbytes or buf.device != dev:
        buf = d[key] = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    return buf


def decode_args(step, **fields):
    """ft_decode_args (include/flowtron_hip.h) filled by field name: the weights every entry takes, H, A, M, temperature, gate_threshold
    (2.0 without a gate layer: never reached) and n_layers from `step`; what differs between the paths from `fields` -- a tensor stands for
    its address, `work` and `wimg` set their byte counts too -- and the rest null / zero.  The caller keeps the tensors alive until the launch."""
    if not fields.keys() <= _FIELDS:
        raise TypeError("ft_decode_args has no field %s" % sorted(fields.keys() - _FIELDS))
    a, p, d, att = step.attention_lstm, step.lstm, step.dense_layer.layers, step.attention_layer
    w = dict(att_w_ih=a.weight_ih_l0, att_w_hh=a.weight_hh_l0, att_b_ih=a.bias_ih_l0, att_b_hh=a.bias_hh_l0,
             w_query=att.query.linear_layer.weight, v=att.v.linear_layer.weight,
             l0_w_ih=p.weight_ih_l0, l0_w_hh=p.weight_hh_l0, l0_b_ih=p.bias_ih_l0, l0_b_hh=p.bias_hh_l0,
             d0_w=d[0].linear_layer.weight, d0_b=d[0].linear_layer.bias, d1_w=d[1].linear_layer.weight, d1_b=d[1].linear_layer.bias,
             conv_w=step.conv.weight, conv_b=step.conv.bias)
    if step.n_lstm_layers >= 2:
        w.update(l1_w_ih=p.weight_ih_l1, l1_w_hh=p.weight_hh_l1, l1_b_ih=p.bias_ih_l1, l1_b_hh=p.bias_hh_l1)
    has_gate = hasattr(step, "gate_layer")
    if has_gate:
        w.update(gate_w=step.gate_layer.linear_layer.weight, gate_b=step.gate_layer.linear_layer.bias)
    w.update(fields)
    w.update({name + "_bytes": w[name].numel() for name in ("work", "wimg") if w.get(name) is not None})
    return L.DecodeArgs(H=p.weight_hh_l0.shape[1], A=att.key.linear_layer.weight.shape[0], M=step.conv.weight.shape[0] // 2,
                        temperature=float(att.temperature), gate_threshold=float(step.gate_threshold) if has_gate else 2.0,
                        n_layers=step.n_lstm_layers,
                        **{name: val.data_ptr() if isinstance(val, torch.Tensor) else val for name, val in w.items()})


def launch_or_staged(launch, persistent, staged):
    """launch(); where that went to a persistent kernel (`persistent`) and one did not complete (grid not co-resident: logged once by
    ops, which switches the device to the staged kernels) staged() in its place, unseen by the caller.  -> what the one that stands returned."""
    r = launch()
    return staged() if persistent and not ops.check_persist_status(raise_on_failure=False) else r


def pad_mels(mels):
    """per-utterance mels [1, M, n_b] -> (float32 [B, M, max n_b], zeros behind each utterance's frames; the list of n_b)"""
    n = [int(m.shape[2]) for m in mels]
    mel = mels[0].new_zeros(len(mels), mels[0].shape[1], max(n), dtype=torch.float32)
    for b, m in enumerate(mels):
        mel[b, :, :n[b]] = m[0]
    return mel, n


def pad_attn_rows(rows, n, width, like):
    """rows[b] = utterance b's attention rows, each [1, 1, L_b] -> a list of n rows [B, 1, width] of `like`'s type, zeros behind
    an utterance's rows and behind its text"""
    att = like.new_zeros(n, len(rows), 1, width)
    for b, r in enumerate(rows):
        if r:
            att[:len(r), b, :, :r[0].shape[-1]] = torch.stack([x.reshape(1, -1) for x in r])
    return [att[t] for t in range(n)]


def infer(step, residual, text, attns, attn_prior, use_graph):
    """AR_Step.infer"""
    N, B, M = residual.shape
    if B != 1:
        if attns is not None:
            raise ValueError("forced alignments (attns=) are taken one utterance at a time")
        outs = [step.infer(residual[:, b:b + 1].contiguous(), text[:, b:b + 1].contiguous(), None,
                           None if attn_prior is None else attn_prior[b:b + 1], use_graph) for b in range(B)]
        n = max(m.shape[0] for m, _ in outs)
        mel = residual.new_zeros(n, B, M)
        for b, (m, _) in enumerate(outs):
            mel[:m.shape[0], b] = m[:, 0]
        return mel, pad_attn_rows([rows for _, rows in outs], n, text.shape[0], residual)
    L.require_cuda(residual, text)
    Lk, E = text.shape[0], text.shape[2]
    att = step.attention_layer
    H, A = step.lstm.weight_hh_l0.shape[1], att.key.linear_layer.weight.shape[0]
    dev = residual.device
    bufs, (K, V, res, mel_out, attn_out, n_done) = shape_bufs(step, "_decode_bufs", (), N, Lk, A, M, dev)
    K.copy_(ops.linear(text, att.key.linear_layer.weight, None).reshape(Lk, A))
    V.copy_(ops.linear(text, att.value.linear_layer.weight, None).reshape(Lk, A))
    res.copy_(residual.reshape(N, M))
    attn_out.zero_()
    # (the temporaries from here on are locals of this frame or held by `fields`: alive until the launch is enqueued)
    prior_rows = forced_rows = None
    if attn_prior is not None:              # [1, N, L] (flowtron.py:799 takes attn_prior[:, i])
        prior_rows = attn_prior.reshape(-1, Lk)[:N].contiguous().float()
        assert prior_rows.shape[0] == N, "attn_prior must cover every residual frame"
    if attns is not None:                   # N rows of [L] (flowtron.py:798 takes attns[i])
        forced_rows = (torch.stack([a_.reshape(-1) for a_ in attns]) if isinstance(attns, (list, tuple)) else attns.reshape(-1, Lk))
        forced_rows = forced_rows[:N].contiguous().float()
        assert forced_rows.shape == (N, Lk), "attns must hold one attention row per residual frame"
    L.require_cuda(prior_rows, forced_rows)
    cumm, nl, has_gate = step.use_cumm_attention, step.n_lstm_layers, hasattr(step, "gate_layer")
    enc2d = text.reshape(Lk, E).contiguous()
    work = scratch(bufs, "work", L.lib().ft_decode_workspace_bytes(Lk, H, A, M, E if cumm else 1, nl), dev)
    use_graph = os.environ.get("FLOWTRON_DECODE_GRAPH", "1") != "0" if use_graph is None else use_graph
    fields = {}
    if cumm:
        c1, c2 = step.attn_cond_layer.location_conv_hidden.conv, step.attn_cond_layer.location_conv_out.conv
        fields = dict(cond_w1=c1.weight, cond_b1=c1.bias, cond_w2=c2.weight, cond_b2=c2.bias, w_key=att.key.linear_layer.weight, enc=enc2d)
    if nl > 2:
        # decoder layers beyond the second (any n_lstm_layers, flowtron.py:654-655): a host array of their four tensors each
        ptrs = [L.ptr(getattr(step.lstm, "%s_l%d" % (nm, k))) for k in range(2, nl) for nm in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
        extra = (C.c_void_p * len(ptrs))(*ptrs)
        fields["extra_layers"] = C.cast(extra, C.c_void_p)
    # 16-bit operand modes: bf16 images of the weights (half the bytes; fp32 activations)
    wimg = scratch(step.__dict__, "_decode_wimg", L.lib().ft_decode_wimg_bytes(H, A, M), dev) if L.is16(L.mfma_mode()) else None
    # one persistent launch per flow (csrc/decode.hip dec_persist_k) where its geometry applies: 16-bit weight images fully register-
    # resident, or (fp32 mode = the reference's inference precision) the fp32 originals, the recurrent matrices resident, the rest streamed
    persistent = nl == 2 and os.environ.get("FLOWTRON_DECODE_PERSIST", "1") != "0" and ops.persist_usable(dev)
    gran = scratch(step.__dict__, "_decode_gran", L.lib().ft_decode_persist_gran_bytes(), dev) if persistent else None
    args = decode_args(step, K=K, V=V, residual=res, mel_out=mel_out, attn_out=attn_out, n_done_dev=n_done, work=work, N=N, L=Lk, E=E,
                       use_graph=int(bool(use_graph)), prior=prior_rows, forced=forced_rows, wimg=wimg, persist_gran=gran,
                       persist_status=ops.persist_status(dev) if persistent else None, **fields)

    def launch():
        L.check(L.lib().ft_decode_flow(C.byref(args), L.stream()), "ft_decode_flow")
        return int(n_done.item()) if has_gate else N          # single host read per flow (the reference syncs every frame)

    def staged():
        args.persist_gran = args.persist_status = None
        attn_out.zero_()
        return launch()
    n = launch_or_staged(launch, persistent, staged)
    # (clones: the persistent buffers are overwritten by the next call)
    return mel_out[:n].clone().reshape(n, 1, M), [row.reshape(1, 1, Lk) for row in attn_out[:n].clone()]


def infer_batch(step, x, text, lens, in_lens, forced):
    """AR_Step.infer_batch"""
    (T, B, M), Lk = x.shape, text.shape[0]
    il = list(in_lens) if in_lens is not None else [Lk] * B
    att = step.attention_layer
    H, A = step.lstm.weight_hh_l0.shape[1], att.key.linear_layer.weight.shape[0]
    dev = x.device
    f32 = dict(device=dev, dtype=torch.float32)
    NB = L.lib().ft_decode_batch_max()
    out = torch.zeros(T, B, M, **f32)
    attn = torch.zeros(T, B, 1, Lk, **f32)
    n_done_all = torch.zeros(B, device=dev, dtype=torch.int32)
    lim_host = torch.tensor(lens, dtype=torch.int32).pin_memory()
    lim_all = lim_host.to(dev, non_blocking=True)
    keys_all = torch.tensor(il, dtype=torch.int32).pin_memory().to(dev, non_blocking=True)
    gran = scratch(step.__dict__, "_decode_batch_gran", L.lib().ft_decode_batch_gran_bytes(NB), dev)
    # bf16 weight images, rounded by the flow's first batched launch
    wimg = scratch(step.__dict__, "_decode_wimg", L.lib().ft_decode_wimg_bytes(H, A, M), dev) if L.is16(L.mfma_mode()) else None
    groups = [list(range(g0, min(g0 + NB, B))) for g0 in range(0, B, NB)]
    singles = [g[0] for g in groups if len(g) == 1 and forced is None]      # a group of one: ft_decode_flow, unless rows are given
    batched = [g for g in groups if len(g) > 1 or forced is not None]
    n = list(lens)

    def launch():                                            # -> the utterances left to decode alone
        for g in batched:
            g0, nb, Ng = g[0], len(g), max(lens[b] for b in g)
            bufs, (K, V, res, mel_out, attn_out, n_done) = shape_bufs(step, "_decode_batch_bufs", (nb,), Ng, Lk, A, M, dev)
            for j, b in enumerate(g):
                # the projections of infer(), one utterance at a time over its own positions (rows behind them are not read)
                tb = text[:il[b], b:b + 1].contiguous()
                if forced is None:
                    K[j, :il[b]].copy_(ops.linear(tb, att.key.linear_layer.weight, None).reshape(il[b], A))
                V[j, :il[b]].copy_(ops.linear(tb, att.value.linear_layer.weight, None).reshape(il[b], A))
            res.copy_(x[:Ng, g0:g0 + nb].transpose(0, 1))
            mel_out.zero_()                                      # rows past an utterance's end are not written
            attn_out.zero_()
            rows = None
            if forced is not None:
                # [nb][Ng][Lk] in a buffer of the group's own: the entry wants 16-byte aligned rows, and `forced` may be a view
                # at any offset of the caller's tensor (a flow's slice of [F,B,N,L], a sliced batch)
                rows = bufs.get("forced")
                if rows is None:
                    rows = bufs["forced"] = torch.empty(nb, Ng, Lk, **f32)
                rows.copy_(forced[g0:g0 + nb, :Ng])
            args = decode_args(step, K=K if forced is None else None, V=V, residual=res, mel_out=mel_out, attn_out=attn_out,
                               n_done_dev=n_done, N=Ng, L=Lk, E=1, forced=rows, wimg=wimg, persist_gran=gran,
                               persist_status=ops.persist_status(dev))
            # wimg_ready: the flow's first batched launch rounds the weights, the later ones find the images
            bargs = L.DecodeBatchArgs(a=args, nb=nb, n_lim=L.ptr(lim_all[g0:g0 + nb]), wimg_ready=int(g is not batched[0]))
            keys = L.ptr(keys_all[g0:g0 + nb]) if any(il[b] < Lk for b in g) else None
            if forced is not None:
                L.check(L.lib().ft_decode_flow_batch_forced(C.byref(bargs), keys, L.stream()), "ft_decode_flow_batch_forced")
            elif keys is not None:                               # texts of different lengths: a key count per utterance
                L.check(L.lib().ft_decode_flow_batch_keys(C.byref(bargs), keys, L.stream()), "ft_decode_flow_batch_keys")
            else:
                L.check(L.lib().ft_decode_flow_batch(C.byref(bargs), L.stream()), "ft_decode_flow_batch")
            # copied out on the stream: the next group may reuse these buffers
            out[:Ng, g0:g0 + nb] = mel_out.transpose(0, 1)
            attn[:Ng, g0:g0 + nb, 0] = attn_out.transpose(0, 1)
            n_done_all[g0:g0 + nb] = n_done
        return singles
    # a batched launch that did not complete: its groups again, one utterance at a time like the groups of one (infer() keeps its own
    # fallback; given rows: its staged forced decode)
    alone = launch_or_staged(launch, bool(batched), lambda: sorted(singles + sum(batched, [])))
    if batched and alone == singles and hasattr(step, "gate_layer"):
        n = n_done_all.tolist()                              # the flow's one host read
    for b in alone:
        m_, rows = step.infer(x[:lens[b], b:b + 1].contiguous(), text[:il[b], b:b + 1].contiguous(),
                              None if forced is None else forced[b, :lens[b], :il[b]].contiguous().float())
        n[b] = m_.shape[0]
        out[:, b] = 0.0
        attn[:, b] = 0.0
        out[:n[b], b] = m_[:, 0]
        if rows:
            attn[:n[b], b, :, :il[b]] = torch.cat(rows, 0)
    return out, attn, n
