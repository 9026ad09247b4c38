"""Host-side mirror of the reference model interface (flowtron.py): same class names, ctor
arguments, submodule attribute names (hence identical state_dict keys) and
forward/infer signatures -- every tensor op underneath is a HIP kernel reached through the
C ABI (flowtron_amd.ops).  torch.nn modules are used only as PARAMETER CONTAINERS (so that
checkpoints keep their layout); their torch forward() is never called.

Reference lines are cited per class.  There is no CPU path: calling forward/infer with
CPU tensors raises (the CPU oracle is oracle/flowtron_oracle.py, test infrastructure).
"""
from __future__ import annotations

import numbers
import os

import numpy as np
import torch
from torch import nn

from . import _lib as L
from . import decode
from . import ops

# NOTE: train.py-format checkpoints pickle the whole nn.Module; torch >= 2.6 refuses them under the default
# weights_only=True.  Running the reference's unmodified train.py resume path (train.py:87,112) therefore needs
# TORCH_FORCE_NO_WEIGHTS_ONLY_LOAD=1 in the environment of THAT process -- this package does not change
# the process-wide torch.load safety default at import.


# --------------------------------------------------------------------------
# thin wrappers (names are baked into state_dict keys) -- flowtron.py:278-309, 95-126, 453-464
# --------------------------------------------------------------------------
class LinearNorm(nn.Module):
    def __init__(self, in_dim, out_dim, bias=True, w_init_gain="linear"):
        super().__init__()
        self.linear_layer = nn.Linear(in_dim, out_dim, bias=bias)
        nn.init.xavier_uniform_(self.linear_layer.weight, gain=nn.init.calculate_gain(w_init_gain))

    def forward(self, x, act=L.ACT_NONE, rowmap=None, fill="y+dx"):
        return ops.linear(x, self.linear_layer.weight, self.linear_layer.bias, act, rowmap=rowmap, fill=fill)


class ConvNorm(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size=1, stride=1, padding=None, dilation=1,
                 bias=True, w_init_gain="linear"):
        super().__init__()
        if padding is None:
            assert kernel_size % 2 == 1
            padding = int(dilation * (kernel_size - 1) / 2)
        assert stride == 1 and dilation == 1, "the hot path only uses stride-1, undilated convolutions"
        self.conv = nn.Conv1d(in_channels, out_channels, kernel_size=kernel_size, stride=stride,
                              padding=padding, dilation=dilation, bias=bias)
        nn.init.xavier_uniform_(self.conv.weight, gain=nn.init.calculate_gain(w_init_gain))


class MaskedInstanceNorm1d(nn.Module):
    """Parameter holder for the length-masked instance norm (flowtron.py:95-126):
    affine, no running statistics -> state_dict has exactly `weight` and `bias`."""

    def __init__(self, num_features, eps=1e-5, affine=True, **_):
        super().__init__()
        self.eps = eps
        self.weight = nn.Parameter(torch.ones(num_features))
        self.bias = nn.Parameter(torch.zeros(num_features))


class DenseLayer(nn.Module):
    def __init__(self, in_dim=1024, sizes=(1024, 1024)):
        super().__init__()
        sizes = list(sizes)
        in_sizes = [in_dim] + sizes[:-1]
        self.layers = nn.ModuleList([LinearNorm(i, o, bias=True) for i, o in zip(in_sizes, sizes)])

    def forward(self, x, rowmap=None):
        for lin in self.layers:
            # GEMM with bias + tanh fused in the epilogue; with a row map only valid frames are multiplied, and since the only
            # reader of a dense output is the next compact GEMM, padded rows stay unwritten (fill = "")
            x = lin(x, L.ACT_TANH, rowmap=rowmap, fill="")
        return x


def encoder_operand_modes():
    """(conv_mode, lstm_mode) of the text encoder -- and of the mel encoder, which follows it -- for the current operand mode."""
    # FLOWTRON_ENCODER_F32 = conv | all: the encoder's convolutions (and its BiLSTM) with fp32 operands inside a 16-bit step -- 2 % of
    # the step's FLOPs; measures how much of the 16-bit gradient noise of the embedding / encoder parameters is made HERE
    enc32 = os.environ.get("FLOWTRON_ENCODER_F32", "")
    conv_mode = L.FT_F32 if enc32 in ("conv", "all") else None
    lstm_mode = L.FT_F32 if enc32 == "all" else None
    m16 = L.mfma_mode()
    if L.is16(m16) and enc32 in ("fwd", "dx", "dw", "fwd+dx"):      # one GEMM of the three in fp32 operands (which one makes the noise?)
        conv_mode = (L.FT_F32 if "fwd" in enc32 else m16, L.FT_F32 if "dx" in enc32 else m16, L.FT_F32 if "dw" in enc32 else m16)
    elif L.is16(m16) and enc32 in ("", "split"):
        # DEFAULT in the 16-bit modes (round 5): the convolutions' FORWARD products from split images (x = hi + lo: one 16-bit GEMM
        # over [hi | lo | hi] x [hi | hi | lo], ops.Bf16Image.split3), backward in the step's 16-bit format.  The products come out
        # 2.5 to 3 digits better than 16-bit operands give (measured at this weight scale, share of sum |x w|: bf16 3e-6 for 1.4e-3,
        # fp16 4e-7 for 2e-4; fp16's weight lo is subnormal, which caps it there: csrc/gemm_bf16.hip) -- "fp32 grade" below means that.
        # Measured on the bench batch: the 16-bit rounding of these three forward GEMMs -- renormalised by the instance norm
        # behind each -- was what made the text-embedding / encoder gradients deviate 0.11 from the fp32 oracle (the real
        # reference under bf16 autocast: 0.17); with fp32-grade forward products the worst gradient of the model reads 0.008.
        # fp32 operands for the input or the weight gradients instead change nothing (0.113).  FLOWTRON_ENCODER_F32=off: 16-bit.
        conv_mode = ("split3", m16, m16)
    return conv_mode, lstm_mode


# --------------------------------------------------------------------------
# Encoder -- flowtron.py:467-525
# --------------------------------------------------------------------------
class Encoder(nn.Module):
    def __init__(self, encoder_n_convolutions=3, encoder_embedding_dim=512, encoder_kernel_size=5,
                 norm_fn=MaskedInstanceNorm1d):
        super().__init__()
        convs = []
        for _ in range(encoder_n_convolutions):
            convs.append(nn.Sequential(
                ConvNorm(encoder_embedding_dim, encoder_embedding_dim, kernel_size=encoder_kernel_size, stride=1,
                         padding=int((encoder_kernel_size - 1) / 2), dilation=1, w_init_gain="relu"),
                norm_fn(encoder_embedding_dim, affine=True)))
        self.convolutions = nn.ModuleList(convs)
        self.lstm = nn.LSTM(encoder_embedding_dim, int(encoder_embedding_dim / 2), 1, batch_first=True,
                            bidirectional=True)
        self.dropout_masks = None     # test hook: list of 3 keep-masks [L,B,C] already scaled by 1/(1-p)

    def _run(self, x, lens):
        """x [L,B,C] time-major, lens int32 [B] -> [L,B,C]."""
        conv_mode, lstm_mode = encoder_operand_modes()
        drawn = None
        if self.dropout_masks is None and self.training:
            # F.dropout(p=0.5) keep-masks (flowtron.py:502) of ALL conv layers in one draw: two kernels per step instead of four per layer
            # (every layer keeps the [L,B,C] shape: the convolutions are C -> C)
            drawn = torch.empty((len(self.convolutions),) + tuple(x.shape), device=x.device, dtype=x.dtype).bernoulli_(0.5).mul_(2.0)
        for i, (conv, norm) in enumerate(self.convolutions):
            keep = None
            if self.dropout_masks is not None:
                keep = self.dropout_masks[i]
            elif drawn is not None:
                keep = drawn[i]
            x = ops.conv_norm_relu(x, lens, conv.conv.weight, conv.conv.bias, norm.weight, norm.bias, keep, norm.eps, mode=conv_mode)
        p = self.lstm
        # both directions in one launch chain when the fragment path applies (ops.bilstm_layer)
        return ops.bilstm_layer(x, lens, (p.weight_ih_l0, p.weight_hh_l0, p.bias_ih_l0, p.bias_hh_l0),
                                (p.weight_ih_l0_reverse, p.weight_hh_l0_reverse, p.bias_ih_l0_reverse, p.bias_hh_l0_reverse), mode=lstm_mode)

    def forward(self, x, in_lens):
        """x [B,C,L] (reference layout) -> [B,L,C]"""
        xt = x.permute(2, 0, 1).contiguous()
        return self._run(xt, ops.lens32(in_lens)).transpose(0, 1)

    def infer(self, x):
        xt = x.permute(2, 0, 1).contiguous()
        lens = torch.full((xt.shape[1],), xt.shape[0], dtype=torch.int32, device=xt.device)
        return self._run(xt, lens).transpose(0, 1)


# --------------------------------------------------------------------------
# Gaussian-mixture prior: MelEncoder + GaussianMixture -- flowtron.py:366-450, 312-363
# --------------------------------------------------------------------------
class MelEncoder(nn.Module):
    """flowtron.py:366-450: two stages of Conv1d(k 3) + masked instance norm + ReLU + dropout 0.5 (80 -> C', C' -> C'), a packed
    BiLSTM (C' -> 2 x C'/2) and the mean over the time axis of its zero-padded output (:437-439) -- whose divisor is therefore the
    batch's LONGEST length, not the utterance's own (ops.TimePoolFn takes it from the lengths on the device).  A batch of one runs
    the unmasked norm (:417), the same formula over all its frames.  The reference zero-fills the caller's mel behind the lengths in
    place (:420); here the input is only read -- the kernels never look behind a length.  The convolutions follow the text
    encoder's operand-mode choice (encoder_operand_modes)."""

    def __init__(self, encoder_embedding_dim=512, encoder_kernel_size=3, encoder_n_convolutions=2, norm_fn=MaskedInstanceNorm1d):
        super().__init__()
        convs = []
        for i in range(encoder_n_convolutions):
            convs.append(nn.Sequential(
                ConvNorm(80 if i == 0 else encoder_embedding_dim, encoder_embedding_dim, kernel_size=encoder_kernel_size, stride=1,
                         padding=int((encoder_kernel_size - 1) / 2), dilation=1, w_init_gain="relu"),
                norm_fn(encoder_embedding_dim, affine=True)))
        self.convolutions = nn.ModuleList(convs)
        self.lstm = nn.LSTM(encoder_embedding_dim, int(encoder_embedding_dim / 2), 1, bidirectional=True)
        self.dropout_masks = None     # test hook: list of keep-masks [T,B,C'] already scaled by 1/(1-p), one per convolution

    def _run(self, x, lens):
        """x [T,B,80] time-major, lens int32 [B] -> the BiLSTM's outputs [T,B,C']"""
        conv_mode, lstm_mode = encoder_operand_modes()
        drawn = None
        if self.dropout_masks is None and self.training:
            Cp = self.convolutions[0][0].conv.weight.shape[0]
            drawn = torch.empty((len(self.convolutions),) + tuple(x.shape[:2]) + (Cp,), device=x.device,
                                dtype=torch.float32).bernoulli_(0.5).mul_(2.0)
        for i, (conv, norm) in enumerate(self.convolutions):
            keep = None
            if self.dropout_masks is not None:
                keep = self.dropout_masks[i]
            elif drawn is not None:
                keep = drawn[i]
            x = ops.conv_norm_relu(x, lens, conv.conv.weight, conv.conv.bias, norm.weight, norm.bias, keep, norm.eps, mode=conv_mode)
        p = self.lstm
        return ops.bilstm_layer(x, lens, (p.weight_ih_l0, p.weight_hh_l0, p.bias_ih_l0, p.bias_hh_l0),
                                (p.weight_ih_l0_reverse, p.weight_hh_l0_reverse, p.bias_ih_l0_reverse, p.bias_hh_l0_reverse), mode=lstm_mode)

    def forward(self, x, lens):
        """x [B,80,T] (reference layout; not modified), lens [B] -> [B,C']"""
        L.require_cuda(x, lens)
        lens32 = ops.lens32(lens)
        h = self._run(x.permute(2, 0, 1).contiguous().float(), lens32)
        return ops.TimePoolFn.apply(h, lens32)

    def infer(self, x):
        """x [B,80,T], every frame valid -> the BiLSTM's outputs [B,T,C'] (flowtron.py:441-450, which nothing in the reference calls:
        it hands the batch-major tensor to a time-major LSTM; the evident intent -- one output row per frame -- is implemented)"""
        L.require_cuda(x)
        xt = x.permute(2, 0, 1).contiguous().float()
        lens = torch.full((xt.shape[1],), xt.shape[0], dtype=torch.int32, device=xt.device)
        return self._run(xt, lens).transpose(0, 1)


class GaussianMixture(nn.Module):
    """flowtron.py:312-363: prob = softmax(prob_layer(e)) [B,C]; mean / log_var either learned heads viewed as [B,M,C] or -- with
    fixed_gaussian -- buffers [1,M,C] that travel in the state_dict (mean: C distinct one-hot rows scaled by mean_scale, drawn with
    np.random.choice at construction; log_var zeros).  The three heads are B-row GEMMs with fp32 operands in every mode."""

    def __init__(self, n_hidden, n_components, n_mel_channels, fixed_gaussian, mean_scale):
        super().__init__()
        self.n_mel_channels = n_mel_channels
        self.n_components = n_components
        self.fixed_gaussian = fixed_gaussian
        self.mean_scale = mean_scale
        self.prob_layer = LinearNorm(n_hidden, n_components)
        if not fixed_gaussian:
            self.mean_layer = LinearNorm(n_hidden, n_mel_channels * n_components)
            self.log_var_layer = LinearNorm(n_hidden, n_mel_channels * n_components)
        else:
            self.register_buffer("mean", self.generate_mean(n_mel_channels, n_components, mean_scale).float())
            self.register_buffer("log_var", self.generate_log_var(n_mel_channels, n_components).float())

    def generate_mean(self, n_dimensions, n_components, scale=3):
        means = torch.eye(n_dimensions).float()
        ids = np.random.choice(range(n_dimensions), n_components, replace=False)
        means = means[ids] * scale
        return means.transpose(0, 1)[None]

    def generate_log_var(self, n_dimensions, n_components):
        return torch.zeros(1, n_dimensions, n_components).float()

    def generate_prob(self):
        return torch.ones(1, 1).float()

    def forward(self, outputs, bs):
        def head(layer):
            return ops.linear(outputs, layer.linear_layer.weight, layer.linear_layer.bias, mode=L.FT_F32)
        prob = ops.SoftmaxRowsFn.apply(head(self.prob_layer))
        if not self.fixed_gaussian:
            mean = head(self.mean_layer).view(bs, self.n_mel_channels, self.n_components)
            log_var = head(self.log_var_layer).view(bs, self.n_mel_channels, self.n_components)
        else:
            mean, log_var = self.mean, self.log_var
        return mean, log_var, prob


# --------------------------------------------------------------------------
# Attention -- flowtron.py:528-592
# --------------------------------------------------------------------------
class Attention(nn.Module):
    def __init__(self, n_mel_channels=80, n_speaker_dim=128, n_text_channels=512, n_att_channels=128, temperature=1.0):
        super().__init__()
        self.temperature = temperature
        self.query = LinearNorm(n_mel_channels, n_att_channels, bias=False, w_init_gain="tanh")
        self.key = LinearNorm(n_text_channels + n_speaker_dim, n_att_channels, bias=False, w_init_gain="tanh")
        self.value = LinearNorm(n_text_channels + n_speaker_dim, n_att_channels, bias=False, w_init_gain="tanh")
        self.v = LinearNorm(n_att_channels, 1, bias=False, w_init_gain="tanh")
        self.score_mask_value = -float("inf")

    def forward(self, queries, keys, values, in_lens32, attn_prior=None, rowmap=None):
        """queries [T,B,H], keys/values source [L,B,E] -> ctx [T,B,A], attn [B,T,L], attn_logprob [B,T,L]."""
        mode = L.mfma_mode()
        K = ops.linear(keys, self.key.linear_layer.weight, None, mode=mode)
        V = ops.linear(values, self.value.linear_layer.weight, None, mode=mode)
        # the score kernel walks every frame (the reference returns the attention of padded frames too): padded query rows are
        # filled with the utterance's first padded row (fill "y"); the query's input gradient only feeds guarded consumers
        Q = ops.linear(queries, self.query.linear_layer.weight, None, mode=mode, rowmap=rowmap, fill="y")
        attn, logprob = ops.AttentionScoresFn.apply(Q, K, self.v.linear_layer.weight, in_lens32, attn_prior,
                                                    self.temperature)
        ctx = ops.ContextFn.apply(attn, V, mode)
        return ctx, attn, logprob


# --------------------------------------------------------------------------
# AttentionConditioningLayer -- flowtron.py:129-152 (location-sensitive / cumulative attention features)
# --------------------------------------------------------------------------
class AttentionConditioningLayer(nn.Module):
    """Conv1d(2->32,k5)+ReLU+Conv1d(32->attention_dim,k3)+Sigmoid over [cumulative attention ; previous attention].
    Same registration as the reference (the nn.Sequential re-registers both convs, so the state_dict carries the
    `location_conv_*` AND `conv_layers.{0,2}` aliases).  Evaluated as im2col + GEMM with the activation fused in the
    GEMM epilogue, directly in the time-major [L,B,C] layout the key modulation needs."""

    def __init__(self, input_dim=2, attention_n_filters=32, attention_kernel_sizes=(5, 3), attention_dim=640):
        super().__init__()
        self.location_conv_hidden = ConvNorm(input_dim, attention_n_filters, kernel_size=attention_kernel_sizes[0],
                                             padding=None, bias=True, stride=1, dilation=1, w_init_gain="relu")
        self.location_conv_out = ConvNorm(attention_n_filters, attention_dim, kernel_size=attention_kernel_sizes[1],
                                          padding=None, bias=True, stride=1, dilation=1, w_init_gain="sigmoid")
        self.conv_layers = nn.Sequential(self.location_conv_hidden, nn.ReLU(), self.location_conv_out, nn.Sigmoid())

    def forward(self, attn_cat_lbc, full_lens):
        """attn_cat_lbc [L,B,2] time-major, full_lens int32 [B] (== L: Conv1d zero-pads only at the ends) -> [L,B,attention_dim]."""
        c1, c2 = self.location_conv_hidden.conv, self.location_conv_out.conv
        col = ops.Im2colFn.apply(attn_cat_lbc, full_lens, c1.weight.shape[2])
        h = ops.linear(col, c1.weight.reshape(c1.weight.shape[0], -1), c1.bias, act=L.ACT_RELU)
        col = ops.Im2colFn.apply(h, full_lens, c2.weight.shape[2])
        return ops.linear(col, c2.weight.reshape(c2.weight.shape[0], -1), c2.bias, act=L.ACT_SIGMOID)


# --------------------------------------------------------------------------
# AR_Step / AR_Back_Step -- flowtron.py:645-828, 595-642
# --------------------------------------------------------------------------
class AR_Step(nn.Module):
    def __init__(self, n_mel_channels, n_speaker_dim, n_text_channels, n_in_channels, n_hidden, n_attn_channels,
                 n_lstm_layers, add_gate, use_cumm_attention):
        super().__init__()
        if n_lstm_layers < 1:
            raise ValueError("n_lstm_layers must be >= 1")
        self.n_lstm_layers = int(n_lstm_layers)       # any depth: training = one recurrence + one batched projection per layer; decode:
        self.use_cumm_attention = use_cumm_attention  # depth 2 on the persistent launch, any other depth on the staged chain
        self.conv = nn.Conv1d(n_hidden, 2 * n_mel_channels, 1)
        self.conv.weight.data = 0.0 * self.conv.weight.data
        self.conv.bias.data = 0.0 * self.conv.bias.data
        self.lstm = nn.LSTM(n_hidden + n_attn_channels, n_hidden, n_lstm_layers)
        self.attention_lstm = nn.LSTM(n_mel_channels, n_hidden)
        self.attention_layer = Attention(n_hidden, n_speaker_dim, n_text_channels, n_attn_channels)
        if self.use_cumm_attention:
            self.attn_cond_layer = AttentionConditioningLayer(input_dim=2, attention_n_filters=32,
                                                              attention_kernel_sizes=[5, 3],
                                                              attention_dim=n_text_channels + n_speaker_dim)
        self.dense_layer = DenseLayer(in_dim=n_hidden, sizes=[n_hidden, n_hidden])
        if add_gate:
            self.gate_threshold = 0.5
            self.gate_layer = LinearNorm(n_hidden + n_attn_channels, 1, bias=True, w_init_gain="sigmoid")

    def __getstate__(self):
        """train.py pickles the whole module into its checkpoints (train.py:131-141): the decode scratch (flowtron_amd.decode:
        buffers per utterance shape, the 54 MB weight image, the hand-off granules -- every `_decode_*` attribute) is runtime
        state, not model state."""
        return {k: v for k, v in self.__dict__.items() if not k.startswith("_decode_")}

    def forward(self, mel, text, in_lens32, out_lens32, attn_prior=None, rowmap=None):
        """Teacher-forced flow. mel [T,B,M], text = encoder outputs [L,B,E].
        Returns (z [T,B,M], log_s [T,B,M], gates [T,B,1] | None, attn [B,T,L], attn_logprob [B,T,L]).
        rowmap (ops.RowMap over out_lens32): the batched GEMMs multiply valid frames only (pack-by-length, flowtron.py:689-694)."""
        T, B, M = mel.shape
        mode = L.mfma_mode()
        rm = rowmap
        mel0 = torch.cat([mel.new_zeros(1, B, M), mel[:-1]], 0)              # flowtron.py:726-729
        a = self.attention_lstm
        # fill "dx": d(mel0) flows into the PREVIOUS flow's z gradient, whose separator rows (first padded frame of an utterance)
        # the compact weight-gradient GEMMs of that flow do read -- padded rows must be zeros, not unwritten memory (T*B*80 floats)
        h_att = ops.lstm_layer(mel0, out_lens32, a.weight_ih_l0, a.weight_hh_l0, a.bias_ih_l0, a.bias_hh_l0, mode=mode, rowmap=rm,
                               fill="dx")
        if self.use_cumm_attention:
            ctx, attn, logprob = self.run_cumm_attn_sequence(h_att, text, in_lens32)   # drops the prior like flowtron.py:742-743
        else:
            ctx, attn, logprob = self.attention_layer(h_att, text, text, in_lens32, attn_prior, rowmap=rm)
        gates = None
        p = self.lstm
        # the gate layer reads [h_att ; ctx] like the decoder LSTM's input projection: where that projection runs over a
        # concatenated operand image, the N = 1 gate projection is taken from the same image (ops.LinearGateFn)
        g = self.gate_layer.linear_layer if hasattr(self, "gate_layer") else None
        H, two = p.weight_hh_l0.shape[1], self.n_lstm_layers == 2
        persist = ops.lstm_persistent(B, H, False, mode, mel.device) or ops.lstm_pad_width(B, H, False, mode, mel.device, T)   # (H < 1024: zero-padded twin)
        n_pair = ops.decoder_pair_chunks(B, H, mode, mel.device, T) if (two and persist and rm is not None) else 0
        path, fuse_gate = ops.decoder_plan(self.n_lstm_layers, g is not None, rm is not None, persist, n_pair,
                                           two and not persist and ops.lstm2_supported(B, H, mode))
        if g is not None and not fuse_gate:
            gates = ops.linear([h_att, ctx], g.weight, g.bias, mode=mode)     # Linear over [h_att ; ctx], no concat

        def first_layer():
            r = ops.lstm_layer(h_att, out_lens32, p.weight_ih_l0, p.weight_hh_l0, p.bias_ih_l0, p.bias_hh_l0, mode=mode,
                               xs_extra=[ctx], rowmap=rm, fill="dx", gate=(g.weight, g.bias) if fuse_gate else None)
            return r if fuse_gate else (r, gates)
        if path == "layers":
            # any other depth (the config schema splats n_lstm_layers into nn.LSTM, flowtron.py:655): the same per-layer pair --
            # batched input projection + one recurrence (persistent where its geometry applies) -- layer after layer
            h, gates = first_layer()
            for l in range(1, self.n_lstm_layers):
                h = ops.lstm_layer(h, out_lens32, getattr(p, "weight_ih_l%d" % l), getattr(p, "weight_hh_l%d" % l),
                                   getattr(p, "bias_ih_l%d" % l), getattr(p, "bias_hh_l%d" % l), mode=mode, rowmap=rm)
        elif path == "pair":
            # both layers CONCURRENTLY on four XCDs each, layer 1 one time chunk behind layer 0, the chunk's input projection between
            # the launches (ops.DecoderPairFn, csrc/lstm_roles.hip): the pair's chain of 2 T dependent steps becomes (1 + 1/n) T
            h, gates_f = ops.decoder_pair(h_att, out_lens32, p, mode, [ctx], rm, "dx", (g.weight, g.bias) if fuse_gate else None, n_pair)
            if fuse_gate:
                gates = gates_f
        elif path == "lstm2":
            # both decoder layers as one software-wavefront launch chain (csrc/lstm2.hip)
            gx0 = ops.LinearFn.apply(p.weight_ih_l0, p.bias_ih_l0 + p.bias_hh_l0, L.ACT_NONE, mode, None, "", h_att, ctx)
            h = ops.LSTM2SeqFn.apply(gx0, p.weight_hh_l0, p.weight_ih_l1, p.bias_ih_l1, p.bias_hh_l1, p.weight_hh_l1, out_lens32, mode)
        else:
            # "persistent": two persistent single-layer recurrences (csrc/lstm_persist.hip, ~2 us per step each) with layer 1's input
            # projection as one batched GEMM between them: faster than the two-layer wavefront launch chain (~8 us per step); "step": the
            # same on the launch-per-step kernels (the context gradient feeds the attention backward, which reduces over ALL frames: "dx")
            h, gates = first_layer()
            h = ops.lstm_layer(h, out_lens32, p.weight_ih_l1, p.weight_hh_l1, p.bias_ih_l1, p.bias_hh_l1, mode=mode, rowmap=rm)
        h = self.dense_layer(h, rowmap=rm)
        # the coupling output is returned for every frame (z, log_s of padded frames are the reference's defined junk): fill "y"
        out = ops.linear(h, self.conv.weight.reshape(self.conv.weight.shape[0], -1), self.conv.bias, mode=mode, rowmap=rm, fill="y")
        z = ops.AffineFn.apply(out, mel)                                      # z = exp(log_s) * mel + b
        log_s = out[..., :M]
        return z, log_s, gates, attn, logprob

    def run_cumm_attn_sequence(self, h_att, text, in_lens32):
        """flowtron.py:697-723: the location features of frame i depend on the attention of frames < i, so the frames are walked
        in order -- by the LIBRARY (ops.CummAttnSeqFn -> csrc/cumm_attn.hip: one C-ABI call per flow forward, one backward), not by
        Python: location convolutions as im2col + GEMM, key modulation, the per-frame key projection, a fused score / softmax /
        context / running-sum kernel.  FLOWTRON_CUMM_LOOP=python keeps the per-frame autograd walk (every operation a HIP kernel
        too; ~250 us of host time per frame) as the yardstick the tests compare the fused path with."""
        mode = L.mfma_mode()
        att = self.attention_layer
        V = ops.linear(text, att.value.linear_layer.weight, None, mode=mode)
        Q = ops.linear(h_att, att.query.linear_layer.weight, None, mode=mode)
        if os.environ.get("FLOWTRON_CUMM_LOOP", "fused") != "python":
            c = self.attn_cond_layer
            return ops.CummAttnSeqFn.apply(Q, V, text, att.key.linear_layer.weight, att.v.linear_layer.weight,
                                           c.location_conv_hidden.conv.weight, c.location_conv_hidden.conv.bias,
                                           c.location_conv_out.conv.weight, c.location_conv_out.conv.bias,
                                           in_lens32, float(att.temperature), mode)
        T, B, _ = h_att.shape
        Lk = text.shape[0]
        full = torch.full((B,), Lk, dtype=torch.int32, device=text.device)
        cumm = text.new_zeros(Lk, B)
        prev = text.new_zeros(Lk, B)
        ctxs, attns, lps = [], [], []
        for i in range(T):
            cond = self.attn_cond_layer(torch.stack([cumm, prev], 2), full)                 # [L,B,E]
            K = ops.linear(ops.MulFn.apply(text, cond), att.key.linear_layer.weight, None, mode=mode)
            a, lp = ops.AttentionScoresFn.apply(Q[i:i + 1], K, att.v.linear_layer.weight, in_lens32, None, att.temperature)
            ctxs.append(ops.ContextFn.apply(a, V, mode))
            attns.append(a)
            lps.append(lp)
            prev = a[:, 0, :].t()
            cumm = ops.AddFn.apply(cumm, prev)
        return torch.cat(ctxs, 0), torch.cat(attns, 1), torch.cat(lps, 1)

    def infer(self, residual, text, attns=None, attn_prior=None, use_graph=None):
        """Sequential inverse (flowtron.py:775-828). residual [N,B,M], text [L,B,E].
        Returns (mel [N',B,M], list of N' attention rows [B,1,L]).
        The decode kernels are batch-1 chains of GEMVs (inference.py decodes one utterance); B > 1 (round 5: the reference's loop takes
        any batch, flowtron.py:775-828) decodes the utterances one after the other through the same kernels -- AR decode does not
        shard, so a batch is B replicas.  With a gate layer every utterance stops at its OWN frame (the reference's
        `if sigmoid(gate) > thr` raises for B > 1); frames behind an utterance's stop are zero, N' = the longest."""
        return decode.infer(self, residual, text, attns, attn_prior, use_graph)

    def infer_batch(self, x, text, lens, in_lens=None, forced=None):
        """Sequential inverse of a batch whose utterances have their own lengths: x [T,B,M] (utterance b's frames 0 .. lens[b]-1;
        the frames behind are not read), text [L,B,E] (utterance b's positions 0 .. in_lens[b]-1, None = all L; the positions behind
        are not read).  Groups of up to ft_decode_batch_max() utterances decode in ONE persistent launch (csrc/decode_batch.hip
        dec_persist_batch_k; ft_decode_flow_batch_keys where a group's texts differ in length), a group of one on ft_decode_flow
        (with `forced`, below, on the batched launch as well); every utterance bit for bit as infer() decodes it alone.  Returns (out [T',B,M] zeros behind each utterance's end, attention
        rows [T',B,1,L] zeros behind its end and its text, frames per utterance).  The caller has checked the geometry
        (Flowtron._batch_decode_usable).
        forced [B,T,L] (utterance-major, as the launch reads it): GIVEN attention rows, in THIS flow's time order -- utterance b
        decodes along forced[b, :lens[b], :in_lens[b]], nothing behind is read.  Every group, a group of one included, then goes
        through ft_decode_flow_batch_forced (csrc/decode_forced.hip): no query projection, scores or softmax, only V is projected,
        and the returned attention rows are the given ones.  Bit for bit independent of the grouping; NOT bit-identical to
        infer(attns=), whose staged chain sums in another order."""
        return decode.infer_batch(self, x, text, lens, in_lens, forced)


class AR_Back_Step(nn.Module):
    def __init__(self, n_mel_channels, n_speaker_dim, n_text_dim, n_in_channels, n_hidden, n_attn_channels,
                 n_lstm_layers, add_gate, use_cumm_attention):
        super().__init__()
        self.ar_step = AR_Step(n_mel_channels, n_speaker_dim, n_text_dim, n_mel_channels + n_speaker_dim, n_hidden,
                               n_attn_channels, n_lstm_layers, add_gate, use_cumm_attention)
        self.ar_step._time_reversed = True

    def forward(self, mel, text, in_lens32, out_lens32, attn_prior=None, rowmap=None):
        # flip + per-sample roll (flowtron.py:606-613) == the reverse-by-length involution, one gather kernel, no host syncs
        mel = ops.reverse_by_length(mel, out_lens32, True)
        if attn_prior is not None:
            attn_prior = ops.reverse_by_length(attn_prior, out_lens32, False)
        z, log_s, gates, attn, logprob = self.ar_step(mel, text, in_lens32, out_lens32, attn_prior, rowmap=rowmap)
        z = ops.reverse_by_length(z, out_lens32, True)
        return z, log_s, gates, attn, logprob

    def infer(self, residual, text, attns=None, attn_prior=None):
        if attn_prior is not None:
            attn_prior = torch.flip(attn_prior, (1,))                     # flowtron.py:631-633 (batch 1: flip only)
        out, attn = self.ar_step.infer(torch.flip(residual, (0,)), text, attns, attn_prior=attn_prior)
        return torch.flip(out, (0,)), attn


def lengths_arg(v, name, B, hi):
    """in_lens / out_lens of Flowtron.infer -> a list of B Python ints in 1 ..= hi (None -> None).  A list or tuple of integers,
    or a one-dimensional integer tensor on the host or the device (read to the host once).  ValueError otherwise."""
    if v is None:
        return None
    if torch.is_tensor(v):
        if v.dtype.is_floating_point or v.dtype.is_complex or v.dtype == torch.bool:
            raise ValueError("%s must hold integers, got a %s tensor" % (name, v.dtype))
        if v.dim() != 1:
            raise ValueError("%s must be one-dimensional [B], got shape %s" % (name, tuple(v.shape)))
        vals = v.tolist()
    else:
        if not isinstance(v, (list, tuple)):
            raise ValueError("%s must be a list, tuple or tensor of integers, got %s" % (name, type(v).__name__))
        if any(isinstance(x, bool) or not isinstance(x, numbers.Integral) for x in v):
            raise ValueError("%s must hold integers, got %r" % (name, list(v)))
        vals = [int(x) for x in v]
    if len(vals) != B:
        raise ValueError("%s has %d entries for a batch of %d" % (name, len(vals), B))
    if any(not 1 <= x <= hi for x in vals):
        raise ValueError("%s must lie in 1 ..= %d, got %r" % (name, hi, vals))
    return vals


def aligned_rows(alignment, flow, n_frames, n_text):
    """The rows flow `flow` decodes along, for a whole batch and in that flow's own time order: alignment [B, N, L] (every flow)
    or [F, B, N, L] (one per flow) in natural time, n_frames: list of B -> float32 [B, max(n_frames), n_text] with
    rows[b, :n_frames[b]] = alignment[.., b, :n_frames[b], :n_text], for an odd (reversed) flow flipped over the utterance's own
    n_frames[b] -- what infer_aligned's utterance loop hands infer(attns=).  Rows behind n_frames[b] are not meant to be read.
    One gather on the tensor's device, no host loop; plain torch, so it runs on CPU tensors as well."""
    a = alignment[flow] if alignment.dim() == 4 else alignment
    n = max(n_frames)
    a = a[:, :n, :n_text]
    if flow % 2 == 1:
        nf = torch.tensor(n_frames, device=a.device)[:, None]
        t = torch.arange(n, device=a.device)[None, :]
        a = torch.gather(a, 1, torch.where(t < nf, nf - 1 - t, t)[:, :, None].expand(-1, -1, a.shape[2]))
    return a.float().contiguous()


# --------------------------------------------------------------------------
# Flowtron -- flowtron.py:831-961
# --------------------------------------------------------------------------
class Flowtron(nn.Module):
    def __init__(self, n_speakers, n_speaker_dim, n_text, n_text_dim, n_flows, n_mel_channels, n_hidden,
                 n_attn_channels, n_lstm_layers, use_gate_layer, mel_encoder_n_hidden, n_components,
                 fixed_gaussian, mean_scale, dummy_speaker_embedding, use_cumm_attention):
        super().__init__()
        norm_fn = MaskedInstanceNorm1d
        self.speaker_embedding = nn.Embedding(n_speakers, n_speaker_dim)
        self.embedding = nn.Embedding(n_text, n_text_dim)
        self.flows = nn.ModuleList()
        self.encoder = Encoder(norm_fn=norm_fn, encoder_embedding_dim=n_text_dim)
        self.dummy_speaker_embedding = dummy_speaker_embedding
        if n_components > 1:                    # flowtron.py:846-851, registered behind the encoder as there
            self.mel_encoder = MelEncoder(mel_encoder_n_hidden, norm_fn=norm_fn)
            self.gaussian_mixture = GaussianMixture(mel_encoder_n_hidden, n_components, n_mel_channels, fixed_gaussian, mean_scale)
        for i in range(n_flows):
            add_gate = bool(i == (n_flows - 1) and use_gate_layer)
            cls = AR_Step if i % 2 == 0 else AR_Back_Step
            self.flows.append(cls(n_mel_channels, n_speaker_dim, n_text_dim, n_mel_channels + n_speaker_dim,
                                  n_hidden, n_attn_channels, n_lstm_layers, add_gate, use_cumm_attention))

    def _encode(self, speaker_ids, text, in_lens):
        """embeddings + encoder + speaker concat -> [L,B,E] (flowtron.py:872-887)."""
        L.require_cuda(speaker_ids, text, self.embedding.weight)
        if self.dummy_speaker_embedding:
            speaker_ids = speaker_ids * 0
        B, Lt = text.shape
        # speaker row broadcast over L by the gather kernel itself (ids repeated), so its backward is the
        # same atomic scatter-add kernel (flowtron.py:886-887 expand + cat)
        spk_ids = speaker_ids.reshape(1, -1).expand(Lt, -1).reshape(-1)
        spk = ops.embedding(spk_ids, self.speaker_embedding.weight, run_stride=B).reshape(Lt, B, -1)   # [L,B,S]; backward: one atomic per 32 positions
        emb = ops.embedding(text.t().contiguous(), self.embedding.weight).reshape(Lt, B, -1)   # time-major [L,B,C]
        if in_lens is None:
            lens = torch.full((B,), Lt, dtype=torch.int32, device=text.device)
        else:
            lens = ops.lens32(in_lens)
        enc = self.encoder._run(emb, lens)
        return torch.cat([enc, spk], 2), lens

    def forward(self, mel, speaker_ids, text, in_lens, out_lens, attn_prior=None, _mixture=True):
        """mel [B,M,T], speaker_ids [B], text [B,L] (sorted by in_lens desc), in_lens/out_lens [B],
        attn_prior [B,T,L] | None -> the reference's 8-tuple (flowtron.py:898-899).  _mixture=False (latents, alignments: callers
        that do not return the mixture) skips the mel encoder of a model built with n_components > 1; elements 5-7 are then None."""
        L.require_cuda(mel, text, in_lens, out_lens, attn_prior)
        ops.weight_images_begin(self)                # (the weights this model's previous forward rounded: one launch at the first request)
        ops.bias_sums_begin(self._lstm_bias_pairs())  # (b_ih + b_hh of every LSTM: one multi-tensor add)
        try:
            return self._forward(mel, speaker_ids, text, in_lens, out_lens, attn_prior, _mixture)
        finally:
            ops.bias_sums_end()
            ops.weight_images_end(self)

    def _lstm_bias_pairs(self):
        """[(b_ih, b_hh)] groups, one per flow / for the encoder: a group is one autograd node, and its parameters' gradients become
        ready together -- per flow, so that the per-flow gradient buckets of the DP overlap regime still complete in backward order"""
        groups = {}
        for mname, m in self.named_modules():
            if isinstance(m, torch.nn.LSTM):
                key = ".".join(mname.split(".")[:2]) if mname.startswith("flows.") else mname.split(".")[0]
                for name, p in m.named_parameters(recurse=False):
                    if name.startswith("bias_ih"):
                        groups.setdefault(key, []).append((p, getattr(m, "bias_hh" + name[len("bias_ih"):])))
        return list(groups.values())

    def _forward(self, mel, speaker_ids, text, in_lens, out_lens, attn_prior=None, mixture=True):
        enc, in32 = self._encode(speaker_ids, text, in_lens)
        out32 = ops.lens32(out_lens)
        x = mel.permute(2, 0, 1).contiguous().float()
        if attn_prior is not None:
            attn_prior = attn_prior.float()
        # pack-by-length for the batched GEMMs of the 16-bit operand modes (one row map per forward, built on the device)
        rm = ops.row_map(out32, x.shape[0], x.shape[1]) if L.is16(L.mfma_mode()) else None

        def run_flows(x, enc):
            log_s_list, attns_list, attns_logprob_list = [], [], []
            gate = None
            for flow in self.flows:
                x, log_s, gate, attn, logprob = flow(x, enc, in32, out32, attn_prior, rowmap=rm)
                log_s_list.append(log_s)
                attns_list.append(attn)
                attns_logprob_list.append(logprob)
            return x, log_s_list, gate, attns_list, attns_logprob_list

        mean = log_var = prob = None
        if mixture and hasattr(self, "gaussian_mixture"):        # flowtron.py:877-881
            mel_embedding = self.mel_encoder(mel, out32)
            mean, log_var, prob = self.gaussian_mixture(mel_embedding, mel_embedding.size(0))
        x0 = x
        x, log_s_list, gate, attns_list, attns_logprob_list = run_flows(x0, enc)
        if not torch.is_grad_enabled() and ops.PERSIST_LAUNCHES:
            # forward-only pass (validation, train.py:143-202): no optimizer step will look at the persistent kernels' status word,
            # so a launch that timed out would hand back garbage silently.  One host read (the validation loop reads its losses
            # with .item() anyway); on a failure -- this pass's, or a stale word of an earlier, already dropped training step --
            # the device has been switched to the launch-per-step kernels (warned once) and the flows run AGAIN on those, like
            # AR_Step.infer does: a validation pass must not kill a run that a training step would survive, and under DP the other
            # ranks must not be left waiting at their next collective
            if not ops.check_persist_status(raise_on_failure=False):
                enc, in32 = self._encode(speaker_ids, text, in_lens)          # (the encoder's persistent BiLSTM may be the one that failed)
                x, log_s_list, gate, attns_list, attns_logprob_list = run_flows(x0, enc)
        return x, log_s_list, gate, attns_list, attns_logprob_list, mean, log_var, prob

    def latents(self, mel, speaker_ids, text, in_lens, out_lens, attn_prior=None):
        """z of a batch of utterances for style transfer (inference_style_transfer.ipynb runs `model(...)[0]` utterance by utterance):
        one no-grad batched forward -> z [B, M, T], zeros behind out_lens[b].  mel [B,M,T], speaker_ids [B], text [B,L], attn_prior
        [B,T,L] | None; in_lens / out_lens as for infer (lists, CPU or device integer tensors, 1 ..= L and 1 ..= T).  The utterances
        may come in any order: the forward sees them sorted by text length, descending, as the reference's collate function hands
        them over, and z comes back in the caller's order.  eval() mode only: the encoder's dropout would make z random."""
        out, unsort, _, ol = self._forward_any_order("latents", mel, speaker_ids, text, in_lens, out_lens, attn_prior)
        with torch.no_grad():
            dev, T = mel.device, mel.shape[2]
            z = unsort(out[0].permute(1, 2, 0))                                                                # [T,B,M] -> [B,M,T]
            pad = torch.arange(T, device=dev)[None, :] >= torch.tensor(ol, device=dev)[:, None]               # [B,T]
            return z.masked_fill(pad[:, None, :], 0.0)

    def _forward_any_order(self, what, mel, speaker_ids, text, in_lens, out_lens, attn_prior):
        """The no-grad batched forward behind latents() and alignments(): the utterances in any order, the forward sees them
        sorted by text length, descending.  -> (the forward's tuple in SORTED order, unsort: a function that puts a tensor
        whose first dimension is the batch back into the caller's order, in_lens and out_lens as lists in the caller's order)."""
        if self.training:
            raise ValueError("%s needs model.eval(): in training mode the encoder's dropout makes z random" % what)
        L.require_cuda(mel, speaker_ids, text, attn_prior)
        if mel.dim() != 3 or text.dim() != 2 or text.shape[0] != mel.shape[0]:
            raise ValueError("mel must be [B, M, T] and text [B, L] with the same B, got %s and %s"
                             % (tuple(mel.shape), tuple(text.shape)))
        B, T = mel.shape[0], mel.shape[2]
        il = lengths_arg(in_lens, "in_lens", B, text.shape[1])
        ol = lengths_arg(out_lens, "out_lens", B, T)
        if il is None or ol is None:
            raise ValueError("in_lens and out_lens must be given")
        dev = mel.device
        order = sorted(range(B), key=lambda b: -il[b])            # stable: equal lengths keep the caller's order
        if order != list(range(B)):
            idx = torch.tensor(order, dtype=torch.long, device=dev)
            mel, speaker_ids, text = mel.index_select(0, idx), speaker_ids.index_select(0, idx), text.index_select(0, idx)
            if attn_prior is not None:
                attn_prior = attn_prior.index_select(0, idx)
        with torch.no_grad():
            out = self(mel, speaker_ids, text, torch.tensor([il[b] for b in order], dtype=torch.long, device=dev),
                       torch.tensor([ol[b] for b in order], dtype=torch.long, device=dev), attn_prior, _mixture=False)
            inv_idx = None
            if order != list(range(B)):
                inv = [0] * B
                for pos, b in enumerate(order):
                    inv[b] = pos
                inv_idx = torch.tensor(inv, dtype=torch.long, device=dev)
        return out, (lambda t: t if inv_idx is None else t.index_select(0, inv_idx)), il, ol

    def alignments(self, mel, speaker_ids, text, in_lens, out_lens, attn_prior=None):
        """The attention of every flow over a batch of utterances, ready for flowtron_amd.align: the same no-grad batched forward
        as latents() -> (z [B, M, T], attn [F, B, T, L], attn_logprob [F, B, T, L]).  Arguments as for latents(): any order of
        the utterances, results in the caller's order, eval() mode only.  EVERY flow is in natural time: the maps of the odd
        flows, which the forward hands back in reversed time, are reversed by length on the device (ops.reverse_by_length).
        Zeros lie behind out_lens[b] and behind in_lens[b]."""
        out, unsort, il, ol = self._forward_any_order("alignments", mel, speaker_ids, text, in_lens, out_lens, attn_prior)
        with torch.no_grad():
            dev, T, Lt = mel.device, mel.shape[2], text.shape[1]
            ol_t, il_t = torch.tensor(ol, device=dev), torch.tensor(il, device=dev)
            pad_t = torch.arange(T, device=dev)[None, :] >= ol_t[:, None]                                      # [B,T]
            pad = pad_t[:, :, None] | (torch.arange(Lt, device=dev)[None, :] >= il_t[:, None])[:, None, :]     # [B,T,L]
            out32 = ol_t.to(torch.int32)
            maps = []
            for per_flow in (out[3], out[4]):
                flows = []
                for f, a in enumerate(per_flow):
                    a = unsort(a.detach())
                    if f % 2 == 1:
                        a = ops.reverse_by_length(a, out32, False)
                    flows.append(a.masked_fill(pad, 0.0))
                maps.append(torch.stack(flows))
            z = unsort(out[0].permute(1, 2, 0)).masked_fill(pad_t[:, None, :], 0.0)
            return z, maps[0], maps[1]

    def log_likelihood(self, mel, speaker_ids, text, in_lens, out_lens, attn_prior=None, sigma=1.0):
        """The exact log-density of every mel frame given text and speaker (the flow's change of variables, per utterance where
        FlowtronLoss gives the batch mean): the same no-grad batched forward as latents() and alignments(), then one reduction on
        the device (flowtron_amd.score, csrc/score.hip).  Arguments as for latents(): any order of the utterances, results in the
        caller's order, eval() mode only.  -> a named tuple
          frame_ll [B, T] float64: ln p(frame t of utterance b) in nats, in natural time -- the log_s of an AR_Back_Step, which the
              forward hands back in that flow's reversed time, is read mirrored over the utterance's own length; 0 behind out_lens[b]
          total [B] float64: the utterance's log-likelihood, the sum of its frames
          nll_per_dim [B] float64: (sum z^2 / (2 sigma^2) - sum log_s) / (out_lens[b] M), FlowtronLoss's NLL restricted to the
              utterance (no Gaussian constant): the frame-weighted mean over a batch is loss_nll.
        NotImplementedError for a model built with n_components > 1: the mixture prior has its own likelihood."""
        from . import score
        return score.log_likelihood(self, mel, speaker_ids, text, in_lens, out_lens, attn_prior, sigma)

    def infer_aligned(self, residual, speaker_ids, text, alignment, in_lens=None, n_frames=None, temperature=1.0,
                      gate_threshold=1.0, persistent=False):
        """Decodes a batch along GIVEN alignments (durations from flowtron_amd.align, or the soft maps of alignments()):
        residual [B, M, N], text [B, L], alignment [B, N, L] (used by every flow) or [F, B, N, L] (one per flow), hard or soft,
        ALWAYS in natural time -- the rows of an odd flow are flipped here, over the utterance's own frames.  in_lens [B]: text
        positions per utterance (None = L); n_frames [B]: frames per utterance (None = N); lists or integer tensors.
        Utterance b is decoded exactly as infer(residual[b:b+1, :, :n_b], speaker_ids[b:b+1], text[b:b+1, :L_b], attns=[its rows
        per flow, in the flow's own time order], gate_threshold=...) decodes it: a loop over the staged forced-decode chain.
        gate_threshold 1.0 (the default) lets the alignment decide the length; a lower one lets the gate cut it.
        -> (mel [B, M, N'] with zeros behind each utterance's frames, lengths: CPU int64 [B]).
        persistent=True: the batch decodes flow by flow in groups of up to ft_decode_batch_max() utterances per persistent launch
        (AR_Step.infer_batch(forced=), csrc/decode_forced.hip) where _batch_decode_usable holds -- the geometry of the batched
        launch on a device whose persistent kernels work; FLOWTRON_DECODE_PERSIST=0 or FLOWTRON_DECODE_BATCH=0 switch it off --
        and takes the loop above otherwise, silently, as infer treats a batch.  Every flow gets the same rows as in the loop
        (aligned_rows: an odd flow's flipped over the GIVEN n_frames[b], of which the frames a gate left are the first).
        Guaranteed then: each utterance is bit for bit what it is when decoded alone with persistent=True, whatever the batch
        and the grouping; each flow is within 10 x the fp32 reference implementation's own deviation from a float64 decode of
        the same inputs (tests/test_gpu_decode_aligned.py), as the staged result is.  It is NOT bit-identical to
        persistent=False: the persistent kernels sum in another order than the staged chain."""
        L.require_cuda(residual, text, alignment)
        if residual.dim() != 3 or text.dim() != 2 or text.shape[0] != residual.shape[0]:
            raise ValueError("residual must be [B, M, N] and text [B, L] with the same B, got %s and %s"
                             % (tuple(residual.shape), tuple(text.shape)))
        B, N, Lt, F_ = residual.shape[0], residual.shape[2], text.shape[1], len(self.flows)
        if not torch.is_tensor(alignment) or tuple(alignment.shape) not in ((B, N, Lt), (F_, B, N, Lt)):
            raise ValueError("alignment must be [B, N, L] = %s or [F, B, N, L] = %s, got %s"
                             % ((B, N, Lt), (F_, B, N, Lt), tuple(alignment.shape) if torch.is_tensor(alignment) else type(alignment).__name__))
        il = lengths_arg(in_lens, "in_lens", B, Lt) or [Lt] * B
        nf = lengths_arg(n_frames, "n_frames", B, N) or [N] * B
        sid = speaker_ids.reshape(B, -1)
        if persistent and self._batch_decode_usable(residual, max(il)):
            mel, _, n = self._infer_batched(residual, sid, text, temperature, gate_threshold, il, nf, alignment)
            return mel, torch.tensor(n, dtype=torch.int64)
        outs = []
        for b in range(B):
            rows = []
            for f in range(F_):
                a = (alignment[f, b] if alignment.dim() == 4 else alignment[b])[:nf[b], :il[b]].float()
                rows.append(torch.flip(a, (0,)) if f % 2 == 1 else a)
            m, _ = self.infer(residual[b:b + 1, :, :nf[b]], sid[b:b + 1], text[b:b + 1, :il[b]], temperature=temperature,
                              gate_threshold=gate_threshold, attns=rows)
            outs.append(m)
        mel, n = decode.pad_mels(outs)
        return mel, torch.tensor(n, dtype=torch.int64)

    def infer(self, residual, speaker_ids, text, temperature=1.0, gate_threshold=0.5, attns=None, attn_prior=None,
              in_lens=None, out_lens=None, return_lengths=False):
        """residual [B,M,N], speaker_ids [B] or [B,1], text [B,L] -> (mel [B,M,N'], attention_weights: per flow a list of N' rows
        [B,1,L]).  The decode kernels are batch-1 chains (inference.py decodes one utterance).  A batch (the reference's loop takes any,
        flowtron.py:775-828, 901-930) is decoded utterance by utterance through ALL flows and padded only at the very end: with a gate
        layer every utterance stops at its OWN frame of the last flow (decoded first), and the flows behind it must see exactly that
        utterance's frames -- padding the batch after each flow would put the shorter utterances' pad frames IN FRONT of their real
        ones once the next (reversed) flow flips the tensor.  Frames behind an utterance's stop are zero; N' = the longest.

        Sentences of different lengths (this project's extension; the reference's infer is batch-1): in_lens [B] text positions and
        out_lens [B] residual frames per utterance (lists, CPU or device integer tensors; 1 ..= L and 1 ..= N; None = all of them).
        Utterance b is decoded exactly as infer(residual[b:b+1, :, :out_lens[b]], speaker_ids[b:b+1], text[b:b+1, :in_lens[b]]):
        token ids and residual frames behind its lengths are never read, and its attention columns >= in_lens[b] are zero.
        attn_prior [B,N,L] is cut the same way.  return_lengths=True appends a CPU int64 [B]: the frames each utterance produced
        (out_lens[b], fewer where the gate stopped it)."""
        L.require_cuda(residual, text)
        B = residual.shape[0]
        if residual.dim() != 3 or text.dim() != 2 or text.shape[0] != B:
            raise ValueError("residual must be [B, M, N] and text [B, L] with the same B, got %s and %s"
                             % (tuple(residual.shape), tuple(text.shape)))
        Lt, N = text.shape[1], residual.shape[2]
        il = lengths_arg(in_lens, "in_lens", B, Lt) or [Lt] * B
        ol = lengths_arg(out_lens, "out_lens", B, N) or [N] * B
        if B > 1 and attns is not None:
            raise ValueError("forced alignments (attns=) are taken one utterance at a time")
        if B == 1:
            if attns is not None and (il[0] < Lt or ol[0] < N):   # one forced alignment per flow: N rows of L
                attns = [(torch.stack([r.reshape(-1) for r in a]) if isinstance(a, (list, tuple)) else a.reshape(-1, Lt))[:ol[0], :il[0]]
                         for a in attns]
            mel, aws = self._infer_one(residual[:, :, :ol[0]], speaker_ids, text[:, :il[0]], temperature, gate_threshold, attns,
                                       None if attn_prior is None else attn_prior[:, :ol[0], :il[0]])
            if il[0] < Lt:                                       # the rows at the width of the given text, zeros behind in_lens
                aws = [[torch.nn.functional.pad(r, (0, Lt - il[0])) for r in rows] for rows in aws]
            n = [int(mel.shape[2])]
        else:
            sid = speaker_ids.reshape(B, -1)
            if attn_prior is None and self._batch_decode_usable(residual, max(il)):
                mel, aws, n = self._infer_batched(residual, sid, text, temperature, gate_threshold, il, ol)
            else:
                outs = [self._infer_one(residual[b:b + 1, :, :ol[b]], sid[b], text[b:b + 1, :il[b]], temperature, gate_threshold,
                                        None, None if attn_prior is None else attn_prior[b:b + 1, :ol[b], :il[b]]) for b in range(B)]
                mel, n = decode.pad_mels([m for m, _ in outs])
                aws = [decode.pad_attn_rows([aw[f] for _, aw in outs], max(n), Lt, mel) for f in range(len(self.flows))]
        if return_lengths:
            return mel, aws, torch.tensor(n, dtype=torch.int64)
        return mel, aws

    def _infer_one(self, residual, speaker_ids, text, temperature, gate_threshold, attns, attn_prior):
        """infer() of one utterance: residual [1,M,N], text [1,L], every position and frame its own"""
        with torch.no_grad():
            enc, _ = self._encode(speaker_ids, text, None)
            x = residual.permute(2, 0, 1).contiguous().float()
            attention_weights = []
            for i, flow in enumerate(reversed(self.flows)):
                self.set_temperature_and_gate(flow, temperature, gate_threshold)
                # attns: one forced alignment per flow, in flows order (the reference indexes `reversed(attns)[i]`, which
                # raises TypeError -- flowtron.py:925; the evident intent is implemented)
                x, aw = flow.infer(x, enc, None if attns is None else attns[len(self.flows) - 1 - i], attn_prior=attn_prior)
                attention_weights.append(aw)
            return x.permute(1, 2, 0), attention_weights

    def _batch_decode_usable(self, residual, n_text):
        """True when a batch decodes through the batched persistent launch (AR_Step.infer_batch): its geometry (H 1024, A 640,
        M 80, longest text n_text <= 1024, two decoder layers, plain attention) on a device whose persistent kernels work, in either
        weight precision.  FLOWTRON_DECODE_BATCH=0 keeps the utterance-by-utterance loop (the yardstick of the tests); so does
        FLOWTRON_DECODE_PERSIST=0."""
        if os.environ.get("FLOWTRON_DECODE_BATCH", "1") == "0" or os.environ.get("FLOWTRON_DECODE_PERSIST", "1") == "0":
            return False
        st = self.flows[0].ar_step if hasattr(self.flows[0], "ar_step") else self.flows[0]
        H = st.lstm.weight_hh_l0.shape[1]
        A = st.attention_layer.key.linear_layer.weight.shape[0]
        return (st.n_lstm_layers == 2 and not st.use_cumm_attention and H == 1024 and A == 640 and residual.shape[1] == 80
                and residual.shape[2] >= 1 and 1 <= n_text <= 1024 and ops.persist_usable(residual.device))

    def _infer_batched(self, residual, sid, text, temperature, gate_threshold, in_lens, out_lens, alignment=None):
        """infer() of a batch, flow by flow, each flow in groups of up to ft_decode_batch_max() utterances per persistent launch.
        Every utterance keeps its own text (in_lens: its own encoder call, keys and values) and its own length between flows
        (out_lens, then its own gate stop; the reversed flows flip its own frames), so each comes out exactly as decoded alone.
        Returns infer()'s batch format and the frames of each utterance.
        alignment (infer_aligned's, natural time): every flow decodes along its rows (aligned_rows over out_lens); the attention
        rows, which are the given ones, are then not returned (None)."""
        B, Lt = residual.shape[0], text.shape[1]
        Lk = max(in_lens)                                        # the text, padded to its longest utterance only
        with torch.no_grad():
            # the encoder, utterance by utterance as the loop runs it, each over its own positions; zeros behind them
            enc = None
            for b in range(B):
                e = self._encode(sid[b], text[b:b + 1, :in_lens[b]], None)[0]
                if enc is None:
                    enc = e.new_zeros(Lk, B, e.shape[2])
                enc[:in_lens[b], b] = e[:, 0]
            x = residual[:, :, :max(out_lens)].permute(2, 0, 1).contiguous().float()    # (frames past out_lens[b] are never read)
            lens = list(out_lens)
            atts = []
            for f in reversed(range(len(self.flows))):
                flow = self.flows[f]
                self.set_temperature_and_gate(flow, temperature, gate_threshold)
                back = hasattr(flow, "ar_step")
                st = flow.ar_step if back else flow
                if back:                                         # flowtron.py:631-633 per utterance: flip its own frames
                    x = ops.reverse_by_length(x, torch.tensor(lens, dtype=torch.int32, device=x.device), True)
                x, aw, lens = st.infer_batch(x, enc, lens, in_lens,
                                             None if alignment is None else aligned_rows(alignment, f, out_lens, Lk))
                if back:
                    x = ops.reverse_by_length(x, torch.tensor(lens, dtype=torch.int32, device=x.device), True)
                atts.append(aw)
            n = max(lens)
            mel = residual.new_zeros(B, x.shape[2], n, dtype=torch.float32)
            mel.copy_(x[:n].permute(1, 2, 0))
            if alignment is not None:
                return mel, None, lens
            rows = []
            for aw in atts:
                a_ = residual.new_zeros(n, B, 1, Lt, dtype=torch.float32)
                k = min(n, aw.shape[0])
                a_[:k, :, :, :Lk] = aw[:k]
                rows.append([a_[t] for t in range(n)])
            return mel, rows, lens

    @staticmethod
    def set_temperature_and_gate(flow, temperature, gate_threshold):
        flow = flow.ar_step if hasattr(flow, "ar_step") else flow
        flow.attention_layer.temperature = temperature
        if hasattr(flow, "gate_layer"):
            flow.gate_threshold = gate_threshold


# --------------------------------------------------------------------------
# Loss -- flowtron.py:155-275
# --------------------------------------------------------------------------
class AttentionCTCLoss(nn.Module):
    """flowtron.py:155-182: the reference loops over samples (slice, log_softmax, CTCLoss with target 1..K,
    reduction='mean' per sample, F*B host synchronisations per step).  Here ONE pair of HIP kernels handles the whole
    batch (ft_attn_ctc_fwd/bwd: log-softmax normaliser + banded alpha/beta recursion, one workgroup per sample).
    Device tensors only -- the torch restatement used to pin the batching lives in tests/test_host_cpu.py."""

    def __init__(self, blank_logprob=-1):
        super().__init__()
        self.blank_logprob = blank_logprob

    def forward(self, attn_logprob, in_lens, out_lens):
        """attn_logprob [B,T,L] in natural time order."""
        L.require_cuda(attn_logprob, in_lens, out_lens)
        return ops.AttnCTCFn.apply(attn_logprob, ops.lens32(in_lens), ops.lens32(out_lens), self.blank_logprob)


class FlowtronLoss(nn.Module):
    def __init__(self, sigma=1.0, gm_loss=False, gate_loss=True, use_ctc_loss=False, ctc_loss_weight=0.0,
                 blank_logprob=-1):
        super().__init__()
        self.sigma = sigma
        self.gm_loss = gm_loss
        self.gate_loss = gate_loss
        self.use_ctc_loss = use_ctc_loss
        self.ctc_loss_weight = ctc_loss_weight
        self.blank_logprob = blank_logprob
        self.attention_loss = AttentionCTCLoss(blank_logprob=self.blank_logprob)

    def forward(self, model_output, gate_target, in_lengths, out_lengths, is_validation=False):
        z, log_s_list, gate_pred, attn_list, attn_logprob_list = model_output[:5]
        out32 = ops.lens32(out_lengths)
        use_gate = self.gate_loss > 0
        lps = list(attn_logprob_list) if self.use_ctc_loss else []
        if self.gm_loss:
            # flowtron.py:217-231: the mixture likelihood as one node (ops.MixtureNLLFn); gate and CTC on the per-term path below
            mean, log_var, prob = model_output[5:8]
            if mean is None or log_var is None or prob is None:
                raise ValueError("gm_loss=True needs the mixture in the model's output (elements 5-7 of its tuple), which a model "
                                 "built with n_components <= 1 does not produce: set n_components > 1, or gm_loss=False")
            loss = ops.MixtureNLLFn.apply(z, mean, log_var, prob, out32, *log_s_list)
            return (loss,) + self._gate_and_ctc(z, gate_pred, gate_target, attn_logprob_list, in_lengths, out_lengths, out32)
        if ops.FUSED_LOSS and len(log_s_list) <= 8 and len(lps) <= 8 and all(lp is not None for lp in lps):
            # one autograd node, ten launches forward + backward (ops.FlowtronLossFn); the per-term path below is its restatement
            loss, gate_loss, loss_ctc = ops.FlowtronLossFn.apply(z, gate_pred if use_gate else None, gate_target if use_gate else None,
                                                                 out32, ops.lens32(in_lengths), float(self.sigma),
                                                                 float(self.blank_logprob), len(log_s_list), *log_s_list, *lps)
            if not self.use_ctc_loss:
                loss_ctc = torch.zeros_like(gate_loss)
            return loss, gate_loss, loss_ctc
        loss = ops.NLLFn.apply(z, out32, float(self.sigma), *log_s_list)
        return (loss,) + self._gate_and_ctc(z, gate_pred, gate_target, attn_logprob_list, in_lengths, out_lengths, out32)

    def _gate_and_ctc(self, z, gate_pred, gate_target, attn_logprob_list, in_lengths, out_lengths, out32):
        """(gate_loss, loss_ctc) term by term (flowtron.py:237-274)"""
        gate_loss = torch.zeros(1, device=z.device)
        if self.gate_loss > 0:
            gate_loss = ops.GateBCEFn.apply(gate_pred, gate_target, out32)
        loss_ctc = torch.zeros_like(gate_loss)
        if self.use_ctc_loss:
            lps = []
            for i, lp in enumerate(attn_logprob_list):
                if i % 2 != 0:
                    lp = ops.reverse_by_length(lp, out32, False)       # back-step flows are in reversed time (:250-256)
                lps.append(lp)
            # the DP is one workgroup per sample and latency-bound in T: F flows stacked along the batch cost the time
            # of one (F*B of 256 CUs busy).  mean over the F*B stacked samples == mean over flows of the per-flow batch means.
            F_ = len(lps)
            loss_ctc = self.attention_loss(torch.cat(lps, 0) if F_ > 1 else lps[0], in_lengths.repeat(F_), out_lengths.repeat(F_))
        return gate_loss, loss_ctc
