// Parameter block of the decode kernels and the bf16 chunk product (csrc/decode.hip, csrc/decode_batch.hip).
// Included inside the anonymous namespace of decode.hip, decode_batch.hip and decode_forced.hip.
#pragma once

typedef unsigned short bf16_t;

struct DecodeDev {
    const float *att_w_ih, *att_w_hh, *att_b_ih, *att_b_hh;
    const float *w_query, *v, *K, *V;
    const float *l0_w_ih, *l0_w_hh, *l0_b_ih, *l0_b_hh, *l1_w_ih, *l1_w_hh, *l1_b_ih, *l1_b_hh;
    const float *d0_w, *d0_b, *d1_w, *d1_b, *conv_w, *conv_b, *gate_w, *gate_b;
    const float* residual; float* mel_out; float* attn_out; int* n_done_dev;
    float *h_att, *c_att, *h0, *c0, *h1, *c1;   // h_*: [2][H] ping-pong by frame parity
    float *q, *ctx, *u1, *u2, *prev;
    // cumulative (location-sensitive) attention, flowtron.py:129-152, :793-806 -- all null when use_cumm_attention is off
    const float *cond_w1, *cond_b1, *cond_w2, *cond_b2, *w_key, *enc;
    const float *prior, *forced;                 // [N,L] attention prior (posterior, flowtron.py:544-557) / forced alignment (:585-588)
    float *cumm, *prev_attn, *keyin, *Kdyn;
    float *escore, *obuf;                        // attention scores [L], 1x1 conv output [2M] (stage hand-offs)
    int* ctl;                                    // [0] frame index, [1] done flag
    // bf16 images of the weight matrices (null = stream the fp32 originals)
    const bf16_t *att_w_ih16, *att_w_hh16, *w_query16, *l0_w_ih16, *l0_w_hh16, *l1_w_ih16, *l1_w_hh16, *d0_w16, *d1_w16, *conv_w16;
    int N, L, H, A, M, E;
    float inv_temp, gate_threshold;
};

// host: the weights, per-utterance operands, outputs and sizes of `a` (what ft_decode_flow and ft_decode_flow_batch both pass)
inline void fill_dev(const ft_decode_args* a, DecodeDev& h) {
    h.att_w_ih = a->att_w_ih; h.att_w_hh = a->att_w_hh; h.att_b_ih = a->att_b_ih; h.att_b_hh = a->att_b_hh;
    h.w_query = a->w_query; h.v = a->v; h.K = a->K; h.V = a->V;
    h.l0_w_ih = a->l0_w_ih; h.l0_w_hh = a->l0_w_hh; h.l0_b_ih = a->l0_b_ih; h.l0_b_hh = a->l0_b_hh;
    h.l1_w_ih = a->l1_w_ih; h.l1_w_hh = a->l1_w_hh; h.l1_b_ih = a->l1_b_ih; h.l1_b_hh = a->l1_b_hh;
    h.d0_w = a->d0_w; h.d0_b = a->d0_b; h.d1_w = a->d1_w; h.d1_b = a->d1_b; h.conv_w = a->conv_w; h.conv_b = a->conv_b;
    h.gate_w = a->gate_w; h.gate_b = a->gate_b;
    h.residual = a->residual; h.mel_out = a->mel_out; h.attn_out = a->attn_out; h.n_done_dev = a->n_done_dev;
    h.E = a->E;
    h.N = a->N; h.L = a->L; h.H = a->H; h.A = a->A; h.M = a->M;
}
// host: the bf16 image addresses (ftdec::make_wimg's img[], DecodeDev order)
inline void set_wimg(DecodeDev& h, const unsigned short* const* img) {
    h.att_w_ih16 = img[0]; h.att_w_hh16 = img[1]; h.w_query16 = img[2]; h.l0_w_ih16 = img[3]; h.l0_w_hh16 = img[4];
    h.l1_w_ih16 = img[5]; h.l1_w_hh16 = img[6]; h.d0_w16 = img[7]; h.d1_w16 = img[8]; h.conv_w16 = img[9];
}

// ---- bf16 weight images (bf16 operand mode): every weight matrix of the flow is rounded ONCE per ft_decode_flow call into a
// bf16 copy (53.7 MB instead of 107.4 MB per frame and flow; the copy stays in the Infinity Cache across frames) and the
// GEMVs stream those; activations and accumulation stay fp32.  16-byte loads = 8 weights per lane.
__device__ __forceinline__ float dot8(const uint4 w, const float4 xa, const float4 xb) {
    return __uint_as_float(w.x << 16) * xa.x + __uint_as_float(w.x & 0xffff0000u) * xa.y + __uint_as_float(w.y << 16) * xa.z +
           __uint_as_float(w.y & 0xffff0000u) * xa.w + __uint_as_float(w.z << 16) * xb.x + __uint_as_float(w.z & 0xffff0000u) * xb.y +
           __uint_as_float(w.w << 16) * xb.z + __uint_as_float(w.w & 0xffff0000u) * xb.w;
}
