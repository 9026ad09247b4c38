// Host code the decode translation units share, included at file scope: by decode.hip for the ftdec:: declarations alone, by
// decode_batch.hip and decode_forced.hip (which define DEC_BATCH_HOST) behind their anonymous namespace with decode_dev.h,
// decode_persist.h and decode_batch_k.h, for the checks and the launch tail of the batched entries as well.
#pragma once

namespace ftdec {  // decode.hip
int make_wimg(const ft_decode_args* a, int n_layers, const unsigned short** img, hipStream_t st, bool round);
int device_cus();
long* prof_buf();
}  // namespace ftdec

#ifdef DEC_BATCH_HOST
namespace {
// FT_CHECK_ARG / FT_CHECK_HIP (common.h) with the public entry's name, `entry`, in place of __func__
#define DEC_CHECK_ARG(cond) if (!(cond)) return ft_fail(FT_EINVAL, "%s: invalid argument: %s", entry, #cond)
#define DEC_CHECK_HIP(expr) if (hipError_t e_ = (expr)) return ft_fail(FT_EHIP, "%s: %s: %s", entry, #expr, hipGetErrorString(e_))

// what ft_decode_flow_batch_keys and ft_decode_flow_batch_forced both ask of their arguments; rows16 = the per-utterance operand
// only one of them reads (K / the given rows), 16-byte aligned like the rest
inline int batch_check_args(const char* entry, const ft_decode_args* a, const int32_t* n_keys, const void* rows16) {
    DEC_CHECK_ARG(a->l0_w_ih && a->l0_w_hh && a->l0_b_ih && a->l0_b_hh && a->l1_w_ih && a->l1_w_hh && a->l1_b_ih && a->l1_b_hh);
    DEC_CHECK_ARG(a->d0_w && a->d0_b && a->d1_w && a->d1_b && a->conv_w && a->conv_b);
    DEC_CHECK_ARG((a->gate_w == nullptr) == (a->gate_b == nullptr));
    DEC_CHECK_ARG(a->residual && a->mel_out && a->attn_out && a->n_done_dev && a->persist_gran && a->persist_status);
    const void* al16[] = {a->att_w_ih, a->att_w_hh, a->w_query, rows16, a->V, a->l0_w_ih, a->l0_w_hh, a->l1_w_ih, a->l1_w_hh,
                          a->d0_w, a->d1_w, a->conv_w, a->residual, a->mel_out, a->attn_out, a->persist_gran};
    for (const void* q : al16) DEC_CHECK_ARG(reinterpret_cast<uintptr_t>(q) % 16 == 0);
    DEC_CHECK_ARG(reinterpret_cast<uintptr_t>(n_keys) % 4 == 0);
    DEC_CHECK_ARG(!a->wimg || (a->wimg_bytes >= ft_decode_wimg_bytes(a->H, a->A, a->M) && reinterpret_cast<uintptr_t>(a->wimg) % 256 == 0));
    return FT_OK;
}
// the launch of checked arguments (two decoder layers): parameter block, bf16 images, cleared granules and frame counts, one
// persistent launch -- FORCED: along a->forced, without scores, so the temperature has nothing to scale
template <bool FORCED>
int batch_launch(const char* entry, const ft_decode_batch_args* ba, const int32_t* n_keys, void* stream) {
    const ft_decode_args* a = &ba->a;
    const int nb = ba->nb;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    DecodeDev h{};
    fill_dev(a, h);
    if (FORCED) h.forced = a->forced;
    h.inv_temp = FORCED ? 1.0f : 1.0f / a->temperature; h.gate_threshold = a->gate_threshold;
    if (a->wimg) {                               // bf16 images, rounded unless an earlier call of this flow did (wimg_ready)
        const unsigned short* img[10];
        const int rc = ftdec::make_wimg(a, 2, img, st, ba->wimg_ready == 0);
        if (rc != FT_OK) return rc;
        set_wimg(h, img);
    }
    DEC_CHECK_HIP(hipMemsetAsync(a->persist_gran, 0, ft_decode_batch_gran_bytes(nb), st));     // tags = 0 (epochs start at 1)
    DEC_CHECK_HIP(hipMemsetAsync(a->n_done_dev, 0, sizeof(int) * nb, st));
    unsigned long long* gr = reinterpret_cast<unsigned long long*>(a->persist_gran);
    DecPB pb{DecP{h, gr, reinterpret_cast<unsigned*>(gr + (size_t)G_TOTAL * nb * 9), a->persist_status, 100000000L / 2, ftdec::prof_buf()},
             ba->n_lim, n_keys, nb};
    if (a->wimg) hipLaunchKernelGGL((dec_persist_batch_k<false, FORCED>), dim3(256), dim3(256), 0, st, pb);
    else hipLaunchKernelGGL((dec_persist_batch_k<true, FORCED>), dim3(256), dim3(256), 0, st, pb);
    if (hipError_t e_ = hipGetLastError()) return ft_fail(FT_EHIP, "%s: launch failed: %s", entry, hipGetErrorString(e_));
    return FT_OK;
}
#undef DEC_CHECK_ARG
#undef DEC_CHECK_HIP
}  // namespace
#endif  // DEC_BATCH_HOST
