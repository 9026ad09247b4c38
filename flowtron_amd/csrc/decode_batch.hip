// Autoregressive decode of one flow for a batch of utterances in ONE persistent launch (dec_persist_batch_k, ft_decode_flow_batch;
// ft_decode_flow_batch_keys: each utterance with its own text length).
// Its own translation unit: the kernel shares the hand-off protocol and the dot / cell / softmax helpers of dec_persist_k
// (decode_persist.h), and compiled into decode.hip's module it changed the register allocation of dec_persist_k<true> (module-level
// optimisation of the shared helpers); apart, both of decode.hip's persistent kernels keep their instruction streams.
#include "common.h"
#include <type_traits>

// decode.hip
namespace ftdec {
int make_wimg(const ft_decode_args* a, int n_layers, const unsigned short** img, hipStream_t st, bool round);
int device_cus();
long* prof_buf();
}  // namespace ftdec

namespace {

#include "decode_dev.h"
#include "decode_persist.h"

#include "decode_batch_k.h"

}  // namespace

extern "C" int ft_decode_batch_max(void) { return DEC_NBMAX; }
// the producers' copy + one copy per XCD, each nb times the single-utterance layout, + the census counters
extern "C" size_t ft_decode_batch_gran_bytes(int nb) { return nb < 1 ? 0 : (size_t)G_TOTAL * nb * 8 * 9 + 64; }

extern "C" int ft_decode_flow_batch_keys(const ft_decode_batch_args* ba, const int32_t* n_keys, void* stream) {
    FT_CHECK_ARG(ba != nullptr);
    const ft_decode_args* a = &ba->a;
    const int nb = ba->nb;
    FT_CHECK_ARG(nb >= 2 && nb <= DEC_NBMAX && ba->n_lim);
    FT_CHECK_ARG(a->att_w_ih && a->att_w_hh && a->att_b_ih && a->att_b_hh && a->w_query && a->v && a->K && a->V);
    FT_CHECK_ARG(a->l0_w_ih && a->l0_w_hh && a->l0_b_ih && a->l0_b_hh && a->l1_w_ih && a->l1_w_hh && a->l1_b_ih && a->l1_b_hh);
    FT_CHECK_ARG(a->d0_w && a->d0_b && a->d1_w && a->d1_b && a->conv_w && a->conv_b);
    FT_CHECK_ARG((a->gate_w == nullptr) == (a->gate_b == nullptr));
    FT_CHECK_ARG(a->residual && a->mel_out && a->attn_out && a->n_done_dev && a->persist_gran && a->persist_status);
    FT_CHECK_ARG(a->N >= 1 && a->L >= 1 && a->temperature > 0.f);
    const void* al16[] = {a->att_w_ih, a->att_w_hh, a->w_query, a->K, a->V, a->l0_w_ih, a->l0_w_hh, a->l1_w_ih, a->l1_w_hh,
                          a->d0_w, a->d1_w, a->conv_w, a->residual, a->mel_out, a->attn_out, a->persist_gran};
    for (const void* q : al16) FT_CHECK_ARG(reinterpret_cast<uintptr_t>(q) % 16 == 0);
    FT_CHECK_ARG(reinterpret_cast<uintptr_t>(n_keys) % 4 == 0);
    FT_CHECK_ARG(!a->wimg || (a->wimg_bytes >= ft_decode_wimg_bytes(a->H, a->A, a->M) && reinterpret_cast<uintptr_t>(a->wimg) % 256 == 0));
    const int n_layers = a->n_layers > 0 ? a->n_layers : 2;
    if (n_layers != 2 || a->cond_w1 || a->prior || a->forced || a->H != 1024 || a->A != 640 || a->M != 80 || a->L > 1024)
        return ft_fail(FT_EUNSUPPORTED, "ft_decode_flow_batch: only the persistent geometry (H 1024, A 640, M 80, L <= 1024, two decoder "
                                        "layers, plain attention, no prior or forced alignment)");
    if (ftdec::device_cus() < 256) return ft_fail(FT_EUNSUPPORTED, "ft_decode_flow_batch: needs a device with 256 CUs");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);

    DecodeDev h{};
    fill_dev(a, h);
    h.inv_temp = 1.0f / a->temperature; h.gate_threshold = a->gate_threshold;
    if (a->wimg) {                               // bf16 images, rounded unless an earlier call of this flow did (wimg_ready)
        const unsigned short* img[10];
        const int rc = ftdec::make_wimg(a, n_layers, img, st, ba->wimg_ready == 0);
        if (rc != FT_OK) return rc;
        set_wimg(h, img);
    }
    FT_CHECK_HIP(hipMemsetAsync(a->persist_gran, 0, ft_decode_batch_gran_bytes(nb), st));     // tags = 0 (epochs start at 1)
    FT_CHECK_HIP(hipMemsetAsync(a->n_done_dev, 0, sizeof(int) * nb, st));
    unsigned long long* gr = reinterpret_cast<unsigned long long*>(a->persist_gran);
    DecPB pb{DecP{h, gr, reinterpret_cast<unsigned*>(gr + (size_t)G_TOTAL * nb * 9), a->persist_status, 100000000L / 2, ftdec::prof_buf()},
             ba->n_lim, n_keys, nb};
    if (a->wimg) hipLaunchKernelGGL((dec_persist_batch_k<false, false>), dim3(256), dim3(256), 0, st, pb);
    else hipLaunchKernelGGL((dec_persist_batch_k<true, false>), dim3(256), dim3(256), 0, st, pb);
    FT_CHECK_LAUNCH();
    return FT_OK;
}

extern "C" int ft_decode_flow_batch(const ft_decode_batch_args* ba, void* stream) { return ft_decode_flow_batch_keys(ba, nullptr, stream); }
