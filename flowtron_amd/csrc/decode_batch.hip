// Autoregressive decode of one flow for a batch of utterances in ONE persistent launch (dec_persist_batch_k, ft_decode_flow_batch;
// ft_decode_flow_batch_keys: each utterance with its own text length).
// Its own translation unit: the kernel shares the hand-off protocol and the dot / cell / softmax helpers of dec_persist_k
// (decode_persist.h), and compiled into decode.hip's module it changed the register allocation of dec_persist_k<true> (module-level
// optimisation of the shared helpers); apart, both of decode.hip's persistent kernels keep their instruction streams.
#include "common.h"
#include <type_traits>

namespace {

#include "decode_dev.h"
#include "decode_persist.h"
#include "decode_batch_k.h"

}  // namespace

#define DEC_BATCH_HOST
#include "decode_host.h"

extern "C" int ft_decode_batch_max(void) { return DEC_NBMAX; }
// the producers' copy + one copy per XCD, each nb times the single-utterance layout, + the census counters
extern "C" size_t ft_decode_batch_gran_bytes(int nb) { return nb < 1 ? 0 : (size_t)G_TOTAL * nb * 8 * 9 + 64; }

extern "C" int ft_decode_flow_batch_keys(const ft_decode_batch_args* ba, const int32_t* n_keys, void* stream) {
    FT_CHECK_ARG(ba != nullptr);
    const ft_decode_args* a = &ba->a;
    const int nb = ba->nb;
    FT_CHECK_ARG(nb >= 2 && nb <= DEC_NBMAX && ba->n_lim);
    FT_CHECK_ARG(a->att_w_ih && a->att_w_hh && a->att_b_ih && a->att_b_hh && a->w_query && a->v && a->K && a->V);
    FT_CHECK_ARG(a->N >= 1 && a->L >= 1 && a->temperature > 0.f);
    if (const int rc = batch_check_args(__func__, a, n_keys, a->K)) return rc;
    const int n_layers = a->n_layers > 0 ? a->n_layers : 2;
    if (n_layers != 2 || a->cond_w1 || a->prior || a->forced || a->H != 1024 || a->A != 640 || a->M != 80 || a->L > 1024)
        return ft_fail(FT_EUNSUPPORTED, "ft_decode_flow_batch: only the persistent geometry (H 1024, A 640, M 80, L <= 1024, two decoder "
                                        "layers, plain attention, no prior or forced alignment)");
    if (ftdec::device_cus() < 256) return ft_fail(FT_EUNSUPPORTED, "ft_decode_flow_batch: needs a device with 256 CUs");
    return batch_launch<false>(__func__, ba, n_keys, stream);
}

extern "C" int ft_decode_flow_batch(const ft_decode_batch_args* ba, void* stream) { return ft_decode_flow_batch_keys(ba, nullptr, stream); }
