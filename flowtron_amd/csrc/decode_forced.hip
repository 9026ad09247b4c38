// Autoregressive decode of one flow for a batch of utterances ALONG GIVEN ALIGNMENT ROWS in one persistent launch
// (dec_persist_batch_k<F32, true>, ft_decode_flow_batch_forced): the forced instantiations of the kernel in decode_batch_k.h.
// Its own translation unit for the reason decode_batch.hip has one: the free-running instantiations keep their instruction
// streams whatever is compiled here.
#include "common.h"
#include <type_traits>

namespace {

#include "decode_dev.h"
#include "decode_persist.h"
#include "decode_batch_k.h"

}  // namespace

#define DEC_BATCH_HOST
#include "decode_host.h"

extern "C" int ft_decode_flow_batch_forced(const ft_decode_batch_args* ba, const int32_t* n_keys, void* stream) {
    FT_CHECK_ARG(ba != nullptr);
    const ft_decode_args* a = &ba->a;
    const int nb = ba->nb;
    const int n_layers = a->n_layers > 0 ? a->n_layers : 2;
    // (before the pointer checks: a caller asks what the entry takes without a single device buffer)
    if (nb < 1 || nb > DEC_NBMAX || !a->forced || a->prior || n_layers != 2 || a->cond_w1 || a->H != 1024 || a->A != 640 || a->M != 80 ||
        a->L > 1024)
        return ft_fail(FT_EUNSUPPORTED, "ft_decode_flow_batch_forced: 1 .. %d utterances along forced alignment rows, only the persistent "
                                        "geometry (H 1024, A 640, M 80, L <= 1024, two decoder layers, plain attention, no prior)", DEC_NBMAX);
    // w_query and K are not read: the rows are given
    FT_CHECK_ARG(ba->n_lim && a->att_w_ih && a->att_w_hh && a->att_b_ih && a->att_b_hh && a->v && a->V);
    FT_CHECK_ARG(a->N >= 1 && a->L >= 1);
    if (const int rc = batch_check_args(__func__, a, n_keys, a->forced)) return rc;
    if (ftdec::device_cus() < 256) return ft_fail(FT_EUNSUPPORTED, "ft_decode_flow_batch_forced: needs a device with 256 CUs");
    return batch_launch<true>(__func__, ba, n_keys, stream);
}
